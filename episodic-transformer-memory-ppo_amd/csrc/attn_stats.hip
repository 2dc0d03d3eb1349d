// Attention statistics (include/etm_hip.h, "attention statistics"; added with the ABI left at 61): where in the memory window the
// attention probabilities att [N, H, L] of a training pass land, per head, as sums a host turns into means and histograms.
//
// A row is (sample n, head h); v = the number of set bytes of mask[n].  A row counts when the mask is a prefix (bytes 0 .. v - 1 set,
// no others) and v >= 1; v = 0 is an empty row, any other mask an irregular one -- both are counted as such and add nothing else.
// The age of window entry l is v - l (the newest stored step has age 1).  Per head 264 doubles (ETM_ATTN_STATS_WORDS):
//   0 counted rows   1 counted rows with v >= 2   2 empty rows   3 irregular rows
//   4 sum of the entropy -sum_l p ln p (valid entries with p > 0, nats)   5 sum over rows with v >= 2 of entropy / ln v
//   6 sum of max_l p over valid entries   7 reserved (0 is added)
//   8 .. 135 age[a - 1] = sum of p at age a   136 .. 263 index[l] = sum of p at entry l      (words beyond L: 0 is added)
//
// Two launches, a launch boundary between them, no atomics:
//   1. attn_stats_partial_kernel, grid (chunks, H), chunks = ceil(N / 64), 512 threads = 8 waves.  Workgroup (c, h) owns samples
//      64 c .. 64 c + 63 of head h; its wave w walks samples 64 c + 8 w .. + 7 (those below N) in order, one row at a time: lane j
//      holds entries j and j + 64, v and the prefix test come from the two 64-bit ballots of the mask bytes, the entropy terms
//      p logf(p) are summed and the maximum taken across the wave in fp32, the age histogram reads p at entry v - a from the lane
//      that holds it (one cross-lane read per half), the index histogram is the lane's own p; entropy / ln v is a product with a
//      double 1 / ln v from a table in LDS.  A window of at most 64 entries skips the second half's arithmetic (a uniform branch).
//      What crosses rows is double, in registers: lane j keeps age words j, j + 64 and index words j, j + 64, every lane the seven
//      scalars.  The 8 waves then add their words into one LDS image IN WAVE ORDER, and the workgroup writes it as its partial.
//      (8 waves of 8 rows: the row arithmetic, not the memory, bounds the pass -- 16 waves of 16 rows left three CUs in four idle at a
//      minibatch of 2048 and measured 20.9 us per call against 12.0 - 12.7; fewer rows per partial make the second launch longer.)
//   2. attn_stats_finish_kernel, one thread per (head, word): the chunks' partials added in chunk order (eight loads in flight), the
//      total added to table.
// Workspace: double [chunks][H][264], partial (c, h) at word (c H + h) 264 -- a pure function of (N, H, L); every word of it is
// written before it is read, so it needs no clearing.  The order of every floating-point sum is fixed by these constants, never by the
// grid's scheduling: two calls on equal inputs give equal bits.  Nothing is booked in the per-kernel profile.
#include "etm_common.h"

namespace {
constexpr int AS_WORDS = 264;      // doubles per head
constexpr int AS_AGE = 8;          // first word of the age histogram
constexpr int AS_INDEX = 136;      // first word of the index histogram
constexpr int AS_MAX_L = 128;
constexpr int AS_MAX_H = 32;
constexpr int AS_WAVES = 8;        // waves per workgroup
constexpr int AS_ROWS = 8;         // samples per wave
constexpr int AS_CHUNK = AS_WAVES * AS_ROWS;

struct AsRow {
  float p0, p1;
  unsigned char m0, m1;
};

__device__ __forceinline__ AsRow as_load(const float *__restrict__ att, const uint8_t *__restrict__ mask, int n, int h, int H, int L,
                                         int lane) {
  AsRow r{0.f, 0.f, 0, 0};
  const float *a = att + ((long long)n * H + h) * L;
  const uint8_t *m = mask + (long long)n * L;
  if (lane < L) {
    r.p0 = a[lane];
    r.m0 = m[lane];
  }
  if (lane + 64 < L) {
    r.p1 = a[lane + 64];
    r.m1 = m[lane + 64];
  }
  return r;
}

__global__ __launch_bounds__(AS_WAVES * 64) void attn_stats_partial_kernel(const float *__restrict__ att, const uint8_t *__restrict__ mask,
                                                                           double *__restrict__ ws, int N, int H, int L) {
  __shared__ double rln_s[AS_MAX_L + 1];      // 1 / ln v, v = 2 .. 128
  __shared__ double acc_s[AS_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.y;
  for (int v = 2 + tid; v <= AS_MAX_L; v += AS_WAVES * 64) rln_s[v] = 1.0 / log((double)v);
  __syncthreads();
  const int n0 = blockIdx.x * AS_CHUNK + wave * AS_ROWS;
  const int n1 = min(N, n0 + AS_ROWS);
  const bool two_halves = L > 64;      // (uniform) a window of at most 64 entries leaves the second half of every lane empty
  double age0 = 0.0, age1 = 0.0, idx0 = 0.0, idx1 = 0.0, s_ent = 0.0, s_nent = 0.0, s_max = 0.0;
  int c_rows = 0, c_rows2 = 0, c_empty = 0, c_irr = 0;
  AsRow nxt{0.f, 0.f, 0, 0};
  if (n0 < n1) nxt = as_load(att, mask, n0, h, H, L, lane);
  for (int n = n0; n < n1; ++n) {
    const AsRow r = nxt;
    if (n + 1 < n1) nxt = as_load(att, mask, n + 1, h, H, L, lane);      // in flight under this row's arithmetic
    const unsigned long long b0 = __builtin_amdgcn_ballot_w64(r.m0 != 0), b1 = __builtin_amdgcn_ballot_w64(r.m1 != 0);
    const int v = __popcll(b0) + __popcll(b1);
    const unsigned long long want0 = v >= 64 ? ~0ull : (1ull << v) - 1ull;
    const unsigned long long want1 = v >= 128 ? ~0ull : (v > 64 ? (1ull << (v - 64)) - 1ull : 0ull);
    if (b0 != want0 || b1 != want1) {      // (wave-uniform: the ballots are)
      ++c_irr;
      continue;
    }
    if (v == 0) {
      ++c_empty;
      continue;
    }
    const float q0 = lane < v ? r.p0 : 0.f, q1 = lane + 64 < v ? r.p1 : 0.f;
    const float t0 = q0 > 0.f ? q0 * logf(q0) : 0.f;      // 0 ln 0 adds 0
    float t1 = 0.f;
    if (two_halves) t1 = q1 > 0.f ? q1 * logf(q1) : 0.f;
    const float ent = -wave_sum(t0 + t1);
    const float mx = wave_max(fmaxf(q0, q1));
    // age a = k + 1 of histogram word k is entry l = v - 1 - k: words lane and lane + 64 both read lane (v - 1 - lane) mod 64
    const int l = v - 1 - lane, src = l & 63;
    const float g0 = __shfl(q0, src, 64), g1 = two_halves ? __shfl(q1, src, 64) : 0.f;
    const float a0 = l < 0 ? 0.f : (l < 64 ? g0 : g1);
    const float a1 = l >= 64 ? g0 : 0.f;      // entry l - 64, below 64 because v <= 128
    ++c_rows;
    s_ent += (double)ent;
    s_max += (double)mx;
    if (v >= 2) {
      ++c_rows2;
      s_nent += (double)ent * rln_s[v];
    }
    age0 += (double)a0;
    idx0 += (double)q0;
    if (two_halves) {
      age1 += (double)a1;
      idx1 += (double)q1;
    }
  }
  double sc = 0.0;      // scalar word `lane` (lanes 0 .. 7)
  sc = lane == 0 ? (double)c_rows : sc;
  sc = lane == 1 ? (double)c_rows2 : sc;
  sc = lane == 2 ? (double)c_empty : sc;
  sc = lane == 3 ? (double)c_irr : sc;
  sc = lane == 4 ? s_ent : sc;
  sc = lane == 5 ? s_nent : sc;
  sc = lane == 6 ? s_max : sc;
  for (int w = 0; w < AS_WAVES; ++w) {       // wave order: the sum's order is fixed
    if (wave == w) {
      if (w == 0) {
        if (lane < AS_AGE) acc_s[lane] = sc;
        acc_s[AS_AGE + lane] = age0;
        acc_s[AS_AGE + 64 + lane] = age1;
        acc_s[AS_INDEX + lane] = idx0;
        acc_s[AS_INDEX + 64 + lane] = idx1;
      } else {
        if (lane < AS_AGE) acc_s[lane] += sc;
        acc_s[AS_AGE + lane] += age0;
        acc_s[AS_AGE + 64 + lane] += age1;
        acc_s[AS_INDEX + lane] += idx0;
        acc_s[AS_INDEX + 64 + lane] += idx1;
      }
    }
    __syncthreads();
  }
  for (int w = tid; w < AS_WORDS; w += AS_WAVES * 64) ws[((long long)blockIdx.x * H + h) * AS_WORDS + w] = acc_s[w];
}

__global__ __launch_bounds__(256) void attn_stats_finish_kernel(const double *__restrict__ ws, double *__restrict__ table, int chunks,
                                                                int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * AS_WORDS) return;
  const long long stride = (long long)H * AS_WORDS;
  double s = 0.0;
  int c = 0;
  for (; c + 8 <= chunks; c += 8) {      // eight loads in flight, added in chunk order
    double t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = ws[(c + k) * stride + i];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += t[k];
  }
  for (; c < chunks; ++c) s += ws[c * stride + i];
  table[i] += s;
}

bool as_shape_ok(int N, int H, int L) { return N >= 1 && H >= 1 && H <= AS_MAX_H && L >= 1 && L <= AS_MAX_L; }
}  // namespace

extern "C" int64_t etm_attn_stats_workspace_bytes(int N, int H, int L) {
  if (!as_shape_ok(N, H, L)) return 0;
  return (int64_t)((N + AS_CHUNK - 1) / AS_CHUNK) * H * AS_WORDS * (int64_t)sizeof(double);
}

extern "C" int etm_attn_stats(const float *att, const uint8_t *mask, double *table, void *workspace, int64_t workspace_bytes, int N, int H,
                              int L, void *stream) {
  (void)hipGetLastError();
  if (!att || !mask || !table || !workspace || !as_shape_ok(N, H, L)) return ETM_EINVAL;
  if ((uintptr_t)table % 8 || (uintptr_t)workspace % 8) return ETM_EINVAL;
  if (workspace_bytes < etm_attn_stats_workspace_bytes(N, H, L)) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (N + AS_CHUNK - 1) / AS_CHUNK;
  hipLaunchKernelGGL(attn_stats_partial_kernel, dim3((unsigned)chunks, (unsigned)H), dim3(AS_WAVES * 64), 0, st, att, mask,
                     (double *)workspace, N, H, L);
  hipLaunchKernelGGL(attn_stats_finish_kernel, dim3((unsigned)((H * AS_WORDS + 255) / 256)), dim3(256), 0, st, (const double *)workspace,
                     table, chunks, H);
  return etm_launch_status();
}
