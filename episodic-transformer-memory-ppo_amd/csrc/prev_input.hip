// previous_step_input: the previous step's action(s) and raw reward as one more addend of lin_hidden's pre-activation.
// A learned table T [R, D]: branch b owns rows off_b .. off_b + A_b - 1 (the flat layout of the action masks), the reward row, when
// there is one, is row R - 1.  utils.previous_step_rows / previous_step_table_grad are the host definitions.
//   etm_prev_input_rows: e_n = sum_b T[off_b + a_nb, :] + r_n T[R - 1, :] (+ bias), started at +0, the branches in ascending b, the
//                        reward term last, every product and sum rounded on its own (no contraction: __fadd_rn / __fmul_rn under
//                        this build's -ffp-contract=on); a sample without a previous step is +0 (+ bias).  Bit for bit the host rule.
//   etm_prev_input_grad: dT[k, :] = sum_n c_nk gm[n, :] without float atomics in a fixed order: a workgroup owns a chunk of PI_CHUNK
//                        samples and a tile of PI_TILE columns, a thread owns one column and walks the chunk's samples in ascending
//                        order into its own column of an [R, PI_TILE] accumulator in LDS (no thread reads another's column: no
//                        barrier); the chunks' partial tables are then added in chunk order by a second small launch (or by
//                        etm_colsum_reduce_grouped: they are P = chunks rows of C = R D partial sums).  Both walks are compensated
//                        sums (two-sum; the reward product's rounding error is kept too): a serial float32 chain over a chunk
//                        alone is several times less accurate than a library one-hot product, the compensated one is not.
#include "etm_common.h"

namespace {
constexpr int PI_MAXR = 64;            // rows of the table (the step kernel's RF_MAXSPLIT bounds the slices, the LDS tile the rows)
constexpr int PI_TILE = 64;            // columns of a workgroup (one wave) of the gradient kernel: 2 x [64, 64] floats = 32 KB of static LDS
constexpr int PI_CHUNK = 64;           // samples of a workgroup of the gradient kernel
constexpr int PI_ROWS_THREADS = 256;

struct PrevIdx {
  const long long *actions;            // [N, >= B] (row stride act_ld); NULL with B == 0
  const float *rewards;                // [N] or NULL: no reward term
  const long long *ep_step;            // [N] or NULL.  Non-NULL (rollout form): a previous step exists where the word is not 0;
                                       // NULL (training form): where actions[n, 0] >= 0 (always, with B == 0)
  long long act_ld;
  int B, R;
  int size[ETM_MAX_BRANCHES];
};

// (an action outside its branch is the caller's error; clamped so that it never reads or writes outside the branch's rows)
__device__ __forceinline__ int pi_row(long long a, int off, int size) {
  return off + (int)(a < 0 ? 0 : (a >= size ? size - 1 : a));
}
__device__ __forceinline__ bool pi_has_prev(const PrevIdx &p, long long n) {
  if (p.ep_step) return p.ep_step[n] != 0;
  return p.B == 0 || p.actions[n * p.act_ld] >= 0;
}

__global__ __launch_bounds__(PI_ROWS_THREADS) void prev_input_rows_kernel(const PrevIdx p, const float *__restrict__ table,
                                                                          const float *__restrict__ bias, float *__restrict__ out,
                                                                          long long out_ld, long long N, int D) {
  const long long e = (long long)blockIdx.x * PI_ROWS_THREADS + threadIdx.x;
  if (e >= N * D) return;
  const long long n = e / D;
  const int c = (int)(e - n * D);
  float acc = 0.f;
  if (pi_has_prev(p, n)) {
    int off = 0;
    for (int b = 0; b < p.B; ++b) {
      acc = __fadd_rn(acc, table[(long long)pi_row(p.actions[n * p.act_ld + b], off, p.size[b]) * D + c]);
      off += p.size[b];
    }
    if (p.rewards) acc = __fadd_rn(acc, __fmul_rn(p.rewards[n], table[(long long)(p.R - 1) * D + c]));
  }
  if (bias) acc = __fadd_rn(acc, bias[c]);
  out[n * out_ld + c] = acc;
}

// s + x exactly as (sum, error) -- Knuth's two-sum, six operations, no assumption on the magnitudes; the error goes to a running
// compensation that is added once at the end.  (The intrinsics keep each operation as written.)
__device__ __forceinline__ void pi_two_sum(float &s, float &comp, float x) {
  const float t = __fadd_rn(s, x);
  const float bp = __fsub_rn(t, s);
  comp = __fadd_rn(comp, __fadd_rn(__fsub_rn(s, __fsub_rn(t, bp)), __fsub_rn(x, bp)));
  s = t;
}

__global__ __launch_bounds__(PI_TILE) void prev_input_grad_kernel(const PrevIdx p, const float *__restrict__ gm, long long gm_ld,
                                                                  float *__restrict__ part, long long N, int D) {
  __shared__ float acc[2][PI_MAXR][PI_TILE];                 // [0]: the running sums, [1]: their compensations
  const int t = threadIdx.x;
  const int c = blockIdx.x * PI_TILE + t;
  if (c >= D) return;                                        // (no barrier below: a thread only touches its own column)
  const int R = p.R;
  for (int r = 0; r < R; ++r) acc[0][r][t] = acc[1][r][t] = 0.f;
  const long long n0 = (long long)blockIdx.y * PI_CHUNK;
  const long long n1 = n0 + PI_CHUNK < N ? n0 + PI_CHUNK : N;
  for (long long n = n0; n < n1; ++n) {
    if (!pi_has_prev(p, n)) continue;
    const float g = gm[n * gm_ld + c];
    int off = 0;
    for (int b = 0; b < p.B; ++b) {
      const int r = pi_row(p.actions[n * p.act_ld + b], off, p.size[b]);
      float s = acc[0][r][t], k = acc[1][r][t];
      pi_two_sum(s, k, g);
      acc[0][r][t] = s;
      acc[1][r][t] = k;
      off += p.size[b];
    }
    if (p.rewards) {
      const float rw = p.rewards[n];
      const float pr = __fmul_rn(rw, g);
      float s = acc[0][R - 1][t], k = acc[1][R - 1][t];
      pi_two_sum(s, k, pr);
      k = __fadd_rn(k, __builtin_fmaf(rw, g, -pr));          // the product's own rounding error (exact)
      acc[0][R - 1][t] = s;
      acc[1][R - 1][t] = k;
    }
  }
  float *dst = part + (long long)blockIdx.y * R * D + c;
  for (int r = 0; r < R; ++r) dst[(long long)r * D] = __fadd_rn(acc[0][r][t], acc[1][r][t]);
}

// d_table[i] = part[0][i] + part[1][i] + ... in chunk order (compensated as above), i < R * D
__global__ __launch_bounds__(256) void prev_input_grad_reduce_kernel(const float *__restrict__ part, float *__restrict__ d_table, int chunks,
                                                                     long long RD) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= RD) return;
  float s = part[i], k = 0.f;
  for (int j = 1; j < chunks; ++j) pi_two_sum(s, k, part[(long long)j * RD + i]);
  d_table[i] = __fadd_rn(s, k);
}

constexpr int PI_MAXD = 1 << 16;
constexpr long long PI_MAXN = 1ll << 22;       // (the chunks are the gradient kernel's grid.y: at most 65535 of them)

inline bool pi_al(const void *ptr, unsigned a) { return ((uintptr_t)ptr & (a - 1)) == 0; }

// the index half of both entries: 0, or the code to return
int pi_make(PrevIdx *p, const int64_t *actions, int64_t act_stride, const int32_t *sizes, int n_branches, const float *rewards,
            const int64_t *ep_step, int R) {
  if (R < 1 || R > PI_MAXR || n_branches < 0 || n_branches > ETM_MAX_BRANCHES) return ETM_EINVAL;
  if (n_branches == 0 && !rewards) return ETM_EINVAL;                 // nothing to feed back
  if (n_branches > 0 && (!actions || !sizes || act_stride < n_branches)) return ETM_EINVAL;
  if (!pi_al(actions, 8) || !pi_al(ep_step, 8) || !pi_al(rewards, 4)) return ETM_EINVAL;
  int total = 0;
  for (int b = 0; b < n_branches; ++b) {
    if (sizes[b] <= 0 || sizes[b] > PI_MAXR) return ETM_EINVAL;
    p->size[b] = sizes[b];
    total += sizes[b];
  }
  if (total + (rewards ? 1 : 0) > R) return ETM_EINVAL;
  p->actions = n_branches ? (const long long *)actions : nullptr;
  p->rewards = rewards;
  p->ep_step = (const long long *)ep_step;
  p->act_ld = act_stride;
  p->B = n_branches;
  p->R = R;
  return 0;
}
}  // namespace

extern "C" int etm_prev_input_supported(int R, int D) { return R >= 1 && R <= PI_MAXR && D >= 1 && D <= PI_MAXD ? 1 : 0; }

extern "C" int etm_prev_input_rows(const float *table, int R, int D, const int64_t *actions, int64_t act_stride, const int32_t *sizes,
                                   int n_branches, const float *rewards, const int64_t *ep_step, const float *bias, float *out,
                                   int64_t out_stride, int64_t N, void *stream) {
  (void)hipGetLastError();
  if (!table || !out || N <= 0 || N > PI_MAXN || D < 1 || D > PI_MAXD || out_stride < D) return ETM_EINVAL;
  if (!pi_al(table, 4) || !pi_al(out, 4) || !pi_al(bias, 4)) return ETM_EINVAL;
  PrevIdx p{};
  if (int rc = pi_make(&p, actions, act_stride, sizes, n_branches, rewards, ep_step, R)) return rc;
  const long long blocks = (N * D + PI_ROWS_THREADS - 1) / PI_ROWS_THREADS;
  if (blocks > 0x7fffffffLL) return ETM_EINVAL;
  EtmProfScope prof(ETM_K_GATHER_ROWS, (hipStream_t)stream);
  hipLaunchKernelGGL(prev_input_rows_kernel, dim3((unsigned)blocks), dim3(PI_ROWS_THREADS), 0, (hipStream_t)stream, p, table, bias, out,
                     (long long)out_stride, (long long)N, D);
  return etm_launch_status();
}

extern "C" int etm_prev_input_grad_chunk(void) { return PI_CHUNK; }
// rows of R * D partial sums the gradient kernel leaves in its workspace (0: bad N)
extern "C" int etm_prev_input_grad_partial_rows(int64_t N) { return N <= 0 || N > PI_MAXN ? 0 : (int)((N + PI_CHUNK - 1) / PI_CHUNK); }
extern "C" int64_t etm_prev_input_grad_workspace_bytes(int64_t N, int R, int D) {
  if (!etm_prev_input_supported(R, D) || N <= 0 || N > PI_MAXN) return 0;
  return (int64_t)etm_prev_input_grad_partial_rows(N) * R * D * (int64_t)sizeof(float);
}

extern "C" int etm_prev_input_grad(const float *gm, int64_t gm_stride, const int64_t *actions, int64_t act_stride, const int32_t *sizes,
                                   int n_branches, const float *rewards, float *d_table, int R, int D, int64_t N, float *workspace,
                                   int64_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (!gm || !workspace || N <= 0 || N > PI_MAXN || D < 1 || D > PI_MAXD || gm_stride < D) return ETM_EINVAL;
  if (!pi_al(gm, 4) || !pi_al(d_table, 4) || !pi_al(workspace, 4)) return ETM_EINVAL;
  PrevIdx p{};
  if (int rc = pi_make(&p, actions, act_stride, sizes, n_branches, rewards, nullptr, R)) return rc;
  if (workspace_bytes < etm_prev_input_grad_workspace_bytes(N, R, D)) return ETM_EWORKSPACE;
  const int chunks = etm_prev_input_grad_partial_rows(N);
  if (chunks > 65535) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_COLSUM, st);
  // one chunk: its partial table IS the result (the same bits the reduction would copy)
  float *part = (chunks == 1 && d_table) ? d_table : workspace;
  hipLaunchKernelGGL(prev_input_grad_kernel, dim3((unsigned)((D + PI_TILE - 1) / PI_TILE), (unsigned)chunks), dim3(PI_TILE), 0, st, p, gm,
                     (long long)gm_stride, part, (long long)N, D);
  int rc = etm_launch_status();
  if (rc || !d_table || chunks == 1) return rc;
  const long long RD = (long long)R * D;
  hipLaunchKernelGGL(prev_input_grad_reduce_kernel, dim3((unsigned)((RD + 255) / 256)), dim3(256), 0, st, workspace, d_table, chunks, RD);
  return etm_launch_status();
}
