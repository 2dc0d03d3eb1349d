// Minibatch gather of the small per-sample fields in ONE launch (the reference indexes every field of the flattened buffer with
// the minibatch indices, /root/reference buffer.py:84-91 `samples_flat[key][mini_batch_indices]`: eight index kernels of ~5 us
// each per minibatch step here).  Fields are byte rows: dst[f][i, :] = src[f][idx[i], :], rows of row_bytes[f] (multiples of
// 4 bytes, contiguous).  Pure data movement: bit-exact.
#include "etm_common.h"
#include "adv_stats.h"

namespace {
constexpr int GR_MAXF = 16;
struct GatherP {
  const unsigned *src[GR_MAXF];
  unsigned *dst[GR_MAXF];
  int words[GR_MAXF];          // row length in 4-byte words
  const long long *idx;
  long long n, src_rows;
};
__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherP p) {
  const int f = blockIdx.y;
  const int words = p.words[f];
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.n * words) return;
  const long long i = e / words;
  const int w = (int)(e - i * words);
  long long r = p.idx[i];
  r = r < 0 ? 0 : (r >= p.src_rows ? p.src_rows - 1 : r);        // out-of-range indices are the caller's error; never fault
  p.dst[f][e] = p.src[f][r * words + w];
}
}  // namespace

// dst[f][i, :] = src[f][idx[i], :] for f < n_fields (<= 16), i < n; src[f] has src_rows rows of row_bytes[f] bytes (% 4 == 0).
extern "C" int etm_gather_rows(const void *const *src, void *const *dst, const int64_t *row_bytes, int n_fields, const int64_t *idx, int64_t n,
                               int64_t src_rows, void *stream) {
  (void)hipGetLastError();
  if (!src || !dst || !row_bytes || !idx || n_fields <= 0 || n <= 0 || src_rows <= 0) return ETM_EINVAL;
  if (n_fields > GR_MAXF) return ETM_EUNSUPPORTED;
  GatherP p{};
  long long most = 0;
  for (int f = 0; f < n_fields; ++f) {
    if (!src[f] || !dst[f] || row_bytes[f] <= 0) return ETM_EINVAL;
    if (row_bytes[f] % 4 != 0 || ((uintptr_t)src[f] % 4) != 0 || ((uintptr_t)dst[f] % 4) != 0 || row_bytes[f] / 4 > (1 << 20)) return ETM_EUNSUPPORTED;
    p.src[f] = static_cast<const unsigned *>(src[f]);
    p.dst[f] = static_cast<unsigned *>(dst[f]);
    p.words[f] = (int)(row_bytes[f] / 4);
    if (n * p.words[f] > most) most = n * p.words[f];
  }
  p.idx = (const long long *)idx; p.n = n; p.src_rows = src_rows;
  EtmProfScope prof(ETM_K_GATHER_ROWS, (hipStream_t)stream);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)n_fields), dim3(256), 0, (hipStream_t)stream, p);
  return etm_launch_status();
}

// ---- Head of the optimisation step as ONE launch: the jobs at the front of a minibatch step that depend only on the minibatch indices
// -- the field gather above, a copy of the indices themselves to the fixed-address vector the later kernels of the step read, and the
// advantage statistics of the loss -- each on a workgroup range of its own (first_block[], as the grouped reductions do), none
// reading what another writes.  The indices are row `*counter % table_rows` of a device-resident table that holds the minibatches
// of a whole epoch, so a replayed graph moves on to the next minibatch without a copy in front of it.
namespace {
constexpr int SH_THREADS = 1024;                   // the advantage job is adv_stats_kernel's workgroup: 16 waves, same merge order
struct StepHeadP {
  const unsigned *src[GR_MAXF];
  unsigned *dst[GR_MAXF];
  int words[GR_MAXF];
  int first_block[GR_MAXF + 3];                    // fields 0 .. n_fields - 1, the index copy, the advantage job, the end
  const long long *idx_table, *counter;
  long long *idx_out;
  const float *adv_src;
  float *stats3;
  long long n, src_rows;
  int n_fields, table_rows;
};
__global__ __launch_bounds__(SH_THREADS) void step_head_kernel(const StepHeadP p) {
  long long c = p.counter ? *p.counter : 0;
  c %= p.table_rows;
  if (c < 0) c += p.table_rows;                                    // (a counter nobody reset: any row, never outside the table)
  const long long *idx = p.idx_table + c * p.n;
  const int b = blockIdx.x, nj = p.n_fields + 2;
  int j = 0;
  for (int q = 1; q < nj; ++q)
    if (b >= p.first_block[q]) j = q;
  const long long e = (long long)(b - p.first_block[j]) * SH_THREADS + threadIdx.x;
  if (j < p.n_fields) {                                            // gather_rows_kernel's copy, element for element
    const int words = p.words[j];
    if (e >= p.n * words) return;
    const long long i = e / words;
    const int w = (int)(e - i * words);
    long long r = idx[i];
    r = r < 0 ? 0 : (r >= p.src_rows ? p.src_rows - 1 : r);
    p.dst[j][e] = p.src[j][r * words + w];
  } else if (j == p.n_fields) {
    if (e < p.n) p.idx_out[e] = idx[e];
  } else {                                                         // one workgroup: adv_stats_kernel over advantages read through idx
    const float *adv = p.adv_src;
    const long long rows = p.src_rows;
    adv_stats_block_1024((int)p.n, p.stats3, [&](int i) {
      long long r = idx[i];
      r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);                  // (the clamp of the gather: the value the gathered vector holds)
      return adv[r];
    });
  }
}
}  // namespace

// etm_gather_rows with idx = row (*counter % table_rows) of idx_table [table_rows, n] (counter NULL: row 0), plus, in the same launch:
// idx_out (may be NULL) [n] = that row; stats3 (may be NULL) = etm_adv_stats of adv_src[idx] (adv_src: src_rows floats), bit for bit.
extern "C" int etm_step_head(const void *const *src, void *const *dst, const int64_t *row_bytes, int n_fields, const int64_t *idx_table,
                             int table_rows, const int64_t *counter, int64_t n, int64_t src_rows, int64_t *idx_out, const float *adv_src,
                             float *stats3, void *stream) {
  (void)hipGetLastError();
  if (!idx_table || table_rows <= 0 || n_fields < 0 || n <= 0 || src_rows <= 0 || (n_fields > 0 && (!src || !dst || !row_bytes))) return ETM_EINVAL;
  if ((stats3 != nullptr) != (adv_src != nullptr)) return ETM_EINVAL;
  if (n_fields > GR_MAXF || (stats3 && n >= ETM_ADV_STATS_SPLIT_MIN)) return ETM_EUNSUPPORTED;      // (large N: etm_adv_stats_ws is another sum)
  StepHeadP p{};
  long long blocks = 0;
  for (int f = 0; f < n_fields; ++f) {
    if (!src[f] || !dst[f] || row_bytes[f] <= 0) return ETM_EINVAL;
    if (row_bytes[f] % 4 != 0 || ((uintptr_t)src[f] % 4) != 0 || ((uintptr_t)dst[f] % 4) != 0 || row_bytes[f] / 4 > (1 << 20)) return ETM_EUNSUPPORTED;
    p.src[f] = static_cast<const unsigned *>(src[f]);
    p.dst[f] = static_cast<unsigned *>(dst[f]);
    p.words[f] = (int)(row_bytes[f] / 4);
    p.first_block[f] = (int)blocks;
    blocks += (n * p.words[f] + SH_THREADS - 1) / SH_THREADS;
  }
  p.first_block[n_fields] = (int)blocks;
  if (idx_out) blocks += (n + SH_THREADS - 1) / SH_THREADS;
  p.first_block[n_fields + 1] = (int)blocks;
  if (stats3) blocks += 1;
  p.first_block[n_fields + 2] = (int)blocks;
  if (blocks <= 0 || blocks > 0x7fffffffLL) return ETM_EINVAL;
  p.idx_table = (const long long *)idx_table; p.counter = (const long long *)counter; p.idx_out = (long long *)idx_out;
  p.adv_src = adv_src; p.stats3 = stats3; p.n = n; p.src_rows = src_rows; p.n_fields = n_fields; p.table_rows = table_rows;
  EtmProfScope prof(ETM_K_GATHER_ROWS, (hipStream_t)stream);
  hipLaunchKernelGGL(step_head_kernel, dim3((unsigned)blocks), dim3(SH_THREADS), 0, (hipStream_t)stream, p);
  return etm_launch_status();
}
