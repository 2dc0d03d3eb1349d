// Rollout step of one worker GROUP for the gated (GTrXL) block layouts -- weights read once per group and step (round 5;
// /root/reference trainer.py:163-186 -> model.py:96-112 -> transformer.py:222-253, :117-172, :287-298).
//
// csrc/rollout_fused.hip gives every WORKER a team of P workgroups that walks the worker's chain as matrix-VECTOR products: every team
// streams every matrix once per step.  For the post-LN layout without gates (3 products per block) that is the right trade; a gated
// block has 15 D x D maps (q, fc_out, fc and 2 x 6 gate maps), 8.85 MB per worker team and step at D = 384 / 4 blocks, and the step
// kernel of BASELINE configs 2 / 5 spent half of its ~280 us streaming them.
//
// Here the G <= 8 workers of a group are the ROWS of every product and its COLUMNS are dealt to RG_WG = 32 workgroups: workgroup j owns
// columns [j CB, (j + 1) CB) (CB = D / 32: 12 at D = 384) of every D x D map -- an 18 KB slice per map, 1.1 MB per step and workgroup
// instead of 8.85 MB, and the 8.85 MB leave L2 / the Infinity Cache ONCE per group and step instead of once per worker.
//   * a product: the slice is requested one or two phases ahead into registers in MFMA B-fragment order; the activations [8, D] sit
//     in LDS (A fragments); wave w contracts k in [w D / 8, (w + 1) D / 8) with D / 32 `v_mfma_f32_16x16x4_f32` (rows 8 .. 15 of the
//     tile mirror rows 0 .. 7), the eight partial tiles are summed through LDS in wave order;
//   * every product ends in an exchange, because the next product needs the full [8, D] activations in every workgroup: a workgroup
//     publishes its [8, CB] piece as tagged 16-byte packets (the exchange format of rollout_fused.hip) and reads all 32 pieces --
//     1,536 packets, three per thread, requested together;
//   * the attention of (worker g, head h) is the job of workgroup u = g H + h (G H <= 32): it alone reads that unit's K | V cache
//     columns, receives the unit's query columns (a scatter: 48 packets) and publishes the unit's context columns; it also owns the
//     unit's cache columns in the tail (reset at episode step 0, projection of the new items), so that -- as in rollout_fused.hip --
//     no cache byte is written by one workgroup and read by another within a launch, and the bank / staging / window rows of worker
//     g are written by workgroup (g, 0);
//   * workgroup 0 samples all workers of the group and hands the actions over.
// Per gated block: 8 product phases and 7 exchanges (q scatter, ctx, r.x, h1, f, r.x, out) where the per-worker form has 15 products
// and 6 exchanges -- the products are now small (latency of one L2 round trip, requested ahead), the exchanges are what is left.
// fc_out is folded into the first gate's maps of y (W (Wo ctx + bo) = (W Wo) ctx + W bo; the caller folds in float64 once per update):
// apart from that association only summation order differs from the other rollout paths.
//
// Matrix layouts the caller packs for THIS kernel (etm_rollout_trxl_group; etm/model.py keeps them next to the per-worker ones):
// every [in = D, out] map transposed and column-blocked [32][D][CB]; gate maps of y as [32][3][D][CB] (Wr, Wz, Wg; the FIRST gate's folded
// with fc_out -- (Wo^T W^T) column-blocked -- and followed by the three bias rows [3][D] = W bo; wo_t / bo are not read), of x as
// [32][2][D][CB] (Ur, Uz); hidden heads [32][NCH][D][CH] with NCH * CH = 2 hid / 32 (CH <= 16); wkv per block and HEAD [nb][H][D][2 hd]
// = [the head's K columns | the head's V columns] (what the per-worker kernel calls member-blocked, with P = H).
#include "rollout_shared.h"

namespace {
constexpr int RG_WG = 32;                  // workgroups of one launch (all resident: they wait for each other)
constexpr int RG_G = 8;                    // worker rows of the activations (MFMA tile rows 8 .. 15 mirror rows 0 .. 7)
constexpr int RG_PIECE = 128;              // payload floats per exchange piece (8 CB <= 128, hd <= 128, 8 (A + 1) <= 128)
constexpr int RG_PART = 8 * 3 * 8 * 16;    // partial tiles [wave][chunk][row][16] of one product phase

struct Grp {
  float *slots;          // exchange slots [n_ex][RG_WG][2 RG_PIECE]
  long long *err;
  int *dead_s;           // LDS flag of this workgroup: a collect of this launch timed out -- the following ones do not wait again
  int base, me;
};
__device__ __forceinline__ float *rg_piece(const Grp &t, int ex, int wg) { return t.slots + ((long long)ex * RG_WG + wg) * (2 * RG_PIECE); }

// Publish: thread t < n holds payload float t (n even) of my piece of exchange ex; even threads take their neighbour's value by a lane shift and
// store the packet -- no staging in LDS, no barrier between the epilogue and the publish.  Call from all threads.
__device__ __forceinline__ void rg_publish_reg(const Grp &t, int ex, float v, int n) {
  const float nxt = __shfl_down(v, 1, 64);
  const int tid = threadIdx.x;
  if (tid < n && !(tid & 1)) packet_store(rg_piece(t, ex, t.me) + 2 * tid, __int_as_float(t.base + ex + 1), v, nxt);
}

// NP packets per thread requested TOGETHER (one round trip per polling pass, not NP)
template <int NP>
__device__ __forceinline__ void rg_load(f32x4 (&v)[NP], const float *const (&ptr)[NP]) {
  static_assert(NP >= 1 && NP <= 4, "1 .. 4 packets per thread");
  if constexpr (NP == 1)
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v[0]) : "v"(ptr[0]) : "memory");
  else if constexpr (NP == 2)
    asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %3, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"(ptr[0]), "v"(ptr[1]) : "memory");
  else if constexpr (NP == 3)
    asm volatile("global_load_dwordx4 %0, %3, off sc0 sc1\n\tglobal_load_dwordx4 %1, %4, off sc0 sc1\n\tglobal_load_dwordx4 %2, %5, off sc0 sc1\n\t"
                 "s_waitcnt vmcnt(0)" : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]) : "v"(ptr[0]), "v"(ptr[1]), "v"(ptr[2]) : "memory");
  else
    asm volatile("global_load_dwordx4 %0, %4, off sc0 sc1\n\tglobal_load_dwordx4 %1, %5, off sc0 sc1\n\tglobal_load_dwordx4 %2, %6, off sc0 sc1\n\t"
                 "global_load_dwordx4 %3, %7, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(ptr[0]), "v"(ptr[1]), "v"(ptr[2]), "v"(ptr[3]) : "memory");
}
// Collect `total` packets of exchange ex: packet pk is read at src(pk) and its two payload floats go to dst(pk)[0], dst(pk)[1] (LDS).
// Thread t takes packets t, t + 512, ...; bounded polling (a partner that never shows up sets the error word).  The caller barriers.
template <int NP, class SrcF, class DstF>
__device__ __forceinline__ void rg_collect(const Grp &t, int ex, int total, SrcF src, DstF dst) {
  const int want = t.base + ex + 1;
  const float *ptr[NP];
  float *out[NP];
  bool need[NP];
  const float *own = rg_piece(t, 0, t.me);        // any mapped address for the unused requests of this thread
  bool any = false;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int pk = (int)threadIdx.x + RF_T * i;
    need[i] = pk < total;
    ptr[i] = need[i] ? src(pk) : own;
    out[i] = need[i] ? dst(pk) : nullptr;
    any |= need[i];
  }
  int spins = 0;
  if (*t.dead_s) any = false;
  while (any) {
    f32x4 v[NP];
    rg_load<NP>(v, ptr);
    any = false;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (need[i]) {
        if (__float_as_int(v[i][0]) == want && __float_as_int(v[i][3]) == want) {
          out[i][0] = v[i][1];
          out[i][1] = v[i][2];
          need[i] = false;
          ptr[i] = own;
        } else {
          any = true;
        }
      }
    }
    if (any && ++spins > RF_SPIN_LIMIT) { *t.err = 1; *t.dead_s = 1; break; }
  }
}

// ---- products.  A chunk = this workgroup's <= 16 columns of one [D, *] map, memory [D][CB].  Wave w contracts rows
// [w D / 8, (w + 1) D / 8) in KM = D / 32 MFMA steps of 4 rows: lane l holds B[k = l / 16][j = l % 16] = W[row0 + 4 m + l / 16][l % 16]
// (lanes with l % 16 >= CB read the neighbouring row's elements or, past the slice, zeros: their output columns are never used).
template <int KM>
__device__ __forceinline__ void wf_issue(float (&wf)[KM], const float *__restrict__ slice, int D, int CB) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)slice, (short)0, D * CB * 4, 0x00020000);
  int off = ((wave * 4 * KM + (lane >> 4)) * CB + (lane & 15)) * 4, step = 16 * CB;
  asm volatile("" : "+v"(off), "+s"(step));          // (as in gemv_issue: keep per-product offsets out of hoisted registers)
#pragma unroll
  for (int m = 0; m < KM; ++m) wf[m] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + m * step, 0, 0));
}
// A fragments of the activations src_s [8][Dp]: lane l holds A[i = l % 16][k = l / 16] = src[(l % 16) & 7][row0 + 4 m + l / 16]
template <int KM>
__device__ __forceinline__ void af_load(float (&af)[KM], const float *src_s, int Dp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *a = src_s + (lane & 7) * Dp + wave * 4 * KM + (lane >> 4);
#pragma unroll
  for (int m = 0; m < KM; ++m) af[m] = a[4 * m];
}
// One chunk: this wave's partial tile -> part_s[wave][ch][row][16] (rows 0 .. 7 = lanes 0 .. 31 of the 16 x 16 result)
template <int KM>
__device__ __forceinline__ void chunk_mfma(const float (&af)[KM], const float (&wf)[KM], float *part_s, int ch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < KM; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m], wf[m], acc, 0, 0, 0);
  if (lane < 32) {
    float *o = part_s + ((wave * 3 + ch) * 8 + 4 * (lane >> 4)) * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r * 16] = acc[r];
  }
}
__device__ __forceinline__ float chunk_sum(const float *part_s, int ch, int g, int c) {
  float s = 0.f;
#pragma unroll
  for (int wv = 0; wv < RF_WAVES; ++wv) s += part_s[((wv * 3 + ch) * 8 + g) * 16 + c];
  return s;
}

// LayerNorm of the 8 rows of src_s [8][Dp] into dst_s (wave w = row w), gains / biases of this lane's columns in registers
template <int NC>
__device__ __forceinline__ void ln_rows(const float *src_s, float *dst_s, int D, int Dp, float eps, const float *gn_s, const float *bs_s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mean, rstd;
  row_stats(src_s + wave * Dp, D, eps, mean, rstd);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = lane + 64 * i;
    if (c < D) dst_s[wave * Dp + c] = (src_s[wave * Dp + c] - mean) * rstd * gn_s[c] + bs_s[c];
  }
}
__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// KM = D / 32 (MFMA steps per wave and chunk), LMAX: window rows the K / V registers of a unit are sized for
// BOX: a Box policy's Gaussian draw (etm_sample_gaussian, float tables p.box) instead of the categorical branches.
// The body is included text (rollout_group_body.inc): the kernels without masks are what they were, the masked kernel (categorical
// policies only) is the same text with MK = true, the Box kernel that also stages the means the same text with MN = true, the
// categorical kernels that also stage every column's log-prob (masks or not) the same text with LP = true.
template <int KM, int LMAX, bool BOX>
__global__ __launch_bounds__(RF_T) void rollout_group_kernel(const RfParams p) {
  constexpr bool MK = false, MN = false, LP = false;
#include "rollout_group_body.inc"
}
template <int KM, int LMAX>
__global__ __launch_bounds__(RF_T) void rollout_group_masked_kernel(const RfParams p) {
  constexpr bool BOX = false, MK = true, MN = false, LP = false;
#include "rollout_group_body.inc"
}
template <int KM, int LMAX>
__global__ __launch_bounds__(RF_T) void rollout_group_gaussian_means_kernel(const RfParams p) {
  constexpr bool BOX = true, MK = false, MN = true, LP = false;
#include "rollout_group_body.inc"
}
template <int KM, int LMAX, bool MK>
__global__ __launch_bounds__(RF_T) void rollout_group_logps_kernel(const RfParams p) {
  constexpr bool BOX = false, MN = false, LP = true;
#include "rollout_group_body.inc"
}

size_t rg_lds_bytes(int D, int nb) { return (size_t)(5 * RG_G * (D + 4) + RG_PART + RF_MAXB * RF_T + 2 * RF_T + nb * 4 * D) * sizeof(float); }
}  // namespace

// 1 when the group kernel takes the shape: GRU-gated blocks, a group of W <= 8 workers with W H <= 32 (worker, head) units, D in
// {128, 384} (the instantiations built: BASELINE configs 2 and 5), whole heads per column block boundary, pieces that fit a slot.
extern "C" int etm_rollout_trxl_group_supported(int D, int H, int L, int hid, int A, int nb, int W, int gtrxl) {
  if (!gtrxl || D <= 0 || H <= 0 || L <= 0 || hid <= 0 || A <= 0 || nb <= 0 || W <= 0 || D % H != 0) return 0;
  if (D != 128 && D != 384) return 0;
  const int hd = D / H, CB = D / RG_WG;
  if (W > RG_G || W * H > RG_WG || nb > RF_MAXB || L > 128 || (D == 128 && L > 64)) return 0;
  if (CB % 2 != 0 || hd % CB != 0 || hd > RG_PIECE || hd % 4 != 0 || RG_G * CB > RG_PIECE) return 0;
  if (RF_T / (hd / 4) < 16 || (hd + 63) / 64 > 2 || hd % ((hd + 63) / 64) != 0) return 0;              // attention mappings of a unit
  if ((2 * hid) % RG_WG != 0) return 0;
  const int CBH = 2 * hid / RG_WG, NCH = (CBH + 15) / 16;
  if (NCH > 3 || CBH % NCH != 0 || CBH > 48 || RG_G * (A + 1) + 1 > RG_PIECE || A + 1 > 16) return 0;
  if (2 * hd > RF_T || (2 * hd) % 4 != 0) return 0;                                                  // tail: K | V columns of a head
  return 1;
}
extern "C" int etm_rollout_trxl_group_grid(void) { return RG_WG; }
extern "C" int64_t etm_rollout_trxl_group_scratch_bytes(int nb) {
  if (nb <= 0) return 0;
  const int64_t n_ex = 7 * (int64_t)nb + 4;                          // exchanges per launch: 7 per gated block + input, embedding, heads
  return 64 + n_ex * RG_WG * 2 * RG_PIECE * (int64_t)sizeof(float);
}

int etm_rf_launch_group(const RfParams &p, hipStream_t st) {
  const dim3 grid(RG_WG), block(RF_T);
  const size_t lds = rg_lds_bytes(p.D, p.nb);
  if (lds + 8192 > 160 * 1024) return ETM_EUNSUPPORTED;
  const bool box = p.box.bx.A > 0;
#define RG_LAUNCH(KM_, LM_)                                                                                                   \
  do {                                                                                                                        \
    auto kern = box ? (p.st_means ? rollout_group_gaussian_means_kernel<KM_, LM_> : rollout_group_kernel<KM_, LM_, true>)     \
                    : p.st_logps ? (p.am ? rollout_group_logps_kernel<KM_, LM_, true> : rollout_group_logps_kernel<KM_, LM_, false>) \
                    : p.am ? rollout_group_masked_kernel<KM_, LM_> : rollout_group_kernel<KM_, LM_, false>;                   \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
    hipLaunchKernelGGL(kern, grid, block, lds, st, p);                                                                        \
  } while (0)
  if (p.D == 128) RG_LAUNCH(4, 64);
  else if (p.L <= 64) RG_LAUNCH(12, 64);
  else RG_LAUNCH(12, 128);
#undef RG_LAUNCH
  return etm_launch_status();
}
