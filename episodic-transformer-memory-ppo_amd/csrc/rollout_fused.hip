// Rollout step, transformer + heads + sampling of one worker group as ONE launch (SURVEY.md section 8 f1;
// /root/reference trainer.py:163-186 -> model.py:96-112 -> transformer.py:222-253 for the post-LN layout without gates).
//
// At 16 - 32 workers a rollout step is not bound by flops or bytes but by the NUMBER of dependent launches on the device
// (5 - 7 us each) and, on the host, by the cost of launching the captured step, which grows with the number of graph nodes
// (~1 us per node).  The block loop of the multi-launch path is 6 launches per block (q GEMM, cached attention, fc_out GEMM,
// residual + LayerNorm, fc GEMM, residual + LayerNorm) + embedding + hidden heads + policy = 21 launches for 3 blocks.
// Workers are independent, so the whole chain of ONE worker is a sequence of matrix-VECTOR products over weights shared by all
// workers.  One workgroup per worker is not enough: a D x D product streams 0.6 MB of weights and one CU takes ~7 us for that
// (measured), no faster than the launch it replaces.  So a worker is handled by a TEAM of P workgroups (P = 4 at H = 4): every
// member owns D / P columns of each product (and H / P heads of the attention), reads a quarter of the weights, and the members
// exchange their pieces through memory (see "team exchange" below).  A team sits on ONE XCD (workgroup b is observed to run on
// XCD b % 8; the block -> (worker, member) map uses that); every spin is bounded (a partner that never shows up sets an error
// word instead of hanging the device).
//
// With the weights split four ways every phase is ONE memory round trip (~2.5 us from the Infinity Cache: the weights do not stay
// in a 4 MB L2 from step to step) and there are ~25 dependent phases, so the kernel is latency-bound, not bandwidth-bound
// (timeline: tools/rollout_stamps.py).  Therefore nothing a phase needs is loaded when the phase starts: the slice of the NEXT
// product sits in registers (512 threads x up to 32 float4) from the moment the previous product has consumed them, the K and V
// columns of the window rows are loaded at the top of the block, biases / gains / mask / sampling inputs before they are needed,
// and the workgroup barriers are bare s_barrier + LDS waits (a __syncthreads() would drain the loads in flight: its release
// fence is s_waitcnt vmcnt(0), loads and stores share that counter on this part).
//
//   exchange E0   h = relu(W_emb x + b)                        each member: its D / P columns           (transformer.py:232)
//   per block b:  item[b] = h (member 0);  q_mine = Wq[:, mine] h;  attention of my heads over the worker's cached K | V rows
//                 (masked_fill(-1e20) BEFORE the / sqrt(D), softmax, att . V: transformer.py:59-75)  -> ctx_mine
//   exchange Ea   partial fc_out products  Wo[mine rows, :] ctx_mine  (all D outputs, summed over the members in member order)
//                 x = LN1(sum + bo + h)                                                                  (transformer.py:143-149)
//   exchange Eb   f_mine = relu(Wfc[:, mine] x + bfc);  h = LN2([f] + x)                                 (transformer.py:160-170)
//   exchange Ez   hidden heads h2_mine = relu(W_heads[:, mine] h + b); partial output-head dot products over h2_mine
//                 member 0: logits / value = sum of the partials + bias, log-softmax, inverse-CDF sample on the pre-drawn uniform
//                 (or the forced action), log-prob, staging rows, action hand-over                       (model.py:104-110)
// Only summation order differs from the multi-launch path.
#include "rollout_shared.h"

namespace {
// GR: rows of a product slice in registers per thread; LMAX: window rows the K / V registers are sized for.
// GEN: the general block layout (pre-LN and / or GRU gates) is compiled in; the post-LN layout without gates (the headline
// configuration) gets a kernel without that code, which keeps its register allocation free of spills.
// BOX: a Box policy's Gaussian draw at the end (etm_sample_gaussian, float tables p.box) instead of the categorical branches.
// The body is included text (rollout_fused_body.inc): the kernels without masks are what they were, the masked kernel (categorical
// policies only) is the same text with MK = true, the Box kernel that also stages the means the same text with MN = true, the
// categorical kernels that also stage every column's log-prob (masks or not) the same text with LP = true.
template <int GR, int LMAX, bool GEN, bool BOX>
__global__ __launch_bounds__(RF_T) void rollout_trxl_kernel(const RfParams p) {
  constexpr bool MK = false, MN = false, LP = false;
#include "rollout_fused_body.inc"
}
template <int GR, int LMAX, bool GEN>
__global__ __launch_bounds__(RF_T) void rollout_trxl_masked_kernel(const RfParams p) {
  constexpr bool BOX = false, MK = true, MN = false, LP = false;
#include "rollout_fused_body.inc"
}
template <int GR, int LMAX, bool GEN>
__global__ __launch_bounds__(RF_T) void rollout_trxl_gaussian_means_kernel(const RfParams p) {
  constexpr bool BOX = true, MK = false, MN = true, LP = false;
#include "rollout_fused_body.inc"
}
template <int GR, int LMAX, bool GEN, bool MK>
__global__ __launch_bounds__(RF_T) void rollout_trxl_logps_kernel(const RfParams p) {
  constexpr bool BOX = false, MN = false, LP = true;
#include "rollout_fused_body.inc"
}
}  // namespace

// ---- lin_hidden of a rollout step as K-slice partial sums (model.py:94-100 without the bias / ReLU, which the consumer adds).
// At 16 rows the [rows, F] x [F, D] product (F = 3136: 4.8 MB of weights) is a latency problem: the library kernel walks K in
// 49 dependent steps on 24 workgroups (13 us).  Here a workgroup owns 32 columns x one of `splits` K slices: all of its weights
// (25 KB) and its slice of the features are requested at once -- one memory round trip on 12 x splits workgroups.
// Thread = (k lane kq of 32, column quad c4 of 8): its weights (16 bytes per owned k row) are all requested up front; rows in
// chunks of 16.  The 32 k lanes are summed in a fixed order: lanes 8 apart inside a 16-lane row by a DPP rotate, the remaining
// 16 partial sums (4 row groups x 4 waves) through LDS.
constexpr int HP_ROWS = 16, HP_KMAX = 256;
__global__ __launch_bounds__(256) void hidden_partial_kernel(const float *__restrict__ x, const float *__restrict__ wt, float *__restrict__ part,
                                                             int W, int F, int D, int kslice) {
  __shared__ float xs[HP_ROWS][HP_KMAX];
  __shared__ __attribute__((aligned(16))) float red[16][HP_ROWS][32];
  const int tid = threadIdx.x, c4 = tid & 7, kq = tid >> 3, lane = tid & 63, wave = tid >> 6;
  const int col0 = (int)blockIdx.x * 32, s = (int)blockIdx.y;
  const int k0 = s * kslice, kn = min(kslice, F - k0);              // this slice: rows k0 .. k0 + kn of the [F, D] matrix
  constexpr int KI = HP_KMAX / 32;
  f32x4 wreg[KI];
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int kk = kq + 32 * i;
    wreg[i] = (kk < kn) ? *reinterpret_cast<const f32x4 *>(wt + (long long)(k0 + kk) * D + col0 + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int r0 = 0; r0 < W; r0 += HP_ROWS) {
    const int rows = min(HP_ROWS, W - r0);
    __syncthreads();
    for (int i = tid; i < HP_ROWS * HP_KMAX; i += 256) {
      const int r = i / HP_KMAX, kk = i - r * HP_KMAX;
      xs[r][kk] = (r < rows && kk < kn) ? x[(long long)(r0 + r) * F + k0 + kk] : 0.f;
    }
    __syncthreads();
    f32x4 acc[HP_ROWS];
#pragma unroll
    for (int r = 0; r < HP_ROWS; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int kk = kq + 32 * i;
#pragma unroll
      for (int r = 0; r < HP_ROWS; ++r) acc[r] += xs[r][kk] * wreg[i];
    }
    const int rg = wave * 4 + (lane >> 4);                         // 16-lane row group: 2 k lanes x 8 column quads
#pragma unroll
    for (int r = 0; r < HP_ROWS; ++r) {
#pragma unroll
      for (int j = 0; j < 4; ++j)                                  // + the lane 8 further in the row (row_ror:8): the other k lane
        acc[r][j] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[r][j]), 0x128, 0xf, 0xf, false));
      if ((lane & 8) == 0) *reinterpret_cast<f32x4 *>(&red[rg][r][c4 * 4]) = acc[r];
    }
    __syncthreads();
    for (int o = tid; o < HP_ROWS * 32; o += 256) {
      const int r = o >> 5, c = o & 31;
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) t += red[g][r][c];
      if (r < rows) part[((long long)s * W + r0 + r) * D + col0 + c] = t;
    }
  }
}

#ifdef ETM_RF_STAMPS
extern "C" int etm_diag_rollout_trxl_stamps(long long *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rf_stamps), sizeof(long long) * 64) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int etm_rollout_trxl_team(int H) { return (H % 4 == 0) ? 4 : ((H % 2 == 0) ? 2 : 1); }

// Placement of a launch's workgroups (process-wide, read at launch): 0 (default) = a team's members on one XCD, 1 = one member
// index per XCD.  Results do not depend on it: members communicate through system-scope packets only, and every cache / bank
// location a member reads was written by itself or by an earlier kernel.
static int g_rf_placement = 0;
extern "C" int etm_rollout_trxl_set_placement(int mode) {
  if (mode != 0 && mode != 1) return ETM_EINVAL;
  g_rf_placement = mode;
  return ETM_OK;
}
// workgroups of one launch for W workers under the current placement (all of them must be resident at once: <= 256)
extern "C" int etm_rollout_trxl_grid(int W, int H) {
  if (W <= 0 || H <= 0) return 0;
  const int P = etm_rollout_trxl_team(H);
  return g_rf_placement == 0 ? (W + 7) / 8 * 8 * P : 8 * ((W + 8 / P - 1) / (8 / P));
}

// 1 when etm_rollout_trxl handles the shape (16-byte pieces, a member's columns on <= 64 lanes x 2 per window row and >= 16 row
// groups in the context phase, full rows on the 512 threads, everything in the static LDS buffers), else 0 (the caller keeps the
// multi-launch path).
extern "C" int etm_rollout_trxl_supported(int D, int H, int L, int hid, int A, int nb) {
  if (D <= 0 || H <= 0 || L <= 0 || hid <= 0 || A <= 0 || nb <= 0 || D % H != 0) return 0;
  const int P = etm_rollout_trxl_team(H);
  if (nb > RF_MAXB || D % (4 * P) != 0 || D > RF_T || H > 8 || L > 128 || (2 * hid) % (4 * P) != 0 || A + 1 > 64 || (D / H) % 4 != 0) return 0;
  const int DS = D / P, OS = 2 * hid / P, cpl = (DS + 63) / 64, HS = H / P;
  if (DS > 128 || DS % cpl != 0 || OS > 256 || (HS > 1 && (DS / cpl != 64 || (HS & (HS - 1)) != 0))) return 0;
  return 1;
}
// Register rows per product slice (20 at D = 384, 32 at D = 512) and the GRU-gate packing that goes with a shape.
static int rf_rows(int D, int H) {
  const int P = etm_rollout_trxl_team(H), DS = D / P;
  const int rows_q = (D + RF_T / (DS / 4) - 1) / (RF_T / (DS / 4)), rows_o = (DS + RF_T / (D / 4) - 1) / (RF_T / (D / 4));
  return (rows_q <= 20 && rows_o <= 20) ? 20 : 32;
}
// 1: a gate's maps of y ([Wr | Wz | Wg]^T) and of x ([Ur | Uz]^T) are ONE product each over the member's 3 DS / 2 DS columns --
// pack them member-blocked as [P][D][3 DS] / [P][D][2 DS]; 0: five separate column blocks -- pack [P][3][D][DS] / [P][2][D][DS].
// Merged when the merged product still fits two register batches (phases are pure latency at small D; at D = 384 the merged
// product would be three batches with two exposed round trips).
extern "C" int etm_rollout_trxl_gate_merged(int D, int H) {
  if (D <= 0 || H <= 0 || D % H != 0) return 0;
  const int P = etm_rollout_trxl_team(H);
  if (D % (4 * P) != 0) return 0;
  const int DS = D / P, kch = RF_T / (3 * DS / 4);
  if (kch <= 0) return 0;
  return (D + kch - 1) / kch <= 2 * rf_rows(D, H) ? 1 : 0;
}
extern "C" int64_t etm_rollout_trxl_scratch_bytes(int W, int D, int H, int nb) {
  if (W <= 0 || D <= 0 || H <= 0 || nb <= 0) return 0;
  const int P = etm_rollout_trxl_team(H);
  const int64_t slots = 6 * (int64_t)nb + 2;                       // exchanges per launch: up to 6 per block (gated layout) + 2
  return 64 + (int64_t)W * slots * P * 2 * D * (int64_t)sizeof(float);
}

// part [splits, W, D] = K-slice sums of x [W, F] @ wt [F, D] (wt = the layer's weight TRANSPOSED); splits = etm_rollout_hidden_splits(F).
extern "C" int etm_rollout_hidden_splits(int F) {
  if (F <= 0) return 0;
  int s = (F + HP_KMAX - 1) / HP_KMAX;            // slices of at most HP_KMAX rows ...
  constexpr int HP_SPLITS = 16;                   // (the consumer adds up to RF_MAXSPLIT = 64 rows; this kernel's grid is tuned for 16)
  if (s < HP_SPLITS && F >= 32 * HP_SPLITS) s = HP_SPLITS;   // ... and as many as that when K is long
  return s <= HP_SPLITS ? s : 0;
}
extern "C" int etm_rollout_hidden_partial(const float *x, const float *wt, float *part, int W, int F, int D, void *stream) {
  (void)hipGetLastError();
  if (!x || !wt || !part || W <= 0 || F <= 0 || D <= 0) return ETM_EINVAL;
  const int splits = etm_rollout_hidden_splits(F);
  if (splits == 0 || D % 32 != 0 || ((uintptr_t)wt % 16) != 0) return ETM_EUNSUPPORTED;
  const int kslice = (F + splits - 1) / splits;
  if (kslice > HP_KMAX) return ETM_EUNSUPPORTED;
  EtmProfScope prof(ETM_K_HIDDEN_PARTIAL, (hipStream_t)stream);
  hipLaunchKernelGGL(hidden_partial_kernel, dim3((unsigned)(D / 32), (unsigned)splits), dim3(256), 0, (hipStream_t)stream, x, wt, part, W, F, D, kslice);
  return etm_launch_status();
}

// One launch per worker group and rollout step.  blocks: nb structs of 19 device pointers each, in the order
// (wq_t, wo_t, bo, ln1_gain, ln1_bias, wfc_t, bfc, ln2_gain, ln2_bias,  gate1: wy_t, ux_t, ug_t, bg,  gate2: the same four,  norm_kv gain,
// norm_kv bias); *_t = the nn.Linear weight TRANSPOSED ([in, out]).  Every matrix that is split by columns over the P =
// etm_rollout_trxl_team(H) members (wemb_t, wq_t, wfc_t, ug_t, wh_t, wkv) is MEMBER-BLOCKED [P][in][out / P]; wo_t (split by rows) stays
// [D, D]; wy_t = [Wr | Wz | Wg]^T and ux_t = [Ur | Uz]^T are [P][D][j DS] if etm_rollout_trxl_gate_merged(D, H), else [P][j][D][DS] (DS = D / P).  The gate entries are read with
// gtrxl != 0 only, the norm_kv entries (both or neither) by the tail of a pre-LN model; pre_ln / gtrxl select the block layout of
// transformer.py:117-172.
// scratch: etm_rollout_trxl_scratch_bytes(W, D, H, nb) bytes, ZEROED once by the caller before the first launch and then left alone
// (int64 launch counter, int64 error word -- non-zero = a team member timed out --, then the exchange slots).
// Tail (wkv != NULL): after the action hand-over the same launch writes the new memory items into bank[slot_l[w], step_l[w]] and
// their K | V projection (items + pos[step_l[w]]) wkv[b] into kv[w, step_l[w]] -- what the multi-launch path does with five more
// launches while the host steps the environments.
// h_splits > 0: h_in is the [h_splits, W, D] output of etm_rollout_hidden_partial and the transformer input is relu(sum + h_bias).
//
// The 12 launch entries (worker and group form of: one branch, MultiDiscrete, with masks, with every column's log-prob, Box, Box with
// the means) share one call record: an entry fills it by field name and hands it to rollout_trxl_run, which validates -- in the
// order written there, the order in which refusals win -- and launches.  The entries hold no checks of their own.
namespace {
struct RfCall {
  RfParams p;                        // the kernels' parameters as the entry's arguments give them; the rest is derived by the validator
  int group;                         // 0: a team of workgroups per worker (this file); 1: the group form (csrc/rollout_group.hip)
  void *scratch;
  int64_t scratch_bytes;
  const void *const *blocks;         // the raw block table: p.nb x RF_BLOCK_PTRS device pointers
  const int32_t *branch_sizes;       // categorical policies: HOST array, or NULL with n_branches = 1 for one branch of p.A actions
  int n_branches;
  bool box;                          // a Box policy: p.box holds the action tables, low / high (HOST arrays or NULL) its bounds
  const float *low, *high;
  bool need_mask, need_means, need_logps;   // the optional tables p.am / p.st_means / p.st_logps that this entry makes mandatory
  hipStream_t stream;
};

// The worker form's kernel of (register rows 20 / 32, window rows 64 / 128, general block layout, variant)
using RfKernel = void (*)(const RfParams);
enum { RF_PLAIN, RF_MASKED, RF_LOGPS, RF_LOGPS_MASKED, RF_BOX, RF_BOX_MEANS, RF_VARIANTS };
#define RF_VARIANT_ROW(GR, LM, GEN)                                                                                                   \
  { rollout_trxl_kernel<GR, LM, GEN, false>, rollout_trxl_masked_kernel<GR, LM, GEN>, rollout_trxl_logps_kernel<GR, LM, GEN, false>, \
    rollout_trxl_logps_kernel<GR, LM, GEN, true>, rollout_trxl_kernel<GR, LM, GEN, true>, rollout_trxl_gaussian_means_kernel<GR, LM, GEN> }
#define RF_LAYOUT_ROWS(GR, LM) { RF_VARIANT_ROW(GR, LM, false), RF_VARIANT_ROW(GR, LM, true) }
const RfKernel rf_kernels[2][2][2][RF_VARIANTS] = {{RF_LAYOUT_ROWS(20, 64), RF_LAYOUT_ROWS(20, 128)},
                                                   {RF_LAYOUT_ROWS(32, 64), RF_LAYOUT_ROWS(32, 128)}};
#undef RF_LAYOUT_ROWS
#undef RF_VARIANT_ROW

int rollout_trxl_run(RfCall &c) {
  RfParams &p = c.p;
  (void)hipGetLastError();
  if (c.need_mask && !p.am) return ETM_EINVAL;
  if (c.box)
    if (const int rc = etm_box_make(c.low, c.high, p.A, &p.box.bx)) return rc;
  if (c.need_means && (!p.st_means || ((uintptr_t)p.st_means & 3u))) return ETM_EINVAL;
  if (c.need_logps && (!p.st_logps || ((uintptr_t)p.st_logps & 3u))) return ETM_EINVAL;
  if (p.ss && (!p.mask_table || !p.index_table || !p.st_mask || !p.st_idx || !p.latch || !p.mask_t || !p.win_t || p.T <= 0)) return ETM_EINVAL;
  if (!p.ss && (!p.win || !p.mask)) return ETM_EINVAL;
  // (a Box policy's action tables are the float ones of p.box; the int64 ones are unused then)
  const bool tables = c.box ? (p.box.log_std && p.box.normals && p.box.actions && p.box.st_actions) : (p.uniforms && p.actions && p.st_actions);
  if (!p.h_in || !p.wemb_t || !p.bemb || !c.blocks || !p.kv || !p.items || !p.wh_t || !p.bh || !p.wp || !p.bp || !p.wv || !p.bv || !tables ||
      !p.t_dev || !p.st_logp || !p.st_values || !p.sync_counter || !c.scratch)
    return ETM_EINVAL;
  if (p.W <= 0 || p.nb <= 0 || p.D <= 0 || p.H <= 0 || p.L <= 0 || p.hid <= 0 || p.A <= 0 || p.stage_W < p.W || p.D % p.H != 0) return ETM_EINVAL;
  if (p.host_flag && !(c.box ? (const void *)p.box.host_actions : (const void *)p.host_actions)) return ETM_EINVAL;
  if (const int rc = etm_action_mask_check(p.am, p.A)) return rc;
  if (p.wkv && (!p.step_l || !p.slot_l || !p.bank)) return ETM_EINVAL;
  if (p.h_splits < 0 || p.h_splits > RF_MAXSPLIT || (p.h_splits > 0 && !p.h_bias)) return ETM_EINVAL;
  p.P = etm_rollout_trxl_team(p.H);
  if (c.group) {
    if (!etm_rollout_trxl_group_supported(p.D, p.H, p.L, p.hid, p.A, p.nb, p.W, p.gtrxl) || (p.wkv && p.P != p.H)) return ETM_EUNSUPPORTED;
    if (c.scratch_bytes < etm_rollout_trxl_group_scratch_bytes(p.nb)) return ETM_EWORKSPACE;
  } else {
    if (!etm_rollout_trxl_supported(p.D, p.H, p.L, p.hid, p.A, p.nb) || etm_rollout_trxl_grid(p.W, p.H) > 256) return ETM_EUNSUPPORTED;   // all teams resident
    if (c.scratch_bytes < etm_rollout_trxl_scratch_bytes(p.W, p.D, p.H, p.nb)) return ETM_EWORKSPACE;
  }
  if (const int rc = etm_branches_make(c.branch_sizes, c.n_branches, p.A, &p.br)) return rc;
  for (int b = 0; b < p.nb; ++b) {
    const float *const *q = reinterpret_cast<const float *const *>(c.blocks) + RF_BLOCK_PTRS * b;
    for (int k = 0; k < 9; ++k) if (!q[k]) return ETM_EINVAL;
    if (p.gtrxl) for (int k = 9; k < 17; ++k) if (!q[k]) return ETM_EINVAL;
    if ((q[17] == nullptr) != (q[18] == nullptr)) return ETM_EINVAL;
    p.blk[b] = RfBlock{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8],
                       RfGate{q[9], q[10], q[11], q[12]}, RfGate{q[13], q[14], q[15], q[16]}, q[17], q[18]};
  }
  // what the kernels take besides the entry's arguments
  p.merge_gate = etm_rollout_trxl_gate_merged(p.D, p.H);
  p.n_slots = 6 * p.nb + 2;
  p.ctl = (long long *)c.scratch;
  p.xbuf = reinterpret_cast<float *>((char *)c.scratch + 64);
  p.sqrt_d = (float)sqrt((double)p.D);
  EtmProfScope prof(ETM_K_ROLLOUT_FUSED, c.stream);
  if (c.group) return etm_rf_launch_group(p, c.stream);        // csrc/rollout_group.hip: weights once per group and step (gated layouts)
  p.map_mode = g_rf_placement;
  const int variant = c.box ? (p.st_means ? RF_BOX_MEANS : RF_BOX) : p.st_logps ? (p.am ? RF_LOGPS_MASKED : RF_LOGPS) : p.am ? RF_MASKED : RF_PLAIN;
  // (rows per thread of the per-block product slices: 20 registers x 4 are enough at D = 384, 32 at D = 512)
  const RfKernel kern = rf_kernels[rf_rows(p.D, p.H) == 20 ? 0 : 1][p.L <= 64 ? 0 : 1][p.pre_ln || p.gtrxl ? 1 : 0][variant];
  hipLaunchKernelGGL(kern, dim3((unsigned)etm_rollout_trxl_grid(p.W, p.H)), dim3(RF_T), 0, c.stream, p);
  return etm_launch_status();
}
}  // namespace

// The C signatures are fixed (include/etm_hip.h), so the shared head and middle of the 12 argument lists are spelled once here and
// once in RF_FILL, which also opens the record `c`; the draw arguments of a categorical (T = int64_t) or Box (T = float) policy lie
// between them, behind `uniforms` or `log_std, normals`.
#define RF_HEAD_ARGS                                                                                                                      \
  const float *h_in, const float *wemb_t, const float *bemb, const void *const *blocks, int nb, float *kv, int64_t kv_worker_stride,     \
      int64_t kv_row_stride, const int64_t *win, const uint8_t *mask, float *items, const float *wh_t, const float *bh, const float *wp,  \
      const float *bp, const float *wv, const float *bv
#define RF_DRAW_ARGS(T) const T *forced, int64_t *t_dev, T *actions, T *st_actions, float *st_logp, float *st_values, T *host_actions
#define RF_MIDDLE_ARGS                                                                                                                    \
  int64_t *host_flag, int32_t *sync_counter, float ln_eps, void *scratch, int64_t scratch_bytes, const float *wkv, const float *pos,     \
      const int64_t *step_l, const int64_t *slot_l, float *bank, int64_t bank_slot_stride, int64_t bank_row_stride,                      \
      int64_t bank_block_stride, const float *h_bias, int h_splits, const int64_t *ss, const uint8_t *mask_table,                        \
      const int64_t *index_table, uint8_t *st_mask, int64_t *st_idx, int64_t *latch, int64_t *t_row, uint8_t *mask_t, int64_t *win_t,    \
      const float *kv_init, int T, int pre_ln, int gtrxl, int W, int D, int H, int L, int hid
#define RF_FILL(form)                                                                                                                     \
  RfCall c{};                                                                                                                             \
  c.group = form; c.blocks = blocks; c.scratch = scratch; c.scratch_bytes = scratch_bytes; c.n_branches = 1; c.stream = (hipStream_t)stream; \
  c.p.h_in = h_in; c.p.wemb_t = wemb_t; c.p.bemb = bemb; c.p.nb = nb; c.p.kv = c.p.kv_out = kv; c.p.kv_w_stride = kv_worker_stride;                   \
  c.p.kv_row_stride = kv_row_stride; c.p.win = (const long long *)win; c.p.mask = mask; c.p.items = items; c.p.wh_t = wh_t; c.p.bh = bh; \
  c.p.wp = wp; c.p.bp = bp; c.p.wv = wv; c.p.bv = bv;                                                                                     \
  c.p.t_dev = (long long *)t_dev; c.p.st_logp = st_logp; c.p.st_values = st_values;                                                       \
  c.p.host_flag = (long long *)host_flag; c.p.sync_counter = (int *)sync_counter; c.p.eps = ln_eps; c.p.wkv = wkv; c.p.pos = pos;        \
  c.p.step_l = (const long long *)step_l; c.p.slot_l = (const long long *)slot_l; c.p.bank = bank;                                       \
  c.p.bank_slot_stride = bank_slot_stride; c.p.bank_row_stride = bank_row_stride; c.p.bank_block_stride = bank_block_stride;             \
  c.p.h_bias = h_bias; c.p.h_splits = h_splits; c.p.ss = (const long long *)ss; c.p.mask_table = mask_table;                             \
  c.p.index_table = (const long long *)index_table; c.p.st_mask = st_mask; c.p.st_idx = (long long *)st_idx;                             \
  c.p.latch = (long long *)latch; c.p.t_row = (long long *)t_row; c.p.mask_t = mask_t; c.p.win_t = (long long *)win_t;                   \
  c.p.kv_init = kv_init; c.p.T = T; c.p.pre_ln = pre_ln; c.p.gtrxl = gtrxl; c.p.W = W; c.p.D = D; c.p.H = H; c.p.L = L; c.p.hid = hid;   \
  c.p.stage_W = stage_W
#define RF_FILL_CATEGORICAL                                                                                                               \
  c.p.uniforms = uniforms; c.p.forced = (const long long *)forced; c.p.actions = (long long *)actions;                                   \
  c.p.st_actions = (long long *)st_actions; c.p.host_actions = (long long *)host_actions
#define RF_FILL_BRANCHES c.branch_sizes = branch_sizes; c.n_branches = n_branches; c.p.A = etm_branches_total(branch_sizes, n_branches)
#define RF_FILL_BOX                                                                                                                       \
  c.box = true; c.low = low; c.high = high; c.p.A = A; c.p.box.log_std = log_std; c.p.box.normals = normals; c.p.box.forced = forced;    \
  c.p.box.actions = actions; c.p.box.st_actions = st_actions; c.p.box.host_actions = host_actions

#define RF_ARGS RF_HEAD_ARGS, const float *uniforms, RF_DRAW_ARGS(int64_t), RF_MIDDLE_ARGS, int A, int stage_W, void *stream
extern "C" int etm_rollout_trxl(RF_ARGS) {
  RF_FILL(0); RF_FILL_CATEGORICAL; c.p.A = A;
  return rollout_trxl_run(c);
}
// The group form (csrc/rollout_group.hip): same arguments, other matrix packings (see there) and scratch size
// (etm_rollout_trxl_group_scratch_bytes); W <= 8 workers, GRU-gated blocks -- etm_rollout_trxl_group_supported.
extern "C" int etm_rollout_trxl_group(RF_ARGS) {
  RF_FILL(1); RF_FILL_CATEGORICAL; c.p.A = A;
  return rollout_trxl_run(c);
}
#undef RF_ARGS

// MultiDiscrete policies: the same two launches with the action branches given by their sizes (wp / bp = the branches' heads
// concatenated, A = the sum of the sizes); uniforms, forced, st_actions and st_logp are [S, stage_W, B], actions and host_actions [W, B].
#define RF_BRANCHED_ARGS                                                                                                                  \
  RF_HEAD_ARGS, const float *uniforms, RF_DRAW_ARGS(int64_t), RF_MIDDLE_ARGS, int stage_W, const int32_t *branch_sizes, int n_branches
extern "C" int etm_rollout_trxl_branched(RF_BRANCHED_ARGS, void *stream) {
  RF_FILL(0); RF_FILL_CATEGORICAL; RF_FILL_BRANCHES;
  return rollout_trxl_run(c);
}
extern "C" int etm_rollout_trxl_group_branched(RF_BRANCHED_ARGS, void *stream) {
  RF_FILL(1); RF_FILL_CATEGORICAL; RF_FILL_BRANCHES;
  return rollout_trxl_run(c);
}
// Invalid-action masks: the two branched launches (a Discrete policy is one branch, n_branches = 1) with action_mask [W] int64, the
// words of this group's workers for this step (bit j = column j of the concatenated policy head is allowed; every branch has a valid
// action -- the host's duty).  Device or pinned host memory: the sampling workgroup reads its word in place at the start of the launch,
// where it fetches the step's uniforms.  ETM_EINVAL: NULL or misaligned mask; ETM_EUNSUPPORTED: more than 63 columns.
extern "C" int etm_rollout_trxl_branched_masked(RF_BRANCHED_ARGS, const int64_t *action_mask, void *stream) {
  RF_FILL(0); RF_FILL_CATEGORICAL; RF_FILL_BRANCHES;
  c.p.am = (const long long *)action_mask; c.need_mask = true;
  return rollout_trxl_run(c);
}
extern "C" int etm_rollout_trxl_group_branched_masked(RF_BRANCHED_ARGS, const int64_t *action_mask, void *stream) {
  RF_FILL(1); RF_FILL_CATEGORICAL; RF_FILL_BRANCHES;
  c.p.am = (const long long *)action_mask; c.need_mask = true;
  return rollout_trxl_run(c);
}
// The exact categorical KL (`exact_kl: true`): the two masked launches with action_mask optional (NULL: no masks) and st_logps
// [S, stage_W, sum(sizes)] (at this group's first worker, as st_actions) before the stream: every column's log-prob lg[j] - lse of
// the row -- sampled, greedy or forced action alike; -inf for a masked-out column; the st_logp entry's bits at the taken action --,
// stored by the sampling thread as it draws.  Every other output is the twin's, bit for bit.  ETM_EINVAL: NULL or 4-byte-misaligned st_logps.
extern "C" int etm_rollout_trxl_branched_logps(RF_BRANCHED_ARGS, const int64_t *action_mask, float *st_logps, void *stream) {
  RF_FILL(0); RF_FILL_CATEGORICAL; RF_FILL_BRANCHES;
  c.p.am = (const long long *)action_mask; c.p.st_logps = st_logps; c.need_logps = true;
  return rollout_trxl_run(c);
}
extern "C" int etm_rollout_trxl_group_branched_logps(RF_BRANCHED_ARGS, const int64_t *action_mask, float *st_logps, void *stream) {
  RF_FILL(1); RF_FILL_CATEGORICAL; RF_FILL_BRANCHES;
  c.p.am = (const long long *)action_mask; c.p.st_logps = st_logps; c.need_logps = true;
  return rollout_trxl_run(c);
}
#undef RF_BRANCHED_ARGS
extern "C" int etm_rollout_trxl_supported_branched(int D, int H, int L, int hid, const int32_t *branch_sizes, int n_branches, int nb) {
  const int A = etm_branches_total(branch_sizes, n_branches);
  return A > 0 && etm_rollout_trxl_supported(D, H, L, hid, A, nb);
}
extern "C" int etm_rollout_trxl_group_supported_branched(int D, int H, int L, int hid, const int32_t *branch_sizes, int n_branches, int nb,
                                                         int W, int gtrxl) {
  const int A = etm_branches_total(branch_sizes, n_branches);
  return A > 0 && etm_rollout_trxl_group_supported(D, H, L, hid, A, nb, W, gtrxl);
}

// Box policies (diagonal Gaussian, A <= 8 dimensions): the same two launches with the A means as the policy head (wp [A, hid], bp [A]),
// the draw of etm_sample_gaussian (normals / forced / st_actions [S, stage_W, A], NaN forced = "sample"; actions / host_actions [W, A]
// receive the actions clipped to [low, high], HOST arrays of A floats or NULL = unbounded) and log_std [A] on the device.
#define RF_GAUSSIAN_ARGS                                                                                                                  \
  RF_HEAD_ARGS, const float *log_std, const float *normals, RF_DRAW_ARGS(float), RF_MIDDLE_ARGS, int A, int stage_W, const float *low,   \
      const float *high
extern "C" int etm_rollout_trxl_gaussian(RF_GAUSSIAN_ARGS, void *stream) {
  RF_FILL(0); RF_FILL_BOX;
  return rollout_trxl_run(c);
}
extern "C" int etm_rollout_trxl_group_gaussian(RF_GAUSSIAN_ARGS, void *stream) {
  RF_FILL(1); RF_FILL_BOX;
  return rollout_trxl_run(c);
}
// The same two entries with the policy's means staged as well: st_means [S, stage_W, A] next to st_actions (at this group's first
// worker, as st_actions), forced action or not.  ETM_EINVAL: NULL or 4-byte-misaligned st_means.
extern "C" int etm_rollout_trxl_gaussian_means(RF_GAUSSIAN_ARGS, float *st_means, void *stream) {
  RF_FILL(0); RF_FILL_BOX;
  c.p.st_means = st_means; c.need_means = true;
  return rollout_trxl_run(c);
}
extern "C" int etm_rollout_trxl_group_gaussian_means(RF_GAUSSIAN_ARGS, float *st_means, void *stream) {
  RF_FILL(1); RF_FILL_BOX;
  c.p.st_means = st_means; c.need_means = true;
  return rollout_trxl_run(c);
}
#undef RF_GAUSSIAN_ARGS
#undef RF_FILL_BOX
#undef RF_FILL_BRANCHES
#undef RF_FILL_CATEGORICAL
#undef RF_FILL
#undef RF_MIDDLE_ARGS
#undef RF_DRAW_ARGS
#undef RF_HEAD_ARGS
extern "C" int etm_rollout_trxl_supported_gaussian(int D, int H, int L, int hid, int A, int nb) {
  return A > 0 && A <= ETM_MAX_BOX && etm_rollout_trxl_supported(D, H, L, hid, A, nb);
}
extern "C" int etm_rollout_trxl_group_supported_gaussian(int D, int H, int L, int hid, int A, int nb, int W, int gtrxl) {
  return A > 0 && A <= ETM_MAX_BOX && etm_rollout_trxl_group_supported(D, H, L, hid, A, nb, W, gtrxl);
}
