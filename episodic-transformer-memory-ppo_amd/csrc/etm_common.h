// Shared device helpers for the gfx950 kernels (wave = 64 lanes, MFMA f32 32x32x2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/etm_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define ETM_WAVE 64

// C/D fragment of v_mfma_f32_32x32x2_f32: lane holds column (lane & 31); register r holds row
//   (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)          (cdna_hip_programming.md section 3)
// A buffer descriptor whose words come from v_readfirstlane (a VALU write of SGPRs) must not be read by a vector-memory instruction
// within 5 wait states.  The compiler pads that hazard for its own instructions but cannot see a buffer_load / buffer_store inside
// inline assembly: a descriptor built right in front of hand-written loads read stale SGPRs (memory access fault at {base_hi, 0}).
// Every descriptor that feeds inline-assembly memory instructions goes through this fence once.
template <class R>
__device__ __forceinline__ void etm_rsrc_fence(R &r) { asm volatile("s_nop 4" : "+s"(r)); }

__device__ __forceinline__ int mfma32_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// Wave-wide reductions on the DPP path (no LDS round trips): xor-1 / xor-2 inside a quad, the other quad of the 8-group
// (row_half_mirror), the other half of the 16-lane row (row_mirror) -- after these every lane of a row holds the row total --
// then the row totals are accumulated into the last row (row_bcast:15 / :31, gfx9) and lane 63 is broadcast through an SGPR.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float etm_dpp(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += etm_dpp<0xB1, 0xF>(0.f, v);    // quad_perm [1,0,3,2]
  v += etm_dpp<0x4E, 0xF>(0.f, v);    // quad_perm [2,3,0,1]
  v += etm_dpp<0x141, 0xF>(0.f, v);   // row_half_mirror
  v += etm_dpp<0x140, 0xF>(0.f, v);   // row_mirror
  v += etm_dpp<0x142, 0xA>(0.f, v);   // row_bcast:15 into rows 1, 3
  v += etm_dpp<0x143, 0xC>(0.f, v);   // row_bcast:31 into rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, etm_dpp<0xB1, 0xF>(v, v));
  v = fmaxf(v, etm_dpp<0x4E, 0xF>(v, v));
  v = fmaxf(v, etm_dpp<0x141, 0xF>(v, v));
  v = fmaxf(v, etm_dpp<0x140, 0xF>(v, v));
  v = fmaxf(v, etm_dpp<0x142, 0xA>(v, v));   // rows not written keep their own value (old = v)
  v = fmaxf(v, etm_dpp<0x143, 0xC>(v, v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// sum over the 32 lanes that share (lane >> 5)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Invalid-action masks (action_masks: true): bit j of a step's 64-bit word says whether column j of the concatenated policy head is
// allowed; branch b owns bits [off_b, off_b + A_b), handed to the branch functions below shifted down by off_b.  MK = true reads
// the logit of a masked-out action as -INFINITY in front of the ONE sampling arithmetic below: its exponential is +0 (adds nothing
// to a sum, and the inverse CDF cannot stop on it), it never equals the branch maximum, and what is left is, operation for
// operation, the unmasked arithmetic on the branch compacted to its valid actions.  MK = false (the default of every template
// here) is exactly the code without masks.  A branch with no valid action never reaches the device (the host refuses the word).
template <bool MK>
__device__ __forceinline__ float etm_masked_logit(const float *lg, int j, unsigned long long m) {
  if constexpr (MK) return ((m >> j) & 1ull) ? lg[j] : -INFINITY;
  else return lg[j];
}

// Inverse-CDF draw from the categorical over the A logits lg with log-normaliser lse (every sampling site: rollout_sample_kernel,
// rollout_policy_kernel and both step kernels).  The action is the smallest j with u < C_j, C_j = the fp32 running sum of
// expf(lg[i] - lse) over i <= j.  That total can end below 1, and below the largest fp32 uniform 1 - 2^-24: a draw at or past it
// takes the LAST action whose term is positive, never one of probability zero (torch.multinomial's contract).
template <bool MK = false>
__device__ __forceinline__ int etm_sample_categorical(const float *lg, int A, float lse, float u, unsigned long long m = 0) {
  float c = 0.f;
  int last = A - 1;
  for (int j = 0; j < A; ++j) {
    const float e = expf(etm_masked_logit<MK>(lg, j, m) - lse);
    c += e;
    if (e > 0.f) last = j;
    if (u < c) return j;
  }
  return last;
}

// Action branches of a MultiDiscrete policy (one per nvec entry): branch b owns logit columns [off_b, off_b + size[b]) of the
// concatenated policy head, off_b = the sum of the sizes before it.  A Discrete policy is n = 1, size[0] = A.  Passed to the
// kernels by value (no device allocation, graph-capturable).
constexpr int ETM_MAX_BRANCHES = 16;
struct EtmBranches {
  int n;
  int size[ETM_MAX_BRANCHES];
};

// Host side: the branch table of (sizes, n) -- sizes == NULL and n <= 1 means one branch of total_a actions.  0 on success;
// ETM_EINVAL for a bad table, ETM_EUNSUPPORTED for more than ETM_MAX_BRANCHES branches or a sum that is not total_a.
static inline int etm_branches_make(const int32_t *sizes, int n, int total_a, EtmBranches *out) {
  if (!sizes && n <= 1) {
    out->n = 1;
    out->size[0] = total_a;
    return total_a > 0 ? 0 : ETM_EINVAL;
  }
  if (!sizes || n <= 0) return ETM_EINVAL;
  if (n > ETM_MAX_BRANCHES) return ETM_EUNSUPPORTED;
  int s = 0;
  out->n = n;
  for (int b = 0; b < n; ++b) {
    if (sizes[b] <= 0) return ETM_EINVAL;
    out->size[b] = sizes[b];
    s += sizes[b];
  }
  return s == total_a ? 0 : ETM_EINVAL;
}
// An optional action-mask word array (int64, one word per worker or sample): NULL = no masks; else 8-byte aligned, and the A
// columns must fit the 63 usable bits.
static inline int etm_action_mask_check(const void *mask, int A) {
  if (!mask) return 0;
  if (((uintptr_t)mask & 7u) != 0) return ETM_EINVAL;
  return A <= 63 ? 0 : ETM_EUNSUPPORTED;
}
static inline int etm_branches_total(const int32_t *sizes, int n) {
  if (!sizes || n <= 0 || n > ETM_MAX_BRANCHES) return 0;
  int s = 0;
  for (int b = 0; b < n; ++b) {
    if (sizes[b] <= 0) return 0;
    s += sizes[b];
  }
  return s;
}

// The mode of one branch: the smallest index whose logit equals the branch's maximum mx (as computed by etm_sample_branch; the last
// index when none compares equal, which only NaN logits can cause).
template <bool MK = false>
__device__ __forceinline__ int etm_branch_mode(const float *lg, int A, float mx, unsigned long long m = 0) {
  for (int j = 0; j < A - 1; ++j)
    if (etm_masked_logit<MK>(lg, j, m) == mx) return j;
  return A - 1;
}

// One branch's draw: log-sum-exp over its own A logits, then the inverse CDF at its own uniform u -- or the forced action when
// forced >= 0, or the MODE of the branch (etm_branch_mode: the first maximum) when the uniform is negative: u < 0 is the greedy
// sentinel of the uniform tables, chosen per (step, worker, branch) entry, so evaluation replays the step graphs captured for
// training.  A uniform in [0, 1) -- and a NaN one, for which u < 0 is false -- takes the inverse CDF exactly as before.  Returns the
// action (inside the branch) and its log-prob lg[a] - lse in all three cases.  With one branch this is exactly the single-branch
// arithmetic of every sampling site (same operations in the same order).
// MK: the branch's bits m of the step's mask word (bit j = action j of THIS branch); a forced action is taken as it is (the host
// checks it against the stored words after the rollout).
// LP (the exact KL of the update needs the distribution that drew the sample, taken, greedy or forced action alike): logps [A], when
// given, receives every column's log-prob lg[j] - lse (-inf for a masked-out column; at the taken action the returned log-prob's
// expression with the same lse, so its bits); lse_out, when given, the branch's lse for a caller that stores the columns itself,
// behind its hand-over.  LP = false reads neither.
template <bool MK = false, bool LP = false>
__device__ __forceinline__ int etm_sample_branch(const float *lg, int A, float u, int forced, float *logp, unsigned long long m = 0,
                                                 float *logps = nullptr, float *lse_out = nullptr) {
  float mx = -INFINITY;
  for (int j = 0; j < A; ++j) mx = fmaxf(mx, etm_masked_logit<MK>(lg, j, m));
  float se = 0.f;
  for (int j = 0; j < A; ++j) se += expf(etm_masked_logit<MK>(lg, j, m) - mx);
  const float lse = mx + logf(se);
  int a = forced;
  if (a < 0) a = u < 0.f ? etm_branch_mode<MK>(lg, A, mx, m) : etm_sample_categorical<MK>(lg, A, lse, u, m);
  *logp = lg[a] - lse;
  if constexpr (LP) {
    if (logps)
      for (int j = 0; j < A; ++j) logps[j] = etm_masked_logit<MK>(lg, j, m) - lse;
    if (lse_out) *lse_out = lse;
  }
  return a;
}

// Every branch of worker w at step t: row = t * stage_W + w indexes the time-major [S, stage_W, B] uniform / forced / staging
// tables (B = 1: [S, stage_W]); actions and host_actions are [W, B].  The value (logit column sum(sizes)) is staged by the caller.
// MK: am points to THIS worker's mask word (any address space); MK = false never reads am.
// LP: st_logps [S, stage_W, total_a] next to st_actions receives the row's log-probs of every column of every branch (MK or not);
// or, for a caller that stores the columns itself behind its hand-over (st_logps == NULL), lse_out [B] receives the branches' lse.
// LP = false reads neither.
template <bool MK = false, bool LP = false>
__device__ __forceinline__ void etm_sample_branches(const float *lg, const EtmBranches &br, long long row, int w, const float *uniforms,
                                                    const long long *forced, long long *actions, long long *host_actions,
                                                    long long *st_actions, float *st_logp, const long long *am = nullptr,
                                                    float *st_logps = nullptr, int total_a = 0, float *lse_out = nullptr) {
  const int B = br.n;
  unsigned long long word = 0ull;
  if constexpr (MK) word = (unsigned long long)*am;
  int off = 0;
  for (int b = 0; b < B; ++b) {
    const long long i = row * B + b;
    const int Ab = br.size[b];
    float lp;
    const int fc = forced ? (int)forced[i] : -1;
    int a;
    if constexpr (LP)
      a = etm_sample_branch<MK, true>(lg + off, Ab, uniforms[i], fc, &lp, word >> off, st_logps ? st_logps + row * total_a + off : nullptr,
                                      lse_out ? lse_out + b : nullptr);
    else if constexpr (MK) a = etm_sample_branch<true>(lg + off, Ab, uniforms[i], fc, &lp, word >> off);
    else a = etm_sample_branch(lg + off, Ab, uniforms[i], fc, &lp);
    actions[(long long)w * B + b] = a;
    if (host_actions) host_actions[(long long)w * B + b] = a;
    st_actions[i] = a;
    st_logp[i] = lp;
    off += Ab;
  }
}

// One column's term of the exact categorical KL(old || new) (utils.categorical_kl is the host definition; the loss kernels sum it over
// a branch's valid columns): lo / l the column's old and current log-prob, pj = exp(l), d = lo - l.
// p_old (expm1(-d) + d) = p_old (lo - l) + (p - p_old): never negative beyond the rounding of the one expm1 + d, exactly 0 at d = 0,
// and no term of size 1 cancels (the added p - p_old sums to zero over a branch).  Below d = -60 (p_old -> 0, lo = -inf included) the
// limit p: the dropped part is under e^-60 |d|, and the case keeps inf * denormal out of the sum.
__device__ __forceinline__ float etm_categorical_kl_term(float lo, float l, float pj) {
  const float d = lo - l;
  return d >= -60.f ? expf(lo) * (expm1f(-d) + d) : pj;
}

// Box (continuous) action spaces: a diagonal Gaussian policy over A <= ETM_MAX_BOX dimensions, mean = the A policy-head outputs,
// sigma_a = exp(log_std[a]) (state-independent).  The environment's bounds travel with the launch by value (no device allocation,
// graph-capturable); the buffer keeps the raw draw, the host gets it clipped to [lo, hi].
constexpr int ETM_MAX_BOX = 8;
struct EtmBox {
  int A;
  float lo[ETM_MAX_BOX], hi[ETM_MAX_BOX];
};
// Host side: the bound table of A dimensions (lo / hi: HOST arrays; NULL = unbounded).  0, ETM_EINVAL or ETM_EUNSUPPORTED (A > 8).
static inline int etm_box_make(const float *lo, const float *hi, int A, EtmBox *out) {
  if (A <= 0) return ETM_EINVAL;
  if (A > ETM_MAX_BOX) return ETM_EUNSUPPORTED;
  out->A = A;
  for (int a = 0; a < ETM_MAX_BOX; ++a) {
    out->lo[a] = (lo && a < A) ? lo[a] : -INFINITY;
    out->hi[a] = (hi && a < A) ? hi[a] : INFINITY;
    if (a < A && !(out->lo[a] <= out->hi[a])) return ETM_EINVAL;
  }
  return 0;
}

// One Gaussian draw of worker w at step t (row = t * stage_W + w of the time-major tables) -- every sampling site of a Box policy:
// x_a = mu_a + sigma_a eps_a with eps = normals[0 .. A) (or the forced action forced[a] where it is not NaN), the joint log-prob
// log p(x) = sum_a [-(x_a - mu_a)^2 / (2 sigma_a^2) - log sigma_a - log(2 pi) / 2] of the stored x, staging of x ([S, stage_W, A]),
// log p and the value ([S, stage_W]); actions / host_actions [W, A] receive clip(x, lo, hi).  normals / forced / log_std: A floats.
// The mode of a Box policy needs no sentinel: a zero in the normals table stores x = mu + sigma * 0 = mu (the deterministic
// rollouts of the evaluator zero the table), and log p is then sum_a [(-0 - log sigma_a) - log(2 pi) / 2].
// MN: the means are staged too, st_means [S, stage_W, A] next to st_actions -- the policy's mu, forced action or not (the exact KL of
// the update needs the distribution that drew the sample); MN = false never reads st_means.
template <bool MN = false>
__device__ __forceinline__ void etm_sample_gaussian(const float *mu, const float *log_std, const EtmBox &bx, const float *normals,
                                                    const float *forced, float value, long long row, int w, float *actions,
                                                    float *host_actions, float *st_actions, float *st_logp, float *st_values,
                                                    float *st_means = nullptr) {
  const int A = bx.A;
  float lp = 0.f;
  for (int a = 0; a < A; ++a) {
    const float ls = log_std[a];
    const float sg = expf(ls);
    float x = forced ? forced[a] : NAN;
    if (x != x) x = mu[a] + sg * normals[a];
    const float z = (x - mu[a]) / sg;
    lp += (-0.5f * z * z - ls) - 0.918938533204672742f;
    const float c = fminf(fmaxf(x, bx.lo[a]), bx.hi[a]);
    actions[(long long)w * A + a] = c;
    if (host_actions) host_actions[(long long)w * A + a] = c;
    st_actions[row * A + a] = x;
    if constexpr (MN) st_means[row * A + a] = mu[a];
  }
  st_logp[row] = lp;
  st_values[row] = value;
}

// uint8 image observations: byte k stands for float(k) / 255.f CORRECTLY ROUNDED (what `obs.astype(np.float32) / 255.` computes on the
// host; k * (1 / 255.f) differs from it for 126 of the 256 bytes).  One definition for every kernel that reads bytes: the quotient estimate
// q = k y (y = the fp32 nearest to 1 / 255) and one residual correction, r = k - 255 q exactly (fma), q + r y rounded once -- the final
// step of a correctly rounded fp32 division without the scaling and fix-up a general divisor needs (v_cvt_f32_ubyteN + 3 operations; the
// host test checks this arithmetic against the quotient for all 256 bytes in exact rational arithmetic, the device test on the device).
__device__ __forceinline__ float etm_byte_unit(unsigned k) {
  constexpr float y = 1.f / 255.f;
  const float a = (float)k;
  const float q = a * y;
  const float r = __builtin_fmaf(-255.f, q, a);
  return __builtin_fmaf(r, y, q);
}
// the four bytes of a little-endian word (byte 0 = lowest address)
__device__ __forceinline__ f32x4 etm_bytes4_unit(unsigned w) {
  return f32x4{etm_byte_unit(w & 0xffu), etm_byte_unit((w >> 8) & 0xffu), etm_byte_unit((w >> 16) & 0xffu), etm_byte_unit(w >> 24)};
}

static inline int etm_launch_status() { return (int)hipGetLastError(); }

// ---- optional per-kernel timing with HIP events (see etm_profile_* in include/etm_hip.h); off by default.
enum EtmKernelId {
  ETM_K_LN_STATS = 0, ETM_K_MHA_FWD, ETM_K_BWD_SCORES, ETM_K_BWD_DW, ETM_K_BWD_REDUCE, ETM_K_BWD_UW, ETM_K_BWD_DX,
  ETM_K_GAE, ETM_K_ADV_STATS, ETM_K_PPO_LOSS, ETM_K_PPO_FINAL, ETM_K_ATTN_CACHED, ETM_K_RESET_ROWS,
  ETM_K_ROLLOUT_WINDOW, ETM_K_ROLLOUT_SAMPLE, ETM_K_ADD_LN, ETM_K_CONV_RELU, ETM_K_ROLLOUT_HEADS, ETM_K_GRU_GATE, ETM_K_WINDOW_FWD, ETM_K_WINDOW_BWD,
  ETM_K_LN_TRAIN_FWD, ETM_K_LN_TRAIN_BWD, ETM_K_COLSUM, ETM_K_GATE_TRAIN, ETM_K_OPTIM,
  ETM_K_CONV_TRAIN_FWD, ETM_K_CONV_TRAIN_DGRAD, ETM_K_CONV_TRAIN_WGRAD, ETM_K_ROLLOUT_FUSED,
  // the encoder passes per layer (kernel size 8 / 4 / 3 = layers 1 / 2 / 3 of model.py:29-31; other geometries keep the ids above)
  ETM_K_CONV_FWD_L1, ETM_K_CONV_FWD_L2, ETM_K_CONV_FWD_L3, ETM_K_CONV_DGRAD_L2, ETM_K_CONV_DGRAD_L3,
  ETM_K_CONV_WGRAD_L1, ETM_K_CONV_WGRAD_L2, ETM_K_CONV_WGRAD_L3, ETM_K_HIDDEN_PARTIAL, ETM_K_RELU_BWD_COLSUM, ETM_K_GATHER_ROWS, ETM_K_GROUPED_DW, ETM_K_BYTES_TO_UNIT,
  ETM_K_RUNNING_NORM,
  ETM_K_COUNT
};
// profile id of an encoder pass by layer (kernel size), falling back to the pass's generic id
static inline int etm_conv_layer_kid(int generic, int l1, int l2, int l3, int KH) { return KH == 8 ? (l1 >= 0 ? l1 : generic) : KH == 4 ? l2 : KH == 3 ? l3 : generic; }
// LayerNorm statistics of the gathered window rows (defined in mha_fwd.hip; shared by the dense and the folded attention).
int etm_launch_ln_stats(const float *bank, int64_t ep_stride, int64_t row_stride, const int64_t *ep, const int64_t *win,
                        const int64_t *pidx, const float *pos, float eps, float *stats, int N, int L, int D, hipStream_t st);
void etm_prof_begin(int kid, hipStream_t st);
void etm_prof_end(int kid, hipStream_t st);
struct EtmProfScope {
  int kid; hipStream_t st;
  EtmProfScope(int k, hipStream_t s) : kid(k), st(s) { etm_prof_begin(kid, st); }
  ~EtmProfScope() { etm_prof_end(kid, st); }
};
