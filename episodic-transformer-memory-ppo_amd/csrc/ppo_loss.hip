// Kernel #3: PPO clipped surrogate + clipped value loss + entropy bonus, forward and backward in one pass
// (replaces /root/reference trainer.py:276-304 and :315-316 for one action branch).
//
// Sample-parallel, coalesced; per-workgroup partial sums go to a scratch buffer and a one-workgroup finalize kernel
// produces the six statistics, so results are deterministic (no float atomics).  Tie handling of torch.min /
// torch.max (gradient split in half) and the inclusive range of torch.clamp's backward are reproduced.
// HBM traffic: 28 + 8 A bytes per sample.
#include "etm_common.h"
#include "adv_stats.h"

namespace {

__global__ __launch_bounds__(1024) void adv_stats_kernel(const float *__restrict__ adv, int N, float *__restrict__ stats3) {
  adv_stats_block_1024(N, stats3, [&](int i) { return adv[i]; });       // (adv_stats.h: shared with the step's head launch)
}

// Large N (the scaled micro-benchmark, data-parallel epochs at many workers): the one-workgroup kernel above reads at 6 GB/s
// (11 ms at 2^24 samples) -- here every workgroup takes a contiguous chunk, computes the chunk's own (count, mean, M2)
// with the same two passes (the second one re-reads the chunk from L2), and a one-workgroup kernel merges the chunks in a fixed tree
// (Chan et al.: M2 = sum M2_i + sum n_i (mean_i - mean)^2, in double).  Deterministic; N < ADV_STATS_SPLIT_MIN keeps the kernel above
// (bit-identical results at the minibatch sizes of the configs).
constexpr int ADV_STATS_CHUNK = 16384;
__global__ __launch_bounds__(1024) void adv_stats_part_kernel(const float *__restrict__ adv, int N, int per, float *__restrict__ partials) {
  __shared__ float red[16];
  __shared__ float mean_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long lo = (long long)blockIdx.x * per;
  const int n = (int)((lo + per <= N) ? per : (N > lo ? N - lo : 0));
  const float *a = adv + lo;
  float s = 0.f;
  for (int i = tid; i < n; i += 1024) s += a[i];
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    mean_s = n > 0 ? t / (float)n : 0.f;
  }
  __syncthreads();
  const float mean = mean_s;
  float m2 = 0.f;
  for (int i = tid; i < n; i += 1024) {
    const float d = a[i] - mean;
    m2 += d * d;
  }
  m2 = wave_sum(m2);
  __syncthreads();
  if (lane == 0) red[wave] = m2;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    partials[3 * blockIdx.x] = (float)n;
    partials[3 * blockIdx.x + 1] = mean;
    partials[3 * blockIdx.x + 2] = t;
  }
}
__global__ __launch_bounds__(1024) void adv_stats_merge_kernel(const float *__restrict__ partials, int nb, float *__restrict__ stats3) {
  __shared__ double sn[1024], sm[1024];
  const int tid = threadIdx.x;
  const double n = tid < nb ? (double)partials[3 * tid] : 0.0, mu = tid < nb ? (double)partials[3 * tid + 1] : 0.0;
  sn[tid] = n; sm[tid] = n * mu;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {                      // fixed tree: the same sums whatever the timing
    if (tid < o) { sn[tid] += sn[tid + o]; sm[tid] += sm[tid + o]; }
    __syncthreads();
  }
  const double N = sn[0], mean = sm[0] / sn[0];
  __syncthreads();
  sm[tid] = tid < nb ? (double)partials[3 * tid + 2] + n * (mu - mean) * (mu - mean) : 0.0;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) sm[tid] += sm[tid + o];
    __syncthreads();
  }
  if (tid == 0) { stats3[0] = (float)N; stats3[1] = (float)mean; stats3[2] = (float)sm[0]; }
}

struct LossParams {
  const float *logits;
  const long long *actions;
  long long action_stride;
  const float *old_logp;
  long long logp_stride;
  const float *adv, *old_value, *value, *adv_stats3;
  float clip, clip_lo, clip_hi, vf_coef, beta, pol_scale, ent_scale, val_scale;
  const double *dyn;   // optional device-resident (clip, beta): same arithmetic as the host-side scalars, read at run time
  int include_value;
  float *d_logits, *d_value, *partials;
  int N, A;
  // MK kernels (invalid-action masks): amask [N] int64 words, the branch's A actions at bits [mask_shift, mask_shift + A)
  const long long *amask;
  int mask_shift;
  // KL kernels (the exact categorical KL statistic): old_logps [N, row stride old_logps_stride], every column's log-prob under the policy
  // that drew the samples; the branch's A columns start at column logps_off of a row
  const float *old_logps;
  long long old_logps_stride;
  int logps_off;
  // PEN kernels (`kl_penalty`): one device float32, the coefficient of the KL term of the loss, read in place
  const float *kl_coef;
};

// SPT samples per thread.  SPT = 4 (large batches, unit strides, A = 3, N % 4 == 0): the four samples' operands come in as
// 16-byte loads (logits: three float4 = 12 floats; advantages, values, old log-probs: one float4 each; actions: two 16-byte
// loads) and the gradients leave the same way -- a quarter of the load / store instructions of the one-sample form, which
// is what bounds this kernel at large N (28 + 8 A = 52 bytes per sample against ~10 scalar memory instructions).
// MK (SPT = 1 only): invalid-action masks.  Log-sum-exp, log-prob and entropy run over the VALID actions only; an invalid action has
// p = 0, is skipped -- not multiplied: 0 * inf -- by the entropy, and its d logit is exactly 0.  What is left is the unmasked
// arithmetic on the compacted branch.
// KL (SPT = 1 only, MK or not): a sixth sum, the branch's exact KL(old || new) -- etm_categorical_kl_term over its valid columns, formed
// where l and pj already are -- into slot 5 of the workgroup's 8 partial floats.  A statistic only: no term of the loss, no gradient,
// unless `kl_penalty`.
// PEN (KL only; `kl_penalty`): the loss gains coef * K, K the exact KL as out8[4] holds it, coef = *kl_coef; a valid column's d logit
// gains coef pol_scale (p_j - p_old_j) (utils.categorical_kl_grad), an invalid one's stays exactly 0.  The term's p_j is
// exp((logit_j - max) - log(sum)), not the exp(logit_j - lse) of the other terms: logit_j - lse carries half a spacing of lse (2.4e-7 at
// lse = 4.3) into every p_j, which coef multiplies (a d logit of size 0.16 was off by 9.6e-7 at coef 7); the form here is exact at the
// largest column, as a float32 log-softmax is.  One more expf per column, in these kernels only.  With the sampler's rows of equal
// logits the term is therefore of rounding size, |p_j - p_old_j| <= p_j (a spacing of lse), not exactly 0 as in the fused kernels.
template <int SPT, bool MK, bool KL = false, bool PEN = false>
__device__ __forceinline__ void ppo_loss_body(const LossParams &p0) {
  static_assert(!PEN || (KL && SPT == 1), "the KL penalty needs the exact KL's operands");
  LossParams p = p0;
  if (p.dyn) {   // schedules that change between replays of a captured training step
    const double c = p.dyn[0];
    p.clip = (float)c; p.clip_lo = (float)(1.0 - c); p.clip_hi = (float)(1.0 + c);
    p.beta = (float)p.dyn[1];
  }
  constexpr int NK = KL ? 6 : 5;
  __shared__ float red[4][NK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (blockIdx.x * 256 + tid) * SPT;
  float acc[NK] = {0.f, 0.f, 0.f, 0.f, 0.f};  // policy, value, entropy, kl, clip fraction (KL: then the exact KL)
  float pen_pol = 0.f;
  if constexpr (PEN) pen_pol = p.kl_coef[0] * p.pol_scale;
  // operands of this thread's samples
  float lgv[SPT][SPT == 1 ? 1 : 3], advv[SPT], oldlp[SPT], vv[SPT], vov[SPT], dlv[SPT][SPT == 1 ? 1 : 3], dvv[SPT];
  int actv[SPT];
  if (SPT == 4 && n0 < p.N) {
    const f32x4 *lq = reinterpret_cast<const f32x4 *>(p.logits + (long long)n0 * 3);
    const f32x4 l0 = lq[0], l1 = lq[1], l2 = lq[2];
    const float flat[12] = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3], l2[0], l2[1], l2[2], l2[3]};
    const f32x4 a4 = *reinterpret_cast<const f32x4 *>(p.adv + n0), o4 = *reinterpret_cast<const f32x4 *>(p.old_logp + n0);
    const longlong2 c0 = *reinterpret_cast<const longlong2 *>(p.actions + n0), c1 = *reinterpret_cast<const longlong2 *>(p.actions + n0 + 2);
    const long long acts[4] = {c0.x, c0.y, c1.x, c1.y};
    f32x4 v4 = {0.f, 0.f, 0.f, 0.f}, vo4 = {0.f, 0.f, 0.f, 0.f};
    if (p.include_value) { v4 = *reinterpret_cast<const f32x4 *>(p.value + n0); vo4 = *reinterpret_cast<const f32x4 *>(p.old_value + n0); }
#pragma unroll
    for (int s = 0; s < SPT; ++s) {
#pragma unroll
      for (int j = 0; j < (SPT == 1 ? 1 : 3); ++j) lgv[s][j] = flat[(s * 3 + j) % 12];
      advv[s] = a4[s & 3]; oldlp[s] = o4[s & 3]; vv[s] = v4[s & 3]; vov[s] = vo4[s & 3]; actv[s] = (int)acts[s & 3];
    }
  }
#pragma unroll
  for (int s = 0; s < SPT; ++s) {
  const int n = n0 + s;
  if (n < p.N) {
    const int A = p.A;
    const float cnt = p.adv_stats3[0], mean = p.adv_stats3[1], m2 = p.adv_stats3[2];
    const float stdv = sqrtf(m2 / (cnt - 1.0f));            // torch.std: unbiased
    const float a_raw = SPT == 4 ? advv[s] : p.adv[n];
    const float a_n = (a_raw - mean) / (stdv + 1e-8f);
    float lgl[3];
    if (SPT == 4) { lgl[0] = lgv[s][0]; lgl[1] = lgv[s][SPT == 1 ? 0 : 1]; lgl[2] = lgv[s][SPT == 1 ? 0 : 2]; }
    const float *lg = SPT == 4 ? lgl : p.logits + (long long)n * A;
    unsigned long long am = ~0ull;
    if constexpr (MK) am = (unsigned long long)p.amask[n] >> p.mask_shift;
    auto ok = [&](int j) { return !MK || ((am >> j) & 1ull) != 0; };
    float mx = -INFINITY;
    for (int j = 0; j < A; ++j) if (ok(j)) mx = fmaxf(mx, lg[j]);
    float se = 0.f;
    for (int j = 0; j < A; ++j) if (ok(j)) se += expf(lg[j] - mx);
    const float lse = mx + logf(se);
    float log_se = 0.f;                                     // (PEN: the penalty's own log-probs, see above)
    if constexpr (PEN) log_se = logf(se);
    const int act = SPT == 4 ? actv[s] : (int)p.actions[(long long)n * p.action_stride];
    float lg_act = lg[0];
    if (SPT == 4) { lg_act = act == 1 ? lgl[1] : (act == 2 ? lgl[2] : lgl[0]); } else { lg_act = lg[act]; }
    const float lp = lg_act - lse;
    float ent = 0.f;
    for (int j = 0; j < A; ++j) {
      if (!ok(j)) continue;
      const float l = lg[j] - lse;
      ent -= expf(l) * l;
    }
    const float log_ratio = lp - (SPT == 4 ? oldlp[s] : p.old_logp[(long long)n * p.logp_stride]);
    const float ratio = expf(log_ratio);
    const bool in_range = (ratio >= p.clip_lo) && (ratio <= p.clip_hi);
    const float s1 = ratio * a_n;
    const float s2 = fminf(fmaxf(ratio, p.clip_lo), p.clip_hi) * a_n;
    acc[0] += fminf(s1, s2);
    float g_ratio;  // d min(s1, s2) / d ratio
    if (s1 < s2) g_ratio = a_n;
    else if (s1 > s2) g_ratio = in_range ? a_n : 0.f;
    else g_ratio = 0.5f * a_n + (in_range ? 0.5f * a_n : 0.f);
    acc[2] += ent;
    acc[3] += (ratio - 1.0f) - log_ratio;
    acc[4] += (fabsf(ratio - 1.0f) > p.clip) ? 1.f : 0.f;
    // d loss / d logits
    const float cpol = -p.pol_scale * g_ratio * ratio;
    const float cent = -p.beta * p.ent_scale;
    float *dl = p.d_logits + (long long)n * A;
    for (int j = 0; j < A; ++j) {
      if (!ok(j)) { dl[j] = 0.f; continue; }               // (MK only, i.e. SPT = 1)
      const float l = lg[j] - lse;
      const float pj = expf(l);
      const float d_lp = ((j == act) ? 1.f : 0.f) - pj;   // d log p[act] / d logit_j
      const float d_ent = -pj * (l + ent);                // d entropy / d logit_j
      float g = cpol * d_lp + cent * d_ent;
      if constexpr (PEN) g += pen_pol * (expf((lg[j] - mx) - log_se) - expf(p.old_logps[(long long)n * p.old_logps_stride + p.logps_off + j]));
      if (SPT == 4) dlv[s][SPT == 1 ? 0 : j] = g; else dl[j] = g;
      if constexpr (KL) acc[NK - 1] += etm_categorical_kl_term(p.old_logps[(long long)n * p.old_logps_stride + p.logps_off + j], l, pj);
    }
    if (p.include_value) {
      const float v = SPT == 4 ? vv[s] : p.value[n], vo = SPT == 4 ? vov[s] : p.old_value[n];
      const float ret = vo + a_raw;
      const float dv = v - vo;
      const bool in_v = (dv >= -p.clip) && (dv <= p.clip);
      const float vc = vo + fminf(fmaxf(dv, -p.clip), p.clip);
      const float e1 = v - ret, e2 = vc - ret;
      const float v1 = e1 * e1, v2 = e2 * e2;
      acc[1] += fmaxf(v1, v2);
      const float g2 = in_v ? 2.f * e2 : 0.f;
      float gv;
      if (v1 > v2) gv = 2.f * e1;
      else if (v1 < v2) gv = g2;
      else gv = e1 + 0.5f * g2;
      if (SPT == 4) dvv[s] = p.vf_coef * p.val_scale * gv; else p.d_value[n] = p.vf_coef * p.val_scale * gv;
    }
  }
  }
  if (SPT == 4 && n0 < p.N) {
    f32x4 *dq = reinterpret_cast<f32x4 *>(p.d_logits + (long long)n0 * 3);
    float flat[12];
#pragma unroll
    for (int s = 0; s < SPT; ++s)
#pragma unroll
      for (int j = 0; j < (SPT == 1 ? 1 : 3); ++j) flat[(s * 3 + j) % 12] = dlv[s][j];
    dq[0] = f32x4{flat[0], flat[1], flat[2], flat[3]};
    dq[1] = f32x4{flat[4], flat[5], flat[6], flat[7]};
    dq[2] = f32x4{flat[8], flat[9], flat[10], flat[11]};
    if (p.include_value) *reinterpret_cast<f32x4 *>(p.d_value + n0) = f32x4{dvv[0], dvv[SPT == 1 ? 0 : 1], dvv[SPT == 1 ? 0 : 2], dvv[SPT == 1 ? 0 : 3]};
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (tid < NK) p.partials[(long long)blockIdx.x * 8 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// The kernels: one body; the instantiations without masks keep their names, the masked one and the ones with the exact KL are kernels
// of their own.
template <int SPT>
__global__ __launch_bounds__(256) void ppo_loss_kernel(const LossParams p0) { ppo_loss_body<SPT, false>(p0); }
__global__ __launch_bounds__(256) void ppo_loss_masked_kernel(const LossParams p0) { ppo_loss_body<1, true>(p0); }
template <bool MK>
__global__ __launch_bounds__(256) void ppo_loss_kl_kernel(const LossParams p0) { ppo_loss_body<1, MK, true>(p0); }
template <bool MK>
__global__ __launch_bounds__(256) void ppo_loss_kl_penalty_kernel(const LossParams p0) { ppo_loss_body<1, MK, true, true>(p0); }

// KL: the sixth partial is the exact KL sum -> out8[4] (scaled as the k3 value, which goes to out8[6])
// PEN (`kl_penalty`, KL only): out8[2] gains coef * out8[4], out8[7] = coef = *kl_coef
template <bool KL, bool PEN = false>
__device__ __forceinline__ void ppo_finalize_body(const float *__restrict__ partials, int n_blocks, float vf_coef, float beta,
                                                  float pol_scale, float ent_scale, float val_scale, float *__restrict__ out8,
                                                  const double *__restrict__ dyn, const float *__restrict__ kl_coef = nullptr) {
  static_assert(!PEN || KL, "the KL penalty needs the exact KL");
  constexpr int NK = KL ? 6 : 5;
  const int lane = threadIdx.x;
  if (dyn) beta = (float)dyn[1];
  float acc[NK] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = lane; b < n_blocks; b += 64)
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] += partials[(long long)b * 8 + k];
#pragma unroll
  for (int k = 0; k < NK; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
    const float pol = acc[0] * pol_scale, val = acc[1] * val_scale, ent = acc[2] * ent_scale;
    out8[0] = pol;
    out8[1] = val;
    out8[2] = -(pol - vf_coef * val + beta * ent);
    out8[3] = ent;
    out8[4] = acc[KL ? 5 : 3] * pol_scale;
    out8[5] = acc[4] * pol_scale;
    out8[6] = KL ? acc[3] * pol_scale : 0.f;
    out8[7] = 0.f;
    if constexpr (PEN) {
      const float coef = kl_coef[0];
      out8[2] = -(pol - vf_coef * val + beta * ent) + coef * (acc[NK - 1] * pol_scale);
      out8[7] = coef;
    }
  }
}
__global__ __launch_bounds__(64) void ppo_finalize_kernel(const float *__restrict__ partials, int n_blocks, float vf_coef, float beta,
                                                          float pol_scale, float ent_scale, float val_scale, float *__restrict__ out8,
                                                          const double *__restrict__ dyn) {
  ppo_finalize_body<false>(partials, n_blocks, vf_coef, beta, pol_scale, ent_scale, val_scale, out8, dyn);
}
__global__ __launch_bounds__(64) void ppo_finalize_kl_kernel(const float *__restrict__ partials, int n_blocks, float vf_coef, float beta,
                                                             float pol_scale, float ent_scale, float val_scale, float *__restrict__ out8,
                                                             const double *__restrict__ dyn) {
  ppo_finalize_body<true>(partials, n_blocks, vf_coef, beta, pol_scale, ent_scale, val_scale, out8, dyn);
}
__global__ __launch_bounds__(64) void ppo_finalize_kl_penalty_kernel(const float *__restrict__ partials, int n_blocks, float vf_coef, float beta,
                                                                     float pol_scale, float ent_scale, float val_scale,
                                                                     float *__restrict__ out8, const double *__restrict__ dyn,
                                                                     const float *__restrict__ kl_coef) {
  ppo_finalize_body<true, true>(partials, n_blocks, vf_coef, beta, pol_scale, ent_scale, val_scale, out8, dyn, kl_coef);
}
}  // namespace

extern "C" int etm_adv_stats(const float *adv, int N, float *stats3, void *stream) {
  (void)hipGetLastError();  // drop stale sticky errors of earlier, unrelated runtime calls
  if (!adv || !stats3 || N <= 0) return ETM_EINVAL;
  EtmProfScope prof(ETM_K_ADV_STATS, (hipStream_t)stream);
  hipLaunchKernelGGL(adv_stats_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, adv, N, stats3);
  return etm_launch_status();
}

extern "C" int64_t etm_adv_stats_workspace_bytes(int N) {
  if (N < ETM_ADV_STATS_SPLIT_MIN) return 0;
  const int nb = (N + ADV_STATS_CHUNK - 1) / ADV_STATS_CHUNK;
  return (int64_t)(nb < 1024 ? nb : 1024) * 3 * sizeof(float);
}
// As etm_adv_stats, over many workgroups when N >= ETM_ADV_STATS_SPLIT_MIN and a workspace of etm_adv_stats_workspace_bytes(N) bytes is
// given (else the one-workgroup kernel: the same results as etm_adv_stats bit for bit).
extern "C" int etm_adv_stats_ws(const float *adv, int N, float *stats3, void *workspace, int64_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (!adv || !stats3 || N <= 0) return ETM_EINVAL;
  const int64_t need = etm_adv_stats_workspace_bytes(N);
  if (need == 0 || !workspace) return etm_adv_stats(adv, N, stats3, stream);
  if (workspace_bytes < need) return ETM_EWORKSPACE;
  int nb = (N + ADV_STATS_CHUNK - 1) / ADV_STATS_CHUNK;
  if (nb > 1024) nb = 1024;
  const int per = (int)((((long long)N + nb - 1) / nb + 3) & ~3LL);
  nb = (int)(((long long)N + per - 1) / per);
  EtmProfScope prof(ETM_K_ADV_STATS, (hipStream_t)stream);
  hipLaunchKernelGGL(adv_stats_part_kernel, dim3(nb), dim3(1024), 0, (hipStream_t)stream, adv, N, per, (float *)workspace);
  hipLaunchKernelGGL(adv_stats_merge_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float *)workspace, nb, stats3);
  return etm_launch_status();
}

extern "C" int64_t etm_ppo_loss_workspace_bytes(int N) { return N <= 0 ? 0 : (int64_t)((N + 255) / 256) * 8 * sizeof(float); }
static bool al16(const void *q) { return ((uintptr_t)q % 16) == 0; }
namespace {
// One call of any of the four entries: the kernels' operands by name (what an entry does not take stays NULL / 0), what only the host needs,
// and what the entry takes: a mandatory action_mask (the exact-KL entries take one or NULL) | old_logps, its stride and offset | kl_coef
struct PlCall {
  LossParams p{};
  double clip = 0;
  float *out8 = nullptr;
  int64_t partials_bytes = 0;
  void *stream = nullptr;
  bool need_mask = false, kl = false, pen = false;
};
// a record `c` with the arguments that all four entries name alike
#define PL_CALL(c)                                                                                                                         \
  PlCall c;                                                                                                                                \
  c.p.logits = logits; c.p.actions = (const long long *)actions; c.p.action_stride = action_stride; c.p.old_logp = old_logp;              \
  c.p.logp_stride = logp_stride; c.p.adv = adv; c.p.old_value = old_value; c.p.value = value; c.p.adv_stats3 = adv_stats3; c.clip = clip; \
  c.p.vf_coef = vf_coef; c.p.beta = beta; c.p.pol_scale = pol_scale; c.p.ent_scale = ent_scale; c.p.val_scale = val_scale;                \
  c.p.include_value = include_value; c.out8 = out8; c.p.d_logits = d_logits; c.p.d_value = d_value; c.p.partials = (float *)partials;     \
  c.partials_bytes = partials_bytes; c.p.dyn = dyn_clip_beta; c.p.N = N; c.p.A = A; c.stream = stream
// Every refusal of every entry, in the one order that include/etm_hip.h states ("Refusals of the loss entries").
int pl_validate(const PlCall &c) {
  const LossParams &p = c.p;
  if (c.pen && (!p.kl_coef || ((uintptr_t)p.kl_coef & 3u))) return ETM_EINVAL;
  if (c.kl && (!p.old_logps || ((uintptr_t)p.old_logps & 3u) || p.logps_off < 0 || p.old_logps_stride < (int64_t)p.logps_off + p.A)) return ETM_EINVAL;
  if (c.need_mask && !p.amask) return ETM_EINVAL;
  if (!p.logits || !p.actions || !p.old_logp || !p.adv || !p.adv_stats3 || !c.out8 || !p.d_logits || !p.partials) return ETM_EINVAL;
  if (p.include_value && (!p.old_value || !p.value || !p.d_value)) return ETM_EINVAL;
  if (p.N <= 0 || p.A <= 0) return ETM_EINVAL;
  if (p.amask && (p.mask_shift < 0 || p.mask_shift + p.A > 63)) return ETM_EUNSUPPORTED;
  if (const int rc = etm_action_mask_check(p.amask, p.A)) return rc;
  if (c.partials_bytes < etm_ppo_loss_workspace_bytes(p.N)) return ETM_EWORKSPACE;
  return c.pen && !c.kl ? ETM_EINVAL : 0;      // (no entry fills the record like this)
}
// The one launcher: validate, the pass, the finalisation.
int pl_launch(PlCall &c) {
  (void)hipGetLastError();  // drop stale sticky errors of earlier, unrelated runtime calls
  if (const int rc = pl_validate(c)) return rc;
  LossParams &p = c.p;
  p.clip = (float)c.clip; p.clip_lo = (float)(1.0 - c.clip); p.clip_hi = (float)(1.0 + c.clip);
  const bool masked = p.amask != nullptr;
  // four samples per thread when every operand can move in 16-byte pieces and there are enough samples to fill the chip (the exact KL:
  // always the one-sample form)
  const bool vec = !c.kl && !masked && p.A == 3 && p.N % 4 == 0 && p.N >= (1 << 16) && p.action_stride == 1 && p.logp_stride == 1 &&
                   al16(p.logits) && al16(p.actions) && al16(p.old_logp) && al16(p.adv) && al16(p.d_logits) &&
                   (!p.include_value || (al16(p.value) && al16(p.old_value) && al16(p.d_value)));
  const int nb = vec ? (p.N / 4 + 255) / 256 : (p.N + 255) / 256;
  // [plain, exact KL, penalty][masked]; the four-sample form is the plain kernel's only
  static constexpr void (*pass[3][2])(const LossParams) = {{ppo_loss_kernel<1>, ppo_loss_masked_kernel},
                                                           {ppo_loss_kl_kernel<false>, ppo_loss_kl_kernel<true>},
                                                           {ppo_loss_kl_penalty_kernel<false>, ppo_loss_kl_penalty_kernel<true>}};
  const auto kernel = vec ? ppo_loss_kernel<4> : pass[c.pen ? 2 : c.kl ? 1 : 0][masked];
  hipStream_t st = (hipStream_t)c.stream;
  {
    EtmProfScope prof(ETM_K_PPO_LOSS, st);
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, st, p);
  }
  if (const int rc = etm_launch_status()) return rc;
  EtmProfScope prof(ETM_K_PPO_FINAL, st);
  const auto finalize = c.kl ? ppo_finalize_kl_kernel : ppo_finalize_kernel;
  if (c.pen)
    hipLaunchKernelGGL(ppo_finalize_kl_penalty_kernel, dim3(1), dim3(64), 0, st, (const float *)p.partials, nb, p.vf_coef, p.beta, p.pol_scale,
                       p.ent_scale, p.val_scale, c.out8, p.dyn, p.kl_coef);
  else
    hipLaunchKernelGGL(finalize, dim3(1), dim3(64), 0, st, (const float *)p.partials, nb, p.vf_coef, p.beta, p.pol_scale, p.ent_scale,
                       p.val_scale, c.out8, p.dyn);
  return etm_launch_status();
}
}  // namespace
// The entries (include/etm_hip.h documents each): fill the record by name, say what the entry takes, launch.
extern "C" int etm_ppo_loss(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp,
                            int64_t logp_stride, const float *adv, const float *old_value, const float *value,
                            const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                            float val_scale, int include_value, float *out8, float *d_logits, float *d_value, void *partials,
                            int64_t partials_bytes, const double *dyn_clip_beta, int N, int A, void *stream) {
  PL_CALL(c);
  return pl_launch(c);
}
// Invalid-action masks: the branch's A actions are bits [mask_shift, mask_shift + A) of the samples' words action_mask [N]
extern "C" int etm_ppo_loss_masked(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp,
                                   int64_t logp_stride, const float *adv, const float *old_value, const float *value,
                                   const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                   float val_scale, int include_value, float *out8, float *d_logits, float *d_value, void *partials,
                                   int64_t partials_bytes, const double *dyn_clip_beta, int N, int A, const int64_t *action_mask,
                                   int mask_shift, void *stream) {
  PL_CALL(c);
  c.p.amask = (const long long *)action_mask; c.p.mask_shift = mask_shift; c.need_mask = true;
  return pl_launch(c);
}
// The exact categorical KL: action_mask optional (NULL: mask_shift is ignored) and old_logps, the branch's A columns from logps_off on
extern "C" int etm_ppo_loss_kl(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp,
                               int64_t logp_stride, const float *adv, const float *old_value, const float *value,
                               const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                               float val_scale, int include_value, float *out8, float *d_logits, float *d_value, void *partials,
                               int64_t partials_bytes, const double *dyn_clip_beta, int N, int A, const int64_t *action_mask,
                               int mask_shift, const float *old_logps, int64_t old_logps_stride, int logps_off, void *stream) {
  PL_CALL(c);
  c.p.amask = (const long long *)action_mask; c.p.mask_shift = action_mask ? mask_shift : 0;
  c.p.old_logps = old_logps; c.p.old_logps_stride = old_logps_stride; c.p.logps_off = logps_off; c.kl = true;
  return pl_launch(c);
}
// `kl_penalty`: etm_ppo_loss_kl with the loss L + coef * K of the branch, K = out8[4], coef = *kl_coef, ONE device float32 read in place
extern "C" int etm_ppo_loss_kl_penalty(const float *logits, const int64_t *actions, int64_t action_stride, const float *old_logp,
                                       int64_t logp_stride, const float *adv, const float *old_value, const float *value,
                                       const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                       float val_scale, int include_value, float *out8, float *d_logits, float *d_value, void *partials,
                                       int64_t partials_bytes, const double *dyn_clip_beta, int N, int A, const int64_t *action_mask,
                                       int mask_shift, const float *old_logps, int64_t old_logps_stride, int logps_off, const float *kl_coef,
                                       void *stream) {
  PL_CALL(c);
  c.p.amask = (const long long *)action_mask; c.p.mask_shift = action_mask ? mask_shift : 0;
  c.p.old_logps = old_logps; c.p.old_logps_stride = old_logps_stride; c.p.logps_off = logps_off; c.kl = true; c.p.kl_coef = kl_coef; c.pen = true;
  return pl_launch(c);
}
#undef PL_CALL
