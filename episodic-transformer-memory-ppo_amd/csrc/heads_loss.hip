// Policy / value heads + PPO loss of the optimisation step, forward AND backward, as one pass over the minibatch
// (/root/reference model.py:101-110 -- ReLU of the two hidden heads, the policy branch, the value head -- under trainer.py:276-304,
// :315-316 and the start of `loss.backward()`, trainer.py:310).
//
// Between the transformer output h [N, D] and the loss sit two hidden layers (library GEMMs, kept) and then only per-sample
// arithmetic: bias + ReLU of the hidden heads, A + 1 dot products of `hid` elements (logits, value), the loss terms of
// csrc/ppo_loss.hip and -- because the loss is a sum over samples -- their gradients straight away: d loss / d logits, d value,
// back through the two output heads and the ReLU masks to the pre-activations of the hidden heads.  As framework ops that is ~25
// launches of ~5 us on 2048 x 384 floats (183 us of the 2.17 ms minibatch step); here it is ONE launch plus one reduction launch:
//
//   one wave per sample; lane l holds columns l, l + 64, ... of the two hidden rows
//   hp = relu(pre_p + b_lp), hv = relu(pre_v + b_lv);  logits[a] = hp . Wb[a] + bb[a];  value = hv . wv + bv      (wave sums, DPP)
//   loss terms, statistics and d logits / d value exactly as ppo_loss_kernel (same expressions, same tie rules)
//   gm_p = (sum_a d logits[a] Wb[a]) * (hp > 0),  gm_v = d value * wv * (hv > 0)        -> written [N, hid] each: the gradients of
//                                                                                           the hidden heads' pre-activations
//   per-lane running sums over the wave's samples of: gm_p, gm_v (bias gradients of lin_policy / lin_value), d logits[a] * hp
//   (policy-branch weight gradient), d value * hv (value-head weight gradient), d logits, d value (their bias gradients)
//   -> the four waves are added in LDS, every workgroup writes ONE partial row; heads_reduce_kernel sums the rows in a fixed order
//      (deterministic) and produces the six loss statistics.
#include "etm_common.h"

namespace {
constexpr int HL_MAXA = 8;             // actions of the policy (all branches together)
constexpr int HL_MAXC = 8;             // hidden columns per lane (hid <= 512)

struct HlParams {
  const float *pre_p, *pre_v;          // [N, hid]: h Wlp^T, h Wlv^T (no bias)
  const float *b_lp, *b_lv;            // [hid]
  const float *wb, *bb;                // policy branch [A, hid], [A]
  const float *wv, *bv;                // value head [hid], [1]
  const long long *actions;            // [N] (stride in elements)
  long long action_stride;
  const float *old_logp;
  long long logp_stride;
  const float *adv, *old_value, *adv_stats3;
  float clip, clip_lo, clip_hi, vf_coef, beta, pol_scale, ent_scale, val_scale;
  const double *dyn;                   // optional device-resident (clip, beta)
  float *gm_p, *gm_v;                  // [N, hid]
  float *logits, *value;               // optional outputs [N, A], [N]
  float *partials;                     // [n_wg][row]: row = (3 + A) * hid floats (sum gm_p | sum gm_v | d wv | d Wb[a] ...) + A + 1 + 5
  int N, A, hid, samples_per_wg;
  // BR kernels (MultiDiscrete): nbr branches; column j of the A logits belongs to branch col_branch[j], which starts at column
  // branch_off[col_branch[j]]; actions / old_logp rows hold one entry per branch
  int nbr;
  int col_branch[HL_MAXA];
  int branch_off[HL_MAXA];
  // GS kernels (Box): the A logits are the means; xact [N, A] (row stride action_stride) the stored raw actions, log_std [A]
  const float *xact, *log_std;
  // MK kernels (invalid-action masks): amask [N] int64, bit j of a sample's word = column j of the A logits was allowed when the
  // sample was drawn
  const long long *amask;
  // KL kernels (Box, the exact KL statistic): old_mean [N, A] (row stride old_mean_stride floats) the means of the policy that drew the
  // samples, old_log_std [A] its log sigma
  const float *old_mean, *old_log_std;
  long long old_mean_stride;
  // KL kernels (categorical, the exact KL statistic): old_logps [N, A] (row stride old_logps_stride floats) every column's log-prob
  // under the policy that drew the samples (-inf at a column that was masked out)
  const float *old_logps;
  long long old_logps_stride;
  // PEN kernels (`kl_penalty`): one device float32, the coefficient of the KL term of the loss, read in place by every launch
  const float *kl_coef;
};

// BR: MultiDiscrete branches; GS: diagonal Gaussian (Box; the row gains d log_std [A] behind the five statistic sums)
// MK: invalid-action masks (BR or not).  A branch's log-sum-exp, log-probs and entropy run over its VALID columns only (ok(j)); an
// invalid column has p = 0, is skipped -- not multiplied: 0 * inf -- by the entropy, and its d logit is exactly 0.  The logit dot
// products and the optional logits output stay raw.  What is left is the unmasked arithmetic on the compacted branch.
// KL (GS only): a sixth running sum, the exact KL(old || new) of the two diagonal Gaussians,
//   KL_n = sum_a [(expm1(2 d_a) / 2 - d_a) + ((mu_old[n, a] - mu[n, a]) / sigma_a)^2 / 2],  d_a = log sigma_old_a - log sigma_a,
// written so that nothing cancels (equal policies give exactly 0).  A statistic only: no term of the loss, no gradient, unless
// `kl_penalty` (PEN, below); the sum sits behind d log_std at the very end of the row, so every other row offset keeps its value.
// KL (categorical, BR and MK or not): the sixth running sum is the exact KL of the two categoricals, per branch the sum over its VALID
// columns of etm_categorical_kl_term(old_logps[n, j], l_j, p_j), formed where l_j and p_j already are; it sits behind the five statistic
// sums at the very end of the row.  Again a statistic only, unless `kl_penalty`.
// PEN (KL only; `kl_penalty`): the loss gains coef * K, K the exact KL as out8[4] holds it, coef = *kl_coef read in place.  Its gradient
// joins d logits where l_j, p_j, mu_a, sigma_a already are (utils.categorical_kl_grad / gaussian_kl_grad are the host definitions):
//   categorical   dl[j] += coef pol_scale (p_j - p_old_j) inside the ok(j) guard (an invalid column's d logit stays exactly 0)
//   Box           dl[a] += coef ent_scale (-q / sigma_a), q = (mu_old - mu) / sigma_a; lane 0 adds coef ent_scale (-expm1(2 d_a) - q^2)
//                 to d log_std[a], the expm1 part formed once per lane, where kl_ls is
// Equal policies add exactly 0 to every gradient; the row layout is the KL kernels'.
template <int HC, bool BR, bool GS, bool MK, bool KL = false, bool PEN = false>
__device__ __forceinline__ void heads_loss_body(const HlParams &p0) {
  static_assert(!PEN || KL, "the KL penalty needs the exact KL's operands");
  HlParams p = p0;
  if (p.dyn) {
    const double c = p.dyn[0];
    p.clip = (float)c; p.clip_lo = (float)(1.0 - c); p.clip_hi = (float)(1.0 + c);
    p.beta = (float)p.dyn[1];
  }
  extern __shared__ float hl_lds[];                                  // [4 waves][row]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = p.A, hid = p.hid;
  // this lane's columns of the small operands
  float blp[HC], blv[HC], wvr[HC], wbr[HL_MAXA][HC];
#pragma unroll
  for (int c = 0; c < HC; ++c) {
    const int k = lane + 64 * c;
    blp[c] = p.b_lp[k]; blv[c] = p.b_lv[k]; wvr[c] = p.wv[k];
#pragma unroll
    for (int a = 0; a < HL_MAXA; ++a) wbr[a][c] = (a < A) ? p.wb[(long long)a * hid + k] : 0.f;
  }
  float bbr[HL_MAXA];
#pragma unroll
  for (int a = 0; a < HL_MAXA; ++a) bbr[a] = (a < A) ? p.bb[a] : 0.f;
  // GS: log sigma, sigma and the entropy sum_a (1/2 + log(2 pi) / 2 + log sigma_a) (the same for every sample); d log sigma sums
  float lsr[HL_MAXA], sgr[HL_MAXA], s_ls[HL_MAXA], ent_gs = 0.f;
  if constexpr (GS) {
#pragma unroll
    for (int a = 0; a < HL_MAXA; ++a) {
      lsr[a] = (a < A) ? p.log_std[a] : 0.f;
      sgr[a] = expf(lsr[a]);
      s_ls[a] = 0.f;
      if (a < A) ent_gs += (0.5f + 0.918938533204672742f) + lsr[a];
    }
  }
  // KL: the part of KL_n that does not depend on the sample (GS), and the sixth sum
  float kl_ls = 0.f, acc_kl = 0.f;
  if constexpr (KL && GS) {
#pragma unroll
    for (int a = 0; a < HL_MAXA; ++a)
      if (a < A) { const float d = p.old_log_std[a] - lsr[a]; kl_ls += 0.5f * expm1f(2.f * d) - d; }
  }
  // PEN: the coefficient times the scale of K, and (GS) the part of d K / d log sigma_a that does not depend on the sample
  float pen_pol = 0.f, pen_ent = 0.f, pen_ls[HL_MAXA];
  if constexpr (PEN) {
    const float coef = p.kl_coef[0];
    pen_pol = coef * p.pol_scale; pen_ent = coef * p.ent_scale;
    if constexpr (GS) {
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a) pen_ls[a] = (a < A) ? pen_ent * -expm1f(2.f * (p.old_log_std[a] - lsr[a])) : 0.f;
    }
  }
  const float bvr = p.bv[0];
  const float cnt = p.adv_stats3[0], mean = p.adv_stats3[1], m2 = p.adv_stats3[2];
  const float stdv = sqrtf(m2 / (cnt - 1.0f));                       // torch.std: unbiased
  // running sums of this lane
  float s_gp[HC], s_gv[HC], s_wv[HC], s_wb[HL_MAXA][HC], s_bb[HL_MAXA], s_bv = 0.f, acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < HC; ++c) {
    s_gp[c] = s_gv[c] = s_wv[c] = 0.f;
#pragma unroll
    for (int a = 0; a < HL_MAXA; ++a) s_wb[a][c] = 0.f;
  }
#pragma unroll
  for (int a = 0; a < HL_MAXA; ++a) s_bb[a] = 0.f;

  constexpr int PER_WAVE = 2;                                        // = HL_SAMPLES_PER_WG / 4
  const int n_begin = blockIdx.x * p.samples_per_wg + wave * PER_WAVE;
  // the rows of both samples are requested before the first one is worked on (a sample is a chain of dependent wave reductions)
  float pre_p_r[PER_WAVE][HC], pre_v_r[PER_WAVE][HC];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int n = min(n_begin + i, p.N - 1);
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const int k = lane + 64 * c;
      pre_p_r[i][c] = p.pre_p[(long long)n * hid + k];
      pre_v_r[i][c] = p.pre_v[(long long)n * hid + k];
    }
  }
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int n = n_begin + i;
    if (n >= p.N) break;                                             // (wave-uniform)
    float hp[HC], hv[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      hp[c] = fmaxf(pre_p_r[i][c] + blp[c], 0.f);
      hv[c] = fmaxf(pre_v_r[i][c] + blv[c], 0.f);
    }
    float lg[HL_MAXA];
#pragma unroll
    for (int a = 0; a < HL_MAXA; ++a) {
      lg[a] = 0.f;
      if (a < A) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < HC; ++c) d += hp[c] * wbr[a][c];
        lg[a] = wave_sum(d) + bbr[a];
      }
    }
    float dv_dot = 0.f;
#pragma unroll
    for (int c = 0; c < HC; ++c) dv_dot += hv[c] * wvr[c];
    const float v = wave_sum(dv_dot) + bvr;
    if (p.logits) {
#pragma unroll
      for (int j = 0; j < HL_MAXA; ++j) if (j < A && lane == j) p.logits[(long long)n * A + j] = lg[j];
    }
    if (p.value && lane == 0) p.value[n] = v;

    // ---- loss terms and their gradients: the expressions of ppo_loss_kernel (one sample, evaluated redundantly by every lane)
    const float a_raw = p.adv[n];
    const float a_n = (a_raw - mean) / (stdv + 1e-8f);
    float dl[HL_MAXA];
    unsigned long long am = ~0ull;
    if constexpr (MK) am = (unsigned long long)p.amask[n];
    auto ok = [&](int j) { return !MK || ((am >> j) & 1ull) != 0; };
    if constexpr (GS) {
      // Box (diagonal Gaussian): log p(x) = sum_a [-z_a^2 / 2 - log sigma_a - log(2 pi) / 2], z_a = (x_a - mu_a) / sigma_a, of the
      // stored raw action x; one ratio per sample, the surrogate's per-sample factor cpol = d loss / d log p as in the other modes;
      // d log p / d mu_a = z_a / sigma_a, d log p / d log sigma_a = z_a^2 - 1, and the entropy adds cent to every d log sigma_a
      float zr[HL_MAXA];
      float lp = 0.f;
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a) {
        zr[a] = 0.f;
        if (a < A) {
          const float x = p.xact[(long long)n * p.action_stride + a];
          zr[a] = (x - lg[a]) / sgr[a];
          lp += (-0.5f * zr[a] * zr[a] - lsr[a]) - 0.918938533204672742f;
        }
      }
      const float log_ratio = lp - p.old_logp[(long long)n * p.logp_stride];
      const float ratio = expf(log_ratio);
      const bool in_range = (ratio >= p.clip_lo) && (ratio <= p.clip_hi);
      const float s1 = ratio * a_n;
      const float s2 = fminf(fmaxf(ratio, p.clip_lo), p.clip_hi) * a_n;
      float g_ratio;
      if (s1 < s2) g_ratio = a_n;
      else if (s1 > s2) g_ratio = in_range ? a_n : 0.f;
      else g_ratio = 0.5f * a_n + (in_range ? 0.5f * a_n : 0.f);
      if (lane == 0) {
        acc[0] += fminf(s1, s2);
        acc[2] += ent_gs;
        acc[3] += (ratio - 1.0f) - log_ratio;
        acc[4] += (fabsf(ratio - 1.0f) > p.clip) ? 1.f : 0.f;
      }
      const float cpol = -p.pol_scale * g_ratio * ratio;
      const float cent = -p.beta * p.ent_scale;
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a) {
        dl[a] = 0.f;
        if (a < A) {
          dl[a] = cpol * (zr[a] / sgr[a]);
          if (lane == 0) s_ls[a] += cpol * (zr[a] * zr[a] - 1.f) + cent;
        }
      }
      if constexpr (KL) {
        float kq = 0.f;
#pragma unroll
        for (int a = 0; a < HL_MAXA; ++a)
          if (a < A) {
            const float q = (p.old_mean[(long long)n * p.old_mean_stride + a] - lg[a]) / sgr[a];
            kq += 0.5f * q * q;
            if constexpr (PEN) {
              dl[a] += pen_ent * (-q / sgr[a]);
              if (lane == 0) s_ls[a] += pen_ls[a] - pen_ent * (q * q);
            }
          }
        if (lane == 0) acc_kl += kl_ls + kq;
      }
    } else if constexpr (!BR) {
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < HL_MAXA; ++j) if (j < A && ok(j)) mx = fmaxf(mx, lg[j]);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < HL_MAXA; ++j) if (j < A && ok(j)) se += expf(lg[j] - mx);
    const float lse = mx + logf(se);
    const int act = (int)p.actions[(long long)n * p.action_stride];
    float lg_act = 0.f;
#pragma unroll
    for (int j = 0; j < HL_MAXA; ++j) if (j == act) lg_act = lg[j];
    const float lp = lg_act - lse;
    float ent = 0.f;
#pragma unroll
    for (int j = 0; j < HL_MAXA; ++j) if (j < A && ok(j)) { const float l = lg[j] - lse; ent -= expf(l) * l; }
    const float log_ratio = lp - p.old_logp[(long long)n * p.logp_stride];
    const float ratio = expf(log_ratio);
    const bool in_range = (ratio >= p.clip_lo) && (ratio <= p.clip_hi);
    const float s1 = ratio * a_n;
    const float s2 = fminf(fmaxf(ratio, p.clip_lo), p.clip_hi) * a_n;
    float g_ratio;
    if (s1 < s2) g_ratio = a_n;
    else if (s1 > s2) g_ratio = in_range ? a_n : 0.f;
    else g_ratio = 0.5f * a_n + (in_range ? 0.5f * a_n : 0.f);
    if (lane == 0) {
      acc[0] += fminf(s1, s2);
      acc[2] += ent;
      acc[3] += (ratio - 1.0f) - log_ratio;
      acc[4] += (fabsf(ratio - 1.0f) > p.clip) ? 1.f : 0.f;
    }
    const float cpol = -p.pol_scale * g_ratio * ratio;
    const float cent = -p.beta * p.ent_scale;
    float kl_n = 0.f;
#pragma unroll
    for (int j = 0; j < HL_MAXA; ++j) {
      dl[j] = 0.f;
      if (j < A && ok(j)) {
        const float l = lg[j] - lse;
        const float pj = expf(l);
        const float d_lp = ((j == act) ? 1.f : 0.f) - pj;
        const float d_ent = -pj * (l + ent);
        dl[j] = cpol * d_lp + cent * d_ent;
        if constexpr (KL) {
          const float lo = p.old_logps[(long long)n * p.old_logps_stride + j];
          kl_n += etm_categorical_kl_term(lo, l, pj);
          if constexpr (PEN) dl[j] += pen_pol * (pj - expf(lo));
        }
      }
    }
    if constexpr (KL) { if (lane == 0) acc_kl += kl_n; }
    } else {
      // MultiDiscrete (ref_algo.ppo_loss): per branch b a log-softmax over its own columns and a ratio; the sample's normalised
      // advantage is repeated over the branches; policy term, KL and clip fraction are summed over (sample, branch) and scaled by
      // pol_scale = 1 / (N B); the entropy is the sum of the branches' entropies (scaled by 1 / N).  Every branch-indexed array
      // is indexed by unrolled constants only (registers, no scratch).
      float lse_c[HL_MAXA], ent_c[HL_MAXA], cpol_c[HL_MAXA];
      int act_col[HL_MAXA];
#pragma unroll
      for (int b = 0; b < HL_MAXA; ++b) {
        act_col[b] = -1;
        if (b < p.nbr) {
          float mx = -INFINITY;
#pragma unroll
          for (int j = 0; j < HL_MAXA; ++j) if (j < A && p.col_branch[j] == b && ok(j)) mx = fmaxf(mx, lg[j]);
          float se = 0.f;
#pragma unroll
          for (int j = 0; j < HL_MAXA; ++j) if (j < A && p.col_branch[j] == b && ok(j)) se += expf(lg[j] - mx);
          const float lse = mx + logf(se);
          const int ac = p.branch_off[b] + (int)p.actions[(long long)n * p.action_stride + b];
          float lg_act = 0.f, ent = 0.f;
#pragma unroll
          for (int j = 0; j < HL_MAXA; ++j) {
            if (j == ac) lg_act = lg[j];
            if (j < A && p.col_branch[j] == b && ok(j)) { const float l = lg[j] - lse; ent -= expf(l) * l; }
          }
          const float lp = lg_act - lse;
          const float log_ratio = lp - p.old_logp[(long long)n * p.logp_stride + b];
          const float ratio = expf(log_ratio);
          const bool in_range = (ratio >= p.clip_lo) && (ratio <= p.clip_hi);
          const float s1 = ratio * a_n;
          const float s2 = fminf(fmaxf(ratio, p.clip_lo), p.clip_hi) * a_n;
          float g_ratio;
          if (s1 < s2) g_ratio = a_n;
          else if (s1 > s2) g_ratio = in_range ? a_n : 0.f;
          else g_ratio = 0.5f * a_n + (in_range ? 0.5f * a_n : 0.f);
          if (lane == 0) {
            acc[0] += fminf(s1, s2);
            acc[2] += ent;
            acc[3] += (ratio - 1.0f) - log_ratio;
            acc[4] += (fabsf(ratio - 1.0f) > p.clip) ? 1.f : 0.f;
          }
          act_col[b] = ac;
          const float cpol = -p.pol_scale * g_ratio * ratio;
#pragma unroll
          for (int j = 0; j < HL_MAXA; ++j)
            if (j < A && p.col_branch[j] == b) { lse_c[j] = lse; ent_c[j] = ent; cpol_c[j] = cpol; }
        }
      }
      const float cent = -p.beta * p.ent_scale;
      float kl_n = 0.f;                                               // (KL: the branches' KLs of this sample, column order)
#pragma unroll
      for (int j = 0; j < HL_MAXA; ++j) {
        dl[j] = 0.f;
        if (j < A && ok(j)) {
          bool taken = false;
#pragma unroll
          for (int b = 0; b < HL_MAXA; ++b) taken = taken || (act_col[b] == j);
          const float l = lg[j] - lse_c[j];
          const float pj = expf(l);
          const float d_lp = (taken ? 1.f : 0.f) - pj;
          const float d_ent = -pj * (l + ent_c[j]);
          dl[j] = cpol_c[j] * d_lp + cent * d_ent;
          if constexpr (KL) {
          const float lo = p.old_logps[(long long)n * p.old_logps_stride + j];
          kl_n += etm_categorical_kl_term(lo, l, pj);
          if constexpr (PEN) dl[j] += pen_pol * (pj - expf(lo));
        }
        }
      }
      if constexpr (KL) { if (lane == 0) acc_kl += kl_n; }
    }
    const float vo = p.old_value[n];
    const float ret = vo + a_raw;
    const float dvv = v - vo;
    const bool in_v = (dvv >= -p.clip) && (dvv <= p.clip);
    const float vc = vo + fminf(fmaxf(dvv, -p.clip), p.clip);
    const float e1 = v - ret, e2 = vc - ret;
    const float v1 = e1 * e1, v2 = e2 * e2;
    if (lane == 0) acc[1] += fmaxf(v1, v2);
    const float g2 = in_v ? 2.f * e2 : 0.f;
    float gv;
    if (v1 > v2) gv = 2.f * e1;
    else if (v1 < v2) gv = g2;
    else gv = e1 + 0.5f * g2;
    const float d_value = p.vf_coef * p.val_scale * gv;

    // ---- back through the output heads and the ReLU masks; running sums of the parameter gradients
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const int k = lane + 64 * c;
      float gp = 0.f;
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a) if (a < A) gp += dl[a] * wbr[a][c];
      gp = hp[c] > 0.f ? gp : 0.f;
      const float gvv = hv[c] > 0.f ? d_value * wvr[c] : 0.f;
      p.gm_p[(long long)n * hid + k] = gp;
      p.gm_v[(long long)n * hid + k] = gvv;
      s_gp[c] += gp; s_gv[c] += gvv; s_wv[c] += d_value * hv[c];
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a) if (a < A) s_wb[a][c] += dl[a] * hp[c];
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a) s_bb[a] += dl[a];
      s_bv += d_value;
    }
  }

  // ---- the four waves' sums -> one partial row per workgroup: [sum gm_p | sum gm_v | d wv | d Wb[0] .. d Wb[A-1] | d bb[A] | d bv | 5 stats]
  //      (GS: then d log_std[A]; KL: then the KL sum)
  const int row = (3 + A) * hid + A + 1 + 5 + (GS ? A : 0) + (KL ? 1 : 0);
  auto put_row = [&](float *dst, bool add) {
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const int k = lane + 64 * c;
      float *q = dst + k;
      if (add) { q[0] += s_gp[c]; q[hid] += s_gv[c]; q[2 * hid] += s_wv[c]; }
      else { q[0] = s_gp[c]; q[hid] = s_gv[c]; q[2 * hid] = s_wv[c]; }
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a)
        if (a < A) { if (add) q[(3 + a) * hid] += s_wb[a][c]; else q[(3 + a) * hid] = s_wb[a][c]; }
    }
    if (lane == 0) {
      float *t = dst + (3 + A) * hid;
#pragma unroll
      for (int a = 0; a < HL_MAXA; ++a)
        if (a < A) { if (add) t[a] += s_bb[a]; else t[a] = s_bb[a]; }
      if (add) t[A] += s_bv; else t[A] = s_bv;
#pragma unroll
      for (int k5 = 0; k5 < 5; ++k5) { if (add) t[A + 1 + k5] += acc[k5]; else t[A + 1 + k5] = acc[k5]; }
      if constexpr (GS) {
#pragma unroll
        for (int a = 0; a < HL_MAXA; ++a)
          if (a < A) { if (add) t[A + 6 + a] += s_ls[a]; else t[A + 6 + a] = s_ls[a]; }
      }
      if constexpr (KL) { const int k = A + 6 + (GS ? A : 0); if (add) t[k] += acc_kl; else t[k] = acc_kl; }
    }
  };
  put_row(hl_lds + (long long)wave * row, false);
  __syncthreads();
  float *dst = p.partials + (long long)blockIdx.x * row;               // fixed order: ((w0 + w1) + w2) + w3
  for (int e = tid; e < row; e += 256) dst[e] = ((hl_lds[e] + hl_lds[row + e]) + hl_lds[2 * row + e]) + hl_lds[3 * row + e];
}

// The kernels: one body; the instantiations without masks keep their names, the masked ones are kernels of their own.
template <int HC, bool BR, bool GS = false>
__global__ __launch_bounds__(256) void heads_loss_kernel(const HlParams p0) { heads_loss_body<HC, BR, GS, false>(p0); }
template <int HC, bool BR>
__global__ __launch_bounds__(256) void heads_loss_masked_kernel(const HlParams p0) { heads_loss_body<HC, BR, false, true>(p0); }
template <int HC>
__global__ __launch_bounds__(256) void heads_loss_gaussian_kl_kernel(const HlParams p0) { heads_loss_body<HC, false, true, false, true>(p0); }
template <int HC, bool BR, bool MK>
__global__ __launch_bounds__(256) void heads_loss_kl_kernel(const HlParams p0) { heads_loss_body<HC, BR, false, MK, true>(p0); }
template <int HC>
__global__ __launch_bounds__(256) void heads_loss_gaussian_kl_penalty_kernel(const HlParams p0) { heads_loss_body<HC, false, true, false, true, true>(p0); }
template <int HC, bool BR, bool MK>
__global__ __launch_bounds__(256) void heads_loss_kl_penalty_kernel(const HlParams p0) { heads_loss_body<HC, BR, false, MK, true, true>(p0); }

// sums the workgroup rows and finishes the loss statistics: out = [row sums ... ], out8 (a Gaussian row's d log_std sums, behind the
// statistics, are summed like every other element).  One workgroup = 64 row elements x 16 row
// groups: thread (e, g) adds the rows g, g + 16, ... (all requested at once: the sum is a latency chain otherwise), the 16 group
// sums are added in group order -- a fixed tree, deterministic.
// KL = 1 (the Gaussian row with the KL sum as its last element): out8[4] = that sum * ent_scale (the exact KL), out8[6] = the k3 value.
// KL = 2 (the categorical row with the KL sum as its last element, right behind the five statistic sums): out8[4] = that sum *
// pol_scale -- the mean over samples AND branches, the convention of the k3 value, which goes to out8[6].
// PEN (`kl_penalty`, KL != 0): out8[2] gains coef * out8[4], out8[7] = coef = *kl_coef.
template <int KL, bool PEN = false>
__device__ __forceinline__ void heads_reduce_body(const float *__restrict__ partials, int n_wg, int row, int A, int hid, float vf_coef,
                                                  float beta, float pol_scale, float ent_scale, float val_scale,
                                                  const double *__restrict__ dyn, float *__restrict__ out, float *__restrict__ out8,
                                                  const float *__restrict__ kl_coef = nullptr) {
  static_assert(!PEN || KL != 0, "the KL penalty needs the exact KL");
  __shared__ float sm[16][64];
  const int el = threadIdx.x & 63, g = threadIdx.x >> 6;
  auto group_sum = [&](int e) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { const int w = g + 16 * u; v[u] = (e < row && w < n_wg) ? partials[(long long)w * row + e] : 0.f; }
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
    if (e < row)
      for (int w = g + 256; w < n_wg; w += 16) s += partials[(long long)w * row + e];    // (more than 256 rows: the rest in order)
    return s;
  };
  const int e = blockIdx.x * 64 + el;
  sm[g][el] = group_sum(e);
  __syncthreads();
  if (g == 0 && e < row) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sm[k][el];
    out[e] = s;
  }
  if (blockIdx.x != 0) return;
  // the five statistic sums (the last five row elements) once more in this workgroup, then out8
  __syncthreads();
  const int st0 = (3 + A) * hid + A + 1;
  if constexpr (KL != 0) sm[g][el] = el < 5 ? group_sum(st0 + el) : el == 5 ? group_sum(st0 + 5 + (KL == 1 ? A : 0)) : 0.f;
  else sm[g][el] = el < 5 ? group_sum(st0 + el) : 0.f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc[5];
    for (int k5 = 0; k5 < 5; ++k5) {
      float t = 0.f;
      for (int k = 0; k < 16; ++k) t += sm[k][k5];
      acc[k5] = t;
    }
    if (dyn) beta = (float)dyn[1];
    const float pol = acc[0] * pol_scale, val = acc[1] * val_scale, ent = acc[2] * ent_scale;
    out8[0] = pol; out8[1] = val; out8[2] = -(pol - vf_coef * val + beta * ent); out8[3] = ent;
    if constexpr (KL != 0) {
      float t = 0.f;
      for (int k = 0; k < 16; ++k) t += sm[k][5];
      const float k = t * (KL == 1 ? ent_scale : pol_scale);
      out8[4] = k; out8[5] = acc[4] * pol_scale; out8[6] = acc[3] * pol_scale; out8[7] = 0.f;
      if constexpr (PEN) { const float coef = kl_coef[0]; out8[2] = -(pol - vf_coef * val + beta * ent) + coef * k; out8[7] = coef; }
    } else {
      out8[4] = acc[3] * pol_scale; out8[5] = acc[4] * pol_scale; out8[6] = 0.f; out8[7] = 0.f;
    }
  }
}
__global__ __launch_bounds__(1024) void heads_reduce_kernel(const float *__restrict__ partials, int n_wg, int row, int A, int hid, float vf_coef,
                                                            float beta, float pol_scale, float ent_scale, float val_scale,
                                                            const double *__restrict__ dyn, float *__restrict__ out, float *__restrict__ out8) {
  heads_reduce_body<0>(partials, n_wg, row, A, hid, vf_coef, beta, pol_scale, ent_scale, val_scale, dyn, out, out8);
}
__global__ __launch_bounds__(1024) void heads_reduce_kl_kernel(const float *__restrict__ partials, int n_wg, int row, int A, int hid,
                                                               float vf_coef, float beta, float pol_scale, float ent_scale, float val_scale,
                                                               const double *__restrict__ dyn, float *__restrict__ out,
                                                               float *__restrict__ out8) {
  heads_reduce_body<1>(partials, n_wg, row, A, hid, vf_coef, beta, pol_scale, ent_scale, val_scale, dyn, out, out8);
}
__global__ __launch_bounds__(1024) void heads_reduce_categorical_kl_kernel(const float *__restrict__ partials, int n_wg, int row, int A, int hid,
                                                                           float vf_coef, float beta, float pol_scale, float ent_scale,
                                                                           float val_scale, const double *__restrict__ dyn,
                                                                           float *__restrict__ out, float *__restrict__ out8) {
  heads_reduce_body<2>(partials, n_wg, row, A, hid, vf_coef, beta, pol_scale, ent_scale, val_scale, dyn, out, out8);
}
__global__ __launch_bounds__(1024) void heads_reduce_kl_penalty_kernel(const float *__restrict__ partials, int n_wg, int row, int A, int hid,
                                                                       float vf_coef, float beta, float pol_scale, float ent_scale,
                                                                       float val_scale, const double *__restrict__ dyn, float *__restrict__ out,
                                                                       float *__restrict__ out8, const float *__restrict__ kl_coef) {
  heads_reduce_body<1, true>(partials, n_wg, row, A, hid, vf_coef, beta, pol_scale, ent_scale, val_scale, dyn, out, out8, kl_coef);
}
__global__ __launch_bounds__(1024) void heads_reduce_categorical_kl_penalty_kernel(const float *__restrict__ partials, int n_wg, int row, int A,
                                                                                   int hid, float vf_coef, float beta, float pol_scale,
                                                                                   float ent_scale, float val_scale,
                                                                                   const double *__restrict__ dyn, float *__restrict__ out,
                                                                                   float *__restrict__ out8, const float *__restrict__ kl_coef) {
  heads_reduce_body<2, true>(partials, n_wg, row, A, hid, vf_coef, beta, pol_scale, ent_scale, val_scale, dyn, out, out8, kl_coef);
}
static_assert(true, "");
constexpr int HL_SAMPLES_PER_WG = 8;      // two samples per wave: the pass is a latency chain per sample, so many short waves
}  // namespace

extern "C" int etm_heads_loss_supported(int N, int hid, int A) { return N > 0 && hid > 0 && hid % 64 == 0 && hid / 64 <= HL_MAXC && A > 0 && A <= HL_MAXA; }
extern "C" int etm_heads_loss_supported_gaussian(int N, int hid, int A) { return A <= ETM_MAX_BOX && etm_heads_loss_supported(N, hid, A); }
extern "C" int etm_heads_loss_supported_branched(int N, int hid, const int32_t *branch_sizes, int n_branches) {
  const int A = etm_branches_total(branch_sizes, n_branches);
  return A > 0 && n_branches <= HL_MAXA && etm_heads_loss_supported(N, hid, A);
}

namespace {
// The row of sums: [d b_lp (hid) | d b_lv (hid) | d wv (hid) | d Wb (A x hid) | d bb (A) | d bv | 5 raw sums], then d log_std (A) for a Box
// policy, then the raw KL sum with the exact KL.  The workspace holds one row per workgroup.
int hl_row_floats(int hid, int A, bool gauss, bool kl) { return (3 + A) * hid + A + 1 + 5 + (gauss ? A : 0) + (kl ? 1 : 0); }
int64_t hl_workspace_bytes(int N, int hid, int A, bool gauss, bool kl) {
  if (!(gauss ? etm_heads_loss_supported_gaussian(N, hid, A) : etm_heads_loss_supported(N, hid, A))) return 0;
  return (int64_t)((N + HL_SAMPLES_PER_WG - 1) / HL_SAMPLES_PER_WG) * hl_row_floats(hid, A, gauss, kl) * (int64_t)sizeof(float);
}
}  // namespace
extern "C" int etm_heads_loss_row_floats(int hid, int A) { return hl_row_floats(hid, A, false, false); }
extern "C" int etm_heads_loss_kl_row_floats(int hid, int A) { return hl_row_floats(hid, A, false, true); }
extern "C" int etm_heads_loss_gaussian_row_floats(int hid, int A) { return hl_row_floats(hid, A, true, false); }
extern "C" int etm_heads_loss_gaussian_kl_row_floats(int hid, int A) { return hl_row_floats(hid, A, true, true); }
extern "C" int64_t etm_heads_loss_workspace_bytes(int N, int hid, int A) { return hl_workspace_bytes(N, hid, A, false, false); }
extern "C" int64_t etm_heads_loss_kl_workspace_bytes(int N, int hid, int A) { return hl_workspace_bytes(N, hid, A, false, true); }
extern "C" int64_t etm_heads_loss_gaussian_workspace_bytes(int N, int hid, int A) { return hl_workspace_bytes(N, hid, A, true, false); }
extern "C" int64_t etm_heads_loss_gaussian_kl_workspace_bytes(int N, int hid, int A) { return hl_workspace_bytes(N, hid, A, true, true); }

namespace {
// One call of any of the eleven entries: the operands by name (what an entry does not take stays NULL / 0) and what the entry requires.
struct HlCall {
  HlParams p{};                           // the kernels' operands, filled by name (partials = the workspace; clip: by the launcher)
  double clip = 0;
  float *sums = nullptr, *out8 = nullptr;
  int64_t workspace_bytes = 0;
  const int32_t *branch_sizes = nullptr;  // with `branched`; p.A is then sum(sizes), set by the validator
  int n_branches = 1;
  void *stream = nullptr;
  // what the calling entry takes: Box (xact, log_std) | branch_sizes, n_branches instead of A | a mandatory action_mask (the exact-KL
  // entries take one or NULL) | the old policy (old_logps, or old_mean / old_log_std of a Box policy) | kl_coef
  bool gauss = false, branched = false, need_mask = false, kl = false, pen = false;
};
// a record `c` with the arguments that all eleven entries name alike
#define HL_CALL(c)                                                                                                                        \
  HlCall c;                                                                                                                               \
  c.p.pre_p = pre_p; c.p.pre_v = pre_v; c.p.b_lp = b_lp; c.p.b_lv = b_lv; c.p.wb = wb; c.p.bb = bb; c.p.wv = wv; c.p.bv = bv;            \
  c.p.action_stride = action_stride; c.p.old_logp = old_logp; c.p.logp_stride = logp_stride; c.p.adv = adv; c.p.old_value = old_value;    \
  c.p.adv_stats3 = adv_stats3; c.clip = clip; c.p.vf_coef = vf_coef; c.p.beta = beta; c.p.pol_scale = pol_scale;                         \
  c.p.ent_scale = ent_scale; c.p.val_scale = val_scale; c.p.dyn = dyn_clip_beta; c.p.gm_p = gm_p; c.p.gm_v = gm_v; c.sums = sums;        \
  c.out8 = out8; c.p.logits = logits; c.p.value = value; c.p.partials = (float *)workspace; c.workspace_bytes = workspace_bytes;         \
  c.p.N = N; c.p.hid = hid; c.stream = stream

bool hl_misaligned4(const void *q) { return ((uintptr_t)q & 3u) != 0; }

// Every refusal of every entry, in the one order that include/etm_hip.h states ("Refusals of the loss entries").
int hl_validate(HlCall &c) {
  HlParams &p = c.p;
  if (c.pen && (!p.kl_coef || hl_misaligned4(p.kl_coef))) return ETM_EINVAL;
  if (c.kl && !c.gauss && (!p.old_logps || hl_misaligned4(p.old_logps) || (!c.branched && p.old_logps_stride < p.A))) return ETM_EINVAL;
  if (c.gauss && !p.xact) return ETM_EINVAL;
  if (c.kl && c.gauss && (!p.old_mean || !p.old_log_std || hl_misaligned4(p.old_mean) || hl_misaligned4(p.old_log_std))) return ETM_EINVAL;
  if (c.need_mask && !p.amask) return ETM_EINVAL;
  if (c.branched) {
    if (!etm_heads_loss_supported_branched(p.N, p.hid, c.branch_sizes, c.n_branches)) return ETM_EUNSUPPORTED;
    p.A = etm_branches_total(c.branch_sizes, c.n_branches);
    if (p.action_stride < c.n_branches || p.logp_stride < c.n_branches || (c.kl && p.old_logps_stride < p.A)) return ETM_EINVAL;
  }
  if (c.gauss && (p.action_stride < p.A || p.logp_stride < 1 || (c.kl && p.old_mean_stride < p.A))) return ETM_EINVAL;
  if (!p.pre_p || !p.pre_v || !p.b_lp || !p.b_lv || !p.wb || !p.bb || !p.wv || !p.bv || !(c.gauss ? (const void *)p.log_std : (const void *)p.actions) ||
      !p.old_logp || !p.adv || !p.old_value || !p.adv_stats3 || !p.gm_p || !p.gm_v || !c.sums || !c.out8 || !p.partials)
    return ETM_EINVAL;
  if ((p.old_logps && c.gauss) || (c.pen && !c.kl)) return ETM_EINVAL;      // (no entry fills the record like this)
  if (p.amask && c.gauss) return ETM_EINVAL;
  if (const int rc = etm_action_mask_check(p.amask, p.A)) return rc;
  if (!(c.gauss ? etm_heads_loss_supported_gaussian(p.N, p.hid, p.A) : etm_heads_loss_supported(p.N, p.hid, p.A))) return ETM_EUNSUPPORTED;
  if (c.workspace_bytes < hl_workspace_bytes(p.N, p.hid, p.A, c.gauss, c.kl)) return ETM_EWORKSPACE;
  return 0;
}

// The kernel of a variant: Box (plain, exact KL, penalty), or categorical [plain, exact KL, penalty][branched][masked].
using HlKernel = void (*)(const HlParams);
template <int HC>
HlKernel hl_kernel(bool gauss, int level, bool branched, bool masked) {
  static constexpr HlKernel box[3] = {heads_loss_kernel<HC, false, true>, heads_loss_gaussian_kl_kernel<HC>, heads_loss_gaussian_kl_penalty_kernel<HC>};
  static constexpr HlKernel cat[3][2][2] = {
      {{heads_loss_kernel<HC, false>, heads_loss_masked_kernel<HC, false>}, {heads_loss_kernel<HC, true>, heads_loss_masked_kernel<HC, true>}},
      {{heads_loss_kl_kernel<HC, false, false>, heads_loss_kl_kernel<HC, false, true>},
       {heads_loss_kl_kernel<HC, true, false>, heads_loss_kl_kernel<HC, true, true>}},
      {{heads_loss_kl_penalty_kernel<HC, false, false>, heads_loss_kl_penalty_kernel<HC, false, true>},
       {heads_loss_kl_penalty_kernel<HC, true, false>, heads_loss_kl_penalty_kernel<HC, true, true>}}};
  return gauss ? box[level] : cat[level][branched][masked];
}

// The one launcher: validate, fill HlParams, the pass, the reduction.
int hl_launch(HlCall &c) {
  (void)hipGetLastError();
  if (const int rc = hl_validate(c)) return rc;
  HlParams &p = c.p;
  EtmBranches br;
  if (const int rc = etm_branches_make(c.branch_sizes, c.n_branches, p.A, &br)) return rc;
  p.nbr = br.n;
  for (int b = 0, j = 0; b < br.n; ++b) {
    p.branch_off[b] = j;
    for (int k = 0; k < br.size[b]; ++k, ++j) p.col_branch[j] = b;
  }
  p.clip = (float)c.clip; p.clip_lo = (float)(1.0 - c.clip); p.clip_hi = (float)(1.0 + c.clip);
  p.samples_per_wg = HL_SAMPLES_PER_WG;
  const int level = c.pen ? 2 : c.kl ? 1 : 0;
  const bool branched = br.n > 1, masked = p.amask != nullptr;
  HlKernel pass = nullptr;
  switch (p.hid / 64) {
    case 1: pass = hl_kernel<1>(c.gauss, level, branched, masked); break;
    case 2: pass = hl_kernel<2>(c.gauss, level, branched, masked); break;
    case 3: pass = hl_kernel<3>(c.gauss, level, branched, masked); break;
    case 4: pass = hl_kernel<4>(c.gauss, level, branched, masked); break;
    case 5: pass = hl_kernel<5>(c.gauss, level, branched, masked); break;
    case 6: pass = hl_kernel<6>(c.gauss, level, branched, masked); break;
    case 7: pass = hl_kernel<7>(c.gauss, level, branched, masked); break;
    case 8: pass = hl_kernel<8>(c.gauss, level, branched, masked); break;
    default: return ETM_EUNSUPPORTED;
  }
  const int n_wg = (p.N + HL_SAMPLES_PER_WG - 1) / HL_SAMPLES_PER_WG;
  const int row = hl_row_floats(p.hid, p.A, c.gauss, c.kl);
  const size_t lds = 4 * (size_t)row * sizeof(float);
  hipStream_t st = (hipStream_t)c.stream;
  {
    EtmProfScope prof(ETM_K_PPO_LOSS, st);
    hipLaunchKernelGGL(pass, dim3((unsigned)n_wg), dim3(256), lds, st, p);
  }
  if (const int rc = etm_launch_status()) return rc;
  EtmProfScope prof(ETM_K_PPO_FINAL, st);
  const dim3 grid((unsigned)((row + 63) / 64));
  if (c.pen) {
    const auto reduce = c.gauss ? heads_reduce_kl_penalty_kernel : heads_reduce_categorical_kl_penalty_kernel;
    hipLaunchKernelGGL(reduce, grid, dim3(1024), 0, st, (const float *)p.partials, n_wg, row, p.A, p.hid, p.vf_coef, p.beta, p.pol_scale,
                       p.ent_scale, p.val_scale, p.dyn, c.sums, c.out8, p.kl_coef);
  } else {
    const auto reduce = !c.kl ? heads_reduce_kernel : c.gauss ? heads_reduce_kl_kernel : heads_reduce_categorical_kl_kernel;
    hipLaunchKernelGGL(reduce, grid, dim3(1024), 0, st, (const float *)p.partials, n_wg, row, p.A, p.hid, p.vf_coef, p.beta, p.pol_scale,
                       p.ent_scale, p.val_scale, p.dyn, c.sums, c.out8);
  }
  return etm_launch_status();
}
}  // namespace

// The entries (include/etm_hip.h documents each): fill the record by name, say what the entry takes, launch.
extern "C" int etm_heads_loss(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb, const float *bb,
                              const float *wv, const float *bv, const int64_t *actions, int64_t action_stride, const float *old_logp,
                              int64_t logp_stride, const float *adv, const float *old_value, const float *adv_stats3, double clip, float vf_coef,
                              float beta, float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v,
                              float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid,
                              int A, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.p.A = A;
  return hl_launch(c);
}
extern "C" int etm_heads_loss_masked(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                     const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                     const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                     const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                     float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                                     float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid, int A,
                                     const int64_t *action_mask, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.p.A = A; c.p.amask = (const long long *)action_mask; c.need_mask = true;
  return hl_launch(c);
}
// MultiDiscrete: wb / bb = the branches' heads concatenated; actions / old_logp rows carry one entry per branch
extern "C" int etm_heads_loss_branched(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                       const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                       const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                       const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                       float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                                       float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid,
                                       const int32_t *branch_sizes, int n_branches, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.branch_sizes = branch_sizes; c.n_branches = n_branches; c.branched = true;
  return hl_launch(c);
}
extern "C" int etm_heads_loss_branched_masked(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                              const float *bb, const float *wv, const float *bv, const int64_t *actions,
                                              int64_t action_stride, const float *old_logp, int64_t logp_stride, const float *adv,
                                              const float *old_value, const float *adv_stats3, double clip, float vf_coef, float beta,
                                              float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                                              float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace,
                                              int64_t workspace_bytes, int N, int hid, const int32_t *branch_sizes, int n_branches,
                                              const int64_t *action_mask, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.branch_sizes = branch_sizes; c.n_branches = n_branches; c.branched = true;
  c.p.amask = (const long long *)action_mask; c.need_mask = true;
  return hl_launch(c);
}
// The exact categorical KL (`exact_kl: true`): the masked entries with action_mask optional (NULL: no masks) and old_logps [N, A]
extern "C" int etm_heads_loss_kl(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                 const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                 const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                 const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                 float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                                 float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid, int A,
                                 const int64_t *action_mask, const float *old_logps, int64_t old_logps_stride, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.p.A = A; c.p.amask = (const long long *)action_mask;
  c.p.old_logps = old_logps; c.p.old_logps_stride = old_logps_stride; c.kl = true;
  return hl_launch(c);
}
extern "C" int etm_heads_loss_branched_kl(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                          const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                          const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                          const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale,
                                          float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v,
                                          float *sums, float *out8, float *logits, float *value, void *workspace, int64_t workspace_bytes,
                                          int N, int hid, const int32_t *branch_sizes, int n_branches, const int64_t *action_mask,
                                          const float *old_logps, int64_t old_logps_stride, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.branch_sizes = branch_sizes; c.n_branches = n_branches; c.branched = true; c.p.amask = (const long long *)action_mask;
  c.p.old_logps = old_logps; c.p.old_logps_stride = old_logps_stride; c.kl = true;
  return hl_launch(c);
}
// Box policies (diagonal Gaussian, A <= 8): wb / bb = the mean head; xact [N, A] the stored raw actions; old_logp [N] the joint log-probs
extern "C" int etm_heads_loss_gaussian(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                       const float *bb, const float *wv, const float *bv, const float *xact, int64_t action_stride,
                                       const float *log_std, const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                       const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                       float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                                       float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid, int A,
                                       void *stream) {
  HL_CALL(c);
  c.p.xact = xact; c.p.log_std = log_std; c.p.A = A; c.gauss = true;
  return hl_launch(c);
}
// ... with the exact KL: old_mean [N, A] the means of the policy that drew the samples, old_log_std [A] a snapshot of its log sigma
extern "C" int etm_heads_loss_gaussian_kl(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                          const float *bb, const float *wv, const float *bv, const float *xact, int64_t action_stride,
                                          const float *log_std, const float *old_logp, int64_t logp_stride, const float *adv,
                                          const float *old_value, const float *adv_stats3, double clip, float vf_coef, float beta,
                                          float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                                          float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace,
                                          int64_t workspace_bytes, int N, int hid, int A, const float *old_mean, int64_t old_mean_stride,
                                          const float *old_log_std, void *stream) {
  HL_CALL(c);
  c.p.xact = xact; c.p.log_std = log_std; c.p.A = A; c.gauss = true;
  c.p.old_mean = old_mean; c.p.old_mean_stride = old_mean_stride; c.p.old_log_std = old_log_std; c.kl = true;
  return hl_launch(c);
}
// `kl_penalty`: the three exact-KL entries with the loss L + coef * K, K = out8[4], coef = *kl_coef, ONE device float32 read in place
extern "C" int etm_heads_loss_kl_penalty(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                         const float *bb, const float *wv, const float *bv, const int64_t *actions, int64_t action_stride,
                                         const float *old_logp, int64_t logp_stride, const float *adv, const float *old_value,
                                         const float *adv_stats3, double clip, float vf_coef, float beta, float pol_scale, float ent_scale,
                                         float val_scale, const double *dyn_clip_beta, float *gm_p, float *gm_v, float *sums, float *out8,
                                         float *logits, float *value, void *workspace, int64_t workspace_bytes, int N, int hid, int A,
                                         const int64_t *action_mask, const float *old_logps, int64_t old_logps_stride, const float *kl_coef,
                                         void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.p.A = A; c.p.amask = (const long long *)action_mask;
  c.p.old_logps = old_logps; c.p.old_logps_stride = old_logps_stride; c.kl = true; c.p.kl_coef = kl_coef; c.pen = true;
  return hl_launch(c);
}
extern "C" int etm_heads_loss_branched_kl_penalty(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                                  const float *bb, const float *wv, const float *bv, const int64_t *actions,
                                                  int64_t action_stride, const float *old_logp, int64_t logp_stride, const float *adv,
                                                  const float *old_value, const float *adv_stats3, double clip, float vf_coef, float beta,
                                                  float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                                                  float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace,
                                                  int64_t workspace_bytes, int N, int hid, const int32_t *branch_sizes, int n_branches,
                                                  const int64_t *action_mask, const float *old_logps, int64_t old_logps_stride,
                                                  const float *kl_coef, void *stream) {
  HL_CALL(c);
  c.p.actions = (const long long *)actions; c.branch_sizes = branch_sizes; c.n_branches = n_branches; c.branched = true; c.p.amask = (const long long *)action_mask;
  c.p.old_logps = old_logps; c.p.old_logps_stride = old_logps_stride; c.kl = true; c.p.kl_coef = kl_coef; c.pen = true;
  return hl_launch(c);
}
extern "C" int etm_heads_loss_gaussian_kl_penalty(const float *pre_p, const float *pre_v, const float *b_lp, const float *b_lv, const float *wb,
                                                  const float *bb, const float *wv, const float *bv, const float *xact, int64_t action_stride,
                                                  const float *log_std, const float *old_logp, int64_t logp_stride, const float *adv,
                                                  const float *old_value, const float *adv_stats3, double clip, float vf_coef, float beta,
                                                  float pol_scale, float ent_scale, float val_scale, const double *dyn_clip_beta, float *gm_p,
                                                  float *gm_v, float *sums, float *out8, float *logits, float *value, void *workspace,
                                                  int64_t workspace_bytes, int N, int hid, int A, const float *old_mean,
                                                  int64_t old_mean_stride, const float *old_log_std, const float *kl_coef, void *stream) {
  HL_CALL(c);
  c.p.xact = xact; c.p.log_std = log_std; c.p.A = A; c.gauss = true;
  c.p.old_mean = old_mean; c.p.old_mean_stride = old_mean_stride; c.p.old_log_std = old_log_std; c.kl = true; c.p.kl_coef = kl_coef; c.pen = true;
  return hl_launch(c);
}
#undef HL_CALL
