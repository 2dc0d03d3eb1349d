// Optimiser step of one minibatch on flat fp32 arenas (replaces /root/reference trainer.py:311-312:
// `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)` + `optimizer.step()` with torch.optim.AdamW defaults).
//
// Parameters, gradients and both AdamW moments live in four flat buffers with one layout (every nn.Parameter is a view into
// the parameter arena, every .grad a view into the gradient arena -- the same buffer the data-parallel all-reduce sums), so
// the whole step is two launches, whatever the number of parameters:
//   etm_grad_sqnorm   per-workgroup partial sums of g^2 (fixed chunking => deterministic), and step += 1
//   etm_adamw_clip    every workgroup adds the partial sums in the same order -> total norm -> clip coefficient
//                     min(1, max_norm / (norm + 1e-6)) (the rule of clip_grad_norm_; data parallel: x 1 / world, the averaging of
//                     the all-reduced sum).  A non-finite norm poisons the step as upstream's does: a NaN gradient makes the norm and
//                     the coefficient NaN, so every gradient, parameter and moment becomes NaN; a +-Inf makes the coefficient 0, so that
//                     element becomes NaN and every other gradient 0.  max_norm <= 0: no clipping, a NaN stays in its element.
//                     Then for its elements:
//                       g *= coef (written back: the monitored gradient norms of model.py:128-151 are taken after clipping)
//                       p *= 1 - lr wd;  m = lerp(m, g, 1 - b1);  v = b2 v + (1 - b2) g g
//                       p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)   (torch's single-tensor AdamW, fp32, same order)
// HBM traffic: 4 B read for the norm + 16 B read / 16 B written per parameter = 36 B x 3.94 M = 142 MB at config 3.
// lr and the step counter are device-resident so a captured HIP graph replays the step under changing schedules.
//   etm_grad_sqnorm_gated / etm_adamw_clip_gated   the same pair under the KL early stop (`target_kl`)
//   etm_grad_sqnorm_adaptive                       the norm launch under the KL-adaptive learning rate (`adaptive_lr`): its deciding
//                     thread moves *lr_dev on the step's own kl before the AdamW launch reads it (with or without the early stop)
#include "etm_common.h"

#include <math.h>

namespace {
constexpr int OPT_THREADS = 256;

__device__ __forceinline__ float block_sum_256(float v, float *sm) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  const float t = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  __syncthreads();
  return t;
}

// ---- KL early stop (etm_grad_sqnorm_gated / etm_adamw_clip_gated): the step is dropped when an earlier step of this update was
// dropped or when !(kl <= kl_limit), kl being the step's own statistic (a NaN stops too).  gate: three 64-bit words, [0] stopped (0 / 1),
// [1] steps applied in this update, [2] the bit pattern of the kl that tripped.  Workgroup 0, thread 0 of the norm launch decides -- no
// other workgroup of that launch reads gate or step -- and every workgroup of the AdamW launch, one launch later, reads gate[0].  GATED
// is a compile-time switch on the ONE body of each kernel: the ungated instantiations hold the code they always held.
// ---- KL-adaptive learning rate (etm_grad_sqnorm_adaptive): ADAPT is the body's second compile-time switch.  Before the gate's test the
// deciding thread moves *lr_dev on the step's own kl -- kl > kl_high: lr = max(lr_min, lr / factor); 0 < kl < kl_low: lr = min(lr_max,
// lr * factor); anything else (a NaN, a kl <= 0, a kl at a limit): nothing -- and counts the decision in lr_state ([0] raises, [1] cuts).
// The AdamW launch, one launch later, reads the new *lr_dev.  A step behind a stopped gate moves nothing.
template <bool GATED, bool ADAPT>
__device__ __forceinline__ void grad_sqnorm_body(const float4 *__restrict__ g, long long n4, float *__restrict__ partial,
                                                 long long *__restrict__ step, const float *__restrict__ kl, float kl_limit,
                                                 unsigned long long *__restrict__ gate, unsigned long long *host_word,
                                                 float *__restrict__ lr_dev, float kl_low, float kl_high, float factor, float lr_min,
                                                 float lr_max, unsigned long long *__restrict__ lr_state) {
  __shared__ float sm[4];
  // the deciding thread's words are asked for first, so that their latency passes under the sum (they were written by earlier
  // launches of the stream)
  unsigned long long stopped = 0ull, applied = 0ull, raises = 0ull, cuts = 0ull;
  float k = 0.f, lr = 0.f;
  if ((GATED || ADAPT) && blockIdx.x == 0 && threadIdx.x == 0) {
    if (ADAPT) {
      lr = *lr_dev;
      raises = lr_state[0];
      cuts = lr_state[1];
    }
    if (GATED) {
      stopped = gate[0];
      applied = gate[1];
    }
    k = *kl;
  }
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * OPT_THREADS) {
    const float4 v = g[i];
    acc += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  const float t = block_sum_256(acc, sm);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = t;
    if (blockIdx.x == 0) {
      if (ADAPT && !(GATED && stopped != 0ull)) {
        if (k > kl_high) {
          *lr_dev = fmaxf(lr_min, __fdiv_rn(lr, factor));
          lr_state[1] = cuts + 1ull;
        } else if (k < kl_low && k > 0.f) {
          *lr_dev = fminf(lr_max, __fmul_rn(lr, factor));
          lr_state[0] = raises + 1ull;
        }
      }
      if (GATED) {
        bool halted = stopped != 0ull;
        if (!halted) {
          if (!(k <= kl_limit)) {
            halted = true;
            gate[0] = 1ull;
            gate[2] = (unsigned long long)__float_as_uint(k);
            if (host_word) {        // (pinned host memory, as the rollout sampler stores its step number into its host flag)
              __threadfence_system();
              __hip_atomic_store(host_word, applied + 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
          }
        }
        if (!halted) {
          if (step) *step += 1;
          gate[1] = applied + 1ull;
        }
      } else if (step) {
        *step += 1;
      }
    }
  }
}

template <bool GATED>
__device__ __forceinline__ void adamw_clip_body(float4 *__restrict__ p, float4 *__restrict__ g, float4 *__restrict__ m,
                                                float4 *__restrict__ v, long long n4, const float *__restrict__ partial, int n_partial,
                                                const float *__restrict__ lr_dev, const long long *__restrict__ step, double beta1,
                                                double beta2, double eps, double weight_decay, float max_norm, float grad_scale,
                                                float *__restrict__ norm_out, const unsigned long long *__restrict__ gate) {
  __shared__ float sm[4];
  const bool dropped = GATED && gate[0] != 0ull;      // (asked for first: its latency passes under the sum of the partials)
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += OPT_THREADS) acc += partial[i];
  // grad_scale: the arena holds grad_scale^-1 times the gradient (data parallel: the all-reduced SUM, grad_scale = 1 / world) --
  // the division rides in the clip coefficient instead of costing a pass over the arena; 1.0f changes no bit
  const float total = sqrtf(block_sum_256(acc, sm)) * grad_scale;
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total;
  if (dropped) return;                        // a dropped step: the norm above and nothing else (uniform over the launch)
  float coef = 1.f;
  if (max_norm > 0.f) {
    // torch.clamp(q, max = 1): a NaN norm gives a NaN coefficient (fminf would hand back the 1); every other q keeps fminf's bits
    const float q = max_norm / (total + 1e-6f);
    coef = !(q >= 1.f) ? q : 1.f;
  }
  coef *= grad_scale;
  // scalars as torch.optim.AdamW forms them (python floats = doubles), then the fp32 tensor arithmetic of its single-tensor
  // path in the same order: p.mul_(1 - lr wd); m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, value = 1 - b2);
  // denom = (v.sqrt() / sqrt(1 - b2^t)).add_(eps); p.addcdiv_(m, denom, value = -lr / (1 - b1^t))
  const double lr = (double)*lr_dev;
  const double t = (double)*step;
  const float keep = (float)(1.0 - lr * weight_decay);
  const float w1 = (float)(1.0 - beta1), b2f = (float)beta2, w2 = (float)(1.0 - beta2);
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
  const float neg_step = (float)(-(lr / (1.0 - pow(beta1, t))));
  const float epsf = (float)eps;
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * OPT_THREADS) {
    float4 pv = p[i], gv = g[i], mv = m[i], vv = v[i];
    float *pp = &pv.x, *gp = &gv.x, *mp = &mv.x, *vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = __fmul_rn(gp[k], coef);
      gp[k] = gk;
      float pk = __fmul_rn(pp[k], keep);
      const float mk = __fadd_rn(mp[k], __fmul_rn(w1, __fsub_rn(gk, mp[k])));
      const float vk = __fadd_rn(__fmul_rn(vp[k], b2f), __fmul_rn(__fmul_rn(w2, gk), gk));
      const float denom = __fadd_rn(__fdiv_rn(sqrtf(vk), bc2_sqrt), epsf);
      pk = __fadd_rn(pk, __fdiv_rn(__fmul_rn(neg_step, mk), denom));
      pp[k] = pk; mp[k] = mk; vp[k] = vk;
    }
    p[i] = pv; g[i] = gv; m[i] = mv; v[i] = vv;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_kernel(const float4 *__restrict__ g, long long n4, float *__restrict__ partial,
                                                                  long long *__restrict__ step) {
  grad_sqnorm_body<false, false>(g, n4, partial, step, nullptr, 0.f, nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f, 0.f, nullptr);
}
__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_gated_kernel(const float4 *__restrict__ g, long long n4, float *__restrict__ partial,
                                                                        long long *__restrict__ step, const float *__restrict__ kl,
                                                                        float kl_limit, unsigned long long *__restrict__ gate,
                                                                        unsigned long long *host_word) {
  grad_sqnorm_body<true, false>(g, n4, partial, step, kl, kl_limit, gate, host_word, nullptr, 0.f, 0.f, 0.f, 0.f, 0.f, nullptr);
}
__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_adaptive_kernel(const float4 *__restrict__ g, long long n4, float *__restrict__ partial,
                                                                           long long *__restrict__ step, const float *__restrict__ kl,
                                                                           float *__restrict__ lr_dev, float kl_low, float kl_high, float factor,
                                                                           float lr_min, float lr_max, unsigned long long *__restrict__ lr_state) {
  grad_sqnorm_body<false, true>(g, n4, partial, step, kl, 0.f, nullptr, nullptr, lr_dev, kl_low, kl_high, factor, lr_min, lr_max, lr_state);
}
__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_adaptive_gated_kernel(const float4 *__restrict__ g, long long n4,
                                                                                 float *__restrict__ partial, long long *__restrict__ step,
                                                                                 const float *__restrict__ kl, float *__restrict__ lr_dev,
                                                                                 float kl_low, float kl_high, float factor, float lr_min,
                                                                                 float lr_max, unsigned long long *__restrict__ lr_state,
                                                                                 float kl_limit, unsigned long long *__restrict__ gate,
                                                                                 unsigned long long *host_word) {
  grad_sqnorm_body<true, true>(g, n4, partial, step, kl, kl_limit, gate, host_word, lr_dev, kl_low, kl_high, factor, lr_min, lr_max, lr_state);
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_clip_kernel(float4 *__restrict__ p, float4 *__restrict__ g, float4 *__restrict__ m,
                                                                 float4 *__restrict__ v, long long n4, const float *__restrict__ partial,
                                                                 int n_partial, const float *__restrict__ lr_dev,
                                                                 const long long *__restrict__ step, double beta1, double beta2, double eps,
                                                                 double weight_decay, float max_norm, float grad_scale,
                                                                 float *__restrict__ norm_out) {
  adamw_clip_body<false>(p, g, m, v, n4, partial, n_partial, lr_dev, step, beta1, beta2, eps, weight_decay, max_norm, grad_scale, norm_out,
                         nullptr);
}
__global__ __launch_bounds__(OPT_THREADS) void adamw_clip_gated_kernel(float4 *__restrict__ p, float4 *__restrict__ g, float4 *__restrict__ m,
                                                                       float4 *__restrict__ v, long long n4, const float *__restrict__ partial,
                                                                       int n_partial, const float *__restrict__ lr_dev,
                                                                       const long long *__restrict__ step, double beta1, double beta2,
                                                                       double eps, double weight_decay, float max_norm, float grad_scale,
                                                                       float *__restrict__ norm_out,
                                                                       const unsigned long long *__restrict__ gate) {
  adamw_clip_body<true>(p, g, m, v, n4, partial, n_partial, lr_dev, step, beta1, beta2, eps, weight_decay, max_norm, grad_scale, norm_out,
                        gate);
}
// Monitored gradient norms (model.py:128-151: one norm per module group, taken after clipping): partial[s] = sum of squares of
// segment s (a run of <= 4096 floats inside ONE parameter tensor), then out[g] = sqrt(sum_s member[g][s] * partial[s]) -- two
// launches whatever the number of tensors and groups, every sum in a fixed order.
__device__ __forceinline__ void segment_sqsum_block(const float *__restrict__ g, const long long *__restrict__ seg_start,
                                                    const int *__restrict__ seg_len, float *__restrict__ partial, int s) {
  __shared__ float sm[4];
  const float *src = g + seg_start[s];
  const int len = seg_len[s];
  float v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = (int)threadIdx.x + k * OPT_THREADS;
    v[k] = i < len ? src[i] : 0.f;
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc += v[k] * v[k];
  const float t = block_sum_256(acc, sm);
  if (threadIdx.x == 0) partial[s] = t;
}
__device__ __forceinline__ float group_norm_block(const float *__restrict__ member, const float *__restrict__ partial, int n_segs, int gidx) {
  __shared__ float sm[4];
  float acc = 0.f;
  for (int s = threadIdx.x; s < n_segs; s += OPT_THREADS) acc += member[(long long)gidx * n_segs + s] * partial[s];
  return sqrtf(block_sum_256(acc, sm));
}
__global__ __launch_bounds__(OPT_THREADS) void segment_sqsum_kernel(const float *__restrict__ g, const long long *__restrict__ seg_start,
                                                                    const int *__restrict__ seg_len, float *__restrict__ partial) {
  segment_sqsum_block(g, seg_start, seg_len, partial, blockIdx.x);
}
__global__ __launch_bounds__(OPT_THREADS) void group_norm_kernel(const float *__restrict__ member, const float *__restrict__ partial, int n_segs,
                                                                 float *__restrict__ out) {
  const float t = group_norm_block(member, partial, n_segs, blockIdx.x);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// ---- End of a minibatch step that keeps its results on the device (etm_step_end / etm_group_norms_step): the step's statistics and
// monitored norms go to row `*counter` of result tables and the counter moves on, so that nothing has to be copied out between two
// replays of the captured step.  One workgroup reads the counter, files the statistics and stores counter + 1 -- a plain store, as
// grad_sqnorm_kernel advances the optimiser's step count -- in a launch in which no other workgroup looks at the counter; the norm
// kernel, one launch later, files its row under counter - 1.  Rows beyond the table are clamped to its last row (never out of bounds).
__device__ __forceinline__ void step_end_block(const float *__restrict__ stats, int n_stats, float *__restrict__ stats_table, int table_rows,
                                               long long *__restrict__ counter) {
  const long long c = *counter;
  const long long row = c < 0 ? 0 : (c >= table_rows ? table_rows - 1 : c);
  if (stats_table)
    for (int i = threadIdx.x; i < n_stats; i += OPT_THREADS) stats_table[row * n_stats + i] = stats[i];
  __syncthreads();
  if (threadIdx.x == 0) *counter = c + 1;
}
__global__ __launch_bounds__(OPT_THREADS) void step_end_kernel(const float *__restrict__ stats, int n_stats, float *__restrict__ stats_table,
                                                               int table_rows, long long *__restrict__ counter) {
  step_end_block(stats, n_stats, stats_table, table_rows, counter);
}
__global__ __launch_bounds__(OPT_THREADS) void segment_sqsum_end_kernel(const float *__restrict__ g, const long long *__restrict__ seg_start,
                                                                        const int *__restrict__ seg_len, float *__restrict__ partial, int n_segs,
                                                                        const float *__restrict__ stats, int n_stats,
                                                                        float *__restrict__ stats_table, int table_rows,
                                                                        long long *__restrict__ counter) {
  if ((int)blockIdx.x < n_segs) segment_sqsum_block(g, seg_start, seg_len, partial, blockIdx.x);
  else step_end_block(stats, n_stats, stats_table, table_rows, counter);
}
__global__ __launch_bounds__(OPT_THREADS) void group_norm_row_kernel(const float *__restrict__ member, const float *__restrict__ partial, int n_segs,
                                                                     float *__restrict__ out, float *__restrict__ norm_table, int table_rows,
                                                                     const long long *__restrict__ counter) {
  const float t = group_norm_block(member, partial, n_segs, blockIdx.x);
  if (threadIdx.x == 0) {
    const long long c = *counter - 1;                              // (segment_sqsum_end_kernel has moved the counter on already)
    const long long row = c < 0 ? 0 : (c >= table_rows ? table_rows - 1 : c);
    out[blockIdx.x] = t;
    norm_table[row * gridDim.x + blockIdx.x] = t;
  }
}
}  // namespace

// out[g] = sqrt(sum over segments of member[g][s] * ||flat[seg_start[s] .. + seg_len[s])||^2); seg_len <= 4096; partial: n_segs floats.
extern "C" int etm_group_norms(const float *flat, const int64_t *seg_start, const int32_t *seg_len, int n_segs, const float *member, int n_groups,
                               float *partial, float *out, void *stream) {
  (void)hipGetLastError();
  if (!flat || !seg_start || !seg_len || !member || !partial || !out || n_segs <= 0 || n_groups <= 0) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  hipLaunchKernelGGL(segment_sqsum_kernel, dim3((unsigned)n_segs), dim3(OPT_THREADS), 0, st, flat, (const long long *)seg_start, seg_len, partial);
  int rc = etm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(group_norm_kernel, dim3((unsigned)n_groups), dim3(OPT_THREADS), 0, st, member, partial, n_segs, out);
  return etm_launch_status();
}

// etm_group_norms whose two launches also end the minibatch step: row r = *counter of stats_table [table_rows, n_stats] = stats,
// row r of norm_table [table_rows, n_groups] = out, then *counter = r + 1.  out holds the same bits as etm_group_norms gives.
extern "C" int etm_group_norms_step(const float *flat, const int64_t *seg_start, const int32_t *seg_len, int n_segs, const float *member,
                                    int n_groups, float *partial, float *out, float *norm_table, const float *stats, int n_stats,
                                    float *stats_table, int table_rows, int64_t *counter, void *stream) {
  (void)hipGetLastError();
  if (!flat || !seg_start || !seg_len || !member || !partial || !out || n_segs <= 0 || n_groups <= 0) return ETM_EINVAL;
  if (!norm_table || !stats || !stats_table || !counter || n_stats <= 0 || table_rows <= 0) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  hipLaunchKernelGGL(segment_sqsum_end_kernel, dim3((unsigned)n_segs + 1), dim3(OPT_THREADS), 0, st, flat, (const long long *)seg_start, seg_len,
                     partial, n_segs, stats, n_stats, stats_table, table_rows, (long long *)counter);
  int rc = etm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(group_norm_row_kernel, dim3((unsigned)n_groups), dim3(OPT_THREADS), 0, st, member, partial, n_segs, out, norm_table,
                     table_rows, (const long long *)counter);
  return etm_launch_status();
}

// The end of a step whose gradient norms are not monitored: the statistics row and the counter alone (one workgroup).
extern "C" int etm_step_end(const float *stats, int n_stats, float *stats_table, int table_rows, int64_t *counter, void *stream) {
  (void)hipGetLastError();
  if (!stats || !stats_table || !counter || n_stats <= 0 || table_rows <= 0) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  hipLaunchKernelGGL(step_end_kernel, dim3(1), dim3(OPT_THREADS), 0, st, stats, n_stats, stats_table, table_rows, (long long *)counter);
  return etm_launch_status();
}

namespace {
int grad_sqnorm_launch(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, const float *kl, float kl_limit, uint64_t *gate,
                       uint64_t *host_word, bool gated, void *stream) {
  (void)hipGetLastError();
  if (!g || !partial || n <= 0 || n % 4 != 0 || n_partial <= 0 || n_partial > 4096) return ETM_EINVAL;
  if ((uintptr_t)g % 16 != 0) return ETM_EINVAL;
  if (gated && (!kl || !gate || (uintptr_t)kl % 4 != 0 || (uintptr_t)gate % 8 != 0 || (uintptr_t)host_word % 8 != 0)) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  if (gated)
    hipLaunchKernelGGL(grad_sqnorm_gated_kernel, dim3((unsigned)n_partial), dim3(OPT_THREADS), 0, st, (const float4 *)g, (long long)(n / 4),
                       partial, (long long *)step, kl, kl_limit, (unsigned long long *)gate, (unsigned long long *)host_word);
  else
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)n_partial), dim3(OPT_THREADS), 0, st, (const float4 *)g, (long long)(n / 4), partial,
                       (long long *)step);
  return etm_launch_status();
}

int adamw_clip_launch(float *p, float *g, float *m, float *v, int64_t n, const float *partial, int n_partial, const float *lr_dev,
                      const int64_t *step, double beta1, double beta2, double eps, double weight_decay, float max_norm, float grad_scale,
                      float *norm_out, const uint64_t *gate, bool gated, void *stream) {
  (void)hipGetLastError();
  if (!p || !g || !m || !v || !partial || !lr_dev || !step || n <= 0 || n % 4 != 0 || n_partial <= 0 || n_partial > 4096) return ETM_EINVAL;
  if ((uintptr_t)p % 16 || (uintptr_t)g % 16 || (uintptr_t)m % 16 || (uintptr_t)v % 16 || !(grad_scale > 0.f)) return ETM_EINVAL;
  if (gated && (!gate || (uintptr_t)gate % 8 != 0)) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  const long long n4 = n / 4;
  long long blocks = (n4 + OPT_THREADS * 4 - 1) / (OPT_THREADS * 4);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  if (gated)
    hipLaunchKernelGGL(adamw_clip_gated_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, (float4 *)p, (float4 *)g, (float4 *)m,
                       (float4 *)v, n4, partial, n_partial, lr_dev, (const long long *)step, beta1, beta2, eps, weight_decay, max_norm,
                       grad_scale, norm_out, (const unsigned long long *)gate);
  else
    hipLaunchKernelGGL(adamw_clip_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, (float4 *)p, (float4 *)g, (float4 *)m, (float4 *)v, n4,
                       partial, n_partial, lr_dev, (const long long *)step, beta1, beta2, eps, weight_decay, max_norm, grad_scale, norm_out);
  return etm_launch_status();
}
}  // namespace

extern "C" int etm_grad_sqnorm(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, void *stream) {
  return grad_sqnorm_launch(g, n, partial, n_partial, step, nullptr, 0.f, nullptr, nullptr, false, stream);
}

extern "C" int etm_grad_sqnorm_gated(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, const float *kl, float kl_limit,
                                     uint64_t *gate, uint64_t *host_word, void *stream) {
  return grad_sqnorm_launch(g, n, partial, n_partial, step, kl, kl_limit, gate, host_word, true, stream);
}

// The norm launch under the KL-adaptive learning rate (with gate: and under the KL early stop); the AdamW launch that follows is
// etm_adamw_clip (gate NULL) or etm_adamw_clip_gated as they are: it reads *lr_dev one launch later.
extern "C" int etm_grad_sqnorm_adaptive(const float *g, int64_t n, float *partial, int n_partial, int64_t *step, const float *kl, float *lr_dev,
                                        float kl_low, float kl_high, float factor, float lr_min, float lr_max, uint64_t *lr_state, float kl_limit,
                                        uint64_t *gate, uint64_t *host_word, void *stream) {
  (void)hipGetLastError();
  if (!g || !partial || n <= 0 || n % 4 != 0 || n_partial <= 0 || n_partial > 4096) return ETM_EINVAL;
  if ((uintptr_t)g % 16 != 0) return ETM_EINVAL;
  if (!kl || !lr_dev || !lr_state || (uintptr_t)kl % 4 != 0 || (uintptr_t)lr_dev % 4 != 0 || (uintptr_t)lr_state % 8 != 0) return ETM_EINVAL;
  if ((uintptr_t)gate % 8 != 0 || (uintptr_t)host_word % 8 != 0 || (host_word && !gate)) return ETM_EINVAL;
  if (!isfinite(kl_low) || !isfinite(kl_high) || !isfinite(factor) || !isfinite(lr_min) || !isfinite(lr_max)) return ETM_EINVAL;
  if (!(factor > 1.f) || !(kl_low >= 0.f) || !(kl_low < kl_high) || !(lr_min > 0.f) || !(lr_min <= lr_max)) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  if (gate)
    hipLaunchKernelGGL(grad_sqnorm_adaptive_gated_kernel, dim3((unsigned)n_partial), dim3(OPT_THREADS), 0, st, (const float4 *)g,
                       (long long)(n / 4), partial, (long long *)step, kl, lr_dev, kl_low, kl_high, factor, lr_min, lr_max,
                       (unsigned long long *)lr_state, kl_limit, (unsigned long long *)gate, (unsigned long long *)host_word);
  else
    hipLaunchKernelGGL(grad_sqnorm_adaptive_kernel, dim3((unsigned)n_partial), dim3(OPT_THREADS), 0, st, (const float4 *)g, (long long)(n / 4),
                       partial, (long long *)step, kl, lr_dev, kl_low, kl_high, factor, lr_min, lr_max, (unsigned long long *)lr_state);
  return etm_launch_status();
}

extern "C" int etm_adamw_clip(float *p, float *g, float *m, float *v, int64_t n, const float *partial, int n_partial, const float *lr_dev,
                              const int64_t *step, double beta1, double beta2, double eps, double weight_decay, float max_norm, float grad_scale,
                              float *norm_out, void *stream) {
  return adamw_clip_launch(p, g, m, v, n, partial, n_partial, lr_dev, step, beta1, beta2, eps, weight_decay, max_norm, grad_scale, norm_out,
                           nullptr, false, stream);
}

extern "C" int etm_adamw_clip_gated(float *p, float *g, float *m, float *v, int64_t n, const float *partial, int n_partial, const float *lr_dev,
                                    const int64_t *step, double beta1, double beta2, double eps, double weight_decay, float max_norm,
                                    float grad_scale, float *norm_out, const uint64_t *gate, void *stream) {
  return adamw_clip_launch(p, g, m, v, n, partial, n_partial, lr_dev, step, beta1, beta2, eps, weight_decay, max_norm, grad_scale, norm_out,
                           gate, true, stream);
}
