// Running observation and return normalisation (include/etm_hip.h, "running normalisation"; ABI 54).
//
// Three entries, each a short sequence of ordinary launches: a grid-wide dependency is a launch boundary, no workgroup ever waits for
// another inside a kernel.  Statistics are (count, mean, M2 = sum (x - mean)^2) triples in double, combined with the pairwise update of
// Chan et al.; every combination order is fixed by the ALGORITHM's constants (rows per chunk, lanes per row, tile shape), never by the
// grid or by timing, and there are no floating-point atomics: the same input gives the same bits on every run.
//
//   etm_obs_stats_update   launch 1: one workgroup per (chunk of OBS_CHUNK rows, tile of <= 64 features).  The 256 threads cover the
//                          chunk's memory flat (thread = (row mod RP, feature), RP = 256 / tile width rows per pass: consecutive threads
//                          read consecutive floats); a thread sums its rows shifted by the first of them (double: exact shifts, no
//                          cancellation against the feature's offset), the RP threads of a feature combine in a fixed tree -> the chunk's
//                          triple.  launch 2: one thread per feature combines the chunk triples IN CHUNK ORDER, merges the result into the
//                          running triple in place and writes the fp32 table (mean, rstd = 1 / sqrt(M2 / count + epsilon), formed in
//                          double, rounded once).
//   etm_obs_normalize      out[n][f] = clamp((x[row(n)][f] - mean[f]) * rstd[f], -clip, +clip) in fp32, subtraction and product rounded
//                          separately (no FMA contraction, as csrc/gae.hip does for its recurrence); NaN stays NaN.  One thread per four
//                          consecutive floats of the dense result; 16-byte loads and stores where F % 4 == 0 and the arrays are aligned.
//   etm_return_scale       launch 1: the per-worker forward recurrence R_t = gamma R_{t-1} + r_t in double (product and sum rounded
//                          separately), R = 0 after a done -- in the shape of csrc/gae.hip: a wave owns 16 workers and walks the time axis
//                          in tiles of 64 steps, loads in the memory layout (next tile in flight under the scan), the dependent chain
//                          on lane w for worker w from a transposed LDS image.  All 64 lanes then sum the tile's R values (each its fixed
//                          16) into per-lane triples; a fixed tree gives the workgroup's partial triple.  launch 2 (one workgroup):
//                          partials -> batch triple (fixed order), merged into the running triple, scale = fp32(1 / sqrt(M2 / count +
//                          epsilon)).  launch 3: scaled = clamp(r * scale, -clip, +clip) in fp32.  (Three launches rather than two: a
//                          scaling grid that merged for itself would read every partial once per workgroup.)
#include "etm_common.h"

namespace {
constexpr int OBS_CHUNK = 256;     // rows per chunk of etm_obs_stats_update: a property of the algorithm (it fixes the summation order)
constexpr int OBS_TILE = 64;       // features per workgroup
constexpr int OBS_MAX_F = 1024;

struct Tri {
  double n, mean, m2;
};

// Chan et al.: the triple of the union of two disjoint samples
__device__ __forceinline__ Tri tri_merge(const Tri &a, const Tri &b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
  return Tri{n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}

// k values summed as s1 = sum (x - K), s2 = sum (x - K)^2 around one of them (K)
__device__ __forceinline__ Tri tri_from_shifted(int k, double K, double s1, double s2) {
  if (k == 0) return Tri{0.0, 0.0, 0.0};
  const double m = s1 / (double)k;
  const double m2 = s2 - s1 * m;
  return Tri{(double)k, K + m, m2 > 0.0 ? m2 : 0.0};
}

// t[i] <- the union of t[i + j * stride], j = 0 .. P - 1 with slot(i) = j, as a fixed binary tree (all threads of the workgroup call this)
__device__ __forceinline__ void tri_tree(Tri *t, int i, int slot, int P, int stride, bool active) {
  for (int s = 1; s < P; s <<= 1) {
    __syncthreads();
    if (active && slot % (2 * s) == 0 && slot + s < P) t[i] = tri_merge(t[i], t[i + s * stride]);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void obs_stats_chunk_kernel(const float *__restrict__ x, int R, int F, double *__restrict__ ws) {
  __shared__ Tri t_s[256];
  const int chunk = blockIdx.x, f0 = blockIdx.y * OBS_TILE;
  const int FT = min(OBS_TILE, F - f0);        // width of this tile
  const int RP = 256 / FT;                     // rows per pass
  const int tid = threadIdx.x;
  const int slot = tid / FT, f = f0 + tid % FT;
  const bool active = slot < RP;
  const int r0 = chunk * OBS_CHUNK, r1 = min(R, r0 + OBS_CHUNK);
  int k = 0;
  double K = 0.0, s1 = 0.0, s2 = 0.0;
  if (active) {
    for (int r = r0 + slot; r < r1; r += RP) {
      const double v = (double)x[(long long)r * F + f];
      if (k == 0) K = v;
      const double d = v - K;
      s1 += d;
      s2 += d * d;
      ++k;
    }
  }
  t_s[tid] = tri_from_shifted(k, K, s1, s2);
  tri_tree(t_s, tid, slot, RP, FT, active);
  if (active && slot == 0) {
    const Tri t = t_s[tid];
    double *o = ws + (long long)chunk * 3 * F + f;
    o[0] = t.n;
    o[F] = t.mean;
    o[2 * (long long)F] = t.m2;
  }
}

__global__ __launch_bounds__(64) void obs_stats_merge_kernel(const double *__restrict__ ws, int chunks, int F, double *__restrict__ stats,
                                                             float *__restrict__ mean, float *__restrict__ rstd, double epsilon) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  Tri b{0.0, 0.0, 0.0};
  for (int c = 0; c < chunks; ++c) {
    const double *p = ws + (long long)c * 3 * F + f;
    b = tri_merge(b, Tri{p[0], p[F], p[2 * (long long)F]});
  }
  const Tri t = tri_merge(Tri{stats[f], stats[F + f], stats[2 * (long long)F + f]}, b);
  stats[f] = t.n;
  stats[F + f] = t.mean;
  stats[2 * (long long)F + f] = t.m2;
  mean[f] = t.n > 0.0 ? (float)t.mean : 0.f;
  rstd[f] = t.n > 0.0 ? (float)(1.0 / sqrt(t.m2 / t.n + epsilon)) : 1.f;
}

__device__ __forceinline__ float norm_one(float v, float m, float r, float clip) {
  const float y = __fmul_rn(__fsub_rn(v, m), r);
  return y < -clip ? -clip : (y > clip ? clip : y);      // (a NaN compares false twice and stays)
}

template <bool VEC>
__global__ __launch_bounds__(256) void obs_normalize_kernel(const float *__restrict__ x, const long long *__restrict__ index,
                                                            const float *__restrict__ mean, const float *__restrict__ rstd, float clip,
                                                            float *__restrict__ out, long long N, int F) {
  const long long total = N * F;
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  if constexpr (VEC) {        // F % 4 == 0: the quad lies in one row; every array 16-byte aligned
    const long long n = e0 / F;
    const int f = (int)(e0 - n * F);
    const f32x4 v = *reinterpret_cast<const f32x4 *>(x + (index ? index[n] : n) * F + f);
    const f32x4 m = *reinterpret_cast<const f32x4 *>(mean + f), r = *reinterpret_cast<const f32x4 *>(rstd + f);
    *reinterpret_cast<f32x4 *>(out + e0) = f32x4{norm_one(v[0], m[0], r[0], clip), norm_one(v[1], m[1], r[1], clip),
                                                 norm_one(v[2], m[2], r[2], clip), norm_one(v[3], m[3], r[3], clip)};
  } else {
    const int cnt = (int)(total - e0 < 4 ? total - e0 : 4);
    long long n = e0 / F;
    int f = (int)(e0 - n * F);
    for (int j = 0; j < cnt; ++j) {
      out[e0 + j] = norm_one(x[(index ? index[n] : n) * F + f], mean[f], rstd[f], clip);
      if (++f == F) { f = 0; ++n; }
    }
  }
}

// ---- returns
constexpr int RS_WPW = 16;                 // workers per wave
constexpr int RS_TT = 1024 / RS_WPW;       // steps per tile
constexpr int RS_HEAD = 16;                // bytes in front of the partial triples in the workspace: the fp32 scale

template <bool VEC>
__global__ __launch_bounds__(64) void return_scan_kernel(const float *__restrict__ rewards, const unsigned char *__restrict__ dones,
                                                         double *__restrict__ ret_carry, double gamma, double *__restrict__ partials,
                                                         int W, int S) {
  constexpr int WPW = RS_WPW, TT = RS_TT;
  constexpr int LPR = TT / 4;        // lanes per worker row of a tile (4 steps per lane)
  constexpr int RW = 64 / LPR;       // worker rows covered by one load instruction of the wave
  constexpr int NI = WPW / RW;       // load instructions per array and tile
  constexpr int LS = TT + 1;
  __shared__ double R_s[WPW * LS];           // the tile's rewards (as doubles), overwritten by the returns
  __shared__ unsigned char d_s[WPW * LS];
  __shared__ Tri t_s[64];
  const int lane = threadIdx.x;
  const int w0 = blockIdx.x * WPW;
  const int rsub = lane / LPR, tsub = (lane % LPR) * 4;
  const int n_tiles = (S + TT - 1) / TT;
  float pr[NI][4];
  unsigned char pd[NI][4];
  auto fetch = [&](int tile) {
    const int t = tile * TT + tsub;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int w = w0 + i * RW + rsub;
      if constexpr (VEC) {                   // S % 4 == 0: a lane's 4 steps are inside or outside together, rows are 16-byte aligned
        const bool ok = w < W && t < S;
        const long long g = ok ? (long long)w * S + t : 0;
        const f32x4 r4 = *reinterpret_cast<const f32x4 *>(rewards + g);
        const uchar4 d4 = *reinterpret_cast<const uchar4 *>(dones + g);
        pr[i][0] = r4[0]; pr[i][1] = r4[1]; pr[i][2] = r4[2]; pr[i][3] = r4[3];
        pd[i][0] = d4.x; pd[i][1] = d4.y; pd[i][2] = d4.z; pd[i][3] = d4.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = w < W && t + j < S;
          const long long g = ok ? (long long)w * S + t + j : 0;
          pr[i][j] = rewards[g];
          pd[i][j] = dones[g];
        }
      }
    }
  };
  fetch(0);
  const int wl = w0 + lane;
  double Rc = (lane < WPW && wl < W) ? ret_carry[wl] : 0.0;      // running return of worker w0 + lane (lanes < WPW)
  Tri acc{0.0, 0.0, 0.0};
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t0 = tile * TT;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        R_s[(i * RW + rsub) * LS + tsub + j] = (double)pr[i][j];
        d_s[(i * RW + rsub) * LS + tsub + j] = pd[i][j];
      }
    __syncthreads();
    if (tile + 1 < n_tiles) fetch(tile + 1);                       // in flight while this tile is scanned
    const int t_hi = min(TT, S - t0);
    if (lane < WPW && wl < W) {
      const int base = lane * LS;
      for (int t = 0; t < t_hi; ++t) {
        Rc = __dadd_rn(__dmul_rn(gamma, Rc), R_s[base + t]);
        R_s[base + t] = Rc;
        if (d_s[base + t]) Rc = 0.0;
      }
    }
    __syncthreads();
    int k = 0;
    double K = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int w = w0 + i * RW + rsub;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (w < W && tsub + j < t_hi) {
          const double v = R_s[(i * RW + rsub) * LS + tsub + j];
          if (k == 0) K = v;
          const double d = v - K;
          s1 += d;
          s2 += d * d;
          ++k;
        }
      }
    }
    acc = tri_merge(acc, tri_from_shifted(k, K, s1, s2));
    __syncthreads();
  }
  if (lane < WPW && wl < W) ret_carry[wl] = Rc;
  t_s[lane] = acc;
  tri_tree(t_s, lane, lane, 64, 1, true);
  if (lane == 0) {
    double *o = partials + (long long)blockIdx.x * 3;
    o[0] = t_s[0].n;
    o[1] = t_s[0].mean;
    o[2] = t_s[0].m2;
  }
}

__global__ __launch_bounds__(256) void return_merge_kernel(const double *__restrict__ partials, int NB, double *__restrict__ stats,
                                                           double epsilon, float *__restrict__ scale) {
  __shared__ Tri t_s[256];
  const int i = threadIdx.x;
  const int per = (NB + 255) / 256;
  Tri a{0.0, 0.0, 0.0};
  for (int b = i * per; b < min(NB, (i + 1) * per); ++b) a = tri_merge(a, Tri{partials[3 * (long long)b], partials[3 * (long long)b + 1], partials[3 * (long long)b + 2]});
  t_s[i] = a;
  tri_tree(t_s, i, i, 256, 1, true);
  if (i == 0) {
    const Tri t = tri_merge(Tri{stats[0], stats[1], stats[2]}, t_s[0]);
    stats[0] = t.n;
    stats[1] = t.mean;
    stats[2] = t.m2;
    *scale = t.n > 0.0 ? (float)(1.0 / sqrt(t.m2 / t.n + epsilon)) : 1.f;
  }
}

__device__ __forceinline__ float scale_one(float r, float s, float clip) {
  const float y = __fmul_rn(r, s);
  return y < -clip ? -clip : (y > clip ? clip : y);
}

template <bool VEC>
__global__ __launch_bounds__(256) void return_apply_kernel(const float *__restrict__ rewards, const float *__restrict__ scale, float clip,
                                                           float *__restrict__ scaled, long long total) {
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  const float s = *scale;
  if (VEC && e0 + 4 <= total) {
    const f32x4 r = *reinterpret_cast<const f32x4 *>(rewards + e0);
    *reinterpret_cast<f32x4 *>(scaled + e0) = f32x4{scale_one(r[0], s, clip), scale_one(r[1], s, clip), scale_one(r[2], s, clip), scale_one(r[3], s, clip)};
  } else {
    for (long long e = e0; e < min(total, e0 + 4); ++e) scaled[e] = scale_one(rewards[e], s, clip);
  }
}
}  // namespace

extern "C" int etm_obs_stats_supported(int F) { return F >= 1 && F <= OBS_MAX_F; }

extern "C" int64_t etm_obs_stats_workspace_bytes(int R, int F) {
  if (R <= 0 || !etm_obs_stats_supported(F)) return 0;
  return (int64_t)((R + OBS_CHUNK - 1) / OBS_CHUNK) * 3 * F * (int64_t)sizeof(double);
}

extern "C" int etm_obs_stats_update(const float *x, int R, int F, double *stats, float *mean, float *rstd, double epsilon, void *workspace,
                                    int64_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (!x || !stats || !mean || !rstd || !workspace || R <= 0 || F <= 0 || !(epsilon > 0.0)) return ETM_EINVAL;
  if (!etm_obs_stats_supported(F)) return ETM_EUNSUPPORTED;
  if ((uintptr_t)workspace % 8 || (uintptr_t)stats % 8) return ETM_EINVAL;
  if (workspace_bytes < etm_obs_stats_workspace_bytes(R, F)) return ETM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_RUNNING_NORM, st);
  const int chunks = (R + OBS_CHUNK - 1) / OBS_CHUNK, tiles = (F + OBS_TILE - 1) / OBS_TILE;
  hipLaunchKernelGGL(obs_stats_chunk_kernel, dim3((unsigned)chunks, (unsigned)tiles), dim3(256), 0, st, x, R, F, (double *)workspace);
  hipLaunchKernelGGL(obs_stats_merge_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, st, (const double *)workspace, chunks, F, stats,
                     mean, rstd, epsilon);
  return etm_launch_status();
}

extern "C" int etm_obs_normalize(const float *x, const int64_t *index, const float *mean, const float *rstd, float clip, float *out,
                                 int64_t N, int F, void *stream) {
  (void)hipGetLastError();
  if (!x || !mean || !rstd || !out || N <= 0 || F <= 0 || !(clip > 0.f)) return ETM_EINVAL;
  const long long quads = (N * F + 3) / 4, blocks = (quads + 255) / 256;
  if (blocks > 0x7fffffffll) return ETM_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_RUNNING_NORM, st);
  const bool vec = F % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)mean % 16 == 0 && (uintptr_t)rstd % 16 == 0 && (uintptr_t)out % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(obs_normalize_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, x, (const long long *)index, mean, rstd, clip, out,
                       (long long)N, F);
  else
    hipLaunchKernelGGL(obs_normalize_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, x, (const long long *)index, mean, rstd, clip, out,
                       (long long)N, F);
  return etm_launch_status();
}

extern "C" int64_t etm_return_scale_workspace_bytes(int W) {
  if (W <= 0) return 0;
  return RS_HEAD + (int64_t)((W + RS_WPW - 1) / RS_WPW) * 3 * (int64_t)sizeof(double);
}

extern "C" int etm_return_scale(const float *rewards, const uint8_t *dones, double *ret_carry, double *stats, double gamma, double epsilon,
                                float clip, float *scaled, int W, int S, void *workspace, int64_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (!rewards || !dones || !ret_carry || !stats || !scaled || !workspace || W <= 0 || S <= 0) return ETM_EINVAL;
  if (!(epsilon > 0.0) || !(clip > 0.f)) return ETM_EINVAL;
  if ((uintptr_t)workspace % 16 || (uintptr_t)stats % 8 || (uintptr_t)ret_carry % 8) return ETM_EINVAL;
  if (workspace_bytes < etm_return_scale_workspace_bytes(W)) return ETM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_RUNNING_NORM, st);
  const int NB = (W + RS_WPW - 1) / RS_WPW;
  float *scale = (float *)workspace;
  double *partials = (double *)((char *)workspace + RS_HEAD);
  const bool vec = S % 4 == 0 && (uintptr_t)rewards % 16 == 0 && (uintptr_t)dones % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(return_scan_kernel<true>, dim3((unsigned)NB), dim3(64), 0, st, rewards, dones, ret_carry, gamma, partials, W, S);
  else
    hipLaunchKernelGGL(return_scan_kernel<false>, dim3((unsigned)NB), dim3(64), 0, st, rewards, dones, ret_carry, gamma, partials, W, S);
  hipLaunchKernelGGL(return_merge_kernel, dim3(1), dim3(256), 0, st, (const double *)partials, NB, stats, epsilon, scale);
  const long long total = (long long)W * S, blocks = ((total + 3) / 4 + 255) / 256;
  if ((uintptr_t)rewards % 16 == 0 && (uintptr_t)scaled % 16 == 0)
    hipLaunchKernelGGL(return_apply_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, rewards, (const float *)scale, clip, scaled, total);
  else
    hipLaunchKernelGGL(return_apply_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, rewards, (const float *)scale, clip, scaled, total);
  return etm_launch_status();
}
