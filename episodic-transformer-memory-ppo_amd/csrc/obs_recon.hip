// obs_reconstruction: the decoder's last layer, ConvTranspose2d(32, C, 8, 4) on a2 NHWC [N, Hi, Wi, 32], fused with the sigmoid
// cross-entropy against the observation and with that loss's gradient: the logits [N, Ho, Wo, C] (Ho = 4 (Hi - 1) + 8) never exist in
// memory.  utils.transposed_conv_last / utils.obs_reconstruction_loss are the host definitions.
//   etm_obs_recon_fwd_loss: a thread owns one 4 x 4 block of output pixels (Y = 4 qy + ry, X = 4 qx + rx; qy <= Hi, qx <= Wi) of one image,
//                           all C channels: 16 C accumulators, in DOUBLE (the gfx950 vector unit issues a double FMA at the rate of an
//                           unpacked float one): the loss, dz and db then come out correctly rounded, which the bound of 4 x a
//                           float32 evaluation's error needs where that evaluation is exact by luck -- db is C numbers.  The block's pixels share their (at most) 2 x 2 input pixels
//                           iy in {qy - 1, qy}, ix in {qx - 1, qx}, and the weight w[ci][c][Y - 4 iy][X - 4 ix] of a product depends on
//                           (ry, rx), not on the block: every lane of a wave multiplies by the same weight, which the compiler reads
//                           through the scalar cache (no LDS, no vector register per weight) from a copy as doubles that a small
//                           launch in front writes into the workspace.  Products in ascending (iy, ix, ci), the
//                           bias last.  A missing input pixel (image edge) multiplies zeros.  Then per element
//                           l = max(z, 0) - z t + log1p(exp(-|z|)), s = sigmoid(z) from exp(-|z|), dz = ((s - t) / count) coef (in double,
//                           rounded once: a float32 1 / count would bias every element the same way, and db with them): the
//                           block's rows leave as 16-byte stores, the loss and db[c] = sum dz as one partial row of doubles per
//                           workgroup (thread sums, a fixed butterfly per wave, the waves in order).
//   obs_recon_reduce_kernel: the partial rows, thread t of 256 adding rows t, t + 256, ... in ascending order and a fixed tree over the
//                           threads, in double, rounded once: out[0] = loss, out[1] = *coef, out[2] = their product, out[3] = 0,
//                           db[c].  No float atomics anywhere: two calls give the same bits.
//   etm_obs_recon_dgrad   : da2[n, iy, ix, ci] = (a2 > 0) sum_{ky, kx, c} dz[n, 4 iy + ky, 4 ix + kx, c] w[ci][c][ky][kx]: a thread
//                           owns one input pixel and its 32 channels; the weight is transposed into LDS once per workgroup as
//                           [(ky, kx, c)][ci] (8 C KB), so that the 32 channels of one (ky, kx, c) are eight 16-byte reads of one
//                           address for the whole wave (a broadcast), and a gradient value is read once per 32 products.  Plain FMA
//                           (the README's section says why).
#include "etm_common.h"

namespace {
constexpr int OR_THREADS = 256;
constexpr int OR_PART = 8;                    // doubles of a workgroup's partial row: the loss sum, db[0 .. 3], padding
constexpr int OR_CIN = 32;                    // channels of a2 (dec_conv2's output)
constexpr int OR_MAXHW = 1 << 12;
constexpr long long OR_MAXTHREADS = 1ll << 31;

__device__ __forceinline__ double or_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// 4 pixels x C channels of one image row of the target, as floats
template <int C, bool U8>
__device__ __forceinline__ void or_load_target(const void *x, long long elem, float *t) {
  if constexpr (U8) {
    const unsigned *p = (const unsigned *)((const uint8_t *)x + elem);       // elem % 4 == 0 (X = 4 qx, Wo % 4 == 0)
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const f32x4 v = etm_bytes4_unit(p[j]);
      t[4 * j] = v[0]; t[4 * j + 1] = v[1]; t[4 * j + 2] = v[2]; t[4 * j + 3] = v[3];
    }
  } else {
    const f32x4 *p = (const f32x4 *)((const float *)x + elem);
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const f32x4 v = p[j];
      t[4 * j] = v[0]; t[4 * j + 1] = v[1]; t[4 * j + 2] = v[2]; t[4 * j + 3] = v[3];
    }
  }
}

template <int C, bool U8>
__global__ __launch_bounds__(OR_THREADS) void obs_recon_fwd_loss_kernel(const float *__restrict__ a2, const double *__restrict__ w,
                                                                        const float *__restrict__ bias, const void *__restrict__ x,
                                                                        const long long *__restrict__ x_index, long long x_images,
                                                                        const float *__restrict__ coef, float *__restrict__ dz,
                                                                        double *__restrict__ part, long long total, int Hi, int Wi,
                                                                        double inv_count) {
  __shared__ double red[OR_THREADS / ETM_WAVE][OR_PART];
  const long long p = (long long)blockIdx.x * OR_THREADS + threadIdx.x;
  double lsum = 0.0;
  double dbs[C];
#pragma unroll
  for (int c = 0; c < C; ++c) dbs[c] = 0.0;
  if (p < total) {
    const int bw = Wi + 1, per = (Hi + 1) * bw;
    const long long n = p / per;
    const int rem = (int)(p - n * per);
    const int qy = rem / bw, qx = rem - qy * bw;
    double acc[C][4][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[c][i >> 2][i & 3] = 0.0;
#pragma unroll 1
    for (int pix = 0; pix < 4; ++pix) {                      // (iy, ix) ascending: (qy - 1, qx - 1), (qy - 1, qx), (qy, qx - 1), (qy, qx)
      const int iy = qy - 1 + (pix >> 1), ix = qx - 1 + (pix & 1);
      const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
      const int koff = ((pix >> 1) ? 0 : 32) + ((pix & 1) ? 0 : 4);       // ky = ry + 4 for the row above, kx = rx + 4 for the column left
      const f32x4 *ap = (const f32x4 *)(a2 + ((n * Hi + (ok ? iy : 0)) * Wi + (ok ? ix : 0)) * OR_CIN);
      const double *wk = w + koff;
#pragma unroll 1
      for (int g = 0; g < OR_CIN / 4; ++g) {
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) a = ap[g];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double *wc = wk + (long long)(4 * g + j) * C * 64;
          const double av = (double)a[j];
#pragma unroll
          for (int c = 0; c < C; ++c)
#pragma unroll
            for (int ry = 0; ry < 4; ++ry)
#pragma unroll
              for (int rx = 0; rx < 4; ++rx) acc[c][ry][rx] = __builtin_fma(av, wc[c * 64 + ry * 8 + rx], acc[c][ry][rx]);
        }
      }
    }
    const int Ho = 4 * Hi + 4, Wo = 4 * Wi + 4;
    const float cf = *coef;
    long long img = n;
    if (x_index) {                       // (an index outside the bank is the caller's error; clamped so that nothing is read outside it)
      img = x_index[n];
      img = img < 0 ? 0 : (img >= x_images ? x_images - 1 : img);
    }
    float bs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) bs[c] = bias[c];
#pragma unroll
    for (int ry = 0; ry < 4; ++ry) {
      const int Y = 4 * qy + ry;
      float t[4 * C], o[4 * C];
      or_load_target<C, U8>(x, ((img * Ho + Y) * Wo + 4 * qx) * C, t);
#pragma unroll
      for (int rx = 0; rx < 4; ++rx)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double zd = acc[c][ry][rx] + (double)bs[c];
          const float z = (float)zd;
          const float tt = t[rx * C + c];
          const float e = expf(-fabsf(z));
          const float l = (fmaxf(z, 0.f) - z * tt) + log1pf(e);
          // the gradient in double, rounded once: db sums N Ho Wo of these, and neither a float32 sigmoid's rounding nor a float32
          // accumulator's averages out over them far enough
          const double ed = exp(-fabs(zd));
          const double rd = 1.0 / (1.0 + ed);
          const double dd = (((zd >= 0.0 ? rd : ed * rd) - (double)tt) * inv_count) * (double)cf;
          const float d = (float)dd;
          o[rx * C + c] = d;
          lsum += (double)l;
          dbs[c] += dd;
        }
      f32x4 *op = (f32x4 *)(dz + ((n * Ho + Y) * Wo + 4 * qx) * C);
#pragma unroll
      for (int j = 0; j < C; ++j) op[j] = f32x4{o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]};
    }
  }
  const int wave = threadIdx.x / ETM_WAVE, lane = threadIdx.x % ETM_WAVE;
  lsum = or_wave_sum(lsum);
#pragma unroll
  for (int c = 0; c < C; ++c) dbs[c] = or_wave_sum(dbs[c]);
  if (lane == 0) {
    red[wave][0] = lsum;
#pragma unroll
    for (int c = 0; c < C; ++c) red[wave][1 + c] = dbs[c];
  }
  __syncthreads();
  if (threadIdx.x < OR_PART) {
    double s = 0.0;
    if (threadIdx.x <= C)
      for (int k = 0; k < OR_THREADS / ETM_WAVE; ++k) s += red[k][threadIdx.x];
    part[(long long)blockIdx.x * OR_PART + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(OR_THREADS) void obs_recon_reduce_kernel(const double *__restrict__ part, long long P, int C, double count,
                                                                      const float *__restrict__ coef, float *__restrict__ out,
                                                                      float *__restrict__ db) {
  __shared__ double sh[OR_THREADS];
  const int t = threadIdx.x;
  for (int j = 0; j <= C; ++j) {
    double s = 0.0;
    for (long long i = t; i < P; i += OR_THREADS) s += part[i * OR_PART + j];
    sh[t] = s;
    __syncthreads();
    for (int o = OR_THREADS / 2; o > 0; o >>= 1) {
      if (t < o) sh[t] += sh[t + o];
      __syncthreads();
    }
    if (t == 0) {
      if (j == 0) {
        const float loss = (float)(sh[0] / count), cf = *coef;
        out[0] = loss;
        out[1] = cf;
        out[2] = __fmul_rn(cf, loss);            // the term of the training loss
        out[3] = 0.f;
      } else {
        db[j - 1] = (float)sh[0];
      }
    }
    __syncthreads();
  }
}

// the weight as doubles, once per call (it changes with every optimiser step): the forward kernel's scalar operands
__global__ __launch_bounds__(OR_THREADS) void obs_recon_weights_kernel(const float *__restrict__ w, double *__restrict__ wd, int n) {
  const int i = blockIdx.x * OR_THREADS + threadIdx.x;
  if (i < n) wd[i] = (double)w[i];
}

template <int C>
__global__ __launch_bounds__(OR_THREADS) void obs_recon_dgrad_kernel(const float *__restrict__ dz, const float *__restrict__ w,
                                                                     const float *__restrict__ a2, float *__restrict__ da2, long long total,
                                                                     int Hi, int Wi) {
  __shared__ __attribute__((aligned(16))) float wl[64 * C][OR_CIN];          // [(ky, kx, c)][ci]
  for (int i = threadIdx.x; i < 64 * C * OR_CIN; i += OR_THREADS) {
    const int ci = i % OR_CIN, kc = i / OR_CIN;
    const int k = kc / C, c = kc - k * C;
    wl[kc][ci] = w[(ci * C + c) * 64 + k];
  }
  __syncthreads();
  const long long p = (long long)blockIdx.x * OR_THREADS + threadIdx.x;
  if (p >= total) return;
  const int per = Hi * Wi;
  const long long n = p / per;
  const int rem = (int)(p - n * per);
  const int iy = rem / Wi, ix = rem - iy * Wi;
  const int Ho = 4 * Hi + 4, Wo = 4 * Wi + 4;
  float acc[OR_CIN];
#pragma unroll
  for (int i = 0; i < OR_CIN; ++i) acc[i] = 0.f;
#pragma unroll 1
  for (int ky = 0; ky < 8; ++ky) {
    const f32x4 *row = (const f32x4 *)(dz + ((n * Ho + 4 * iy + ky) * Wo + 4 * ix) * C);      // 8 pixels x C channels, contiguous
    f32x4 v[2 * C];
#pragma unroll
    for (int j = 0; j < 2 * C; ++j) v[j] = row[j];
#pragma unroll
    for (int q = 0; q < 8 * C; ++q) {                                                           // q = kx C + c
      const float d = v[q >> 2][q & 3];
      const f32x4 *wr = (const f32x4 *)wl[ky * 8 * C + q];
#pragma unroll
      for (int g = 0; g < OR_CIN / 4; ++g) {
        const f32x4 ww = wr[g];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[4 * g + j] = __builtin_fmaf(d, ww[j], acc[4 * g + j]);
      }
    }
  }
  const f32x4 *ap = (const f32x4 *)(a2 + p * OR_CIN);
  f32x4 *op = (f32x4 *)(da2 + p * OR_CIN);
#pragma unroll
  for (int g = 0; g < OR_CIN / 4; ++g) {
    const f32x4 a = ap[g];
    op[g] = f32x4{a[0] > 0.f ? acc[4 * g] : 0.f, a[1] > 0.f ? acc[4 * g + 1] : 0.f, a[2] > 0.f ? acc[4 * g + 2] : 0.f,
                  a[3] > 0.f ? acc[4 * g + 3] : 0.f};
  }
}

inline bool or_al(const void *ptr, unsigned a) { return ((uintptr_t)ptr & (a - 1)) == 0; }

template <int C, bool U8>
void or_launch_fwd(unsigned blocks, hipStream_t st, const float *a2, const double *w, const float *bias, const void *x, const int64_t *x_index,
                   int64_t x_images, const float *coef, float *dz, double *part, long long total, int Hi, int Wi, double inv_count) {
  hipLaunchKernelGGL((obs_recon_fwd_loss_kernel<C, U8>), dim3(blocks), dim3(OR_THREADS), 0, st, a2, w, bias, x, (const long long *)x_index,
                     (long long)x_images, coef, dz, part, total, Hi, Wi, inv_count);
}
template <bool U8, class... A>
void or_dispatch_fwd(int C, A... a) {
  switch (C) {
    case 1: or_launch_fwd<1, U8>(a...); break;
    case 2: or_launch_fwd<2, U8>(a...); break;
    case 3: or_launch_fwd<3, U8>(a...); break;
    default: or_launch_fwd<4, U8>(a...); break;
  }
}
}  // namespace

extern "C" int etm_obs_recon_supported(int C, int Hi, int Wi) {
  return C >= 1 && C <= 4 && Hi >= 1 && Wi >= 1 && Hi <= OR_MAXHW && Wi <= OR_MAXHW ? 1 : 0;
}

// workgroups of the forward launch = partial rows of its workspace (0: outside the entry's support)
static long long or_fwd_blocks(int64_t N, int C, int Hi, int Wi) {
  if (!etm_obs_recon_supported(C, Hi, Wi) || N < 1) return 0;
  const long long total = (long long)N * (Hi + 1) * (Wi + 1);
  if (total >= OR_MAXTHREADS || (long long)N * (4 * Hi + 4) * (4 * Wi + 4) * C >= (1ll << 40)) return 0;
  return (total + OR_THREADS - 1) / OR_THREADS;
}

// the workspace: the workgroups' partial rows, then the weight as doubles
extern "C" int64_t etm_obs_recon_workspace_bytes(int64_t N, int C, int Hi, int Wi) {
  const long long blocks = or_fwd_blocks(N, C, Hi, Wi);
  return blocks ? (blocks * OR_PART + (int64_t)OR_CIN * C * 64) * (int64_t)sizeof(double) : 0;
}

extern "C" int etm_obs_recon_fwd_loss(const float *a2, const float *w, const float *bias, const void *x, int x_is_u8, const int64_t *x_index,
                                      int64_t x_images, const float *coef, float *dz, float *out, float *db, void *workspace,
                                      int64_t workspace_bytes, int64_t N, int C, int Hi, int Wi, void *stream) {
  (void)hipGetLastError();
  if (!a2 || !w || !bias || !x || !coef || !dz || !out || !db || !workspace || N < 1 || C < 1 || C > 4) return ETM_EINVAL;
  if (x_index && x_images < 1) return ETM_EINVAL;
  if (!or_al(a2, 16) || !or_al(dz, 16) || !or_al(w, 4) || !or_al(bias, 4) || !or_al(coef, 4) || !or_al(out, 4) || !or_al(db, 4) ||
      !or_al(workspace, 8) || !or_al(x_index, 8) || !or_al(x, x_is_u8 ? 4 : 16))
    return ETM_EINVAL;
  const long long blocks = or_fwd_blocks(N, C, Hi, Wi);
  if (blocks == 0) return ETM_EUNSUPPORTED;
  if (workspace_bytes < etm_obs_recon_workspace_bytes(N, C, Hi, Wi)) return ETM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)N * (Hi + 1) * (Wi + 1);
  const double count = (double)N * (4 * Hi + 4) * (4 * Wi + 4) * C;
  double *part = (double *)workspace, *wd = part + blocks * OR_PART;
  {
    EtmProfScope prof(ETM_K_CONV_TRAIN_FWD, st);
    const int nw = OR_CIN * C * 64;
    hipLaunchKernelGGL(obs_recon_weights_kernel, dim3((unsigned)((nw + OR_THREADS - 1) / OR_THREADS)), dim3(OR_THREADS), 0, st, w, wd, nw);
    if (int rc = etm_launch_status()) return rc;
    if (x_is_u8)
      or_dispatch_fwd<true>(C, (unsigned)blocks, st, a2, (const double *)wd, bias, x, x_index, x_images, coef, dz, part, total, Hi, Wi, 1.0 / count);
    else
      or_dispatch_fwd<false>(C, (unsigned)blocks, st, a2, (const double *)wd, bias, x, x_index, x_images, coef, dz, part, total, Hi, Wi, 1.0 / count);
    if (int rc = etm_launch_status()) return rc;
  }
  EtmProfScope prof(ETM_K_COLSUM, st);
  hipLaunchKernelGGL(obs_recon_reduce_kernel, dim3(1), dim3(OR_THREADS), 0, st, (const double *)part, blocks, C, count, coef, out, db);
  return etm_launch_status();
}

extern "C" int etm_obs_recon_dgrad(const float *dz, const float *w, const float *a2, float *da2, int64_t N, int C, int Hi, int Wi, void *stream) {
  (void)hipGetLastError();
  if (!dz || !w || !a2 || !da2 || N < 1 || C < 1 || C > 4) return ETM_EINVAL;
  if (!or_al(dz, 16) || !or_al(a2, 16) || !or_al(da2, 16) || !or_al(w, 4)) return ETM_EINVAL;
  if (or_fwd_blocks(N, C, Hi, Wi) == 0) return ETM_EUNSUPPORTED;
  const long long total = (long long)N * Hi * Wi;
  const unsigned blocks = (unsigned)((total + OR_THREADS - 1) / OR_THREADS);
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_CONV_TRAIN_DGRAD, st);
  switch (C) {
    case 1: hipLaunchKernelGGL(obs_recon_dgrad_kernel<1>, dim3(blocks), dim3(OR_THREADS), 0, st, dz, w, a2, da2, total, Hi, Wi); break;
    case 2: hipLaunchKernelGGL(obs_recon_dgrad_kernel<2>, dim3(blocks), dim3(OR_THREADS), 0, st, dz, w, a2, da2, total, Hi, Wi); break;
    case 3: hipLaunchKernelGGL(obs_recon_dgrad_kernel<3>, dim3(blocks), dim3(OR_THREADS), 0, st, dz, w, a2, da2, total, Hi, Wi); break;
    default: hipLaunchKernelGGL(obs_recon_dgrad_kernel<4>, dim3(blocks), dim3(OR_THREADS), 0, st, dz, w, a2, da2, total, Hi, Wi); break;
  }
  return etm_launch_status();
}
