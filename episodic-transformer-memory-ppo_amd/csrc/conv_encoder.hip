// Rollout-only encoder convolution: implicit GEMM on fp32 MFMA with fused bias + ReLU (forward, no grad).
//
// Replaces, on the no-grad path, one `relu(conv2d(x))` of /root/reference model.py:90-92 (MIOpen + bias + ReLU launches;
// at n_workers = 32 the three layers cost ~110 us per rollout step, mostly launch overhead).  The optimisation phase
// keeps the library convolution (it needs the backward).
//
//   out[m, co] = relu(bias[co] + sum_k A[m, k] * Wt[co, k]),   m = (n, oy, ox),  k = (segment, offset)
// K is a list of memory-contiguous SEGMENTS of the input window of one output pixel:
//   NCHW input (layer 1, as it arrives from the host): segment = (c, ky), length KW          -> weights in native layout
//   NHWC input (layers 2, 3):                          segment = ky,      length KW * C      -> weights pre-permuted to
//                                                                                               [Cout][KH][KW][C]
// so every lane fetches its A fragment with 16-byte loads straight from global memory/L2 (no LDS staging, no barrier in
// the main loop).  One workgroup = one tile of 32 output pixels x all Cout (NT = Cout/32 accumulator tiles); its eight
// waves split K (interleaved 8-wide k-groups, all operands of a batch requested up front) and are reduced through LDS, then bias + ReLU + store (NHWC for the next
// layer, NCHW for the last one so that the flatten order of model.py:94 is unchanged).
#include "etm_common.h"

namespace {
struct ConvParams {
  const long long *in_index;   // optional: input = in + *in_index * in_index_stride (row of a time-major staging array)
  long long in_index_stride;
  union {
    const float *in;
    const unsigned char *in8;  // conv_relu_u8_kernel: the input is bytes
  };
  const float *w, *bias;
  float *out;
  int N, C, H, W, Cout, KH, KW, S, Ho, Wo;
  int in_nhwc, out_nchw;
  int seg_len, n_seg, groups;  // K = n_seg * seg_len, groups = K / 8
  int nt_total;                // channel tiles of the layer (Cout / 32); a workgroup covers NT of them from blockIdx.y * NT
};

constexpr int CONV_NW = 8;   // waves per workgroup = K slices
// GB (template parameter) = 8-wide k-groups per wave and batch: all operands of a batch are requested before its first MFMA;
// the launcher picks the smallest instantiated GB that covers a wave's share of K in one batch.

// U8 (conv_relu_u8_kernel): the NCHW first layer on byte observations -- p.in is then a byte pointer, offsets and in_index_stride count
// elements (= bytes), a lane's four window elements are one 4-byte load and become etm_byte_unit of each; everything after the load is the
// fp32 kernel.  One body for both (conv_relu_body.inc).
template <int NT, int GB>
__global__ __launch_bounds__(CONV_NW * 64) void conv_relu_kernel(const ConvParams p) {
  constexpr bool U8 = false;
#include "conv_relu_body.inc"
}
template <int NT, int GB>
__global__ __launch_bounds__(CONV_NW * 64) void conv_relu_u8_kernel(const ConvParams p) {
  constexpr bool U8 = true;
#include "conv_relu_body.inc"
}
}  // namespace

namespace {
// the instantiation (NT, GB) of the float or the byte kernel
// (the byte form is the first layer: one channel tile, Cout 32 -- etm_conv_relu_u8 refuses every other width)
#define ETM_CONV_KERNEL(NT_, GB_) (U8 ? conv_relu_u8_kernel<NT_, GB_> : conv_relu_kernel<NT_, GB_>)
template <bool U8>
int conv_relu_launch(const float *in, const int64_t *in_index, int64_t in_index_stride, const float *w, const float *bias,
                     float *out, int N, int C, int H, int W, int Cout, int KH, int KW, int S, int in_nhwc, int out_nchw,
                     void *stream) {
  (void)hipGetLastError();
  if (!in || !w || !bias || !out || N <= 0 || C <= 0 || H < KH || W < KW || Cout <= 0 || KH <= 0 || KW <= 0 || S <= 0) return ETM_EINVAL;
  ConvParams p;
  p.in_index = (const long long *)in_index; p.in_index_stride = in_index_stride;
  p.in = in; p.w = w; p.bias = bias; p.out = out; p.N = N; p.C = C; p.H = H; p.W = W; p.Cout = Cout; p.KH = KH; p.KW = KW; p.S = S;
  p.Ho = (H - KH) / S + 1; p.Wo = (W - KW) / S + 1; p.in_nhwc = in_nhwc; p.out_nchw = out_nchw;
  p.seg_len = in_nhwc ? KW * C : KW;
  p.n_seg = in_nhwc ? KH : C * KH;
  const int K = p.n_seg * p.seg_len;
  // 16-byte loads: every segment start and the 8-wide k-groups must be 4-float aligned
  const bool aligned = in_nhwc ? (C % 4 == 0) : (W % 4 == 0 && S % 4 == 0);
  if (p.seg_len % 8 != 0 || K % 8 != 0 || !aligned || (Cout != 32 && Cout != 64)) return ETM_EUNSUPPORTED;
  p.groups = K / 8;
  p.nt_total = Cout / 32;
  const int M = N * p.Ho * p.Wo;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_CONV_RELU, st);
  const dim3 grid((unsigned)((M + 31) / 32));
  const int gpw = (p.groups + CONV_NW - 1) / CONV_NW;     // k-groups per wave
  const dim3 block(CONV_NW * 64);
  if (Cout == 32) {
    if (gpw <= 4) hipLaunchKernelGGL(ETM_CONV_KERNEL(1, 4), grid, block, 0, st, p);
    else hipLaunchKernelGGL(ETM_CONV_KERNEL(1, 12), grid, block, 0, st, p);
  } else if constexpr (U8) {
    return ETM_EUNSUPPORTED;
  } else if (2 * grid.x <= 256) {
    // few pixel tiles (a worker group of a rollout step): one channel tile per workgroup -- twice the CUs, half the MFMA chain
    // and half the operand requests per wave; the A fragments are fetched twice, which is nothing at this size
    const dim3 grid2(grid.x, 2);
    if (gpw <= 4) hipLaunchKernelGGL((conv_relu_kernel<1, 4>), grid2, block, 0, st, p);
    else hipLaunchKernelGGL((conv_relu_kernel<1, 12>), grid2, block, 0, st, p);
  } else {
    if (gpw <= 4) hipLaunchKernelGGL((conv_relu_kernel<2, 4>), grid, block, 0, st, p);
    else if (gpw <= 8) hipLaunchKernelGGL((conv_relu_kernel<2, 8>), grid, block, 0, st, p);
    else if (gpw <= 10) hipLaunchKernelGGL((conv_relu_kernel<2, 10>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((conv_relu_kernel<2, 12>), grid, block, 0, st, p);
  }
  return etm_launch_status();
}
#undef ETM_CONV_KERNEL
}  // namespace

extern "C" int etm_conv_relu(const float *in, const int64_t *in_index, int64_t in_index_stride, const float *w, const float *bias,
                             float *out, int N, int C, int H, int W, int Cout, int KH, int KW, int S, int in_nhwc, int out_nchw,
                             void *stream) {
  return conv_relu_launch<false>(in, in_index, in_index_stride, w, bias, out, N, C, H, W, Cout, KH, KW, S, in_nhwc, out_nchw, stream);
}

// The NCHW first layer on byte observations (include/etm_hip.h): the fp32 kernel's address arithmetic in elements = bytes, one 4-byte
// load per lane and k-group (W % 4 == 0, S % 4 == 0, 8-wide groups: 4-byte aligned when the base and the row stride are).
extern "C" int etm_conv_relu_u8(const uint8_t *in, const int64_t *in_index, int64_t in_index_stride, const float *w, const float *bias,
                                float *out, int N, int C, int H, int W, int Cout, int KH, int KW, int S, int in_nhwc, int out_nchw,
                                void *stream) {
  if (in_nhwc || Cout != 32) return ETM_EUNSUPPORTED;
  if ((uintptr_t)in % 4 || in_index_stride % 4 || ((int64_t)C * H * W) % 4) return ETM_EINVAL;
  return conv_relu_launch<true>(reinterpret_cast<const float *>(in), in_index, in_index_stride, w, bias, out, N, C, H, W, Cout, KH, KW, S, 0,
                                out_nchw, stream);
}
