// Body of conv_relu_kernel / conv_relu_u8_kernel (csrc/conv_encoder.hip), included once into each: the two kernels are the same code but
// for the load of the A fragment, and each keeps a name of its own (the float kernel the one it always had).  In scope: NT, GB (template
// parameters), U8 (constexpr bool: p.in is a byte pointer), p (ConvParams).
  constexpr int NW = CONV_NW;
  __shared__ float red[NW * NT * 16 * 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int M = p.N * p.Ho * p.Wo;
  const int m = min((int)blockIdx.x * 32 + col, M - 1);
  const int n = m / (p.Ho * p.Wo);
  const int rem = m - n * p.Ho * p.Wo;
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  const long long in_row = p.in_index ? *p.in_index * p.in_index_stride : 0;      // elements in front of the input row
  const float *in_base = p.in + in_row;
  const unsigned char *in8_base = p.in8 + in_row;      // (U8)
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // weights arrive packed in fragment order (etm_hip.h): the B fragment of (k-group g, tile t) is 64 lanes x 4 floats,
  // contiguous -- one fully coalesced 1 KB load per wave instead of 64 different cache lines
  const int t_first = (int)blockIdx.y * NT;
  const float *wlane = p.w + lane * 4 + (long long)t_first * 256;

  // this lane's four window elements of the k-group that starts at k0, from the input row's base (float or byte elements)
  auto a_ptr = [&](auto *row_base, int k0) {
    const int seg = k0 / p.seg_len, off = k0 - seg * p.seg_len;
    long long base;
    if (p.in_nhwc) {            // seg = ky
      base = (((long long)n * p.H + oy * p.S + seg) * p.W + ox * p.S) * p.C;
    } else {                    // seg = c * KH + ky
      const int c = seg / p.KH, ky = seg - c * p.KH;
      base = (((long long)n * p.C + c) * p.H + oy * p.S + ky) * p.W + ox * p.S;
    }
    return row_base + base + off + half * 4;
  };
  auto a_load = [&](int k0) -> f32x4 {
    if constexpr (U8) return etm_bytes4_unit(*reinterpret_cast<const unsigned *>(a_ptr(in8_base, k0)));
    else return *reinterpret_cast<const f32x4 *>(a_ptr(in_base, k0));
  };

  // Wave w takes k-groups w, w + NW, ... in batches of GB.  Every operand of a batch is requested up front (unconditional
  // loads, groups past the end clamped to the last one), so a batch exposes ONE global-memory round trip; the three encoder
  // layers (3 / 8 / 9 groups per wave) are a single batch.  (The first version exposed a round trip per pair of groups, the
  // second one per four: at 32 images the kernel is pure latency.)
  f32x4 a_cur[GB], b_cur[GB][NT];
  const int last = p.groups - 1;
#define ETM_CONV_LOAD(dst_a, dst_b, g0_)                                                          \
  _Pragma("unroll") for (int u = 0; u < GB; ++u) {                                                \
    const int g_ = (g0_) + u * NW;                                                                \
    const int gc_ = g_ < p.groups ? g_ : last;                                                    \
    dst_a[u] = a_load(gc_ * 8);                                                                   \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) dst_b[u][t] = *reinterpret_cast<const f32x4 *>(wlane + ((long long)gc_ * p.nt_total + t) * 256); \
  }
  for (int g0 = wave; g0 < p.groups; g0 += GB * NW) {
    ETM_CONV_LOAD(a_cur, b_cur, g0)
#pragma unroll
    for (int u = 0; u < GB; ++u) {
      if (g0 + u * NW < p.groups) {     // wave-uniform: groups past the end are skipped
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[u][j], b_cur[u][t][j], acc[t], 0, 0, 0);
      }
    }
  }
#undef ETM_CONV_LOAD

  // reduce the K-slices of the waves through LDS (lane-contiguous: conflict-free)
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave * NT + t) * 16 + r) * 64 + lane] = acc[t][r];
  __syncthreads();
  // each thread finishes (t, r) pairs for its lane: NT*16 pairs over the waves
  for (int pr = wave; pr < NT * 16; pr += NW) {
    const int t = pr / 16, r = pr - t * 16;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[((w * NT + t) * 16 + r) * 64 + lane];
    const int row = mfma32_row(r, lane);
    const int mm = (int)blockIdx.x * 32 + row;
    if (mm < M) {
      const int co = (t_first + t) * 32 + col;
      v = fmaxf(v + p.bias[co], 0.f);
      if (p.out_nchw) {
        const int nn = mm / (p.Ho * p.Wo);
        const int rr = mm - nn * p.Ho * p.Wo;
        p.out[((long long)nn * p.Cout + co) * p.Ho * p.Wo + rr] = v;
      } else {
        p.out[(long long)mm * p.Cout + co] = v;
      }
    }
  }
