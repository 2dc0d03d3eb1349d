// uint8 image observations -> fp32 (include/etm_hip.h, byte observations): dst[r][j] = etm_byte_unit(src[row(r)][j]).
//
// The general fallback in front of every fp32 kernel that has no byte form (the fp32-MFMA and library encoders, geometries outside the
// bf16 kernels', inputs the rollout encoder does not take).  Any row length and any alignment of the source; the destination is dense, so
// a thread owns four consecutive floats of the FLAT result and writes them with one 16-byte store (the last thread: the 1 - 3 floats that
// remain, one by one).  Its four bytes come as one 4-byte load where they lie in one source row at a 4-byte aligned address, else byte
// by byte (a row boundary inside the quad, a row gather, an odd source offset).  64-bit offsets throughout.
#include "etm_common.h"

namespace {
__global__ __launch_bounds__(256) void bytes_to_unit_kernel(const unsigned char *__restrict__ src, const long long *__restrict__ index,
                                                            float *__restrict__ dst, long long rows, long long row_bytes) {
  const long long total = rows * row_bytes;
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  const long long r = e0 / row_bytes, c = e0 - r * row_bytes;
  const unsigned char *s = src + (index ? index[r] : r) * row_bytes + c;
  if (c + 4 <= row_bytes && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
    *reinterpret_cast<f32x4 *>(dst + e0) = etm_bytes4_unit(*reinterpret_cast<const unsigned *>(s));
    return;
  }
  float v[4];
  const int n = (int)(total - e0 < 4 ? total - e0 : 4);
  long long rr = r, cc = c;
  for (int j = 0; j < n; ++j) {
    v[j] = etm_byte_unit(src[(index ? index[rr] : rr) * row_bytes + cc]);
    if (++cc == row_bytes) { cc = 0; ++rr; }
  }
  if (n == 4) {
    *reinterpret_cast<f32x4 *>(dst + e0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int j = 0; j < n; ++j) dst[e0 + j] = v[j];
  }
}
}  // namespace

extern "C" int etm_bytes_to_unit(const uint8_t *src, const int64_t *index, float *dst, int64_t rows, int64_t row_bytes, void *stream) {
  (void)hipGetLastError();
  if (!src || !dst || rows <= 0 || row_bytes <= 0) return ETM_EINVAL;
  if ((uintptr_t)dst % 16) return ETM_EINVAL;
  const long long quads = (rows * row_bytes + 3) / 4, blocks = (quads + 255) / 256;
  if (blocks > 0x7fffffffll) return ETM_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_BYTES_TO_UNIT, st);
  hipLaunchKernelGGL(bytes_to_unit_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, (const long long *)index, dst, (long long)rows,
                     (long long)row_bytes);
  return etm_launch_status();
}
