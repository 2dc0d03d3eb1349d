// Device body of the fixed-order column-sum reduction at the end of a backward pass, shared by its own launch (block_train.hip:
// colsum_reduce_grouped_kernel) and by the extra workgroups of the grouped weight-gradient launch (grouped_dw.hip:
// etm_grouped_dw_tail).  One source for both: every element is summed in one order whichever launch carries the workgroup, so the
// results are the same bits.
#pragma once
#include "etm_common.h"

// out[c] = sum_p partial[p * ld + c] for the 64 columns of workgroup `blk` of the problem: 256 threads, wave w adds the rows
// p = w, w + 4, ... into 8 accumulators (8 loads in flight per lane), tree over the 8, then the four waves in wave order.
__device__ __forceinline__ void colsum_reduce_block(const float *__restrict__ partial, int P, int C, int ld, float *__restrict__ out, int blk) {
  __shared__ float sm[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blk * 64 + lane;
  const int cc = c < C ? c : 0;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  int p = wave;
  for (; p + 7 * 4 < P; p += 8 * 4) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += partial[(long long)(p + k * 4) * ld + cc];
  }
  for (; p < P; p += 4) acc[0] += partial[(long long)p * ld + cc];
  sm[wave][lane] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (wave == 0 && c < C) out[c] = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
}
