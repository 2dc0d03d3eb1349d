// (count, mean, M2) of N advantages on ONE workgroup of 1024 threads: the body of adv_stats_kernel (ppo_loss.hip) and of the
// advantage job of step_head_kernel (gather.hip).  `load(i)` is advantage i of the minibatch -- a plain read of the gathered
// vector in the first, a read through the minibatch indices in the second: the same values in the same order through the same
// expressions, so both give the same three numbers bit for bit.
#pragma once
#include "etm_common.h"

template <typename Load>
__device__ __forceinline__ void adv_stats_block_1024(int N, float *__restrict__ stats3, Load load) {
  __shared__ float red[16];
  __shared__ float mean_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float s = 0.f;
  for (int i = tid; i < N; i += 1024) s += load(i);
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    mean_s = t / (float)N;
  }
  __syncthreads();
  const float mean = mean_s;
  float m2 = 0.f;
  for (int i = tid; i < N; i += 1024) {
    const float d = load(i) - mean;
    m2 += d * d;
  }
  m2 = wave_sum(m2);
  __syncthreads();
  if (lane == 0) red[wave] = m2;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    stats3[0] = (float)N;
    stats3[1] = mean;
    stats3[2] = t;
  }
}
