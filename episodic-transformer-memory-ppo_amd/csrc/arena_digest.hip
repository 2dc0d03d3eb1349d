// Digest of a flat fp32 arena taken as raw bits (checkpointing: trainer.save_checkpoint / load_checkpoint / state_digest; absent
// upstream, whose checkpoint holds the model's state dict alone).  One pass over the n words b_i of the arena gives four 64-bit words:
//   out4[0]  fingerprint  sum_i mix(i * 0x9E3779B97F4A7C15 + b_i)  mod 2^64  (mix = the splitmix64 finaliser): position dependent
//            (swapping two unequal elements changes it) and bit exact (-0 and +0 differ)
//   out4[1]  number of words whose exponent field is all ones (Inf or NaN)
//   out4[2]  bit pattern of the largest |x| among the finite words (0: none) -- of non-negative floats the bit patterns order as the values
//   out4[3]  n
// Every reduction is an integer sum or an integer max, so no order of summation changes a bit: per-workgroup partial words (one launch),
// then one workgroup adds them up (a second launch) -- the structure of etm_grad_sqnorm / etm_adamw_clip (optim.hip).  No atomics.
// Any 4-byte-aligned base and any n >= 1: 16-byte loads cover the aligned middle, the <= 3 words before the first 16-byte boundary and the
// <= 3 words after the last whole quad are read one by one by workgroup 0.  16 MB at config 3 (3.94 M floats): launch-latency bound.
#include "etm_common.h"

namespace {
constexpr int DG_THREADS = 256;

struct DigestAcc {
  unsigned long long sum, bad;
  unsigned mx;
};

__device__ __forceinline__ void digest_word(DigestAcc &a, unsigned long long i, unsigned b) {
  unsigned long long z = i * 0x9E3779B97F4A7C15ull + (unsigned long long)b;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  a.sum += z;
  const unsigned mag = b & 0x7fffffffu;
  if (mag >= 0x7f800000u) a.bad += 1;
  else a.mx = mag > a.mx ? mag : a.mx;
}

// sums and the maximum over the workgroup's 256 threads, valid in thread 0
__device__ __forceinline__ void digest_block_reduce(DigestAcc &a) {
  __shared__ unsigned long long s_sum[DG_THREADS], s_bad[DG_THREADS];
  __shared__ unsigned s_mx[DG_THREADS];
  const int t = threadIdx.x;
  s_sum[t] = a.sum; s_bad[t] = a.bad; s_mx[t] = a.mx;
  __syncthreads();
  for (int half = DG_THREADS / 2; half > 0; half >>= 1) {
    if (t < half) {
      s_sum[t] += s_sum[t + half];
      s_bad[t] += s_bad[t + half];
      s_mx[t] = s_mx[t + half] > s_mx[t] ? s_mx[t + half] : s_mx[t];
    }
    __syncthreads();
  }
  a.sum = s_sum[0]; a.bad = s_bad[0]; a.mx = s_mx[0];
}

// partial: [3][n_partial] words (sums, non-finite counts, maxima); workgroup w writes column w.  head = words before the aligned middle,
// n4 = quads of the middle.
__global__ __launch_bounds__(DG_THREADS) void arena_digest_partial_kernel(const unsigned *__restrict__ x, long long n, int head, long long n4,
                                                                          unsigned long long *__restrict__ partial) {
  DigestAcc a{0ull, 0ull, 0u};
  const uint4 *__restrict__ mid = (const uint4 *)(x + head);
  for (long long j = (long long)blockIdx.x * DG_THREADS + threadIdx.x; j < n4; j += (long long)gridDim.x * DG_THREADS) {
    const uint4 v = mid[j];
    const unsigned long long i = (unsigned long long)head + 4ull * (unsigned long long)j;
    digest_word(a, i, v.x);
    digest_word(a, i + 1, v.y);
    digest_word(a, i + 2, v.z);
    digest_word(a, i + 3, v.w);
  }
  if (blockIdx.x == 0) {
    const long long t = threadIdx.x;
    const long long tail0 = (long long)head + 4 * n4;       // first word after the middle
    if (t < head) digest_word(a, (unsigned long long)t, x[t]);
    if (tail0 + t < n) digest_word(a, (unsigned long long)(tail0 + t), x[tail0 + t]);      // (n - tail0 <= 3)
  }
  digest_block_reduce(a);
  if (threadIdx.x == 0) {
    const int P = gridDim.x;
    partial[blockIdx.x] = a.sum;
    partial[P + blockIdx.x] = a.bad;
    partial[2 * P + blockIdx.x] = (unsigned long long)a.mx;
  }
}

__global__ __launch_bounds__(DG_THREADS) void arena_digest_final_kernel(const unsigned long long *__restrict__ partial, int n_partial, long long n,
                                                                        unsigned long long *__restrict__ out4) {
  DigestAcc a{0ull, 0ull, 0u};
  for (int i = threadIdx.x; i < n_partial; i += DG_THREADS) {
    a.sum += partial[i];
    a.bad += partial[n_partial + i];
    const unsigned m = (unsigned)partial[2 * n_partial + i];
    a.mx = m > a.mx ? m : a.mx;
  }
  digest_block_reduce(a);
  if (threadIdx.x == 0) {
    out4[0] = a.sum;
    out4[1] = a.bad;
    out4[2] = (unsigned long long)a.mx;
    out4[3] = (unsigned long long)n;
  }
}
}  // namespace

extern "C" int etm_arena_digest(const float *x, int64_t n, uint64_t *partial, int n_partial, uint64_t *out4, void *stream) {
  (void)hipGetLastError();
  if (!x || !partial || !out4 || n <= 0 || n_partial < 1 || n_partial > 4096) return ETM_EINVAL;
  if ((uintptr_t)x % 4 != 0 || (uintptr_t)partial % 8 != 0 || (uintptr_t)out4 % 8 != 0) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  EtmProfScope prof(ETM_K_OPTIM, st);
  long long head = (long long)(((16 - (uintptr_t)x % 16) % 16) / 4);      // words before the first 16-byte boundary: 0 .. 3
  if (head > n) head = n;
  const long long n4 = (n - head) / 4;
  hipLaunchKernelGGL(arena_digest_partial_kernel, dim3((unsigned)n_partial), dim3(DG_THREADS), 0, st, (const unsigned *)x, (long long)n, (int)head,
                     n4, (unsigned long long *)partial);
  int rc = etm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(arena_digest_final_kernel, dim3(1), dim3(DG_THREADS), 0, st, (const unsigned long long *)partial, n_partial, (long long)n,
                     (unsigned long long *)out4);
  return etm_launch_status();
}
