// The body of rollout_sample_gaussian_kernel and rollout_sample_gaussian_means_kernel of csrc/rollout_glue.hip (included text, one
// definition): the including kernel provides the arguments, the constant MN (the means are staged too) and st_means.
  const long long t = *t_dev;
  const int A = bx.A;
  for (int w = threadIdx.x; w < W; w += 1024) {
    const long long row = t * W + w;
    etm_sample_gaussian<MN>(mean + (long long)w * A, log_std, bx, normals + row * A, forced ? forced + row * A : nullptr, value[w], row, w,
                            actions, nullptr, st_actions, st_logp, st_values, st_means);
  }
  __syncthreads();
  if (threadIdx.x == 0) *t_dev = t + 1;
