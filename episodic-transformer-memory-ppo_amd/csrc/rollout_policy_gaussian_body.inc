// The body of rollout_policy_gaussian_kernel and rollout_policy_gaussian_means_kernel of csrc/rollout_glue.hip (included text, one
// definition): the including kernel provides the arguments, the constant MN (the means are staged too) and st_means.
  __shared__ float out_s[ETM_MAX_BOX + 1];
  const int w = blockIdx.x, A = bx.A;
  const long long t = *t_dev;
  policy_heads_lds(h, wp, bp, wv, bv, h_bias, out_s, w, A, hid);
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long row = t * stage_W + w;
    etm_sample_gaussian<MN>(out_s, log_std, bx, normals + row * A, forced ? forced + row * A : nullptr, out_s[A], row, w, actions,
                            host_actions, st_actions, st_logp, st_values, st_means);
    policy_arrive(host_actions != nullptr, t, t_dev, host_flag, sync_counter, W);
  }
