// The body of the per-worker step kernels of csrc/rollout_fused.hip (included text, one definition): the including kernel provides the
// template parameters GR, LMAX, GEN, BOX, the launch parameters `p` and the constant MK (invalid-action masks: the sampler's word is
// fetched with the step's uniforms and the masked instantiation of the shared sampler draws) and the constant MN (BOX only: the
// Gaussian draw also stages the means into p.st_means) and the constant LP (categorical only, MK or not: every column's log-prob of
// the row goes to p.st_logps, stored by the sampling thread as it draws).
  constexpr int KR = LMAX / RF_WAVES;                             // window rows per wave (energies)
  constexpr int VR = LMAX / 16;                                   // window rows per thread (context): >= 16 row groups (D / P <= 128)
  __shared__ __attribute__((aligned(16))) float x_s[RF_T];        // current hidden state h_b (full row, every member)
  __shared__ __attribute__((aligned(16))) float y_s[RF_T];        // q (mine) / ctx (mine) / x (full) / hidden heads (mine)
  __shared__ __attribute__((aligned(16))) float part_s[4 * RF_T + 16];
  __shared__ float t_s[RF_T];                                     // LayerNorm inputs / pieces to publish
  __shared__ float e_s[8 * 128];
  __shared__ long long off_s[128];
  __shared__ unsigned char mask_s[128];
  __shared__ float out_s[64];
  __shared__ float items_s[RF_MAXB * RF_T];                       // every block's input (the new memory items), for the tail
  __shared__ float a_s[RF_T], h1_s[RF_T], g_s[RF_T], n_s[RF_T], pub_s[RF_T];   // gated / pre-LN layouts: full rows between the sub-layers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = p.D, L = p.L, H = p.H, hd = D / H, P = p.P;
  // block -> (worker, member).  Placement is a speed matter only (workgroup b is observed on XCD b % 8; every exchange is
  // system-scope, i.e. correct under any placement):
  //   0  the members of a team share b % 8: one XCD hosts whole teams -- and therefore ALL weight slices (7 MB at D = 384: more than
  //      its 4 MB L2, so every step re-streams them from the Infinity Cache);
  //   1  XCD x hosts member x % P of 8 / P-th of the workers: it only ever touches that member's slices (a quarter of every
  //      matrix at P = 4), which stay L2-resident from step to step next to the workers' K | V columns of that member.
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  int me, w;
  if (p.map_mode == 0) { me = idx % P; w = (idx / P) * 8 + xcd; }
  else { me = xcd % P; w = idx * (8 / P) + xcd / P; }
  if (w >= p.W) return;
  const int DS = D / P, d0 = me * DS;                              // my columns of every D-wide product
  const int HS = H / P;                                            // my heads: me * HS ...
  const int OUTH = 2 * p.hid, OS = OUTH / P, o0 = me * OS;         // my columns of the hidden heads
  // Column-split matrices arrive MEMBER-BLOCKED: [P][K][columns of the member], so a member's slice of a product is one contiguous
  // run (147 KB at D = 384) instead of 384-byte pieces at the row stride of the whole matrix -- the K-split fc_out product, whose
  // slice always was contiguous, was the fastest product of the timeline.
  const long long mcol = (long long)me * D * DS;                   // my block of a [D, D] matrix split by columns
  const long long mhead = (long long)me * D * OS;                  // my block of the [D, 2 hid] hidden heads
  Team team;
  team.P = P; team.me = me; team.D = D;
  team.slots = p.xbuf + (long long)w * p.n_slots * P * 2 * D;
  team.err = p.ctl + 1;
  team.base = p.ctl[0] * 64;                                       // launch counter (bumped by the last workgroup of a launch)
  int ex = 0;

  RF_STAMP(0);
  f32x4 wr[GR];                                                    // the product slice in flight
  gemv_issue<GR>(wr, p.wemb_t + mcol, D, 0, DS, 0, DS, 0);
  // inputs of the sampling at the very end (thread 0 of member 0 samples; threads b < B fetch branch b's entries now)
  const long long t_now = *p.t_dev;                                 // (uniform) step counter of the rollout
  __shared__ int forced_s[ETM_MAX_BRANCHES];
  __shared__ float u_s[ETM_MAX_BRANCHES];
  __shared__ long long am_s;                                       // MK: the worker's action-mask word
  __shared__ float box_s[3 * ETM_MAX_BOX];                         // BOX: normals | forced | log-std of (t, w), dimension a at [a]
  if constexpr (BOX) {
    if (me == 0 && tid < p.box.bx.A) {
      const long long i = (t_now * p.stage_W + w) * p.box.bx.A + tid;
      box_s[tid] = p.box.normals[i];
      box_s[ETM_MAX_BOX + tid] = p.box.forced ? p.box.forced[i] : NAN;
      box_s[2 * ETM_MAX_BOX + tid] = p.box.log_std[tid];
    }
  } else {
    if (me == 0 && tid < p.br.n) {
      const long long i = (t_now * p.stage_W + w) * p.br.n + tid;
      forced_s[tid] = p.forced ? (int)p.forced[i] : -1;
      u_s[tid] = p.uniforms[i];
      // the worker's action-mask word (optional; read in place, possibly from pinned host memory: hidden under the transformer)
      if constexpr (MK) { if (tid == 0) am_s = p.am[w]; }
    }
  }
  if (tid < D) {
    float v;
    if (p.h_splits > 0) {                                          // lin_hidden arrives as K-slice sums: add them in slice order
      float part[RF_MAXSPLIT];
#pragma unroll
      for (int s = 0; s < RF_MAXSPLIT; ++s) part[s] = (s < p.h_splits) ? p.h_in[((long long)s * p.W + w) * D + tid] : 0.f;
      v = 0.f;
#pragma unroll
      for (int s = 0; s < RF_MAXSPLIT; ++s) v += part[s];
      v = fmaxf(v + p.h_bias[tid], 0.f);
    } else {
      v = p.h_in[(long long)w * D + tid];
    }
    x_s[tid] = v;
  }
  long long step_w = 0, slot_w = 0;
  if (p.ss) { step_w = p.ss[w]; slot_w = p.ss[p.W + w]; }   // read in place (possibly from pinned host memory)
  else if (p.wkv) { step_w = p.step_l[w]; slot_w = p.slot_l[w]; }
  const float bemb_r = (tid < DS) ? p.bemb[d0 + tid] : 0.f;
  rf_sync();
  // E0: linear_embedding + ReLU, my columns; collect the full row
  gemv_finish<GR>(wr, p.wemb_t + mcol, D, x_s, part_s, 0, D, DS, 0, DS);
  gemv_issue<GR>(wr, p.blk[0].wq_t + mcol, D, 0, DS, 0, DS, 0);
  rf_sync();
  if (tid < DS) t_s[tid] = fmaxf(gemv_sum(part_s, DS, tid) + bemb_r, 0.f);
  rf_sync();
  RF_STAMP(1);
  if (P > 1) {
    team_publish(team, ex, t_s, DS);
    if (tid < DS) x_s[d0 + tid] = t_s[tid];
    for (int m = 0; m < P; ++m)
      if (m != me) team_collect(team, ex, m, x_s + m * DS, DS, 64 * (m - (m > me)));   // one wave per partner
    ++ex;
  } else {
    if (tid < D) x_s[tid] = t_s[tid];
  }
  rf_sync();
  RF_STAMP(2);
  // The step's window lookup (and a new episode's cache reset) is done HERE, after the first exchange: the (step, slot) words were
  // requested at kernel start (possibly from pinned host memory, ~2 us) and are consumed only now.
  if (tid < L) {                                                   // the window rows of this worker in the K | V cache (block 0's offsets)
    long long idx;
    unsigned char m;
    if (p.ss) {                                                    // the lookup of trainer.py:165-169 (rollout_window_kernel's job)
      const long long r = step_w < 0 ? 0 : (step_w > L - 1 ? L - 1 : step_w);
      m = p.mask_table[r * L + tid];
      idx = p.index_table[step_w * L + tid];
      if (me == 0) {                                               // ... with its staging: the step's buffer rows, the group's current rows
        const long long t = t_now;
        p.mask_t[(long long)w * L + tid] = m;
        p.win_t[(long long)w * L + tid] = idx;
        p.st_mask[(t * p.stage_W + w) * L + tid] = m;
        p.st_idx[(t * p.stage_W + w) * L + tid] = idx;
        if (tid == 0) {
          p.latch[w] = step_w;
          p.latch[p.W + w] = slot_w;
          if (w == 0 && p.t_row) *p.t_row = t;
        }
      }
    } else {
      idx = p.win[(long long)w * L + tid];
      m = p.mask[(long long)w * L + tid];
    }
    off_s[tid] = (long long)w * p.kv_w_stride + idx * p.kv_row_stride;
    mask_s[tid] = m;
  }
  if (p.ss && p.kv_init && step_w == 0) {
    // a new episode: its cache rows hold the projection of an empty memory (trainer.py:208-213 in cache form).  Every member
    // resets exactly the K and V columns it reads, so no member depends on another one's stores.
    const int q4 = DS >> 2;
    const long long rowf = (long long)p.nb * 2 * D;                // floats per cache row of kv_init
    for (long long i = tid; i < (long long)p.T * p.nb * 2 * q4; i += RF_T) {
      const int c4 = (int)(i % q4);
      const long long rest = i / q4;
      const int kvh = (int)(rest & 1), b = (int)((rest >> 1) % p.nb);
      const long long r = (rest >> 1) / p.nb;
      const long long col = (long long)b * 2 * D + kvh * D + d0 + c4 * 4;
      *reinterpret_cast<f32x4 *>(p.kv_out + (long long)w * p.kv_w_stride + r * p.kv_row_stride + col) =
          *reinterpret_cast<const f32x4 *>(p.kv_init + r * rowf + col);
    }
    __syncthreads();                                               // stores complete and visible to the whole workgroup
  }
  rf_sync();

  // mappings of the attention phases
  const int cpl = (DS + 63) / 64;                                  // energies: my columns per lane (DS = 96 -> 2 on 48 lanes)
  const int lanes_used = DS / cpl, lph = lanes_used / HS;          // lanes per head
  const int cols4 = DS >> 2, vgroups = RF_T / cols4;               // context: thread = (row group, 4 columns)
  const int vg = tid / cols4, vc4 = tid - vg * cols4;

  for (int b = 0; b < p.nb; ++b) {
    const RfBlock &B = p.blk[b];
    const float *kvb = p.kv + (long long)b * 2 * D;                // this block's K | V columns of a cache row
    if (me == 0 && tid < D) p.items[((long long)b * p.W + w) * D + tid] = x_s[tid];   // the block's input is the new memory item
    if (tid < D) items_s[b * D + tid] = x_s[tid];
    // K and V of my columns: in flight now, used two and three phases later
    float kreg[KR][2];
    f32x4 vreg[VR];
#pragma unroll
    for (int j = 0; j < KR; ++j) {
      const int l = wave + j * RF_WAVES;
      kreg[j][0] = 0.f; kreg[j][1] = 0.f;
      if (l < L && lane < lanes_used) {
        const float *krow = kvb + off_s[l] + d0 + lane * cpl;
        kreg[j][0] = krow[0];
        if (cpl == 2) kreg[j][1] = krow[1];
      }
    }
#pragma unroll
    for (int j = 0; j < VR; ++j) {
      const int l = vg + j * vgroups;
      vreg[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (vg < vgroups && l < L) vreg[j] = *reinterpret_cast<const f32x4 *>(kvb + off_s[l] + D + d0 + vc4 * 4);
    }
    // this block's biases and gains of my rows
    float bo_r = 0.f, g1_r = 0.f, b1_r = 0.f, g2_r = 0.f, b2_r = 0.f, bfc_r = 0.f;
    if (tid < D) { bo_r = B.bo[tid]; g1_r = B.g1[tid]; b1_r = B.b1[tid]; g2_r = B.g2[tid]; b2_r = B.b2[tid]; }
    if (tid < DS) bfc_r = B.bfc[d0 + tid];
    // q (my columns = my heads); pre-LN: from LayerNorm1(h) (transformer.py:128-131)
    const float *qsrc = x_s;
    if (GEN && p.pre_ln) {
      float mq, rq;
      row_stats(x_s, D, p.eps, mq, rq);
      if (tid < D) n_s[tid] = (x_s[tid] - mq) * rq * g1_r + b1_r;
      rf_sync();
      qsrc = n_s;
    }
    gemv_finish<GR>(wr, B.wq_t + mcol, D, qsrc, part_s, 0, D, DS, 0, DS);
    gemv_issue<GR>(wr, B.wo_t, D, d0, D, 0, D, 0);
    rf_sync();
    if (tid < DS) y_s[tid] = gemv_sum(part_s, DS, tid);
    rf_sync();
    RF_STAMP(3 + 8 * b);
    // energies of my heads: one wave per window row (rows wave, wave + 8, ...), lanes over my DS columns
#pragma unroll
    for (int j = 0; j < KR; ++j) {
      const int l = wave + j * RF_WAVES;
      if (l < L) {                                                 // wave-uniform
        float sdot = 0.f;
        if (lane < lanes_used) {
          sdot = kreg[j][0] * y_s[lane * cpl];
          if (cpl == 2) sdot += kreg[j][1] * y_s[lane * cpl + 1];
        }
        if (HS == 1) {
          sdot = wave_sum(sdot);
          if (lane == 0) e_s[l] = sdot;
        } else {                                                   // lanes_used == 64, lph a power of two
          for (int o = 1; o < lph; o <<= 1) sdot += __shfl_xor(sdot, o, 64);
          if ((lane & (lph - 1)) == 0) e_s[(lane / lph) * 128 + l] = sdot;
        }
      }
    }
    rf_sync();
    RF_STAMP(4 + 8 * b);
    if (wave < HS) {                                              // masked softmax of my head `wave` over the window
      float ev[2], xv[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int l = lane + 64 * j;
        float en = -INFINITY;
        if (l < L) {
          en = e_s[wave * 128 + l];
          if (mask_s[l] == 0) en = -1e20f;                        // fill BEFORE the scale (transformer.py:66, :69)
          en = en / p.sqrt_d;
        }
        ev[j] = en;
      }
      const float m = wave_max(fmaxf(ev[0], ev[1]));
#pragma unroll
      for (int j = 0; j < 2; ++j) xv[j] = (lane + 64 * j < L) ? expf(ev[j] - m) : 0.f;
      const float denom = wave_sum(xv[0] + xv[1]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int l = lane + 64 * j;
        if (l < L) e_s[wave * 128 + l] = xv[j] / denom;
      }
    }
    rf_sync();
    // ctx of my columns: the row groups split the window rows
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float *arow = e_s + ((vc4 * 4) / hd) * 128;          // hd % 4 == 0: the 4 columns share a head
#pragma unroll
      for (int j = 0; j < VR; ++j) {
        const int l = vg + j * vgroups;
        if (vg < vgroups && l < L) acc += arow[l] * vreg[j];
      }
      if (vg < vgroups) *reinterpret_cast<f32x4 *>(&part_s[vg * DS + vc4 * 4]) = acc;
      rf_sync();
      if (tid < DS) {
        float sacc = 0.f;
        for (int gg = 0; gg < vgroups; ++gg) sacc += part_s[gg * DS + tid];
        y_s[d0 + tid] = sacc;                                     // ctx, at its position in the full row
      }
      rf_sync();
    }
    RF_STAMP(5 + 8 * b);
    if constexpr (GEN) {
      // ---- general layout (transformer.py:117-172): attention -> gate1 or residual -> (post: norm1) -> (pre: norm2) -> fc ->
      // gate2 or residual -> (post: norm2).  Same machinery: every product's slice is requested when the previous product has
      // consumed the registers; full rows are assembled by exchanges.
      struct Nxt { const float *w; int k0, OUT, o0, OUTS; };
      const bool merge_gate = p.merge_gate != 0;                   // etm_rollout_trxl_gate_merged(D, H): the caller packed the gates accordingly
      const Nxt after_block = (b + 1 < p.nb) ? Nxt{p.blk[b + 1].wq_t + mcol, 0, DS, 0, DS} : Nxt{p.wh_t + mhead, 0, OS, 0, OS};
      auto slice_prod = [&](const float *wt, const float *src_s, const Nxt &nx) -> float {   // a contiguous [D, DS] block
        gemv_finish<GR>(wr, wt, D, src_s, part_s, 0, D, DS, 0, DS);
        gemv_issue<GR>(wr, nx.w, D, nx.k0, nx.OUT, nx.o0, nx.OUTS, 0);
        rf_sync();
        const float r = (tid < DS) ? gemv_sum(part_s, DS, tid) : 0.f;
        rf_sync();
        return r;
      };
      auto col_prod = [&](const float *wt, const float *src_s, const Nxt &nx) -> float {     // my DS columns of wt^T src (member-blocked wt)
        gemv_finish<GR>(wr, wt + mcol, D, src_s, part_s, 0, D, DS, 0, DS);
        gemv_issue<GR>(wr, nx.w, D, nx.k0, nx.OUT, nx.o0, nx.OUTS, 0);
        rf_sync();
        const float r = (tid < DS) ? gemv_sum(part_s, DS, tid) : 0.f;
        rf_sync();
        return r;
      };
      auto gather_full = [&](float mine, float *dst_s) {           // every member's DS values -> the full row in dst_s
        if (tid < DS) pub_s[tid] = mine;
        rf_sync();
        if (P > 1) {
          team_publish(team, ex, pub_s, DS);
          if (tid < DS) dst_s[d0 + tid] = pub_s[tid];
          for (int m = 0; m < P; ++m)
            if (m != me) team_collect(team, ex, m, dst_s + m * DS, DS, 64 * (m - (m > me)));
          ++ex;
        } else {
          if (tid < D) dst_s[tid] = pub_s[tid];
        }
        rf_sync();
      };
      auto gate = [&](const RfGate &G, const float *xs, const float *ys, float *dst_s, const Nxt &nx) {   // dst = GRUGate(x, y)
        // the three maps of y are ONE product over my 3 DS columns of [Wr | Wz | Wg]^T, the two maps of x one over 2 DS columns
        // of [Ur | Uz]^T: two phases instead of five (a phase costs a round trip whatever its size)
        // -- when the merged product still fits two register batches (small D: phases are pure latency); at D = 384 a merged
        // product is three batches, two of them exposed round trips, and five pre-requested slices are faster (measured:
        // config 2 step graph 209 -> 183 us merged, config 5 312 -> 356 us merged).
        float ar = 0.f, az = 0.f, ag = 0.f, br = 0.f, bz = 0.f;
        // my block of [Wr | Wz | Wg]^T / [Ur | Uz]^T: merged form [P][D][j DS] (one product over j DS columns), else [P][j][D][DS]
        // (j contiguous [D, DS] blocks)
        const float *wy = G.wy + (long long)me * 3 * D * DS, *ux = G.ux + (long long)me * 2 * D * DS;
        const long long blk = (long long)D * DS;
        if (merge_gate) {
          gemv_finish<GR>(wr, wy, D, ys, part_s, 0, D, 3 * DS, 0, 3 * DS);
          gemv_issue<GR>(wr, ux, D, 0, 2 * DS, 0, 2 * DS, 0);
          rf_sync();
          if (tid < DS) { ar = gemv_sum(part_s, 3 * DS, tid); az = gemv_sum(part_s, 3 * DS, DS + tid); ag = gemv_sum(part_s, 3 * DS, 2 * DS + tid); }
          rf_sync();
          gemv_finish<GR>(wr, ux, D, xs, part_s, 0, D, 2 * DS, 0, 2 * DS);
          gemv_issue<GR>(wr, G.ugx + mcol, D, 0, DS, 0, DS, 0);
          rf_sync();
          if (tid < DS) { br = gemv_sum(part_s, 2 * DS, tid); bz = gemv_sum(part_s, 2 * DS, DS + tid); }
          rf_sync();
        } else {
          ar = slice_prod(wy, ys, Nxt{wy + blk, 0, DS, 0, DS});
          az = slice_prod(wy + blk, ys, Nxt{wy + 2 * blk, 0, DS, 0, DS});
          ag = slice_prod(wy + 2 * blk, ys, Nxt{ux, 0, DS, 0, DS});
          br = slice_prod(ux, xs, Nxt{ux + blk, 0, DS, 0, DS});
          bz = slice_prod(ux + blk, xs, Nxt{G.ugx + mcol, 0, DS, 0, DS});
        }
        float xm = 0.f, r = 0.f, z = 0.f;
        if (tid < DS) {
          xm = xs[d0 + tid];
          r = 1.0f / (1.0f + expf(-(ar + br)));
          z = 1.0f / (1.0f + expf(-(az + bz - G.bg[d0 + tid])));
        }
        gather_full(r * xm, g_s);                                  // r * x, full row, for Ug
        const float c = col_prod(G.ugx, g_s, nx);
        const float hh = tanhf(ag + c);
        gather_full((1.0f - z) * xm + z * hh, dst_s);
      };
      // fc_out as a K-split (as below): partial rows summed in member order, + bias
      gemv_finish<GR>(wr, B.wo_t, D, y_s, part_s, d0, d0 + DS, D, 0, D);
      if (p.gtrxl) {
        const int ow = merge_gate ? 3 * DS : DS;
        gemv_issue<GR>(wr, B.gate1.wy + (long long)me * 3 * D * DS, D, 0, ow, 0, ow, 0);
      } else {
        gemv_issue<GR>(wr, B.wfc_t + mcol, D, 0, DS, 0, DS, 0);
      }
      rf_sync();
      if (tid < D) t_s[tid] = gemv_sum(part_s, D, tid);
      rf_sync();
      float av = 0.f;
      if (P > 1) {
        team_publish(team, ex, t_s, D);
        for (int m = 0; m < P; ++m)
          if (m != me) team_collect(team, ex, m, part_s + m * D, D, 0);
        rf_sync();
        if (tid < D)
          for (int m = 0; m < P; ++m) av += (m == me) ? t_s[tid] : part_s[m * D + tid];
        ++ex;
      } else if (tid < D) {
        av = t_s[tid];
      }
      av += bo_r;
      rf_sync();
      float mean2, rstd2;
      // h1 = gate1(h, attention) or attention + h; post-LN: norm1 of it
      if (p.gtrxl) {
        if (tid < D) a_s[tid] = av;
        rf_sync();
        gate(B.gate1, x_s, a_s, p.pre_ln ? h1_s : t_s, Nxt{B.wfc_t + mcol, 0, DS, 0, DS});
      } else {
        if (tid < D) (p.pre_ln ? h1_s : t_s)[tid] = av + x_s[tid];
        rf_sync();
      }
      if (!p.pre_ln) {
        row_stats(t_s, D, p.eps, mean2, rstd2);
        if (tid < D) h1_s[tid] = (t_s[tid] - mean2) * rstd2 * g1_r + b1_r;
        rf_sync();
      }
      const float *fsrc = h1_s;
      if (p.pre_ln) {                                              // pre-LN: the projection reads norm2(h1)
        row_stats(h1_s, D, p.eps, mean2, rstd2);
        if (tid < D) n_s[tid] = (h1_s[tid] - mean2) * rstd2 * g2_r + b2_r;
        rf_sync();
        fsrc = n_s;
      }
      const int ow2 = merge_gate ? 3 * DS : DS;
      const float f = fmaxf(col_prod(B.wfc_t, fsrc, p.gtrxl ? Nxt{B.gate2.wy + (long long)me * 3 * D * DS, 0, ow2, 0, ow2} : after_block) + bfc_r, 0.f);
      gather_full(f, a_s);                                         // fc output, full row
      if (p.gtrxl) {
        gate(B.gate2, h1_s, a_s, p.pre_ln ? x_s : t_s, after_block);
      } else {
        if (tid < D) (p.pre_ln ? x_s : t_s)[tid] = a_s[tid] + h1_s[tid];
        rf_sync();
      }
      if (!p.pre_ln) {
        row_stats(t_s, D, p.eps, mean2, rstd2);
        if (tid < D) x_s[tid] = (t_s[tid] - mean2) * rstd2 * g2_r + b2_r;
        rf_sync();
      }
    } else {
    // Ea: fc_out as a K-split: my rows of Wo^T (my ctx columns) x all D outputs -> partial row; the members' partial rows are
    // summed in member order; x = LayerNorm1(sum + bo + h)
    gemv_finish<GR>(wr, B.wo_t, D, y_s, part_s, d0, d0 + DS, D, 0, D);
    gemv_issue<GR>(wr, B.wfc_t + mcol, D, 0, DS, 0, DS, 0);
    rf_sync();
    float v = 0.f, mean, rstd;
    if (tid < D) t_s[tid] = gemv_sum(part_s, D, tid);
    rf_sync();
    RF_STAMP(6 + 8 * b);
    if (P > 1) {
      team_publish(team, ex, t_s, D);
      for (int m = 0; m < P; ++m)                                 // the partners' partial rows -> part_s[m][D] (part_s is free now)
        if (m != me) team_collect(team, ex, m, part_s + m * D, D, 0);
      rf_sync();
      if (tid < D) {
        for (int m = 0; m < P; ++m) v += (m == me) ? t_s[tid] : part_s[m * D + tid];   // member order: the same sum in every member
        v += bo_r + x_s[tid];
      }
      ++ex;
      rf_sync();
      if (tid < D) t_s[tid] = v;
    } else {
      if (tid < D) { v = t_s[tid] + bo_r + x_s[tid]; }
      rf_sync();
      if (tid < D) t_s[tid] = v;
    }
    rf_sync();
    RF_STAMP(7 + 8 * b);
    row_stats(t_s, D, p.eps, mean, rstd);
    if (tid < D) y_s[tid] = (v - mean) * rstd * g1_r + b1_r;      // x (full row)
    rf_sync();
    RF_STAMP(8 + 8 * b);
    // Eb: f = relu(Wfc x + bfc), my columns; h = LayerNorm2(f + x)
    gemv_finish<GR>(wr, B.wfc_t + mcol, D, y_s, part_s, 0, D, DS, 0, DS);
    if (b + 1 < p.nb) gemv_issue<GR>(wr, p.blk[b + 1].wq_t + mcol, D, 0, DS, 0, DS, 0);
    else gemv_issue<GR>(wr, p.wh_t + mhead, D, 0, OS, 0, OS, 0);
    rf_sync();
    if (tid < DS) t_s[tid] = fmaxf(gemv_sum(part_s, DS, tid) + bfc_r, 0.f);
    rf_sync();
    RF_STAMP(9 + 8 * b);
    if (P > 1) {
      team_publish(team, ex, t_s, DS);
      if (tid < DS) part_s[d0 + tid] = t_s[tid];                  // f (full row) -> part_s[0 .. D)
      for (int m = 0; m < P; ++m)
        if (m != me) team_collect(team, ex, m, part_s + m * DS, DS, 64 * (m - (m > me)));
      ++ex;
    } else {
      if (tid < D) part_s[tid] = t_s[tid];
    }
    rf_sync();
    v = 0.f;
    if (tid < D) v = part_s[tid] + y_s[tid];
    rf_sync();
    if (tid < D) t_s[tid] = v;
    rf_sync();
    row_stats(t_s, D, p.eps, mean, rstd);
    if (tid < D) x_s[tid] = (v - mean) * rstd * g2_r + b2_r;
    rf_sync();
    RF_STAMP(10 + 8 * b);
    }
  }

  // Ez: hidden heads [lin_policy ; lin_value] + ReLU (model.py:104-107), my columns of the 2 hid outputs, then the partial dot
  // products of the A + 1 output heads over my columns (model.py:108-110)
  const float bh_r = (tid < OS) ? p.bh[o0 + tid] : 0.f;
  float hw[4] = {0.f, 0.f, 0.f, 0.f};                              // my columns of output head `wave` (the first A + 1 <= 8 outputs)
  {
    const int o = wave;
    if (o < p.A + 1) {
      const int hoff = (o < p.A) ? 0 : p.hid;
      const float *wt = (o < p.A) ? p.wp + (long long)o * p.hid : p.wv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j, col = o0 + c - hoff;
        if (c < OS && col >= 0 && col < p.hid) hw[j] = wt[col];
      }
    }
  }
  const float bout_r = (me == 0 && tid < p.A + 1) ? (tid < p.A ? p.bp[tid] : p.bv[0]) : 0.f;
  gemv_finish<GR>(wr, p.wh_t + mhead, D, x_s, part_s, 0, D, OS, 0, OS);
  rf_sync();
  if (tid < OS) y_s[tid] = fmaxf(gemv_sum(part_s, OS, tid) + bh_r, 0.f);
  rf_sync();
  for (int o = wave; o < p.A + 1; o += RF_WAVES) {                // one wave per output
    float s = 0.f;
    if (o < RF_WAVES) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int c = lane + 64 * j; if (c < OS) s += y_s[c] * hw[j]; }
    } else {
      const int hoff = (o < p.A) ? 0 : p.hid;                     // the output reads hidden columns [hoff, hoff + hid)
      const float *wt = (o < p.A) ? p.wp + (long long)o * p.hid : p.wv;
      for (int c = lane; c < OS; c += 64) {
        const int col = o0 + c - hoff;                            // position inside the output's hidden half
        if (col >= 0 && col < p.hid) s += y_s[c] * wt[col];
      }
    }
    s = wave_sum(s);
    if (lane == 0) t_s[o] = s;
  }
  rf_sync();
  RF_STAMP(40);
  if (P > 1) {
    if (me != 0) team_publish(team, ex, t_s, p.A + 1);
    if (me == 0) {
      for (int m = 1; m < P; ++m) team_collect(team, ex, m, part_s + m * 64, p.A + 1, 64 * (m - 1));
      rf_sync();
      if (tid < p.A + 1) {
        float s = t_s[tid];
        for (int m = 1; m < P; ++m) s += part_s[m * 64 + tid];
        out_s[tid] = s + bout_r;
      }
    }
    ++ex;
  } else {
    if (tid < p.A + 1) out_s[tid] = t_s[tid] + bout_r;
  }
  rf_sync();
  RF_STAMP(41);
  if (tid == 0) {
    if (me == 0) {                                                // sampling + staging + hand-over: as rollout_policy_kernel
      const long long t = t_now;
      const int A = p.A, B = p.br.n;
      const long long row = t * p.stage_W + w;
      if constexpr (BOX) {                                          // the A means, the step's normals / forced row, clipped hand-over
        etm_sample_gaussian<MN>(out_s, box_s + 2 * ETM_MAX_BOX, p.box.bx, box_s, p.box.forced ? box_s + ETM_MAX_BOX : nullptr, out_s[A], row,
                                w, p.box.actions, p.box.host_actions, p.box.st_actions, p.st_logp, p.st_values, MN ? p.st_means : nullptr);
      } else {
        int off = 0;
        for (int b = 0; b < B; ++b) {                               // per branch: its own logit segment, uniform and forced entry
          const int Ab = p.br.size[b];
          float lp;
          int a;
          if constexpr (LP) {
            unsigned long long mb = 0ull;
            if constexpr (MK) mb = (unsigned long long)am_s >> off;
#ifndef ETM_LOGPS_TAIL          // the columns are stored by the sampling thread as it draws (the measured faster of the two placements)
            a = etm_sample_branch<MK, true>(out_s + off, Ab, u_s[b], forced_s[b], &lp, mb, p.st_logps + row * A + off);
#else                           // (diagnostic build: stored behind the hand-over; the branch's lse takes the place of its uniform)
            a = etm_sample_branch<MK, true>(out_s + off, Ab, u_s[b], forced_s[b], &lp, mb, nullptr, u_s + b);
#endif
          }
          else if constexpr (MK) a = etm_sample_branch<true>(out_s + off, Ab, u_s[b], forced_s[b], &lp, (unsigned long long)am_s >> off);
          else a = etm_sample_branch(out_s + off, Ab, u_s[b], forced_s[b], &lp);
          p.actions[(long long)w * B + b] = a;
          if (p.host_actions) p.host_actions[(long long)w * B + b] = a;
          p.st_actions[row * B + b] = a;
          p.st_logp[row * B + b] = lp;
          off += Ab;
        }
        p.st_values[row] = out_s[A];
      }
      RF_STAMP(42);
      // this worker's rows are visible before the arrival below -- system scope when the action went to pinned host memory: the
      // host reads it as soon as it sees the flag that the LAST sampler stores, so every sampler's store must have completed at
      // system scope before its arrival (an agent-scope fence does not promise that for host memory)
      if (BOX ? p.box.host_actions != nullptr : p.host_actions != nullptr) __threadfence_system();
      else __threadfence();
      // the last SAMPLER of the step: every team has finished its exchanges, i.e. every workgroup of the launch has read the
      // launch counter and (the samplers) the step counter -- both may move on, and the host may have its actions
      if (atomicAdd(p.sync_counter, 1) == p.W - 1) {
        *p.sync_counter = 0;
        p.ctl[0] += 1;                                            // launch counter: the next launch's sequence numbers
        *p.t_dev = t + 1;
        if (p.host_flag) {
          __threadfence_system();
          __hip_atomic_store(p.host_flag, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  }
#ifdef ETM_LOGPS_TAIL
  // (diagnostic build, the other store placement: measured slower on the replayed step graph, profiles/r18/exact_kl.txt)
  // LP: every column's log-prob of this worker's row, behind the hand-over (they need only be there when the launch ends): one column
  // per thread from the logits still in out_s and the branch's lse that the sampler left in u_s -- at the taken action the expression
  // and the operands of the staged log-prob, so its bits; a masked-out column is -inf
  if constexpr (LP) {
    if (me == 0) {                                                  // (uniform per workgroup)
      rf_sync();
      if (tid < p.A) {
        int b = 0, off = p.br.size[0];
        while (tid >= off) off += p.br.size[++b];
        float l = out_s[tid];
        if constexpr (MK) { if (!(((unsigned long long)am_s >> tid) & 1ull)) l = -INFINITY; }
        p.st_logps[(t_now * p.stage_W + w) * p.A + tid] = l - u_s[b];
      }
    }
  }
#endif
  // ---- tail, after the hand-over (the host is stepping the environments now): bank[slot, step, b] = item_b (member 0) and
  // cache[w, step, b] = (item_b + pos[step]) [Wk ; Wv]^T, the D / P columns of K and of V that I read (transformer.py:236-237 applied to one new row;
  // the rows of this step are not part of any window of this launch that is still being read: a member gets here only after
  // its last exchange, i.e. after every partner's last attention phase).
  if (p.wkv) {
    const float pos_r = (p.pos && tid < D) ? p.pos[step_w * D + tid] : 0.f;   // positional row of this step, my element
    const int OUTK = 2 * D, KS = OUTK / P;
    const float *wkv_m = p.wkv + (long long)me * D * KS;            // [nb][P][D][KS]: my contiguous block of block 0 = [my K columns | my V columns]
    const long long wkv_b = (long long)P * D * KS;
    gemv_issue<GR>(wr, wkv_m, D, 0, KS, 0, KS, 0);
    for (int b = 0; b < p.nb; ++b) {
      float xin = 0.f;
      if (tid < D) {
        const float it = items_s[b * D + tid];
        if (me == 0) p.bank[slot_w * p.bank_slot_stride + step_w * p.bank_row_stride + (long long)b * p.bank_block_stride + tid] = it;
        xin = it + pos_r;
        ((GEN && p.blk[b].nkv_g) ? n_s : t_s)[tid] = xin;
      }
      rf_sync();
      if (GEN && p.blk[b].nkv_g) {                                 // pre-LN: the cache holds projections of norm_kv(memory) (transformer.py:128-131)
        float mk, rk;
        row_stats(n_s, D, p.eps, mk, rk);
        if (tid < D) t_s[tid] = (xin - mk) * rk * p.blk[b].nkv_g[tid] + p.blk[b].nkv_b[tid];
        rf_sync();
      }
      const float *wb = wkv_m + b * wkv_b;
      gemv_finish<GR>(wr, wb, D, t_s, part_s, 0, D, KS, 0, KS);
      if (b + 1 < p.nb) gemv_issue<GR>(wr, wb + wkv_b, D, 0, KS, 0, KS, 0);
      rf_sync();
      // my block of wkv holds MY K columns followed by MY V columns (the D / P columns this member reads in the attention
      // phases): the cache columns a member reads are only ever written by that member -- no data flows between members through
      // plain memory, so nothing depends on where the members of a team are placed
      if (tid < KS) {
        const int col = (tid < DS) ? d0 + tid : D + d0 + (tid - DS);
        p.kv_out[(long long)w * p.kv_w_stride + step_w * p.kv_row_stride + (long long)b * OUTK + col] = gemv_sum(part_s, KS, tid);
      }
      rf_sync();
    }
  }
