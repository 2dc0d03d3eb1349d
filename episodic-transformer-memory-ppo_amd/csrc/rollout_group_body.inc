// The body of the group step kernels of csrc/rollout_group.hip (included text, one definition): the including kernel provides the
// template parameters KM, LMAX, BOX, the launch parameters `p` and the constant MK (invalid-action masks: workgroup 0 fetches the
// workers' words next to the (step, slot) block and the masked instantiation of the shared sampler draws) and the constant MN (BOX
// only: the Gaussian draw also stages the means into p.st_means) and the constant LP (categorical only, MK or not: every column's
// log-prob of every worker's row goes to p.st_logps, stored by the sampling thread as it draws).
  constexpr int GR = 20;                                          // tail: rows of a K | V projection slice per thread and batch
  constexpr int KR = LMAX / RF_WAVES, VR = LMAX / 16;
  constexpr int NPK = (KM + 3) / 4;                               // packets per thread of a full gather: 32 * 8 CB / 2 / 512 = D / 128
  constexpr int NC = (KM + 1) / 2;                                // columns per lane of a row: D / 64
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float e_s[128];
  __shared__ long long off_s[128];
  __shared__ unsigned char mask_s[128];
  __shared__ float h2_s[RG_G * 48];
  __shared__ float out_s[RG_G * 16];
  __shared__ int dead_s;
  __shared__ long long am_s[RG_G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = p.D, Dp = D + 4, L = p.L, H = p.H, hd = D / H, W = p.W, A = p.A;
  const int CB = D / RG_WG;
  const int wg = blockIdx.x;
  float *X_s = lds, *N_s = X_s + RG_G * Dp, *A_s = N_s + RG_G * Dp, *H1_s = A_s + RG_G * Dp, *R_s = H1_s + RG_G * Dp;
  float *part_s = R_s + RG_G * Dp;                                 // RG_PART floats (>= 4 RF_T + 16: the tail's gemv partial sums)
  float *items_s = part_s + RG_PART;                               // [nb][D]: my worker's block inputs (the new memory items)
  float *t_s = items_s + RF_MAXB * RF_T, *n_s = t_s + RF_T;        // tail: projection input, norm_kv input
  float *ln_s = n_s + RF_T;                                        // [nb][4][D]: gains / biases of norm1, norm2 of every block
  const bool unit = wg < W * H;                                    // I am (worker g, head h)
  const int g = unit ? wg / H : 0, h = unit ? wg % H : 0;
  const int d0 = h * hd;                                           // my head's columns
  Grp grp;
  grp.slots = p.xbuf;
  grp.err = p.ctl + 1;
  grp.base = (int)(p.ctl[0] * 128);
  grp.me = wg;
  grp.dead_s = &dead_s;
  if (tid == 0) dead_s = 0;
  int ex = 0;
  // epilogue mapping: thread e < 8 CB owns (worker eg, column ec) of this workgroup's pieces
  const int eg = tid / CB, ec = tid - eg * CB, ecol = wg * CB + ec;
  const bool eact = tid < RG_G * CB;

  // product slices in flight: slot A (3 chunks), slot B (1 chunk); the embedding's chunk starts in A[0]
  float wfA[3][KM], wfB[1][KM], af[KM];
  const long long cblk = (long long)D * CB;                        // floats of one chunk
  const float *my = nullptr;
  wf_issue<KM>(wfA[0], p.wemb_t + (long long)wg * cblk, D, CB);
  const long long t_now = *p.t_dev;
  for (int i = tid; i < 5 * RG_G * Dp; i += RF_T) lds[i] = 0.f;    // rows >= W stay zero
  // LayerNorm gains / biases of all blocks -> LDS (requested now, stored behind the first exchange: 4 registers instead of 4 D / 64
  // per thread live through every block)
  float lnr[RF_MAXB][4];
#pragma unroll
  for (int b = 0; b < RF_MAXB; ++b) {
    const bool ok = b < p.nb && tid < D;
    lnr[b][0] = ok ? p.blk[b].g1[tid] : 0.f; lnr[b][1] = ok ? p.blk[b].b1[tid] : 0.f;
    lnr[b][2] = ok ? p.blk[b].g2[tid] : 0.f; lnr[b][3] = ok ? p.blk[b].b2[tid] : 0.f;
  }
  long long step_w = 0, slot_w = 0;
  if (unit) {
    if (p.ss) { step_w = p.ss[g]; slot_w = p.ss[W + g]; }
    else if (p.wkv) { step_w = p.step_l[g]; slot_w = p.slot_l[g]; }
  }
  // the workers' action-mask words (optional; read in place next to the (step, slot) block, possibly from pinned host memory)
  if constexpr (MK) { if (wg == 0 && tid < W) am_s[tid] = p.am[tid]; }
  const float bemb_r = eact ? p.bemb[ecol] : 0.f;
  __syncthreads();

  // ---- transformer input.  lin_hidden as partial rows (h_splits > 0): unit (g, h) adds worker g's columns of head h in slice order
  // (+ bias, ReLU: model.py:97) and the units' pieces are gathered; else every workgroup reads the [W, D] input itself.
  if (p.h_splits > 0) {
    float xin0 = 0.f;
    if (unit && tid < hd) {
      float part[RF_MAXSPLIT];
#pragma unroll
      for (int s = 0; s < RF_MAXSPLIT; ++s) part[s] = (s < p.h_splits) ? p.h_in[((long long)s * W + g) * D + d0 + tid] : 0.f;
      float v = 0.f;
#pragma unroll
      for (int s = 0; s < RF_MAXSPLIT; ++s) v += part[s];
      xin0 = fmaxf(v + p.h_bias[d0 + tid], 0.f);
    }
    if (unit) rg_publish_reg(grp, ex, xin0, hd);
    {
      const int ppp = hd >> 1;
      rg_collect<NPK>(grp, ex, W * H * ppp,
                      [&](int pk) { return rg_piece(grp, ex, pk / ppp) + 4 * (pk % ppp); },
                      [&](int pk) { const int u = pk / ppp, q = pk - u * ppp; return A_s + (u / H) * Dp + (u % H) * hd + 2 * q; });
    }
    ++ex;
  } else {
    for (int i = tid; i < W * D; i += RF_T) A_s[(i / D) * Dp + (i % D)] = p.h_in[i];
  }
  if (tid < D) {
#pragma unroll
    for (int b = 0; b < RF_MAXB; ++b)
      if (b < p.nb) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ln_s[(b * 4 + k) * D + tid] = lnr[b][k];
      }
  }
  rf_sync();
  // ---- E0: h = relu(W_emb x + b_emb) (transformer.py:232), my columns, then the full rows
  af_load<KM>(af, A_s, Dp);
  chunk_mfma<KM>(af, wfA[0], part_s, 0);
  rf_sync();
  rg_publish_reg(grp, ex, eact ? fmaxf(chunk_sum(part_s, 0, eg, ec) + bemb_r, 0.f) : 0.f, RG_G * CB);      // (published from registers, before the
  // next slices are requested: the pieces leave first)
  // the first block's slices: A = [q, Ur, Uz] (the gate's maps of x read the block input), B = [fc_out]
  my = p.blk[0].wq_t + (long long)wg * cblk;
  wf_issue<KM>(wfA[0], my, D, CB);
  my = p.blk[0].gate1.ux + (long long)wg * 2 * cblk;
  wf_issue<KM>(wfA[1], my, D, CB);
  wf_issue<KM>(wfA[2], my + cblk, D, CB);
  wf_issue<KM>(wfB[0], p.blk[0].gate1.ugx + (long long)wg * cblk, D, CB);
  auto gather_cols = [&](float *dst_s) {                            // every workgroup's [8][CB] piece -> dst_s [8][Dp]
    const int ppp = 4 * CB;
    rg_collect<NPK>(grp, ex, RG_WG * ppp,
                    [&](int pk) { return rg_piece(grp, ex, pk / ppp) + 4 * (pk % ppp); },
                    [&](int pk) { const int pw = pk / ppp, i2 = 2 * (pk - pw * ppp), gg = i2 / CB; return dst_s + gg * Dp + pw * CB + (i2 - gg * CB); });
    ++ex;
    rf_sync();
  };
  gather_cols(X_s);

  // ---- the step's window lookup (trainer.py:165-169) and a new episode's cache reset, per unit (as in rollout_fused.hip)
  if (unit) {
    if (tid < L) {
      long long idx;
      unsigned char m;
      if (p.ss) {
        const long long r = step_w < 0 ? 0 : (step_w > L - 1 ? L - 1 : step_w);
        m = p.mask_table[r * L + tid];
        idx = p.index_table[step_w * L + tid];
        if (h == 0) {
          const long long t = t_now;
          p.mask_t[(long long)g * L + tid] = m;
          p.win_t[(long long)g * L + tid] = idx;
          p.st_mask[(t * p.stage_W + g) * L + tid] = m;
          p.st_idx[(t * p.stage_W + g) * L + tid] = idx;
          if (tid == 0) {
            p.latch[g] = step_w;
            p.latch[W + g] = slot_w;
            if (g == 0 && p.t_row) *p.t_row = t;
          }
        }
      } else {
        idx = p.win[(long long)g * L + tid];
        m = p.mask[(long long)g * L + tid];
      }
      off_s[tid] = (long long)g * p.kv_w_stride + idx * p.kv_row_stride;
      mask_s[tid] = m;
    }
    if (p.ss && p.kv_init && step_w == 0) {                          // my head's K and V columns of every cache row of worker g
      const int q4 = hd >> 2;
      const long long rowf = (long long)p.nb * 2 * D;
      for (long long i = tid; i < (long long)p.T * p.nb * 2 * q4; i += RF_T) {
        const int c4 = (int)(i % q4);
        const long long rest = i / q4;
        const int kvh = (int)(rest & 1), b = (int)((rest >> 1) % p.nb);
        const long long r = (rest >> 1) / p.nb;
        const long long col = (long long)b * 2 * D + kvh * D + d0 + c4 * 4;
        *reinterpret_cast<f32x4 *>(p.kv_out + (long long)g * p.kv_w_stride + r * p.kv_row_stride + col) =
            *reinterpret_cast<const f32x4 *>(p.kv_init + r * rowf + col);
      }
      __syncthreads();
    }
  }
  rf_sync();

  // attention mappings of a unit (one head: rollout_fused.hip's with DS = hd, HS = 1)
  const int cpl = (hd + 63) / 64, lanes_used = hd / cpl;
  const int cols4 = hd >> 2, vgroups = RF_T / cols4;
  const int vg = tid / cols4, vc4 = tid - vg * cols4;

  for (int b = 0; b < p.nb; ++b) {
    const RfBlock &B = p.blk[b];
    const bool last = b + 1 == p.nb;
    if (unit) {
      if (h == 0 && tid < D) p.items[((long long)b * W + g) * D + tid] = X_s[g * Dp + tid];   // the block's input is the new memory item
      if (tid < D) items_s[b * D + tid] = X_s[g * Dp + tid];
    }
    const float *g1s = ln_s + (b * 4 + 0) * D, *b1s = g1s + D, *g2s = b1s + D, *b2s = g2s + D;    // this block's LayerNorm gains / biases
    float bfc_r = 0.f, bg1_r = 0.f, bg2_r = 0.f, fb_r = 0.f, fb_z = 0.f, fb_g = 0.f;
    if (eact) {
      bfc_r = B.bfc[ecol]; bg1_r = B.gate1.bg[ecol]; bg2_r = B.gate2.bg[ecol];
      const float *fb = B.gate1.wy + 3LL * D * D;                    // [3][D] = Wr bo, Wz bo, Wg bo behind the folded maps
      fb_r = fb[ecol]; fb_z = fb[D + ecol]; fb_g = fb[2 * D + ecol];
    }
    // ---- P1: q = Wq (pre-LN: norm1(h)) and the first gate's maps of x = h
    const float *qsrc = X_s;
    if (p.pre_ln) {
      ln_rows<NC>(X_s, N_s, D, Dp, p.eps, g1s, b1s);
      rf_sync();
      qsrc = N_s;
    }
    af_load<KM>(af, qsrc, Dp);
    chunk_mfma<KM>(af, wfA[0], part_s, 0);
    af_load<KM>(af, X_s, Dp);
    chunk_mfma<KM>(af, wfA[1], part_s, 1);
    chunk_mfma<KM>(af, wfA[2], part_s, 2);
    // K and V of my (worker, head): requested now (P1's fragments are dead), used behind the q scatter
    float kreg[KR][2];
    f32x4 vreg[VR];
    if (unit) {
      const float *kvb = p.kv + (long long)b * 2 * D;
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
    }
    rf_sync();
    float br = 0.f, bz = 0.f;
    float pv = 0.f;
    if (eact) { pv = chunk_sum(part_s, 0, eg, ec); br = chunk_sum(part_s, 1, eg, ec); bz = chunk_sum(part_s, 2, eg, ec); }
    rg_publish_reg(grp, ex, pv, RG_G * CB);
    my = B.gate1.wy + (long long)wg * 3 * cblk;
    wf_issue<KM>(wfA[0], my, D, CB);
    wf_issue<KM>(wfA[1], my + cblk, D, CB);
    wf_issue<KM>(wfA[2], my + 2 * cblk, D, CB);
    // ---- E1 (scatter): unit (g, h) takes row g of the pieces that hold its head's columns
    if (unit) {
      const int ppr = CB >> 1, per_head = hd / CB, first = d0 / CB;           // packets per piece row, pieces per head
      rg_collect<1>(grp, ex, per_head * ppr,
                    [&](int pk) { const int pw = pk / ppr, q = pk - pw * ppr; return rg_piece(grp, ex, first + pw) + 4 * ((g * CB) / 2 + q); },
                    [&](int pk) { const int pw = pk / ppr, q = pk - pw * ppr; return N_s + RG_G * Dp - RF_T + pw * CB + 2 * q; });
    }
    ++ex;
    rf_sync();
    // (q of my head sits at the end of N_s: N_s' rows are dead until the next LayerNorm)
    const float *q_s = N_s + RG_G * Dp - RF_T;
    if (unit) {
      // ---- attention of my (worker, head) over the worker's cached K | V rows (transformer.py:59-75)
#pragma unroll
      for (int j = 0; j < KR; ++j) {
        const int l = wave + j * RF_WAVES;
        if (l < L) {
          float sdot = 0.f;
          if (lane < lanes_used) {
            sdot = kreg[j][0] * q_s[lane * cpl];
            if (cpl == 2) sdot += kreg[j][1] * q_s[lane * cpl + 1];
          }
          sdot = wave_sum(sdot);
          if (lane == 0) e_s[l] = sdot;
        }
      }
      rf_sync();
      if (wave == 0) {
        float ev[2], xv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int l = lane + 64 * j;
          float en = -INFINITY;
          if (l < L) {
            en = e_s[l];
            if (mask_s[l] == 0) en = -1e20f;                       // fill BEFORE the scale (transformer.py:66, :69)
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
          if (l < L) e_s[l] = xv[j] / denom;
        }
      }
      rf_sync();
      {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < VR; ++j) {
          const int l = vg + j * vgroups;
          if (vg < vgroups && l < L) acc += e_s[l] * vreg[j];
        }
        if (vg < vgroups) *reinterpret_cast<f32x4 *>(&part_s[vg * hd + vc4 * 4]) = acc;
        rf_sync();
        float sacc = 0.f;
        if (tid < hd)
          for (int gg = 0; gg < vgroups; ++gg) sacc += part_s[gg * hd + tid];
        rg_publish_reg(grp, ex, sacc, hd);
      }
    }
    // ---- E2: the units' context columns -> R_s (full rows)
    {
      const int ppp = hd >> 1;
      rg_collect<NPK>(grp, ex, W * H * ppp,
                      [&](int pk) { return rg_piece(grp, ex, pk / ppp) + 4 * (pk % ppp); },
                      [&](int pk) { const int u = pk / ppp, q = pk - u * ppp; return R_s + (u / H) * Dp + (u % H) * hd + 2 * q; });
      ++ex;
      rf_sync();
    }
    // ---- P3: gate 1, maps of y = a = Wo ctx + bo (transformer.py:83): r = sigmoid(Wr y + Ur x), z = sigmoid(Wz y + Uz x - bg)
    // (transformer.py:294-295).  The first gate's maps of y arrive FOLDED with fc_out -- W a = (W Wo) ctx + W bo, folded in float64 once per
    // update by the caller (etm/model.py) -- so the attention output is never assembled: one product and one all-gather fewer per block
    // (a is read by nothing else).  Publish r * x.
    af_load<KM>(af, R_s, Dp);
    chunk_mfma<KM>(af, wfA[0], part_s, 0);
    chunk_mfma<KM>(af, wfA[1], part_s, 1);
    chunk_mfma<KM>(af, wfA[2], part_s, 2);
    rf_sync();
    float zz = 0.f, ag = 0.f, xm = 0.f;
    if (eact) {
      const float ar = chunk_sum(part_s, 0, eg, ec) + fb_r, az = chunk_sum(part_s, 1, eg, ec) + fb_z;
      ag = chunk_sum(part_s, 2, eg, ec) + fb_g;
      xm = X_s[eg * Dp + ecol];
      const float r = sigmoidf_(ar + br);
      zz = sigmoidf_(az + bz - bg1_r);
      pv = r * xm;
    }
    rg_publish_reg(grp, ex, pv, RG_G * CB);
    my = B.gate2.ux + (long long)wg * 2 * cblk;
    wf_issue<KM>(wfA[0], my, D, CB);
    wf_issue<KM>(wfA[1], my + cblk, D, CB);
    wf_issue<KM>(wfA[2], B.wfc_t + (long long)wg * cblk, D, CB);
    gather_cols(R_s);                                                // E4
    // ---- P4: h1 = (1 - z) x + z tanh(Wg y + Ug (r x)) (transformer.py:296-297)
    af_load<KM>(af, R_s, Dp);
    chunk_mfma<KM>(af, wfB[0], part_s, 0);
    rf_sync();
    if (eact) {
      const float hh = tanhf(ag + chunk_sum(part_s, 0, eg, ec));
      pv = (1.0f - zz) * xm + zz * hh;
    }
    rg_publish_reg(grp, ex, pv, RG_G * CB);
    wf_issue<KM>(wfB[0], B.gate2.ugx + (long long)wg * cblk, D, CB);
    gather_cols(H1_s);                                               // E5
    if (!p.pre_ln) {                                                 // post-LN: norm1 of the gate's output (transformer.py:143-149)
      ln_rows<NC>(H1_s, N_s, D, Dp, p.eps, g1s, b1s);
      rf_sync();
      for (int i = tid; i < RG_G * Dp; i += RF_T) H1_s[i] = N_s[i];
      rf_sync();
    }
    // ---- P5: the second gate's maps of x = h1, and f = relu(Wfc (pre-LN: norm2(h1)) + bfc) (transformer.py:152-160)
    const float *fsrc = H1_s;
    if (p.pre_ln) {
      ln_rows<NC>(H1_s, N_s, D, Dp, p.eps, g2s, b2s);
      rf_sync();
      fsrc = N_s;
    }
    af_load<KM>(af, H1_s, Dp);
    chunk_mfma<KM>(af, wfA[0], part_s, 0);
    chunk_mfma<KM>(af, wfA[1], part_s, 1);
    af_load<KM>(af, fsrc, Dp);
    chunk_mfma<KM>(af, wfA[2], part_s, 2);
    rf_sync();
    if (eact) {
      br = chunk_sum(part_s, 0, eg, ec);
      bz = chunk_sum(part_s, 1, eg, ec);
      pv = fmaxf(chunk_sum(part_s, 2, eg, ec) + bfc_r, 0.f);
    }
    rg_publish_reg(grp, ex, pv, RG_G * CB);
    my = B.gate2.wy + (long long)wg * 3 * cblk;
    wf_issue<KM>(wfA[0], my, D, CB);
    wf_issue<KM>(wfA[1], my + cblk, D, CB);
    wf_issue<KM>(wfA[2], my + 2 * cblk, D, CB);
    gather_cols(A_s);                                                // E6
    // ---- P6: gate 2, maps of y = f; publish r * h1
    af_load<KM>(af, A_s, Dp);
    chunk_mfma<KM>(af, wfA[0], part_s, 0);
    chunk_mfma<KM>(af, wfA[1], part_s, 1);
    chunk_mfma<KM>(af, wfA[2], part_s, 2);
    rf_sync();
    if (eact) {
      const float ar = chunk_sum(part_s, 0, eg, ec), az = chunk_sum(part_s, 1, eg, ec);
      ag = chunk_sum(part_s, 2, eg, ec);
      xm = H1_s[eg * Dp + ecol];
      const float r = sigmoidf_(ar + br);
      zz = sigmoidf_(az + bz - bg2_r);
      pv = r * xm;
    }
    rg_publish_reg(grp, ex, pv, RG_G * CB);
    if (!last) {                                                     // the next block's [q, Ur, Uz]
      my = p.blk[b + 1].wq_t + (long long)wg * cblk;
      wf_issue<KM>(wfA[0], my, D, CB);
      my = p.blk[b + 1].gate1.ux + (long long)wg * 2 * cblk;
      wf_issue<KM>(wfA[1], my, D, CB);
      wf_issue<KM>(wfA[2], my + cblk, D, CB);
    }
    gather_cols(R_s);                                                // E7
    // ---- P7: out = gate2(h1, f)
    af_load<KM>(af, R_s, Dp);
    chunk_mfma<KM>(af, wfB[0], part_s, 0);
    rf_sync();
    if (eact) {
      const float hh = tanhf(ag + chunk_sum(part_s, 0, eg, ec));
      pv = (1.0f - zz) * xm + zz * hh;
    }
    rg_publish_reg(grp, ex, pv, RG_G * CB);
    if (!last) wf_issue<KM>(wfB[0], p.blk[b + 1].gate1.ugx + (long long)wg * cblk, D, CB);
    gather_cols(X_s);                                                // E8
    if (!p.pre_ln) {                                                 // post-LN: norm2 of the block's output (transformer.py:164-170)
      ln_rows<NC>(X_s, N_s, D, Dp, p.eps, g2s, b2s);
      rf_sync();
      for (int i = tid; i < RG_G * Dp; i += RF_T) X_s[i] = N_s[i];
      rf_sync();
    }
  }

  // ---- hidden heads [lin_policy ; lin_value] + ReLU (model.py:104-107): my 2 hid / 32 columns in NCH chunks of CH <= 16, then the
  // partial dot products of the A + 1 output heads over my columns (model.py:108-110); workgroup 0 adds the pieces and samples
  const int CBH = 2 * p.hid / RG_WG, NCH = (CBH + 15) / 16, CH = CBH / NCH;
  const long long hblk = (long long)D * CH;
  const float *whm = p.wh_t + (long long)wg * NCH * hblk;            // (static slot indices: a runtime index would put the slots in scratch memory)
  wf_issue<KM>(wfA[0], whm, D, CH);
  if (NCH > 1) wf_issue<KM>(wfA[1], whm + hblk, D, CH);
  if (NCH > 2) wf_issue<KM>(wfA[2], whm + 2 * hblk, D, CH);
  af_load<KM>(af, X_s, Dp);
  chunk_mfma<KM>(af, wfA[0], part_s, 0);
  if (NCH > 1) chunk_mfma<KM>(af, wfA[1], part_s, 1);
  if (NCH > 2) chunk_mfma<KM>(af, wfA[2], part_s, 2);
  rf_sync();
  for (int i = tid; i < RG_G * CBH; i += RF_T) {
    const int gg = i / CBH, cc = i - gg * CBH, ch = cc / CH, c = cc - ch * CH;
    h2_s[gg * 48 + cc] = fmaxf(chunk_sum(part_s, ch, gg, c) + p.bh[wg * CBH + cc], 0.f);
  }
  rf_sync();
  const int AO = A + 1, npub = RG_G * AO + ((RG_G * AO) & 1);
  float hv_pub = 0.f;
  if (tid < npub) {
    float s = 0.f;
    if (tid < RG_G * AO) {
      const int gg = tid / AO, o = tid - gg * AO;
      for (int cc = 0; cc < CBH; ++cc) {
        const int col = wg * CBH + cc;                              // position among the 2 hid hidden-head outputs
        if (o < A) { if (col < p.hid) s += h2_s[gg * 48 + cc] * p.wp[(long long)o * p.hid + col]; }
        else if (col >= p.hid) s += h2_s[gg * 48 + cc] * p.wv[col - p.hid];
      }
    }
    hv_pub = s;
  }
  rg_publish_reg(grp, ex, hv_pub, npub);
  if (wg == 0) {
    const int ppp = npub >> 1;
    rg_collect<4>(grp, ex, RG_WG * ppp,
                  [&](int pk) { return rg_piece(grp, ex, pk / ppp) + 4 * (pk % ppp); },
                  [&](int pk) { const int pw = pk / ppp; return lds + pw * RG_PIECE + 2 * (pk - pw * ppp); });   // (the activation rows are dead now)
    rf_sync();
    if (tid < RG_G * AO) {
      const int o = tid % AO;
      float s = 0.f;
      for (int pw = 0; pw < RG_WG; ++pw) s += lds[pw * RG_PIECE + tid];        // workgroup order: one fixed sum
      out_s[(tid / AO) * 16 + o] = s + (o < A ? p.bp[o] : p.bv[0]);
    }
    rf_sync();
    if (tid < W) {                                                   // sampling + staging + hand-over of worker tid (as rollout_policy_kernel)
      const long long t = t_now;
      const float *lg = out_s + tid * 16;
      if constexpr (BOX) {
        // the A means; the normals / forced row [S, stage_W, A] of (t, tid); clipped hand-over
        const long long row = t * p.stage_W + tid;
        etm_sample_gaussian<MN>(lg, p.box.log_std, p.box.bx, p.box.normals + row * A, p.box.forced ? p.box.forced + row * A : nullptr, lg[A],
                                row, tid, p.box.actions, p.box.host_actions, p.box.st_actions, p.st_logp, p.st_values,
                                MN ? p.st_means : nullptr);
      } else {
        // per branch: its own logit segment, uniform and forced entry ([S, stage_W, B] tables; B = 1: [S, stage_W])
#ifndef ETM_LOGPS_TAIL          // LP: the columns are stored by the sampling thread as it draws (the measured faster of the two placements)
        etm_sample_branches<MK, LP>(lg, p.br, t * p.stage_W + tid, tid, p.uniforms, p.forced, p.actions, p.host_actions, p.st_actions,
                                    p.st_logp, am_s + tid, LP ? p.st_logps : nullptr, A);
#else                           // (diagnostic build) LP: the branches' lse go to the dead hidden-head rows (h2_s [worker][16]) for the stores behind the hand-over
        etm_sample_branches<MK, LP>(lg, p.br, t * p.stage_W + tid, tid, p.uniforms, p.forced, p.actions, p.host_actions, p.st_actions,
                                    p.st_logp, am_s + tid, nullptr, A, LP ? h2_s + tid * 16 : nullptr);
#endif
        p.st_values[t * p.stage_W + tid] = lg[A];
      }
      if (BOX ? p.box.host_actions != nullptr : p.host_actions != nullptr) __threadfence_system();
      else __threadfence();
    }
    __syncthreads();                                                 // every sampler's stores are complete (and fenced)
    if (tid == 0) {
      // every workgroup has published its last piece, i.e. has read the launch counter and the step counter: both may move on
      p.ctl[0] += 1;
      *p.t_dev = t_now + 1;
      if (p.host_flag) {
        __threadfence_system();
        __hip_atomic_store(p.host_flag, t_now + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
#ifdef ETM_LOGPS_TAIL
    // (diagnostic build, the other store placement: not faster on the replayed step graph, profiles/r18/exact_kl.txt)
    // LP: every column's log-prob of every worker's row, behind the hand-over (they need only be there when the launch ends): one
    // (worker, column) per thread from the logits still in out_s and the branch's lse the sampler left in h2_s -- at the taken
    // action the expression and the operands of the staged log-prob, so its bits; a masked-out column is -inf
    if constexpr (LP) {
      if (tid < W * A) {
        const int gw = tid / A, j = tid - gw * A;
        int b = 0, off = p.br.size[0];
        while (j >= off) off += p.br.size[++b];
        float l = out_s[gw * 16 + j];
        if constexpr (MK) { if (!(((unsigned long long)am_s[gw] >> j) & 1ull)) l = -INFINITY; }
        p.st_logps[(t_now * p.stage_W + gw) * A + j] = l - h2_s[gw * 16 + b];
      }
    }
#endif
  }
  ++ex;
  // ---- tail (units): bank[slot, step, b] = item_b (head 0's workgroup) and my head's K | V columns of the new cache row
  // (transformer.py:236-237 for one new row; rollout_fused.hip's tail with P = H, DS = hd)
  if (p.wkv && unit) {
    f32x4 wr[GR];
    rf_sync();
    const float pos_r = (p.pos && tid < D) ? p.pos[step_w * D + tid] : 0.f;
    const int KS = 2 * hd;
    const float *wkv_m = p.wkv + (long long)h * D * KS;             // [nb][H][D][2 hd]
    const long long wkv_b = (long long)H * D * KS;
    gemv_issue<GR>(wr, wkv_m, D, 0, KS, 0, KS, 0);
    for (int b = 0; b < p.nb; ++b) {
      float xin = 0.f;
      if (tid < D) {
        const float it = items_s[b * D + tid];
        if (h == 0) p.bank[slot_w * p.bank_slot_stride + step_w * p.bank_row_stride + (long long)b * p.bank_block_stride + tid] = it;
        xin = it + pos_r;
        (p.blk[b].nkv_g ? n_s : t_s)[tid] = xin;
      }
      rf_sync();
      if (p.blk[b].nkv_g) {                                          // pre-LN: the cache holds projections of norm_kv(memory) (transformer.py:128-131)
        float mk, rk;
        row_stats(n_s, D, p.eps, mk, rk);
        if (tid < D) t_s[tid] = (xin - mk) * rk * p.blk[b].nkv_g[tid] + p.blk[b].nkv_b[tid];
        rf_sync();
      }
      const float *wb = wkv_m + b * wkv_b;
      gemv_finish<GR>(wr, wb, D, t_s, part_s, 0, D, KS, 0, KS);
      if (b + 1 < p.nb) gemv_issue<GR>(wr, wb + wkv_b, D, 0, KS, 0, KS, 0);
      rf_sync();
      if (tid < KS) {
        const int col = (tid < hd) ? d0 + tid : D + d0 + (tid - hd);
        p.kv_out[(long long)g * p.kv_w_stride + step_w * p.kv_row_stride + (long long)b * 2 * D + col] = gemv_sum(part_s, KS, tid);
      }
      rf_sync();
    }
  }
