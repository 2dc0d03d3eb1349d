"""-m gpu: every rollout-step path, sample by sample, against a float64 evaluation of the model (oracle/ref_model.py).

One sampled rollout per case (Synthetic env, vector observations).  Each sample (w, t) is checked LOCALLY: the inputs are the
device's own history (observation, episode bank, window indices and mask), the expected values are ``ref_model.actor_critic``
run on the device in float64 with the trainer's fp32 weights cast to float64.  Compared per sample: the value, the log-prob at
the sampled action, the new memory item (the block inputs) and the sampled action itself (float64 inverse CDF of the uniform
draw).  After the rollout: the K | V cache of every worker's current episode, the cache's initial rows (``kv_init``), the
bootstrap value and the advantages.  The rollout's uniforms are crafted (``_sample_training_data(uniforms=...)``): random draws
plus 0 and the largest fp32 uniform 1 - 2^-24, and in half the cases the last action has probability zero (its policy row is
zero, its bias -200) -- no kernel may ever sample it.

The matrix covers every instantiation of the per-worker step kernel (rollout_trxl_kernel<GR, LMAX, GEN>), of the group kernel
(rollout_group_kernel<KM, LMAX>) and the multi-launch paths; ``test_step_matrix_covers_every_instantiation`` restates the
dispatch rules of csrc/rollout_fused.hip / csrc/rollout_group.hip and checks that.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Bounds (relative, see _rel): about 4x the worst error measured over the matrix on the MI355X (second column), and inside
# the caps 1e-5 max(1, |ref|) for values / log-probs, 1e-5 max|ref row| for items / K|V rows, 2e-5 max(1, |ref|) for advantages.
BOUNDS = {
    "value": 3.5e-6,         # 9.5e-7  multi_no_fused_block
    "logp": 1.1e-6,          # 2.8e-7  g4_64
    "item": 2.8e-6,          # 7.2e-7  g12_128_two_groups
    "kv": 2.3e-6,            # 6.0e-7  ln_none
    "kv_init": 4.8e-6,       # 1.2e-6  w32_*
    "last_value": 5.0e-6,    # 1.25e-6 w32_128_post
    "adv": 5.6e-6,           # 1.4e-6  w32_128_post
}
BOUNDARY_GAP = 1e-5          # a random draw this close to a float64 CDF boundary may take either neighbouring action
U_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))      # largest fp32 uniform, 1 - 2^-24


# ------------------------------------------------------------------ dispatch rules (python restatement of the host code)
def _team(H):
    """etm_rollout_trxl_team: workgroups per worker."""
    return 4 if H % 4 == 0 else (2 if H % 2 == 0 else 1)


def _rf_rows(D, H):
    """rf_rows (csrc/rollout_fused.hip): register rows per product slice, 20 or 32."""
    P = _team(H)
    DS = D // P
    kq, ko = 512 // (DS // 4), 512 // (D // 4)
    return 20 if -(-D // kq) <= 20 and -(-DS // ko) <= 20 else 32


def _worker_inst(D, H, L, pre_ln, gtrxl):
    return ("worker", _rf_rows(D, H), 64 if L <= 64 else 128, bool(pre_ln or gtrxl))


def _group_inst(D, L):
    return ("group", 4, 64) if D == 128 else ("group", 12, 64 if L <= 64 else 128)


ALL_INSTANTIATIONS = ({("worker", gr, lm, gen) for gr in (20, 32) for lm in (64, 128) for gen in (False, True)}
                      | {("group", 4, 64), ("group", 12, 64), ("group", 12, 128)})


def _case(name, D, H, L, nb, A, W, ln="post", gtrxl=False, gtrxl_bias=1.0, pos="relative", path="worker", zero_last=False, **over):
    return dict(name=name, D=D, H=H, L=L, nb=nb, A=A, W=W, ln=ln, gtrxl=gtrxl, gtrxl_bias=gtrxl_bias, pos=pos, path=path,
                zero_last=zero_last, over=over)


# path: "worker" = per-worker step kernel, "group" = group kernel, "policy" = multi-launch with rollout_policy,
# "sample" = window kernels over the bank + rollout_sample
CASES = [
    _case("w20_64_post", 384, 4, 64, 2, 3, 16),
    _case("w20_128_post", 384, 4, 128, 2, 3, 9, zero_last=True),
    _case("w32_64_post", 512, 4, 64, 2, 3, 8, zero_last=True),
    _case("w32_128_post", 512, 4, 128, 2, 5, 8),
    _case("w20_64_gtrxl", 384, 4, 64, 2, 3, 8, ln="pre", gtrxl=True, rollout_group_kernel=False, zero_last=True),
    _case("w20_128_gtrxl", 384, 4, 128, 2, 3, 8, ln="pre", gtrxl=True, rollout_group_kernel=False),
    _case("w32_64_pre", 512, 4, 64, 2, 3, 8, ln="pre"),
    _case("w32_128_gtrxl", 512, 4, 128, 2, 3, 8, ln="pre", gtrxl=True, gtrxl_bias=2.0, zero_last=True),
    _case("team1_h1", 128, 1, 32, 2, 4, 8, zero_last=True),
    _case("team2_h2", 256, 2, 32, 2, 4, 8),
    _case("team4_h8", 256, 8, 48, 2, 5, 8, ln="pre", zero_last=True),
    _case("a63", 128, 2, 32, 2, 63, 8, zero_last=True),
    _case("pos_learned", 128, 2, 32, 2, 3, 8, pos="learned"),
    _case("pos_none", 128, 2, 32, 2, 3, 8, pos="none", zero_last=True),
    _case("ln_none", 128, 2, 32, 2, 3, 8, ln="none", path="policy", zero_last=True),
    _case("g4_64", 128, 1, 32, 2, 4, 8, ln="pre", gtrxl=True, gtrxl_bias=0.0, path="group", zero_last=True),
    _case("g12_64", 384, 4, 64, 2, 3, 6, ln="post", gtrxl=True, gtrxl_bias=2.0, path="group"),
    _case("g12_128_two_groups", 384, 4, 128, 4, 3, 16, ln="pre", gtrxl=True, path="group", rollout_groups=2, zero_last=True),
    _case("g12_128_ragged_a14", 384, 4, 128, 2, 14, 3, ln="pre", gtrxl=True, path="group"),
    _case("multi_no_fused_block", 384, 4, 64, 2, 3, 8, path="policy", fused_rollout_block=False, zero_last=True),
    _case("multi_no_fused_tail", 384, 4, 64, 2, 3, 8, ln="pre", fused_rollout_tail=False),
    _case("multi_no_kv_cache", 128, 2, 32, 2, 3, 8, path="sample", kv_cache_rollout=False, zero_last=True),
    _case("group_eager", 384, 4, 64, 2, 3, 8, ln="pre", gtrxl=True, path="group", hip_graph_rollout=False),
]


def _instantiation(c):
    if c["path"] == "worker":
        return _worker_inst(c["D"], c["H"], c["L"], c["ln"] == "pre", c["gtrxl"])
    if c["path"] == "group":
        return _group_inst(c["D"], c["L"])
    return ("multi", c["path"])


def _config(c):
    """worker_steps L + 12, episodes of at most L + 5 steps, p_done 0.5 / L: about 60 % of the episodes live past L steps, so
    windows slide past L, and episodes end (early or at L + 5) and restart inside the rollout."""
    L = c["L"]
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[7], num_actions=c["A"], max_episode_steps=L + 5, seed=3, p_done=0.5 / L, pool=4),
               gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=c["W"], worker_steps=L + 12, n_mini_batch=1,
               value_loss_coefficient=0.5, hidden_layer_size=c["D"], max_grad_norm=0.5, rollout_groups=1, rollout_min_group_size=2,
               transformer=dict(num_blocks=c["nb"], embed_dim=c["D"], num_heads=c["H"], memory_length=L, positional_encoding=c["pos"],
                                layer_norm=c["ln"], gtrxl=c["gtrxl"], gtrxl_bias=c["gtrxl_bias"] if c["gtrxl"] else 0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    cfg.update(json.loads(json.dumps(c["over"])))
    return cfg


def _uniforms(W, S, seed):
    """[W, S] draws: random, with 0 and the largest fp32 uniform mixed in; second value: which entries are crafted."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((W, S), generator=g)
    crafted = torch.zeros((W, S), dtype=torch.bool)
    ww, tt = torch.meshgrid(torch.arange(W), torch.arange(S), indexing="ij")
    top = (ww + tt) % 3 == 0
    u[top] = U_MAX
    u[(ww + 2 * tt) % 11 == 5] = 0.0
    crafted |= top | ((ww + 2 * tt) % 11 == 5)
    return u, crafted


def _rel(dev, ref, floor_one=True):
    """|dev - ref| / max(1, |ref|) elementwise (floor_one) or / max|ref| over the last dimension (rows)."""
    dev, ref = dev.double(), ref.double()
    if floor_one:
        return (dev - ref).abs() / ref.abs().clamp(min=1.0)
    scale = ref.abs().amax(dim=-1, keepdim=True).clamp(min=1e-30)
    return (dev - ref).abs() / scale


def _norm_kv(sd, blocks, x, eps):
    """x [..., nb, D] -> norm_kv of every block (pre-LN), else x."""
    outs = []
    for i in range(blocks):
        p = f"transformer.transformer_blocks.{i}.norm_kv"
        xi = x[..., i, :]
        outs.append(F.layer_norm(xi, (xi.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps) if p + ".weight" in sd else xi)
    return torch.stack(outs, dim=-2)


def _kv_ref(sd, nb, items_pos, eps):
    """float64 K | V rows of (items + pos): [..., nb, D] -> [..., nb, 2D]."""
    x = _norm_kv(sd, nb, items_pos, eps)
    outs = []
    for i in range(nb):
        p = f"transformer.transformer_blocks.{i}.attention"
        w = torch.cat((sd[p + ".keys.weight"], sd[p + ".values.weight"]), dim=0)
        outs.append(x[..., i, :] @ w.t())
    return torch.stack(outs, dim=-2)


def _inverse_cdf(p64, u):
    """float64 inverse CDF: (smallest j with u < C_j, or the last positive action; distance of u to the nearest boundary C_j, j < A-1)."""
    C = torch.cumsum(p64, dim=-1)
    A = p64.shape[-1]
    a = (C <= u[:, None]).sum(dim=-1)
    pos = p64 > 1e-30
    last_pos = A - 1 - torch.flip(pos, dims=[-1]).int().argmax(dim=-1)
    a = torch.where(a >= A, last_pos, a)
    gap = (C[:, : A - 1] - u[:, None]).abs().amin(dim=-1) if A > 1 else torch.full_like(u, float("inf"))
    return a, gap


def _run_case(c):
    from etm import ops
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    cfg = _config(c)
    torch.manual_seed(29)
    tr = PPOTrainer(cfg, run_id="f64step", device=dev, tensorboard=False)
    try:
        W, S, L, T, nb, D, A = c["W"], cfg["worker_steps"], c["L"], tr.max_episode_length, c["nb"], c["D"], c["A"]
        with torch.no_grad():
            for prm in tr.model.parameters():          # non-trivial LayerNorm gains / biases / gate biases
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
            if c["zero_last"]:                         # the last action gets probability zero
                tr.model.policy_branches[0].weight[-1].zero_()
                tr.model.policy_branches[0].bias[-1] = -200.0
        u, crafted = _uniforms(W, S, seed=len(c["name"]))
        s0 = tr.worker_current_episode_step.copy()
        tr._sample_training_data(uniforms=u)
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()

        # ---- launch health: the intended path, no team time-out
        use_graph = bool(cfg.get("hip_graph_rollout", True))
        groups = tr._groups if use_graph else [tr._group_all]
        path = c["path"]
        assert tr._use_kv_cache == (path != "sample"), (c["name"], "K | V cache")
        if path != "sample":         # (without the cache the trainer never reaches the step kernels, whatever the model packed)
            assert (tr.model._rf is not None) == (path in ("worker", "group")), (c["name"], "fused step kernel")
        assert all((g.rf_scratch is not None) == (path in ("worker", "group")) for g in groups), (c["name"], "step kernel")
        if path in ("worker", "group"):
            assert all(g.group_kernel == (path == "group") for g in groups), (c["name"], "group kernel")
            assert all(g.tail_in_kernel == cfg.get("fused_rollout_tail", True) for g in groups), (c["name"], "tail")
        if "rollout_groups" in c["over"]:
            assert len(tr._groups) == c["over"]["rollout_groups"]
        for g in tr._groups + [tr._group_all]:
            if g.rf_scratch is not None:
                assert int(ops.rollout_trxl_error(g.rf_scratch).item()) == 0, (c["name"], "step kernel error word")

        b = tr.buffer
        dones = torch.from_numpy(b.dones.copy())
        rewards = torch.from_numpy(b.rewards.copy()).double()
        # ---- episode step of every sample, tracked on the host
        steps = torch.zeros((W, S), dtype=torch.int64)
        s = torch.from_numpy(s0.astype(np.int64))
        for t in range(S):
            steps[:, t] = s
            s = torch.where(dones[:, t], torch.zeros_like(s), s + 1)
        assert torch.equal(s, torch.from_numpy(tr.worker_current_episode_step.astype(np.int64)))
        assert bool((steps < T).all())
        mask_table, index_table = rm.window_tables(L, T)
        assert torch.equal(b.memory_indices.cpu(), index_table[steps]), c["name"]
        assert torch.equal(b.memory_mask.cpu(), mask_table[steps.clamp(max=L - 1)].bool()), c["name"]
        slots = b.memory_index.cpu()
        assert torch.equal(slots[:, 1:] != slots[:, :-1], dones[:, :-1]), (c["name"], "a new episode slot exactly after every done")

        sd = {k: v.detach().double() for k, v in tr.model.state_dict().items()}
        pos = tr.model.transformer._pos()
        pos64 = pos.detach().double() if pos is not None else None
        tcfg = dict(cfg["transformer"], positional_encoding="none")     # the positions are added here, from the model's own table
        ocfg = dict(cfg, transformer=tcfg)
        eps = tr.model.transformer.transformer_blocks[0].norm1.eps

        def forward64(obs, slot, rows, step, mask, pidx):
            """float64 actor_critic on windows bank[slot, rows] with rows >= step zeroed (not written yet) + pos[pidx]."""
            win = b.memories[slot[:, None], rows].double()
            win = win * (rows < step[:, None]).to(win.dtype)[:, :, None, None]
            if pos64 is not None:
                win = win + pos64[pidx].unsqueeze(2)
            return rm.actor_critic(sd, ocfg, obs.double(), win, mask, pidx, T)

        # ---- per sample
        N = W * S
        flat = lambda x: x.reshape(N, *x.shape[2:]).to(dev)
        slot_f, idx_f, mask_f = flat(b.memory_index), flat(b.memory_indices), flat(b.memory_mask)
        step_f, obs_f = flat(steps), flat(b.obs)
        act_f, lp_f, v_f = flat(b.actions)[:, 0], flat(b.log_probs)[:, 0], flat(b.values)
        u_f, crafted_f = flat(tr._uniforms.t().cpu()), flat(crafted)
        worst = {}
        upd = lambda k, e: worst.__setitem__(k, max(worst.get(k, 0.0), float(e.max()) if e.numel() else 0.0))
        skipped = n_random = 0
        with torch.no_grad():
            for lo in range(0, N, 256):
                sl = slice(lo, min(N, lo + 256))
                logits, value, item = forward64(obs_f[sl], slot_f[sl], idx_f[sl], step_f[sl], mask_f[sl], idx_f[sl])
                lsm = torch.log_softmax(logits[0], dim=-1)
                a = act_f[sl]
                assert bool(((a >= 0) & (a < A)).all()), c["name"]
                upd("value", _rel(v_f[sl], value))
                upd("logp", _rel(lp_f[sl], lsm.gather(1, a[:, None])[:, 0]))
                upd("item", _rel(b.memories[slot_f[sl], step_f[sl]], item, floor_one=False))
                p64 = lsm.exp()
                pa = p64.gather(1, a[:, None])[:, 0]
                assert float(pa.min()) >= 1e-30, (c["name"], "sampled an action of float64 probability", float(pa.min()),
                                                  int(a[pa.argmin()]), float(u_f[sl][pa.argmin()]))
                a_ref, gap = _inverse_cdf(p64, u_f[sl].double())
                near = gap < BOUNDARY_GAP
                bad = (a != a_ref) & ~near
                assert not bool(bad.any()), (c["name"], "inverse CDF", int(bad.sum()), a[bad][:8].tolist(), a_ref[bad][:8].tolist(),
                                             u_f[sl][bad][:8].tolist())
                rnd = ~crafted_f[sl]
                skipped += int((near & rnd).sum())
                n_random += int(rnd.sum())
        assert skipped <= 2 + 1e-3 * n_random, (c["name"], "draws within 1e-5 of a CDF boundary", skipped, n_random)

        # ---- after the rollout: K | V cache of the current episodes, its initial rows
        if cfg.get("kv_cache_rollout", True):
            zeros = torch.zeros((T, nb, D), dtype=torch.float64, device=dev)
            init_ref = _kv_ref(sd, nb, zeros + (pos64[:, None, :] if pos64 is not None else 0), eps)
            upd("kv_init", _rel(tr._kv_init, init_ref, floor_one=False))
            for w in range(W):
                s_end = int(tr.worker_current_episode_step[w])
                if s_end == 0:
                    continue
                items = b.bank[int(tr.worker_episode_slot[w]), :s_end].double()
                if pos64 is not None:
                    items = items + pos64[:s_end, None, :]
                upd("kv", _rel(tr._kv_cache[w, :s_end], _kv_ref(sd, nb, items, eps), floor_one=False))

        # ---- bootstrap value (upstream's window rule, Q5) and GAE in float64
        with torch.no_grad():
            s_last = torch.from_numpy(tr.worker_current_episode_step.astype(np.int64)).to(dev)
            rows = torch.clamp(s_last - L, min=0)[:, None] + torch.arange(L, device=dev)[None, :]
            slot = torch.from_numpy(tr.worker_episode_slot.astype(np.int64)).to(dev)
            mask = mask_table.to(dev)[torch.clamp(s_last, max=L - 1)].bool()
            _, lv64, _ = forward64(tr._lv.obs, slot, rows, s_last, mask, b.memory_indices[:, -1])
            upd("last_value", _rel(tr._lv.out, lv64))
            vals = b.values.double()
            alive = (~dones).to(dev).double()
            rw = rewards.to(dev)
            adv = torch.zeros_like(vals)
            nv, na = lv64, torch.zeros_like(lv64)
            for t in range(S - 1, -1, -1):
                nv, na = nv * alive[:, t], na * alive[:, t]
                na = rw[:, t] + cfg["gamma"] * nv - vals[:, t] + cfg["gamma"] * cfg["lamda"] * na
                adv[:, t] = na
                nv = vals[:, t]
            upd("adv", _rel(b.advantages, adv))
        n_eps = int(dones.sum())
        print(f"[f64] {c['name']:<22} {str(_instantiation(c)):<28} samples {N:5d} episodes ended {n_eps:3d} skipped {skipped} "
              + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        for k, v in worst.items():
            assert v <= BOUNDS[k], (c["name"], k, v, BOUNDS[k])
        assert n_eps > 0 and bool((steps >= L).any()), (c["name"], "windows must slide past L and episodes restart")
    finally:
        tr.close()


def test_step_matrix_covers_every_instantiation():
    """The matrix reaches all eight per-worker and all three group instantiations, and every case is a supported shape of its path."""
    from etm import lib as etm_lib
    lib = etm_lib.load()
    insts = {_instantiation(c) for c in CASES}
    assert ALL_INSTANTIATIONS <= insts, sorted(map(str, ALL_INSTANTIATIONS - insts))
    assert {("multi", "policy"), ("multi", "sample")} <= insts
    for c in CASES:
        if c["path"] == "worker":
            assert lib.etm_rollout_trxl_supported(c["D"], c["H"], c["L"], c["D"], c["A"], c["nb"]), c["name"]
        if c["path"] == "group":
            w = min(c["W"], 8)
            assert lib.etm_rollout_trxl_group_supported(c["D"], c["H"], c["L"], c["D"], c["A"], c["nb"], w, 1), c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_rollout_step_vs_float64(case):
    _run_case(case)


# ------------------------------------------------------------------ sampling contract of the sampling kernels
def _crafted_rows():
    """Logit rows by action count: trailing / leading -200, all equal, one dominant, random (with a trailing -200)."""
    g = torch.Generator().manual_seed(11)
    rows = {}
    for A in (1, 2, 3, 4, 15, 63):
        r = [torch.zeros(A), torch.full((A,), 3.5)]
        if A > 1:
            dom = torch.zeros(A)
            dom[A // 2] = 30.0
            r.append(dom)
            for _ in range(24):
                x = torch.randn(A, generator=g) * 3
                x[-1] = -200.0
                r.append(x)
            x = torch.randn(A, generator=g) * 3
            x[0] = -200.0
            r.append(x)
        if A == 3:
            r += [torch.tensor([10.0, 10.0, -200.0]), torch.tensor([-200.0, 10.0, 10.0])]
        rows[A] = torch.stack(r)
    return rows


def _probe_uniforms(lg):
    """0, the largest fp32 uniform, and each fp32 running CDF sum (as the kernels form it) and one ulp either side."""
    lg32 = lg.numpy().astype(np.float32)
    mx = lg32.max()
    se = np.float32(0)
    for x in lg32:
        se = np.float32(se + np.exp(np.float32(x - mx), dtype=np.float32))
    lse = np.float32(mx + np.log(se, dtype=np.float32))
    us, c = [0.0, U_MAX], np.float32(0)
    for x in lg32:
        c = np.float32(c + np.exp(np.float32(x - lse), dtype=np.float32))
        for v in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(2))):
            if 0 <= v < 1:
                us.append(float(v))
    return us


def _check_draws(lg, u, a, logp, what):
    """Inverse-CDF contract on (logits [N, A], uniforms [N]) -> the kernel's actions and log-probs."""
    lg64 = lg.double()
    lsm = torch.log_softmax(lg64, dim=-1)
    p64 = lsm.exp()
    A = lg.shape[1]
    C = torch.cumsum(p64, dim=-1)
    Cm = torch.cat((torch.zeros_like(C[:, :1]), C[:, :-1]), dim=-1)
    u64 = u.double()
    pa = p64.gather(1, a[:, None])[:, 0]
    assert float(pa.min()) >= 1e-30, (what, "zero-probability action", lg[pa.argmin()].tolist(), float(u[pa.argmin()]), int(a[pa.argmin()]))
    # the action's interval [C_{a-1}, C_a) holds u up to rounding of the fp32 sums (a few ulp); past the last positive
    # action's lower boundary the action IS that action
    tol = 1e-6
    lo_ok = Cm.gather(1, a[:, None])[:, 0] - tol <= u64
    hi_ok = (u64 < C.gather(1, a[:, None])[:, 0] + tol)
    pos = p64 > 1e-30
    last_pos = A - 1 - torch.flip(pos, dims=[-1]).int().argmax(dim=-1)
    past = u64 > Cm.gather(1, last_pos[:, None])[:, 0] + tol
    hi_ok |= past & (a == last_pos)
    bad = ~(lo_ok & hi_ok) | (past & (a != last_pos))
    assert not bool(bad.any()), (what, lg[bad][:3].tolist(), u[bad][:3].tolist(), a[bad][:3].tolist())
    err = _rel(logp, lsm.gather(1, a[:, None])[:, 0])
    assert float(err.max()) <= 1e-5 * 4, (what, "log-prob", float(err.max()))


def test_sampling_kernels_inverse_cdf_contract():
    """ops.rollout_sample and ops.rollout_policy on crafted logits and uniforms: the smallest j with u < C_j, the last action of
    positive probability for draws at or past the fp32 total (never a zero-probability one), float64 log-probs, and actions that
    never decrease as u grows."""
    from etm import ops
    dev = torch.device("cuda", 0)
    hid = 64
    for A, rows in _crafted_rows().items():
        lgs, us, rid = [], [], []
        for i, r in enumerate(rows):
            for u in _probe_uniforms(r):
                lgs.append(r)
                us.append(u)
                rid.append(i)
        lg = torch.stack(lgs)
        u = torch.tensor(us, dtype=torch.float32)
        W = lg.shape[0]
        for kernel in ("sample", "policy"):
            t_dev = torch.zeros((), dtype=torch.int64, device=dev)
            acts = torch.zeros((W, 1), dtype=torch.int64, device=dev)
            st_a = torch.zeros((1, W, 1), dtype=torch.int64, device=dev)
            st_lp = torch.zeros((1, W, 1), dtype=torch.float32, device=dev)
            st_v = torch.zeros((1, W), dtype=torch.float32, device=dev)
            uni = u[None, :].to(dev).contiguous()
            if kernel == "sample":
                value = torch.randn(W, device=dev)
                ops.rollout_sample(lg.to(dev), value, uni, None, t_dev, acts, st_a, st_lp, st_v)
                v_ref = value.double()
            else:
                ph, vh = torch.nn.Linear(hid, A).to(dev), torch.nn.Linear(hid, 1).to(dev)
                with torch.no_grad():
                    ph.weight.zero_()                  # logits = bias exactly
                    h2 = torch.rand((W, 2 * hid), device=dev)
                    v_ref = (h2[:, hid:].double() @ vh.weight.double().t())[:, 0] + vh.bias.double()
                with torch.no_grad():
                    for i in range(rows.shape[0]):     # one launch per logits row: the policy bias IS the row
                        sel = torch.tensor([k for k in range(W) if rid[k] == i], device=dev)
                        n = sel.numel()
                        ph.bias.copy_(rows[i].to(dev))
                        tt = torch.zeros((), dtype=torch.int64, device=dev)
                        sa = torch.zeros((1, n, 1), dtype=torch.int64, device=dev)
                        sl = torch.zeros((1, n, 1), dtype=torch.float32, device=dev)
                        sv = torch.zeros((1, n), dtype=torch.float32, device=dev)
                        ops.rollout_policy(h2[sel].contiguous(), ph, vh, uni[:, sel].contiguous(), None, tt,
                                           torch.zeros((n, 1), dtype=torch.int64, device=dev), sa, sl, sv)
                        assert int(tt.item()) == 1, (kernel, "step counter")
                        st_a[0, sel], st_lp[0, sel], st_v[0, sel] = sa[0], sl[0], sv[0]
                t_dev.fill_(1)
            torch.cuda.synchronize()
            assert int(t_dev.item()) == 1, (kernel, "step counter")
            a = st_a[0, :, 0].cpu()
            _check_draws(lg, u, a, st_lp[0, :, 0].cpu(), (kernel, A))
            assert float(_rel(st_v[0].cpu(), v_ref.cpu()).max()) <= 1e-5, (kernel, "value")
            if kernel == "sample":
                assert torch.equal(acts[:, 0].cpu(), a)
            for i in range(rows.shape[0]):                       # monotone in u
                sel = [k for k in range(W) if rid[k] == i]
                order = sorted(sel, key=lambda k: us[k])
                seq = a[order]
                assert bool((seq[1:] >= seq[:-1]).all()), (kernel, A, rows[i].tolist(), [us[k] for k in order], seq.tolist())
