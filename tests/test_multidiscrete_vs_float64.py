"""-m gpu: MultiDiscrete action spaces (several action branches) on every fused path, against float64.

* Rollout, per sample (the pattern of test_rollout_step_vs_float64.py): for branch shapes (3, 3) and (2, 4, 3) on the per-worker
  step kernel (post-LN, pre-LN, gated, D = 512), the group kernel, ``rollout_policy`` (``fused_rollout_block: false``) and the
  multi-launch ``rollout_sample`` (eager and captured), with one and two worker groups.  Compared with ``ref_model.actor_critic``
  in float64: the value, every branch's log-prob, every branch's action as the float64 inverse CDF of that branch's uniform, the new
  memory items and the K | V rows.  In every branch the last action has probability zero and is never sampled (the uniforms include
  1 - 2^-24); forced actions, different per branch, are honoured.
* Discrete(n) and nvec = [n] give bit-identical rollouts and updates.
* ``ops.heads_ppo_loss`` with branches against ``ref_algo.ppo_loss`` in float64 (loss, statistics, every gradient), and the per-branch
  ``ops.ppo_loss`` for a shape beyond the fused kernel's predicate.
* One update of ``synthetic_multidiscrete`` (small), eager and captured: the first minibatch step's gradient arena against float64
  autograd through ``ref_model.actor_critic`` + ``ref_algo.ppo_loss``.
"""
import gc
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Bounds (relative, see _rel): about 4x the worst error measured on the MI355X, inside the caps of test_rollout_step_vs_float64.py
# (worst measured: value 9.3e-7 w_forced_243, logp 2.2e-7 w_d512_243, item 4.2e-7 g_*, kv 3.5e-7 policy_243, kv_init 1.03e-6 w_d512_243)
BOUNDS = {"value": 3.7e-6, "logp": 9.0e-7, "item": 1.7e-6, "kv": 1.4e-6, "kv_init": 4.1e-6}
BOUNDARY_GAP = 1e-5
U_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))      # largest fp32 uniform, 1 - 2^-24


@pytest.fixture(autouse=True)
def _collect_between_tests():
    """Every test builds trainers that capture HIP graphs: collect the previous test's garbage first (see _release)."""
    gc.collect()
    yield
    gc.collect()


def _release(tr):
    """Close a trainer and collect its captured graphs NOW: a graph object freed by the garbage collector while the next trainer
    captures its step graph would be destroyed inside that capture (not permitted on the runtime: the process aborts)."""
    tr.close()
    del tr
    gc.collect()
    torch.cuda.synchronize()


def _rel(dev, ref, floor_one=True):
    dev, ref = dev.double(), ref.double()
    if floor_one:
        return (dev - ref).abs() / ref.abs().clamp(min=1.0)
    return (dev - ref).abs() / ref.abs().amax(dim=-1, keepdim=True).clamp(min=1e-30)


def _kv_ref(sd, nb, x, eps):
    outs = []
    for i in range(nb):
        p = f"transformer.transformer_blocks.{i}"
        xi = x[..., i, :]
        if p + ".norm_kv.weight" in sd:
            xi = F.layer_norm(xi, (xi.shape[-1],), sd[p + ".norm_kv.weight"], sd[p + ".norm_kv.bias"], eps)
        w = torch.cat((sd[p + ".attention.keys.weight"], sd[p + ".attention.values.weight"]), dim=0)
        outs.append(xi @ w.t())
    return torch.stack(outs, dim=-2)


def _inverse_cdf(p64, u):
    C = torch.cumsum(p64, dim=-1)
    A = p64.shape[-1]
    a = (C <= u[:, None]).sum(dim=-1)
    pos = p64 > 1e-30
    last_pos = A - 1 - torch.flip(pos, dims=[-1]).int().argmax(dim=-1)
    a = torch.where(a >= A, last_pos, a)
    gap = (C[:, : A - 1] - u[:, None]).abs().amin(dim=-1) if A > 1 else torch.full_like(u, float("inf"))
    return a, gap


def _case(name, branches, D, H, L, W, ln="post", gtrxl=False, path="worker", forced=False, **over):
    return dict(name=name, br=tuple(branches), D=D, H=H, L=L, W=W, ln=ln, gtrxl=gtrxl, path=path, forced=forced, over=over)


CASES = [
    _case("w_post_33", (3, 3), 384, 4, 32, 8),
    _case("w_pre_243", (2, 4, 3), 384, 4, 32, 8, ln="pre"),
    _case("w_gated_33", (3, 3), 384, 4, 32, 8, ln="pre", gtrxl=True, rollout_group_kernel=False),
    _case("w_d512_243", (2, 4, 3), 512, 4, 32, 8),
    _case("w_two_groups_33", (3, 3), 384, 4, 32, 16, rollout_groups=2, rollout_min_group_size=2),
    _case("w_forced_243", (2, 4, 3), 384, 4, 32, 8, forced=True),
    _case("g_33", (3, 3), 384, 4, 32, 6, ln="pre", gtrxl=True, path="group"),
    _case("g_two_groups_243", (2, 4, 3), 384, 4, 32, 16, ln="pre", gtrxl=True, path="group", rollout_groups=2, rollout_min_group_size=2),
    _case("g_forced_33", (3, 3), 384, 4, 32, 6, ln="pre", gtrxl=True, path="group", forced=True),
    _case("policy_243", (2, 4, 3), 384, 4, 32, 8, path="policy", fused_rollout_block=False),
    _case("policy_forced_33", (3, 3), 384, 4, 32, 8, path="policy", fused_rollout_block=False, forced=True),
    _case("sample_captured_33", (3, 3), 128, 2, 32, 8, path="sample", kv_cache_rollout=False),
    _case("sample_eager_243", (2, 4, 3), 128, 2, 32, 8, path="sample", kv_cache_rollout=False, hip_graph_rollout=False),
    _case("sample_forced_243", (2, 4, 3), 128, 2, 32, 8, path="sample", kv_cache_rollout=False, forced=True),
]


def _config(c, num_actions=None):
    L = c["L"]
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[7], num_actions=list(c["br"]) if num_actions is None else num_actions,
                                max_episode_steps=L + 5, seed=3, p_done=0.5 / L, pool=4),
               gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=c["W"], worker_steps=L + 12, n_mini_batch=1,
               value_loss_coefficient=0.5, hidden_layer_size=c["D"], max_grad_norm=0.5, rollout_groups=1, rollout_min_group_size=2,
               transformer=dict(num_blocks=2, embed_dim=c["D"], num_heads=c["H"], memory_length=L, positional_encoding="relative",
                                layer_norm=c["ln"], gtrxl=c["gtrxl"], gtrxl_bias=1.0 if c["gtrxl"] else 0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    cfg.update(c["over"])
    return cfg


def _uniforms(W, S, B, seed):
    """[W, S, B] draws: random, with 0 and the largest fp32 uniform mixed in; second value: which entries are crafted."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((W, S, B), generator=g)
    ww, tt, bb = torch.meshgrid(torch.arange(W), torch.arange(S), torch.arange(B), indexing="ij")
    top = (ww + tt + bb) % 3 == 0
    low = (ww + 2 * tt + 5 * bb) % 11 == 5
    u[top] = U_MAX
    u[low] = 0.0
    return u, top | low


def _run_case(c):
    from etm import ops
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    cfg = _config(c)
    torch.manual_seed(31)
    tr = PPOTrainer(cfg, run_id="f64md", device=dev, tensorboard=False)
    br = c["br"]
    B = len(br)
    try:
        assert tr.action_space_shape == br and len(tr.model.policy_branches) == B
        W, S, L, T, nb, D = c["W"], cfg["worker_steps"], c["L"], tr.max_episode_length, 2, c["D"]
        with torch.no_grad():
            for prm in tr.model.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
            for head in tr.model.policy_branches:        # every branch: the last action gets probability zero
                head.weight[-1].zero_()
                head.bias[-1] = -200.0
        u, crafted = _uniforms(W, S, B, seed=len(c["name"]))
        forced = None
        if c["forced"]:
            g = torch.Generator().manual_seed(7)
            forced = torch.stack([torch.randint(0, max(1, a - 1), (W, S), generator=g) for a in br], dim=2)
            forced[(torch.arange(W)[:, None] + torch.arange(S)[None, :]) % 4 == 0] = -1      # some samples are drawn
            forced[:, :, 0][(torch.arange(W)[:, None] + torch.arange(S)[None, :]) % 4 == 1] = -1   # ... some only in branch 0
        s0 = tr.worker_current_episode_step.copy()
        tr._sample_training_data(uniforms=u, forced_actions=forced)
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()

        # ---- the intended path, no team time-out
        use_graph = bool(cfg.get("hip_graph_rollout", True))
        groups = tr._groups if use_graph else [tr._group_all]
        path = c["path"]
        assert tr._use_kv_cache == (path != "sample"), c["name"]
        if path != "sample":
            assert (tr.model._rf is not None) == (path in ("worker", "group")), (c["name"], "fused step kernel")
        assert all((g.rf_scratch is not None) == (path in ("worker", "group")) for g in groups), (c["name"], "step kernel")
        if path in ("worker", "group"):
            assert all(g.group_kernel == (path == "group") for g in groups), (c["name"], "group kernel")
        if "rollout_groups" in c["over"]:
            assert len(tr._groups) == c["over"]["rollout_groups"]
        for g in tr._groups + [tr._group_all]:
            if g.rf_scratch is not None:
                assert int(ops.rollout_trxl_error(g.rf_scratch).item()) == 0, (c["name"], "step kernel error word")

        b = tr.buffer
        assert tuple(b.actions.shape) == (W, S, B) and tuple(b.log_probs.shape) == (W, S, B)
        dones = torch.from_numpy(b.dones.copy())
        steps = torch.zeros((W, S), dtype=torch.int64)
        s = torch.from_numpy(s0.astype(np.int64))
        for t in range(S):
            steps[:, t] = s
            s = torch.where(dones[:, t], torch.zeros_like(s), s + 1)
        assert torch.equal(s, torch.from_numpy(tr.worker_current_episode_step.astype(np.int64)))
        sd = {k: v.detach().double() for k, v in tr.model.state_dict().items()}
        pos = tr.model.transformer._pos()
        pos64 = pos.detach().double() if pos is not None else None
        ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
        eps = tr.model.transformer.transformer_blocks[0].norm1.eps

        def forward64(obs, slot, rows, step, mask, pidx):
            win = b.memories[slot[:, None], rows].double()
            win = win * (rows < step[:, None]).to(win.dtype)[:, :, None, None]
            if pos64 is not None:
                win = win + pos64[pidx].unsqueeze(2)
            return rm.actor_critic(sd, ocfg, obs.double(), win, mask, pidx, T)

        N = W * S
        flat = lambda x: x.reshape(N, *x.shape[2:]).to(dev)
        slot_f, idx_f, mask_f = flat(b.memory_index), flat(b.memory_indices), flat(b.memory_mask)
        step_f, obs_f = flat(steps), flat(b.obs)
        act_f, lp_f, v_f = flat(b.actions), flat(b.log_probs), flat(b.values)
        u_f, crafted_f = flat(u), flat(crafted)
        forced_f = flat(forced) if forced is not None else None
        worst = {}
        upd = lambda k, e: worst.__setitem__(k, max(worst.get(k, 0.0), float(e.max()) if e.numel() else 0.0))
        skipped = n_random = n_top = 0
        with torch.no_grad():
            for lo in range(0, N, 256):
                sl = slice(lo, min(N, lo + 256))
                logits, value, item = forward64(obs_f[sl], slot_f[sl], idx_f[sl], step_f[sl], mask_f[sl], idx_f[sl])
                assert len(logits) == B
                upd("value", _rel(v_f[sl], value))
                upd("item", _rel(b.memories[slot_f[sl], step_f[sl]], item, floor_one=False))
                for k in range(B):
                    lsm = torch.log_softmax(logits[k], dim=-1)
                    a = act_f[sl, k]
                    assert bool(((a >= 0) & (a < br[k])).all()), (c["name"], k)
                    upd("logp", _rel(lp_f[sl, k], lsm.gather(1, a[:, None])[:, 0]))
                    p64 = lsm.exp()
                    pa = p64.gather(1, a[:, None])[:, 0]
                    assert float(pa.min()) >= 1e-30, (c["name"], "branch", k, "sampled an action of probability zero")
                    assert not bool((a == br[k] - 1).any()) or br[k] == 1, (c["name"], "branch", k, "took its last action")
                    uk = u_f[sl, k]
                    n_top += int((uk == U_MAX).sum())
                    a_ref, gap = _inverse_cdf(p64, uk.double())
                    take = torch.ones_like(a, dtype=torch.bool)
                    if forced_f is not None:
                        fk = forced_f[sl, k]
                        assert torch.equal(a[fk >= 0], fk[fk >= 0]), (c["name"], "forced action of branch", k)
                        take = fk < 0
                    near = gap < BOUNDARY_GAP
                    bad = (a != a_ref) & ~near & take
                    assert not bool(bad.any()), (c["name"], "inverse CDF of branch", k, int(bad.sum()))
                    rnd = ~crafted_f[sl, k] & take
                    skipped += int((near & rnd).sum())
                    n_random += int(rnd.sum())
        assert n_top > 0
        assert skipped <= 2 + 1e-3 * n_random, (c["name"], "draws within 1e-5 of a CDF boundary", skipped, n_random)
        if cfg.get("kv_cache_rollout", True):
            zeros = torch.zeros((T, nb, D), dtype=torch.float64, device=dev)
            upd("kv_init", _rel(tr._kv_init, _kv_ref(sd, nb, zeros + (pos64[:, None, :] if pos64 is not None else 0), eps), floor_one=False))
            for w in range(W):
                s_end = int(tr.worker_current_episode_step[w])
                if s_end == 0:
                    continue
                items = b.bank[int(tr.worker_episode_slot[w]), :s_end].double()
                if pos64 is not None:
                    items = items + pos64[:s_end, None, :]
                upd("kv", _rel(tr._kv_cache[w, :s_end], _kv_ref(sd, nb, items, eps), floor_one=False))
        print(f"[f64md] {c['name']:<20} samples {N:5d} episodes ended {int(dones.sum()):3d} skipped {skipped} "
              + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        for k, v in worst.items():
            assert v <= BOUNDS[k], (c["name"], k, v, BOUNDS[k])
        assert int(dones.sum()) > 0 and bool((steps >= L).any())
    finally:
        _release(tr)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_multidiscrete_rollout_vs_float64(case):
    _run_case(case)


@pytest.mark.parametrize("over", [dict(), dict(fused_rollout_block=False), dict(kv_cache_rollout=False)], ids=["step_kernel", "policy", "sample"])
def test_discrete_equals_single_entry_nvec_bit_for_bit(over):
    """Discrete(3) and MultiDiscrete([3]) run the same kernels on the same draws: rollout buffers and one update are bit-identical."""
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    c = _case("eq", (3,), 384, 4, 32, 8, **over)
    out = []
    for num_actions in (3, [3]):
        torch.manual_seed(5)
        tr = PPOTrainer(_config(c, num_actions=num_actions), run_id="eq", device=dev, tensorboard=False)
        try:
            assert tr.action_space_shape == (3,) and tuple(tr._uniforms.shape) == (tr.config["worker_steps"], 8)
            torch.manual_seed(9)
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            bufs = {k: getattr(tr.buffer, k).clone() for k in ("actions", "log_probs", "values", "advantages")}
            torch.manual_seed(10)
            st, _ = tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            out.append((bufs, np.array(st), [p.detach().clone() for p in tr.params]))
        finally:
            _release(tr)
        del tr
        gc.collect()               # (the next trainer captures graphs: nothing of this one may be collected during that capture)
    (b0, s0, p0), (b1, s1, p1) = out
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k
    assert np.array_equal(s0, s1)
    assert all(torch.equal(x, y) for x, y in zip(p0, p1))


# ------------------------------------------------------------------ heads + loss
# (worst measured: statistics 1.5e-7 at N = 2048 (3, 3); gradients 5.3e-6, branch 3's bias at N = 37 (2, 2, 2, 2) -- the cap 1e-5 binds)
HEADS_BOUNDS = {"stats": 6.2e-7, "grad": 1e-5}


def _heads_problem(N, branches, D=384, hid=384, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * N + len(branches))
    mods = dict(lin_policy=torch.nn.Linear(D, hid), lin_value=torch.nn.Linear(D, hid), value=torch.nn.Linear(hid, 1))
    heads = [torch.nn.Linear(hid, a) for a in branches]
    with torch.no_grad():
        for m in list(mods.values()) + heads:
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[1] ** 0.5)
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
        for hd in heads:
            hd.weight.mul_(3.0)
    h = torch.randn((N, D), generator=g)
    actions = torch.stack([torch.randint(0, a, (N,), generator=g) for a in branches], dim=1)
    adv = torch.randn(N, generator=g) if N > 1 else torch.tensor([0.7])
    old_value = torch.randn(N, generator=g)
    return mods, heads, h, actions, adv, old_value, g


def _ref_heads(mods, heads, h, actions, old_logp, adv, old_value, clip, vf, beta, N):
    from oracle import ref_algo as ra
    P = {k: v.detach().double().requires_grad_(True) for m in ("lin_policy", "lin_value", "value") for k, v in
         ((m + ".w", mods[m].weight), (m + ".b", mods[m].bias))}
    HB = [(hd.weight.detach().double().requires_grad_(True), hd.bias.detach().double().requires_grad_(True)) for hd in heads]
    x = h.detach().double().requires_grad_(True)
    hp = torch.relu(x @ P["lin_policy.w"].t() + P["lin_policy.b"])
    hv = torch.relu(x @ P["lin_value.w"].t() + P["lin_value.b"])
    logits = [hp @ w.t() + b for w, b in HB]
    value = (hv @ P["value.w"].t() + P["value.b"]).reshape(-1)
    loss, stats = ra.ppo_loss(logits, value, actions, old_logp.double(), adv.double(), old_value.double(), clip, vf, beta)
    loss.backward()
    grads = {"h": x.grad, **{k: v.grad for k, v in P.items()}}
    for i, (w, b) in enumerate(HB):
        grads[f"branch{i}.w"], grads[f"branch{i}.b"] = w.grad, b.grad
    return loss.detach(), stats.detach(), grads, [torch.log_softmax(lg, -1).detach() for lg in logits]


@pytest.mark.parametrize("N", [1, 37, 2048])
@pytest.mark.parametrize("branches", [(3, 3), (2, 2, 2, 2), (4, 4), (5, 4)], ids=["33", "2222", "44_largest", "54_beyond"])
def test_heads_loss_with_branches_vs_float64(N, branches):
    """``ops.heads_ppo_loss`` (fused, sum of the branch sizes <= 8) or, beyond its predicate, the per-branch ``ops.ppo_loss``, against
    ``ref_algo.ppo_loss`` in float64: loss, the six statistics and the gradients of h, both hidden heads, every branch and the value
    head.  Old log-probs put a quarter of the ratios at the clip boundary, a quarter far outside the range and the rest near 1.
    Loss and statistics are compared with the boundary samples; the gradients on a second draw with those samples moved inside the
    range: at the boundary the fp32 products r a and clamp(r) a can tie where float64 does not, and torch's tie rule (which the
    kernels follow) then halves that sample's policy gradient."""
    import copy
    import ctypes
    from etm import lib as etm_lib
    from etm import ops
    dev = torch.device("cuda", 0)
    clip, vf, beta = 0.2, 0.5, 0.01
    mods, heads, h, actions, adv, old_value, g = _heads_problem(N, branches)
    B = len(branches)
    with torch.no_grad():
        hp = torch.relu(h.double() @ mods["lin_policy"].weight.double().t() + mods["lin_policy"].bias.double())
        lp = torch.stack([torch.log_softmax(hp @ hd.weight.double().t() + hd.bias.double(), -1).gather(1, actions[:, k:k + 1])[:, 0]
                          for k, hd in enumerate(heads)], dim=1)
        kind = torch.randint(0, 4, (N, B), generator=g)
        far, near = 0.5 * torch.randn(N, B, generator=g).double(), 0.03 * torch.randn(N, B, generator=g).double()
        # boundary: ratio = 1 + clip where the normalised advantage is negative, 1 - clip where it is positive
        edge = torch.where((adv - adv.mean())[:, None] < 0, np.log1p(clip), np.log1p(-clip)) * torch.ones(N, B, dtype=torch.float64)
    tab = (ctypes.c_int32 * B)(*branches)
    fused = bool(etm_lib.load().etm_heads_loss_supported_branched(N, 384, tab, B))
    assert fused == (sum(branches) <= 8)

    def run(with_edge):
        shift = torch.where(kind == 1, far, near)
        if with_edge:
            shift = torch.where(kind == 0, edge, shift)
        old_logp = (lp - shift).float()
        dm = {k: copy.deepcopy(m).to(dev) for k, m in mods.items()}      # (Module.to moves in place: the float64 reference keeps the CPU set)
        dh = [copy.deepcopy(x).to(dev) for x in heads]
        hd_ = h.to(dev).requires_grad_(True)
        if fused:
            assert ops.heads_loss_supported(hd_, dm["lin_policy"], dh)
            loss, st = ops.heads_ppo_loss(hd_, dm["lin_policy"], dm["lin_value"], dh, dm["value"], actions.to(dev), old_logp.to(dev),
                                          adv.to(dev), old_value.to(dev), clip, vf, beta)
        else:
            assert not ops.heads_loss_supported(hd_, dm["lin_policy"], dh)
            hp_ = ops.linear_relu(dm["lin_policy"], hd_)
            hv_ = ops.linear_relu(dm["lin_value"], hd_)
            loss, st = ops.ppo_loss([x(hp_) for x in dh], dm["value"](hv_).reshape(-1), actions.to(dev), old_logp.to(dev), adv.to(dev),
                                    old_value.to(dev), clip, vf, beta)
        loss.backward()
        torch.cuda.synchronize()
        ref_loss, ref_st, ref_g, _ = _ref_heads(mods, heads, h, actions, old_logp, adv, old_value, clip, vf, beta, N)
        got = {"h": hd_.grad, "lin_policy.w": dm["lin_policy"].weight.grad, "lin_policy.b": dm["lin_policy"].bias.grad,
               "lin_value.w": dm["lin_value"].weight.grad, "lin_value.b": dm["lin_value"].bias.grad,
               "value.w": dm["value"].weight.grad, "value.b": dm["value"].bias.grad}
        for i, x in enumerate(dh):
            got[f"branch{i}.w"], got[f"branch{i}.b"] = x.weight.grad, x.bias.grad
        e_grad = {k: float((got[k].detach().cpu().double() - ref_g[k]).norm() / ref_g[k].norm().clamp(min=1e-30)) for k in ref_g}
        return float(loss), st.detach().cpu().double(), float(ref_loss), ref_st, e_grad

    loss, st, ref_loss, ref_st, e_edge = run(True)
    if N == 1:
        # one sample: the unbiased advantage std is 0 / 0 in torch and in the kernels alike -- every policy term is NaN; the value
        # loss and the value head's gradients are still defined
        assert bool(torch.isnan(ref_st[0])) and bool(torch.isnan(st[0]))
        assert abs(float(st[1]) - float(ref_st[1])) <= HEADS_BOUNDS["stats"] * max(1.0, abs(float(ref_st[1])))
        for k in ("value.w", "value.b"):
            assert e_edge[k] <= HEADS_BOUNDS["grad"], (k, e_edge[k])
        return
    n_edge = int((kind == 0).sum())
    assert n_edge > 0
    e_stats = [abs(float(st[i] - ref_st[i])) / max(1.0, abs(float(ref_st[i]))) for i in range(5)]
    e_stats.append(abs(loss - ref_loss) / max(1.0, abs(ref_loss)))
    assert abs(float(st[5]) - float(ref_st[5])) <= n_edge / (N * B) + 1e-6, ("clip fraction", float(st[5]), float(ref_st[5]))
    _, st2, _, ref_st2, e_grad = run(False)
    e_stats += [abs(float(st2[i] - ref_st2[i])) / max(1.0, abs(float(ref_st2[i]))) for i in range(6)]
    print(f"[heads] N={N} {branches} fused={fused} stats {max(e_stats):.2e} grad {max(e_grad.values()):.2e} ({max(e_grad, key=e_grad.get)})")
    assert max(e_stats) <= HEADS_BOUNDS["stats"], e_stats
    for k, e in e_grad.items():
        assert e <= HEADS_BOUNDS["grad"], (k, e)


# ------------------------------------------------------------------ whole trainer
def _small_multidiscrete_config(graph):
    from yaml_parser import YamlParser
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = YamlParser(os.path.join(repo, "episodic-transformer-memory-ppo_amd", "configs", "synthetic_multidiscrete.yaml")).get_config()
    cfg.update(n_workers=4, worker_steps=24, epochs=1, n_mini_batch=4, hip_graph_train=graph)
    cfg["environment"] = dict(cfg["environment"], pool=8, gen_threads=1, copy_threads=1, p_done=0.06)
    return cfg


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_synthetic_multidiscrete_update_vs_float64(graph):
    from oracle import ref_algo as ra
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    cfg = _small_multidiscrete_config(graph)
    torch.manual_seed(3)
    tr = PPOTrainer(cfg, run_id="md_update", device=dev, tensorboard=False)
    try:
        assert tr.action_space_shape == (3, 3)
        before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        names = [n for n, p in tr.model.named_parameters() if p.requires_grad]
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()
        assert tr.model._rf is not None and tr._groups[0].rf_scratch is not None   # the per-worker step kernel sampled both branches
        b = tr.buffer
        assert tuple(b.actions.shape) == (4, 24, 2) and bool(torch.isfinite(b.log_probs).all())
        first = {}
        step0 = tr.optimizer.step

        def spy(*a, **k):
            if not first and not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
                first["g"] = [p.grad.detach().clone() for p in tr.params]
            return step0(*a, **k)

        tr.optimizer.step = spy
        N = b.batch_size
        mbs = N // 4
        perm = torch.randperm(N)
        lr, beta, clip = tr.schedules(0)
        stats, _ = tr._train_epochs(lr, clip, beta, perms=[perm.numpy()])
        torch.cuda.synchronize()
        assert "g" in first and np.isfinite(np.array(stats)).all()
        assert (tr._train_graph is not None) == graph                 # minibatches 3 and 4 replay the captured step
        # float64 autograd over the first minibatch (sorted: the same set)
        idx = perm[:mbs].sort().values.to(dev)
        sd = {k: v.double().requires_grad_(v.is_floating_point() and k in names) for k, v in before.items()}
        for k, v in tr.model.state_dict().items():
            sd.setdefault(k, v.double())
        sf = b.samples_flat
        obs = sf["obs"].index_select(0, idx).double()
        ep = sf["memory_index"].index_select(0, idx)
        ind = sf["memory_indices"].index_select(0, idx)
        win = b.memories[ep[:, None], ind].double()
        pos = tr.model.transformer._pos()                 # (the positions are added here, from the model's own table, on the device)
        if pos is not None:
            win = win + pos.double()[ind].unsqueeze(2)
        ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
        logits, value, _ = rm.actor_critic(sd, ocfg, obs, win, sf["memory_mask"].index_select(0, idx), ind, tr.max_episode_length)
        loss, _ = ra.ppo_loss(logits, value, sf["actions"].index_select(0, idx), sf["log_probs"].index_select(0, idx).double(),
                              sf["advantages"].index_select(0, idx).double(), sf["values"].index_select(0, idx).double(), clip,
                              cfg["value_loss_coefficient"], beta)
        ref = torch.autograd.grad(loss, [sd[n] for n in names])
        worst = 0.0
        for n, gd, gr in zip(names, first["g"], ref):
            e = float((gd.double() - gr).norm() / gr.norm().clamp(min=1e-30))
            worst = max(worst, e)
            assert bool(torch.isfinite(gd).all()), n
            assert e <= 7e-6, (n, e)            # (worst measured 1.7e-6, eager and captured)
        print(f"[md update] graph={graph} worst gradient error {worst:.2e}")
        after = dict(tr.model.named_parameters())
        for n, p in after.items():
            assert bool(torch.isfinite(p).all()), n
        for k in range(2):
            for s in ("weight", "bias"):
                n = f"policy_branches.{k}.{s}"
                assert not torch.equal(after[n].detach(), before[n]), (n, "did not move")
    finally:
        _release(tr)
