"""-m gpu: Box (continuous) action spaces -- a diagonal Gaussian policy -- on every fused path, against float64.

* Rollout, per sample (the pattern of test_multidiscrete_vs_float64.py): the per-worker step kernel (post-LN, pre-LN, gated), the group
  kernel, ``rollout_policy`` (``fused_rollout_block: false``) and the multi-launch ``rollout_sample`` (eager and captured), with one
  and two worker groups, at ``policy_log_std`` -5, 0 and 2.  Compared with ``ref_model.actor_critic`` in float64 (its "logits[0]" is
  the mean) and the Gaussian restated here: the value, the raw action mu + sigma eps for the given normals, the joint log-prob, the
  clipped host action, the new memory items and the K | V rows.  Forced actions, some outside the bounds, are honoured.
* ``ops.heads_ppo_loss_gaussian`` against float64 autograd of the same loss written with ``torch.distributions.Normal``.
* One update of a small Box config, eager and captured: the first minibatch step's gradient arena (``policy_log_std`` included).
* A checkpoint (state_dict, config) reloads and runs one episode through ``enjoy.run_episode`` on the device.
"""
import gc
import math
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Bounds (relative, see _rel): about 4x the worst error measured on the MI355X, inside the caps of test_multidiscrete_vs_float64.py
# (worst measured: value 1.06e-6 sample_*, log-prob 5.0e-7 policy_3 (after the mean's conditioning allowance), item 4.9e-7 sample_*,
# kv 3.5e-7 w_pre_3, kv_init 9.1e-7 w_pre_3, raw action 1.3e-7 sample_captured_3; where 4x exceeds a cap, the cap)
BOUNDS = {"value": 3.7e-6, "logp": 9.0e-7, "item": 1.7e-6, "kv": 1.4e-6, "kv_init": 3.7e-6, "action": 5e-7}
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@pytest.fixture(autouse=True)
def _collect_between_tests():
    gc.collect()
    yield
    gc.collect()


def _release(tr):
    """Close a trainer and collect its captured graphs now (see test_multidiscrete_vs_float64._release)."""
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


def _case(name, A, D, H, L, W, ln="post", gtrxl=False, path="worker", forced=False, log_std=(-5.0, 0.0, 2.0), **over):
    return dict(name=name, A=A, D=D, H=H, L=L, W=W, ln=ln, gtrxl=gtrxl, path=path, forced=forced, log_std=log_std, over=over)


CASES = [
    _case("w_post_3", 3, 384, 4, 32, 8),
    _case("w_pre_3", 3, 384, 4, 32, 8, ln="pre"),
    _case("w_gated_3", 3, 384, 4, 32, 8, ln="pre", gtrxl=True, rollout_group_kernel=False),
    _case("w_post_8", 8, 384, 4, 32, 8),
    _case("w_two_groups_1", 1, 384, 4, 32, 16, log_std=(0.0,), rollout_groups=2, rollout_min_group_size=2),
    _case("w_forced_3", 3, 384, 4, 32, 8, forced=True),
    _case("g_3", 3, 384, 4, 32, 6, ln="pre", gtrxl=True, path="group"),
    _case("g_two_groups_3", 3, 384, 4, 32, 16, ln="pre", gtrxl=True, path="group", rollout_groups=2, rollout_min_group_size=2),
    _case("g_forced_3", 3, 384, 4, 32, 6, ln="pre", gtrxl=True, path="group", forced=True),
    _case("policy_3", 3, 384, 4, 32, 8, path="policy", fused_rollout_block=False),
    _case("policy_forced_8", 8, 384, 4, 32, 8, path="policy", fused_rollout_block=False, forced=True),
    _case("sample_captured_3", 3, 128, 2, 32, 8, path="sample", kv_cache_rollout=False),
    _case("sample_eager_3", 3, 128, 2, 32, 8, path="sample", kv_cache_rollout=False, hip_graph_rollout=False),
    _case("sample_forced_3", 3, 128, 2, 32, 8, path="sample", kv_cache_rollout=False, forced=True),
]
LOW, HIGH = -1.0, 1.5


def _config(c):
    L = c["L"]
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[7], continuous_actions=c["A"], action_low=LOW, action_high=HIGH,
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


def _run_case(c):
    from etm import ops
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    cfg = _config(c)
    torch.manual_seed(31)
    tr = PPOTrainer(cfg, run_id="f64box", device=dev, tensorboard=False)
    A = c["A"]
    try:
        assert tr.box is not None and tr.action_space_shape == (A,) and tr.model.continuous
        W, S, L, T, nb, D = c["W"], cfg["worker_steps"], c["L"], tr.max_episode_length, 2, c["D"]
        with torch.no_grad():
            for prm in tr.model.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
            ls = torch.tensor([c["log_std"][a % len(c["log_std"])] for a in range(A)], dtype=torch.float32)
            tr.model.policy_log_std.copy_(ls)
        g = torch.Generator().manual_seed(len(c["name"]))
        normals = torch.randn((W, S, A), generator=g)
        forced = None
        if c["forced"]:
            forced = 3.0 * torch.randn((W, S, A), generator=g)                    # many outside [LOW, HIGH]
            ww, tt = torch.meshgrid(torch.arange(W), torch.arange(S), indexing="ij")
            forced[(ww + tt) % 4 == 0] = float("nan")                              # some samples are drawn
            forced[..., 0][(ww + tt) % 4 == 1] = float("nan")                      # ... some only in dimension 0
        s0 = tr.worker_current_episode_step.copy()
        tr._sample_training_data(normals=normals, forced_actions=forced)
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()

        use_graph = bool(cfg.get("hip_graph_rollout", True))
        groups = tr._groups if use_graph else [tr._group_all]
        path = c["path"]
        assert tr._use_kv_cache == (path != "sample"), c["name"]
        if path != "sample":
            assert (tr.model._rf is not None) == (path in ("worker", "group")), (c["name"], "fused step kernel")
        assert all((g_.rf_scratch is not None) == (path in ("worker", "group")) for g_ in groups), (c["name"], "step kernel")
        if path in ("worker", "group"):
            assert all(g_.group_kernel == (path == "group") for g_ in groups), (c["name"], "group kernel")
        if "rollout_groups" in c["over"]:
            assert len(tr._groups) == c["over"]["rollout_groups"]
        for g_ in tr._groups + [tr._group_all]:
            if g_.rf_scratch is not None:
                assert int(ops.rollout_trxl_error(g_.rf_scratch).item()) == 0, (c["name"], "step kernel error word")

        b = tr.buffer
        assert b.actions.dtype == torch.float32 and tuple(b.actions.shape) == (W, S, A) and tuple(b.log_probs.shape) == (W, S, 1)
        # the host received clip(x) of the last step
        last = b.actions[:, S - 1].cpu()
        assert torch.equal(tr._act_pin, last.clamp(LOW, HIGH)), (c["name"], "clipped host actions")
        dones = torch.from_numpy(b.dones.copy())
        steps = torch.zeros((W, S), dtype=torch.int64)
        s = torch.from_numpy(s0.astype(np.int64))
        for t in range(S):
            steps[:, t] = s
            s = torch.where(dones[:, t], torch.zeros_like(s), s + 1)
        sd = {k: v.detach().double() for k, v in tr.model.state_dict().items()}
        pos = tr.model.transformer._pos()
        pos64 = pos.detach().double() if pos is not None else None
        ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
        eps = tr.model.transformer.transformer_blocks[0].norm1.eps
        ls64 = sd["policy_log_std"]
        sg64 = ls64.exp()

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
        x_f, lp_f, v_f = flat(b.actions), flat(b.log_probs)[:, 0], flat(b.values)
        n_f = flat(normals).double()
        forced_f = flat(forced) if forced is not None else torch.full((N, A), float("nan"), device=dev)
        worst = {}
        upd = lambda k, e: worst.__setitem__(k, max(worst.get(k, 0.0), float(e.max()) if e.numel() else 0.0))
        n_forced = n_outside = 0
        with torch.no_grad():
            for lo in range(0, N, 256):
                sl = slice(lo, min(N, lo + 256))
                logits, value, item = forward64(obs_f[sl], slot_f[sl], idx_f[sl], step_f[sl], mask_f[sl], idx_f[sl])
                mu = logits[0]
                upd("value", _rel(v_f[sl], value))
                upd("item", _rel(b.memories[slot_f[sl], step_f[sl]], item, floor_one=False))
                x, fk = x_f[sl], forced_f[sl]
                forced_m = ~torch.isnan(fk)
                assert torch.equal(x[forced_m], fk[forced_m]), (c["name"], "forced actions")
                n_forced += int(forced_m.sum())
                n_outside += int((forced_m & ((fk < LOW) | (fk > HIGH))).sum())
                drawn = ~forced_m
                x_ref = mu + sg64 * n_f[sl]
                upd("action", _rel(x[drawn], x_ref[drawn]))
                # joint log-prob of the stored x at the float64 mean.  d log p / d mu_a = z_a / sigma_a: the device's fp32 mean moves it
                # by |z_a| d mu_a / sigma_a -- 150x d mu at log sigma = -5 --, which is allowed on top of the bound.  d mu: measured
                # where the action was drawn (x - (mu64 + sigma eps), plus the rounding of x), the action bound where it was forced
                z = (x.double() - mu) / sg64
                lp_ref = (-0.5 * z * z - ls64 - HALF_LOG_2PI).sum(dim=1)
                d_mu = torch.where(drawn, (x.double() - x_ref).abs() + 6e-8 * x.double().abs(), BOUNDS["action"] * mu.abs().clamp(min=1.0))
                slack = (z.abs() * d_mu / sg64).sum(dim=1)
                e_lp = ((lp_f[sl].double() - lp_ref).abs() - slack).clamp(min=0.0) / lp_ref.abs().clamp(min=1.0)
                upd("logp", e_lp)
        if c["forced"]:
            assert n_forced > 0 and n_outside > 0
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
        print(f"[f64box] {c['name']:<18} samples {N:5d} episodes ended {int(dones.sum()):3d} "
              + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        for k, v in worst.items():
            assert v <= BOUNDS[k], (c["name"], k, v, BOUNDS[k])
        assert int(dones.sum()) > 0
    finally:
        _release(tr)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_box_rollout_vs_float64(case):
    _run_case(case)


# ------------------------------------------------------------------ heads + loss
HEADS_BOUNDS = {"stats": 6.2e-7, "grad": 8e-6}          # (worst measured: stats 3.5e-7, gradients 2.0e-6 of log_std)


def _ref_gaussian(mods, mean_head, log_std, h, x, old_logp, adv, old_value, clip, vf, beta):
    from torch.distributions import Normal
    P = {k: v.detach().double().requires_grad_(True) for m in ("lin_policy", "lin_value", "value") for k, v in
         ((m + ".w", mods[m].weight), (m + ".b", mods[m].bias))}
    mw, mb = mean_head.weight.detach().double().requires_grad_(True), mean_head.bias.detach().double().requires_grad_(True)
    ls = log_std.detach().double().requires_grad_(True)
    hx = h.detach().double().requires_grad_(True)
    hp = torch.relu(hx @ P["lin_policy.w"].t() + P["lin_policy.b"])
    hv = torch.relu(hx @ P["lin_value.w"].t() + P["lin_value.b"])
    dist = Normal(hp @ mw.t() + mb, ls.exp().expand(h.shape[0], -1))
    value = (hv @ P["value.w"].t() + P["value.b"]).reshape(-1)
    logp = dist.log_prob(x.double()).sum(1)
    entropy = dist.entropy().sum(1)
    adv = adv.double()
    norm_adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    log_ratio = logp - old_logp.double()
    ratio = log_ratio.exp()
    policy = torch.min(ratio * norm_adv, ratio.clamp(1 - clip, 1 + clip) * norm_adv).mean()
    ov = old_value.double()
    ret = ov + adv
    vfl = torch.max((value - ret) ** 2, (ov + (value - ov).clamp(-clip, clip) - ret) ** 2).mean()
    ent = entropy.mean()
    loss = -(policy - vf * vfl + beta * ent)
    kl = ((ratio - 1) - log_ratio).mean()
    cf = ((ratio - 1).abs() > clip).double().mean()
    loss.backward()
    grads = {"h": hx.grad, **{k: v.grad for k, v in P.items()}, "mean.w": mw.grad, "mean.b": mb.grad, "log_std": ls.grad}
    return float(loss), torch.stack([policy, vfl, loss, ent, kl, cf]).detach(), grads, logp.detach()


@pytest.mark.parametrize("N", [1, 37, 2048])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_heads_loss_gaussian_vs_float64(N, A):
    """Loss, the six statistics and the gradients of h, both hidden heads, the mean head, the value head and ``policy_log_std``.
    A quarter of the ratios sit at the clip boundary, a quarter far outside, the rest near 1; the gradients are compared on a second
    draw without the boundary samples (fp32 ties there, see test_multidiscrete_vs_float64)."""
    import copy
    from etm import ops
    dev = torch.device("cuda", 0)
    D = hid = 384
    clip, vf, beta = 0.2, 0.5, 0.01
    g = torch.Generator().manual_seed(17 * N + A)
    mods = dict(lin_policy=torch.nn.Linear(D, hid), lin_value=torch.nn.Linear(D, hid), value=torch.nn.Linear(hid, 1))
    mean_head = torch.nn.Linear(hid, A)
    with torch.no_grad():
        for m in list(mods.values()) + [mean_head]:
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[1] ** 0.5)
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    log_std = torch.nn.Parameter(torch.tensor([(-0.5, 0.0, 0.7)[a % 3] for a in range(A)]))
    h = torch.randn((N, D), generator=g)
    adv = torch.randn(N, generator=g) if N > 1 else torch.tensor([0.7])
    old_value = torch.randn(N, generator=g)
    with torch.no_grad():
        mu = torch.relu(h.double() @ mods["lin_policy"].weight.double().t() + mods["lin_policy"].bias.double()) @ \
            mean_head.weight.double().t() + mean_head.bias.double()
        x = (mu + log_std.double().exp() * torch.randn((N, A), generator=g).double()).float()
        lp = (-0.5 * ((x.double() - mu) / log_std.double().exp()) ** 2 - log_std.double() - HALF_LOG_2PI).sum(1)
        kind = torch.randint(0, 4, (N,), generator=g)
        far, near = 0.5 * torch.randn(N, generator=g).double(), 0.03 * torch.randn(N, generator=g).double()
        edge = torch.where(adv - adv.mean() < 0, np.log1p(clip), np.log1p(-clip)) * torch.ones(N, dtype=torch.float64)

    def run(with_edge):
        shift = torch.where(kind == 1, far, near)
        if with_edge:
            shift = torch.where(kind == 0, edge, shift)
        old_logp = (lp - shift).float()
        dm = {k: copy.deepcopy(m).to(dev) for k, m in mods.items()}
        dmean = copy.deepcopy(mean_head).to(dev)
        dls = torch.nn.Parameter(log_std.detach().clone().to(dev))
        hd_ = h.to(dev).requires_grad_(True)
        assert ops.heads_loss_supported_gaussian(hd_, dm["lin_policy"], dmean)
        loss, st = ops.heads_ppo_loss_gaussian(hd_, dm["lin_policy"], dm["lin_value"], dmean, dls, dm["value"], x.to(dev),
                                               old_logp[:, None].to(dev), adv.to(dev), old_value.to(dev), clip, vf, beta)
        loss.backward()
        torch.cuda.synchronize()
        ref_loss, ref_st, ref_g, _ = _ref_gaussian(mods, mean_head, log_std, h, x, old_logp, adv, old_value, clip, vf, beta)
        got = {"h": hd_.grad, "lin_policy.w": dm["lin_policy"].weight.grad, "lin_policy.b": dm["lin_policy"].bias.grad,
               "lin_value.w": dm["lin_value"].weight.grad, "lin_value.b": dm["lin_value"].bias.grad, "value.w": dm["value"].weight.grad,
               "value.b": dm["value"].bias.grad, "mean.w": dmean.weight.grad, "mean.b": dmean.bias.grad, "log_std": dls.grad}
        e_grad = {k: float((got[k].detach().cpu().double() - ref_g[k]).norm() / ref_g[k].norm().clamp(min=1e-30)) for k in ref_g
                  if ref_g[k] is not None and bool(torch.isfinite(ref_g[k]).all())}
        return float(loss), st.detach().cpu().double(), ref_loss, ref_st, e_grad

    loss, st, ref_loss, ref_st, e_edge = run(True)
    if N == 1:
        # one sample: the unbiased advantage std is 0 / 0 -- every policy term is NaN in both; the value loss and head are defined
        assert bool(torch.isnan(ref_st[0])) and bool(torch.isnan(st[0]))
        assert abs(float(st[1]) - float(ref_st[1])) <= HEADS_BOUNDS["stats"] * max(1.0, abs(float(ref_st[1])))
        assert abs(float(st[3]) - float(ref_st[3])) <= HEADS_BOUNDS["stats"] * max(1.0, abs(float(ref_st[3])))
        for k in ("value.w", "value.b"):
            assert e_edge[k] <= HEADS_BOUNDS["grad"], (k, e_edge[k])
        return
    n_edge = int((kind == 0).sum())
    assert n_edge > 0
    e_stats = [abs(float(st[i] - ref_st[i])) / max(1.0, abs(float(ref_st[i]))) for i in range(5)]
    e_stats.append(abs(loss - ref_loss) / max(1.0, abs(ref_loss)))
    assert abs(float(st[5]) - float(ref_st[5])) <= n_edge / N + 1e-6, ("clip fraction", float(st[5]), float(ref_st[5]))
    _, st2, _, ref_st2, e_grad = run(False)
    e_stats += [abs(float(st2[i] - ref_st2[i])) / max(1.0, abs(float(ref_st2[i]))) for i in range(6)]
    print(f"[heads gaussian] N={N} A={A} stats {max(e_stats):.2e} grad {max(e_grad.values()):.2e} ({max(e_grad, key=e_grad.get)})")
    assert max(e_stats) <= HEADS_BOUNDS["stats"], e_stats
    assert "log_std" in e_grad and "mean.w" in e_grad
    for k, e in e_grad.items():
        assert e <= HEADS_BOUNDS["grad"], (k, e)


# ------------------------------------------------------------------ whole trainer
def _small_continuous_config(graph):
    from yaml_parser import YamlParser
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = YamlParser(os.path.join(repo, "episodic-transformer-memory-ppo_amd", "configs", "synthetic_continuous.yaml")).get_config()
    cfg.update(n_workers=4, worker_steps=24, epochs=1, n_mini_batch=4, hip_graph_train=graph, action_log_std_init=-0.5)
    cfg["environment"] = dict(cfg["environment"], pool=8, gen_threads=1, copy_threads=1, p_done=0.06)
    return cfg


def _gaussian_loss64(mean, log_std, value, x, old_logp, adv, old_value, clip, vf, beta):
    from torch.distributions import Normal
    dist = Normal(mean, log_std.exp().expand_as(mean))
    logp = dist.log_prob(x).sum(1)
    norm_adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    log_ratio = logp - old_logp
    ratio = log_ratio.exp()
    policy = torch.min(ratio * norm_adv, ratio.clamp(1 - clip, 1 + clip) * norm_adv).mean()
    ret = old_value + adv
    vfl = torch.max((value - ret) ** 2, (old_value + (value - old_value).clamp(-clip, clip) - ret) ** 2).mean()
    return -(policy - vf * vfl + beta * dist.entropy().sum(1).mean())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_synthetic_continuous_update_vs_float64(graph):
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    cfg = _small_continuous_config(graph)
    torch.manual_seed(3)
    tr = PPOTrainer(cfg, run_id="box_update", device=dev, tensorboard=False)
    try:
        assert tr.action_space_shape == (3,) and tr.box is not None
        names = [n for n, _ in tr.model.arena_parameters()]              # (the order of tr.params: policy_log_std last)
        assert names[-1] == "policy_log_std" and len(names) == len(tr.params)
        assert torch.equal(tr.model.policy_log_std.detach().cpu(), torch.full((3,), -0.5))
        # the parameter lives in the optimiser's flat arena like every other one
        assert any(p is tr.model.policy_log_std for p in tr.params)
        before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()
        assert tr.model._rf is not None and tr._groups[0].rf_scratch is not None   # the per-worker step kernel drew the actions
        b = tr.buffer
        assert tuple(b.actions.shape) == (4, 24, 3) and bool(torch.isfinite(b.log_probs).all()) and bool(torch.isfinite(b.actions).all())
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
        assert (tr._train_graph is not None) == graph
        idx = perm[:mbs].sort().values.to(dev)
        sd = {k: v.double().requires_grad_(v.is_floating_point() and k in names) for k, v in before.items()}
        for k, v in tr.model.state_dict().items():
            sd.setdefault(k, v.double())
        sf = b.samples_flat
        obs = sf["obs"].index_select(0, idx).double()
        ep = sf["memory_index"].index_select(0, idx)
        ind = sf["memory_indices"].index_select(0, idx)
        win = b.memories[ep[:, None], ind].double()
        pos = tr.model.transformer._pos()
        if pos is not None:
            win = win + pos.double()[ind].unsqueeze(2)
        ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
        logits, value, _ = rm.actor_critic(sd, ocfg, obs, win, sf["memory_mask"].index_select(0, idx), ind, tr.max_episode_length)
        loss = _gaussian_loss64(logits[0], sd["policy_log_std"], value, sf["actions"].index_select(0, idx).double(),
                                sf["log_probs"].index_select(0, idx)[:, 0].double(), sf["advantages"].index_select(0, idx).double(),
                                sf["values"].index_select(0, idx).double(), clip, cfg["value_loss_coefficient"], beta)
        ref = torch.autograd.grad(loss, [sd[n] for n in names])
        worst = 0.0
        for n, gd, gr in zip(names, first["g"], ref):
            e = float((gd.double() - gr).norm() / gr.norm().clamp(min=1e-30))
            worst = max(worst, e)
            assert bool(torch.isfinite(gd).all()), n
            assert e <= 5.3e-6, (n, e)          # (worst measured 1.32e-6, eager and captured)
        print(f"[box update] graph={graph} worst gradient error {worst:.2e}")
        after = dict(tr.model.named_parameters())
        for n, p in after.items():
            assert bool(torch.isfinite(p).all()), n
        for n in ("policy_branches.0.weight", "policy_branches.0.bias", "policy_log_std"):
            assert not torch.equal(after[n].detach(), before[n]), (n, "did not move")
    finally:
        _release(tr)


def test_box_checkpoint_runs_one_episode(tmp_path):
    """The pickle format (state_dict, config) of a Box run reloads and plays one episode through enjoy.run_episode on the device."""
    import enjoy
    from environments import action_space_kind
    from model import ActorCriticModel
    from utils import create_env
    dev = torch.device("cuda", 0)
    cfg = _small_continuous_config(False)
    cfg["environment"] = dict(cfg["environment"], obs_shape=[3, 84, 84], max_episode_steps=80)
    env = create_env(cfg["environment"])
    kind = action_space_kind(env.action_space)
    torch.manual_seed(5)
    model = ActorCriticModel(cfg, env.observation_space, kind.shape, env.max_episode_steps, continuous=kind.is_box)
    path = tmp_path / "box.nn"
    with open(path, "wb") as f:
        pickle.dump((model.state_dict(), cfg), f)
    with open(path, "rb") as f:
        state_dict, config = pickle.load(f)
    m2 = ActorCriticModel(config, env.observation_space, kind.shape, env.max_episode_steps, continuous=True)
    m2.load_state_dict(state_dict)
    m2.to(dev).eval()
    assert torch.equal(m2.policy_log_std.detach().cpu(), model.policy_log_std.detach())
    seen = []
    step0 = env.step

    def spy(a):
        seen.append(np.asarray(a).copy())
        return step0(a)

    env.step = spy
    with torch.no_grad():
        rewards, info = enjoy.run_episode(m2, env, config, dev)
    assert 0 < len(rewards) <= 80 and len(seen) == len(rewards)
    for a in seen:
        assert a.shape == (3,) and a.dtype == np.float32 and bool(np.all(a >= -1.0)) and bool(np.all(a <= 1.0))
    env.close()
