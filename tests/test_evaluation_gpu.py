"""-m gpu: greedy actions on the fused rollout and the batched evaluator behind ``PPOTrainer.evaluate``.

* Kernel level: ``ops.rollout_sample`` / ``ops.rollout_policy`` on crafted logit rows with the greedy sentinel (u < 0) and ordinary
  uniforms in the same launches -- the mode is EXACTLY the first fp32 maximum, the other entries keep the inverse-CDF contract.
* Step level: one short rollout per sampling site with a ``uniforms=`` table that is half sentinel, half random; every sample is
  checked locally against the float64 model (as tests/test_rollout_step_vs_float64.py does).
* Box: ``deterministic=True`` stores the mean; the joint log-prob is the fp32 sum the kernel forms at z = 0.
* The evaluator end to end on PocMemoryEnv with an "always left" policy against a CPU re-simulation of the same seeded
  environments; training with evaluations interleaved is bit-identical to training without; evaluate.py, the periodic
  evaluation of ``run_training`` and ``enjoy.run_episode(deterministic=True)``.
"""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")

GREEDY_BAND = 1e-5           # a greedy action's float64 logit lies within this of the branch's float64 maximum
GREEDY_BAND_SHARE = 0.02     # at most this share of a case's greedy entries may have a float64 top-two gap inside the band


@pytest.fixture(autouse=True)
def _collect_between_tests():
    """Every test builds trainers that capture HIP graphs: collect the previous test's garbage first (see _release)."""
    gc.collect()
    yield
    gc.collect()


def _release(tr):
    """Close a trainer and collect its captured graphs NOW (not inside the next trainer's capture)."""
    tr.close()
    del tr
    gc.collect()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ kernel level
def _greedy_rows():
    """Logit rows by action count: the crafted rows of the inverse-CDF test (all equal, one dominant, [10, 10, -200],
    [-200, 10, 10], random with a -200 end) plus plain random rows and rows whose maximum appears twice."""
    from test_rollout_step_vs_float64 import _crafted_rows
    g = torch.Generator().manual_seed(23)
    rows = {}
    for A, base in _crafted_rows().items():
        extra = [torch.randn(A, generator=g) * 3 for _ in range(8)]
        if A > 2:
            for _ in range(4):               # the maximum at two places: the first one is the mode
                x = torch.randn(A, generator=g)
                i, j = sorted(torch.randperm(A, generator=g)[:2].tolist())
                x[i] = x[j] = 4.25
                extra.append(x)
        rows[A] = torch.cat((base, torch.stack(extra)))
    assert {1, 2, 3, 4, 15, 63} == set(rows)
    return rows


def test_sampling_kernels_greedy_sentinel():
    """u = -1.0 and u = -0.25 select the first fp32 maximum of the row, exactly (the logits are the bias: no band); the log-prob is
    float64's within the 4e-5 bound of the inverse-CDF test; the value is staged and the step counter advanced; rows with u in
    [0, 1) ride in the same launches and keep the inverse-CDF contract."""
    from etm import ops
    from test_rollout_step_vs_float64 import _check_draws, _probe_uniforms, _rel
    dev = torch.device("cuda", 0)
    hid = 64
    for A, rows in _greedy_rows().items():
        lgs, us, rid = [], [], []
        for i, r in enumerate(rows):
            for u in [-1.0, -0.25] + _probe_uniforms(r)[:6]:
                lgs.append(r)
                us.append(u)
                rid.append(i)
        lg = torch.stack(lgs)
        u = torch.tensor(us, dtype=torch.float32)
        greedy = u < 0
        assert bool(greedy.any()) and bool((~greedy).any())
        first_max = torch.from_numpy(np.array([int(np.argmax(r.numpy().astype(np.float32))) for r in lgs]))
        if A == 3:
            for r, want in (([10.0, 10.0, -200.0], 0), ([-200.0, 10.0, 10.0], 1)):
                hit = [k for k in range(len(lgs)) if lgs[k].tolist() == r]
                assert hit and all(int(first_max[k]) == want for k in hit)
        W = lg.shape[0]
        for kernel in ("sample", "policy"):
            t_dev = torch.zeros((), dtype=torch.int64, device=dev)
            acts = torch.zeros((W, 1), dtype=torch.int64, device=dev)
            st_a = torch.full((1, W, 1), -7, dtype=torch.int64, device=dev)
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
            a, lp = st_a[0, :, 0].cpu(), st_lp[0, :, 0].cpu()
            bad = greedy & (a != first_max)
            assert not bool(bad.any()), (kernel, A, "mode", lg[bad][:3].tolist(), u[bad][:3].tolist(), a[bad][:3].tolist(),
                                         first_max[bad][:3].tolist())
            lsm = torch.log_softmax(lg.double(), dim=-1)
            err = _rel(lp[greedy], lsm.gather(1, first_max[:, None])[:, 0][greedy])
            print(f"[greedy] {kernel:<6} A {A:2d} greedy entries {int(greedy.sum()):4d} log-prob error {float(err.max()):.2e}")
            assert float(err.max()) <= 1e-5 * 4, (kernel, A, "log-prob of the mode", float(err.max()))
            _check_draws(lg[~greedy], u[~greedy], a[~greedy], lp[~greedy], (kernel, A))
            assert float(_rel(st_v[0].cpu(), v_ref.cpu()).max()) <= 1e-5, (kernel, "value")
            if kernel == "sample":
                assert torch.equal(acts[:, 0].cpu(), a)


# ------------------------------------------------------------------ step level
def _step_case(name, site, D, H, L, branches, W, **over):
    return dict(name=name, site=site, D=D, H=H, L=L, br=tuple(branches), W=W, over=over)


STEP_CASES = [
    _step_case("worker_a4", "worker", 128, 1, 32, (4,), 8),
    _step_case("worker_324", "worker", 384, 4, 64, (3, 2, 4), 8),
    _step_case("group_a4", "group", 128, 1, 32, (4,), 8),
    _step_case("group_324", "group", 384, 4, 64, (3, 2, 4), 6),
    _step_case("policy_a4", "policy", 128, 2, 32, (4,), 8, fused_rollout_block=False),
    _step_case("sample_a4", "sample", 128, 2, 32, (4,), 8, kv_cache_rollout=False),
]


def _step_config(c):
    L, gated = c["L"], c["site"] == "group"
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[7], num_actions=list(c["br"]), max_episode_steps=L + 5, seed=3,
                                p_done=0.5 / L, pool=4),
               gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=c["W"], worker_steps=L + 12, n_mini_batch=1,
               value_loss_coefficient=0.5, hidden_layer_size=c["D"], max_grad_norm=0.5, rollout_groups=1, rollout_min_group_size=2,
               transformer=dict(num_blocks=2, embed_dim=c["D"], num_heads=c["H"], memory_length=L, positional_encoding="relative",
                                layer_norm="pre" if gated else "post", gtrxl=gated, gtrxl_bias=1.0 if gated else 0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    cfg.update(c["over"])
    return cfg


@pytest.mark.parametrize("case", STEP_CASES, ids=[c["name"] for c in STEP_CASES])
def test_rollout_step_mixes_greedy_and_sampled_entries(case):
    """Entries with (w + t) % 2 == 0 carry the sentinel -1, the rest random uniforms: one launch mixes both modes.  Greedy
    entries: the action's float64 logit within 1e-5 of the branch's float64 maximum, the float64 argmax where the top-two gap
    exceeds 1e-5, at most 2 % of them inside the band.  Sampled entries and every value / log-prob / memory item: the checks and
    bounds of the float64 step tests (Discrete: test_rollout_step_vs_float64, MultiDiscrete: test_multidiscrete_vs_float64)."""
    import test_multidiscrete_vs_float64 as md
    import test_rollout_step_vs_float64 as sv
    from etm import ops
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    c = case
    dev = torch.device("cuda", 0)
    cfg = _step_config(c)
    br = c["br"]
    B = len(br)
    bounds = sv.BOUNDS if B == 1 else md.BOUNDS
    boundary_gap = sv.BOUNDARY_GAP if B == 1 else md.BOUNDARY_GAP
    torch.manual_seed(37)
    tr = PPOTrainer(cfg, run_id="f64greedy", device=dev, tensorboard=False)
    try:
        assert tr.action_space_shape == br
        W, S, L, T = c["W"], cfg["worker_steps"], c["L"], tr.max_episode_length
        with torch.no_grad():
            for prm in tr.model.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
        g = torch.Generator().manual_seed(len(c["name"]))
        u = torch.rand((W, S, B), generator=g)
        ww, tt = torch.meshgrid(torch.arange(W), torch.arange(S), indexing="ij")
        greedy = ((ww + tt) % 2 == 0)[:, :, None].expand(W, S, B).clone()
        u[greedy] = -1.0
        s0 = tr.worker_current_episode_step.copy()
        tr._sample_training_data(uniforms=u[:, :, 0] if B == 1 else u)
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()

        # ---- the intended site, no team time-out
        site = c["site"]
        assert tr._use_kv_cache == (site != "sample"), c["name"]
        if site != "sample":
            assert (tr.model._rf is not None) == (site in ("worker", "group")), (c["name"], "fused step kernel")
        assert all((g_.rf_scratch is not None) == (site in ("worker", "group")) for g_ in tr._groups), (c["name"], "step kernel")
        if site in ("worker", "group"):
            assert all(g_.group_kernel == (site == "group") for g_ in tr._groups), (c["name"], "group kernel")
        for g_ in tr._groups + [tr._group_all]:
            if g_.rf_scratch is not None:
                assert int(ops.rollout_trxl_error(g_.rf_scratch).item()) == 0, (c["name"], "step kernel error word")

        b = tr.buffer
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
        u_f, greedy_f = flat(u), flat(greedy)
        worst = {}
        upd = lambda k, e: worst.__setitem__(k, max(worst.get(k, 0.0), float(e.max()) if e.numel() else 0.0))
        n_greedy = n_band = skipped = n_random = 0
        with torch.no_grad():
            for lo in range(0, N, 256):
                sl = slice(lo, min(N, lo + 256))
                logits, value, item = forward64(obs_f[sl], slot_f[sl], idx_f[sl], step_f[sl], mask_f[sl], idx_f[sl])
                assert len(logits) == B
                upd("value", sv._rel(v_f[sl], value))
                upd("item", sv._rel(b.memories[slot_f[sl], step_f[sl]], item, floor_one=False))
                for k in range(B):
                    lg64 = logits[k]
                    lsm = torch.log_softmax(lg64, dim=-1)
                    a = act_f[sl, k]
                    assert bool(((a >= 0) & (a < br[k])).all()), (c["name"], k)
                    upd("logp", sv._rel(lp_f[sl, k], lsm.gather(1, a[:, None])[:, 0]))
                    gk = greedy_f[sl, k]
                    # greedy entries
                    top2 = lg64.topk(min(2, br[k]), dim=-1).values
                    gap = top2[:, 0] - top2[:, 1] if br[k] > 1 else torch.full_like(top2[:, 0], float("inf"))
                    la = lg64.gather(1, a[:, None])[:, 0]
                    off = gk & (la < top2[:, 0] - GREEDY_BAND)
                    assert not bool(off.any()), (c["name"], "branch", k, "greedy action below the float64 maximum by",
                                                 float((top2[:, 0] - la)[gk].max()))
                    wrong = gk & (gap > GREEDY_BAND) & (a != lg64.argmax(dim=-1))
                    assert not bool(wrong.any()), (c["name"], "branch", k, "greedy action is not the float64 argmax", int(wrong.sum()))
                    n_greedy += int(gk.sum())
                    n_band += int((gk & (gap <= GREEDY_BAND)).sum())
                    # sampled entries: the float64 inverse CDF, as in the float64 step tests
                    a_ref, cgap = sv._inverse_cdf(lsm.exp(), u_f[sl, k].double().clamp(min=0.0))
                    near = cgap < boundary_gap
                    bad = ~gk & (a != a_ref) & ~near
                    assert not bool(bad.any()), (c["name"], "inverse CDF of branch", k, int(bad.sum()))
                    skipped += int((near & ~gk).sum())
                    n_random += int((~gk).sum())
        print(f"[f64greedy] {c['name']:<12} samples {N:5d} episodes ended {int(dones.sum()):3d} greedy {n_greedy} in band {n_band} "
              f"sampled {n_random} near a boundary {skipped} " + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        assert n_greedy > 0 and n_random > 0
        assert n_band <= GREEDY_BAND_SHARE * n_greedy, (c["name"], "greedy entries inside the band", n_band, n_greedy)
        assert skipped <= 2 + 1e-3 * n_random, (c["name"], "draws within 1e-5 of a CDF boundary", skipped, n_random)
        for k, v in worst.items():
            assert v <= bounds[k], (c["name"], k, v, bounds[k])
        assert int(dones.sum()) > 0 and bool((steps >= L).any()), (c["name"], "windows must slide past L and episodes restart")
    finally:
        _release(tr)


# ------------------------------------------------------------------ Box
@pytest.mark.parametrize("site", ["worker", "sample"])
def test_box_deterministic_rollout_stores_the_mean(site):
    """deterministic=True zeroes the normals: staged actions = the float64 mean within the value bound of the Box float64 test, the
    staged joint log-prob EQUALS sum_a((-0.f - log_std[a]) - 0.918938533f) accumulated in index order in fp32, the host receives
    clip(staged)."""
    import test_continuous_vs_float64 as bx
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    c = bx._case("det_" + site, 3, 128, 2 if site == "sample" else 1, 32, 8, path=site,
                 **(dict(kv_cache_rollout=False) if site == "sample" else {}))
    cfg = bx._config(c)
    torch.manual_seed(41)
    tr = PPOTrainer(cfg, run_id="f64boxdet", device=dev, tensorboard=False)
    try:
        A, W, S, T = 3, c["W"], cfg["worker_steps"], tr.max_episode_length
        assert tr.box is not None and tr._use_kv_cache == (site != "sample")
        with torch.no_grad():
            for prm in tr.model.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
            tr.model.policy_log_std.copy_(torch.tensor([-5.0, 0.0, 2.0]))
            tr.model.policy_branches[0].weight.mul_(10.0)          # (means of the size of the value)
        tr._normals.fill_(3.0)                                       # (must not survive)
        s0 = tr.worker_current_episode_step.copy()
        tr._sample_training_data(deterministic=True)
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()
        assert all((g_.rf_scratch is not None) == (site == "worker") for g_ in tr._groups)
        b = tr.buffer
        assert torch.equal(tr._act_pin, b.actions[:, S - 1].cpu().clamp(bx.LOW, bx.HIGH)), "clipped host actions"
        ls = tr.model.policy_log_std.detach().cpu().numpy().astype(np.float32)
        lp = np.float32(0.0)
        for a in range(A):
            lp = np.float32(lp + np.float32(np.float32(np.float32(-0.0) - ls[a]) - np.float32(0.918938533)))
        assert torch.equal(b.log_probs.cpu(), torch.full((W, S, 1), float(lp))), (float(lp), b.log_probs.flatten()[:4].tolist())
        dones = torch.from_numpy(b.dones.copy())
        steps = torch.zeros((W, S), dtype=torch.int64)
        s = torch.from_numpy(s0.astype(np.int64))
        for t in range(S):
            steps[:, t] = s
            s = torch.where(dones[:, t], torch.zeros_like(s), s + 1)
        sd = {k: v.detach().double() for k, v in tr.model.state_dict().items()}
        pos64 = tr.model.transformer._pos().detach().double()
        ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
        N = W * S
        flat = lambda x: x.reshape(N, *x.shape[2:]).to(dev)
        slot_f, idx_f, mask_f, step_f, obs_f = flat(b.memory_index), flat(b.memory_indices), flat(b.memory_mask), flat(steps), flat(b.obs)
        with torch.no_grad():
            win = b.memories[slot_f[:, None], idx_f].double()
            win = win * (idx_f < step_f[:, None]).to(win.dtype)[:, :, None, None] + pos64[idx_f].unsqueeze(2)
            logits, value, _ = rm.actor_critic(sd, ocfg, obs_f.double(), win, mask_f, idx_f, T)
        err = float(bx._rel(flat(b.actions), logits[0]).max())
        outside = int(((logits[0] < bx.LOW) | (logits[0] > bx.HIGH)).sum())
        print(f"[f64boxdet] {site:<6} samples {N} mean error {err:.2e} means outside the bounds {outside}")
        assert err <= bx.BOUNDS["value"], (site, "staged action vs the float64 mean", err)
        assert float(bx._rel(flat(b.values), value).max()) <= bx.BOUNDS["value"]
        assert int(dones.sum()) > 0
    finally:
        _release(tr)


# ------------------------------------------------------------------ the evaluator, exact and end to end
ENV_SEED, EVAL_SEED = 5, 100000


def _poc_config(worker_steps=16, **over):
    cfg = dict(environment=dict(type="PocMemoryEnv", seed=ENV_SEED, vectorize="serial"),
               gamma=0.99, lamda=0.95, updates=2, epochs=1, n_workers=8, worker_steps=worker_steps, n_mini_batch=2,
               value_loss_coefficient=0.1, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False,
               transformer=dict(num_blocks=2, embed_dim=64, num_heads=1, memory_length=32, positional_encoding="",
                                layer_norm="pre", gtrxl=True, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.2, final=0.2, power=1.0, max_decay_steps=10))
    cfg.update(over)
    return cfg


def _always_left(tr):
    with torch.no_grad():
        tr.model.policy_branches[0].weight.zero_()
        tr.model.policy_branches[0].bias.copy_(torch.tensor([5.0, 0.0]))


def _resimulate(env_cfg, first_worker_id, n_workers, episodes):
    """The seeded environments of workers first_worker_id .. on the CPU under "always left": [(worker, index, reward, length, success)]."""
    from utils import create_env
    out = []
    for w in range(n_workers):
        env = create_env(env_cfg, worker_id=first_worker_id + w)
        for i in range(episodes):
            env.reset()
            info = None
            while not info:
                _, _, _, info = env.step([0])
            out.append((w, i, info["reward"], info["length"], info["success"]))
        env.close()
    return out


def _as_tuples(episodes):
    return [(e["worker"], e["index"], e["reward"], e["length"], e["success"]) for e in episodes]


@pytest.mark.parametrize("worker_steps,graph,groups", [(8, True, 1), (40, False, 1), (40, True, 2), (8, False, 2)],
                         ids=["s8_graph_g1", "s40_eager_g1", "s40_graph_g2", "s8_eager_g2"])
def test_evaluate_matches_cpu_resimulation(worker_steps, graph, groups):
    """evaluate(episodes_per_worker=3, n_workers=8) under an "always left" policy returns exactly the episodes of the CPU
    re-simulation, whatever the chunk length (episodes of up to 32 steps span chunk borders), the rollout path and the groups;
    two calls in a row are equal, and so are two sampled calls with one seed."""
    from trainer import PPOTrainer
    cfg = _poc_config(hip_graph_rollout=graph, rollout_groups=groups, rollout_min_group_size=2)
    expected = _resimulate(cfg["environment"], EVAL_SEED, 8, 3)
    assert len({e[3] for e in expected}) > 1 and max(e[3] for e in expected) > 8, "episodes of several lengths, some longer than a chunk"
    torch.manual_seed(3)
    tr = PPOTrainer(cfg, run_id="evalpoc", device=torch.device("cuda", 0), tensorboard=False)
    try:
        _always_left(tr)
        first = tr.evaluate(episodes_per_worker=3, n_workers=8, worker_steps=worker_steps)
        assert _as_tuples(first["episodes"]) == expected
        ro = tr._evaluator.rollout
        assert len(ro._groups) == groups and (ro._step_graph is not None) == graph
        assert ro.env is not tr.env and ro.buffer is not tr.buffer and ro._uniforms.data_ptr() != tr._uniforms.data_ptr()
        assert first["steps"] % (8 * worker_steps) == 0 and first["steps"] > 0 and first["seconds"] > 0
        assert abs(first["result"]["reward_mean"] - np.mean([e[2] for e in expected])) < 1e-12
        assert abs(first["result"]["success_percent"] - np.mean([e[4] for e in expected])) < 1e-12
        second = tr.evaluate(episodes_per_worker=3, n_workers=8, worker_steps=worker_steps)
        assert second["episodes"] == first["episodes"] and tr._evaluator.rollout is ro
        sampled = [tr.evaluate(episodes_per_worker=3, n_workers=8, worker_steps=worker_steps, deterministic=False, seed=77)
                   for _ in range(2)]
        assert sampled[0]["episodes"] == sampled[1]["episodes"] and len(sampled[0]["episodes"]) == 24
    finally:
        _release(tr)


# ------------------------------------------------------------------ training is untouched
def _train_two_updates(evaluate):
    """Two updates of a small Synthetic config from a fixed seed -> the state after each update.  ``evaluate``: None, or the
    ``deterministic`` argument of an evaluation after each update."""
    from trainer import PPOTrainer
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[7], num_actions=3, max_episode_steps=24, seed=2, p_done=0.05, pool=4),
               gamma=0.99, lamda=0.95, updates=2, epochs=2, n_workers=8, worker_steps=16, n_mini_batch=2, value_loss_coefficient=0.5,
               hidden_layer_size=128, max_grad_norm=0.5, tunable_gemm=False,
               transformer=dict(num_blocks=2, embed_dim=128, num_heads=2, memory_length=8, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    torch.manual_seed(1234)
    tr = PPOTrainer(cfg, run_id="evaltrain", device=torch.device("cuda", 0), tensorboard=False)
    states = []
    try:
        for _ in range(2):
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            opt = tr.optimizer
            states.append([t.clone() for t in (opt.flat_params, opt.exp_avg, opt.exp_avg_sq, tr.buffer.actions, tr.buffer.log_probs)])
            if evaluate is not None:
                out = tr.evaluate(episodes_per_worker=1, n_workers=4, deterministic=evaluate, worker_steps=8)
                assert len(out["episodes"]) == 4
    finally:
        _release(tr)
    return states


def test_training_with_evaluations_is_bit_identical():
    """Evaluations between and after the updates (greedy in one run, sampled in another) change no bit of the parameter arena, the
    AdamW moments or the buffer's actions and log-probs."""
    base = _train_two_updates(None)
    for mode in (True, False):
        got = _train_two_updates(mode)
        for upd, (x, y) in enumerate(zip(base, got)):
            for name, p, q in zip(("parameters", "exp_avg", "exp_avg_sq", "actions", "log_probs"), x, y):
                assert torch.equal(p, q), ("deterministic" if mode else "sampled", "update", upd, name)


# ------------------------------------------------------------------ interfaces
def test_evaluate_py_prints_one_json_line(tmp_path, monkeypatch):
    """evaluate.py, as a fresh child process, on a checkpoint written by _save_model."""
    from trainer import PPOTrainer
    monkeypatch.chdir(tmp_path)
    cfg = _poc_config()
    tr = PPOTrainer(cfg, run_id="ckpt", device=torch.device("cuda", 0), tensorboard=False)
    try:
        _always_left(tr)
        tr._save_model()
    finally:
        _release(tr)
    env = dict(os.environ, ETM_QUIET="1", ETM_TUNABLE_GEMM="0")
    p = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--model", str(tmp_path / "models" / "ckpt.nn"),
                        "--workers", "4", "--episodes-per-worker", "2", "--seed", "300"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert set(out) == {"result", "steps", "seconds"}
    expected = _resimulate(cfg["environment"], 300, 4, 2)
    assert abs(out["result"]["reward_mean"] - np.mean([e[2] for e in expected])) < 1e-9
    assert abs(out["result"]["length_mean"] - np.mean([e[3] for e in expected])) < 1e-9


class _StubWriter:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def close(self):
        pass


def test_run_training_writes_evaluation_scalars(tmp_path, monkeypatch, capsys):
    """evaluation.interval: 1 over two updates: evaluation/<key> scalars after each update, one printed line each."""
    from trainer import PPOTrainer
    monkeypatch.chdir(tmp_path)
    cfg = _poc_config(evaluation=dict(interval=1, episodes_per_worker=2, n_workers=4, deterministic=True, seed=100000))
    tr = PPOTrainer(cfg, run_id="evalrun", device=torch.device("cuda", 0), tensorboard=False)
    try:
        assert tr._evaluator is None, "nothing is allocated before the first evaluation"
        tr.writer = _StubWriter()
        tr.run_training()
        tags = [(t, s) for t, _, s in tr.writer.scalars if t.startswith("evaluation/")]
        for update in (0, 1):
            for key in ("reward_mean", "length_mean", "success_percent", "env_steps_per_second"):
                assert ("evaluation/" + key, update) in tags, (key, update, tags)
        assert not any("std" in t for t, _ in tags)
        printed = [l for l in capsys.readouterr().out.splitlines() if " evaluation episodes=8" in l]
        assert len(printed) == 2, printed
    finally:
        _release(tr)


def test_enjoy_deterministic_matches_cpu_resimulation():
    """enjoy.run_episode(..., deterministic=True) on the [5, 0] policy plays "always left"."""
    import enjoy
    from trainer import PPOTrainer
    from utils import create_env
    cfg = _poc_config()
    dev = torch.device("cuda", 0)
    tr = PPOTrainer(cfg, run_id="enjoydet", device=dev, tensorboard=False)
    try:
        _always_left(tr)
        for wid in (0, 9):
            env = create_env(cfg["environment"], worker_id=wid)
            rewards, info = enjoy.run_episode(tr.model, env, cfg, dev, deterministic=True)
            (_, _, reward, length, success), = _resimulate(cfg["environment"], wid, 1, 1)
            assert (info["reward"], info["length"], info["success"]) == (reward, length, success) and len(rewards) == length
    finally:
        _release(tr)
