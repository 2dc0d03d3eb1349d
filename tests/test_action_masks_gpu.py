"""-m gpu: invalid-action masks (``action_masks: true``) from the sampler to the loss.

1. Rollout per sample against float64 (the pattern of test_multidiscrete_vs_float64.py) with crafted masks per (worker, step) -- all
   valid, one valid action per branch, first action invalid, last action invalid, random p = 0.5 -- on the per-worker step kernel,
   the group kernel, two worker groups (vector observations, and image observations: the pipelined plan), ``rollout_policy`` with a branch that straddles bit 32, ``rollout_sample`` captured and
   eager, and one forced case: every action is allowed, equals the float64 inverse CDF over the COMPACTED valid set, log-prob and
   value are within that file's bounds, the buffer's words are the environment's.
2. Bit identities: all-valid masks against no masks (rollout, two updates; eager and captured); a constant mask against the unmasked
   call on the compacted branch for ``ops.rollout_sample``, ``ops.heads_ppo_loss`` and ``ops.ppo_loss``.
3. ``ops.heads_ppo_loss`` / ``ops.ppo_loss`` with per-sample masks against a float64 restatement of the rule.
4. One update of ``synthetic_multidiscrete_masked`` (small), eager and captured, against float64 autograd.
5. An environment that raises on an illegal action survives a rollout and a greedy evaluation.
6. A word with an empty branch raises ValueError before the step is launched.
"""
import copy
import gc
import os

import numpy as np
import pytest
import torch

import test_action_masks_host as mh
import test_multidiscrete_vs_float64 as md

pytestmark = pytest.mark.gpu

# The bounds of test_multidiscrete_vs_float64.py, copied (a masked draw is arithmetically the unmasked draw on the compacted branch).
# Worst measured here on the MI355X: value 1.07e-6 (sample_eager_243), logp 2.6e-7 (w_two_groups_img_33), item 5.9e-7 (policy_30_5);
# no draw within 1e-5 of an inner boundary in any case (0 left out of 264 - 704 samples per case); masked loss against float64: statistics
# 1.2e-7, gradients 2.7e-6 (branch 2's bias, (2, 4, 2) at hid 128); the update's gradient arena 1.3e-6, eager and captured.
BOUNDS = {"value": 3.7e-6, "logp": 9.0e-7, "item": 1.7e-6}
HEADS_BOUNDS = {"stats": 6.2e-7, "grad": 1e-5}
BOUNDARY_GAP = 1e-5
U_MAX = md.U_MAX


def test_bounds_are_those_of_the_multidiscrete_file():
    assert all(BOUNDS[k] == md.BOUNDS[k] for k in BOUNDS) and HEADS_BOUNDS == md.HEADS_BOUNDS and BOUNDARY_GAP == md.BOUNDARY_GAP


@pytest.fixture(autouse=True)
def _collect_between_tests():
    gc.collect()
    yield
    gc.collect()


# ------------------------------------------------------------------ crafted masks
def crafted_words(br, worker_ids, K, seed=11):
    """uint64 [len(worker_ids), K]: the word of worker w for its k-th emitted observation cycles through all valid / one valid action
    per branch / first action invalid / last action invalid / random p = 0.5 (the largest draw of a branch stays valid)."""
    A = sum(br)
    out = np.zeros((len(worker_ids), K), dtype=np.uint64)
    for i, w in enumerate(worker_ids):
        rng = np.random.default_rng((seed, int(w)))
        for k in range(K):
            kind, r, valid, off = (w + k) % 5, rng.random(A), np.ones(A, dtype=bool), 0
            for a in br:
                if kind == 1:
                    valid[off:off + a] = False
                    valid[off + (w + 2 * k) % a] = True
                elif kind == 2 and a > 1:
                    valid[off] = False
                elif kind == 3 and a > 1:
                    valid[off + a - 1] = False
                elif kind == 4:
                    v = r[off:off + a] >= 0.5
                    v[r[off:off + a].argmax()] = True
                    valid[off:off + a] = v
                off += a
            out[i, k] = sum(1 << j for j in range(A) if valid[j])
    return out


def _crafted_env(br, n, first, env_cfg, K, words=None):
    """A thin subclass of the synthetic front-end whose ``action_masks`` hands out ``crafted_words``."""
    from environments.synthetic import SyntheticVecEnv

    class CraftedMaskEnv(SyntheticVecEnv):
        def __init__(self):
            kw = {k: v for k, v in env_cfg.items() if k not in ("type", "num_actions")}
            kw["obs_shape"] = tuple(kw["obs_shape"])
            super().__init__(n, num_actions=list(br) if len(br) > 1 else int(br[0]), first_worker_id=first, **kw)
            self.words = crafted_words(br, range(first, first + n), K) if words is None else words
            self.k = -1

        def reset(self, out=None):
            self.k += 1
            return super().reset(out)

        def step(self, actions, out=None, on_rows=None):
            self.k += 1
            return super().step(actions, out=out, on_rows=on_rows)

        def action_masks(self, out=None):
            w = self.words[:, self.k]
            if out is None:
                return w.copy()
            out.view(np.uint64)[...] = w
            return out

    return CraftedMaskEnv()


def _valid_columns(words, A, dev):
    """int64 words [N] -> bool [N, A]."""
    w = torch.as_tensor(np.asarray(words).astype(np.int64), device=dev).reshape(-1, 1)
    return ((w >> torch.arange(A, device=dev)) & 1).bool()


def _masked_inverse_cdf(logits64, valid, u):
    """Softmax and inverse CDF over the compacted valid set, mapped back to column indices: -> (action, gap of u to the nearest INNER
    boundary of the compacted CDF, log-softmax over the valid set)."""
    lsm = torch.log_softmax(logits64.masked_fill(~valid, float("-inf")), dim=-1)
    p = lsm.exp()                                         # exact zeros at the invalid columns: the running sum is the compacted one
    C = torch.cumsum(p, dim=-1)
    A = p.shape[-1]
    idx = torch.arange(A, device=p.device)
    pos = valid & (p > 1e-30)
    last_pos = A - 1 - torch.flip(pos, dims=[-1]).int().argmax(dim=-1)
    gt = (C > u[:, None]) & valid
    a = torch.where(gt.any(dim=-1), gt.int().argmax(dim=-1), last_pos)
    last_valid = A - 1 - torch.flip(valid, dims=[-1]).int().argmax(dim=-1)
    inner = valid & (idx[None, :] != last_valid[:, None])
    gap = torch.where(inner, (C - u[:, None]).abs(), torch.full_like(C, float("inf"))).amin(dim=-1)
    return a, gap, lsm


CASES = [
    md._case("w_post_5", (5,), 384, 4, 32, 8),
    md._case("w_pre_243", (2, 4, 3), 384, 4, 32, 8, ln="pre"),
    md._case("g_33", (3, 3), 384, 4, 32, 6, ln="pre", gtrxl=True, path="group"),
    md._case("w_two_groups_33", (3, 3), 384, 4, 32, 16, rollout_groups=2, rollout_min_group_size=2),
    # image observations, two groups: the pipelined plan (every case reads its words in place from pinned memory; here (step, slot) too)
    md._case("w_two_groups_img_33", (3, 3), 384, 4, 32, 16, rollout_groups=2, rollout_min_group_size=2, image=True),
    md._case("policy_30_5", (30, 5), 128, 2, 32, 8, path="policy", fused_rollout_block=False),
    md._case("sample_captured_33", (3, 3), 128, 2, 32, 8, path="sample", kv_cache_rollout=False),
    md._case("sample_eager_243", (2, 4, 3), 128, 2, 32, 8, path="sample", kv_cache_rollout=False, hip_graph_rollout=False),
    md._case("w_forced_243", (2, 4, 3), 384, 4, 32, 8, forced=True),
]


def _masked_trainer(c, seed=31):
    from environments.vec_env import CompositeVecEnv
    from trainer import PPOTrainer
    cfg = md._config(c)
    cfg["action_masks"] = True
    if cfg.pop("image", False):
        cfg["environment"] = dict(cfg["environment"], obs_shape=[3, 36, 36])
    W, S, br = c["W"], cfg["worker_steps"], c["br"]
    n_groups = int(c["over"].get("rollout_groups", 1))
    per = W // n_groups
    parts = [_crafted_env(br, per, g * per, cfg["environment"], S + 1) for g in range(n_groups)]
    env = parts[0] if n_groups == 1 else CompositeVecEnv(parts)
    torch.manual_seed(seed)
    tr = PPOTrainer(cfg, run_id="f64mask", device=torch.device("cuda", 0), env=env, tensorboard=False)
    return tr, cfg, np.concatenate([p.words for p in parts], axis=0)


def _run_case(c):
    from etm import ops
    from oracle import ref_model as rm
    dev = torch.device("cuda", 0)
    tr, cfg, words = _masked_trainer(c)
    br = c["br"]
    B, A = len(br), sum(br)
    try:
        assert tr.action_space_shape == br and tr._masked and tr.buffer.action_masks is not None
        W, S, L, T = c["W"], cfg["worker_steps"], c["L"], tr.max_episode_length
        with torch.no_grad():
            for prm in tr.model.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
        u, crafted = md._uniforms(W, S, B, seed=len(c["name"]))
        valid_ws = _valid_columns(words[:, :S].reshape(-1), A, "cpu").reshape(W, S, A)
        forced = None
        if c["forced"]:
            # a forced action must be allowed by its step's word: the first or the last valid action of the branch, or -1 = sample
            ww, tt = torch.meshgrid(torch.arange(W), torch.arange(S), indexing="ij")
            forced, off = torch.full((W, S, B), -1, dtype=torch.int64), 0
            for k, a in enumerate(br):
                v = valid_ws[:, :, off:off + a]
                first, last = v.int().argmax(dim=-1), a - 1 - torch.flip(v, dims=[-1]).int().argmax(dim=-1)
                forced[:, :, k] = torch.where((ww + tt + k) % 2 == 0, first, last)
                off += a
            forced[(ww + tt) % 4 == 0] = -1
            forced[:, :, 0][(ww + tt) % 4 == 1] = -1
        s0 = tr.worker_current_episode_step.copy()
        tr._sample_training_data(uniforms=u if B > 1 else u[:, :, 0], forced_actions=forced)
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
        if c["over"].get("image"):
            assert tr._plan.own_stream and tr._plan.stream_obs, (c["name"], "not the pipelined plan")
        # every sampling kernel read its words in place from the pinned block (no device twin in the step)
        assert tr._mask_in_place and all(g.am_pin.is_pinned() and g.am_pin.data_ptr() == tr._am_pin[g.lo:g.hi].data_ptr() for g in groups)
        for g in tr._groups + [tr._group_all]:
            if g.rf_scratch is not None:
                assert int(ops.rollout_trxl_error(g.rf_scratch).item()) == 0, (c["name"], "step kernel error word")

        b = tr.buffer
        # the buffer's words are what the environment handed out, on the host and (after prepare_batch_dict) on the device
        assert np.array_equal(b.action_masks_host.view(np.uint64), words[:, :S])
        assert np.array_equal(b.action_masks.cpu().numpy().view(np.uint64), words[:, :S])
        assert "action_masks" in b.samples_flat and tuple(b.samples_flat["action_masks"].shape) == (W * S,)
        assert 0.0 < tr.last_valid_action_share < 1.0
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
        u_f, crafted_f, valid_f = flat(u), flat(crafted), flat(valid_ws)
        forced_f = flat(forced) if forced is not None else None
        worst = {}
        upd = lambda k, e: worst.__setitem__(k, max(worst.get(k, 0.0), float(e.max()) if e.numel() else 0.0))
        skipped = n_random = n_top = n_zero_lead = n_single = 0
        with torch.no_grad():
            for lo in range(0, N, 256):
                sl = slice(lo, min(N, lo + 256))
                logits, value, item = forward64(obs_f[sl], slot_f[sl], idx_f[sl], step_f[sl], mask_f[sl], idx_f[sl])
                assert len(logits) == B
                upd("value", md._rel(v_f[sl], value))
                upd("item", md._rel(b.memories[slot_f[sl], step_f[sl]], item, floor_one=False))
                off = 0
                for k in range(B):
                    a, vk, uk = act_f[sl, k], valid_f[sl, off:off + br[k]], u_f[sl, k]
                    assert bool(((a >= 0) & (a < br[k])).all()), (c["name"], k)
                    assert bool(vk.gather(1, a[:, None]).all()), (c["name"], "branch", k, "took a masked-out action")
                    a_ref, gap, lsm = _masked_inverse_cdf(logits[k], vk, uk.double())
                    upd("logp", md._rel(lp_f[sl, k], lsm.gather(1, a[:, None])[:, 0]))
                    single = vk.sum(dim=-1) == 1
                    assert bool((lp_f[sl, k][single] == 0).all()), (c["name"], "one valid action: log p = 0")
                    n_single += int(single.sum())
                    n_top += int((uk == U_MAX).sum())
                    take = torch.ones_like(a, dtype=torch.bool)
                    if forced_f is not None:
                        fk = forced_f[sl, k]
                        assert torch.equal(a[fk >= 0], fk[fk >= 0]), (c["name"], "forced action of branch", k)
                        take = fk < 0
                    near = gap < BOUNDARY_GAP
                    bad = (a != a_ref) & ~near & take
                    assert not bool(bad.any()), (c["name"], "inverse CDF of branch", k, int(bad.sum()))
                    # u = 0 under a leading invalid action: compared (never "near": 0 is no inner boundary) and the first VALID action
                    zl = (uk == 0) & ~vk[:, 0] & take
                    first_valid = vk.int().argmax(dim=-1)
                    assert torch.equal(a[zl], first_valid[zl]) and not bool((near & zl).any()), (c["name"], "u = 0, leading invalid action")
                    n_zero_lead += int(zl.sum())
                    rnd = ~crafted_f[sl, k] & take
                    skipped += int((near & rnd).sum())
                    n_random += int(rnd.sum())
                    off += br[k]
        assert n_top > 0 and n_zero_lead > 0 and n_single > 0, (n_top, n_zero_lead, n_single)
        assert skipped <= 2 + 1e-3 * n_random, (c["name"], "draws within 1e-5 of an inner CDF boundary", skipped, n_random)
        print(f"[f64mask] {c['name']:<20} samples {N:5d} episodes ended {int(dones.sum()):3d} skipped {skipped} u=0/leading-invalid "
              f"{n_zero_lead} single {n_single} " + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
        for k, v in worst.items():
            assert v <= BOUNDS[k], (c["name"], k, v, BOUNDS[k])
        assert int(dones.sum()) > 0 and bool((steps >= L).any())
    finally:
        md._release(tr)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_masked_rollout_vs_float64(case):
    _run_case(case)


def test_forced_action_that_is_masked_out_raises():
    c = md._case("forced_bad", (2, 4, 3), 384, 4, 32, 8)
    tr, cfg, words = _masked_trainer(c)
    try:
        W, S = c["W"], cfg["worker_steps"]
        forced = torch.full((W, S, 3), -1, dtype=torch.int64)
        w, t = 1, 1                                   # kind (w + t) % 5 == 2: the first action of every branch is masked out
        assert (int(words[w, t]) >> 2) & 1 == 0
        forced[w, t, 1] = 0
        with pytest.raises(ValueError, match=r"worker 1, step 1, branch 1.*masked out"):
            tr._sample_training_data(forced_actions=forced)
    finally:
        md._release(tr)


# ------------------------------------------------------------------ 6. empty branch
def test_word_with_an_empty_branch_raises_before_the_launch():
    c = md._case("empty", (2, 4, 3), 384, 4, 32, 8)
    cfg = md._config(c)
    cfg["action_masks"] = True
    S, K = cfg["worker_steps"], 3
    words = crafted_words(c["br"], range(8), S + 1)
    words[5, K] &= np.uint64(~(0b1111 << 2) & 0x1FF)            # worker 5, observation 3: branch 1 (bits 2..5) has nothing left
    from trainer import PPOTrainer
    env = _crafted_env(c["br"], 8, 0, cfg["environment"], S + 1, words=words)
    tr = PPOTrainer(cfg, run_id="empty", device=torch.device("cuda", 0), env=env, tensorboard=False)
    try:
        with pytest.raises(ValueError, match=r"worker 5, step 3, branch 1 has no valid action"):
            tr._sample_training_data()
        torch.cuda.synchronize()
        assert int(tr._groups[0].t_dev.item()) == K              # steps 0 .. 2 ran; step 3 was never launched
    finally:
        md._release(tr)


# ------------------------------------------------------------------ 2. bit identities
def _small_config(graph, masks, p=0.0):
    cfg = md._small_multidiscrete_config(graph)
    cfg["hip_graph_rollout"] = graph
    if masks:
        cfg["action_masks"] = True
        cfg["environment"] = dict(cfg["environment"], action_mask_p=p)
    return cfg


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_all_valid_masks_equal_no_masks_bit_for_bit(graph):
    """``action_masks: true`` with all-valid words against the key absent: the rollout's actions, log-probs, values and advantages
    and the training state after two updates are the same bits."""
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    out = []
    for masks in (False, True):
        torch.manual_seed(5)
        tr = PPOTrainer(_small_config(graph, masks), run_id="ident", device=dev, tensorboard=False)
        try:
            assert tr._masked == masks and (tr.buffer.action_masks is not None) == masks
            bufs = None
            for upd in range(2):
                torch.manual_seed(9 + upd)
                tr._sample_training_data()
                tr.buffer.prepare_batch_dict()
                assert ("action_masks" in tr.buffer.samples_flat) == masks
                if bufs is None:
                    bufs = {k: getattr(tr.buffer, k).cpu().numpy() for k in ("actions", "log_probs", "values", "advantages")}
                torch.manual_seed(20 + upd)
                tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            if masks:
                assert (tr.buffer.action_masks_host == (1 << 6) - 1).all() and tr.last_valid_action_share == 1.0
            assert (tr._step_graph is not None) == graph and (tr._train_graph is not None) == graph
            out.append((bufs, tr.state_digest()))
        finally:
            md._release(tr)
    (b0, d0), (b1, d1) = out
    for k in b0:
        assert np.array_equal(b0[k], b1[k]), k
    assert d0 == d1, (d0, d1)


KEEP = [0, 2, 3]                 # the constant mask {0, 2, 3} on 5 logits
KEEP_WORD = sum(1 << j for j in KEEP)


def test_rollout_sample_constant_mask_equals_compacted_call():
    from etm import ops
    dev = torch.device("cuda", 0)
    W = 96
    g = torch.Generator().manual_seed(2)
    logits5 = (2.0 * torch.randn((W, 5), generator=g)).to(dev)
    value = torch.randn(W, generator=g).to(dev)
    u = torch.rand((1, W), generator=g)
    u[0, ::7], u[0, 3::7], u[0, 5::7] = 0.0, U_MAX, -1.0               # (-1: the greedy sentinel)
    u = u.to(dev)
    res = []
    for masked in (True, False):
        lg = logits5 if masked else logits5[:, KEEP].contiguous()
        t_dev = torch.zeros((), dtype=torch.int64, device=dev)
        actions = torch.zeros((W, 1), dtype=torch.int64, device=dev)
        st_a = torch.zeros((1, W), dtype=torch.int64, device=dev)
        st_lp, st_v = torch.zeros((1, W), device=dev), torch.zeros((1, W), device=dev)
        am = torch.full((W,), KEEP_WORD, dtype=torch.int64, device=dev) if masked else None
        ops.rollout_sample(lg, value, u, None, t_dev, actions, st_a, st_lp, st_v, action_mask=am)
        torch.cuda.synchronize()
        assert int(t_dev.item()) == 1 and torch.equal(actions[:, 0], st_a[0])
        res.append((st_a[0].cpu(), st_lp[0].cpu().numpy(), st_v[0].cpu().numpy()))
    (a5, lp5, v5), (a3, lp3, v3) = res
    assert torch.equal(a5, torch.tensor(KEEP)[a3]) and len(set(a5.tolist())) == 3
    assert np.array_equal(lp5, lp3) and np.array_equal(v5, v3)
    # a misaligned word array is refused by the entry (ETM_EINVAL) and nothing is launched
    import ctypes
    from etm import lib as etm_lib
    am = torch.full((W + 1,), KEEP_WORD, dtype=torch.int64, device=dev)
    t_dev = torch.zeros((), dtype=torch.int64, device=dev)
    tab = (ctypes.c_int32 * 1)(5)
    rc = etm_lib.load().etm_rollout_sample_branched_masked(logits5.data_ptr(), value.data_ptr(), u.data_ptr(), None, t_dev.data_ptr(),
                                                            actions.data_ptr(), st_a.data_ptr(), st_lp.data_ptr(), st_v.data_ptr(), W, tab, 1,
                                                            am.data_ptr() + 4, None)
    torch.cuda.synchronize()
    assert rc == -1 and int(t_dev.item()) == 0


def _mask_problem(N, hid):
    mods, heads, h, _, adv, old_value, g = md._heads_problem(N, (5,), D=hid, hid=hid)
    act3 = torch.randint(0, 3, (N, 1), generator=g)
    old_logp = -1.0 + 0.3 * torch.randn((N, 1), generator=g)
    return mods, heads[0], h, act3, adv, old_value, old_logp


@pytest.mark.parametrize("N", [37, 256])
def test_heads_loss_constant_mask_equals_compacted_head(N):
    """The fused heads + loss kernel with the constant mask {0, 2, 3} on a 5-action head against the unmasked call on the head's rows
    0, 2, 3: loss, the six statistics and every gradient are the same bits; rows 1 and 4 of the head get exactly zero."""
    from etm import ops
    dev = torch.device("cuda", 0)
    mods, head5, h, act3, adv, old_value, old_logp = _mask_problem(N, 384)
    res = []
    for masked in (True, False):
        dm = {k: copy.deepcopy(m).to(dev) for k, m in mods.items()}
        hd = copy.deepcopy(head5)
        if not masked:
            hd = torch.nn.Linear(384, 3)
            with torch.no_grad():
                hd.weight.copy_(head5.weight[KEEP]), hd.bias.copy_(head5.bias[KEEP])
        hd = hd.to(dev)
        x = h.to(dev).requires_grad_(True)
        actions = (torch.tensor(KEEP)[act3] if masked else act3).to(dev)
        am = torch.full((N,), KEEP_WORD, dtype=torch.int64, device=dev) if masked else None
        loss, st = ops.heads_ppo_loss(x, dm["lin_policy"], dm["lin_value"], hd, dm["value"], actions, old_logp.to(dev), adv.to(dev),
                                      old_value.to(dev), 0.2, 0.5, 0.01, action_mask=am)
        loss.backward()
        torch.cuda.synchronize()
        grads = {"h": x.grad, "head.w": hd.weight.grad, "head.b": hd.bias.grad}
        for k, m in dm.items():
            grads[k + ".w"], grads[k + ".b"] = m.weight.grad, m.bias.grad
        res.append((loss.detach().cpu().numpy(), st.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in grads.items()}))
    (l5, s5, g5), (l3, s3, g3) = res
    assert np.isfinite(s5).all() and np.array_equal(l5, l3) and np.array_equal(s5, s3)
    for k in g3:
        if k.startswith("head"):
            assert np.array_equal(g5[k][KEEP], g3[k]), k
            assert not g5[k][[1, 4]].any(), (k, "a masked row received a gradient")
        else:
            assert np.array_equal(g5[k], g3[k]), k


@pytest.mark.parametrize("N", [37, 300])
def test_ppo_loss_constant_mask_equals_compacted_logits(N):
    """``ops.ppo_loss`` with the constant mask on [N, 5] logits against the unmasked call on columns 0, 2, 3 of the same logits."""
    from etm import ops
    dev = torch.device("cuda", 0)
    _, _, _, act3, adv, old_value, old_logp = _mask_problem(N, 128)
    g = torch.Generator().manual_seed(N)
    logits5, value = 2.0 * torch.randn((N, 5), generator=g), torch.randn(N, generator=g)
    res = []
    for masked in (True, False):
        lg = (logits5 if masked else logits5[:, KEEP]).contiguous().to(dev).requires_grad_(True)
        v = value.to(dev).requires_grad_(True)
        actions = (torch.tensor(KEEP)[act3] if masked else act3).to(dev)
        am = torch.full((N,), KEEP_WORD, dtype=torch.int64, device=dev) if masked else None
        loss, st = ops.ppo_loss([lg], v, actions, old_logp.to(dev), adv.to(dev), old_value.to(dev), 0.2, 0.5, 0.01, action_mask=am)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().cpu().numpy(), st.detach().cpu().numpy(), lg.grad.cpu().numpy(), v.grad.cpu().numpy()))
    (l5, s5, dl5, dv5), (l3, s3, dl3, dv3) = res
    assert np.isfinite(s5).all() and np.array_equal(l5, l3) and np.array_equal(s5, s3) and np.array_equal(dv5, dv3)
    assert np.array_equal(dl5[:, KEEP], dl3) and not dl5[:, [1, 4]].any()


# ------------------------------------------------------------------ 3. loss against float64
def masked_ppo_loss64(logits_list, value, actions, old_logp, adv, old_values, valid_list, clip, vf_coef, beta):
    """The rule of ``action_masks`` in float64 (oracle ref_algo.ppo_loss with masks): per branch with valid set V the log-sum-exp runs
    over V only, log p_j = l_j - lse_V on V and p_j = 0 elsewhere, the entropy is -sum_{j in V} p_j log p_j (invalid columns are
    skipped, not multiplied); ratio, clipping, KL, clip fraction, value loss, advantage normalisation and scales are untouched."""
    logp, ent = [], []
    for b, (logits, valid) in enumerate(zip(logits_list, valid_list)):
        lsm = torch.log_softmax(logits.masked_fill(~valid, float("-inf")), dim=-1)
        logp.append(lsm.gather(1, actions[:, b:b + 1]).squeeze(1))
        ent.append(-(lsm.exp() * lsm.masked_fill(~valid, 0.0)).sum(-1))
    logp = torch.stack(logp, dim=1)
    entropy = torch.stack(ent, dim=1).sum(1)
    norm_adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).unsqueeze(1).repeat(1, len(logits_list))
    log_ratio = logp - old_logp
    ratio = torch.exp(log_ratio)
    policy = torch.min(ratio * norm_adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * norm_adv).mean()
    ret = old_values + adv
    clipped = old_values + (value - old_values).clamp(min=-clip, max=clip)
    vf = torch.max((value - ret) ** 2, (clipped - ret) ** 2).mean()
    loss = -(policy - vf_coef * vf + beta * entropy.mean())
    kl = ((ratio - 1.0) - log_ratio).mean()
    clip_frac = (abs(ratio - 1.0) > clip).double().mean()
    return loss, torch.stack([policy.detach(), vf.detach(), loss.detach(), entropy.mean().detach(), kl.detach(), clip_frac])


@pytest.mark.parametrize("hid", [128, 384])
@pytest.mark.parametrize("branches", [(5,), (2, 4, 2), (30, 5)], ids=["5", "242", "30_5_beyond"])
def test_masked_loss_vs_float64(branches, hid):
    import ctypes
    from etm import lib as etm_lib
    from etm import ops
    dev = torch.device("cuda", 0)
    N, clip, vf, beta = 37, 0.2, 0.5, 0.01
    B, A = len(branches), sum(branches)
    mods, heads, h, _, adv, old_value, g = md._heads_problem(N, branches, D=hid, hid=hid)
    # per-sample masks: random p = 0.5 with every branch kept non-empty; rows 0 .. 4 have ONE valid action per branch, row 5 all
    r = torch.rand((N, A), generator=g)
    valid, off = r >= 0.5, 0
    for a in branches:
        seg = valid[:, off:off + a]
        seg[torch.arange(N), r[:, off:off + a].argmax(dim=1)] = True
        seg[:5] = False
        seg[torch.arange(5), r[:5, off:off + a].argmax(dim=1)] = True
        off += a
    valid[5] = True
    words = torch.from_numpy(mh_pack(valid.numpy()))
    valid_list = list(valid.split(list(branches), dim=1))
    # a valid action per (sample, branch); old log-probs near the new ones, a quarter far off (clipped ratios)
    actions = torch.stack([torch.multinomial(v.float(), 1, generator=g)[:, 0] for v in valid_list], dim=1)
    with torch.no_grad():
        hp = torch.relu(h.double() @ mods["lin_policy"].weight.double().t() + mods["lin_policy"].bias.double())
        lp = torch.stack([torch.log_softmax((hp @ hd.weight.double().t() + hd.bias.double()).masked_fill(~v, float("-inf")), -1)
                          .gather(1, actions[:, k:k + 1])[:, 0] for k, (hd, v) in enumerate(zip(heads, valid_list))], dim=1)
        far = torch.randint(0, 4, (N, B), generator=g) == 1
        shift = torch.where(far, 0.5 * torch.randn(N, B, generator=g).double(), 0.03 * torch.randn(N, B, generator=g).double())
    old_logp = (lp - shift).float()
    tab = (ctypes.c_int32 * B)(*branches)
    fused = bool(etm_lib.load().etm_heads_loss_supported_branched(N, hid, tab, B))
    assert fused == (A <= 8)

    dm = {k: copy.deepcopy(m).to(dev) for k, m in mods.items()}
    dh = [copy.deepcopy(x).to(dev) for x in heads]
    x = h.to(dev).requires_grad_(True)
    am = words.to(dev)
    if fused:
        loss, st = ops.heads_ppo_loss(x, dm["lin_policy"], dm["lin_value"], dh if B > 1 else dh[0], dm["value"], actions.to(dev), old_logp.to(dev),
                                      adv.to(dev), old_value.to(dev), clip, vf, beta, action_mask=am)
    else:
        hp_, hv_ = ops.linear_relu(dm["lin_policy"], x), ops.linear_relu(dm["lin_value"], x)
        loss, st = ops.ppo_loss([m(hp_) for m in dh], dm["value"](hv_).reshape(-1), actions.to(dev), old_logp.to(dev), adv.to(dev),
                                old_value.to(dev), clip, vf, beta, action_mask=am)
    loss.backward()
    torch.cuda.synchronize()
    got = {"h": x.grad, **{f"{k}.{s}": getattr(dm[k], n).grad for k in dm for s, n in (("w", "weight"), ("b", "bias"))}}
    for i, m in enumerate(dh):
        got[f"branch{i}.w"], got[f"branch{i}.b"] = m.weight.grad, m.bias.grad

    P = {f"{k}.{s}": getattr(mods[k], n).detach().double().requires_grad_(True) for k in mods for s, n in (("w", "weight"), ("b", "bias"))}
    HB = [(m.weight.detach().double().requires_grad_(True), m.bias.detach().double().requires_grad_(True)) for m in heads]
    x64 = h.double().requires_grad_(True)
    hp64 = torch.relu(x64 @ P["lin_policy.w"].t() + P["lin_policy.b"])
    hv64 = torch.relu(x64 @ P["lin_value.w"].t() + P["lin_value.b"])
    ref_loss, ref_st = masked_ppo_loss64([hp64 @ w.t() + b_ for w, b_ in HB], (hv64 @ P["value.w"].t() + P["value.b"]).reshape(-1), actions,
                                         old_logp.double(), adv.double(), old_value.double(), valid_list, clip, vf, beta)
    ref_loss.backward()
    ref = {"h": x64.grad, **{k: v.grad for k, v in P.items()}}
    for i, (w, b_) in enumerate(HB):
        ref[f"branch{i}.w"], ref[f"branch{i}.b"] = w.grad, b_.grad

    st = st.detach().cpu().double()
    assert bool(torch.isfinite(st).all()) and np.isfinite(float(loss.detach()))
    e_stats = [abs(float(st[i] - ref_st[i])) / max(1.0, abs(float(ref_st[i]))) for i in range(6)]
    e_stats.append(abs(float(loss.detach()) - float(ref_loss)) / max(1.0, abs(float(ref_loss))))
    e_grad = {}
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), (k, "NaN / Inf")
        e_grad[k] = float((got[k].detach().cpu().double() - ref[k]).norm() / ref[k].norm().clamp(min=1e-30))
    print(f"[masked loss] hid={hid} {branches} fused={fused} stats {max(e_stats):.2e} grad {max(e_grad.values()):.2e} ({max(e_grad, key=e_grad.get)})")
    assert max(e_stats) <= HEADS_BOUNDS["stats"], e_stats
    for k, e in e_grad.items():
        assert e <= HEADS_BOUNDS["grad"], (k, e)
    # d loss / d l_j = 0 exactly outside V: an action that no sample allows gets exactly zero in its row of the branch head
    off = 0
    for i, a in enumerate(branches):
        never = ~valid[:, off:off + a].any(dim=0)
        assert not bool(got[f"branch{i}.w"].cpu()[never].any()) and not bool(got[f"branch{i}.b"].cpu()[never].any())
        off += a


def mh_pack(valid):
    from environments import pack_action_masks
    return pack_action_masks(valid).view(np.int64)


# ------------------------------------------------------------------ 4. whole trainer
def _small_masked_config(graph):
    from yaml_parser import YamlParser
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = YamlParser(os.path.join(repo, "episodic-transformer-memory-ppo_amd", "configs", "synthetic_multidiscrete_masked.yaml")).get_config()
    assert cfg["action_masks"] is True and cfg["environment"]["action_mask_p"] == 0.3
    cfg.update(n_workers=4, worker_steps=24, epochs=1, n_mini_batch=4, hip_graph_train=graph)
    cfg["environment"] = dict(cfg["environment"], pool=8, gen_threads=1, copy_threads=1, p_done=0.06)
    return cfg


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_synthetic_masked_update_vs_float64(graph):
    from environments import empty_mask_branches
    from oracle import ref_model as rm
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    cfg = _small_masked_config(graph)
    torch.manual_seed(3)
    tr = PPOTrainer(cfg, run_id="mask_update", device=dev, tensorboard=False)
    try:
        assert tr.action_space_shape == (3, 3) and tr._masked
        before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        names = [n for n, p in tr.model.named_parameters() if p.requires_grad]
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()
        assert tr.model._rf is not None and tr._groups[0].rf_scratch is not None
        b = tr.buffer
        words = b.action_masks.cpu().numpy()
        assert not empty_mask_branches(words.reshape(-1), (3, 3)).any() and 0.6 < tr.last_valid_action_share < 0.9
        valid = _valid_columns(words.reshape(-1), 6, dev)                                  # [N, 6]
        acts = b.actions.reshape(-1, 2)
        assert bool(valid[:, :3].gather(1, acts[:, :1]).all()) and bool(valid[:, 3:].gather(1, acts[:, 1:]).all())
        assert bool(torch.isfinite(b.log_probs).all())
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
        v_mb = valid.index_select(0, idx)
        loss, _ = masked_ppo_loss64(logits, value, sf["actions"].index_select(0, idx), sf["log_probs"].index_select(0, idx).double(),
                                    sf["advantages"].index_select(0, idx).double(), sf["values"].index_select(0, idx).double(),
                                    [v_mb[:, :3], v_mb[:, 3:]], clip, cfg["value_loss_coefficient"], beta)
        ref = torch.autograd.grad(loss, [sd[n] for n in names])
        worst = 0.0
        for n, gd, gr in zip(names, first["g"], ref):
            e = float((gd.double() - gr).norm() / gr.norm().clamp(min=1e-30))
            worst = max(worst, e)
            assert bool(torch.isfinite(gd).all()), n
            assert e <= 7e-6, (n, e)
        print(f"[mask update] graph={graph} worst gradient error {worst:.2e}")
        for n, p in tr.model.named_parameters():
            assert bool(torch.isfinite(p).all()), n
    finally:
        md._release(tr)


# ------------------------------------------------------------------ 5. an environment that raises on an illegal action
class _StrictEnv(mh._GridEnv):
    """``_GridEnv`` of the host tests (raises on an action its mask forbids) with episodes of 5 steps and a time limit of 12."""

    def __init__(self, worker_id=0):
        super().__init__(worker_id, length=5)
        self.max_episode_steps = 12


def test_strict_environment_survives_rollout_and_greedy_evaluation(monkeypatch):
    import utils
    from trainer import PPOTrainer
    monkeypatch.setattr(utils, "create_env", lambda cfg, worker_id=0, **kw: _StrictEnv(worker_id), raising=True)
    c = md._case("strict", (2, 3), 128, 2, 8, 8)
    cfg = md._config(c)
    cfg["environment"] = dict(type="Grid", vectorize="serial")
    cfg.update(action_masks=True, worker_steps=16)
    torch.manual_seed(1)
    tr = PPOTrainer(cfg, run_id="strict", device=torch.device("cuda", 0), tensorboard=False)
    try:
        assert tr.action_space_shape == (2, 3) and tr._masked
        infos = tr._sample_training_data()                     # an illegal action would raise inside env.step
        assert len(infos) == 8 * 3 and tr.last_valid_action_share == 0.6
        ev = tr.evaluate(episodes_per_worker=2, n_workers=8, deterministic=True, seed=50)
        assert len(ev["episodes"]) == 16 and all(e["length"] == 5 for e in ev["episodes"])
    finally:
        md._release(tr)
