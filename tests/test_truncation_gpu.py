"""-m gpu: time-limit bootstrapping (``bootstrap_truncated``) -- the GAE select kernel and the trainer around it.

1. ``etm_gae_truncated`` bit for bit against a float32 numpy loop (select form, separate multiplies and adds) at every worker / step
   count at which the kernel takes another path, flags at the tile and lane edges, ``boot`` NaN wherever no flag is set.
2. The defining equivalence on a scripted deterministic environment: a rollout whose every worker is cut at its last step, key on,
   against the same rollout never cut, key off -- the bootstrap values are ``get_last_value()``'s and the advantages agree; with the
   key off the cut rollout's last advantage is r - v.
3. Mid-rollout bookkeeping: records, flags, slots and windows rebuilt by the test; advantages bit-identical to the numpy loop on the
   buffer's own arrays; the returned infos carry neither new key; one PocMemoryEnv run with two worker groups.
4. Key on with nothing to bootstrap = key off, bit for bit, without a forward pass; one full ``run_training`` on a truncating environment.

Measured on the MI355X (profiles/r11/truncation.txt): every difference of 2. and 3. is 0 -- the bootstrap pass and get_last_value run
the same fp32 kernels at the same batch shape (W rows) -- so both assert equality; the bound that would apply otherwise is the
project's per-tensor floor of the kink-free tests, 2e-6 (tests/test_gpu_parity.py:NOKINK_GRAD_REL).
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

@pytest.fixture(autouse=True)
def _collect_between_tests():
    """Every test builds trainers that capture HIP graphs: collect the previous test's garbage first."""
    gc.collect()
    yield
    gc.collect()


def _release(tr):
    tr.close()
    del tr
    gc.collect()
    torch.cuda.synchronize()


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------ 1. the kernel
def gae_truncated_numpy(r, d, tr, v, boot, last, gamma, lamda):
    """The definition, float32 with every product and sum rounded on its own:
    next = tr ? boot : v_{t+1} * (1 - done);  delta = (r + gamma * next) - v;  la = delta + gamma_lambda * (la * (1 - done))."""
    g, gl = np.float32(gamma), np.float32(gamma * lamda)
    W, S = r.shape
    adv = np.empty_like(r)
    nv, la = last.astype(np.float32).copy(), np.zeros(W, dtype=np.float32)
    for t in range(S - 1, -1, -1):
        m = (~d[:, t]).astype(np.float32)
        nxt = np.where(tr[:, t], boot[:, t], nv * m).astype(np.float32)
        la = la * m
        delta = (r[:, t] + g * nxt) - v[:, t]
        la = delta + gl * la
        adv[:, t] = la
        nv = v[:, t]
    return adv


def _kernel_case(W, S, seed):
    """Random terminations (one step in ten), half of them flagged as truncations, plus truncations at t = 0, S - 1, the tile edge
    (63, 64), a lane edge (3, 4) and two consecutive steps (9, 10) on every other worker; boot is NaN wherever no flag is set."""
    rng = np.random.default_rng(seed)
    r = rng.normal(size=(W, S)).astype(np.float32)
    v = rng.normal(size=(W, S)).astype(np.float32)
    last = rng.normal(size=(W,)).astype(np.float32)
    d = rng.random((W, S)) < 0.1
    tr = d & (rng.random((W, S)) < 0.5)
    for t in (0, S - 1, 63, 64, 3, 4, 9, 10):
        if 0 <= t < S:
            d[::2, t] = True
            tr[::2, t] = True
    boot = np.full((W, S), np.nan, dtype=np.float32)
    boot[tr] = rng.normal(size=int(tr.sum())).astype(np.float32)
    return r, d, tr, v, boot, last


def _offset_view(x, dev):
    """``x`` on the device inside a [W, S + 1] allocation, starting one ELEMENT behind its beginning: the same values, contiguous, at
    an address that is not a multiple of 16 (floats) / 4 (flag bytes)."""
    t = torch.from_numpy(x)
    store = torch.zeros(x.shape[0] * (x.shape[1] + 1), dtype=t.dtype, device=dev)
    view = store[1: 1 + t.numel()].view(x.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % (4 * t.element_size()) != 0
    return view


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("S", (1, 3, 4, 63, 64, 65, 130))
@pytest.mark.parametrize("W", (1, 5, 16, 17, 33))
def test_gae_truncated_kernel_bit_for_bit(W, S):
    from etm import ops
    dev = _dev()
    r, d, tr, v, boot, last = _kernel_case(W, S, 1000 * W + S)
    ref = gae_truncated_numpy(r, d, tr, v, boot, last, 0.99, 0.95)
    assert np.isfinite(ref).all() and tr.any() and (tr <= d).all()
    to = lambda x: torch.from_numpy(x).to(dev)
    got = ops.gae(to(r), to(d), to(v), to(last), 0.99, 0.95, truncated=to(tr), boot=to(boot)).cpu().numpy()
    assert np.isfinite(got).all(), "an element of boot without a flag entered the result"
    assert _same_bits(got, ref), np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:8]
    # the key matters: the plain kernel differs wherever a truncation was flagged
    plain = ops.gae(to(r), to(d), to(v), to(last), 0.99, 0.95).cpu().numpy()
    assert not _same_bits(plain, ref)


@pytest.mark.parametrize("which", ("rewards", "values", "truncated", "boot", "out", "all"))
def test_gae_truncated_kernel_unaligned_arrays(which):
    """S % 4 == 0 at addresses that rule the vector loads out, one array at a time and all together."""
    from etm import ops
    dev, W, S = _dev(), 17, 64
    r, d, tr, v, boot, last = _kernel_case(W, S, 77)
    ref = gae_truncated_numpy(r, d, tr, v, boot, last, 0.99, 0.95)
    place = lambda name, x: _offset_view(x, dev) if which in (name, "all") else torch.from_numpy(x).to(dev)
    out = _offset_view(np.zeros((W, S), dtype=np.float32), dev) if which in ("out", "all") else torch.zeros((W, S), device=dev)
    got = ops.gae(place("rewards", r), place("dones", d), place("values", v), torch.from_numpy(last).to(dev), 0.99, 0.95, out=out,
                  truncated=place("truncated", tr), boot=place("boot", boot))
    assert got.data_ptr() == out.data_ptr()
    assert _same_bits(got.cpu().numpy(), ref)


@pytest.mark.parametrize("W,S", ((5, 3), (17, 64), (33, 130), (16, 65)))
def test_gae_truncated_without_flags_is_the_plain_kernel(W, S):
    from etm import ops
    dev = _dev()
    r, d, _, v, _, last = _kernel_case(W, S, 5)
    to = lambda x: torch.from_numpy(x).to(dev)
    plain = ops.gae(to(r), to(d), to(v), to(last), 0.99, 0.95).cpu().numpy()
    got = ops.gae(to(r), to(d), to(v), to(last), 0.99, 0.95, truncated=torch.zeros((W, S), dtype=torch.bool, device=dev),
                  boot=torch.full((W, S), float("nan"), device=dev)).cpu().numpy()
    assert _same_bits(got, plain)
    with pytest.raises(TypeError, match="come together"):
        ops.gae(to(r), to(d), to(v), to(last), 0.99, 0.95, truncated=torch.zeros((W, S), dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="truncated / boot"):
        ops.gae(to(r), to(d), to(v), to(last), 0.99, 0.95, truncated=torch.zeros((W, S + 1), dtype=torch.bool, device=dev),
                boot=torch.zeros((W, S + 1), device=dev))


# ------------------------------------------------------------------ the scripted environment and the small trainer
class ScriptedVecEnv:
    """W deterministic environments behind the VecEnv protocol.  Observation of worker w at episode step s: a fixed function of
    (w, s); reward of the step taken at episode step s: a function of s; actions are ignored.  Worker w's episodes are cut
    (``"truncated": True`` when ``report``) after ``cut_at(w)`` steps and at ``max_episode_steps``, and end genuinely after
    ``ends_at(w)`` steps (None: never).  ``log`` [W, steps] records the truncations by rollout step."""

    def __init__(self, W, cut_at=None, ends_at=None, report=True, max_episode_steps=24):
        self.num_envs, self.observation_space_shape = W, (5,)
        self.action_space_shape, self.num_actions = (3,), 3
        self.max_episode_steps = max_episode_steps
        self.cut_at = cut_at if callable(cut_at) else (lambda w, c=cut_at: c)
        self.ends_at = ends_at if callable(ends_at) else (lambda w, c=ends_at: c)
        self.report = report
        self.s = np.zeros(W, dtype=np.int64)
        self.t = 0
        self.log = []           # per step: [W] bool
        self.ended = []         # per step: [W] bool (genuine ends)

    @staticmethod
    def observation(w, s):
        return np.sin(0.37 * (w + 1) + 0.61 * s + 0.9 * np.arange(5)).astype(np.float32)

    @staticmethod
    def reward(s):
        return np.float32(0.25 * np.cos(0.8 * s) - 0.1)

    def reset(self, out=None):
        out = np.zeros((self.num_envs, 5), dtype=np.float32) if out is None else out
        self.s[:] = 0
        for w in range(self.num_envs):
            out[w] = self.observation(w, 0)
        return out

    def step(self, actions, out=None, on_rows=None):
        W = self.num_envs
        out = np.zeros((W, 5), dtype=np.float32) if out is None else out
        rewards, dones, infos = np.zeros(W, dtype=np.float32), np.zeros(W, dtype=bool), [None] * W
        cut, ended = np.zeros(W, dtype=bool), np.zeros(W, dtype=bool)
        for w in range(W):
            rewards[w] = self.reward(self.s[w])
            self.s[w] += 1
            s = int(self.s[w])
            obs = self.observation(w, s)
            if self.ends_at(w) is not None and s == self.ends_at(w):
                dones[w] = ended[w] = True
                infos[w] = {"reward": float(s), "length": s}
            elif s == self.max_episode_steps or (self.cut_at(w) is not None and s == self.cut_at(w)):
                dones[w] = cut[w] = True
                infos[w] = {"reward": float(s), "length": s}
                if self.report:
                    infos[w]["truncated"] = True
                    infos[w]["final_observation"] = obs.copy()
            if dones[w]:
                self.s[w] = 0
                obs = self.observation(w, 0)
            out[w] = obs
        if on_rows is not None:
            on_rows(0, W)
        self.log.append(cut)
        self.ended.append(ended)
        self.t += 1
        return out, rewards, dones, infos

    def close(self):
        pass


def _config(S, W=8, **over):
    cfg = dict(environment=dict(type="Scripted"), gamma=0.99, lamda=0.95, updates=2, epochs=1, n_workers=W, worker_steps=S,
               n_mini_batch=2, value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False,
               transformer=dict(num_blocks=2, embed_dim=64, num_heads=1, memory_length=8, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    cfg.update(over)
    return cfg


def _trainer(cfg, env, seed=11):
    from trainer import PPOTrainer
    torch.manual_seed(seed)
    return PPOTrainer(cfg, run_id="trunc", device=_dev(), env=env, tensorboard=False)


def _forced(W, S):
    return (np.arange(W)[:, None] + np.arange(S)[None, :]) % 3


def _profile_line(text):
    """A measured figure, printed before anything is asserted on it (pytest -s shows it)."""
    print("\n[truncation] " + text, flush=True)


# ------------------------------------------------------------------ 2. the defining equivalence
@pytest.mark.parametrize("S", (12, 5), ids=["s_ge_L", "s_lt_L"])
def test_cut_at_the_last_step_equals_the_uncut_rollout(S):
    W = 8
    # A: every worker is cut at t = S - 1, reported, key on
    a = _trainer(_config(S, bootstrap_truncated=True), ScriptedVecEnv(W, cut_at=S))
    try:
        infos = a._sample_training_data(forced_actions=_forced(W, S))
        assert len(infos) == W and all(set(i) == {"reward", "length"} for i in infos)
        assert a.last_truncations == [(w, S - 1, w, S) for w in range(W)]
        assert a.buffer.truncated[:, S - 1].all() and not a.buffer.truncated[:, :S - 1].any()
        a_boot = a.buffer.bootstrap_values.cpu().numpy()
        a_adv, a_val = a.buffer.advantages.cpu().numpy(), a.buffer.values.cpu().numpy()
    finally:
        _release(a)
    # B: never cut, key off
    b = _trainer(_config(S), ScriptedVecEnv(W))
    try:
        assert b.buffer.truncated is None and b.buffer.bootstrap_values is None and not hasattr(b, "_bs")
        assert b._sample_training_data(forced_actions=_forced(W, S)) == []
        b_last = b.get_last_value().cpu().numpy().copy()
        b_adv, b_val = b.buffer.advantages.cpu().numpy(), b.buffer.values.cpu().numpy()
    finally:
        _release(b)
    assert np.array_equal(a_val, b_val), "the same rollout up to the cut"
    assert (a_boot[:, :S - 1] == 0).all()
    rel_boot, rel_adv = _rel(a_boot[:, S - 1], b_last), _rel(a_adv, b_adv)
    _profile_line(f"equivalence S={S}: bootstrap values vs get_last_value rel={rel_boot:.3e} max_abs="
                  f"{np.abs(a_boot[:, S - 1] - b_last).max():.3e}; advantages rel={rel_adv:.3e}")
    assert np.array_equal(a_boot[:, S - 1], b_last) and np.array_equal(a_adv, b_adv), (rel_boot, rel_adv)
    # A': the same cut rollout with the key off -- the value after the cut counts as 0
    c = _trainer(_config(S), ScriptedVecEnv(W, cut_at=S))
    try:
        infos = c._sample_training_data(forced_actions=_forced(W, S))
        assert len(infos) == W and all(set(i) == {"reward", "length"} for i in infos) and c.last_truncations == []
        c_adv, c_val = c.buffer.advantages.cpu().numpy(), c.buffer.values.cpu().numpy()
        r = c.buffer.rewards[:, S - 1].astype(np.float32)
    finally:
        _release(c)
    assert np.array_equal(c_val, a_val)
    assert np.array_equal(c_adv[:, S - 1], r - c_val[:, S - 1]), "key off: adv = r - v at a cut"
    assert not np.array_equal(c_adv[:, S - 1], a_adv[:, S - 1]), "the key matters"


# ------------------------------------------------------------------ 3. mid-rollout bookkeeping
def _check_rollout_against_rebuild(tr, env, S, tag):
    """Every record of the last rollout rebuilt by hand -> the value at buffer.bootstrap_values[w, t]; flags; advantages."""
    from etm.ops import WindowSpec
    buf, L, W = tr.buffer, tr.memory_length, tr.num_workers
    log, ended = np.stack(env.log[-S:], axis=1), np.stack(env.ended[-S:], axis=1)
    assert np.array_equal(buf.truncated, log), "buffer.truncated is the environment's own log"
    assert not buf.truncated[ended].any() and buf.dones[ended].all() and buf.dones[log].all()
    recs = tr.last_truncations
    assert sorted((w, t) for w, t, _, _ in recs) == sorted(map(tuple, np.argwhere(log)))
    boot = buf.bootstrap_values.cpu().numpy()
    assert (boot[~log] == 0).all()
    mem_index = buf.memory_index_host
    worst = 0.0
    for w, t, slot, s in recs:
        assert slot == mem_index[w, t], "the slot of the episode that was cut, not of the one opened after it"
        first = t - s + 1                      # rollout step of the episode's first step (negative: it began in an earlier rollout)
        assert first <= 0 or buf.dones[w, first - 1], (w, t, s)
        # (the record's row W times: the batch shape the pass and get_last_value run at)
        rows = (torch.clamp(torch.tensor([s - L]), min=0).unsqueeze(1) + torch.arange(L).unsqueeze(0)).repeat(W, 1)
        mask = tr._mask_table[min(max(s, 0), L - 1)].unsqueeze(0).repeat(W, 1)
        pidx = buf.memory_indices[w, t].unsqueeze(0).repeat(W, 1)
        obs = torch.from_numpy(env.observation(w, s)).unsqueeze(0).repeat(W, 1).to(tr.device)
        with torch.no_grad():
            spec = WindowSpec.from_bank(buf.bank, torch.full((W,), slot, device=tr.device), rows.to(tr.device), pidx, mask)
            value = tr.model.forward_logits(obs, spec, want_items=False)[1].cpu().numpy()
        assert (value == value[0]).all()
        worst = max(worst, abs(float(value[0]) - float(boot[w, t])) / max(abs(float(value[0])), 1e-30))
    _profile_line(f"bookkeeping {tag}: {len(recs)} records, bootstrap value vs the test's own forward pass, worst relative difference {worst:.3e}")
    assert worst == 0.0, worst
    ref = gae_truncated_numpy(buf.rewards.astype(np.float32), buf.dones.copy(), buf.truncated.copy(), buf.values.cpu().numpy(), boot,
                              tr._lv.out.cpu().numpy(), tr.config["gamma"], tr.config["lamda"])
    assert _same_bits(buf.advantages.cpu().numpy(), ref)
    return recs


@pytest.mark.parametrize("graph", (True, False), ids=["graph", "eager"])
def test_mid_rollout_truncations(graph):
    W, S = 8, 20
    env = ScriptedVecEnv(W, cut_at=lambda w: None if w < 2 else 7 + (w % 3), ends_at=lambda w: 4 if w < 2 else None)
    tr = _trainer(_config(S, bootstrap_truncated=True, hip_graph_rollout=graph), env)
    try:
        for rollout in range(3):               # (the third one replays the captured bootstrap pass when graphs are on)
            infos = tr._sample_training_data(forced_actions=_forced(W, S))
            assert infos and all(set(i) == {"reward", "length"} for i in infos), "neither new key reaches the episode infos"
            recs = _check_rollout_against_rebuild(tr, env, S, f"{'graph' if graph else 'eager'} rollout {rollout}")
            assert len(recs) > W and {w for w, _, _, _ in recs} == set(range(2, W))
            assert {s for _, _, _, s in recs} == {7, 8, 9}
        assert (tr._step_graph is not None) == graph
        if graph:
            assert tr._bs.graph is not None, "the bootstrap pass was not captured"
    finally:
        _release(tr)


def test_poc_memory_env_two_groups():
    """environment: {type: PocMemoryEnv, report_truncation: true} through SerialVecEnv parts, 16 workers in two rollout groups."""
    from trainer import PPOTrainer
    cfg = _config(40, W=16, bootstrap_truncated=True, rollout_groups=2,
                  environment=dict(type="PocMemoryEnv", seed=3, vectorize="serial", report_truncation=True))
    cfg["transformer"] = dict(cfg["transformer"], memory_length=32)
    torch.manual_seed(5)
    tr = PPOTrainer(cfg, run_id="truncpoc", device=_dev(), tensorboard=False)
    try:
        assert len(tr._groups) == 2
        # a policy that dithers never reaches an end: every episode is cut at 32 steps
        forced = np.broadcast_to(np.arange(40)[None, :] % 2, (16, 40)).copy()
        infos = tr._sample_training_data(forced_actions=forced)
        assert len(infos) == 16 and all(set(i) == {"success", "reward", "length"} and i["length"] == 32 for i in infos)
        expect = np.zeros((16, 40), dtype=bool)
        expect[:, 31] = True
        assert np.array_equal(tr.buffer.truncated, expect) and np.array_equal(tr.buffer.dones, expect)
        assert tr.last_truncations and all(t == 31 and s == 32 and slot == w for w, t, slot, s in tr.last_truncations)
        assert torch.isfinite(tr.buffer.advantages).all()
        assert (tr.buffer.bootstrap_values[:, 31] != 0).all()
    finally:
        _release(tr)


# ------------------------------------------------------------------ 4. no change when off or idle
def _two_updates(key_on):
    W, S = 8, 16
    env = ScriptedVecEnv(W, ends_at=lambda w: 5 + w)        # genuine ends only, well before max_episode_steps
    cfg = _config(S, **({"bootstrap_truncated": True} if key_on else {}))
    tr = _trainer(cfg, env)
    calls = [0]
    inner = tr.model.forward_logits

    def counted(*a, **k):
        calls[0] += 1
        return inner(*a, **k)

    tr.model.forward_logits = counted
    out = []
    try:
        for _ in range(2):
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            out.append((tr.buffer.advantages.cpu().numpy().copy(), tr.buffer.actions.cpu().numpy().copy(),
                        tr.optimizer.flat_params.detach().cpu().numpy().copy()))
        if key_on:
            assert tr.last_truncations == [] and not tr.buffer.truncated.any() and tr._bs.calls == 0 and tr._bs.graph is None
            assert not tr.buffer.bootstrap_values.any()
    finally:
        _release(tr)
    return out, calls[0]


def test_key_on_without_truncations_changes_nothing():
    off, calls_off = _two_updates(False)
    on, calls_on = _two_updates(True)
    assert calls_on == calls_off, "no bootstrap forward pass without a record"
    for (adv_a, act_a, par_a), (adv_b, act_b, par_b) in zip(off, on):
        assert _same_bits(adv_a, adv_b) and np.array_equal(act_a, act_b) and _same_bits(par_a, par_b)


class _StubWriter:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def close(self):
        pass


def test_run_training_on_a_truncating_environment(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    W, S = 8, 16
    env = ScriptedVecEnv(W, cut_at=lambda w: 6 + (w % 4), ends_at=lambda w: 3 if w == 0 else None)
    tr = _trainer(_config(S, bootstrap_truncated=True), env)
    try:
        tr.writer = _StubWriter()
        tr.run_training()
        losses = [v for t, v, _ in tr.writer.scalars if t.startswith("losses/")]
        assert len(losses) == 8 and np.isfinite(losses).all()
        assert {t for t, _, _ in tr.writer.scalars if t.startswith("episode/")} == {"episode/reward_mean", "episode/length_mean"}
        assert tr.last_truncations and torch.isfinite(tr.buffer.advantages).all()
    finally:
        _release(tr)
