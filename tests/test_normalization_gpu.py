"""-m gpu: running observation and return normalisation -- the three kernels of csrc/running_norm.hip and the trainer around them.

1. ``etm_obs_stats_update`` against EXACT rational statistics (tests/normalization_reference.py): count equal, mean and M2 within
   1e-10 relative (TRIPLE_REL there: ~50 x the worst case of an ordered double sum of 16,384 terms), the fp32 table within 1 ulp of the
   exact value rounded to fp32, identical bits from run to run.
2. ``etm_obs_normalize`` bit for bit against the float32 numpy expression, with and without the row gather.
3. ``etm_return_scale``: the carry bit for bit against the float64 numpy recurrence, the triple against the exact one, scale and scaled
   rewards within 1 fp32 ulp, two halves of a rollout = the whole.
4. Table equivalence through the trainer: a trainer with ``normalize_observations`` and a hand-written table computes the same bits as
   a trainer without the key on an environment that emits the normalised rows -- rollout, optimisation, a second round on the
   refreshed table through the captured graphs --; the evaluator reads the refreshed table.
5. ``normalize_rewards`` through the trainer, with and without a time-limit truncation.
6. A checkpoint of the normalising trainer evaluated through evaluate.py's path.
"""
import gc
import pickle

import numpy as np
import pytest
import torch

import normalization_reference as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _collect_between_tests():
    """Every trainer test captures HIP graphs: collect the previous test's garbage first."""
    gc.collect()
    yield
    gc.collect()


def _release(*trainers):
    for tr in trainers:
        tr.close()
    del trainers
    gc.collect()
    torch.cuda.synchronize()


def _dev():
    return torch.device("cuda", 0)


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _figure(text):
    """A measured figure, printed before anything is asserted on it (pytest -s shows it)."""
    print("\n[normalization] " + text, flush=True)


# ------------------------------------------------------------------ 1. etm_obs_stats_update
EPS = 1e-8
# (R, F): the issue's shapes, one row past the chunk of 256 rows, the widest supported row with a few rows
STATS_SHAPES = ((1, 1), (7, 3), (64, 4), (1000, 17), (4099, 33), (257, 5), (3, 1024))


def _stats_data(R, F, seed):
    """fp32 draws with a per-feature offset and scale, |mean| <= 10 std; the last feature (F >= 2) is constant."""
    rng = np.random.default_rng(seed)
    std = 10.0 ** rng.uniform(-3, 3, size=F)
    off = std * rng.uniform(-10, 10, size=F)
    x = (off + std * rng.normal(size=(R, F))).astype(np.float32)
    if F >= 2:
        x[:, F - 1] = np.float32(-3.75)
    return x


def _check_triple(stats, mean, rstd, data, tag):
    """The kernel's triple and table against the exact statistics of ``data`` [R, F]."""
    exact = nr.exact_triples_per_feature(data)
    worst_mean = worst_m2 = 0.0
    for f, (n, m, q) in enumerate(exact):
        scale = float(np.abs(data[:, f]).max()) or 1.0
        assert stats[0, f] == n, (tag, f)
        worst_mean = max(worst_mean, nr.triple_error(stats[1, f], m, scale))
        worst_m2 = max(worst_m2, nr.triple_error(stats[2, f], q, scale * scale))
    want_mean = np.array([nr.round_to_f32(e[1]) for e in exact], dtype=np.float32)
    want_rstd = np.array([nr.exact_rstd_f32(e[0], e[2], EPS) for e in exact], dtype=np.float32)
    u_mean, u_rstd = int(nr.ulps32(mean, want_mean).max()), int(nr.ulps32(rstd, want_rstd).max())
    _figure(f"obs_stats {tag}: mean rel {worst_mean:.2e}, M2 rel {worst_m2:.2e} (bound {nr.TRIPLE_REL:.0e}); table ulps mean {u_mean} rstd {u_rstd}")
    assert worst_mean <= nr.TRIPLE_REL and worst_m2 <= nr.TRIPLE_REL
    assert u_mean <= 1 and u_rstd <= 1


@pytest.mark.parametrize("R,F", STATS_SHAPES)
def test_obs_stats_update_against_exact_statistics(R, F):
    from etm import ops
    dev = _dev()
    a, b = _stats_data(R, F, 100 * R + F), _stats_data(max(1, R // 2 + 3), F, 7 * R + F + 1)
    runs = []
    for _ in range(2):                 # the same input twice: identical bits
        stats = torch.zeros((3, F), dtype=torch.float64, device=dev)
        mean, rstd = torch.full((F,), 9.0, device=dev), torch.full((F,), 9.0, device=dev)
        ptrs = (stats.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        ops.obs_stats_update(_to(a), stats, mean, rstd, EPS)
        first = (stats.cpu().numpy().copy(), mean.cpu().numpy().copy(), rstd.cpu().numpy().copy())
        ops.obs_stats_update(_to(b), stats, mean, rstd, EPS)
        assert ptrs == (stats.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        runs.append(first + (stats.cpu().numpy(), mean.cpu().numpy(), rstd.cpu().numpy()))
    for x, y in zip(*runs):
        assert _same_bits(x, y), "two runs on the same input differ"
    s1, m1, r1, s2, m2, r2 = runs[0]
    _check_triple(s1, m1, r1, a, f"({R}, {F}) first merge")
    _check_triple(s2, m2, r2, np.concatenate([a, b]), f"({R}, {F}) second merge")
    if F >= 2:
        assert s1[2, F - 1] == 0.0 and r1[F - 1] == np.float32(1.0 / np.sqrt(EPS)), "a constant feature has M2 = 0 exactly"


def test_obs_stats_update_refuses_what_it_does_not_take():
    from etm import ops
    dev = _dev()
    assert ops.obs_stats_supported(1) and ops.obs_stats_supported(1024) and not ops.obs_stats_supported(0) and not ops.obs_stats_supported(1025)
    x = torch.zeros((4, 3), device=dev)
    good = (torch.zeros((3, 3), dtype=torch.float64, device=dev), torch.zeros(3, device=dev), torch.ones(3, device=dev))
    with pytest.raises(TypeError, match="float64"):
        ops.obs_stats_update(x, good[0].float(), good[1], good[2], EPS)
    with pytest.raises(ValueError, match="1 to 1024"):
        ops.obs_stats_update(torch.zeros((2, 1025), device=dev), torch.zeros((3, 1025), dtype=torch.float64, device=dev),
                             torch.zeros(1025, device=dev), torch.ones(1025, device=dev), EPS)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.obs_stats_update(x.cpu(), *good, EPS)


# ------------------------------------------------------------------ 2. etm_obs_normalize
CLIP = 2.5


def _normalize_case(N, F, seed, rows=None):
    """A table whose feature 0 is (mean 1, rstd 0.5) -- x = 1 + 2 c lands exactly on +c, its float32 neighbours just inside and just
    beyond -- and random elsewhere; rows 0 .. 5 of x hold those values in every feature they fit."""
    rng = np.random.default_rng(seed)
    rows = N if rows is None else rows
    mean = (rng.normal(size=F) * 20).astype(np.float32)
    rstd = (1.0 / (0.05 + 5 * rng.random(F))).astype(np.float32)
    mean[0], rstd[0] = 1.0, 0.5
    x = (mean + 1.5 * rng.normal(size=(rows, F)) / rstd).astype(np.float32)
    on = np.float32(1.0 + 2.0 * CLIP)
    edge = [on, np.nextafter(on, np.float32(np.inf)), np.nextafter(on, np.float32(0)), np.float32(1.0 - 2.0 * CLIP),
            np.nextafter(np.float32(1.0 - 2.0 * CLIP), np.float32(-np.inf)), np.float32(1e6)]
    for i, v in enumerate(edge[:rows]):
        x[i, 0] = v
    return x, mean, rstd


@pytest.mark.parametrize("indexed", (False, True), ids=["dense", "indexed"])
@pytest.mark.parametrize("F", (1, 4, 33))
@pytest.mark.parametrize("N", (1, 5, 64, 2049))
def test_obs_normalize_bit_for_bit(N, F, indexed):
    from etm import ops
    rows = N + 6 if indexed else N
    x, mean, rstd = _normalize_case(N, F, 31 * N + F, rows)
    if indexed:      # repeats and a non-monotone order; the rows with the values on and beyond the clip are among them
        rng = np.random.default_rng(N)
        idx = rng.integers(0, rows, size=N)
        idx[: min(N, 6)] = np.arange(min(N, 6))[::-1]
        if N >= 3:
            idx[-1] = idx[0]
        ref = nr.obs_normalize_f32(x[idx], mean, rstd, CLIP)
        got = ops.obs_normalize(_to(x), _to(mean), _to(rstd), CLIP, index=_to(idx.astype(np.int64)))
    else:
        ref = nr.obs_normalize_f32(x, mean, rstd, CLIP)
        got = ops.obs_normalize(_to(x), _to(mean), _to(rstd), CLIP)
    got = got.cpu().numpy()
    assert (ref[:, 0] == np.float32(CLIP)).any(), "the case holds a value on or beyond the clip"
    assert got.shape == ref.shape and _same_bits(got, ref), np.argwhere(_bits(got) != _bits(ref))[:8]


def test_obs_normalize_unaligned_rows_and_out():
    """F % 4 == 0 at addresses that rule the 16-byte accesses out; ``out=`` is written in place; NaN stays NaN."""
    from etm import ops
    dev = _dev()
    x, mean, rstd = _normalize_case(70, 8, 5)
    x[9, 3] = np.nan
    ref = nr.obs_normalize_f32(x, mean, rstd, CLIP)
    store = torch.zeros(70 * 8 + 1, device=dev)
    xv = store[1:].view(70, 8)
    xv.copy_(torch.from_numpy(x))
    assert xv.data_ptr() % 16 != 0
    out = torch.empty((70, 8), device=dev)
    got = ops.obs_normalize(xv, _to(mean), _to(rstd), CLIP, out=out)
    assert got.data_ptr() == out.data_ptr() and _same_bits(got.cpu().numpy(), ref) and np.isnan(ref[9, 3])
    assert _same_bits(ops.obs_normalize(_to(x), _to(mean), _to(rstd), CLIP).cpu().numpy(), ref)


# ------------------------------------------------------------------ 3. etm_return_scale
GAMMA, RCLIP = 0.99, 1.25


def _dones(pattern, W, S, rng):
    d = np.zeros((W, S), dtype=bool)
    if pattern == "all":
        d[:] = True
    elif pattern == "first":
        d[:, 0] = True
    elif pattern == "last":
        d[:, S - 1] = True
    elif pattern == "random":
        d = rng.random((W, S)) < 0.2
    return d


def _call_return_scale(r, d, carry, stats):
    from etm import ops
    scaled, scale = ops.return_scale(_to(r), _to(d), carry, stats, GAMMA, EPS, RCLIP)
    return scaled.cpu().numpy(), scale.cpu().numpy().copy()


def _check_return_triple(stats, ref, tag):
    scale = float(np.abs(ref["every"]).max()) or 1.0
    e_mean, e_m2 = nr.triple_error(stats[1], ref["mean"], scale), nr.triple_error(stats[2], ref["m2"], scale * scale)
    _figure(f"return_scale {tag}: mean rel {e_mean:.2e}, M2 rel {e_m2:.2e} (bound {nr.TRIPLE_REL:.0e})")
    assert stats[0] == ref["count"] and e_mean <= nr.TRIPLE_REL and e_m2 <= nr.TRIPLE_REL


@pytest.mark.parametrize("pattern", ("none", "all", "first", "last", "random"))
@pytest.mark.parametrize("S", (1, 8, 129))
@pytest.mark.parametrize("W", (1, 3, 32))
def test_return_scale_kernel(W, S, pattern):
    dev = _dev()
    rng = np.random.default_rng(1000 * W + 10 * S + len(pattern))
    r = (0.3 + rng.normal(size=(W, S))).astype(np.float32)
    d = _dones(pattern, W, S, rng)
    carry0 = rng.normal(size=W) * 2            # the rollout continues earlier returns
    ref = nr.return_rule_exact(r, d, carry0, np.zeros(0), GAMMA, EPS, RCLIP)
    carry, stats = _to(carry0), torch.zeros(3, dtype=torch.float64, device=dev)
    scaled, scale = _call_return_scale(r, d, carry, stats)
    assert _same_bits(carry.cpu().numpy(), ref["carry"]), "ret_carry differs from the float64 recurrence"
    _check_return_triple(stats.cpu().numpy(), ref, f"W={W} S={S} {pattern}")
    u_scale, u_scaled = int(nr.ulps32(scale, ref["scale"]).max()), int(nr.ulps32(scaled, ref["scaled"]).max())
    _figure(f"return_scale W={W} S={S} {pattern}: ulps scale {u_scale} scaled {u_scaled}")
    assert u_scale <= 1 and u_scaled <= 1 and np.abs(scaled).max() <= np.float32(RCLIP)
    # a second rollout joins the running triple and continues the carry
    r2 = (rng.normal(size=(W, S)) * 3).astype(np.float32)
    ref2 = nr.return_rule_exact(r2, d, ref["carry"], ref["R"], GAMMA, EPS, RCLIP)
    scaled2, scale2 = _call_return_scale(r2, d, carry, stats)
    assert _same_bits(carry.cpu().numpy(), ref2["carry"])
    _check_return_triple(stats.cpu().numpy(), ref2, f"W={W} S={S} {pattern} second rollout")
    assert nr.ulps32(scale2, ref2["scale"]).max() <= 1 and nr.ulps32(scaled2, ref2["scaled"]).max() <= 1
    if S >= 2:      # two calls over the two halves of the first rollout
        h = S // 2
        carry_h, stats_h = _to(carry0), torch.zeros(3, dtype=torch.float64, device=dev)
        _call_return_scale(r[:, :h], d[:, :h], carry_h, stats_h)
        _call_return_scale(r[:, h:], d[:, h:], carry_h, stats_h)
        assert _same_bits(carry_h.cpu().numpy(), ref["carry"]), "two halves leave another carry than the whole"
        _check_return_triple(stats_h.cpu().numpy(), ref, f"W={W} S={S} {pattern} two halves")


def test_return_scale_kernel_vector_path_over_several_tiles():
    """S % 4 == 0 past two tiles of 64 steps, a last workgroup of one worker; twice: identical bits."""
    dev, W, S = _dev(), 17, 192
    rng = np.random.default_rng(3)
    r = rng.normal(size=(W, S)).astype(np.float32)
    d = rng.random((W, S)) < 0.05
    d[:, 63] = d[::2, 64] = True
    ref = nr.return_rule_exact(r, d, np.zeros(W), np.zeros(0), GAMMA, EPS, RCLIP)
    outs = []
    for _ in range(2):
        carry, stats = torch.zeros(W, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
        scaled, scale = _call_return_scale(r, d, carry, stats)
        outs.append((carry.cpu().numpy(), stats.cpu().numpy(), scaled, scale))
    for x, y in zip(*outs):
        assert _same_bits(x, y)
    assert _same_bits(outs[0][0], ref["carry"])
    _check_return_triple(outs[0][1], ref, "W=17 S=192")
    assert nr.ulps32(outs[0][3], ref["scale"]).max() <= 1 and nr.ulps32(outs[0][2], ref["scaled"]).max() <= 1


# ------------------------------------------------------------------ the scripted environment and the tiny trainer
F_OBS = 5
OFFSET = np.array([1000.0, -3.0, 0.0, 250.0, 1e-3], dtype=np.float32)
SCALE = np.array([50.0, 1e-3, 1.0, 1000.0, 1e-4], dtype=np.float32)


class OffsetVecEnv:
    """W deterministic environments behind the VecEnv protocol whose observations are offset and scaled per feature:
    obs(w, s) = OFFSET + SCALE * sin(...).  Rewards depend on (w, s); worker w's episodes end after ``ends_at(w)`` steps and are cut
    (reported as truncations) after ``cut_at(w)`` steps.  ``table`` = (mean, rstd, clip): the environment emits
    clamp((obs - mean) * rstd) computed in float32 numpy instead -- what a host-side wrapper would hand the trainer."""

    def __init__(self, W, ends_at=None, cut_at=None, table=None, max_episode_steps=16):
        self.num_envs, self.observation_space_shape = W, (F_OBS,)
        self.action_space_shape, self.num_actions = (3,), 3
        self.max_episode_steps = max_episode_steps
        self.ends_at = ends_at if callable(ends_at) else (lambda w, c=ends_at: c)
        self.cut_at = cut_at if callable(cut_at) else (lambda w, c=cut_at: c)
        self.table = table
        self.s = np.zeros(W, dtype=np.int64)

    def raw(self, w, s):
        return (OFFSET + SCALE * np.sin(0.37 * (w + 1) + 0.61 * s + 0.9 * np.arange(F_OBS)).astype(np.float32)).astype(np.float32)

    def observation(self, w, s):
        x = self.raw(w, s)
        if self.table is None:
            return x
        mean, rstd, clip = self.table
        return nr.obs_normalize_f32(x, mean, rstd, clip)

    @staticmethod
    def reward(w, s):
        return np.float32(0.02 * (w + 1) * np.cos(0.8 * s) + 0.05)

    def reset(self, out=None):
        out = np.zeros((self.num_envs, F_OBS), dtype=np.float32) if out is None else out
        self.s[:] = 0
        for w in range(self.num_envs):
            out[w] = self.observation(w, 0)
        return out

    def step(self, actions, out=None, on_rows=None):
        W = self.num_envs
        out = np.zeros((W, F_OBS), dtype=np.float32) if out is None else out
        rewards, dones, infos = np.zeros(W, dtype=np.float32), np.zeros(W, dtype=bool), [None] * W
        for w in range(W):
            rewards[w] = self.reward(w, self.s[w])
            self.s[w] += 1
            s = int(self.s[w])
            obs = self.observation(w, s)
            if self.ends_at(w) is not None and s == self.ends_at(w):
                dones[w] = True
                infos[w] = {"reward": float(s), "length": s}
            elif s == self.max_episode_steps or (self.cut_at(w) is not None and s == self.cut_at(w)):
                dones[w] = True
                infos[w] = {"reward": float(s), "length": s, "truncated": True, "final_observation": obs.copy()}
            if dones[w]:
                self.s[w] = 0
                obs = self.observation(w, 0)
            out[w] = obs
        if on_rows is not None:
            on_rows(0, W)
        return out, rewards, dones, infos

    def close(self):
        pass


W_T, S_T = 4, 16


def _config(**over):
    """W = 4, S = 16, memory_length 4, one block, the smallest widths the fused paths admit, one epoch, two minibatches.  The
    ``environment`` section is what the evaluator builds its own environments from (the trainers get theirs through ``env=``)."""
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[F_OBS], num_actions=3, max_episode_steps=16, seed=2, p_done=0.1, pool=4),
               gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=W_T, worker_steps=S_T, n_mini_batch=2,
               value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False,
               transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    cfg.update(over)
    return cfg


def _trainer(cfg, env, seed=11, run_id="norm"):
    from trainer import PPOTrainer
    torch.manual_seed(seed)
    return PPOTrainer(cfg, run_id=run_id, device=_dev(), env=env, tensorboard=False)


def _hand_table():
    """A non-identity table near (not at) the data's location and spread; clip 1.5 cuts part of the rows."""
    mean = (OFFSET + np.float32(0.3) * SCALE).astype(np.float32)
    rstd = (np.float32(1.7) / SCALE).astype(np.float32)
    return mean, rstd


def _set_table(tr, mean, rstd):
    ptrs = (tr.model.obs_norm_mean.data_ptr(), tr.model.obs_norm_rstd.data_ptr())
    with torch.no_grad():
        tr.model.obs_norm_mean.copy_(torch.from_numpy(mean))
        tr.model.obs_norm_rstd.copy_(torch.from_numpy(rstd))
    assert ptrs == (tr.model.obs_norm_mean.data_ptr(), tr.model.obs_norm_rstd.data_ptr())


def _round(tr, uniforms, perm):
    tr._sample_training_data(uniforms=uniforms)
    tr.buffer.prepare_batch_dict()
    tr._train_epochs(3e-4, 0.1, 1e-3, perms=[perm])
    torch.cuda.synchronize()
    buf = tr.buffer
    return dict(values=buf.values.cpu().numpy(), log_probs=buf.log_probs.cpu().numpy(), actions=buf.actions.cpu().numpy(),
                advantages=buf.advantages.cpu().numpy(), obs=buf.obs.cpu().numpy(),
                params={n: p.detach().cpu().numpy().copy() for n, p in tr.model.named_parameters()})


# ------------------------------------------------------------------ 4. table equivalence through the trainer
@pytest.mark.parametrize("graph", (True, False), ids=["graph", "eager"])
def test_table_equivalence_through_the_trainer(graph):
    clip = 1.5
    ends = lambda w: 5 + 2 * w
    over = dict(hip_graph_rollout=graph, hip_graph_train=graph)
    env_a, env_b = OffsetVecEnv(W_T, ends_at=ends), OffsetVecEnv(W_T, ends_at=ends, table=_hand_table() + (clip,))
    a = _trainer(_config(normalize_observations={"clip": clip}, **over), env_a)
    b = _trainer(_config(**over), env_b)
    try:
        assert a.obs_norm is not None and b.obs_norm is None and a.return_norm is None
        assert not a.obs_norm["stats"].any() and (a.obs_norm["rstd"] == 1).all(), "rollout 0 would run on the identity table"
        for (na, pa), (nb_, pb) in zip(a.model.named_parameters(), b.model.named_parameters()):
            assert na == nb_ and torch.equal(pa, pb), "the two trainers start from the same weights"
        _set_table(a, *_hand_table())
        table_ptrs = [t.data_ptr() for t in (a.model.obs_norm_stats, a.model.obs_norm_mean, a.model.obs_norm_rstd)]
        rng = np.random.default_rng(4)
        seen = []
        for rnd in range(2):           # round 1 runs on the refreshed table, through the graphs captured in round 0
            uniforms = rng.random((W_T, S_T)).astype(np.float32)
            perm = rng.permutation(W_T * S_T)
            ra, rb = _round(a, uniforms, perm), _round(b, uniforms, perm)
            for key in ("values", "log_probs", "actions", "advantages"):
                assert _same_bits(ra[key].astype(np.float32), rb[key].astype(np.float32)), (rnd, key)
            for name in ra["params"]:
                assert _same_bits(ra["params"][name], rb["params"][name]), (rnd, name)
            # A keeps the raw rows, B's are the normalised ones
            assert ra["obs"].shape == (W_T, S_T, F_OBS) and ra["obs"][..., 0].min() > 900 and np.abs(rb["obs"]).max() <= clip
            mean_used = _hand_table()[0] if rnd == 0 else seen[-1][1]
            rstd_used = _hand_table()[1] if rnd == 0 else seen[-1][2]
            assert _same_bits(nr.obs_normalize_f32(ra["obs"], mean_used, rstd_used, clip), rb["obs"])
            # after the update: the triple is the merge of every raw row seen so far, the table is refreshed in place
            every = np.concatenate([s[0] for s in seen] + [ra["obs"].reshape(-1, F_OBS)])
            stats, mean, rstd = (t.cpu().numpy() for t in (a.model.obs_norm_stats, a.model.obs_norm_mean, a.model.obs_norm_rstd))
            _check_triple(stats, mean, rstd, every, f"trainer {'graph' if graph else 'eager'} round {rnd}")
            assert table_ptrs == [t.data_ptr() for t in (a.model.obs_norm_stats, a.model.obs_norm_mean, a.model.obs_norm_rstd)]
            seen.append((ra["obs"].reshape(-1, F_OBS), mean, rstd))
            # B's wrapper follows A's refreshed table, from the observation the next rollout starts with on
            env_b.table = (mean, rstd, clip)
            for w in range(W_T):
                b.obs[w] = env_b.observation(w, int(env_b.s[w]))
        assert (a._step_graph is not None) == graph
        if graph:
            assert a._train_graph is not None, "round 1 replays the captured optimisation step"
        # the evaluator of A reads the refreshed table (its model's buffers, filled before the run)
        out = a.evaluate(episodes_per_worker=1, n_workers=4, worker_steps=8)
        assert len(out["episodes"]) == 4
        em = a._evaluator.rollout.model
        for name in ("obs_norm_stats", "obs_norm_mean", "obs_norm_rstd"):
            assert getattr(em, name).data_ptr() != getattr(a.model, name).data_ptr()
            assert torch.equal(getattr(em, name), getattr(a.model, name)), name
        assert _same_bits(em.obs_norm_rstd.cpu().numpy(), seen[-1][2]) and not (em.obs_norm_rstd == 1).any()
    finally:
        _release(a, b)


def test_trainer_refuses_a_data_parallel_run_before_it_builds_anything():
    from types import SimpleNamespace
    from trainer import PPOTrainer
    for key in ("normalize_observations", "normalize_rewards"):
        with pytest.raises(ValueError, match="data-parallel"):
            PPOTrainer(_config(**{key: True}), device=_dev(), env=object(), dp=SimpleNamespace(world=2, rank=0), tensorboard=False)
    with pytest.raises(ValueError, match="unknown keys"):
        PPOTrainer(_config(normalize_rewards={"clipp": 1.0}), device=_dev(), env=object(), tensorboard=False)


# ------------------------------------------------------------------ 5. rewards through the trainer
@pytest.mark.parametrize("truncation", (False, True), ids=["plain", "truncated"])
def test_rewards_through_the_trainer(truncation):
    from etm import ops
    clip, eps = 0.75, 1e-8
    over = dict(normalize_rewards={"clip": clip, "epsilon": eps})
    if truncation:
        over["bootstrap_truncated"] = True
    env = OffsetVecEnv(W_T, ends_at=lambda w: 6 + w if w != 1 else None, cut_at=lambda w: 9 if (truncation and w == 1) else None)
    tr = _trainer(_config(**over), env)
    try:
        assert tr.obs_norm is None and not [n for n, _ in tr.model.named_buffers() if "obs_norm" in n]
        rn = tr.return_norm
        assert rn["clip"] == clip and not rn["stats"].any() and not rn["carry"].any()
        rng = np.random.default_rng(9)
        carry, before = np.zeros(W_T), np.zeros(0)
        for rollout in range(2):
            tr._sample_training_data(uniforms=rng.random((W_T, S_T)).astype(np.float32))
            torch.cuda.synchronize()
            buf = tr.buffer
            assert buf.rewards.dtype == np.float32 and buf.rewards.shape == (W_T, S_T)
            assert np.abs(buf.rewards).max() < 0.2 and _same_bits(tr.buffer.rewards_dev.cpu().numpy(), buf.rewards), "buffer.rewards is raw"
            if truncation:
                assert len(tr.last_truncations) == int(buf.truncated.sum()) >= 1 and not buf.truncated[[0, 2, 3]].any()
            ref = nr.return_rule_exact(buf.rewards, buf.dones, carry, before, 0.99, eps, clip)
            scaled = rn["scaled"].cpu().numpy()
            u_scale, u_scaled = int(nr.ulps32(rn["scale"].cpu().numpy(), ref["scale"]).max()), int(nr.ulps32(scaled, ref["scaled"]).max())
            _figure(f"trainer rewards rollout {rollout} truncation={truncation}: scale {float(rn['scale'].item()):.6g}, ulps scale {u_scale} scaled {u_scaled}")
            assert u_scale <= 1 and u_scaled <= 1
            assert (np.abs(scaled) == np.float32(clip)).any() and not _same_bits(scaled, buf.rewards)
            assert _same_bits(rn["carry"].cpu().numpy(), ref["carry"])
            _check_return_triple(rn["stats"].cpu().numpy(), ref, f"trainer rollout {rollout}")
            kw = dict(truncated=buf.truncated_dev, boot=buf.bootstrap_values) if truncation else {}
            adv = ops.gae(rn["scaled"], buf.dones_dev, buf.values, tr._lv.out, 0.99, 0.95, **kw)
            assert _same_bits(adv.cpu().numpy(), buf.advantages.cpu().numpy()), "GAE read the scaled rewards"
            adv_raw = ops.gae(buf.rewards_dev, buf.dones_dev, buf.values, tr._lv.out, 0.99, 0.95, **kw)
            assert not _same_bits(adv_raw.cpu().numpy(), buf.advantages.cpu().numpy()), "the key matters"
            carry, before = ref["carry"], ref["every"]
    finally:
        _release(tr)


# ------------------------------------------------------------------ 6. checkpoint round trip
def test_checkpoint_round_trip_through_the_evaluator(tmp_path, monkeypatch):
    """Save the normalising trainer, load (state_dict, config) the way evaluate.py does, and play the same greedy episodes as the
    trainer's own evaluator: same observations, same actions."""
    from evaluation import Evaluator
    monkeypatch.chdir(tmp_path)
    cfg = _config(normalize_observations={"clip": 1.5}, normalize_rewards=True)
    a = _trainer(cfg, None, run_id="normckpt")
    ev = None
    try:
        rng = np.random.default_rng(1)
        for _ in range(2):
            _round(a, rng.random((W_T, S_T)).astype(np.float32), rng.permutation(W_T * S_T))
        assert a.obs_norm["stats"][0, 0].item() == 2 * W_T * S_T and not (a.obs_norm["rstd"] == 1).any()
        a._save_model()
        own = a.evaluate(episodes_per_worker=2, n_workers=4, worker_steps=8)
        ro = a._evaluator.rollout
        own_obs, own_act = ro.buffer.obs.cpu().numpy().copy(), ro.buffer.actions.cpu().numpy().copy()
        with open(tmp_path / "models" / "normckpt.nn", "rb") as f:
            state_dict, config = pickle.load(f)
        assert {"obs_norm_stats", "obs_norm_mean", "obs_norm_rstd"} <= set(state_dict) and state_dict["obs_norm_stats"].dtype == torch.float64
        assert not [k for k in state_dict if "ret_" in k or "return" in k], "the return triple is trainer state"
        ev = Evaluator(config, _dev(), run_id="evaluate")
        ev.load_state_dict(state_dict)
        got = ev.run(episodes_per_worker=2, n_workers=4, worker_steps=8)
        for name in ("obs_norm_stats", "obs_norm_mean", "obs_norm_rstd"):
            assert torch.equal(getattr(ev.rollout.model, name), getattr(a.model, name)), name
        assert ev.rollout.return_norm is None, "the evaluator scales no rewards"
        assert got["episodes"] == own["episodes"]
        assert _same_bits(ev.rollout.buffer.obs.cpu().numpy(), own_obs) and np.array_equal(ev.rollout.buffer.actions.cpu().numpy(), own_act)
    finally:
        if ev is not None:
            ev.close()
        _release(a)
