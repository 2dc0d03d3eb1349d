"""MultiDiscrete action spaces on the host side: the branch rule, the environment front-ends and the kernels' shape predicates.

An action space with ``nvec`` has one action branch per entry; any other space is Discrete, ``(n,)``.  The synthetic environment takes
``num_actions: [3, 2]`` for MultiDiscrete; its streams do not depend on the action space.  No GPU is needed here (the predicates
are host functions of the kernel library)."""
from types import SimpleNamespace

import numpy as np
import pytest


def test_branch_rule():
    from environments import action_space_shape
    assert action_space_shape(SimpleNamespace(n=4)) == (4,)
    assert action_space_shape(SimpleNamespace(nvec=np.array([3, 2]), shape=(2,))) == (3, 2)
    assert action_space_shape(SimpleNamespace(nvec=[5])) == (5,)
    assert all(type(a) is int for a in action_space_shape(SimpleNamespace(nvec=np.array([3, 2], dtype=np.int64))))
    with pytest.raises(ValueError):
        action_space_shape(SimpleNamespace(nvec=[3, 0]))


def _drain(env, W, steps, actions):
    out = []
    obs = env.reset().copy()
    for t in range(steps):
        o, r, d, inf = env.step(actions(t))
        out.append((o.copy(), r.copy(), d.copy(), list(inf)))
    return obs, out


def test_synthetic_multidiscrete_single_and_vector_forms():
    from environments.synthetic import SyntheticEnv, SyntheticVecEnv
    from environments.vec_env import SerialVecEnv
    kw = dict(obs_shape=(2, 3), max_episode_steps=7, seed=5, p_done=0.2, p_reward=0.4, pool=5)
    e = SyntheticEnv(num_actions=[3, 2], **kw)
    assert list(e.action_space.nvec) == [3, 2] and e.action_space.shape == (2,) and not hasattr(e.action_space, "n")
    assert e.observation_space.shape == (2, 3)
    e.reset()
    obs, rew, done, info = e.step(np.array([2, 1]))
    assert obs.shape == (2, 3)
    W = 4
    v = SyntheticVecEnv(W, num_actions=[3, 2], **kw)
    assert v.action_space_shape == (3, 2) and v.num_actions == 5 and list(v.action_space.nvec) == [3, 2]
    s = SerialVecEnv([SyntheticEnv(num_actions=[3, 2], worker_id=w, **kw) for w in range(W)])
    assert s.action_space_shape == (3, 2) and s.num_actions == 5
    acts = lambda t: np.stack([np.arange(W) % 3, (np.arange(W) + t) % 2], axis=1)          # [W, 2]
    o_v, r_v = _drain(v, W, 30, acts)
    o_s, r_s = _drain(s, W, 30, acts)
    assert np.array_equal(o_v, o_s)
    for (a, b, c, d), (a2, b2, c2, d2) in zip(r_v, r_s):
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(c, c2) and d == d2


@pytest.mark.parametrize("pool", [5, 0])
def test_synthetic_streams_do_not_depend_on_the_action_space(pool):
    """Observation, reward and done streams at num_actions [3, 2] are bit-identical to num_actions 3 at the same seed."""
    from environments.synthetic import SyntheticEnv, SyntheticVecEnv
    kw = dict(obs_shape=(2, 5), max_episode_steps=6, seed=11, p_done=0.15, p_reward=0.3, pool=pool)
    W, S = 5, 40
    md = SyntheticVecEnv(W, num_actions=[3, 2], **kw)
    dc = SyntheticVecEnv(W, num_actions=3, **kw)
    o1, r1 = _drain(md, W, S, lambda t: np.ones((W, 2), dtype=np.int64))
    o2, r2 = _drain(dc, W, S, lambda t: np.zeros(W, dtype=np.int64))
    assert np.array_equal(o1, o2)
    assert any(x[2].any() for x in r1), "episodes must end inside the window"
    for (a, b, c, d), (a2, b2, c2, d2) in zip(r1, r2):
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(c, c2) and d == d2
    e1, e2 = SyntheticEnv(num_actions=[3, 2], **kw), SyntheticEnv(num_actions=3, **kw)
    assert np.array_equal(e1.reset(), e2.reset())
    for t in range(S):
        x1, x2 = e1.step([t % 3, t % 2]), e2.step(t % 3)
        assert np.array_equal(x1[0], x2[0]) and x1[1:] == x2[1:]
        if x1[2]:
            assert np.array_equal(e1.reset(), e2.reset())


class _StubMultiDiscreteEnv:
    """Upstream env API with a MultiDiscrete space; reward = the action vector's value as a mixed-radix number."""

    def __init__(self, nvec, worker_id):
        self.nvec = list(nvec)
        self.w = worker_id
        self.t = 0
        self.seen = []

    observation_space = SimpleNamespace(shape=(3,))
    max_episode_steps = 9

    @property
    def action_space(self):
        return SimpleNamespace(nvec=np.array(self.nvec), shape=(len(self.nvec),))

    def reset(self):
        self.t = 0
        return np.full(3, self.w, dtype=np.float32)

    def step(self, action):
        action = np.asarray(action)
        assert action.shape == (len(self.nvec),)
        assert all(0 <= int(a) < n for a, n in zip(action, self.nvec))
        self.seen.append(action.tolist())
        self.t += 1
        r = float(sum(int(a) * 10 ** i for i, a in enumerate(action)))
        done = self.t >= 4
        return np.full(3, self.w + self.t, dtype=np.float32), r, done, ({"reward": r, "length": self.t} if done else None)

    def close(self):
        pass


def test_serial_and_composite_vec_env_take_one_action_row_per_environment():
    from environments.vec_env import CompositeVecEnv, SerialVecEnv
    W = 4
    envs = [_StubMultiDiscreteEnv([3, 2, 4], w) for w in range(W)]
    s = SerialVecEnv(envs)
    assert s.action_space_shape == (3, 2, 4) and s.num_actions == 9
    s.reset()
    acts = np.array([[0, 1, 3], [2, 0, 1], [1, 1, 0], [2, 1, 2]])
    _, r, d, _ = s.step(acts)
    assert np.array_equal(r, [100 * a[2] + 10 * a[1] + a[0] for a in acts])
    assert [e.seen[-1] for e in envs] == acts.tolist()
    c = CompositeVecEnv([SerialVecEnv(envs[:2]), SerialVecEnv(envs[2:])])
    assert c.action_space_shape == (3, 2, 4) and c.num_actions == 9 and c.num_envs == W
    _, r2, _, _ = c.step(acts[::-1])
    assert np.array_equal(r2, [100 * a[2] + 10 * a[1] + a[0] for a in acts[::-1]])
    assert [e.seen[-1] for e in envs] == acts[::-1].tolist()


def test_make_vec_env_carries_the_branches_through_every_front_end():
    from environments.vec_env import make_vec_env
    cfg = dict(type="Synthetic", obs_shape=[2, 5], num_actions=[3, 3], max_episode_steps=9, seed=3, p_done=0.1, pool=4)
    one = make_vec_env(cfg, 4)
    two = make_vec_env(cfg, 4, groups=2)
    assert one.action_space_shape == two.action_space_shape == (3, 3)
    assert len(two.parts) == 2 and all(p.action_space_shape == (3, 3) for p in two.parts)
    o1, r1 = _drain(one, 4, 12, lambda t: np.zeros((4, 2), dtype=np.int64))
    o2, r2 = _drain(two, 4, 12, lambda t: np.zeros((4, 2), dtype=np.int64))
    assert np.array_equal(o1, o2) and all(np.array_equal(a[1], b[1]) for a, b in zip(r1, r2))
    d = make_vec_env(dict(cfg, num_actions=3), 4)
    assert d.action_space_shape == (3,) and d.num_actions == 3


def test_worker_processes_refuse_several_branches_with_a_useful_message():
    from environments.shm_env import _probe_env
    cfg = dict(type="Synthetic", obs_shape=[3], num_actions=[3, 2], max_episode_steps=9)
    with pytest.raises(NotImplementedError, match="worker_processes: false"):
        _probe_env(cfg)
    assert _probe_env(dict(cfg, num_actions=[4]))[1] == 4          # one nvec entry is one branch: fine
    assert _probe_env(dict(cfg, num_actions=3))[1] == 3


def test_branched_shape_predicates():
    """The branched predicates are the single-branch ones at A = sum of the branch sizes (step kernels), plus the branch count
    limits; the single-branch entries are unchanged."""
    import ctypes
    from etm import lib as etm_lib
    from etm import ops
    lib = etm_lib.load()
    tab = lambda s: ((ctypes.c_int32 * len(s))(*s), len(s))
    # per-worker step kernel: sum + 1 <= 64
    assert ops.rollout_trxl_supported(384, 4, 64, 384, (3, 3), 3)
    assert ops.rollout_trxl_supported(384, 4, 64, 384, (2, 4, 3), 3)
    assert ops.rollout_trxl_supported(384, 4, 64, 384, (40, 23), 3) and not ops.rollout_trxl_supported(384, 4, 64, 384, (40, 24), 3)
    assert ops.rollout_trxl_supported(384, 4, 64, 384, 63, 3) and not ops.rollout_trxl_supported(384, 4, 64, 384, 64, 3)
    assert ops.rollout_trxl_supported(384, 4, 64, 384, (63,), 3)                     # one branch = Discrete
    assert not lib.etm_rollout_trxl_supported_branched(384, 4, 64, 384, *tab([1] * 17), 3)        # > 16 branches
    assert lib.etm_rollout_trxl_supported_branched(384, 4, 64, 384, *tab([1] * 16), 3)
    assert not lib.etm_rollout_trxl_supported_branched(384, 4, 64, 384, *tab([3, 0]), 3)
    # group kernel (config 5 shape): the exchange piece holds 8 (sum + 1) + 1 <= 128 floats, i.e. sum <= 14
    rfg = dict(D=384, H=4, nb=4, gtrxl=1)
    assert ops.rollout_trxl_group_ok(rfg, 8, 128, 384, (3, 3)) and ops.rollout_trxl_group_ok(rfg, 8, 128, 384, (8, 6))
    assert not ops.rollout_trxl_group_ok(rfg, 8, 128, 384, (8, 7)) and not ops.rollout_trxl_group_ok(rfg, 8, 128, 384, 15)
    assert ops.rollout_trxl_group_ok(rfg, 8, 128, 384, 14) and ops.rollout_trxl_group_ok(rfg, 8, 128, 384, (14,))
    # fused heads + loss: sum <= 8 (and at most 8 branches), hid % 64 == 0, hid <= 512
    assert lib.etm_heads_loss_supported_branched(37, 384, *tab([3, 3]))
    assert lib.etm_heads_loss_supported_branched(2048, 512, *tab([2, 2, 2, 2]))
    assert lib.etm_heads_loss_supported_branched(1, 64, *tab([1] * 8))
    assert not lib.etm_heads_loss_supported_branched(37, 384, *tab([5, 4]))
    assert not lib.etm_heads_loss_supported_branched(37, 96, *tab([3, 3]))
    assert lib.etm_heads_loss_supported(37, 384, 8) and not lib.etm_heads_loss_supported(37, 384, 9)
    assert ops._branch_sizes(None) is None and ops._branch_sizes(3) is None and ops._branch_sizes((3,)) is None
    assert ops._branch_sizes([3, 2]) == (3, 2)


def test_multidiscrete_config_is_config_3_with_two_branches():
    import os
    from yaml_parser import YamlParser
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "episodic-transformer-memory-ppo_amd", "configs")
    md = YamlParser(os.path.join(here, "synthetic_multidiscrete.yaml")).get_config()
    c3 = YamlParser(os.path.join(here, "synthetic_minigrid.yaml")).get_config()
    assert list(md["environment"]["num_actions"]) == [3, 3]
    md["environment"]["num_actions"] = 3
    assert md == c3
