"""Box (continuous) action spaces on the host side: the kind helper, the environment front-ends, the early refusals and the kernels'
Box shape predicates.

A space with ``low``, ``high`` and a 1-D ``shape`` (and neither ``n`` nor ``nvec``) is a Box of A dimensions; the synthetic environment
takes ``continuous_actions: A`` with ``action_low`` / ``action_high``.  Its streams do not depend on the action space.  No GPU is
needed here (the predicates are host functions of the kernel library)."""
from types import SimpleNamespace

import numpy as np
import pytest


def test_action_space_kind():
    from environments import action_space_kind
    k = action_space_kind(SimpleNamespace(n=4))
    assert k.kind == "discrete" and k.shape == (4,) and not k.is_box and k.low is None
    k = action_space_kind(SimpleNamespace(nvec=np.array([3, 2]), shape=(2,)))
    assert k.kind == "multidiscrete" and k.shape == (3, 2) and not k.is_box
    k = action_space_kind(SimpleNamespace(low=-2.0, high=np.array([1.0, 2.0, 3.0]), shape=(3,)))
    assert k.kind == "box" and k.is_box and k.shape == (3,)
    assert k.low.dtype == np.float32 and k.low.tolist() == [-2.0] * 3 and k.high.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="1-D"):
        action_space_kind(SimpleNamespace(low=-1.0, high=1.0, shape=(2, 3)))
    with pytest.raises(ValueError):
        action_space_kind(SimpleNamespace(low=1.0, high=-1.0, shape=(2,)))


def test_action_space_shape_is_unchanged():
    from environments import action_space_shape
    assert action_space_shape(SimpleNamespace(n=4)) == (4,)
    assert action_space_shape(SimpleNamespace(nvec=np.array([3, 2]), shape=(2,))) == (3, 2)
    with pytest.raises(AttributeError):          # (the Discrete / MultiDiscrete rule: a Box goes through action_space_kind)
        action_space_shape(SimpleNamespace(low=-1.0, high=1.0, shape=(3,)))


def _drain(env, steps, actions):
    out = []
    obs = env.reset().copy()
    for t in range(steps):
        o, r, d, inf = env.step(actions(t))
        out.append((o.copy(), r.copy(), d.copy(), list(inf)))
    return obs, out


def test_synthetic_box_single_and_vector_forms():
    from environments.synthetic import SyntheticEnv, SyntheticVecEnv
    from environments.vec_env import CompositeVecEnv, SerialVecEnv
    kw = dict(obs_shape=(2, 3), max_episode_steps=7, seed=5, p_done=0.2, p_reward=0.4, pool=5)
    e = SyntheticEnv(continuous_actions=3, action_low=[-1, -2, 0], action_high=2.0, num_actions=7, **kw)
    sp = e.action_space
    assert sp.shape == (3,) and sp.low.tolist() == [-1, -2, 0] and sp.high.tolist() == [2, 2, 2]
    assert not hasattr(sp, "n") and not hasattr(sp, "nvec")
    e.reset()
    obs, rew, done, info = e.step(np.array([0.5, -1.5, 0.25], dtype=np.float32))
    assert obs.shape == (2, 3)
    W = 4
    v = SyntheticVecEnv(W, continuous_actions=3, **kw)
    assert v.action_space_shape == (3,) and v.num_actions == 3 and v.action_kind.is_box
    assert v.action_kind.low.tolist() == [-1.0] * 3 and v.action_kind.high.tolist() == [1.0] * 3
    s = SerialVecEnv([SyntheticEnv(continuous_actions=3, worker_id=w, **kw) for w in range(W)])
    assert s.action_space_shape == (3,) and s.action_kind.is_box
    c = CompositeVecEnv([SerialVecEnv([SyntheticEnv(continuous_actions=3, worker_id=w, **kw) for w in range(2)]),
                         SerialVecEnv([SyntheticEnv(continuous_actions=3, worker_id=w, **kw) for w in range(2, 4)])])
    assert c.action_space_shape == (3,) and c.action_kind.is_box
    acts = lambda t: np.full((W, 3), 0.1 * t, dtype=np.float32)
    o_v, r_v = _drain(v, 30, acts)
    o_s, r_s = _drain(s, 30, acts)
    o_c, r_c = _drain(c, 30, acts)
    assert np.array_equal(o_v, o_s) and np.array_equal(o_v, o_c)
    for (a, b, cc, d), (a2, b2, c2, d2), (a3, b3, c3, d3) in zip(r_v, r_s, r_c):
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(cc, c2) and d == d2
        assert np.array_equal(a, a3) and np.array_equal(b, b3) and np.array_equal(cc, c3)


@pytest.mark.parametrize("pool", [5, 0])
def test_synthetic_box_streams_equal_three_discrete_actions(pool):
    """Observation, reward and done streams at continuous_actions 3 are bit-identical to num_actions 3 at the same seed."""
    from environments.synthetic import SyntheticEnv, SyntheticVecEnv
    kw = dict(obs_shape=(2, 5), max_episode_steps=6, seed=11, p_done=0.15, p_reward=0.3, pool=pool)
    W, S = 5, 40
    box = SyntheticVecEnv(W, continuous_actions=3, **kw)
    dis = SyntheticVecEnv(W, num_actions=3, **kw)
    o1, r1 = _drain(box, S, lambda t: np.random.default_rng(t).uniform(-1, 1, (W, 3)).astype(np.float32))
    o2, r2 = _drain(dis, S, lambda t: np.zeros(W, dtype=np.int64))
    assert np.array_equal(o1, o2)
    for (a, b, c, d), (a2, b2, c2, d2) in zip(r1, r2):
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(c, c2) and d == d2
    e1 = SyntheticEnv(continuous_actions=3, worker_id=2, **kw)
    e2 = SyntheticEnv(num_actions=3, worker_id=2, **kw)
    assert np.array_equal(e1.reset(), e2.reset())
    for t in range(S):
        x1, x2 = e1.step(np.zeros(3, dtype=np.float32)), e2.step(0)
        assert np.array_equal(x1[0], x2[0]) and x1[1:] == x2[1:]


def test_box_clip_semantics():
    """The environment receives clip(x, low, high) per dimension (what etm_sample_gaussian hands over); the buffer keeps x."""
    from environments import action_space_kind
    k = action_space_kind(SimpleNamespace(low=np.array([-1.0, 0.0, -np.inf]), high=np.array([1.0, 0.5, np.inf]), shape=(3,)))
    x = np.array([[3.0, -2.0, 1e30], [-0.25, 0.25, -7.0]], dtype=np.float32)
    c = np.clip(x, k.low, k.high)
    assert c.tolist() == [[1.0, 0.0, np.float32(1e30)], [-0.25, 0.25, -7.0]]


def test_worker_processes_refuse_box_with_a_useful_message():
    from environments.shm_env import _probe_env
    cfg = dict(type="Synthetic", obs_shape=[3], num_actions=3, continuous_actions=2, max_episode_steps=9)
    with pytest.raises(NotImplementedError, match="worker_processes: false"):
        _probe_env(cfg)
    cfg.pop("continuous_actions")
    assert _probe_env(cfg)[1] == 3


def test_box_policy_refused_early():
    from trainer import check_box_policy
    cfg = dict(hidden_layer_size=384, environment=dict(type="Synthetic", continuous_actions=3))
    assert check_box_policy(cfg) == 3
    assert check_box_policy(dict(cfg, environment=dict(type="Synthetic", num_actions=3))) is None
    assert check_box_policy(dict(cfg, environment=dict(type="Synthetic", continuous_actions=8))) == 8
    with pytest.raises(ValueError, match="1 to 8"):
        check_box_policy(dict(cfg, environment=dict(type="Synthetic", continuous_actions=9)))
    with pytest.raises(ValueError, match="1 to 8"):
        check_box_policy(dict(cfg, environment=dict(type="Synthetic", continuous_actions=0)))
    with pytest.raises(ValueError, match="hidden_layer_size"):
        check_box_policy(dict(cfg, hidden_layer_size=96))
    with pytest.raises(ValueError, match="hidden_layer_size"):
        check_box_policy(dict(cfg, hidden_layer_size=576))
    from environments import action_space_kind
    with pytest.raises(ValueError):
        action_space_kind(SimpleNamespace(low=np.zeros((2, 2)), high=np.ones((2, 2)), shape=(2, 2)))


def test_box_shape_predicates():
    """The Box predicates are the Discrete ones at A, limited to A <= 8."""
    from etm import lib as etm_lib
    from etm import ops
    lib = etm_lib.load()
    for A in (1, 3, 8):
        assert ops.rollout_trxl_supported(384, 4, 64, 384, A, 3, gaussian=True)
        assert lib.etm_heads_loss_supported_gaussian(37, 384, A) and lib.etm_heads_loss_supported_gaussian(2048, 512, A)
    assert not ops.rollout_trxl_supported(384, 4, 64, 384, 9, 3, gaussian=True)
    assert ops.rollout_trxl_supported(384, 4, 64, 384, 9, 3)                     # (Discrete 9: fine)
    assert not ops.rollout_trxl_supported(384, 4, 64, 384, 0, 3, gaussian=True)
    assert not ops.rollout_trxl_supported(384, 4, 129, 384, 3, 3, gaussian=True)
    rfg = dict(D=384, H=4, nb=4, gtrxl=1)
    assert ops.rollout_trxl_group_ok(rfg, 8, 128, 384, 8, gaussian=True) and ops.rollout_trxl_group_ok(rfg, 8, 128, 384, 1, gaussian=True)
    assert not ops.rollout_trxl_group_ok(rfg, 8, 128, 384, 9, gaussian=True) and ops.rollout_trxl_group_ok(rfg, 8, 128, 384, 9)
    assert not ops.rollout_trxl_group_ok(rfg, 9, 128, 384, 3, gaussian=True)
    assert not ops.rollout_trxl_group_ok(dict(rfg, gtrxl=0), 8, 128, 384, 3, gaussian=True)
    assert not lib.etm_heads_loss_supported_gaussian(37, 384, 9) and not lib.etm_heads_loss_supported_gaussian(37, 96, 3)
    assert not lib.etm_heads_loss_supported_gaussian(0, 384, 3) and not lib.etm_heads_loss_supported_gaussian(37, 576, 3)
    assert lib.etm_heads_loss_gaussian_row_floats(384, 3) == lib.etm_heads_loss_row_floats(384, 3) + 3
    assert lib.etm_heads_loss_gaussian_workspace_bytes(16, 384, 3) == 2 * 4 * (lib.etm_heads_loss_row_floats(384, 3) + 3)


def test_continuous_config_is_config_3_with_a_gaussian_head():
    import os
    from yaml_parser import YamlParser
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "episodic-transformer-memory-ppo_amd", "configs")
    bx = YamlParser(os.path.join(here, "synthetic_continuous.yaml")).get_config()
    c3 = YamlParser(os.path.join(here, "synthetic_minigrid.yaml")).get_config()
    assert bx["environment"]["continuous_actions"] == 3 and "num_actions" not in bx["environment"]
    del bx["environment"]["continuous_actions"]
    bx["environment"]["num_actions"] = 3
    assert bx == c3
