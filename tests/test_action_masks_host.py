"""Invalid-action masks, host side (no GPU): the packing, every refusal of ``check_action_mask_config``, the ``action_masks`` method of
the vectorised front-ends (the new episode's mask after an auto-reset included), the synthetic mask stream, and the ctypes mirror of
the masked entries."""
import os
import re

import numpy as np
import pytest


# ------------------------------------------------------------------ packing
def test_pack_action_masks_bits_31_32_62():
    from environments import MAX_MASKED_ACTIONS, empty_mask_branches, pack_action_masks, valid_action_share
    assert MAX_MASKED_ACTIONS == 63
    m = np.zeros((3, 63), dtype=bool)
    m[0, [0, 31]] = True
    m[1, [32, 62]] = True
    m[2, :] = True
    w = pack_action_masks(m)
    assert w.dtype == np.uint64 and w.shape == (3,)
    assert int(w[0]) == (1 << 0) | (1 << 31) and int(w[1]) == (1 << 32) | (1 << 62) and int(w[2]) == (1 << 63) - 1
    # into an int64 block (the trainer's pinned words): the same bits, no sign trouble below bit 63
    out = np.zeros(3, dtype=np.int64)
    assert pack_action_masks(m, out=out) is out
    assert [int(x) for x in out] == [int(x) for x in w] and (out >= 0).all()
    # every single bit on its own, and a 1-D row is one worker
    for j in range(63):
        row = np.zeros(63, dtype=bool)
        row[j] = True
        assert int(pack_action_masks(row)[0]) == 1 << j
    for bad in (np.zeros((2, 64), dtype=bool), np.zeros((2, 0), dtype=bool), np.zeros((2, 3, 4), dtype=bool)):
        with pytest.raises(ValueError):
            pack_action_masks(bad)
    # a branch that straddles bit 32: (30, 5) owns bits [0, 30) and [30, 35)
    e = empty_mask_branches(np.array([1 << 29, 1 << 30, (1 << 34) | 1, 1 << 35], dtype=np.int64), (30, 5))
    assert e.tolist() == [[False, True], [True, False], [False, False], [True, True]]      # (bit 35 is past the last column: ignored)
    assert valid_action_share(np.array([[0b0111, 0b0001]], dtype=np.int64), 4) == 0.5
    assert valid_action_share(np.array([(1 << 63) - 1], dtype=np.uint64), 63) == 1.0


# ------------------------------------------------------------------ refusals
def _cfg(**over):
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[4], num_actions=[2, 4, 3], action_mask_p=0.3), n_workers=4, hidden_layer_size=64,
               action_masks=True)
    cfg.update(over)
    return cfg


class _Front:
    num_envs = 4


class _MaskedFront(_Front):
    def action_masks(self, out=None):
        return np.ones(4, dtype=np.uint64)


def test_check_action_mask_config_refusals():
    from trainer import check_action_mask_config as check
    assert check(dict(environment={})) is False and check(_cfg(action_masks=False)) is False      # absent / false: nothing to do
    assert check(_cfg()) is True
    assert check(_cfg(), _MaskedFront(), (2, 4, 3)) is True
    with pytest.raises(ValueError, match="Box"):
        check(_cfg(environment=dict(type="Synthetic", continuous_actions=2)))
    with pytest.raises(ValueError, match="Box"):
        check(_cfg(), _MaskedFront(), (2,), box=True)
    with pytest.raises(ValueError, match="at most 63"):
        check(_cfg(environment=dict(type="Synthetic", num_actions=[60, 4])))
    with pytest.raises(ValueError, match="at most 63"):
        check(_cfg(), _MaskedFront(), (64,))
    assert check(_cfg(environment=dict(type="Synthetic", num_actions=[60, 3]))) is True          # 63 fits
    with pytest.raises(ValueError, match="worker_processes"):
        check(_cfg(worker_processes=True))
    assert check(_cfg(worker_processes=True), _MaskedFront()) is True                             # a supplied environment is stepped in process
    with pytest.raises(ValueError, match="no action_masks"):
        check(_cfg(), _Front(), (2, 4, 3))
    # every message says what to do instead
    for kw in (dict(environment=dict(type="Synthetic", continuous_actions=2)), dict(environment=dict(type="Synthetic", num_actions=70)),
               dict(worker_processes=True)):
        with pytest.raises(ValueError, match="remove the key|set worker_processes: false"):
            check(_cfg(**kw))
    # data-parallel runs are not refused: the function takes no world size, and the trainer calls it the same way on every rank
    import inspect
    assert "world" not in inspect.signature(check).parameters


def test_synthetic_front_end_without_the_key_has_no_action_masks():
    from environments.vec_env import make_vec_env
    env = make_vec_env(dict(type="Synthetic", obs_shape=[4], num_actions=[2, 3], pool=4), 4)
    assert not hasattr(env, "action_masks")
    from trainer import check_action_mask_config as check
    with pytest.raises(ValueError, match="action_mask_p"):
        check(dict(action_masks=True, environment=dict(type="Synthetic", num_actions=[2, 3])), env, (2, 3))
    with pytest.raises(ValueError):
        make_vec_env(dict(type="Synthetic", obs_shape=[4], continuous_actions=2, action_mask_p=0.3, pool=4), 4)


# ------------------------------------------------------------------ front-ends over single environments
class _GridEnv:
    """Upstream env API with ``action_masks()``: MultiDiscrete([2, 3]); the allowed set depends on (episode, step), episodes last
    ``length`` steps.  Raises on an action its own mask forbids."""

    def __init__(self, worker_id=0, length=3):
        from types import SimpleNamespace
        self.worker_id, self.length = int(worker_id), int(length)
        self.observation_space = SimpleNamespace(shape=(2,), dtype=np.float32)
        self.action_space = SimpleNamespace(nvec=np.array([2, 3]), shape=(2,))
        self.max_episode_steps = 8
        self.episode, self.t = -1, 0

    def reset(self):
        self.episode += 1
        self.t = 0
        return np.array([self.episode, self.t], dtype=np.float32)

    def action_masks(self):
        m = np.ones(5, dtype=bool)
        m[(self.worker_id + self.episode + self.t) % 2] = False                  # branch 0: one of its two actions
        m[2 + (self.worker_id + 2 * self.episode + self.t) % 3] = False          # branch 1: one of its three
        return m

    def step(self, action):
        m = self.action_masks()
        a = np.asarray(action).reshape(-1)
        if not (m[int(a[0])] and m[2 + int(a[1])]):
            raise RuntimeError(f"illegal action {a.tolist()} at episode {self.episode} step {self.t}")
        self.t += 1
        done = self.t >= self.length
        return np.array([self.episode, self.t], dtype=np.float32), 1.0, done, ({"reward": float(self.t), "length": self.t} if done else None)

    def close(self):
        pass


def _expected(worker_id, episode, t):
    e = _GridEnv(worker_id)
    e.episode, e.t = episode, t
    from environments import pack_action_masks
    return int(pack_action_masks(e.action_masks())[0])


def _legal(words):
    """One allowed action per branch of MultiDiscrete([2, 3]) from the words."""
    acts = np.zeros((len(words), 2), dtype=np.int64)
    for w, word in enumerate(words):
        word = int(word)
        acts[w, 0] = next(j for j in range(2) if (word >> j) & 1)
        acts[w, 1] = next(j for j in range(3) if (word >> (2 + j)) & 1)
    return acts


def _drive(env, worker_ids, steps=7):
    """reset + ``steps`` steps on legal actions: after every call the words are those of the observation just returned, which after
    an auto-reset is the NEW episode's first one."""
    obs = env.reset()
    seen_reset = False
    for _ in range(steps + 1):
        words = env.action_masks()
        assert words.dtype == np.uint64 and words.shape == (len(worker_ids),)
        for w, wid in enumerate(worker_ids):
            episode, t = int(obs[w, 0]), int(obs[w, 1])
            assert int(words[w]) == _expected(wid, episode, t), (wid, episode, t)
            seen_reset = seen_reset or (episode > 0 and t == 0)
        out = np.zeros(len(worker_ids), dtype=np.int64)
        assert env.action_masks(out=out) is out and [int(x) for x in out] == [int(x) for x in words]
        obs, _, _, _ = env.step(_legal(words))
    assert seen_reset


def test_serial_vec_env_action_masks_follow_auto_reset():
    from environments.vec_env import CompositeVecEnv, SerialVecEnv
    _drive(SerialVecEnv([_GridEnv(w) for w in range(3)]), [0, 1, 2])
    comp = CompositeVecEnv([SerialVecEnv([_GridEnv(0), _GridEnv(1)]), SerialVecEnv([_GridEnv(2, length=2), _GridEnv(3)])])
    _drive(comp, [0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="illegal action"):
        env = SerialVecEnv([_GridEnv(0)])
        env.reset()
        env.step(np.array([[0, 0]]))                 # worker 0, episode 0, step 0: action 0 of both branches is masked out


def test_serial_vec_env_without_masks_raises():
    from environments.vec_env import SerialVecEnv

    assert callable(SerialVecEnv([_GridEnv(0)]).action_masks)
    plain = type("Plain", (), {k: v for k, v in vars(_GridEnv).items() if k != "action_masks"})
    with pytest.raises(AttributeError, match="no action_masks"):
        SerialVecEnv([plain(0)]).action_masks()


def test_pipe_vec_env_action_masks(monkeypatch):
    """The ``("action_masks", None)`` command of worker.py through real worker processes."""
    import utils
    from environments.vec_env import PipeVecEnv
    monkeypatch.setattr(utils, "create_env", lambda cfg, worker_id=0, **kw: _GridEnv(worker_id), raising=True)
    env = PipeVecEnv(dict(type="Grid"), 2, first_worker_id=5)
    try:
        _drive(env, [5, 6])
    finally:
        env.close()
        for wk in env.workers:
            wk.process.join(timeout=10)


# ------------------------------------------------------------------ the synthetic stream
def _syn(n, first=0, seed=3, p=0.5, groups=1, **over):
    from environments.vec_env import make_vec_env
    cfg = dict(type="Synthetic", obs_shape=[6], num_actions=[2, 4, 3], max_episode_steps=9, seed=seed, p_done=0.1, pool=4)
    if p is not None:
        cfg["action_mask_p"] = p
    cfg.update(over)
    return make_vec_env(cfg, n, first, groups=groups)


def _stream(env, steps):
    obs, rew, don, words = [env.reset().copy()], [], [], []
    if hasattr(env, "action_masks"):
        words.append(env.action_masks().copy())
    for _ in range(steps):
        o, r, d, _ = env.step(np.zeros((env.num_envs, 3), dtype=np.int64))
        obs.append(o.copy()), rew.append(r.copy()), don.append(d.copy())
        if hasattr(env, "action_masks"):
            words.append(env.action_masks().copy())
    return np.stack(obs), np.stack(rew), np.stack(don), (np.stack(words) if words else None)


def test_synthetic_masks_deterministic_per_seed_and_worker():
    from environments import empty_mask_branches
    steps = 300                                              # (past one chunk of 256 pre-drawn positions)
    o4, r4, d4, w4 = _stream(_syn(4), steps)
    assert w4.shape == (steps + 1, 4) and w4.dtype == np.uint64
    # the same workers give the same words: alone, as parts of a composite front-end, with another first worker id
    _, _, _, w_again = _stream(_syn(4), steps)
    _, _, _, w_parts = _stream(_syn(4, groups=2), steps)
    _, _, _, w_tail = _stream(_syn(2, first=2), steps)
    assert np.array_equal(w4, w_again) and np.array_equal(w4, w_parts) and np.array_equal(w4[:, 2:], w_tail)
    _, _, _, w_seed = _stream(_syn(4, seed=4), steps)
    assert not np.array_equal(w4, w_seed)
    assert len({int(x) for x in w4[:, 0]}) > 8 and not np.array_equal(w4[:, 0], w4[:, 1])
    # no branch is ever empty, bits past the 9 columns are never set, and p = 0.5 really masks
    assert not empty_mask_branches(w4.reshape(-1), (2, 4, 3)).any()
    assert int(w4.max()) < (1 << 9)
    share = np.unpackbits(w4.reshape(-1).view(np.uint8)).sum() / (w4.size * 9)
    # expected share: 1 - p, plus a branch whose A draws are all below p keeping one: 0.5 + (0.5^2 + 0.5^4 + 0.5^3) / 9 = 0.549; the
    # 10,836 bits have a standard deviation of 0.005
    assert 0.52 < share < 0.58
    # ... and the rule itself, from the documented generator
    rng = np.random.default_rng((3 + 1, 2))                  # worker 1
    u = rng.random((256, 9))
    valid = u >= 0.5
    for lo, hi in ((0, 2), (2, 6), (6, 9)):
        valid[np.arange(256), lo + u[:, lo:hi].argmax(axis=1)] = True
    expect = (valid.astype(np.uint64) << np.arange(9, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert np.array_equal(w4[:256, 1], expect)


def test_synthetic_streams_keep_their_bits_with_masks():
    for over in (dict(), dict(pool=0)):
        a = _stream(_syn(3, p=None, **over), 40)
        b = _stream(_syn(3, p=0.3, **over), 40)
        assert a[3] is None and b[3] is not None
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x, y)
    all_valid = _stream(_syn(3, p=0.0), 10)[3]
    assert (all_valid == (1 << 9) - 1).all()


# ------------------------------------------------------------------ ABI mirror
def test_masked_entries_mirror_the_header():
    import ctypes
    from etm import lib
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "etm_hip.h")).read()
    masked = sorted(n for n in lib.SIGNATURES if n.endswith("_masked") and n[:-len("_masked")] in lib.SIGNATURES)
    assert masked == ["etm_heads_loss_branched_masked", "etm_heads_loss_masked", "etm_ppo_loss_masked", "etm_rollout_policy_branched_masked",
                      "etm_rollout_sample_branched_masked", "etm_rollout_trxl_branched_masked", "etm_rollout_trxl_group_branched_masked"]
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "int32_t": ctypes.c_int}

    def declared(name):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        out = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            out.append(ctypes.c_void_p if "*" in arg else ctype[arg.replace("const ", "").rsplit(" ", 1)[0]])
        return out

    for name in masked:
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == declared(name), name
        base = lib.SIGNATURES[name[:-len("_masked")]][1]
        assert declared(name[:-len("_masked")]) == base                                     # (the parser reads the plain entries right)
        extra = [ctypes.c_void_p, ctypes.c_int] if name == "etm_ppo_loss_masked" else [ctypes.c_void_p]
        assert args == base[:-1] + extra + base[-1:], name                                  # the mask goes in front of the stream
    handle = lib.load()
    assert handle.etm_abi_version() == lib.ABI_VERSION >= 58
    assert all(hasattr(handle, n) for n in masked)
    assert re.search(r"#?\s*define ETM_EINVAL", header) or "ETM_EINVAL" in header


# ------------------------------------------------------------------ torch path and enjoy.py
def test_masked_logits_bool_and_words_agree():
    import torch
    from environments import pack_action_masks
    from model import masked_logits
    g = torch.Generator().manual_seed(0)
    N, br = 6, (30, 5)                                           # the second branch straddles bit 32
    logits = [torch.randn((N, a), generator=g) for a in br]
    valid = torch.rand((N, 35), generator=g) >= 0.5
    valid[:, 0], valid[:, 34], valid[0, 31:33] = True, True, False
    out_b = masked_logits(logits, valid)
    words = pack_action_masks(valid.numpy())
    for form in (words, words.view(np.int64), torch.from_numpy(words.view(np.int64)), valid.numpy()):
        out_w = masked_logits(logits, form)
        assert all(torch.equal(a, b) for a, b in zip(out_b, out_w))
    off = 0
    for l, o, a in zip(logits, out_b, br):
        v = valid[:, off:off + a]
        assert torch.equal(o[v], l[v]) and bool((o[~v] == float("-inf")).all()) and o.shape == l.shape
        off += a
    assert out_b[1][0, 1].item() == float("-inf") and out_b[1][0, 2].item() == float("-inf")      # columns 31 and 32 = branch 1's 1 and 2
    p = torch.distributions.Categorical(logits=out_b[1]).probs
    assert bool((p[~valid[:, 30:]] == 0).all()) and torch.allclose(p.sum(-1), torch.ones(N))
    # a Discrete policy is one branch; bit 62 works
    one = masked_logits([torch.zeros((1, 63))], np.array([1 << 62], dtype=np.uint64))
    assert one[0][0, 62].item() == 0.0 and bool((one[0][0, :62] == float("-inf")).all())


def test_box_policy_refuses_a_mask_on_the_torch_path():
    from types import SimpleNamespace
    from model import ActorCriticModel
    with pytest.raises(ValueError, match="Box policy has no action mask"):
        ActorCriticModel.forward_banked(SimpleNamespace(continuous=True), None, None, action_mask=np.ones((1, 2), dtype=bool))


def test_enjoy_asks_the_environment_for_its_mask():
    """enjoy.run_episode hands ``action_masks()`` of the current observation to the model; with the mask applied the sampled actions
    never make the strict environment raise."""
    import torch
    import enjoy
    from model import masked_logits
    from torch.distributions import Categorical
    L, T, nb, D = 4, 8, 1, 32
    cfg = {"transformer": {"memory_length": L, "num_blocks": nb, "embed_dim": D}}
    env = _GridEnv(worker_id=1, length=6)
    seen = []

    def model(obs, in_memory, m, indices, action_mask=None):
        assert action_mask is not None and action_mask.shape == (1, 5) and np.array_equal(action_mask[0], env.action_masks())
        seen.append(action_mask[0].copy())
        lg = masked_logits([torch.zeros(1, 2), torch.zeros(1, 3)], action_mask)
        return [Categorical(logits=l) for l in lg], torch.zeros(1), torch.zeros((1, nb, D))

    torch.manual_seed(0)
    rewards, info = enjoy.run_episode(model, env, cfg, torch.device("cpu"))
    assert len(rewards) == 6 == len(seen) and info["length"] == 6
    rewards, _ = enjoy.run_episode(model, _reset_to(env), cfg, torch.device("cpu"), deterministic=True)      # argmax of the masked logits
    assert len(rewards) == 6


def _reset_to(env):
    env.episode = -1
    return env
