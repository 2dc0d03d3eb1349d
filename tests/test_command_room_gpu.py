"""CommandRoom on the device against the host rule, byte for byte: the kernel through the C ABI (csrc/device_env.hip) and the
device-resident front-end (environments/device_env.py) against a SerialVecEnv of host twins."""
import numpy as np
import pytest
import torch

import command_room_reference as ref

pytestmark = pytest.mark.gpu

GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
WIDTHS = [1, 3, 33]
CASES = [(1, 1, 0, 41), (3, 2, 1, 41), (5, 1, 2, 41), (16, 1, 0, 70)]        # (K, show_steps, gap_steps, steps)
SEED, FIRST = 11, 5
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()


class _Call:
    """Device and pinned operands of one sequence of kernel calls: the frame destination is rows [2, 2 + W) of a block of W + 4 rows
    with a pitch above the frame size, everything else filled with the sentinel."""

    def __init__(self, lib, G, P, W, K, show, gap, pinned_words=True):
        self.lib, self.rule = lib, (W, G, P, K, show, gap, SEED + FIRST)
        self.W, self.fb = W, 3 * G * P * G * P
        self.pitch = self.fb + 16
        dev = torch.device("cuda", 0)
        self.state = torch.zeros(int(lib.etm_command_room_state_bytes(W)) // 8, dtype=torch.int64, device=dev)
        self.block = torch.full((W + 4, self.pitch), SENTINEL, dtype=torch.uint8, device=dev)
        self.actions = torch.zeros((W, 3), dtype=torch.int64, device=dev)       # (a row stride of 3: the action is column 0)

        def words(dtype):
            t = torch.zeros(W + 2, dtype=dtype)
            return t.pin_memory() if pinned_words else t.to(dev)
        self.rewards, self.flags, self.returns = words(torch.float32), words(torch.uint8), words(torch.float32)
        self.lengths, self.masks = words(torch.int32), words(torch.int64)
        self.done = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.fill_words()

    def fill_words(self):
        for t, v in ((self.rewards, -7.0), (self.flags, SENTINEL), (self.returns, -7.0), (self.lengths, -7), (self.masks, -7)):
            t.fill_(v)

    def ptrs(self, **replace):
        # the words' destinations start at entry 1: entries 0 and W + 1 are sentinels
        p = dict(state=self.state.data_ptr(), actions=self.actions.data_ptr(), frames=self.block[2].data_ptr(), pitch=self.pitch,
                 rewards=self.rewards[1:].data_ptr(), flags=self.flags[1:].data_ptr(), returns=self.returns[1:].data_ptr(),
                 lengths=self.lengths[1:].data_ptr(), masks=self.masks[1:].data_ptr(), done=self.done.data_ptr(), value=0)
        p.update(replace)
        return p

    def reset(self, rule=None, **replace):
        p = self.ptrs(**replace)
        return self.lib.etm_command_room_reset(p["state"], p["frames"], p["pitch"], p["rewards"], p["flags"], p["returns"], p["lengths"],
                                               p["masks"], p["done"], p["value"], *(rule or self.rule), None)

    def step(self, table=None, rule=None, act_stride=3, **replace):
        if table is not None:
            self.actions[:, 0] = torch.from_numpy(np.array(table, dtype=np.int64)).to(self.actions.device)
        p = self.ptrs(**replace)
        return self.lib.etm_command_room_step(p["state"], p["actions"], act_stride, p["frames"], p["pitch"], p["rewards"], p["flags"],
                                              p["returns"], p["lengths"], p["masks"], p["done"], p["value"], *(rule or self.rule), None)

    def read(self):
        """(frames [W, fb], rewards, flags, returns, lengths, masks) of the last call; asserts every sentinel."""
        torch.cuda.synchronize()
        block = self.block.cpu().numpy()
        W = self.W
        assert (block[:2] == SENTINEL).all() and (block[2 + W:] == SENTINEL).all(), "a frame row outside [lo, hi) was written"
        assert (block[2:2 + W, self.fb:] == SENTINEL).all(), "bytes between a frame's end and the pitch were written"
        outs = [t.cpu().numpy() for t in (self.rewards, self.flags, self.returns, self.lengths, self.masks)]
        for o, v in zip(outs, (-7.0, SENTINEL, -7.0, -7, -7)):
            assert o[0] == v and o[-1] == v, "a result word outside [0, W) was written"
        return (block[2:2 + W, :self.fb].copy(),) + tuple(o[1:-1].copy() for o in outs)

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.block.cpu().numpy() == SENTINEL).all()
        for t, v in ((self.rewards, -7.0), (self.flags, SENTINEL), (self.returns, -7.0), (self.lengths, -7), (self.masks, -7)):
            assert (t.cpu().numpy() == v).all()
        assert int(self.done[0]) == 0 and (self.state.cpu().numpy() == 0).all()


def _run(call, raw, S):
    """reset + S steps -> per step (frames, rewards, flags, returns, lengths, masks); the completion word counts the calls."""
    assert call.reset(value=100) == 0
    out = [call.read()]
    assert int(call.done[0]) == 100
    for t in range(S):
        assert call.step(raw[t], value=t + 1) == 0
        out.append(call.read())
        assert int(call.done[0]) == t + 1
    return out


@pytest.mark.parametrize("G, P", GEOMETRIES)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("K, show, gap, S", CASES)
def test_kernel_equals_the_rule_byte_for_byte(lib, G, P, W, K, show, gap, S):
    want = ref.kernel_case(G, P, W, K, show, gap, S)
    raw = want["raw"]                                                   # the kernel is given the raw values, -1 .. 6
    if W == 33:
        ref.assert_covered(want["cover"])
    assert lib.etm_command_room_supported(G, P, K) == 1 and lib.etm_command_room_state_bytes(W) == 32 * W
    call = _Call(lib, G, P, W, K, show, gap)
    got = _run(call, raw, S)
    side = G * P
    for t, (frames, rewards, flags, returns, lengths, masks) in enumerate(got):
        assert np.array_equal(frames.reshape(W, 3, side, side), want["frames"][t]), f"frames of step {t}"
        assert np.array_equal(masks.view(np.uint64), want["masks"][t]), f"mask words of step {t}"
        if t == 0:
            assert not rewards.any() and not flags.any() and not returns.any() and not lengths.any()
            continue
        assert np.array_equal(rewards.view(np.uint32), want["rewards"][t - 1].view(np.uint32)), f"rewards of step {t}"
        assert np.array_equal(flags, want["flags"][t - 1]), f"flags of step {t}"
        assert np.array_equal(returns.view(np.uint32), want["returns"][t - 1].view(np.uint32)), f"returns of step {t}"
        assert np.array_equal(lengths, want["lengths"][t - 1]), f"lengths of step {t}"
    # two runs from equal state are equal -- with the result words in device memory this time
    again = _run(_Call(lib, G, P, W, K, show, gap, pinned_words=False), raw, S)
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_step_advances_the_state_exactly_once(lib):
    # two steps from one reset: the second call continues from the first one's state (not from the reset's)
    G, P, W, K, show, gap, S = 5, 8, 3, 1, 1, 0, 41
    want = ref.kernel_case(G, P, W, K, show, gap, S)
    call = _Call(lib, G, P, W, K, show, gap)
    assert call.reset() == 0
    first = call.read()
    assert call.step(want["raw"][0]) == 0 and call.step(want["raw"][1]) == 0
    frames = call.read()[0]
    assert np.array_equal(frames.reshape(want["frames"][2].shape), want["frames"][2])
    assert not np.array_equal(first[0], frames)


def test_einval_leaves_every_sentinel_in_place(lib):
    EINVAL = -1
    G, P, W, K = 5, 8, 3, 3
    call = _Call(lib, G, P, W, K, 2, 1)
    good = call.ptrs()
    bad_rules = [(0, G, P, K, 2, 1, 0), (-3, G, P, K, 2, 1, 0), (W, 4, P, K, 2, 1, 0), (W, 1, P, K, 2, 1, 0), (W, 33, P, K, 2, 1, 0),
                 (W, G, 6, K, 2, 1, 0), (W, G, 0, K, 2, 1, 0), (W, G, 68, K, 2, 1, 0), (W, G, P, 0, 2, 1, 0), (W, G, P, 17, 2, 1, 0),
                 (W, G, P, -1, 2, 1, 0), (W, G, P, K, 0, 1, 0), (W, G, P, K, 2, -1, 0), (W, G, P, K, 2 ** 30, 2 ** 30, 0)]
    for rule in bad_rules:
        assert call.reset(rule=rule) == EINVAL, rule
        assert call.step(rule=rule) == EINVAL, rule
    for name in ("state", "frames", "rewards", "flags", "returns", "lengths", "masks"):
        assert call.reset(**{name: None}) == EINVAL, name
        assert call.step(**{name: None}) == EINVAL, name
    assert call.step(actions=None) == EINVAL
    for name, off in (("state", 4), ("frames", 2), ("rewards", 2), ("returns", 1), ("lengths", 2), ("masks", 4), ("done", 4)):
        assert call.reset(**{name: good[name] + off}) == EINVAL, name
        assert call.step(**{name: good[name] + off}) == EINVAL, name
    assert call.step(actions=good["actions"] + 4) == EINVAL
    assert call.step(act_stride=0) == EINVAL
    for pitch in (call.fb - 4, call.fb + 2, 0, -call.pitch):
        assert call.reset(pitch=pitch) == EINVAL, pitch
        assert call.step(pitch=pitch) == EINVAL, pitch
    call.untouched()
    assert lib.etm_command_room_state_bytes(0) == 0 and lib.etm_command_room_supported(7, 12, 16) == 1
    assert lib.etm_command_room_supported(7, 12, 17) == 0 and lib.etm_command_room_supported(6, 12, 8) == 0
    # and the calls above left no error behind: a good call still runs, without a completion word too
    assert call.reset(pitch=call.fb, done=None) == 0
    torch.cuda.synchronize()
    assert int(call.done[0]) == 0


# ---------------------------------------------------------------------------------------------------------------- the front-end
def _host_vec(cfg, W, first):
    from environments.vec_env import make_vec_env
    return make_vec_env(dict(cfg, device=False, vectorize="serial"), W, first_worker_id=first)


@pytest.mark.parametrize("groups", [1, "parts"])
def test_front_end_equals_a_serial_vec_env_of_host_twins(groups):
    from environments.device_env import CommandRoomDeviceVecEnv, DeviceVecEnv
    from environments.vec_env import CompositeVecEnv, make_vec_env
    cfg = dict(type="CommandRoom", grid=3, cell=12, command_count=2, show_steps=1, gap_steps=1, seed=21, device=True)
    W, S, first = 5, 30, 4
    if groups == 1:
        dev = make_vec_env(cfg, W, first_worker_id=first)
        assert isinstance(dev, CommandRoomDeviceVecEnv) and isinstance(dev, DeviceVecEnv)
    else:           # parts of 2 and 3 workers with consecutive worker ids: the streams of a single front-end
        dev = CompositeVecEnv([make_vec_env(cfg, 2, first_worker_id=first), make_vec_env(cfg, 3, first_worker_id=first + 2)])
        assert all(isinstance(p, CommandRoomDeviceVecEnv) and p.device_resident for p in dev.parts)
    host = _host_vec(cfg, W, first)
    assert dev.observation_dtype == np.uint8 and dev.observation_space_shape == host.observation_space_shape == (3, 36, 36)
    assert tuple(dev.action_space_shape) == tuple(host.action_space_shape) == (5,) and dev.num_actions == host.num_actions == 5
    assert dev.max_episode_steps == host.max_episode_steps == 6 and dev.num_envs == W
    rows = torch.zeros((W, 3, 36, 36), dtype=torch.uint8).pin_memory().numpy()
    # the correct command three times in four where one is due, so that episodes end both ways
    rng = np.random.default_rng(8)
    assert np.array_equal(dev.reset(out=rows), host.reset())
    assert np.array_equal(dev.action_masks(), host.action_masks())
    ended = succeeded = 0
    for t in range(S):
        acts = rng.integers(0, 5, size=W).astype(np.int64)
        for w, e in enumerate(host.envs):
            if e.t >= e.show_length and rng.integers(0, 4) != 0:
                acts[w] = e.commands[e.t - e.show_length]
        seen = []
        obs, rewards, dones, infos = dev.step(acts, out=rows, on_rows=lambda a, b: seen.append((a, b)))
        h_obs, h_rewards, h_dones, h_infos = host.step(acts)
        assert obs is rows and np.array_equal(obs, h_obs), t
        assert rewards.dtype == np.float32 and np.array_equal(rewards, h_rewards) and dones.dtype == bool and np.array_equal(dones, h_dones)
        assert list(infos) == list(h_infos), t
        assert seen and seen[0][0] == 0 and seen[-1][1] == W and all(a[1] == b[0] for a, b in zip(seen, seen[1:]))
        words = np.zeros(W, dtype=np.int64)
        assert dev.action_masks(out=words) is words and np.array_equal(words.view(np.uint64), host.action_masks())
        ended += int(dones.sum())
        succeeded += sum(i["success"] for i in infos if i)
    assert ended >= W and 0 < succeeded < ended
    # a plain (unpinned) destination and none at all
    acts = np.zeros(W, dtype=np.int64)
    assert np.array_equal(dev.step(acts, out=np.zeros_like(rows))[0], host.step(acts)[0])
    assert np.array_equal(dev.step(acts + 4)[0], host.step(acts + 4)[0])
    with pytest.raises(ValueError, match="outside Discrete"):
        dev.step(np.full(W, 5))
    with pytest.raises(ValueError, match="outside Discrete"):
        dev.step(np.full(W, -1))
    dev.close()


def test_step_device_writes_the_rows_it_is_given():
    from environments.device_env import CommandRoomDeviceVecEnv
    W, first = 3, 2
    cfg = dict(type="CommandRoom", grid=3, cell=12, command_count=1, show_steps=1, gap_steps=0, seed=1)
    dev = CommandRoomDeviceVecEnv(W, grid=3, cell=12, command_count=1, show_steps=1, gap_steps=0, seed=1, first_worker_id=first)
    host = _host_vec(cfg, W, first)
    dev.reset(), host.reset()
    stage = torch.full((4, W + 2, 3, 36, 36), SENTINEL, dtype=torch.uint8, device="cuda")      # rows [1, 1 + W) of row t + 1
    act_dev = torch.zeros((W, 1), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    acts = np.random.default_rng(3).integers(0, 5, size=(3, W)).astype(np.int64)
    for t in range(3):
        act_dev[:, 0] = torch.from_numpy(acts[t]).cuda()
        torch.cuda.synchronize()
        if t == 1:
            rewards, dones, infos = dev.step_device(act_dev, stage[t + 1, 1:1 + W].data_ptr(), side)
        else:
            rewards, dones, infos = dev.step_device(act_dev, stage[t + 1, 1:1 + W])
        h_obs, h_rewards, h_dones, h_infos = host.step(acts[t])
        got = stage.cpu().numpy()
        assert np.array_equal(got[t + 1, 1:1 + W], h_obs) and np.array_equal(rewards, h_rewards) and np.array_equal(dones, h_dones)
        assert list(infos) == list(h_infos)
        assert np.array_equal(dev.action_masks(), host.action_masks())
        assert (got[t + 1, 0] == SENTINEL).all() and (got[t + 1, W + 1] == SENTINEL).all() and (got[t + 2:] == SENTINEL).all()
    assert dev.device_steps == 3 and dev.protocol_steps == 0
    # the protocol path continues from the same state
    assert np.array_equal(dev.step(acts[0])[0], host.step(acts[0])[0]) and dev.protocol_steps == 1
