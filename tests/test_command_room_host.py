"""CommandRoom's host rule (environments/command_room_env.py), on a machine without a GPU: the episode draw, the phases, rewards,
infos and masks, the frame against a per-cell reconstruction, auto-reset through SerialVecEnv, the front-ends of the host twin and
every refusal."""
import numpy as np
import pytest

import command_room_reference as ref
from environments import observation_dtype, pack_action_masks
from environments.command_room_env import (MOVES, PALETTE, CommandRoomEnv, command_room_section, episode_draw, pack_commands, shown)
from environments.device_types import check_device_env_config
from environments.vec_env import PipeVecEnv, SerialVecEnv, make_vec_env
from utils import create_env, process_episode_info

# ---------------------------------------------------------------------------------------------------------------- the episode draw
def _mix(z):
    """splitmix64 in numpy's uint64 arithmetic (wraps by itself): the second implementation."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _second_draw(stream, episode, G, K):
    """The draw written a second time, independently: uint64 arrays, the valid moves as a bit word whose set bits are counted off."""
    with np.errstate(over="ignore"):
        h = _mix(_mix(np.uint64(stream)) + np.uint64(episode))
    start = int((h >> np.uint64(8)) % np.uint64(G * G))
    r, c = divmod(start, G)
    row, col, x, word = r, c, h, 0
    for j in range(K):
        x = _mix(x)
        bits = (r > 0) | (c < G - 1) << 1 | (r < G - 1) << 2 | (c > 0) << 3 | 1 << 4
        pick = int((x >> np.uint64(16)) % np.uint64(bin(bits).count("1")))
        a = [b for b in range(5) if bits >> b & 1][pick]
        word |= a << (3 * j)
        r += (a == 2) - (a == 0)
        c += (a == 1) - (a == 3)
    return row, col, word


def test_episode_draw_matches_hand_computed_values():
    # worked out step by step from the stated rule with the published splitmix64 constants (test_device_env_host.py checks the mixer
    # against its published vector).  Key (stream 0, episode 0), G = 3: h = 0xa706dd2f4d197e6f, (h >> 8) mod 9 = 6 -> cell (2, 0);
    # there up is on the grid, right is, down and left are not: the list is (up, right, stay) and pick 1 is right; at (2, 1) the list
    # is (up, right, left, stay) and pick 0 is up; at (1, 1) all five, pick 0: up; at (0, 1) (right, down, left, stay), pick 3: stay
    assert episode_draw(0, 0, 3, 4) == (2, 0, (1, 0, 0, 4))
    # key (stream 12, episode 5), G = 7: h = 0x5fc468e3fa43f985, (h >> 8) mod 49 = 19 -> cell (2, 5); picks 1 of 5, then at the right
    # edge 0, 1, 3, 3, 2 of (up, down, left, stay), then 4 of 5 twice
    assert episode_draw(12, 5, 7, 8) == (2, 5, (1, 0, 2, 4, 4, 3, 4, 4))
    assert pack_commands((1, 0, 0, 4)) == 1 | 4 << 9 and pack_commands((4,) * 16) == int("4" * 16, 8)


def test_episode_draw_equals_a_second_implementation_over_1000_keys():
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(1000):
        stream, episode = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 40))
        G, K = int(rng.choice([3, 5, 7, 9, 31])), int(rng.integers(1, 17))
        row, col, commands = episode_draw(stream, episode, G, K)
        assert (row, col, pack_commands(commands)) == _second_draw(stream, episode, G, K)
        assert len(commands) == K and pack_commands(commands) < 1 << 48
        seen.update(commands)
    assert seen == {0, 1, 2, 3, 4}
    # the stream is taken mod 2^64, and seed + worker_id is the stream
    assert episode_draw((1 << 64) + 3, 2, 5, 6) == episode_draw(3, 2, 5, 6)
    a, b = CommandRoomEnv(7, 12, seed=3, worker_id=4), CommandRoomEnv(7, 12, seed=0, worker_id=7)
    for _ in range(4):
        assert np.array_equal(a.reset(), b.reset()) and (a.row, a.col, a.commands) == (b.row, b.col, b.commands)


def test_every_drawn_sequence_stays_on_the_grid_at_the_smallest_grid():
    G, K = 3, 16
    starts = set()
    for stream in range(4):
        for episode in range(250):
            r, c, commands = episode_draw(stream, episode, G, K)
            starts.add((r, c))
            for a in commands:
                r, c = r + MOVES[a][0], c + MOVES[a][1]
                assert 0 <= r < G and 0 <= c < G
    assert len(starts) == G * G


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("G, P, K, show, gap", [(3, 12, 1, 1, 0), (5, 8, 3, 2, 1), (7, 12, 5, 1, 2), (9, 4, 16, 1, 0)])
def test_phases_rewards_infos_masks_and_frames(G, P, K, show, gap):
    L = show + gap
    e = CommandRoomEnv(G, P, K, show, gap, seed=4, worker_id=1)
    assert e.max_episode_steps == K * L + K and e.action_space.n == 5 and observation_dtype(e.observation_space) == np.uint8
    assert len({tuple(p) for p in PALETTE}) == 4
    rng = np.random.default_rng(G)
    outcomes = set()
    for episode in range(12):
        obs = e.reset()
        assert (e.row, e.col, e.commands) == episode_draw(4 + 1, episode, G, K)
        stop_at = K if episode % 2 == 0 else int(rng.integers(0, K))        # the command that is answered wrongly (K: none)
        row, col = e.row, e.col
        for t in range(K * L + K):
            assert obs.dtype == np.uint8 and obs.shape == (3, G * P, G * P)
            if t < K * L:
                phase = "show" if t % L < show else "gap"
                assert shown(t, K, show, gap) == (phase, t // L)
                assert np.array_equal(obs, ref.frame_from_cells(G, P, phase, e.commands[t // L], row, col))
                assert e.action_masks().all() and e.action_masks().shape == (5,)
                obs, r, d, info = e.step(int(rng.integers(0, 5)))           # ignored
                assert (r, d, info) == (0.0, False, None) and (e.row, e.col) == (row, col)
                continue
            k = t - K * L
            assert shown(t, K, show, gap) == ("execute", k)
            assert np.array_equal(obs, ref.frame_from_cells(G, P, "execute", 4, row, col))
            assert list(e.action_masks()) == [row > 0, col < G - 1, row < G - 1, col > 0, True]
            cmd = e.commands[k]
            assert e.action_masks()[cmd]
            if k == stop_at:
                obs, r, d, info = e.step((cmd + 1 + int(rng.integers(0, 4))) % 5)
                assert r == 0.0 and d and info == {"reward": float(np.float32(k) * np.float32(0.1)), "length": t + 1, "success": 0}
                assert (e.row, e.col) == (row, col)
                outcomes.add("failure")
                break
            obs, r, d, info = e.step(cmd)
            row, col = row + MOVES[cmd][0], col + MOVES[cmd][1]
            assert np.float32(r) == np.float32(0.1) and (e.row, e.col) == (row, col) and d == (k == K - 1)
            if d:
                assert info == {"reward": float(np.float32(K) * np.float32(0.1)), "length": K * L + K, "success": 1}
                outcomes.add("success")
            else:
                assert info is None
    assert outcomes == {"success", "failure"}
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(5)
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(-1)
    with pytest.raises(RuntimeError, match="before reset"):
        CommandRoomEnv(G, P, K, show, gap).step(0)
    res = process_episode_info([{"reward": 0.3, "length": 9, "success": 1}, {"reward": 0.0, "length": 7, "success": 0}])
    assert res["success_percent"] == 0.5


def test_stay_has_no_pointer_cell_and_a_gap_is_all_floor():
    floor, mark, pointer, agent = (PALETTE[i] for i in range(4))
    f = ref.frame_from_cells(3, 12, "show", 4, 0, 0)
    assert (f[:, 18, 18] == mark).all() and not (f == pointer[:, None, None]).all(axis=0).any()
    f = ref.frame_from_cells(3, 12, "show", 1, 0, 0)
    assert (f[:, 18, 30] == pointer).all() and (f[:, 18, 18] == mark).all() and (f[:, 0, 0] == floor).all()
    assert (ref.frame_from_cells(3, 12, "gap", 1, 0, 0) == floor[:, None, None]).all()
    assert (ref.frame_from_cells(3, 12, "execute", 4, 2, 0)[:, 30, 6] == agent).all()


def test_auto_reset_through_serial_vec_env_and_cover():
    G, P, K, show, gap, W, S = 3, 12, 3, 1, 1, 4, 80
    out = ref.run_rule(G, P, K, show, gap, seed=3, first_worker_id=0, S=S, W=W, table_seed=5)
    ref.assert_covered(out["cover"])
    assert out["raw"].min() == -1 and out["raw"].max() == 6
    episode = np.zeros(W, dtype=int)
    for t in range(S):
        for w in range(W):
            if out["flags"][t, w] & ref.DONE:
                # the returned row of a finished worker is the first frame of its next episode; the words are that frame's
                episode[w] += 1
                r, c, commands = episode_draw(3 + w, episode[w], G, K)
                assert np.array_equal(out["frames"][t + 1, w], ref.frame_from_cells(G, P, "show", commands[0], r, c))
                assert out["masks"][t + 1, w] == pack_action_masks(np.ones((1, 5), dtype=bool))[0] == 31
                assert K * (show + gap) + 1 <= out["lengths"][t, w] <= K * (show + gap) + K
                n = out["lengths"][t, w] - K * (show + gap) - (0 if out["flags"][t, w] & ref.SUCCESS else 1)
                assert out["returns"][t, w] == np.float32(n) * np.float32(0.1)
            else:
                assert out["infos"][t][w] is None and out["lengths"][t, w] == 0
    assert episode.min() >= 5
    assert out["vec"].observation_dtype == np.uint8 and out["vec"].action_space_shape == (5,) and out["vec"].max_episode_steps == 9


def test_front_ends_of_the_host_twin():
    cfg = dict(type="CommandRoom", grid=3, cell=12, command_count=2, show_steps=1, gap_steps=1, seed=7)
    e = create_env(cfg, worker_id=3)
    assert isinstance(e, CommandRoomEnv) and e.stream == 10 and e.max_episode_steps == 6
    assert isinstance(create_env(dict(cfg, device=True)), CommandRoomEnv)         # (the key means nothing to a single environment)
    serial = make_vec_env(dict(cfg, vectorize="serial", device=False), 3, first_worker_id=2)
    assert isinstance(serial, SerialVecEnv) and [x.stream for x in serial.envs] == [9, 10, 11]
    parts = make_vec_env(dict(cfg, vectorize="serial", device=False), 4, first_worker_id=2, groups=2)
    assert [x.stream for p in parts.parts for x in p.envs] == [9, 10, 11, 12]
    pipe = make_vec_env(cfg, 2, first_worker_id=2)      # the worker processes, through utils.create_env
    try:
        assert isinstance(pipe, PipeVecEnv) and pipe.observation_dtype == np.uint8 and pipe.num_actions == 5
        acts = np.random.default_rng(1).integers(0, 5, size=(12, 2))
        assert np.array_equal(pipe.reset(), serial.reset()[:2])
        two = SerialVecEnv(serial.envs[:2])
        for t in range(12):
            ra, rb = pipe.step(acts[t]), two.step(acts[t])
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
            assert np.array_equal(pipe.action_masks(), two.action_masks())
    finally:
        pipe.close()


# ---------------------------------------------------------------------------------------------------------------- the refusals
BASE = dict(type="CommandRoom", grid=7, cell=12, command_count=8, show_steps=1, gap_steps=1, seed=0)


def test_section_defaults():
    assert command_room_section(dict(type="CommandRoom")) == dict(grid=7, cell=12, command_count=8, show_steps=1, gap_steps=1, seed=0,
                                                                  device=False)
    assert command_room_section(dict(BASE, device=True, vectorize="serial"))["device"] is True


@pytest.mark.parametrize("change, match", [
    (dict(colour="red"), "unknown keys"),
    (dict(cue_steps=2), "unknown keys"),
    (dict(grid=4), "odd"),
    (dict(grid=1), "odd"),
    (dict(grid=33), "odd"),
    (dict(cell=10), "multiple of 4"),
    (dict(cell=0), "multiple of 4"),
    (dict(cell=68), "multiple of 4"),
    (dict(grid=3, cell=8), "too small for the image encoder"),
    (dict(command_count=0), "command_count"),
    (dict(command_count=17), "command_count"),
    (dict(show_steps=0), "show_steps"),
    (dict(gap_steps=-1), "gap_steps"),
    (dict(grid=7.0), "integer"),
    (dict(command_count=True), "integer"),
    (dict(gap_steps="1"), "integer"),
    (dict(device="yes"), "true or false"),
    (dict(device=1), "true or false"),
])
def test_refused_sections(change, match):
    with pytest.raises(ValueError, match=match):
        command_room_section(dict(BASE, **change))
    with pytest.raises(ValueError, match=match):
        create_env(dict(BASE, **change))
    with pytest.raises(ValueError, match=match):
        make_vec_env(dict(BASE, **change), 2)


def test_refused_combinations_of_device_true():
    cfg = dict(environment=dict(BASE, device=True))
    assert check_device_env_config(cfg) is True
    assert check_device_env_config(dict(environment=dict(BASE))) is False
    assert check_device_env_config(dict(environment=dict(BASE, device=False), worker_processes=True, bootstrap_truncated=True)) is False
    with pytest.raises(ValueError, match="worker_processes: false"):
        check_device_env_config(dict(cfg, worker_processes=True))
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        check_device_env_config(dict(cfg, bootstrap_truncated=True))
    with pytest.raises(ValueError, match="data-parallel"):
        check_device_env_config(cfg, world=2)
    with pytest.raises(ValueError, match="command_count"):      # the section's own refusals come first
        check_device_env_config(dict(environment=dict(BASE, device=True, command_count=0)))
    # max_episode_steps = K L + K below memory_length: the existing rule of the window tables
    from trainer import build_window_tables, check_byte_observation_transport
    with pytest.raises(ValueError, match="memory_length"):
        build_window_tables(CommandRoomEnv(7, 12, 2, 1, 0).max_episode_steps + 1, CommandRoomEnv(7, 12, 2, 1, 0).max_episode_steps)
    # the shared segment of the worker processes types its rows as float32: the type has no float form
    with pytest.raises(ValueError, match="uint8"):
        check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=True))
    check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=False))


def test_config_twins_differ_in_the_device_key_only():
    import os

    from yaml_parser import YamlParser
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "episodic-transformer-memory-ppo_amd", "configs")
    host = YamlParser(os.path.join(here, "command_room.yaml")).get_config()
    dev = YamlParser(os.path.join(here, "command_room_device.yaml")).get_config()
    hs, ds = command_room_section(host["environment"]), command_room_section(dev["environment"])
    assert not hs["device"] and ds["device"]
    assert host["environment"]["vectorize"] == dev["environment"]["vectorize"] == "serial"
    dev["environment"]["device"] = host["environment"].get("device", False)
    host["environment"].setdefault("device", False)
    assert host == dev
    K, L = hs["command_count"], hs["show_steps"] + hs["gap_steps"]
    assert host["transformer"]["memory_length"] <= K * L + K
