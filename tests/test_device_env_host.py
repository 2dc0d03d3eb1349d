"""CueRoom's host rule (environments/cue_room_env.py), on a machine without a GPU: the episode draw, the cue, the frame as a palette
fill of the stated cells, moves and masks, the three ways an episode ends, auto-reset through SerialVecEnv, and every refusal."""
import numpy as np
import pytest

import cue_room_reference as ref
from environments import observation_dtype, pack_action_masks
from environments.cue_room_env import CueRoomEnv, PALETTE, corner_cells, cue_room_section, episode_draw, splitmix64
from environments.device_types import check_device_env_config
from environments.vec_env import PipeVecEnv, SerialVecEnv, make_vec_env
from utils import create_env, process_episode_info


def test_splitmix64_known_values():
    # the published test vector of splitmix64: the first outputs of the stream seeded with 0 are mix(0), mix(gamma), ... -- here one
    # call adds gamma and mixes, so splitmix64(0) is the first output
    assert splitmix64(0) == 0xE220A8397B1DCDAF
    assert splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert splitmix64((1 << 64) - 1) < 1 << 64


def test_episode_is_a_function_of_seed_worker_and_index():
    G = 7
    for stream in (0, 3, 12345):
        for ep in range(50):
            target, r, c = episode_draw(stream, ep, G)
            assert episode_draw(stream, ep, G) == (target, r, c)
            assert 0 <= target < 4 and 0 <= r < G and 0 <= c < G and (r, c) not in corner_cells(G)
    # seed + worker_id is the stream: (seed 3, worker 4) is (seed 0, worker 7)
    a, b = CueRoomEnv(7, 12, seed=3, worker_id=4), CueRoomEnv(7, 12, seed=0, worker_id=7)
    for _ in range(5):
        assert np.array_equal(a.reset(), b.reset()) and (a.target, a.row, a.col) == (b.target, b.row, b.col)
    # two workers differ, and so do a worker's episodes
    draws = [[episode_draw(w, ep, G) for ep in range(20)] for w in range(2)]
    assert draws[0] != draws[1] and len(set(draws[0])) > 10
    # every target and every start cell is drawn
    many = [episode_draw(1, ep, 3) for ep in range(400)]
    assert {d[0] for d in many} == {0, 1, 2, 3} and {d[1:] for d in many} == {(0, 1), (1, 0), (1, 1), (1, 2), (2, 1)}


def test_a_second_env_with_the_same_key_replays_the_episodes():
    acts = np.random.default_rng(0).integers(0, 4, size=60)
    runs = []
    for _ in range(2):
        e, log = CueRoomEnv(5, 8, 2, 7, seed=9, worker_id=2), []
        obs = e.reset()
        for a in acts:
            o, r, d, info = e.step(a)
            log.append((o.tobytes(), r, d, None if info is None else tuple(sorted(info.items()))))
            if d:
                log.append(e.reset().tobytes())
        runs.append((obs.tobytes(), log))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("cue_steps", [1, 2, 3])
def test_cue_is_visible_in_exactly_the_first_observations(cue_steps):
    G, P = 7, 12
    e = CueRoomEnv(G, P, cue_steps, 32, seed=1)
    cue = PALETTE[2]
    for _ in range(6):
        obs = [e.reset()]
        # walk up and down in the start column's interior so that no corner ends the episode early
        for k in range(8):
            down = e.row < G - 2 and (e.row <= 1 or k % 2 == 0)
            o, _, d, _ = e.step(2 if down else 0)
            assert not d
            obs.append(o)
        shows = [bool(((o == cue[:, None, None]).all(axis=0)).any()) for o in obs]
        assert shows == [i < cue_steps for i in range(len(obs))]
        r, c = corner_cells(G)[e.target]
        assert (obs[0][:, r * P, c * P] == cue).all()


def test_frame_is_the_palette_fill_of_the_stated_cells():
    assert len({tuple(p) for p in PALETTE}) == 4
    for G, P, cue_steps in ((3, 12, 1), (5, 8, 3), (7, 12, 2)):
        e = CueRoomEnv(G, P, cue_steps, 6, seed=4, worker_id=1)
        obs = e.reset()
        acts = np.random.default_rng(G).integers(0, 4, size=40)
        for a in acts:
            assert obs.dtype == np.uint8 and obs.shape == (3, G * P, G * P)
            assert np.array_equal(obs, ref.frame_from_cells(G, P, e.row, e.col, e.target, e.t, cue_steps))
            obs, _, done, _ = e.step(a)
            if done:       # the terminal frame shows the agent on its last cell, drawn over whatever the cell held
                assert np.array_equal(obs, ref.frame_from_cells(G, P, e.row, e.col, e.target, e.t, cue_steps))
                obs = e.reset()
    assert observation_dtype(e.observation_space) == np.uint8 and e.action_space.n == 4


def test_off_grid_move_is_a_no_op_and_its_mask_bit_is_clear():
    G = 5
    e = CueRoomEnv(G, 8, 2, 1000, seed=0)
    e.reset()
    seen = 0
    for r in range(G):
        for c in range(G):
            if (r, c) in corner_cells(G):
                continue
            e.row, e.col = r, c
            m = e.action_masks()
            assert m.dtype == bool and m.shape == (4,) and m.sum() >= 2
            assert list(m) == [r > 0, c < G - 1, r < G - 1, c > 0]
            for a in range(4):
                e.row, e.col, t0 = r, c, e.t
                e.step(a)
                assert ((e.row, e.col) == (r, c)) == (not m[a]) and e.t == t0 + 1
                seen += not m[a]
    assert seen > 0
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(4)
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(-1)


def _walk_to(e, r, c):
    """Moves from the agent's cell to (r, c): rows first (never through a corner other than the goal itself)."""
    out = []
    rr, cc = e.row, e.col
    if cc in (0, e.grid - 1) and rr != r:      # leave an edge column before moving along it towards a corner row
        step = 1 if cc == 0 else -1
        out.append(1 if step == 1 else 3)
        cc += step
    while rr != r:
        out.append(2 if r > rr else 0)
        rr += 1 if r > rr else -1
    while cc != c:
        out.append(1 if c > cc else 3)
        cc += 1 if c > cc else -1
    return out


def test_three_ways_of_ending_an_episode_and_their_infos():
    G = 5
    e = CueRoomEnv(G, 8, 2, 12, seed=2)
    # the target: reward 1, done, success 1
    e.reset()
    path = _walk_to(e, *corner_cells(G)[e.target])
    for i, a in enumerate(path):
        o, r, d, info = e.step(a)
        assert d == (i == len(path) - 1)
        if not d:
            assert r == 0.0 and info is None
    assert r == 1.0 and info == {"reward": 1.0, "length": len(path), "success": 1}
    # another corner: reward 0, done, success 0
    e.reset()
    path = _walk_to(e, *corner_cells(G)[(e.target + 2) % 4])
    for a in path:
        o, r, d, info = e.step(a)
    assert d and r == 0.0 and info == {"reward": 0.0, "length": len(path), "success": 0}
    # the time limit: done, truncated, success 0
    e.reset()
    for i in range(12):
        down = e.row < G - 2 and (e.row <= 1 or i % 2 == 0)
        o, r, d, info = e.step(2 if down else 0)
        assert d == (i == 11) and r == 0.0
    assert info == {"reward": 0.0, "length": 12, "success": 0, "truncated": True}
    res = process_episode_info([{"reward": 1.0, "length": 3, "success": 1}, {"reward": 0.0, "length": 12, "success": 0}])
    assert res["success_percent"] == 0.5


def test_auto_reset_through_serial_vec_env_and_cover():
    G, P, T, W, S = 3, 12, 6, 4, 60
    acts = np.random.default_rng(5).integers(0, 4, size=(S, W)).astype(np.int64)
    out = ref.run_rule(G, P, 2, T, seed=3, first_worker_id=0, actions=acts)
    ref.assert_covered(out["cover"])
    # the returned row of a finished worker is the first frame of its next episode; the words are that frame's
    episode = np.zeros(W, dtype=int)
    for t in range(S):
        for w in range(W):
            if out["flags"][t, w] & ref.DONE:
                episode[w] += 1
                target, r, c = episode_draw(3 + w, episode[w], G)
                assert np.array_equal(out["frames"][t + 1, w], ref.frame_from_cells(G, P, r, c, target, 0, 2))
                m = [r > 0, c < G - 1, r < G - 1, c > 0]
                assert out["masks"][t + 1, w] == pack_action_masks(np.array(m))[0]
                assert 1 <= out["lengths"][t, w] <= T
                assert bool(out["flags"][t, w] & ref.TRUNCATED) == (out["lengths"][t, w] == T and not out["flags"][t, w] & ref.SUCCESS
                                                                      and out["infos"][t][w].get("truncated", False))
            else:
                assert out["infos"][t][w] is None and out["rewards"][t, w] == 0.0
    assert episode.min() >= 5
    assert out["vec"].observation_dtype == np.uint8 and out["vec"].action_space_shape == (4,)
    # SerialVecEnv hands a cut episode's last frame over (bootstrap_truncated reads it)
    vec = SerialVecEnv([CueRoomEnv(7, 12, 2, 3, seed=0)])
    vec.reset()
    infos = [vec.step(np.array([0 if vec.envs[0].row > 1 else 2]))[3][0] for _ in range(3)]
    assert infos[2]["truncated"] and infos[2]["final_observation"].shape == (3, 84, 84)


def test_front_ends_of_the_host_twin():
    cfg = dict(type="CueRoom", grid=3, cell=12, cue_steps=2, max_episode_steps=6, seed=7)
    e = create_env(cfg, worker_id=3)
    assert isinstance(e, CueRoomEnv) and e.stream == 10 and e.max_episode_steps == 6
    serial = make_vec_env(dict(cfg, vectorize="serial"), 3, first_worker_id=2)
    assert isinstance(serial, SerialVecEnv) and [x.stream for x in serial.envs] == [9, 10, 11]
    parts = make_vec_env(dict(cfg, vectorize="serial", device=False), 4, first_worker_id=2, groups=2)
    assert [x.stream for p in parts.parts for x in p.envs] == [9, 10, 11, 12]
    pipe = make_vec_env(cfg, 2, first_worker_id=2)      # the worker processes, through utils.create_env
    try:
        assert isinstance(pipe, PipeVecEnv) and pipe.observation_dtype == np.uint8
        acts = np.random.default_rng(1).integers(0, 4, size=(12, 2))
        a, b = pipe.reset(), serial.reset()
        assert np.array_equal(a, b[:2])
        two = SerialVecEnv(serial.envs[:2])
        for t in range(12):
            ra, rb = pipe.step(acts[t]), two.step(acts[t])
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
            assert np.array_equal(pipe.action_masks(), two.action_masks())
    finally:
        pipe.close()


BASE = dict(type="CueRoom", grid=7, cell=12, cue_steps=2, max_episode_steps=32, seed=0)


@pytest.mark.parametrize("change, match", [
    (dict(colour="red"), "unknown keys"),
    (dict(grid=4), "odd"),
    (dict(grid=1), "odd"),
    (dict(cell=10), "multiple of 4"),
    (dict(cell=0), "multiple of 4"),
    (dict(cue_steps=0), "cue_steps"),
    (dict(max_episode_steps=0), "max_episode_steps"),
    (dict(grid=3, cell=8), "too small for the image encoder"),
    (dict(grid=7.0), "integer"),
    (dict(device="yes"), "true or false"),
])
def test_refused_sections(change, match):
    with pytest.raises(ValueError, match=match):
        cue_room_section(dict(BASE, **change))
    with pytest.raises(ValueError, match=match):
        create_env(dict(BASE, **change))
    with pytest.raises(ValueError, match=match):
        make_vec_env(dict(BASE, **change), 2)


def test_refused_combinations_of_device_true():
    cfg = dict(environment=dict(BASE, device=True))
    assert check_device_env_config(cfg) is True
    assert check_device_env_config(dict(environment=dict(BASE))) is False
    assert check_device_env_config(dict(environment=dict(BASE, device=False), worker_processes=True, bootstrap_truncated=True)) is False
    assert check_device_env_config(dict(environment=dict(type="Synthetic"), worker_processes=True)) is False
    with pytest.raises(ValueError, match="worker_processes: false"):
        check_device_env_config(dict(cfg, worker_processes=True))
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        check_device_env_config(dict(cfg, bootstrap_truncated=True))
    with pytest.raises(ValueError, match="data-parallel"):
        check_device_env_config(cfg, world=2)
    # max_episode_steps below memory_length: the existing rule of the window tables
    from trainer import build_window_tables, check_byte_observation_transport
    with pytest.raises(ValueError, match="memory_length"):
        build_window_tables(8, 6)
    # the shared segment of the worker processes types its rows as float32: CueRoom has no float form
    with pytest.raises(ValueError, match="uint8"):
        check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=True))


def test_config_twins_differ_in_the_device_key_only():
    import os

    from yaml_parser import YamlParser
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "episodic-transformer-memory-ppo_amd", "configs")
    host = YamlParser(os.path.join(here, "cue_room.yaml")).get_config()
    dev = YamlParser(os.path.join(here, "cue_room_device.yaml")).get_config()
    assert not cue_room_section(host["environment"])["device"] and cue_room_section(dev["environment"])["device"]
    dev["environment"]["device"] = host["environment"].get("device", False)
    host["environment"].setdefault("device", False)
    assert host == dev
    assert host["environment"]["max_episode_steps"] >= host["transformer"]["memory_length"]
