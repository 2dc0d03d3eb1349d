"""PathRoom's host rule (environments/path_room_env.py), on a machine without a GPU: the episode draw, every branch of the step
rule, rewards, infos and masks, the frame against a per-cell reconstruction, auto-reset through SerialVecEnv, the cover condition of
the kernel test's action tables, the front-ends of the host twin and every refusal."""
import numpy as np
import pytest

import path_room_reference as ref
from environments import observation_dtype, pack_action_masks
from environments.device_types import DEVICE_ENV_TYPES, check_device_env_config
from environments.path_room_env import (MOVES, PALETTE, PathRoomEnv, episode_draw, pack_moves, path_cells, path_room_section,
                                        unpack_moves)
from environments.vec_env import PipeVecEnv, SerialVecEnv, make_vec_env
from utils import create_env, process_episode_info

UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3
TENTH = np.float32(0.1)


# ---------------------------------------------------------------------------------------------------------------- the episode draw
def _mix(z):
    """splitmix64 in numpy's uint64 arithmetic (wraps by itself): the second implementation."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _second_draw(stream, episode, G, M):
    """The draw written a second time, independently: uint64 arrays, the candidates as a bit word whose set bits are counted off,
    the path word built in place.  -> (origin row, n, word)."""
    with np.errstate(over="ignore"):
        h = _mix(_mix(np.uint64(stream)) + np.uint64(episode))
    r = origin = int((h >> np.uint64(8)) % np.uint64(G))
    c, x, word, n, last = 0, h, 0, 0, None
    while n < M and c != G - 1:
        x = _mix(x)
        bits = (r > 0 and last != DOWN) | 1 << 1 | (r < G - 1 and last != UP) << 2
        pick = int((x >> np.uint64(16)) % np.uint64(bin(bits).count("1")))
        last = [b for b in range(3) if bits >> b & 1][pick]
        word |= last << (2 * n)
        r += (last == DOWN) - (last == UP)
        c += last == RIGHT
        n += 1
    return origin, n, word


def test_episode_draw_matches_hand_computed_values():
    # worked out step by step from the stated rule with the published splitmix64 constants (test_device_env_host.py checks the mixer
    # against its published vector).  Key (stream 0, episode 0), G = 3: h = 0xa706dd2f4d197e6f, (h >> 8) mod 3 = 0 -> the origin is
    # (0, 0); there up is off the grid: the list is (right, down) and pick 0 of 2 is right; at (0, 1) the same list, pick 0: right;
    # (0, 2) is in the last column: the walk stops after 2 of the 32 moves
    assert episode_draw(0, 0, 3, 32) == (0, (1, 1)) == episode_draw(0, 0, 3, 2)
    assert episode_draw(0, 0, 3, 1) == (0, (1,))
    # key (stream 12, episode 5), G = 7: h = 0x5fc468e3fa43f985, (h >> 8) mod 7 = 5 -> (5, 0); all three candidates, pick 2: down;
    # at (6, 0) after down neither up (it would undo the move) nor down (the edge): right alone; then (up, right) with picks 1, 1, 1:
    # right three times, and pick 0: up
    assert episode_draw(12, 5, 7, 6) == (5, (2, 1, 1, 1, 1, 0))
    assert path_cells(5, (2, 1, 1, 1, 1, 0)) == [(5, 0), (6, 0), (6, 1), (6, 2), (6, 3), (6, 4), (5, 4)]
    assert pack_moves((1, 0, 0, 2)) == 1 | 2 << 6 and unpack_moves(1 | 2 << 6, 4) == (1, 0, 0, 2)
    assert pack_moves((2,) * 32) == int("2" * 32, 4) and pack_moves((2,) * 32) >> 63 == 1


def test_episode_draw_equals_a_second_implementation_and_keeps_its_promises():
    rng = np.random.default_rng(0)
    seen, lengths, stopped_early = set(), set(), 0
    for _ in range(1500):
        stream, episode = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 40))
        G, M = int(rng.choice([3, 5, 7, 9, 31])), int(rng.integers(1, 33))
        origin, moves = episode_draw(stream, episode, G, M)
        n = len(moves)
        assert (origin, n, pack_moves(moves)) == _second_draw(stream, episode, G, M)
        assert unpack_moves(pack_moves(moves), n) == moves and pack_moves(moves) < 1 << 64
        assert 1 <= n <= M and 0 <= origin < G and set(moves) <= {UP, RIGHT, DOWN}
        cells = path_cells(origin, moves)
        assert cells[0] == (origin, 0) and len(set(cells)) == n + 1 and cells[-1] != cells[0]
        assert all(0 <= r < G and 0 <= c < G for r, c in cells)
        # it stops exactly on reaching the last column: no earlier cell is there, and a shorter walk used all M moves
        assert all(c < G - 1 for _, c in cells[:-1])
        assert n == M or cells[-1][1] == G - 1
        stopped_early += n < M
        # never up after down, never down after up
        assert all({a, b} != {UP, DOWN} for a, b in zip(moves, moves[1:]))
        seen.update(moves)
        lengths.add(n)
    assert seen == {UP, RIGHT, DOWN} and stopped_early > 100 and {1, 32} <= lengths
    # the stream is taken mod 2^64, and seed + worker_id is the stream
    assert episode_draw((1 << 64) + 3, 2, 5, 6) == episode_draw(3, 2, 5, 6)
    a, b = PathRoomEnv(7, 12, seed=3, worker_id=4), PathRoomEnv(7, 12, seed=0, worker_id=7)
    for _ in range(4):
        assert np.array_equal(a.reset(), b.reset()) and (a.origin, a.moves) == (b.origin, b.moves)


def test_bit_63_of_the_path_word_is_used_at_the_largest_grid():
    # G = 31, M = 32 is the only geometry where move 31 exists and can be "down" (2 = binary 10: bit 63)
    words = [pack_moves(episode_draw(stream, episode, 31, 32)[1]) for stream in range(8) for episode in range(40)]
    high = [w for w in words if w >> 63]
    assert 20 < len(high) < len(words) - 20
    assert all(unpack_moves(w, 32)[31] == DOWN for w in high)
    # with one move fewer the word ends below bit 62
    assert not any(pack_moves(episode_draw(s, e, 31, 31)[1]) >> 62 for s in range(4) for e in range(40))


# ---------------------------------------------------------------------------------------------------------------- the rule
class _Fixed(PathRoomEnv):
    """A twin whose path is given, not drawn: the rule on a layout worked out by hand."""

    def __init__(self, origin, moves, grid=5, cell=8, max_episode_steps=64):
        super().__init__(grid, cell, max(1, len(moves)), max_episode_steps)
        self._fixed = (origin, tuple(moves))

    def reset(self, **kwargs):
        super().reset()
        self.origin, self.moves = self._fixed
        self.cells = path_cells(self.origin, self.moves)
        self.row, self.col = self.origin, 0
        return self._obs()


def _f32(k):
    return float(np.float32(k) * TENTH)


def test_every_branch_of_the_step_rule_on_a_path_with_a_bend():
    # G = 5, origin (2, 0); the path: down, down, right, up, up, up, right ->
    # (2,0) (3,0) (4,0) (4,1) (3,1) (2,1) (1,1) (1,2): n = 7, the goal (1, 2); (2,1) is index 5 and lies right of the origin
    G, P = 5, 8
    e = _Fixed(2, (DOWN, DOWN, RIGHT, UP, UP, UP, RIGHT))
    goal = (1, 2)
    obs = e.reset()
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, None, (2, 0)))
    # off the grid: a no-op
    obs, r, d, info = e.step(LEFT)
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.best, e.t) == (2, 0, 0, 1)
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, None, (2, 0)))
    # progress: one index forwards pays one tenth
    obs, r, d, info = e.step(DOWN)
    assert (r, d, info) == (_f32(1), False, None) and (e.row, e.col, e.best) == (3, 0, 1)
    # backwards pays nothing and keeps best
    obs, r, d, info = e.step(UP)
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.best) == (2, 0, 1)
    # a jump across the bend: from the origin (index 0) right onto (2, 1), index 5, pays 5 - best = 4 tenths
    obs, r, d, info = e.step(RIGHT)
    assert (r, d, info) == (_f32(4), False, None) and (e.row, e.col, e.best) == (2, 1, 5)
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, None, (2, 1)))
    # a jump backwards across the bend (index 5 -> index 0) pays nothing
    obs, r, d, info = e.step(LEFT)
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.best) == (2, 0, 5)
    # a fall: (1, 0) is not on the path -> back on the origin, the cell marked in the next observation only, best kept
    obs, r, d, info = e.step(UP)
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.best, e.mark) == (2, 0, 5, (1, 0))
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, (1, 0), (2, 0)))
    # progress that was paid is not paid again: index 1 <= best
    obs, r, d, info = e.step(DOWN)
    assert (r, d, info) == (0.0, False, None) and e.mark is None
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, None, (3, 0)))
    # a fall from a cell further on also ends on the origin
    e.step(UP), e.step(RIGHT)
    obs, r, d, info = e.step(RIGHT)                                      # (2, 2) is not on the path
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.mark) == (2, 0, (2, 2))
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, (2, 2), (2, 0)))
    # on to the goal: index 6 pays 1, the goal pays 1 + 10
    e.step(RIGHT)
    obs, r, d, info = e.step(UP)
    assert (r, d, info) == (_f32(1), False, None) and e.best == 6
    t = e.t
    obs, r, d, info = e.step(RIGHT)
    assert np.float32(r) == np.float32(11) * TENTH and d
    assert info == {"reward": float(np.float32(17) * TENTH), "length": t + 1, "success": 1}
    assert np.array_equal(obs, ref.frame_from_cells(G, P, goal, None, goal))      # (the agent is drawn over the goal)
    # the rewards of the episode sum to the info's reward in tenths: 1 + 4 + 1 + 11
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(4)
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(-1)
    with pytest.raises(RuntimeError, match="before reset"):
        PathRoomEnv(5, 8).step(0)


def test_time_limit_cuts_with_truncated_unless_the_step_reaches_the_goal():
    e = _Fixed(0, (RIGHT, RIGHT), grid=3, cell=12, max_episode_steps=3)
    e.reset()
    assert e.step(UP)[1:] == (0.0, False, None)
    assert e.step(RIGHT)[1:] == (_f32(1), False, None)
    obs, r, d, info = e.step(DOWN)                                       # a fall in the last step: cut, the mark still in its frame
    assert r == 0.0 and d and info == {"reward": _f32(1), "length": 3, "success": 0, "truncated": True}
    assert np.array_equal(obs, ref.frame_from_cells(3, 12, (0, 2), (1, 1), (0, 0)))
    e.reset()
    e.step(RIGHT), e.step(LEFT)
    assert e.step(UP)[3] == {"reward": _f32(1), "length": 3, "success": 0, "truncated": True}
    e = _Fixed(0, (RIGHT, RIGHT), grid=3, cell=12, max_episode_steps=2)
    e.reset()
    e.step(RIGHT)
    obs, r, d, info = e.step(RIGHT)                                      # the goal in the last step: not a cut
    assert np.float32(r) == np.float32(11) * TENTH and d and info == {"reward": float(np.float32(12) * TENTH), "length": 2, "success": 1}
    e = _Fixed(1, (RIGHT,), grid=3, cell=12, max_episode_steps=1)
    e.reset()
    assert e.step(UP)[3] == {"reward": 0.0, "length": 1, "success": 0, "truncated": True}


def test_info_arithmetic_is_one_float32_multiply():
    # float32(k) * float32(0.1), widened to a Python float: not the float64 product
    assert float(np.float32(7) * TENTH) == 0.699999988079071 != 0.7 and float(np.float32(3) * TENTH) == 0.30000001192092896
    e = _Fixed(0, (RIGHT,) * 4, grid=5, cell=8)
    e.reset()
    rewards = [e.step(RIGHT) for _ in range(4)]
    assert [np.float32(r[1]) for r in rewards] == [TENTH, TENTH, TENTH, np.float32(11) * TENTH]
    assert rewards[-1][3] == {"reward": float(np.float32(14) * TENTH), "length": 4, "success": 1}
    res = process_episode_info([{"reward": 1.4, "length": 4, "success": 1}, {"reward": 0.2, "length": 64, "success": 0}])
    assert res["success_percent"] == 0.5


@pytest.mark.parametrize("G, P, M, limit", [(3, 12, 1, 4), (5, 8, 5, 9), (7, 12, 16, 64), (9, 4, 32, 40), (31, 4, 32, 40)])
def test_drawn_episodes_masks_frames_and_rewards(G, P, M, limit):
    e = PathRoomEnv(G, P, M, limit, seed=4, worker_id=1)
    assert e.max_episode_steps == limit and e.action_space.n == 4 and observation_dtype(e.observation_space) == np.uint8
    assert e.observation_space.shape == (3, G * P, G * P)
    rng = np.random.default_rng(G + M)
    outcomes = set()
    for episode in range(10):
        obs = e.reset()
        origin, moves = episode_draw(5, episode, G, M)
        cells = path_cells(origin, moves)
        assert (e.origin, e.moves, e.cells) == (origin, moves, cells) and (e.row, e.col) == (origin, 0)
        best = paid = 0
        mark = None
        for t in range(limit):
            assert obs.dtype == np.uint8 and np.array_equal(obs, ref.frame_from_cells(G, P, cells[-1], mark, (e.row, e.col)))
            row, col = e.row, e.col
            assert list(e.action_masks()) == [row > 0, col < G - 1, row < G - 1, col > 0] and e.action_masks().sum() >= 2
            here = cells.index((row, col))
            a = moves[here] if episode % 2 == 0 or rng.integers(0, 4) else int(rng.integers(0, 4))
            what = ref.classify(e, a)
            obs, r, d, info = e.step(a)
            mark = None
            if what == "off_grid":
                assert (e.row, e.col) == (row, col) and r == 0.0 and not e.action_masks()[a]
            elif what == "fall":
                mark = (row + MOVES[a][0], col + MOVES[a][1])
                assert (e.row, e.col) == (origin, 0) and r == 0.0 and e.mark == mark
            else:
                k = max(what - best, 0) + (10 if what == len(moves) else 0)
                best = max(best, what)
                paid += k
                assert (e.row, e.col) == cells[what] and np.float32(r) == np.float32(k) * TENTH
            if d:
                success = int(what == len(moves))
                want = {"reward": float(np.float32(paid) * TENTH), "length": t + 1, "success": success}
                if not success:
                    assert t + 1 == limit
                    want["truncated"] = True
                assert info == want and paid == best + 10 * success
                outcomes.add("success" if success else "cut")
                break
            assert info is None
        else:
            raise AssertionError("the episode outlived max_episode_steps")
    assert "success" in outcomes


def test_frame_colours():
    floor, goal, mark, agent = (PALETTE[i] for i in range(4))
    assert [tuple(p) for p in PALETTE] == [(28, 28, 36), (64, 192, 96), (232, 64, 200), (240, 200, 48)]
    f = ref.frame_from_cells(3, 12, (0, 2), (1, 1), (2, 0))
    assert (f[:, 6, 30] == goal).all() and (f[:, 18, 18] == mark).all() and (f[:, 30, 6] == agent).all() and (f[:, 0, 0] == floor).all()
    assert (ref.frame_from_cells(3, 12, (0, 2), None, (0, 2))[:, 6, 30] == agent).all()      # the agent is drawn last
    e = PathRoomEnv(3, 12, 3, 6, seed=2)
    obs = e.reset()
    counts = {tuple(c): int((obs == np.asarray(c, dtype=np.uint8)[:, None, None]).all(axis=0).sum()) for c in (floor, goal, mark, agent)}
    assert counts == {tuple(floor): 7 * 144, tuple(goal): 144, tuple(mark): 0, tuple(agent): 144}      # path and origin are not drawn


def test_auto_reset_through_serial_vec_env():
    G, P, M, limit, W, S = 3, 12, 3, 6, 4, 80
    out = ref.run_rule(G, P, M, limit, seed=3, first_worker_id=0, S=S, W=W, table_seed=5)
    assert out["raw"].min() == -1 and out["raw"].max() == 5
    episode = np.zeros(W, dtype=int)
    cut = 0
    for t in range(S):
        for w in range(W):
            if out["flags"][t, w] & ref.DONE:
                # the returned row of a finished worker is the first frame of its next episode; the words are that frame's
                episode[w] += 1
                origin, moves = episode_draw(3 + w, episode[w], G, M)
                goal = path_cells(origin, moves)[-1]
                assert np.array_equal(out["frames"][t + 1, w], ref.frame_from_cells(G, P, goal, None, (origin, 0)))
                want = pack_action_masks(np.array([[origin > 0, True, origin < G - 1, False]]))[0]
                assert out["masks"][t + 1, w] == want
                assert 1 <= out["lengths"][t, w] <= limit
                info = out["infos"][t][w]
                if out["flags"][t, w] & ref.TRUNCATED:
                    cut += 1
                    assert out["lengths"][t, w] == limit and not out["flags"][t, w] & ref.SUCCESS
                    assert info["truncated"] is True and info["final_observation"].shape == (3, G * P, G * P)
            else:
                assert out["infos"][t][w] is None and out["lengths"][t, w] == 0 and out["returns"][t, w] == 0
    assert episode.min() >= 5 and cut >= 1
    assert out["vec"].observation_dtype == np.uint8 and out["vec"].action_space_shape == (4,) and out["vec"].max_episode_steps == limit


# the kernel test's cases (tests/test_path_room_gpu.py): the cover condition is one on their action tables, from the rule alone
GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
CASES = [(1, 4, 41), (5, 9, 41), (12, 20, 41), (32, 40, 70)]        # (M, max_steps, steps)


@pytest.mark.parametrize("G, P", GEOMETRIES)
def test_the_kernel_cases_cover_every_branch_at_least_ten_times(G, P):
    total = ref.assert_covered([ref.kernel_case(G, P, 33, M, limit, S)["cover"] for M, limit, S in CASES])
    assert set(total) == set(ref.COVERED)


def test_the_largest_grid_case_has_bit_63_live():
    case = ref.kernel_case(31, 4, 3, 32, 40, 70)
    assert any(pack_moves(episode_draw(e.stream, ep, 31, 32)[1]) >> 63 for e in case["envs"] for ep in range(e.episode + 1))


def test_front_ends_of_the_host_twin():
    cfg = dict(type="PathRoom", grid=3, cell=12, path_moves=3, max_episode_steps=6, seed=7)
    e = create_env(cfg, worker_id=3)
    assert isinstance(e, PathRoomEnv) and e.stream == 10 and e.max_episode_steps == 6
    assert isinstance(create_env(dict(cfg, device=True)), PathRoomEnv)         # (the key means nothing to a single environment)
    serial = make_vec_env(dict(cfg, vectorize="serial", device=False), 3, first_worker_id=2)
    assert isinstance(serial, SerialVecEnv) and [x.stream for x in serial.envs] == [9, 10, 11]
    parts = make_vec_env(dict(cfg, vectorize="serial", device=False), 4, first_worker_id=2, groups=2)
    assert [x.stream for p in parts.parts for x in p.envs] == [9, 10, 11, 12]
    pipe = make_vec_env(cfg, 2, first_worker_id=2)      # the worker processes, through utils.create_env
    try:
        assert isinstance(pipe, PipeVecEnv) and pipe.observation_dtype == np.uint8 and pipe.num_actions == 4
        acts = np.random.default_rng(1).integers(0, 4, size=(12, 2))
        assert np.array_equal(pipe.reset(), serial.reset()[:2])
        two = SerialVecEnv(serial.envs[:2])
        for t in range(12):
            ra, rb = pipe.step(acts[t]), two.step(acts[t])
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
            assert np.array_equal(pipe.action_masks(), two.action_masks())
    finally:
        pipe.close()


# ---------------------------------------------------------------------------------------------------------------- the refusals
BASE = dict(type="PathRoom", grid=7, cell=12, path_moves=16, max_episode_steps=64, seed=0)


def test_section_defaults_and_the_table_row():
    assert path_room_section(dict(type="PathRoom")) == dict(grid=7, cell=12, path_moves=16, max_episode_steps=64, seed=0, device=False)
    assert path_room_section(dict(BASE, device=True, vectorize="serial"))["device"] is True
    assert tuple(DEVICE_ENV_TYPES["PathRoom"]) == ("environments.path_room_env", "path_room_section", "PathRoomEnv", "PathRoomDeviceVecEnv")


@pytest.mark.parametrize("change, match", [
    (dict(colour="red"), r"environment \(PathRoom\): unknown keys \['colour'\] .*; remove them"),
    (dict(command_count=2), "unknown keys"),
    (dict(grid=4), r"environment.grid must be odd and between 3 and 31 .*, got 4: use 5"),
    (dict(grid=1), "odd"),
    (dict(grid=33), r"got 33: use 31"),
    (dict(cell=10), r"environment.cell must be a multiple of 4 between 4 and 64 .*, got 10: use 12"),
    (dict(cell=0), "multiple of 4"),
    (dict(cell=68), "multiple of 4"),
    (dict(grid=3, cell=8), r"a 24 x 24 frame \(grid 3 x cell 8\) is too small for the image encoder .*side of at least 36\): raise grid or cell"),
    (dict(path_moves=0), r"environment.path_moves must be between 1 and 32 \(the path is one 64-bit word, 2 bits per move\), got 0: use 1"),
    (dict(path_moves=33), r"environment.path_moves must be between 1 and 32 .*, got 33: use 32"),
    (dict(max_episode_steps=0), r"environment.max_episode_steps must be at least 1 \(an episode needs a step\), got 0: use 1 or more"),
    (dict(max_episode_steps=-5), "max_episode_steps must be at least 1"),
    (dict(grid=7.0), r"environment.grid \(PathRoom\) must be an integer, got 7.0"),
    (dict(path_moves=True), r"environment.path_moves \(PathRoom\) must be an integer, got True"),
    (dict(max_episode_steps="64"), "integer"),
    (dict(device="yes"), "environment.device must be true or false, got 'yes'"),
    (dict(device=1), "true or false"),
])
def test_refused_sections(change, match):
    with pytest.raises(ValueError, match=match):
        path_room_section(dict(BASE, **change))
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
    with pytest.raises(ValueError, match="path_moves"):      # the section's own refusals come first
        check_device_env_config(dict(environment=dict(BASE, device=True, path_moves=0)))
    # max_episode_steps below memory_length: the existing rule of the window tables
    from trainer import build_window_tables, check_byte_observation_transport
    with pytest.raises(ValueError, match="memory_length"):
        build_window_tables(PathRoomEnv(7, 12, 2, 6).max_episode_steps + 1, PathRoomEnv(7, 12, 2, 6).max_episode_steps)
    # the shared segment of the worker processes types its rows as float32: the type has no float form
    with pytest.raises(ValueError, match="uint8"):
        check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=True))
    check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=False))


def test_config_twins_differ_in_the_device_key_only():
    import os

    from yaml_parser import YamlParser
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "episodic-transformer-memory-ppo_amd", "configs")
    host = YamlParser(os.path.join(here, "path_room.yaml")).get_config()
    dev = YamlParser(os.path.join(here, "path_room_device.yaml")).get_config()
    command = YamlParser(os.path.join(here, "command_room_device.yaml")).get_config()
    hs, ds = path_room_section(host["environment"]), path_room_section(dev["environment"])
    assert not hs["device"] and ds["device"]
    assert ds == dict(grid=7, cell=12, path_moves=16, max_episode_steps=64, seed=0, device=True)
    assert host["environment"]["vectorize"] == dev["environment"]["vectorize"] == "serial"
    dev["environment"]["device"] = host["environment"].get("device", False)
    host["environment"].setdefault("device", False)
    assert host == dev
    assert host["transformer"]["memory_length"] == 32 <= hs["max_episode_steps"]
    # the model is command_room_device.yaml's: everything but the environment and the window
    for cfg in (host, command):
        cfg.pop("environment")
        cfg["transformer"].pop("memory_length")
    assert host == command
