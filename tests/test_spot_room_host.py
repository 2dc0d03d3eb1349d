"""SpotRoom's host rule (environments/spot_room_env.py), on a machine without a GPU: the episode draw, the spotlights' triangle
wave, every branch of the step order, rewards, infos and masks, the frame against a per-cell reconstruction, auto-reset through
SerialVecEnv, the cover condition of the kernel test's action tables, the front-ends of the host twin and every refusal."""
import numpy as np
import pytest

import spot_room_reference as ref
from environments import observation_dtype, pack_action_masks
from environments.device_types import DEVICE_ENV_TYPES, check_device_env_config
from environments.spot_room_env import PALETTE, SpotRoomEnv, episode_draw, lit_cells, spot_centre, spot_room_section
from environments.vec_env import PipeVecEnv, SerialVecEnv, make_vec_env
from utils import create_env, process_episode_info

UP, RIGHT, DOWN, LEFT, STAY = 0, 1, 2, 3, 4
TENTH = np.float32(0.1)


# ---------------------------------------------------------------------------------------------------------------- the episode draw
def _mix(z):
    """splitmix64 in numpy's uint64 arithmetic (wraps by itself): the second implementation."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _second_draw(stream, episode, G, N):
    """The draw written a second time, independently: uint64 arrays, and the picks as index bumps over the cells left out (no list
    of cells is built).  -> (start, coin, exit) as row-major indices and the spotlights."""
    with np.errstate(over="ignore"):
        h = _mix(_mix(np.uint64(stream)) + np.uint64(episode))
    field = np.uint64(0xFFFFFF)
    start = int((h >> np.uint64(8)) & field) % (G * G)
    x = _mix(h)
    coin = int((x >> np.uint64(16)) & field) % (G * G - 1)
    coin += coin >= start
    x = _mix(x)
    leave = int((x >> np.uint64(16)) & field) % (G * G - 2)
    for skipped in sorted((start, coin)):
        leave += leave >= skipped
    spots = []
    for _ in range(N):
        x = _mix(x)
        v = int(x)
        spots.append((v >> 16 & 1, (v >> 20 & 0xFFFF) % G, (v >> 40 & 0xFFFF) % (2 * G - 2)))
    return start, coin, leave, tuple(spots)


def _third_draw(stream, episode, G, N):
    """And a third time, in Python integers with the mixer spelled out and the entries counted off cell by cell."""
    m = (1 << 64) - 1

    def mix(x):
        z = (x + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    def entry(k, without):
        for cell in range(G * G):
            if cell in without:
                continue
            if k == 0:
                return cell
            k -= 1
        raise AssertionError("no such entry")
    h = mix((mix(stream & m) + episode) & m)
    start = ((h >> 8) & 0xFFFFFF) % (G * G)
    x = mix(h)
    coin = entry(((x >> 16) & 0xFFFFFF) % (G * G - 1), {start})
    x = mix(x)
    leave = entry(((x >> 16) & 0xFFFFFF) % (G * G - 2), {start, coin})
    spots = []
    for _ in range(N):
        x = mix(x)
        spots.append(((x >> 16) & 1, ((x >> 20) & 0xFFFF) % G, ((x >> 40) & 0xFFFF) % (2 * G - 2)))
    return start, coin, leave, tuple(spots)


def _indices(draw, G):
    start, coin, leave, spots = draw
    return start[0] * G + start[1], coin[0] * G + coin[1], leave[0] * G + leave[1], spots


def test_episode_draw_equals_two_independent_re_derivations_and_keeps_its_promises():
    rng = np.random.default_rng(0)
    axes, lanes, phases = set(), set(), set()
    for i in range(1500):
        stream, episode = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 40))
        G, N = int(rng.choice([3, 5, 7, 9, 31])), int(rng.integers(0, 5))
        draw = episode_draw(stream, episode, G, N)
        start, coin, leave, spots = draw
        assert _indices(draw, G) == _second_draw(stream, episode, G, N)
        if i < 60:
            assert _indices(draw, G) == _third_draw(stream, episode, G, N)
        assert len({start, coin, leave}) == 3 and all(0 <= r < G and 0 <= c < G for r, c in (start, coin, leave))
        assert len(spots) == N
        for axis, lane, phase in spots:
            assert axis in (0, 1) and 0 <= lane < G and 0 <= phase < 2 * G - 2
            if G == 31:
                axes.add(axis), lanes.add(lane), phases.add(phase)
    # at the largest grid lane bit 4 and phase bit 5 are live
    assert axes == {0, 1} and max(lanes) >= 16 and max(phases) >= 32
    # fewer spotlights are a prefix of more, and the cells do not depend on N
    assert episode_draw(7, 3, 9, 2) == episode_draw(7, 3, 9, 4)[:3] + (episode_draw(7, 3, 9, 4)[3][:2],)
    # the stream is taken mod 2^64, and seed + worker_id is the stream
    assert episode_draw((1 << 64) + 3, 2, 5, 2) == episode_draw(3, 2, 5, 2)
    a, b = SpotRoomEnv(7, 12, seed=3, worker_id=4), SpotRoomEnv(7, 12, seed=0, worker_id=7)
    for _ in range(4):
        assert np.array_equal(a.reset(), b.reset()) and (a.coin, a.exit, a.spots) == (b.coin, b.exit, b.spots)


def test_every_cell_is_drawn_for_every_role():
    G = 3
    seen = [set(), set(), set()]
    for episode in range(400):
        for k, cell in enumerate(episode_draw(1, episode, G, 0)[:3]):
            seen[k].add(cell)
    assert all(len(s) == G * G for s in seen)


# ---------------------------------------------------------------------------------------------------------------- the spotlights
@pytest.mark.parametrize("G, light, period", [(3, 1, 1), (5, 2, 3), (7, 3, 2), (31, 1, 2)])
def test_spotlight_position_is_a_triangle_wave(G, light, period):
    wave = list(range(G)) + list(range(G - 2, 0, -1))            # 0 .. G - 1 and back to 1: 2 G - 2 positions
    assert len(wave) == 2 * G - 2
    for axis in (0, 1):
        for lane in (0, G // 2, G - 1):
            for phase in (0, 1, G - 1, G, 2 * G - 3):
                previous = None
                for t in range(light, light + 3 * period * len(wave)):
                    moved = (t - light) // period                # it rests ``period`` observations on a cell
                    pos = wave[(phase + moved) % len(wave)]
                    centre = spot_centre((axis, lane, phase), t, G, light, period)
                    assert centre == ((lane, pos) if axis == 0 else (pos, lane))
                    if previous is not None:
                        step = abs(pos - previous)
                        assert step == (1 if (t - light) % period == 0 else 0)
                    previous = pos
    # the lit cells: the 3 x 3 block around the centre, clipped to the grid; nothing before light_steps
    spot = (0, 0, 0)
    assert not lit_cells((spot,), light - 1, G, light, period).any()
    lit = lit_cells((spot,), light, G, light, period)            # the centre is (0, 0): a 2 x 2 block is left
    assert lit.sum() == 4 and lit[:2, :2].all()
    lit = lit_cells(((1, G // 2, G // 2), (0, 0, 0)), light, G, light, period)
    middle = G // 2
    assert lit[middle - 1:middle + 2, middle - 1:middle + 2].all() and lit.sum() == {3: 9, 5: 12}.get(G, 13)      # (the blocks overlap in one cell at G = 5)


# ---------------------------------------------------------------------------------------------------------------- the rule
class _Fixed(SpotRoomEnv):
    """A twin whose layout is given, not drawn: the rule on a layout worked out by hand."""

    def __init__(self, start, coin, leave, spots, grid=5, cell=8, **keys):
        super().__init__(grid, cell, spotlights=len(spots), **keys)
        self._fixed = (start, coin, leave, tuple(spots))

    def reset(self, **kwargs):
        super().reset()
        (self.row, self.col), self.coin, self.exit, self.spots = self._fixed
        return self._obs()


def _f32(k):
    return float(np.float32(k) * TENTH)


def _frame(e, light, centres, coin, agent):
    return ref.frame_from_cells(e.grid, e.cell, light, centres, coin, e.exit, agent)


def test_every_branch_of_the_step_order():
    # G = 5, light_steps 2, period 1; one spotlight on row 0 (axis 0, lane 0) with phase 0: at t >= 2 its centre is (0, t - 2) on the
    # way out, so at t = 2 it lights rows 0 .. 1 x columns 0 .. 1, at t = 3 columns 0 .. 2, at t = 4 columns 1 .. 3, ...
    e = _Fixed((1, 1), (1, 2), (3, 2), [(0, 0, 0)], light_steps=2, spot_period=1, health=3, max_episode_steps=64)
    coin = (1, 2)
    obs = e.reset()
    assert np.array_equal(obs, _frame(e, True, [], coin, (1, 1)))
    # t = 0 -> 1, still light: a move off the grid is a no-op ... from (1, 1) up to (0, 1), then up again
    obs, r, d, info = e.step(UP)
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.t, e.health) == (0, 1, 1, 3)
    assert np.array_equal(obs, _frame(e, True, [], coin, (0, 1)))
    # t = 1 -> 2: off the grid; observation 2 is the first dark one, the centre is (0, 0) and (0, 1) is lit: damage, the agent is drawn
    obs, r, d, info = e.step(UP)
    assert (r, d, info) == (_f32(-1), False, None) and (e.row, e.col, e.health) == (0, 1, 2)
    assert np.array_equal(obs, _frame(e, False, [(0, 0)], coin, (0, 1)))
    assert (obs[:, 4, 12] == PALETTE[4]).all() and (obs[:, 20, 4] == PALETTE[0]).all() and (obs[:, 4, 4] == PALETTE[1]).all()
    # t = 2 -> 3: down to (1, 1), then right onto the coin at (1, 2) at t = 4: the centre is (0, 2) then, the coin cell is lit --
    # coin and damage in ONE step, +5 - 1, and the last health point: dead with the coin, 5 - 3 tenths
    obs, r, d, info = e.step(DOWN)
    assert (r, d, info) == (_f32(-1), False, None) and e.health == 1            # (centre (0, 1): (1, 1) is lit)
    obs, r, d, info = e.step(RIGHT)
    assert np.float32(r) == np.float32(4) * TENTH and d and info == {"reward": _f32(2), "length": 4, "success": 0}


def test_coin_and_damage_in_one_step():
    # the spotlight rests on column 2 of row 0 (period 100, phase 2): (1, 2) is lit from observation 1 on
    e = _Fixed((1, 1), (1, 2), (3, 2), [(0, 0, 2)], light_steps=1, spot_period=100, health=3)
    e.reset()
    obs, r, d, info = e.step(RIGHT)
    assert np.float32(r) == np.float32(4) * TENTH and (d, info) == (False, None) and e.coin_taken and e.health == 2
    assert np.array_equal(obs, _frame(e, False, [(0, 2)], None, (1, 2)))       # the coin is gone, the agent is seen
    # STAY on a lit cell costs health again; the coin pays once
    obs, r, d, info = e.step(STAY)
    assert (r, d, info) == (_f32(-1), False, None) and e.health == 1
    # leaving the light: the agent is no longer drawn, the step is free
    obs, r, d, info = e.step(DOWN)
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col, e.health) == (2, 2, 1)
    assert np.array_equal(obs, _frame(e, False, [(0, 2)], None, (2, 2)))
    assert not (obs == PALETTE[4][:, None, None]).all(axis=0).any()
    # on to the exit with the coin: +10, success, the info sums 5 + 10 - 2
    t = e.t
    obs, r, d, info = e.step(DOWN)
    assert np.float32(r) == np.float32(10) * TENTH and d
    assert info == {"reward": float(np.float32(13) * TENTH), "length": t + 1, "success": 1}
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(5)
    with pytest.raises(ValueError, match="outside Discrete"):
        e.step(-1)
    with pytest.raises(RuntimeError, match="before reset"):
        SpotRoomEnv(5, 8).step(0)


def test_exit_with_the_coin_on_a_lit_cell_ends_with_no_damage():
    # the exit (1, 2) is lit all the time; the coin (1, 1) is lit too
    e = _Fixed((1, 0), (1, 1), (1, 2), [(0, 0, 2)], light_steps=1, spot_period=100, health=2)
    e.reset()
    assert e.step(RIGHT)[1:] == (_f32(4), False, None) and e.health == 1       # coin and damage
    obs, r, d, info = e.step(RIGHT)
    assert np.float32(r) == np.float32(10) * TENTH and d and e.health == 1      # no damage in the step that leaves
    assert info == {"reward": float(np.float32(14) * TENTH), "length": 2, "success": 1}
    # with health 1 the coin step is death already, and the coin still counts: 5 - 1
    e = _Fixed((1, 0), (1, 1), (1, 2), [(0, 0, 2)], light_steps=1, spot_period=100, health=1)
    e.reset()
    obs, r, d, info = e.step(RIGHT)
    assert np.float32(r) == np.float32(4) * TENTH and d and info == {"reward": _f32(4), "length": 1, "success": 0}


def test_the_exit_without_the_coin_does_nothing():
    e = _Fixed((2, 0), (0, 4), (2, 1), [], light_steps=1, spot_period=1, health=1, max_episode_steps=5)
    e.reset()
    obs, r, d, info = e.step(RIGHT)                                          # onto the exit, the coin not taken
    assert (r, d, info) == (0.0, False, None) and (e.row, e.col) == (2, 1)
    # no spotlight: all dark, the agent is not drawn, the exit is (the agent stands on it, unseen)
    assert np.array_equal(obs, _frame(e, False, [], (0, 4), (2, 1)))
    assert (obs[:, 20, 12] == PALETTE[3]).all()
    assert e.step(STAY)[1:] == (0.0, False, None)
    assert e.step(LEFT)[1:] == (0.0, False, None) and e.step(LEFT)[1:] == (0.0, False, None)      # the second one off the grid
    obs, r, d, info = e.step(RIGHT)                                          # the time limit, on the exit without the coin
    assert r == 0.0 and d and info == {"reward": 0.0, "length": 5, "success": 0, "truncated": True}


def test_death_and_the_time_limit_on_one_step_is_death():
    # the agent stays under a resting spotlight: health 3 and max_episode_steps 3 run out in the same step
    e = _Fixed((0, 0), (4, 4), (4, 0), [(0, 0, 0)], light_steps=1, spot_period=100, health=3, max_episode_steps=3)
    e.reset()
    assert e.step(STAY)[1:] == (_f32(-1), False, None) and e.step(UP)[1:] == (_f32(-1), False, None)
    obs, r, d, info = e.step(STAY)
    assert np.float32(r) == -TENTH and d and info == {"reward": _f32(-3), "length": 3, "success": 0}      # dead, not truncated
    # with one health point more it is the time limit, and the lost health is in the return
    e = _Fixed((0, 0), (4, 4), (4, 0), [(0, 0, 0)], light_steps=1, spot_period=100, health=4, max_episode_steps=3)
    e.reset()
    e.step(STAY), e.step(STAY)
    assert e.step(STAY)[3] == {"reward": _f32(-3), "length": 3, "success": 0, "truncated": True}
    # success in the last step is no cut either
    e = _Fixed((1, 0), (1, 1), (1, 2), [], light_steps=1, spot_period=1, health=1, max_episode_steps=2)
    e.reset()
    e.step(RIGHT)
    assert e.step(RIGHT)[3] == {"reward": float(np.float32(15) * TENTH), "length": 2, "success": 1}
    e = _Fixed((1, 0), (1, 1), (1, 2), [], light_steps=1, spot_period=1, health=1, max_episode_steps=1)
    e.reset()
    assert e.step(UP)[3] == {"reward": 0.0, "length": 1, "success": 0, "truncated": True}


def test_stay_on_a_cell_that_becomes_lit():
    # a spotlight walks along row 2 (axis 0, lane 2, phase 0, one cell every 2 observations from observation 1 on): its centre is
    # (2, 0) at t = 1, 2, (2, 1) at t = 3, 4, (2, 2) at t = 5, 6; the agent waits on (2, 3), lit once the centre is (2, 2)
    e = _Fixed((2, 3), (0, 0), (4, 4), [(0, 2, 0)], light_steps=1, spot_period=2, health=2)
    obs = e.reset()
    for t in range(1, 5):
        obs, r, d, info = e.step(STAY)
        assert (r, d, info) == (0.0, False, None) and e.t == t
        assert np.array_equal(obs, _frame(e, False, [(2, (t - 1) // 2)], (0, 0), (2, 3)))
        assert not (obs == PALETTE[4][:, None, None]).all(axis=0).any()                          # in the dark, unseen
    obs, r, d, info = e.step(STAY)
    assert (r, d, info) == (_f32(-1), False, None) and e.health == 1
    assert np.array_equal(obs, _frame(e, False, [(2, 2)], (0, 0), (2, 3)))
    assert (obs[:, 20, 28] == PALETTE[4]).all()                                                  # seen, and it cost health
    obs, r, d, info = e.step(STAY)
    assert np.float32(r) == -TENTH and d and info == {"reward": _f32(-2), "length": 6, "success": 0}      # both points lost


def test_info_arithmetic_is_one_float32_multiply():
    # float32(k) * float32(0.1), widened to a Python float: not the float64 product
    assert float(np.float32(7) * TENTH) == 0.699999988079071 != 0.7 and float(np.float32(-3) * TENTH) == -0.30000001192092896
    res = process_episode_info([{"reward": 1.4, "length": 4, "success": 1}, {"reward": -0.2, "length": 64, "success": 0}])
    assert res["success_percent"] == 0.5


@pytest.mark.parametrize("G, P, N, light, period, health, limit", [
    (3, 12, 0, 1, 1, 1, 6), (5, 8, 1, 2, 1, 2, 9), (7, 12, 2, 2, 2, 5, 64), (9, 4, 4, 3, 3, 15, 40), (31, 4, 4, 3, 3, 15, 40)])
def test_drawn_episodes_masks_frames_rewards_and_the_agent_is_drawn_exactly_when_damaged(G, P, N, light, period, health, limit):
    e = SpotRoomEnv(G, P, N, light, period, health, limit, seed=4, worker_id=1)
    assert e.max_episode_steps == limit and e.action_space.n == 5 and observation_dtype(e.observation_space) == np.uint8
    assert e.observation_space.shape == (3, G * P, G * P)
    rng = np.random.default_rng(G + N)
    agent_colour = PALETTE[4][:, None, None]
    outcomes = set()
    for episode in range(8):
        obs = e.reset()
        start, coin, leave, spots = episode_draw(5, episode, G, N)
        assert ((e.row, e.col), e.coin, e.exit, e.spots) == (start, coin, leave, spots)
        lost = taken = 0
        for t in range(limit):
            assert obs.dtype == np.uint8 and np.array_equal(obs, ref.frame_of(e))
            row, col = e.row, e.col
            assert list(e.action_masks()) == [row > 0, col < G - 1, row < G - 1, col > 0, True] and e.action_masks().sum() >= 3
            a = ref.toward(e, bool(rng.integers(0, 2))) if episode % 2 == 0 or rng.integers(0, 4) else int(rng.integers(0, 5))
            obs, r, d, info = e.step(a)
            k = int(round(r * 10))
            took = int(e.coin_taken) - taken
            taken += took
            success = int(d and info["success"])
            hurt = 5 * took + 10 * success - k
            assert hurt in (0, 1) and np.float32(r) == np.float32(k) * TENTH
            lost += hurt
            if not d:
                # in the dark the agent is drawn exactly on the frames that cost health
                drawn = bool((obs == agent_colour).all(axis=0).any())
                assert drawn == (e.t < light or hurt == 1) and e.health == health - lost
            if d:
                want = {"reward": float(np.float32(5 * taken + 10 * success - lost) * TENTH), "length": t + 1, "success": success}
                if not success and lost < health:
                    assert t + 1 == limit
                    want["truncated"] = True
                assert info == want
                outcomes.add("success" if success else ("death" if lost == health else "cut"))
                break
            assert info is None
        else:
            raise AssertionError("the episode outlived max_episode_steps")
    assert "success" in outcomes or G == 31


def test_frame_colours():
    colours = [tuple(int(v) for v in p) for p in PALETTE]
    assert colours == [(12, 12, 20), (96, 92, 72), (248, 208, 40), (56, 176, 112), (224, 64, 200)]
    # pairwise distinct in every channel and in the channel sum: a wrong colour cannot hide
    for values in list(zip(*colours)) + [tuple(sum(c) for c in colours)]:
        assert len(set(values)) == 5
    f = ref.frame_from_cells(3, 12, False, [(0, 0)], (0, 2), (2, 2), (1, 1))
    assert (f[:, 6, 30] == PALETTE[2]).all() and (f[:, 30, 30] == PALETTE[3]).all() and (f[:, 18, 18] == PALETTE[4]).all()
    assert (f[:, 6, 6] == PALETTE[1]).all() and (f[:, 30, 6] == PALETTE[0]).all()
    assert (ref.frame_from_cells(3, 12, False, [(0, 0)], (0, 2), (2, 2), (2, 0))[:, 30, 6] == PALETTE[0]).all()      # unlit: not drawn
    assert (ref.frame_from_cells(3, 12, True, [], (0, 2), (2, 2), (2, 2))[:, 30, 30] == PALETTE[4]).all()            # the agent last
    e = SpotRoomEnv(3, 12, 1, 2, 1, 2, 6, seed=2)
    obs = e.reset()
    counts = [int((obs == np.asarray(c, dtype=np.uint8)[:, None, None]).all(axis=0).sum()) for c in colours]
    assert counts == [0, 6 * 144, 144, 144, 144]                             # the first frame: everything lit, everything drawn


def test_auto_reset_through_serial_vec_env():
    G, P, W, S = 3, 12, 4, 80
    out = ref.run_rule(G, P, 1, 1, 1, 2, 6, seed=3, first_worker_id=0, S=S, W=W, table_seed=5)
    assert out["raw"].min() == -1 and out["raw"].max() == 6
    episode = np.zeros(W, dtype=int)
    cut = 0
    for t in range(S):
        for w in range(W):
            if out["flags"][t, w] & ref.DONE:
                # the returned row of a finished worker is the first frame of its next episode; the words are that frame's
                episode[w] += 1
                start, coin, leave, spots = episode_draw(3 + w, episode[w], G, 1)
                assert np.array_equal(out["frames"][t + 1, w], ref.frame_from_cells(G, P, True, [], coin, leave, start))
                row, col = start
                want = pack_action_masks(np.array([[row > 0, col < G - 1, row < G - 1, col > 0, True]]))[0]
                assert out["masks"][t + 1, w] == want
                assert 1 <= out["lengths"][t, w] <= 6
                info = out["infos"][t][w]
                if out["flags"][t, w] & ref.TRUNCATED:
                    cut += 1
                    assert out["lengths"][t, w] == 6 and not out["flags"][t, w] & ref.SUCCESS
                    assert info["truncated"] is True and info["final_observation"].shape == (3, G * P, G * P)
            else:
                assert out["infos"][t][w] is None and out["lengths"][t, w] == 0 and out["returns"][t, w] == 0
    assert episode.min() >= 5 and cut >= 1
    assert out["vec"].observation_dtype == np.uint8 and out["vec"].action_space_shape == (5,) and out["vec"].max_episode_steps == 6


# the kernel test's cases (tests/test_spot_room_gpu.py): the cover condition is one on their action tables, from the rule alone
GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
CASES = [(0, 1, 1, 1, 6, 41), (1, 2, 1, 2, 9, 41), (2, 1, 2, 3, 20, 41), (4, 3, 3, 15, 40, 70)]      # (N, light, period, health, max_steps, steps)


@pytest.mark.parametrize("G, P", GEOMETRIES)
def test_the_kernel_cases_cover_every_branch_at_least_ten_times(G, P):
    total = ref.assert_covered([ref.kernel_case(G, P, 33, *case)["cover"] for case in CASES])
    assert set(total) == set(ref.COVERED)
    print(f"cover at grid {G}, cell {P}: {total}")


def test_the_largest_grid_case_has_lane_bit_4_and_phase_bit_5_live():
    case = ref.kernel_case(31, 4, 3, 4, 3, 3, 15, 40, 70)
    spots = [s for e in case["envs"] for ep in range(e.episode + 1) for s in episode_draw(e.stream, ep, 31, 4)[3]]
    assert any(lane >= 16 for _, lane, _ in spots) and any(phase >= 32 for _, _, phase in spots)


def test_front_end_test_actions_end_episodes_both_ways():
    # the chooser of the GPU front-end test, run on the host twins alone: it must see successes and other endings
    cfg = dict(type="SpotRoom", grid=3, cell=12, spotlights=1, light_steps=1, spot_period=1, health=2, max_episode_steps=6, seed=21)
    host = make_vec_env(dict(cfg, vectorize="serial", device=False), 5, first_worker_id=4)
    host.reset()
    choose = ref.front_end_chooser(5)
    ended = succeeded = 0
    for t in range(30):
        _, _, dones, infos = host.step(choose(t, host))
        ended += int(dones.sum())
        succeeded += sum(i["success"] for i in infos if i)
    assert ended >= 5 and 0 < succeeded < ended


def test_front_ends_of_the_host_twin():
    cfg = dict(type="SpotRoom", grid=3, cell=12, spotlights=1, light_steps=1, spot_period=1, health=2, max_episode_steps=6, seed=7)
    e = create_env(cfg, worker_id=3)
    assert isinstance(e, SpotRoomEnv) and e.stream == 10 and e.max_episode_steps == 6
    assert isinstance(create_env(dict(cfg, device=True)), SpotRoomEnv)         # (the key means nothing to a single environment)
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
BASE = dict(type="SpotRoom", grid=7, cell=12, spotlights=2, light_steps=2, spot_period=2, health=5, max_episode_steps=64, seed=0)


def test_section_defaults_and_the_table_row():
    assert spot_room_section(dict(type="SpotRoom")) == dict(grid=7, cell=12, spotlights=2, light_steps=2, spot_period=2, health=5,
                                                            max_episode_steps=64, seed=0, device=False)
    assert spot_room_section(dict(BASE, device=True, vectorize="serial"))["device"] is True
    assert spot_room_section(dict(BASE, spotlights=0, health=15))["spotlights"] == 0
    assert tuple(DEVICE_ENV_TYPES["SpotRoom"]) == ("environments.spot_room_env", "spot_room_section", "SpotRoomEnv", "SpotRoomDeviceVecEnv")


@pytest.mark.parametrize("change, match", [
    (dict(colour="red"), r"environment \(SpotRoom\): unknown keys \['colour'\] .*; remove them"),
    (dict(path_moves=2), "unknown keys"),
    (dict(grid=4), r"environment.grid must be odd and between 3 and 31 .*, got 4: use 5"),
    (dict(grid=1), "odd"),
    (dict(grid=33), r"got 33: use 31"),
    (dict(cell=10), r"environment.cell must be a multiple of 4 between 4 and 64 .*, got 10: use 12"),
    (dict(cell=0), "multiple of 4"),
    (dict(cell=68), "multiple of 4"),
    (dict(grid=3, cell=8), r"a 24 x 24 frame \(grid 3 x cell 8\) is too small for the image encoder .*side of at least 36\): raise grid or cell"),
    (dict(spotlights=-1), r"environment.spotlights must be between 0 and 4 \(a frame word is tested against at most four boxes\), got -1: use 0"),
    (dict(spotlights=5), r"environment.spotlights must be between 0 and 4 .*, got 5: use 4"),
    (dict(light_steps=0), r"environment.light_steps must be at least 1 \(the first observation shows the room\), got 0: use 1 or more"),
    (dict(light_steps=-2), "light_steps must be at least 1"),
    (dict(spot_period=0), r"environment.spot_period must be at least 1 \(the steps a spotlight rests on a cell\), got 0: use 1 or more"),
    (dict(spot_period=-1), "spot_period must be at least 1"),
    (dict(health=0), r"environment.health must be between 1 and 15 \(four bits of the state\), got 0: use 1"),
    (dict(health=16), r"environment.health must be between 1 and 15 .*, got 16: use 15"),
    (dict(max_episode_steps=0), r"environment.max_episode_steps must be at least 1 \(an episode needs a step\), got 0: use 1 or more"),
    (dict(max_episode_steps=-5), "max_episode_steps must be at least 1"),
    (dict(grid=7.0), r"environment.grid \(SpotRoom\) must be an integer, got 7.0"),
    (dict(spotlights=True), r"environment.spotlights \(SpotRoom\) must be an integer, got True"),
    (dict(health="5"), "integer"),
    (dict(spot_period=2.0), "integer"),
    (dict(device="yes"), "environment.device must be true or false, got 'yes'"),
    (dict(device=1), "true or false"),
])
def test_refused_sections(change, match):
    with pytest.raises(ValueError, match=match):
        spot_room_section(dict(BASE, **change))
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
    with pytest.raises(ValueError, match="spotlights"):      # the section's own refusals come first
        check_device_env_config(dict(environment=dict(BASE, device=True, spotlights=9)))
    # max_episode_steps below memory_length: the existing rule of the window tables
    from trainer import build_window_tables, check_byte_observation_transport
    limit = SpotRoomEnv(7, 12, max_episode_steps=6).max_episode_steps
    with pytest.raises(ValueError, match="memory_length"):
        build_window_tables(limit + 1, limit)
    # the shared segment of the worker processes types its rows as float32: the type has no float form
    with pytest.raises(ValueError, match="uint8"):
        check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=True))
    check_byte_observation_transport(dict(environment=dict(BASE), worker_processes=False))


def test_config_twins_differ_in_the_device_key_only():
    import os

    from yaml_parser import YamlParser
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "episodic-transformer-memory-ppo_amd", "configs")
    host = YamlParser(os.path.join(here, "spot_room.yaml")).get_config()
    dev = YamlParser(os.path.join(here, "spot_room_device.yaml")).get_config()
    path = YamlParser(os.path.join(here, "path_room_device.yaml")).get_config()
    hs, ds = spot_room_section(host["environment"]), spot_room_section(dev["environment"])
    assert not hs["device"] and ds["device"]
    assert ds == dict(grid=7, cell=12, spotlights=2, light_steps=2, spot_period=2, health=5, max_episode_steps=64, seed=0, device=True)
    assert host["environment"]["vectorize"] == dev["environment"]["vectorize"] == "serial"
    dev["environment"]["device"] = host["environment"].get("device", False)
    host["environment"].setdefault("device", False)
    assert host == dev
    assert host["transformer"]["memory_length"] == 32 <= hs["max_episode_steps"] and host["previous_step_input"] is True
    # the model is path_room_device.yaml's: everything but the environment and the previous step as input
    host.pop("environment"), path.pop("environment")
    assert host.pop("previous_step_input") is True and "previous_step_input" not in path
    assert host == path
