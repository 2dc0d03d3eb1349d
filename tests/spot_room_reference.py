"""Shared by the SpotRoom tests: the host rule run over a table of actions that is built step by step against the host twins (the
reference every device result is compared with), a per-cell reconstruction of a frame from (centres, coin, exit, agent) that does not
use the rule's renderer, and the cover condition."""
import functools

import numpy as np

from environments.spot_room_env import MOVES, PALETTE, SpotRoomEnv, spot_centre
from environments.vec_env import SerialVecEnv

DONE, TRUNCATED, SUCCESS = 1, 2, 4
COVERED = ("success", "coin", "death", "cut", "damage", "off_grid", "stay", "early_exit", "clamped")
COVER_AT_LEAST = 10


def frame_from_cells(G, P, light, centres, coin, leave, agent):
    """The frame of an observation, cell by cell and pixel by pixel from the stated rule.  ``light``: the observation index is below
    light_steps (all floor lit, the agent drawn); ``centres``: the (row, column) centres of the spotlights at this observation;
    ``coin``: (row, column) or None (taken); the exit and the agent are cells.  Floor dark, lit within one cell of a centre; then the
    coin, the exit, and the agent last -- where it is lit."""
    dark, lit, coin_colour, exit_colour, agent_colour = (PALETTE[i] for i in range(5))

    def is_lit(r, c):
        return light or any(abs(r - cr) <= 1 and abs(c - cc) <= 1 for cr, cc in centres)
    out = np.zeros((3, G * P, G * P), dtype=np.uint8)
    for r in range(G):
        for c in range(G):
            colour = lit if is_lit(r, c) else dark
            if coin is not None and (r, c) == tuple(coin):
                colour = coin_colour
            if (r, c) == tuple(leave):
                colour = exit_colour
            if (r, c) == tuple(agent) and is_lit(r, c):
                colour = agent_colour
            for ch in range(3):
                out[ch, r * P:(r + 1) * P, c * P:(c + 1) * P] = colour[ch]
    return out


def frame_of(env):
    """``frame_from_cells`` of the twin's current observation."""
    light = env.t < env.light_steps
    centres = [] if light else [spot_centre(s, env.t, env.grid, env.light_steps, env.spot_period) for s in env.spots]
    return frame_from_cells(env.grid, env.cell, light, centres, None if env.coin_taken else env.coin, env.exit, (env.row, env.col))


def clamp(actions):
    return np.clip(actions, 0, 4)


def toward(env, row_first):
    """The move that brings the twin ``env`` nearer its target -- the coin, or the exit once the coin is taken --, along the rows
    first or along the columns first.  (The agent never stands on its target: the coin is taken and the exit ends the episode.)"""
    tr, tc = env.exit if env.coin_taken else env.coin
    vertical = 0 if tr < env.row else (2 if tr > env.row else None)
    horizontal = 3 if tc < env.col else (1 if tc > env.col else None)
    first, second = (vertical, horizontal) if row_first else (horizontal, vertical)
    return first if first is not None else second


def run_rule(G, P, N, light, period, health, max_steps, seed, first_worker_id, S, W, table_seed):
    """S steps of a ``SerialVecEnv`` of W host twins over an action table built step by step from ``default_rng(table_seed)``: the
    move toward the coin -- toward the exit once the coin is taken -- is taken 6 times in 8, otherwise a raw value in -1 .. 6.  The
    host rule takes the values clamped to 0 .. 4; ``raw`` [S, W] is what the kernel is given.  -> a dict: raw, frames
    [S + 1, W, 3, GP, GP] (row 0: the reset), rewards [S, W] f32, flags [S, W] u8 (DONE | TRUNCATED | SUCCESS), returns [S, W] f32 and
    lengths [S, W] i32 of the episodes that ended, masks [S + 1, W] u64, infos [S][W], and ``cover``: how often each of ``COVERED``
    occurred -- successes, coins taken, deaths, episodes cut by the time limit, steps that cost health, moves off the grid (no-ops),
    stays, exits entered without the coin, raw values outside 0 .. 4."""
    rng = np.random.default_rng(table_seed)
    envs = [SpotRoomEnv(G, P, N, light, period, health, max_steps, seed, worker_id=first_worker_id + w) for w in range(W)]
    vec = SerialVecEnv(envs)
    side = G * P
    raw = np.zeros((S, W), dtype=np.int64)
    frames = np.zeros((S + 1, W, 3, side, side), dtype=np.uint8)
    rewards, flags = np.zeros((S, W), dtype=np.float32), np.zeros((S, W), dtype=np.uint8)
    returns, lengths = np.zeros((S, W), dtype=np.float32), np.zeros((S, W), dtype=np.int32)
    masks = np.zeros((S + 1, W), dtype=np.uint64)
    cover = dict.fromkeys(COVERED, 0)
    all_infos = []
    vec.reset(out=frames[0])
    vec.action_masks(out=masks[0])
    for t in range(S):
        values, aimed, row_first = rng.integers(-1, 7, size=W), rng.integers(0, 8, size=W) < 6, rng.integers(0, 2, size=W)
        before = []
        for w, e in enumerate(envs):
            if aimed[w]:
                values[w] = toward(e, bool(row_first[w]))
            raw[t, w] = values[w]
            a = int(clamp(values[w]))
            r, c = e.row + MOVES[a][0], e.col + MOVES[a][1]
            on_grid = 0 <= r < G and 0 <= c < G
            cover["clamped"] += int(values[w] < 0 or values[w] > 4)
            cover["stay"] += int(a == 4)
            cover["off_grid"] += int(not on_grid)
            cover["early_exit"] += int(on_grid and a != 4 and (r, c) == e.exit and not e.coin_taken and (r, c) != e.coin)
            before.append((e.episode, e.health, e.coin_taken))
        _, rewards[t], dones, infos = vec.step(clamp(raw[t]), out=frames[t + 1])
        vec.action_masks(out=masks[t + 1])
        for w, info in enumerate(infos):
            assert (info is not None) == bool(dones[w])
            e = envs[w]
            tenths = int(round(float(rewards[t, w]) * 10))
            # what the step did, from its reward alone: +5 the coin, +10 the exit, -1 a lit observation (no two sums coincide)
            took, left, hurt = {0: (0, 0, 0), 5: (1, 0, 0), 10: (0, 1, 0), 15: (1, 1, 0), -1: (0, 0, 1), 4: (1, 0, 1)}[tenths]
            cover["coin"] += took
            cover["damage"] += hurt
            if info is not None:
                cut = bool(info.get("truncated"))
                assert not (cut and info["success"]) and ("final_observation" in info) == cut and left == info["success"]
                flags[t, w] = DONE | (TRUNCATED if cut else 0) | (SUCCESS if info["success"] else 0)
                returns[t, w], lengths[t, w] = info["reward"], info["length"]
                cover["cut"] += int(cut)
                cover["success"] += int(info["success"])
                cover["death"] += int(not cut and not info["success"])
            else:
                assert not left and e.episode == before[w][0] and e.health == before[w][1] - hurt
        all_infos.append(list(infos))
    return dict(raw=raw, frames=frames, rewards=rewards, flags=flags, returns=returns, lengths=lengths, masks=masks, infos=all_infos,
                cover=cover, envs=envs, vec=vec)


@functools.lru_cache(maxsize=None)
def kernel_case(G, P, W, N, light, period, health, max_steps, S, seed=11, first_worker_id=5):
    """The reference of one case of the kernel test.  Cached: computed once, shared, never modified."""
    table_seed = 100000 * G + 1000 * P + 100 * N + 10 * health + max_steps + 7 * W
    ref = run_rule(G, P, N, light, period, health, max_steps, seed, first_worker_id, S, W, table_seed=table_seed)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def assert_covered(covers):
    """``covers``: the cover counts of several cases; summed, each of ``COVERED`` occurs at least ``COVER_AT_LEAST`` times."""
    total = {what: sum(c[what] for c in covers) for what in COVERED}
    for what in COVERED:
        assert total[what] >= COVER_AT_LEAST, f"the action tables produced too few of: {what} ({total})"
    return total


def front_end_chooser(W, seed=8):
    """``choose(t, host)`` for the front-end test: the move toward the target three times in four, else any of the five actions, so
    that episodes end every way."""
    rng = np.random.default_rng(seed)

    def choose(t, host):
        acts = rng.integers(0, 5, size=W).astype(np.int64)
        for w, e in enumerate(host.envs):
            if rng.integers(0, 4) != 0:
                acts[w] = toward(e, bool(rng.integers(0, 2)))
        return acts
    return choose
