"""Shared by the PathRoom tests: the host rule run over a table of actions that is built step by step against the host twins (the
reference every device result is compared with), a per-cell reconstruction of a frame from (goal, mark, agent) that does not use the
rule's renderer, and the cover condition."""
import functools

import numpy as np

from environments.path_room_env import MOVES, PALETTE, PathRoomEnv
from environments.vec_env import SerialVecEnv

DONE, TRUNCATED, SUCCESS = 1, 2, 4
COVERED = ("success", "fall", "off_grid", "backward", "jump", "cut", "clamped")
COVER_AT_LEAST = 10


def frame_from_cells(G, P, goal, mark, agent):
    """The frame of an observation, cell by cell and pixel by pixel from the stated rule: floor, the goal cell, the mark cell (None:
    the previous step was no fall), the agent cell last.  Cells are (row, column)."""
    floor, goal_colour, mark_colour, agent_colour = (PALETTE[i] for i in range(4))
    out = np.zeros((3, G * P, G * P), dtype=np.uint8)
    for r in range(G):
        for c in range(G):
            colour = floor
            if (r, c) == tuple(goal):
                colour = goal_colour
            if mark is not None and (r, c) == tuple(mark):
                colour = mark_colour
            if (r, c) == tuple(agent):
                colour = agent_colour
            for ch in range(3):
                out[ch, r * P:(r + 1) * P, c * P:(c + 1) * P] = colour[ch]
    return out


def clamp(actions):
    return np.clip(actions, 0, 3)


def classify(env, a):
    """What the (clamped) action ``a`` does to the twin ``env`` before it is taken: "off_grid", "fall", or the index of the path cell
    it moves onto."""
    r, c = env.row + MOVES[a][0], env.col + MOVES[a][1]
    if not (0 <= r < env.grid and 0 <= c < env.grid):
        return "off_grid"
    return env.cells.index((r, c)) if (r, c) in env.cells else "fall"


def run_rule(G, P, M, max_steps, seed, first_worker_id, S, W, table_seed):
    """S steps of a ``SerialVecEnv`` of W host twins over an action table built step by step from ``default_rng(table_seed)``: the
    move from the agent's path cell to the next one is taken 6 times in 8, otherwise a raw value in -1 .. 5.  The host rule takes the
    values clamped to 0 .. 3; ``raw`` [S, W] is what the kernel is given.  -> a dict: raw, frames [S + 1, W, 3, GP, GP] (row 0: the
    reset), rewards [S, W] f32, flags [S, W] u8 (DONE | TRUNCATED | SUCCESS), returns [S, W] f32 and lengths [S, W] i32 of the
    episodes that ended, masks [S + 1, W] u64, infos [S][W], and ``cover``: how often each of ``COVERED`` occurred -- successes, falls,
    moves off the grid (no-ops), moves onto a path cell of a lower index, moves onto a path cell more than one index away (a jump
    across a bend), episodes cut by the time limit, raw values outside 0 .. 3."""
    rng = np.random.default_rng(table_seed)
    envs = [PathRoomEnv(G, P, M, max_steps, seed, worker_id=first_worker_id + w) for w in range(W)]
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
        values, on_path = rng.integers(-1, 6, size=W), rng.integers(0, 8, size=W) < 6
        for w, e in enumerate(envs):
            here = e.cells.index((e.row, e.col))
            if on_path[w] and here < len(e.moves):
                values[w] = e.moves[here]
            raw[t, w] = values[w]
            cover["clamped"] += int(values[w] < 0 or values[w] > 3)
            what = classify(e, int(clamp(values[w])))
            if isinstance(what, str):
                cover[what] += 1
            else:
                cover["backward"] += int(what < here)
                cover["jump"] += int(abs(what - here) > 1)
        _, rewards[t], dones, infos = vec.step(clamp(raw[t]), out=frames[t + 1])
        vec.action_masks(out=masks[t + 1])
        for w, info in enumerate(infos):
            assert (info is not None) == bool(dones[w])
            if info is not None:
                cut = bool(info.get("truncated"))
                assert not (cut and info["success"]) and ("final_observation" in info) == cut
                flags[t, w] = DONE | (TRUNCATED if cut else 0) | (SUCCESS if info["success"] else 0)
                returns[t, w], lengths[t, w] = info["reward"], info["length"]
                cover["cut"] += int(cut)
                cover["success"] += int(info["success"])
        all_infos.append(list(infos))
    return dict(raw=raw, frames=frames, rewards=rewards, flags=flags, returns=returns, lengths=lengths, masks=masks, infos=all_infos,
                cover=cover, envs=envs, vec=vec)


@functools.lru_cache(maxsize=None)
def kernel_case(G, P, W, M, max_steps, S, seed=11, first_worker_id=5):
    """The reference of one case of the kernel test.  Cached: computed once, shared, never modified."""
    ref = run_rule(G, P, M, max_steps, seed, first_worker_id, S, W, table_seed=100000 * G + 1000 * P + 100 * M + max_steps + 7 * W)
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
