"""Shared by the CueRoom tests: the host rule run over a table of actions (the reference every device result is compared with), a
per-cell reconstruction of a frame from (position, target, step) that does not use the rule's renderer, and the cover condition --
target hits, wrong corners, time-limit cuts and off-grid moves each occurred."""
import functools

import numpy as np

from environments.cue_room_env import CueRoomEnv, PALETTE, corner_cells
from environments.vec_env import SerialVecEnv

DONE, TRUNCATED, SUCCESS = 1, 2, 4


def frame_from_cells(G, P, row, col, target, step, cue_steps):
    """The frame of a state, cell by cell and pixel by pixel from the stated rule (floor; the four corners goals; the target in the
    cue colour while step < cue_steps; the agent last)."""
    floor, goal, cue, agent = (PALETTE[i] for i in range(4))
    out = np.zeros((3, G * P, G * P), dtype=np.uint8)
    for r in range(G):
        for c in range(G):
            colour = floor
            if (r, c) in corner_cells(G):
                colour = cue if step < cue_steps and corner_cells(G).index((r, c)) == target else goal
            if (r, c) == (row, col):
                colour = agent
            for ch in range(3):
                out[ch, r * P:(r + 1) * P, c * P:(c + 1) * P] = colour[ch]
    return out


def run_rule(G, P, cue_steps, max_steps, seed, first_worker_id, actions):
    """``actions`` int64 [S, W], every entry in 0 .. 3 -> a dict of what a ``SerialVecEnv`` of host twins returns over the S steps:
    frames [S + 1, W, 3, GP, GP] (row 0: the reset), rewards [S, W] f32, flags [S, W] u8 (DONE | TRUNCATED | SUCCESS), returns [S, W]
    f32 and lengths [S, W] i32 of the episodes that ended, masks [S + 1, W] u64, infos [S][W], and ``cover``: how often a target was
    hit, a wrong corner entered, an episode cut, a move left the grid."""
    S, W = actions.shape
    envs = [CueRoomEnv(G, P, cue_steps, max_steps, seed, worker_id=first_worker_id + w) for w in range(W)]
    vec = SerialVecEnv(envs)
    side = G * P
    frames = np.zeros((S + 1, W, 3, side, side), dtype=np.uint8)
    rewards, flags = np.zeros((S, W), dtype=np.float32), np.zeros((S, W), dtype=np.uint8)
    returns, lengths = np.zeros((S, W), dtype=np.float32), np.zeros((S, W), dtype=np.int32)
    masks = np.zeros((S + 1, W), dtype=np.uint64)
    cover = dict(hit=0, wrong=0, cut=0, off_grid=0)
    all_infos = []
    vec.reset(out=frames[0])
    vec.action_masks(out=masks[0])
    for t in range(S):
        for w, e in enumerate(envs):
            if not e.action_masks()[actions[t, w]]:
                cover["off_grid"] += 1
        _, rewards[t], dones, infos = vec.step(actions[t], out=frames[t + 1])
        vec.action_masks(out=masks[t + 1])
        clean = []
        for w, info in enumerate(infos):
            assert (info is not None) == bool(dones[w])
            if info is not None:
                cut = bool(info.get("truncated"))
                flags[t, w] = DONE | (TRUNCATED if cut else 0) | (SUCCESS if info["success"] else 0)
                returns[t, w], lengths[t, w] = info["reward"], info["length"]
                cover["cut" if cut else ("hit" if info["success"] else "wrong")] += 1
                info = {k: v for k, v in info.items() if k != "final_observation"}
            clean.append(info)
        all_infos.append(clean)
    return dict(frames=frames, rewards=rewards, flags=flags, returns=returns, lengths=lengths, masks=masks, infos=all_infos, cover=cover,
                envs=envs, vec=vec)


def raw_actions(seed, S, W):
    """[S, W] int64 in -1 .. 5 from a fixed generator: valid moves and, for the kernel's clamp, values on both sides of 0 .. 3."""
    return np.random.default_rng(seed).integers(-1, 6, size=(S, W)).astype(np.int64)


def clamp(actions):
    return np.clip(actions, 0, 3)


@functools.lru_cache(maxsize=None)
def kernel_case(G, P, W, cue_steps, max_steps, S=41, seed=11, first_worker_id=5):
    """The reference of one case of the kernel test: S steps (the last one checks the carried state) of ``raw_actions``, clamped for
    the host rule.  Cached: computed once, shared, never modified."""
    raw = raw_actions(1000 * G + 10 * P + W + cue_steps + max_steps, S, W)
    ref = run_rule(G, P, cue_steps, max_steps, seed, first_worker_id, clamp(raw))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    raw.setflags(write=False)
    return raw, ref


def assert_covered(cover):
    for what, n in cover.items():
        assert n >= 1, f"the action sequences never produced: {what} ({cover})"
