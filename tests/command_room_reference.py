"""Shared by the CommandRoom tests: the host rule run over a table of actions that is built step by step against the host twins (the
reference every device result is compared with), a per-cell reconstruction of a frame from (phase, command, row, col) that does not
use the rule's renderer, and the cover condition."""
import functools

import numpy as np

from environments.command_room_env import CommandRoomEnv, PALETTE
from environments.vec_env import SerialVecEnv

DONE, TRUNCATED, SUCCESS = 1, 2, 4


def frame_from_cells(G, P, phase, command, row, col):
    """The frame of an observation, cell by cell and pixel by pixel from the stated rule.  ``phase``: "show" (the centre in the mark
    colour, its neighbour in the direction of ``command`` in the pointer colour, none for stay), "gap" (floor) or "execute" (floor with
    the agent cell)."""
    floor, mark, pointer, agent = (PALETTE[i] for i in range(4))
    mid = G // 2
    neighbour = {0: (mid - 1, mid), 1: (mid, mid + 1), 2: (mid + 1, mid), 3: (mid, mid - 1), 4: None}[command] if phase == "show" else None
    out = np.zeros((3, G * P, G * P), dtype=np.uint8)
    for r in range(G):
        for c in range(G):
            colour = floor
            if phase == "show" and (r, c) == (mid, mid):
                colour = mark
            if phase == "show" and (r, c) == neighbour:
                colour = pointer
            if phase == "execute" and (r, c) == (row, col):
                colour = agent
            for ch in range(3):
                out[ch, r * P:(r + 1) * P, c * P:(c + 1) * P] = colour[ch]
    return out


def clamp(actions):
    return np.clip(actions, 0, 4)


def run_rule(G, P, K, show_steps, gap_steps, seed, first_worker_id, S, W, table_seed):
    """S steps of a ``SerialVecEnv`` of W host twins over an action table built step by step from ``default_rng(table_seed)``: every
    entry is a raw value in -1 .. 6, and where the twin is in its execute phase the raw value is replaced by the correct command with
    probability 7 / 8.  The host rule takes the values clamped to 0 .. 4; ``raw`` [S, W] is what the kernel is given.  -> a dict:
    raw, frames [S + 1, W, 3, GP, GP] (row 0: the reset), rewards [S, W] f32, flags [S, W] u8 (DONE | SUCCESS), returns [S, W] f32 and
    lengths [S, W] i32 of the episodes that ended, masks [S + 1, W] u64, infos [S][W], and ``cover``: successes, failures, clamped
    actions, ignored actions (taken on a show or gap observation), and how often each of the five commands was executed."""
    rng = np.random.default_rng(table_seed)
    envs = [CommandRoomEnv(G, P, K, show_steps, gap_steps, seed, worker_id=first_worker_id + w) for w in range(W)]
    vec = SerialVecEnv(envs)
    side = G * P
    raw = np.zeros((S, W), dtype=np.int64)
    frames = np.zeros((S + 1, W, 3, side, side), dtype=np.uint8)
    rewards, flags = np.zeros((S, W), dtype=np.float32), np.zeros((S, W), dtype=np.uint8)
    returns, lengths = np.zeros((S, W), dtype=np.float32), np.zeros((S, W), dtype=np.int32)
    masks = np.zeros((S + 1, W), dtype=np.uint64)
    cover = dict(success=0, failure=0, clamped=0, ignored=0, executed=[0] * 5)
    all_infos = []
    vec.reset(out=frames[0])
    vec.action_masks(out=masks[0])
    for t in range(S):
        values, correct = rng.integers(-1, 7, size=W), rng.integers(0, 8, size=W) != 0
        for w, e in enumerate(envs):
            k = e.t - e.show_length
            if k >= 0 and correct[w]:
                values[w] = e.commands[k]
            raw[t, w] = values[w]
            cover["clamped"] += int(values[w] < 0 or values[w] > 4)
            if k < 0:
                cover["ignored"] += 1
            elif clamp(values[w]) == e.commands[k]:
                cover["executed"][e.commands[k]] += 1
        _, rewards[t], dones, infos = vec.step(clamp(raw[t]), out=frames[t + 1])
        vec.action_masks(out=masks[t + 1])
        for w, info in enumerate(infos):
            assert (info is not None) == bool(dones[w])
            if info is not None:
                assert "truncated" not in info and "final_observation" not in info
                flags[t, w] = DONE | (SUCCESS if info["success"] else 0)
                returns[t, w], lengths[t, w] = info["reward"], info["length"]
                cover["success" if info["success"] else "failure"] += 1
        all_infos.append(list(infos))
    return dict(raw=raw, frames=frames, rewards=rewards, flags=flags, returns=returns, lengths=lengths, masks=masks, infos=all_infos,
                cover=cover, envs=envs, vec=vec)


@functools.lru_cache(maxsize=None)
def kernel_case(G, P, W, K, show_steps, gap_steps, S, seed=11, first_worker_id=5):
    """The reference of one case of the kernel test (the last step checks the carried state).  Cached: computed once, shared, never
    modified."""
    ref = run_rule(G, P, K, show_steps, gap_steps, seed, first_worker_id, S, W,
                   table_seed=100000 * G + 1000 * P + 100 * K + 10 * show_steps + gap_steps + 7 * W)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def assert_covered(cover):
    """At least one success, one failure, one clamped action, one ignored action, and each of the five commands executed."""
    for what in ("success", "failure", "clamped", "ignored"):
        assert cover[what] >= 1, f"the action table never produced: {what} ({cover})"
    for a, n in enumerate(cover["executed"]):
        assert n >= 1, f"command {a} was never executed ({cover})"
