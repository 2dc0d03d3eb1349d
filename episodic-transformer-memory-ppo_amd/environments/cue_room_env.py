"""CueRoom: a small image task that needs memory, with a rule in integer arithmetic only.

A room of ``grid`` x ``grid`` cells (G odd, >= 3), each ``cell`` x ``cell`` pixels (P, a multiple of 4); the frame is
[3, G P, G P] uint8 in CHW order and there is no float form.  The four corners are goals and one of them is the episode's target.
The agent starts on a non-corner cell.  In the first ``cue_steps`` observations of an episode the target corner is drawn in the cue
colour; from then on all four corners look alike, so walking to the right corner needs memory of the cue.

* actions ``Discrete(4)``: 0 up, 1 right, 2 down, 3 left; a move off the grid leaves the position unchanged, and an action outside
  0..3 raises ValueError (the device kernel clamps instead: csrc/device_env.hip).
* ``action_masks()`` (sb3-contrib's protocol): entry a is True when move a stays on the grid; every cell keeps at least two.
* entering the target: reward 1.0, done, success 1; entering another corner: reward 0.0, done, success 0; reaching
  ``max_episode_steps``: done, ``"truncated": True``, success 0.  The info of a finished episode is {"reward", "length", "success"}.
* the episode (target, start cell) is a function of ``(seed + worker_id, episode index)`` alone: ``episode_draw``, splitmix64 in
  64-bit integer arithmetic -- the same key gives the same episode here and in the kernel.  ``reset()`` starts the next episode
  (the first call: episode 0).

This module is the ONE definition of the rule: the tests, enjoy.py and the worker processes use ``CueRoomEnv``; the device-resident
front-end (environments/device_env.py) runs the same rule as one HIP kernel per step and is tested against it byte for byte.
``cue_room_section`` reads and checks the config keys.
"""
from types import SimpleNamespace

import numpy as np

# flat colours (R, G, B) by what a cell shows; the agent is drawn last
FLOOR, GOAL, CUE, AGENT = 0, 1, 2, 3
PALETTE = np.array([[24, 24, 32], [64, 160, 64], [240, 208, 32], [224, 48, 48]], dtype=np.uint8)
# (row, column) steps of the four moves: up, right, down, left
MOVES = ((-1, 0), (0, 1), (1, 0), (0, -1))
MAX_GRID, MAX_CELL = 31, 64        # what the kernel admits (etm_cue_room_supported)

KEYS = ("type", "grid", "cell", "cue_steps", "max_episode_steps", "seed", "device", "vectorize")
_MASK64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """One step of splitmix64 on a 64-bit word (Python integers reduced mod 2^64: what uint64 arithmetic does)."""
    z = (int(x) + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def corner_cells(G: int):
    """(row, column) of corner k: 0 top left, 1 top right, 2 bottom right, 3 bottom left."""
    return ((0, 0), (0, G - 1), (G - 1, G - 1), (G - 1, 0))


def episode_draw(stream: int, episode: int, G: int):
    """(target corner, start row, start column) of episode ``episode`` of the worker stream ``stream`` (= seed + worker_id).
    h = splitmix64(splitmix64(stream) + episode); target = h & 3; the start is non-corner cell (h >> 8) mod (G G - 4) in row-major
    order with the corners left out."""
    h = splitmix64((splitmix64(int(stream) & _MASK64) + int(episode)) & _MASK64)
    target = h & 3
    c = (h >> 8) % (G * G - 4) + 1        # row-major index with the corners skipped: past (0, 0) ...
    if c >= G - 1:                        # ... past (0, G - 1) ...
        c += 1
    if c >= G * (G - 1):                  # ... and past (G - 1, 0)
        c += 1
    return int(target), int(c // G), int(c % G)


def encoder_takes(side: int) -> bool:
    """The model's image encoder (8x8 stride 4, 4x4 stride 2, 3x3 stride 1, no padding) leaves at least one position."""
    o1 = (side - 8) // 4 + 1 if side >= 8 else 0
    o2 = (o1 - 4) // 2 + 1 if o1 >= 4 else 0
    return o2 - 2 >= 1


def cue_room_section(env_config: dict) -> dict:
    """The ``environment`` section of a ``type: CueRoom`` config -> {"grid", "cell", "cue_steps", "max_episode_steps", "seed",
    "device"} with the defaults (7, 12, 2, 32, 0, False) filled in.  Refused, each with what to do instead: unknown sub-keys, an even
    grid or one below 3 (or above what the kernel admits), a cell that is no multiple of 4, cue_steps < 1, max_episode_steps < 1, a
    side grid * cell the encoder cannot take."""
    unknown = sorted(set(env_config) - set(KEYS))
    if unknown:
        raise ValueError(f"environment (CueRoom): unknown keys {unknown} (known: {sorted(KEYS)}); remove them")
    G, P = env_config.get("grid", 7), env_config.get("cell", 12)
    cue, T = env_config.get("cue_steps", 2), env_config.get("max_episode_steps", 32)
    for name, v in (("grid", G), ("cell", P), ("cue_steps", cue), ("max_episode_steps", T), ("seed", env_config.get("seed", 0))):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"environment.{name} (CueRoom) must be an integer, got {v!r}")
    if G < 3 or G % 2 == 0 or G > MAX_GRID:
        raise ValueError(f"environment.grid must be odd and between 3 and {MAX_GRID} (the corners and a centre need it), got {G}: "
                         f"use {max(3, min(MAX_GRID, G + 1 - G % 2 if G >= 3 else 3))}")
    if P < 4 or P % 4 != 0 or P > MAX_CELL:
        raise ValueError(f"environment.cell must be a multiple of 4 between 4 and {MAX_CELL} (frames are written in 4-byte words that "
                         f"never straddle two cells), got {P}: use {max(4, min(MAX_CELL, (P + 3) // 4 * 4))}")
    if cue < 1:
        raise ValueError(f"environment.cue_steps must be at least 1 (observation 0 is the only one that can show the cue then), got {cue}")
    if T < 1:
        raise ValueError(f"environment.max_episode_steps must be at least 1, got {T}")
    if not encoder_takes(G * P):
        raise ValueError(f"environment: a {G * P} x {G * P} frame (grid {G} x cell {P}) is too small for the image encoder (8x8/4, 4x4/2, "
                         "3x3/1 need a side of at least 36): raise grid or cell")
    dev = env_config.get("device", False)
    if not isinstance(dev, bool):
        raise ValueError(f"environment.device must be true or false, got {dev!r}")
    return dict(grid=int(G), cell=int(P), cue_steps=int(cue), max_episode_steps=int(T), seed=int(env_config.get("seed", 0)), device=dev)


def check_device_env_config(config: dict, world: int = 1) -> bool:
    """``environment.device: true`` against the rest of the config, before anything is built -> whether the key is on.  Refused:
    ``worker_processes: true`` (the environments live on the device, no process steps them), ``bootstrap_truncated: true`` (the
    front-end keeps no final observation) and a data-parallel run (``world`` > 1: not built, not measured).  Every type of
    environments/device_types.py is covered alike."""
    from environments.device_types import device_env_section
    sec = device_env_section(config.get("environment", {}))
    if sec is None or not sec["device"]:
        return False
    if config.get("worker_processes", False):
        raise ValueError("environment.device: true keeps the environments on the device, worker_processes: true in host processes: set "
                         "worker_processes: false, or device: false to step the host twin in the worker processes")
    if config.get("bootstrap_truncated", False):
        raise ValueError("environment.device: true does not carry bootstrap_truncated: true (the device front-end keeps no final "
                         "observation): set device: false (the host twin hands it over in its info), or leave bootstrap_truncated off")
    if int(world) > 1:
        raise ValueError("environment.device: true is not built for data-parallel runs (every rank would need its own worker streams and "
                         "nothing here has run more than one rank): run one rank, or set device: false")
    return True


def render(G: int, P: int, row: int, col: int, target: int, cue_visible: bool, out=None):
    """The frame [3, G P, G P] uint8 of a state: floor, the four goals, the target in the cue colour while it shows, the agent last."""
    cells = np.full((G, G), FLOOR, dtype=np.intp)
    for k, (r, c) in enumerate(corner_cells(G)):
        cells[r, c] = CUE if cue_visible and k == target else GOAL
    cells[row, col] = AGENT
    frame = PALETTE[cells].transpose(2, 0, 1).repeat(P, axis=1).repeat(P, axis=2)      # [G, G, 3] -> [3, G P, G P]
    if out is None:
        return np.ascontiguousarray(frame)
    out[...] = frame
    return out


class CueRoomEnv:
    def __init__(self, grid: int = 7, cell: int = 12, cue_steps: int = 2, max_episode_steps: int = 32, seed: int = 0, worker_id: int = 0):
        sec = cue_room_section(dict(grid=grid, cell=cell, cue_steps=cue_steps, max_episode_steps=max_episode_steps, seed=seed))
        self.grid, self.cell, self.cue_steps = sec["grid"], sec["cell"], sec["cue_steps"]
        self.max_episode_steps = sec["max_episode_steps"]
        self.stream = sec["seed"] + int(worker_id)
        self.episode = -1                       # reset() starts episode 0
        self.target = self.row = self.col = self.t = 0
        self._return = 0.0

    @property
    def observation_space(self):
        side = self.grid * self.cell
        return SimpleNamespace(shape=(3, side, side), low=0, high=255, dtype=np.uint8)

    @property
    def action_space(self):
        return SimpleNamespace(n=4)

    def _obs(self):
        return render(self.grid, self.cell, self.row, self.col, self.target, self.t < self.cue_steps)

    def reset(self, **kwargs):
        self.episode += 1
        self.target, self.row, self.col = episode_draw(self.stream, self.episode, self.grid)
        self.t, self._return = 0, 0.0
        return self._obs()

    def action_masks(self):
        G = self.grid
        return np.array([self.row > 0, self.col < G - 1, self.row < G - 1, self.col > 0], dtype=bool)

    def step(self, action):
        a = int(np.asarray(action).reshape(-1)[0])
        if a < 0 or a > 3:
            raise ValueError(f"CueRoom: action {a} is outside Discrete(4)")
        if self.episode < 0:
            raise RuntimeError("CueRoom: step() before reset()")
        G = self.grid
        r, c = self.row + MOVES[a][0], self.col + MOVES[a][1]
        if 0 <= r < G and 0 <= c < G:
            self.row, self.col = r, c
        self.t += 1
        reward, done, info = 0.0, False, None
        corners = corner_cells(G)
        if (self.row, self.col) in corners:
            hit = corners.index((self.row, self.col)) == self.target
            reward, done = (1.0 if hit else 0.0), True
            self._return += reward
            info = {"reward": float(self._return), "length": int(self.t), "success": int(hit)}
        elif self.t >= self.max_episode_steps:
            done = True
            info = {"reward": float(self._return), "length": int(self.t), "success": 0, "truncated": True}
        return self._obs(), reward, done, info

    def close(self):
        return None
