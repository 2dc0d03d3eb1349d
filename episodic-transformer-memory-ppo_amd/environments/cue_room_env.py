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

# (importable from here as before, defined where they belong: the mixer with the rooms' shared code, the check beside the type table)
from environments.device_types import check_device_env_config  # noqa: F401
from environments.grid_room import splitmix64  # noqa: F401
from environments.grid_room import check_encoder_side, episode_hash, paint, read_device, read_integers

# flat colours (R, G, B) by what a cell shows; the agent is drawn last
FLOOR, GOAL, CUE, AGENT = 0, 1, 2, 3
PALETTE = np.array([[24, 24, 32], [64, 160, 64], [240, 208, 32], [224, 48, 48]], dtype=np.uint8)
# (row, column) steps of the four moves: up, right, down, left
MOVES = ((-1, 0), (0, 1), (1, 0), (0, -1))

DEFAULTS = dict(grid=7, cell=12, cue_steps=2, max_episode_steps=32, seed=0)
KEYS = ("type", *DEFAULTS, "device", "vectorize")


def corner_cells(G: int):
    """(row, column) of corner k: 0 top left, 1 top right, 2 bottom right, 3 bottom left."""
    return ((0, 0), (0, G - 1), (G - 1, G - 1), (G - 1, 0))


def episode_draw(stream: int, episode: int, G: int):
    """(target corner, start row, start column) of episode ``episode`` of the worker stream ``stream`` (= seed + worker_id).
    h = splitmix64(splitmix64(stream) + episode); target = h & 3; the start is non-corner cell (h >> 8) mod (G G - 4) in row-major
    order with the corners left out."""
    h = episode_hash(stream, episode)
    target = h & 3
    c = (h >> 8) % (G * G - 4) + 1        # row-major index with the corners skipped: past (0, 0) ...
    if c >= G - 1:                        # ... past (0, G - 1) ...
        c += 1
    if c >= G * (G - 1):                  # ... and past (G - 1, 0)
        c += 1
    return int(target), int(c // G), int(c % G)


def cue_room_section(env_config: dict) -> dict:
    """The ``environment`` section of a ``type: CueRoom`` config -> {"grid", "cell", "cue_steps", "max_episode_steps", "seed",
    "device"} with the defaults (7, 12, 2, 32, 0, False) filled in.  Refused, each with what to do instead: unknown sub-keys, an even
    grid or one below 3 (or above what the kernel admits), a cell that is no multiple of 4, cue_steps < 1, max_episode_steps < 1, a
    side grid * cell the encoder cannot take."""
    sec = read_integers("CueRoom", env_config, KEYS, DEFAULTS, "the corners and a centre need it")
    if sec["cue_steps"] < 1:
        raise ValueError("environment.cue_steps must be at least 1 (observation 0 is the only one that can show the cue then), got "
                         f"{sec['cue_steps']}")
    if sec["max_episode_steps"] < 1:
        raise ValueError(f"environment.max_episode_steps must be at least 1, got {sec['max_episode_steps']}")
    check_encoder_side(sec["grid"], sec["cell"])
    return dict(sec, device=read_device(env_config))


def render(G: int, P: int, row: int, col: int, target: int, cue_visible: bool, out=None):
    """The frame [3, G P, G P] uint8 of a state: floor, the four goals, the target in the cue colour while it shows, the agent last."""
    cells = np.full((G, G), FLOOR, dtype=np.intp)
    for k, (r, c) in enumerate(corner_cells(G)):
        cells[r, c] = CUE if cue_visible and k == target else GOAL
    cells[row, col] = AGENT
    return paint(PALETTE, cells, P, out)


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
