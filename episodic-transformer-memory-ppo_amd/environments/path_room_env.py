"""PathRoom: a hidden-path memory task in the mould of Mystery Path (Grid), with a rule in integer arithmetic only.

A room of ``grid`` x ``grid`` cells (G odd, 3 .. 31), each ``cell`` x ``cell`` pixels (P, a multiple of 4, 4 .. 64); the frame is
[3, G P, G P] uint8 in CHW order and there is no float form.  An invisible path leads from an origin in column 0 to a goal; the
agent finds it by trial.  After every fall it stands on the origin again, on a frame that looks like the first one, so only the
memory of the earlier steps says which moves have already failed.  It is not Memory Gym's rule or pixels.

* actions ``Discrete(4)``: 0 up, 1 right, 2 down, 3 left; an action outside 0 .. 3 raises ValueError (the device kernel clamps
  instead: csrc/device_env.hip).
* the episode is a function of ``(seed + worker_id, episode index)`` alone (``episode_draw``, uint64 arithmetic):
  h = splitmix64(splitmix64(stream) + episode); the origin is row (h >> 8) mod G of column 0; a cursor starts there with x = h and no
  previous move, and for j = 0 .. M - 1 (M = ``path_moves``, 1 .. 32): stop if the cursor is in column G - 1; x = splitmix64(x); the
  candidates are listed in the order (up, right, down) -- up if the row > 0 and the previous move was not down, right always, down
  if the row < G - 1 and the previous move was not up; move j is entry (x >> 16) mod n of the list (n = 1, 2 or 3) and the cursor
  moves by it.  The path is the n + 1 cells visited (n <= M moves), its last cell the goal: the walk is never stuck, visits no cell
  twice, and the goal differs from the origin.  The moves pack into one 64-bit word, 2 bits each (``pack_moves``).
* the agent starts on the origin with best = 0.  A move off the grid is a no-op.  A move onto the path cell of index i moves the
  agent there -- forwards, backwards, or across a bend to a cell several indices away --, earns k = max(i - best, 0) tenths and sets
  best = max(best, i); arriving on the goal (i = n) adds 10 tenths and ends the episode with success 1.  A move onto a cell that is
  not on the path is a FALL: reward 0, not done, the agent stands on the origin again, that cell is the mark of the next observation
  only, and best is kept (progress is paid once).  The step's reward is float32(k) * float32(0.1), one multiply.
* a step that did not end the episode with t + 1 >= ``max_episode_steps``: done, ``"truncated": True``, success 0.
* the info of a finished episode is {"reward", "length", "success"}: reward = float32(best + 10 success) * float32(0.1) (one
  multiply, no accumulation), length = t + 1.
* the observation: floor, then the goal cell, then the mark cell (if the previous step was a fall), then the agent cell, drawn in
  this order.  The path and the origin are never drawn.
* ``action_masks()``: entry a is True when move a stays on the grid.

This module is the ONE definition of the rule: the tests, enjoy.py, utils.create_env and the serial / worker-process front-ends use
``PathRoomEnv``; the device-resident front-end (environments/device_env.py) runs the same rule as one HIP kernel per step and is
tested against it byte for byte.  ``path_room_section`` reads and checks the config keys.
"""
from types import SimpleNamespace

import numpy as np

from environments.grid_room import check_encoder_side, episode_hash, paint, read_device, read_integers, splitmix64

# flat colours (R, G, B) by what a cell shows; drawn in this order, the agent last
FLOOR, GOAL, MARK, AGENT = 0, 1, 2, 3
PALETTE = np.array([[28, 28, 36], [64, 192, 96], [232, 64, 200], [240, 200, 48]], dtype=np.uint8)
# (row, column) steps of the four moves: up, right, down, left
MOVES = ((-1, 0), (0, 1), (1, 0), (0, -1))
MAX_MOVES = 32                     # what the kernel admits (etm_path_room_supported): 2 bits each in one 64-bit word
REWARD = np.float32(0.1)
GOAL_TENTHS = 10

DEFAULTS = dict(grid=7, cell=12, path_moves=16, max_episode_steps=64, seed=0)
KEYS = ("type", *DEFAULTS, "device", "vectorize")


def episode_draw(stream: int, episode: int, G: int, M: int):
    """(origin row, the n <= M moves of the path) of episode ``episode`` of the worker stream ``stream`` (= seed + worker_id); the
    origin is in column 0 and every move is 0 (up), 1 (right) or 2 (down)."""
    h = episode_hash(stream, episode)
    origin = (h >> 8) % G
    r, c, x, previous, moves = origin, 0, h, -1, []
    for _ in range(M):
        if c == G - 1:
            break
        x = splitmix64(x)
        candidates = []
        if r > 0 and previous != 2:
            candidates.append(0)
        candidates.append(1)
        if r < G - 1 and previous != 0:
            candidates.append(2)
        a = candidates[(x >> 16) % len(candidates)]
        moves.append(a)
        r, c, previous = r + MOVES[a][0], c + MOVES[a][1], a
    return int(origin), tuple(moves)


def pack_moves(moves) -> int:
    """The path as one 64-bit word: move j in bits [2 j, 2 j + 2)."""
    word = 0
    for j, a in enumerate(moves):
        word |= int(a) << (2 * j)
    return word


def unpack_moves(word: int, n: int):
    return tuple(int(word) >> (2 * j) & 3 for j in range(n))


def path_cells(origin: int, moves):
    """The n + 1 cells (row, column) of the path, the origin first and the goal last."""
    cells = [(int(origin), 0)]
    for a in moves:
        cells.append((cells[-1][0] + MOVES[a][0], cells[-1][1] + MOVES[a][1]))
    return cells


def path_room_section(env_config: dict) -> dict:
    """The ``environment`` section of a ``type: PathRoom`` config -> {"grid", "cell", "path_moves", "max_episode_steps", "seed",
    "device"} with the defaults (7, 12, 16, 64, 0, False) filled in.  Refused, each with what to do instead: unknown sub-keys,
    non-integers, an even grid or one outside 3 .. 31, a cell that is no multiple of 4 in 4 .. 64, a side grid * cell the encoder
    cannot take, path_moves outside 1 .. 32, max_episode_steps < 1, a ``device`` that is no bool."""
    sec = read_integers("PathRoom", env_config, KEYS, DEFAULTS, "the path crosses the room from a cell of the left column")
    check_encoder_side(sec["grid"], sec["cell"])
    M, limit = sec["path_moves"], sec["max_episode_steps"]
    if M < 1 or M > MAX_MOVES:
        raise ValueError(f"environment.path_moves must be between 1 and {MAX_MOVES} (the path is one 64-bit word, 2 bits per move), "
                         f"got {M}: use {max(1, min(MAX_MOVES, M))}")
    if limit < 1:
        raise ValueError(f"environment.max_episode_steps must be at least 1 (an episode needs a step), got {limit}: use 1 or more")
    return dict(sec, device=read_device(env_config))


def render(G: int, P: int, goal, mark, agent, out=None):
    """The frame [3, G P, G P] uint8: floor, the goal cell, the mark cell (``mark``: (row, column) or None), the agent cell last."""
    cells = np.full((G, G), FLOOR, dtype=np.intp)
    cells[goal] = GOAL
    if mark is not None:
        cells[mark] = MARK
    cells[agent] = AGENT
    return paint(PALETTE, cells, P, out)


class PathRoomEnv:
    def __init__(self, grid: int = 7, cell: int = 12, path_moves: int = 16, max_episode_steps: int = 64, seed: int = 0,
                 worker_id: int = 0):
        sec = path_room_section(dict(grid=grid, cell=cell, path_moves=path_moves, max_episode_steps=max_episode_steps, seed=seed))
        self.grid, self.cell, self.path_moves = sec["grid"], sec["cell"], sec["path_moves"]
        self.max_episode_steps = sec["max_episode_steps"]
        self.stream = sec["seed"] + int(worker_id)
        self.episode = -1                       # reset() starts episode 0
        self.origin, self.moves, self.cells = 0, (), [(0, 0)]
        self.row = self.col = self.t = self.best = 0
        self.mark = None

    @property
    def observation_space(self):
        side = self.grid * self.cell
        return SimpleNamespace(shape=(3, side, side), low=0, high=255, dtype=np.uint8)

    @property
    def action_space(self):
        return SimpleNamespace(n=4)

    def _obs(self):
        return render(self.grid, self.cell, self.cells[-1], self.mark, (self.row, self.col))

    def reset(self, **kwargs):
        self.episode += 1
        self.origin, self.moves = episode_draw(self.stream, self.episode, self.grid, self.path_moves)
        self.cells = path_cells(self.origin, self.moves)
        self.row, self.col, self.mark = self.origin, 0, None
        self.t = self.best = 0
        return self._obs()

    def action_masks(self):
        G = self.grid
        return np.array([self.row > 0, self.col < G - 1, self.row < G - 1, self.col > 0], dtype=bool)

    def step(self, action):
        a = int(np.asarray(action).reshape(-1)[0])
        if a < 0 or a > 3:
            raise ValueError(f"PathRoom: action {a} is outside Discrete(4)")
        if self.episode < 0:
            raise RuntimeError("PathRoom: step() before reset()")
        G, n = self.grid, len(self.moves)
        k, success, done, info = 0, 0, False, None
        self.mark = None
        target = (self.row + MOVES[a][0], self.col + MOVES[a][1])
        if 0 <= target[0] < G and 0 <= target[1] < G:
            if target in self.cells:
                i = self.cells.index(target)
                self.row, self.col = target
                k = max(i - self.best, 0)
                self.best = max(self.best, i)
                if i == n:
                    k += GOAL_TENTHS
                    success, done = 1, True
            else:                               # a fall: back to the origin, the cell marked for one observation
                self.row, self.col, self.mark = self.origin, 0, target
        if done:
            info = {}
        elif self.t + 1 >= self.max_episode_steps:
            done, info = True, {"truncated": True}
        if done:
            info = dict({"reward": float(np.float32(self.best + GOAL_TENTHS * success) * REWARD), "length": int(self.t + 1),
                         "success": success}, **info)
        self.t += 1
        return self._obs(), float(np.float32(k) * REWARD), done, info

    def close(self):
        return None
