"""CommandRoom: a command-sequence memory task in the mould of Mortar Mayhem (Grid), with a rule in integer arithmetic only.

A room of ``grid`` x ``grid`` cells (G odd, 3 .. 31), each ``cell`` x ``cell`` pixels (P, a multiple of 4, 4 .. 64); the frame is
[3, G P, G P] uint8 in CHW order and there is no float form.  An episode first SHOWS ``command_count`` (K, 1 .. 16) commands one
after the other, then the agent has to EXECUTE them from memory, one per step.  It is not Memory Gym's rule or pixels.

* actions ``Discrete(5)``: 0 up, 1 right, 2 down, 3 left, 4 stay; an action outside 0 .. 4 raises ValueError (the device kernel
  clamps instead: csrc/device_env.hip).
* the episode is a function of ``(seed + worker_id, episode index)`` alone (``episode_draw``, uint64 arithmetic):
  h = splitmix64(splitmix64(stream) + episode); the start cell is (h >> 8) mod G G, row-major; a cursor starts there with x = h and
  for j = 0 .. K - 1: x = splitmix64(x), the moves among (up, right, down, left, stay) that keep the cursor on the grid are listed in
  that order (3 to 5 of them), cmd_j is entry (x >> 16) mod n of the list and the cursor moves by it -- every drawn sequence can be
  walked.  The sequence packs into one 64-bit word, 3 bits per command (``pack_commands``).
* phases by the observation index t within the episode (t = 0 is the reset frame), L = show_steps + gap_steps:
  - show, t < K L: command j = t div L is visible while t mod L < show_steps -- the centre cell has the mark colour and the centre's
    neighbour in the command's direction the pointer colour (``stay``: no neighbour cell); in a gap observation the whole frame is
    floor.  The agent is not drawn.  The action taken on such an observation is ignored (reward 0, not done); all five mask bits set.
  - execute, t >= K L, e = t - K L: floor with the agent cell; mask bit a set when move a stays on the grid, bit 4 always.  The
    action equal to cmd_e: reward 0.1, the agent moves, n += 1, and after the last command (e = K - 1) done with success 1; any
    other action: reward 0.0, done, success 0.
* the info of a finished episode is {"reward", "length", "success"}: reward = float32(n) * float32(0.1) (one multiply, no
  accumulation), length = t + 1.  No time limit, no truncation: an episode lasts at most K L + K steps (``max_episode_steps``).

This module is the ONE definition of the rule: the tests, enjoy.py, utils.create_env and the serial / worker-process front-ends use
``CommandRoomEnv``; the device-resident front-end (environments/device_env.py) runs the same rule as one HIP kernel per step and is
tested against it byte for byte.  ``command_room_section`` reads and checks the config keys.
"""
from types import SimpleNamespace

import numpy as np

from environments.grid_room import check_encoder_side, episode_hash, paint, read_device, read_integers, splitmix64

# flat colours (R, G, B) by what a cell shows
FLOOR, MARK, POINTER, AGENT = 0, 1, 2, 3
PALETTE = np.array([[20, 24, 40], [208, 208, 216], [48, 176, 232], [232, 96, 32]], dtype=np.uint8)
# (row, column) steps of the five moves: up, right, down, left, stay
MOVES = ((-1, 0), (0, 1), (1, 0), (0, -1), (0, 0))
MAX_COMMANDS = 16                  # what the kernel admits (etm_command_room_supported): 3 bits each in one 64-bit word
REWARD = np.float32(0.1)

DEFAULTS = dict(grid=7, cell=12, command_count=8, show_steps=1, gap_steps=1, seed=0)
KEYS = ("type", *DEFAULTS, "device", "vectorize")


def episode_draw(stream: int, episode: int, G: int, K: int):
    """(start row, start column, the K commands) of episode ``episode`` of the worker stream ``stream`` (= seed + worker_id)."""
    h = episode_hash(stream, episode)
    start = (h >> 8) % (G * G)
    row, col = start // G, start % G
    r, c, x, commands = row, col, h, []
    for _ in range(K):
        x = splitmix64(x)
        valid = [a for a, (dr, dc) in enumerate(MOVES) if 0 <= r + dr < G and 0 <= c + dc < G]
        a = valid[(x >> 16) % len(valid)]
        commands.append(a)
        r, c = r + MOVES[a][0], c + MOVES[a][1]
    return int(row), int(col), tuple(commands)


def pack_commands(commands) -> int:
    """The sequence as one 64-bit word: command j in bits [3 j, 3 j + 3)."""
    word = 0
    for j, a in enumerate(commands):
        word |= int(a) << (3 * j)
    return word


def command_room_section(env_config: dict) -> dict:
    """The ``environment`` section of a ``type: CommandRoom`` config -> {"grid", "cell", "command_count", "show_steps", "gap_steps",
    "seed", "device"} with the defaults (7, 12, 8, 1, 1, 0, False) filled in.  Refused, each with what to do instead: unknown
    sub-keys, non-integers, an even grid or one outside 3 .. 31, a cell that is no multiple of 4 in 4 .. 64, a side grid * cell the
    encoder cannot take, command_count outside 1 .. 16, show_steps < 1, gap_steps < 0, a ``device`` that is no bool."""
    sec = read_integers("CommandRoom", env_config, KEYS, DEFAULTS, "the commands are shown around a centre cell")
    check_encoder_side(sec["grid"], sec["cell"])
    K, show, gap = sec["command_count"], sec["show_steps"], sec["gap_steps"]
    if K < 1 or K > MAX_COMMANDS:
        raise ValueError(f"environment.command_count must be between 1 and {MAX_COMMANDS} (the sequence is one 64-bit word, 3 bits per "
                         f"command), got {K}: use {max(1, min(MAX_COMMANDS, K))}")
    if show < 1:
        raise ValueError(f"environment.show_steps must be at least 1 (a command that is never visible cannot be memorised), got {show}: "
                         "use 1")
    if gap < 0:
        raise ValueError(f"environment.gap_steps must be at least 0, got {gap}: use 0 for commands shown back to back")
    return dict(sec, device=read_device(env_config))


def shown(t: int, K: int, show_steps: int, gap_steps: int):
    """What observation ``t`` of an episode shows: ("show", j) while command j is visible, ("gap", j) between, ("execute", e) after."""
    L = show_steps + gap_steps
    if t < K * L:
        return ("show" if t % L < show_steps else "gap"), t // L
    return "execute", t - K * L


def render(G: int, P: int, phase: str, command: int, row: int, col: int, out=None):
    """The frame [3, G P, G P] uint8: floor; while a command shows, the centre in the mark colour and its neighbour in the command's
    direction in the pointer colour; in the execute phase the agent cell."""
    cells = np.full((G, G), FLOOR, dtype=np.intp)
    if phase == "show":
        mid = G // 2
        cells[mid, mid] = MARK
        if command != 4:
            cells[mid + MOVES[command][0], mid + MOVES[command][1]] = POINTER
    elif phase == "execute":
        cells[row, col] = AGENT
    return paint(PALETTE, cells, P, out)


class CommandRoomEnv:
    def __init__(self, grid: int = 7, cell: int = 12, command_count: int = 8, show_steps: int = 1, gap_steps: int = 1, seed: int = 0,
                 worker_id: int = 0):
        sec = command_room_section(dict(grid=grid, cell=cell, command_count=command_count, show_steps=show_steps, gap_steps=gap_steps,
                                        seed=seed))
        self.grid, self.cell, self.command_count = sec["grid"], sec["cell"], sec["command_count"]
        self.show_steps, self.gap_steps = sec["show_steps"], sec["gap_steps"]
        self.show_length = self.command_count * (self.show_steps + self.gap_steps)      # K L: the first execute observation
        self.max_episode_steps = self.show_length + self.command_count
        self.stream = sec["seed"] + int(worker_id)
        self.episode = -1                       # reset() starts episode 0
        self.commands = ()
        self.row = self.col = self.t = self.n = 0

    @property
    def observation_space(self):
        side = self.grid * self.cell
        return SimpleNamespace(shape=(3, side, side), low=0, high=255, dtype=np.uint8)

    @property
    def action_space(self):
        return SimpleNamespace(n=5)

    def _obs(self):
        phase, j = shown(self.t, self.command_count, self.show_steps, self.gap_steps)
        return render(self.grid, self.cell, phase, self.commands[j] if phase == "show" else 4, self.row, self.col)

    def reset(self, **kwargs):
        self.episode += 1
        self.row, self.col, self.commands = episode_draw(self.stream, self.episode, self.grid, self.command_count)
        self.t = self.n = 0
        return self._obs()

    def action_masks(self):
        if self.t < self.show_length:
            return np.ones(5, dtype=bool)
        G = self.grid
        return np.array([self.row > 0, self.col < G - 1, self.row < G - 1, self.col > 0, True], dtype=bool)

    def step(self, action):
        a = int(np.asarray(action).reshape(-1)[0])
        if a < 0 or a > 4:
            raise ValueError(f"CommandRoom: action {a} is outside Discrete(5)")
        if self.episode < 0:
            raise RuntimeError("CommandRoom: step() before reset()")
        reward, done, info = 0.0, False, None
        e = self.t - self.show_length
        if e >= 0:
            if e < self.command_count and a == self.commands[e]:
                reward = float(REWARD)
                self.row, self.col = self.row + MOVES[a][0], self.col + MOVES[a][1]
                self.n += 1
                done = e == self.command_count - 1
            else:
                done = True
            if done:
                info = {"reward": float(np.float32(self.n) * REWARD), "length": int(self.t + 1),
                        "success": int(self.n == self.command_count)}
        self.t += 1
        return self._obs(), reward, done, info

    def close(self):
        return None
