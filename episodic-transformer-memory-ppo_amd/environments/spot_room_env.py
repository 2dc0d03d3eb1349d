"""SpotRoom: a dark-room task with moving spotlights in the mould of Searing Spotlights, with a rule in integer arithmetic only.

A room of ``grid`` x ``grid`` cells (G odd, 3 .. 31), each ``cell`` x ``cell`` pixels (P, a multiple of 4, 4 .. 64); the frame is
[3, G P, G P] uint8 in CHW order and there is no float form.  The agent collects a coin and then leaves through an exit.  After the
first ``light_steps`` observations the room is dark: the agent sees ITSELF only while one of the moving spotlights is on it, and
that costs health -- so it has to keep its own position from its earlier observations and its own earlier actions.  It is not Memory
Gym's rule or pixels.

* actions ``Discrete(5)``: 0 up, 1 right, 2 down, 3 left, 4 stay; an action outside 0 .. 4 raises ValueError (the device kernel
  clamps instead: csrc/device_env.hip).
* the episode is a function of ``(seed + worker_id, episode index)`` alone (``episode_draw``, uint64 arithmetic), with
  f(x) = (x >> 16) & 0xFFFFFF: h = splitmix64(splitmix64(stream) + episode); the agent's start cell (row-major) is
  ((h >> 8) & 0xFFFFFF) mod G^2; x = h; x = splitmix64(x), the coin is entry f(x) mod (G^2 - 1) of the cells, in row-major order,
  that are not the start cell; x = splitmix64(x), the exit is entry f(x) mod (G^2 - 2) of the cells that are neither; for every
  spotlight i < N (``spotlights``, 0 .. 4): x = splitmix64(x), axis = (x >> 16) & 1, lane = ((x >> 20) & 0xFFFF) mod G,
  phase = ((x >> 40) & 0xFFFF) mod (2 G - 2).  Every pick is a 32-bit remainder.
* a spotlight is active at observation index t >= T0 (``light_steps``, >= 1): q = (phase + (t - T0) div ``spot_period``) mod
  (2 G - 2), pos = q if q < G else 2 G - 2 - q (a triangle wave over its lane), its centre is (row, column) = (lane, pos) for
  axis 0 and (pos, lane) for axis 1, and it lights the 3 x 3 block around the centre, clipped to the grid.  A cell is *lit at t*
  when t >= T0 and some spotlight lights it.
* the step from observation t to t + 1, in this order: (1) the move -- off the grid, or stay, leaves the agent where it is;
  (2) on the coin cell with the coin not yet taken: the coin is taken, +5 tenths; (3) on the exit cell with the coin taken: +10
  tenths, done with success 1 (the exit without the coin does nothing); (4) if (3) did not end the episode and the agent's cell is
  lit at t + 1: health (``health`` H at the start, 1 .. 15) drops by 1, -1 tenth, and at health 0 the episode is done with success
  0; (5) not done and t + 1 >= ``max_episode_steps``: done, ``"truncated": True``.  The step's reward is float32(k) * float32(0.1),
  k the signed sum of tenths: one multiply.
* the info of a finished episode is {"reward", "length", "success"}: reward = float32(5 coin + 10 success - (H - health)) *
  float32(0.1) (one multiply, no accumulation), length = t + 1.
* the observation at t: for t < T0 all floor is lit floor, otherwise floor is dark and the lit cells are lit floor; then the coin
  (if not taken), the exit and the agent are drawn in this order -- the agent only if t < T0 or its cell is lit at t.  In the dark
  the agent appears exactly on the frames that cost health.
* ``action_masks()``: entry a < 4 is True when move a stays on the grid; entry 4 (stay) is always True.

This module is the ONE definition of the rule: the tests, enjoy.py, utils.create_env and the serial / worker-process front-ends use
``SpotRoomEnv``; the device-resident front-end (environments/device_env.py) runs the same rule as one HIP kernel per step and is
tested against it byte for byte.  ``spot_room_section`` reads and checks the config keys.
"""
from types import SimpleNamespace

import numpy as np

from environments.grid_room import check_encoder_side, episode_hash, paint, read_device, read_integers, splitmix64

# flat colours (R, G, B) by what a cell shows; drawn in this order, the agent last.  Pairwise distinct in every channel and in the
# sum of the channels: a wrong colour cannot hide
DARK, LIT, COIN, EXIT, AGENT = 0, 1, 2, 3, 4
PALETTE = np.array([[12, 12, 20], [96, 92, 72], [248, 208, 40], [56, 176, 112], [224, 64, 200]], dtype=np.uint8)
# (row, column) steps of the five actions: up, right, down, left, stay
MOVES = ((-1, 0), (0, 1), (1, 0), (0, -1), (0, 0))
MAX_SPOTLIGHTS = 4                 # what the kernel admits (etm_spot_room_supported): 12 bits each in one 64-bit word, four boxes
MAX_HEALTH = 15                    # four bits of the state
REWARD = np.float32(0.1)
COIN_TENTHS, EXIT_TENTHS = 5, 10

DEFAULTS = dict(grid=7, cell=12, spotlights=2, light_steps=2, spot_period=2, health=5, max_episode_steps=64, seed=0)
KEYS = ("type", *DEFAULTS, "device", "vectorize")


def _field(x: int) -> int:
    return (x >> 16) & 0xFFFFFF


def episode_draw(stream: int, episode: int, G: int, N: int):
    """(start, coin, exit, spotlights) of episode ``episode`` of the worker stream ``stream`` (= seed + worker_id): three distinct
    cells (row, column) and N tuples (axis, lane, phase)."""
    cells = G * G
    h = episode_hash(stream, episode)
    start = ((h >> 8) & 0xFFFFFF) % cells
    x = splitmix64(h)
    coin = [c for c in range(cells) if c != start][_field(x) % (cells - 1)]
    x = splitmix64(x)
    leave = [c for c in range(cells) if c != start and c != coin][_field(x) % (cells - 2)]
    spots = []
    for _ in range(N):
        x = splitmix64(x)
        spots.append((int((x >> 16) & 1), int(((x >> 20) & 0xFFFF) % G), int(((x >> 40) & 0xFFFF) % (2 * G - 2))))
    return divmod(start, G), divmod(coin, G), divmod(leave, G), tuple(spots)


def spot_centre(spot, t: int, G: int, light_steps: int, spot_period: int):
    """The centre (row, column) of the spotlight ``spot`` = (axis, lane, phase) at observation index t >= light_steps."""
    axis, lane, phase = spot
    q = (phase + (t - light_steps) // spot_period) % (2 * G - 2)
    pos = q if q < G else 2 * G - 2 - q
    return (lane, pos) if axis == 0 else (pos, lane)


def lit_cells(spots, t: int, G: int, light_steps: int, spot_period: int):
    """[G, G] bool: the cells lit at observation index t (none before ``light_steps``: the room's own light is not a spotlight)."""
    lit = np.zeros((G, G), dtype=bool)
    if t >= light_steps:
        for spot in spots:
            r, c = spot_centre(spot, t, G, light_steps, spot_period)
            lit[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = True
    return lit


def spot_room_section(env_config: dict) -> dict:
    """The ``environment`` section of a ``type: SpotRoom`` config -> {"grid", "cell", "spotlights", "light_steps", "spot_period",
    "health", "max_episode_steps", "seed", "device"} with the defaults (7, 12, 2, 2, 2, 5, 64, 0, False) filled in.  Refused, each
    with what to do instead: unknown sub-keys, non-integers, an even grid or one outside 3 .. 31, a cell that is no multiple of 4 in
    4 .. 64, a side grid * cell the encoder cannot take, spotlights outside 0 .. 4, light_steps < 1, spot_period < 1, health
    outside 1 .. 15, max_episode_steps < 1, a ``device`` that is no bool."""
    sec = read_integers("SpotRoom", env_config, KEYS, DEFAULTS, "the spotlights sweep lanes of the room from wall to wall")
    check_encoder_side(sec["grid"], sec["cell"])
    N, H = sec["spotlights"], sec["health"]
    if N < 0 or N > MAX_SPOTLIGHTS:
        raise ValueError(f"environment.spotlights must be between 0 and {MAX_SPOTLIGHTS} (a frame word is tested against at most four "
                         f"boxes), got {N}: use {max(0, min(MAX_SPOTLIGHTS, N))}")
    if sec["light_steps"] < 1:
        raise ValueError(f"environment.light_steps must be at least 1 (the first observation shows the room), got {sec['light_steps']}: "
                         "use 1 or more")
    if sec["spot_period"] < 1:
        raise ValueError(f"environment.spot_period must be at least 1 (the steps a spotlight rests on a cell), got {sec['spot_period']}: "
                         "use 1 or more")
    if H < 1 or H > MAX_HEALTH:
        raise ValueError(f"environment.health must be between 1 and {MAX_HEALTH} (four bits of the state), got {H}: "
                         f"use {max(1, min(MAX_HEALTH, H))}")
    if sec["max_episode_steps"] < 1:
        raise ValueError(f"environment.max_episode_steps must be at least 1 (an episode needs a step), got {sec['max_episode_steps']}: "
                         "use 1 or more")
    return dict(sec, device=read_device(env_config))


def render(G: int, P: int, lit, coin, leave, agent, out=None):
    """The frame [3, G P, G P] uint8: dark floor, lit floor where ``lit`` [G, G] bool says so, then the coin, the exit and the agent
    cell ((row, column), or None: not drawn) in this order."""
    cells = np.where(lit, LIT, DARK).astype(np.intp)
    if coin is not None:
        cells[coin] = COIN
    cells[leave] = EXIT
    if agent is not None:
        cells[agent] = AGENT
    return paint(PALETTE, cells, P, out)


class SpotRoomEnv:
    def __init__(self, grid: int = 7, cell: int = 12, spotlights: int = 2, light_steps: int = 2, spot_period: int = 2, health: int = 5,
                 max_episode_steps: int = 64, seed: int = 0, worker_id: int = 0):
        sec = spot_room_section(dict(grid=grid, cell=cell, spotlights=spotlights, light_steps=light_steps, spot_period=spot_period,
                                     health=health, max_episode_steps=max_episode_steps, seed=seed))
        self.grid, self.cell, self.spotlights = sec["grid"], sec["cell"], sec["spotlights"]
        self.light_steps, self.spot_period, self.full_health = sec["light_steps"], sec["spot_period"], sec["health"]
        self.max_episode_steps = sec["max_episode_steps"]
        self.stream = sec["seed"] + int(worker_id)
        self.episode = -1                       # reset() starts episode 0
        self.coin, self.exit, self.spots = (0, 1), (0, 2), ()
        self.row = self.col = self.t = 0
        self.health, self.coin_taken = self.full_health, False

    @property
    def observation_space(self):
        side = self.grid * self.cell
        return SimpleNamespace(shape=(3, side, side), low=0, high=255, dtype=np.uint8)

    @property
    def action_space(self):
        return SimpleNamespace(n=5)

    def lit(self, t=None):
        """[G, G] bool: the cells a spotlight lights at observation index ``t`` (None: the current one)."""
        return lit_cells(self.spots, self.t if t is None else t, self.grid, self.light_steps, self.spot_period)

    def _obs(self):
        G = self.grid
        if self.t < self.light_steps:
            lit, seen = np.ones((G, G), dtype=bool), True
        else:
            lit = self.lit()
            seen = bool(lit[self.row, self.col])
        return render(G, self.cell, lit, None if self.coin_taken else self.coin, self.exit, (self.row, self.col) if seen else None)

    def reset(self, **kwargs):
        self.episode += 1
        (self.row, self.col), self.coin, self.exit, self.spots = episode_draw(self.stream, self.episode, self.grid, self.spotlights)
        self.t, self.health, self.coin_taken = 0, self.full_health, False
        return self._obs()

    def action_masks(self):
        G = self.grid
        return np.array([self.row > 0, self.col < G - 1, self.row < G - 1, self.col > 0, True], dtype=bool)

    def step(self, action):
        a = int(np.asarray(action).reshape(-1)[0])
        if a < 0 or a > 4:
            raise ValueError(f"SpotRoom: action {a} is outside Discrete(5)")
        if self.episode < 0:
            raise RuntimeError("SpotRoom: step() before reset()")
        G = self.grid
        k, success, done, info = 0, 0, False, None
        r, c = self.row + MOVES[a][0], self.col + MOVES[a][1]
        if 0 <= r < G and 0 <= c < G:
            self.row, self.col = r, c
        here = (self.row, self.col)
        if here == self.coin and not self.coin_taken:
            self.coin_taken = True
            k += COIN_TENTHS
        if here == self.exit and self.coin_taken:
            k += EXIT_TENTHS
            success, done, info = 1, True, {}
        elif self.lit(self.t + 1)[here]:
            self.health -= 1
            k -= 1
            if self.health == 0:
                done, info = True, {}
        if not done and self.t + 1 >= self.max_episode_steps:
            done, info = True, {"truncated": True}
        if done:
            tenths = COIN_TENTHS * int(self.coin_taken) + EXIT_TENTHS * success - (self.full_health - self.health)
            info = dict({"reward": float(np.float32(tenths) * REWARD), "length": int(self.t + 1), "success": success}, **info)
        self.t += 1
        return self._obs(), float(np.float32(k) * REWARD), done, info

    def close(self):
        return None
