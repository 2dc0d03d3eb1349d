"""What the grid-room image tasks (CueRoom, CommandRoom, PathRoom, SpotRoom) share on the host: the 64-bit mixer and the episode hash every
draw starts from, the geometry the kernel admits, the shared part of a section reader and the painter that turns a table of cell
colours into the frame.  A task's module (cue_room_env.py, command_room_env.py, path_room_env.py, spot_room_env.py) holds what is its own -- the rule,
the palette, the draw, its keys and their checks -- and imports from here, never from another task.  csrc/device_env.hip is laid out
the same way.
"""
import numpy as np

MAX_GRID, MAX_CELL = 31, 64        # what the kernel admits (the tasks' etm_*_supported entries)
_MASK64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """One step of splitmix64 on a 64-bit word (Python integers reduced mod 2^64: what uint64 arithmetic does)."""
    z = (int(x) + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def episode_hash(stream: int, episode: int) -> int:
    """h = splitmix64(splitmix64(stream) + episode) in uint64 arithmetic: the word a task draws episode ``episode`` of the worker
    stream ``stream`` (= seed + worker_id) from."""
    return splitmix64((splitmix64(int(stream) & _MASK64) + int(episode)) & _MASK64)


def encoder_takes(side: int) -> bool:
    """The model's image encoder (8x8 stride 4, 4x4 stride 2, 3x3 stride 1, no padding) leaves at least one position."""
    o1 = (side - 8) // 4 + 1 if side >= 8 else 0
    o2 = (o1 - 4) // 2 + 1 if o1 >= 4 else 0
    return o2 - 2 >= 1


def read_integers(task: str, env_config: dict, keys, defaults: dict, grid_reason: str) -> dict:
    """The first checks of a task's section reader, in their order: unknown sub-keys (``keys`` are the known ones), every key of
    ``defaults`` an integer (filled in where absent), the grid, the cell.  -> {key: value} in the order of ``defaults``."""
    unknown = sorted(set(env_config) - set(keys))
    if unknown:
        raise ValueError(f"environment ({task}): unknown keys {unknown} (known: {sorted(keys)}); remove them")
    sec = {name: env_config.get(name, default) for name, default in defaults.items()}
    for name, v in sec.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"environment.{name} ({task}) must be an integer, got {v!r}")
    G, P = sec["grid"], sec["cell"]
    if G < 3 or G % 2 == 0 or G > MAX_GRID:
        raise ValueError(f"environment.grid must be odd and between 3 and {MAX_GRID} ({grid_reason}), got {G}: "
                         f"use {max(3, min(MAX_GRID, G + 1 - G % 2 if G >= 3 else 3))}")
    if P < 4 or P % 4 != 0 or P > MAX_CELL:
        raise ValueError(f"environment.cell must be a multiple of 4 between 4 and {MAX_CELL} (frames are written in 4-byte words that "
                         f"never straddle two cells), got {P}: use {max(4, min(MAX_CELL, (P + 3) // 4 * 4))}")
    return {name: int(v) for name, v in sec.items()}


def check_encoder_side(G: int, P: int) -> None:
    if not encoder_takes(G * P):
        raise ValueError(f"environment: a {G * P} x {G * P} frame (grid {G} x cell {P}) is too small for the image encoder (8x8/4, 4x4/2, "
                         "3x3/1 need a side of at least 36): raise grid or cell")


def read_device(env_config: dict) -> bool:
    dev = env_config.get("device", False)
    if not isinstance(dev, bool):
        raise ValueError(f"environment.device must be true or false, got {dev!r}")
    return dev


def paint(palette, cells, P: int, out=None):
    """``cells`` [G, G], indices into ``palette`` [n, 3] uint8 -> the frame [3, G P, G P] uint8 (into ``out`` where given)."""
    frame = palette[cells].transpose(2, 0, 1).repeat(P, axis=1).repeat(P, axis=2)      # [G, G, 3] -> [3, G P, G P]
    if out is None:
        return np.ascontiguousarray(frame)
    out[...] = frame
    return out
