"""Host side of checkpoint and resume (absent upstream, whose ``models/<run_id>.nn`` holds the model's state dict and the config and
nothing that continues a run).  Pure python + numpy: no device, no torch.

A training checkpoint ``models/<run_id>.ckpt`` is a pickle of ONE dict of numpy arrays, python scalars, lists and dicts (never a
tensor), with ``format: 1``.  It is written next to the unchanged ``.nn`` file by ``PPOTrainer.save_checkpoint`` and read by
``PPOTrainer.load_checkpoint`` / ``PPOTrainer(..., resume=path)``; what it holds is listed there.  Every arena in it travels with its
digest -- the four words of ``etm_arena_digest`` (csrc/arena_digest.hip), which ``digest_numpy`` computes on the host -- so a file is
verified before a byte of it is uploaded, and the upload is verified on the device afterwards.
"""
import os
import pickle

import numpy as np

FORMAT = 1
SEGMENT_STRIDE = 1_000_000

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_MIX1 = np.uint64(0xBF58476D1CE4E5B9)
_MIX2 = np.uint64(0x94D049BB133111EB)


def digest_numpy(x, offset: int = 0):
    """The four words of ``etm_arena_digest`` over the float32 array ``x`` taken as raw bits b_i, as python ints:
    (sum over i of mix(i * 0x9E3779B97F4A7C15 + b_i) mod 2^64, number of Inf / NaN words, bit pattern of the largest finite |x| or 0,
    number of words).  ``offset``: the index of ``x[0]`` -- the first word of a concatenation is the sum (mod 2^64) of its parts'
    first words, each computed with the offset of its part (what the kernel's per-workgroup partial words rely on)."""
    x = np.ascontiguousarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"digest_numpy takes float32, got {x.dtype}")
    b = x.reshape(-1).view(np.uint32)
    n = int(b.size)
    z = np.arange(n, dtype=np.uint64) + np.uint64(int(offset) % (1 << 64))       # uint64 arrays wrap mod 2^64
    z = z * _GOLDEN + b.astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= _MIX1
    z ^= z >> np.uint64(27)
    z *= _MIX2
    z ^= z >> np.uint64(31)
    mag = b & np.uint32(0x7FFFFFFF)
    bad = mag >= np.uint32(0x7F800000)
    finite = mag[~bad]
    return (int(np.sum(z, dtype=np.uint64)) if n else 0, int(np.count_nonzero(bad)), int(finite.max()) if finite.size else 0, n)


def write_checkpoint(path: str, state: dict) -> None:
    """``state`` (numpy arrays, python scalars, lists, dicts; ``format`` is set here) -> ``path``, through ``path + ".tmp"`` and
    ``os.replace``: never a torn file at the final path (as ``_save_model`` writes the ``.nn`` file)."""
    state = dict(state, format=FORMAT)
    _refuse_tensors(state, "state")
    try:
        with open(path + ".tmp", "wb") as f:
            pickle.dump(state, f, protocol=pickle.HIGHEST_PROTOCOL)
            f.flush()
            os.fsync(f.fileno())
    except BaseException:
        if os.path.exists(path + ".tmp"):
            os.remove(path + ".tmp")
        raise
    os.replace(path + ".tmp", path)


def read_checkpoint(path: str) -> dict:
    """The dict ``write_checkpoint`` wrote.  A truncated or foreign file raises ValueError; so does another ``format``."""
    try:
        with open(path, "rb") as f:
            state = pickle.load(f)
    except (pickle.UnpicklingError, EOFError, AttributeError, ImportError, IndexError, ValueError) as exc:
        raise ValueError(f"{path}: not a readable training checkpoint ({type(exc).__name__}: {exc})") from exc
    return check_format(state, path)


def check_format(state, what: str = "checkpoint") -> dict:
    if not isinstance(state, dict) or "format" not in state:
        raise ValueError(f"{what}: not a training checkpoint (a .ckpt file holds one dict with a `format` entry; the .nn file next to "
                         "it is the model for evaluate.py / enjoy.py)")
    if state["format"] != FORMAT:
        raise ValueError(f"{what}: checkpoint format {state['format']!r}, this build reads format {FORMAT}")
    return state


def _refuse_tensors(obj, where):
    if isinstance(obj, dict):
        for k, v in obj.items():
            _refuse_tensors(v, f"{where}[{k!r}]")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _refuse_tensors(v, f"{where}[{i}]")
    elif type(obj).__module__.split(".")[0] == "torch":
        raise TypeError(f"write_checkpoint: {where} is a {type(obj).__name__}; a checkpoint holds numpy arrays and python values only")


def config_differences(saved, current, prefix: str = "") -> list:
    """The key paths (``a.b.c``) at which the two (nested) configs differ, sorted; a key present on one side only counts."""
    out = []
    if isinstance(saved, dict) and isinstance(current, dict):
        for k in sorted(set(saved) | set(current), key=str):
            path = f"{prefix}.{k}" if prefix else str(k)
            if k not in saved or k not in current:
                out.append(path)
            else:
                out.extend(config_differences(saved[k], current[k], path))
    elif isinstance(saved, (list, tuple)) and isinstance(current, (list, tuple)):
        if list(saved) != list(current):
            out.append(prefix)
    elif saved != current:
        out.append(prefix)
    return out


def segment_first_worker_id(base: int, segment: int) -> int:
    """First worker id of the environments of training segment ``segment`` (the number of resumes so far): ``base + segment *
    1_000_000``.  The seeded streams of a resumed run are then not those of the segment before it, and -- the trainer admits at most
    65,536 workers -- no segment's ids meet another's or, from segment 1 on, the evaluator's default ids (100000 onwards)."""
    if int(segment) < 0:
        raise ValueError("segment must be >= 0")
    return int(base) + int(segment) * SEGMENT_STRIDE


def check_checkpoint_config(config: dict, world: int = 1, resume: bool = False):
    """The optional key ``checkpoint_interval`` -> its value (an integer >= 1) or None when absent (write the ``.nn`` file once, at the
    end, as ever).  Refused, before anything is built: a value that is no integer >= 1; the key, or a resume (``resume``), in a
    data-parallel run (``world`` > 1): generator states and environments are per rank, and per-rank files and their agreement are not
    built."""
    k = config.get("checkpoint_interval")
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
        raise ValueError(f"checkpoint_interval: {k!r} (need an integer >= 1, or leave the key out: one model file at the end)")
    on = [name for name, flag in (("checkpoint_interval", k is not None), ("resume", bool(resume))) if flag]
    if on and int(world) > 1:
        raise ValueError(f"{' / '.join(on)} in a data-parallel run: generator states and environments are per rank (per-rank checkpoint "
                         "files and their agreement are not built); remove it, or train on one device")
    return k
