"""Environment front-ends of the trainer (see vec_env.py for the VecEnv protocol)."""


def action_space_shape(space):
    """The action branches of an action space: one per ``nvec`` entry for a MultiDiscrete space, ``(n,)`` for any other
    (Discrete) space -- what the policy builds one head for each (upstream model.py:62)."""
    nvec = getattr(space, "nvec", None)
    if nvec is not None:
        shape = tuple(int(n) for n in nvec)
        if not shape or min(shape) <= 0:
            raise ValueError(f"MultiDiscrete action space with nvec {list(shape)}: every branch needs at least one action")
        return shape
    return (int(space.n),)


def observation_dtype(env_or_space):
    """The dtype of the observations a front-end (``observation_dtype``) or an environment's ``observation_space`` (``dtype``)
    declares, as the trainer keeps them: ``numpy.uint8`` for byte images (byte k stands for float32(k) / float32(255); the frame
    is handed over as it is, nothing divides on the host), ``numpy.float32`` for everything else and where nothing is declared."""
    import numpy as np
    dt = getattr(env_or_space, "observation_dtype", None)
    if dt is None:
        space = getattr(env_or_space, "observation_space", env_or_space)
        dt = getattr(space, "dtype", None)
    try:
        return np.dtype(np.uint8) if dt is not None and np.dtype(dt) == np.uint8 else np.dtype(np.float32)
    except TypeError:
        return np.dtype(np.float32)


class ActionKind:
    """The kind of an action space: ``kind`` is "discrete", "multidiscrete" or "box"; ``shape`` is ``action_space_shape`` for the
    first two and ``(A,)`` for a Box; ``low`` / ``high`` (Box only) are float32 arrays of A bounds."""

    def __init__(self, kind, shape, low=None, high=None):
        self.kind, self.shape, self.low, self.high = kind, tuple(int(a) for a in shape), low, high

    @property
    def is_box(self):
        return self.kind == "box"

    def __repr__(self):
        return f"ActionKind({self.kind!r}, {self.shape})"


def action_space_kind(space):
    """Discrete (``n``), MultiDiscrete (``nvec``) or Box (``low``, ``high`` and a 1-D ``shape``, neither ``n`` nor ``nvec``): an
    ``ActionKind``.  A Box whose shape is not 1-D raises ValueError."""
    if getattr(space, "nvec", None) is not None:
        return ActionKind("multidiscrete", action_space_shape(space))
    if getattr(space, "n", None) is None and hasattr(space, "low") and hasattr(space, "high") and hasattr(space, "shape"):
        import numpy as np
        shape = tuple(int(a) for a in space.shape)
        if len(shape) != 1 or shape[0] <= 0:
            raise ValueError(f"Box action space of shape {shape}: only 1-D Box spaces (one vector of A actions) are supported")
        A = shape[0]
        low = np.broadcast_to(np.asarray(space.low, dtype=np.float32), (A,)).copy()
        high = np.broadcast_to(np.asarray(space.high, dtype=np.float32), (A,)).copy()
        if not np.all(low <= high):
            raise ValueError(f"Box action space with low {low.tolist()} above high {high.tolist()}")
        return ActionKind("box", (A,), low, high)
    return ActionKind("discrete", action_space_shape(space))


MAX_MASKED_ACTIONS = 63      # columns of the concatenated policy head that one 64-bit action-mask word describes


def pack_action_masks(masks, out=None):
    """bool [W, sum A_b] (sb3-contrib's flat ``action_masks()`` layout: the branches' actions side by side) -> uint64 [W]: bit j of
    worker w's word is set when column j is allowed.  The one place that packs; at most 63 columns."""
    import numpy as np
    m = np.asarray(masks)
    if m.ndim == 1:
        m = m[None, :]
    if m.ndim != 2 or m.shape[1] < 1 or m.shape[1] > MAX_MASKED_ACTIONS:
        raise ValueError(f"action masks are bool [W, A] with 1 <= A <= {MAX_MASKED_ACTIONS} (all branches together), got {m.shape}")
    bits = np.uint64(1) << np.arange(m.shape[1], dtype=np.uint64)
    words = (m.astype(bool).astype(np.uint64) * bits[None, :]).sum(axis=1, dtype=np.uint64)
    if out is None:
        return words
    out.view(np.uint64)[...] = words
    return out


def branch_bit_masks(branches):
    """uint64 [B]: the bits [off_b, off_b + A_b) of branch b in a mask word."""
    import numpy as np
    out, off = np.zeros(len(branches), dtype=np.uint64), 0
    for b, a in enumerate(branches):
        out[b] = ((1 << int(a)) - 1) << off
        off += int(a)
    return out


def empty_mask_branches(words, branches, bits=None):
    """bool [W, B]: branch b of worker w has no allowed action in ``words`` (uint64 / int64 [W]) -- one vectorised test over the
    workers and branches.  ``bits``: ``branch_bit_masks(branches)`` when the caller keeps it."""
    import numpy as np
    w = np.asarray(words)
    w = w.view(np.uint64) if w.dtype == np.int64 else w.astype(np.uint64, copy=False)
    bits = branch_bit_masks(branches) if bits is None else bits
    return (w[:, None] & bits[None, :]) == 0


def valid_action_share(words, total):
    """Mean share of set bits among the ``total`` columns over all words (any shape)."""
    import numpy as np
    w = np.asarray(words).reshape(-1)
    w = w.view(np.uint64) if w.dtype == np.int64 else w.astype(np.uint64)
    w = w & np.uint64((1 << int(total)) - 1)
    bits = np.unpackbits(w.view(np.uint8)).sum()
    return float(bits) / float(max(w.size, 1) * int(total))
