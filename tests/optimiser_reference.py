"""The optimiser step (global-norm clipping + AdamW) and the monitored gradient norms restated in plain numpy, shared by
tests/test_optimiser_host.py and tests/test_optimiser_vs_float64.py.  No product code is imported here.

* ``step64``: the definition in float64 -- ``torch.nn.utils.clip_grad_norm_`` followed by one step of torch's single-tensor AdamW.
  The values the device holds as float32 (``lr``, ``max_norm``, ``grad_scale``: a device float and two ``float`` arguments of the C
  entry points) are taken as those float32 values, widened exactly.
* ``step32``: the same formulas in numpy float32, every product, sum, quotient and root rounded on its own, the scalars formed as
  doubles and then rounded to float32 as the header of csrc/optim.hip states them.  The first moment is ``m + (1 - b1) * (g - m)``
  for every ``b1`` (torch's ``lerp_`` switches to the mirrored form ``g - (g - m) * b1`` at a weight >= 0.5, which differs by a
  rounding in float32 and by nothing that 1e-12 sees in float64).
* ``group_norms64``: sqrt(member @ per-segment sums of squares).
* The inputs of the GPU tests (``arena``, ``element_cases``): the host test measures ``step32`` against ``step64`` on exactly these.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # half a unit in the last place of float32, relative
# step32 against step64 on the GPU test's one-step inputs, max |dp| / (|p| + |update|): measured by tests/test_optimiser_host.py (which
# prints it and fails if it is exceeded) -- the reference's own float32 error, on the CPU, no kernel involved
E_REF = 2.95e-7                     # measured 2.946490e-07 = 4.943 * 2^-24 (n 4100, lr 1.0, step 12344, no clipping, default hyper-parameters)

NS = (4, 1020, 1024, 1028, 4092, 4096, 4100, 40004)
N_PARTIALS = (1, 3, 255, 256, 257, 1024, 4096)
N_CAP = 4 * (2048 * 1024 + 257)     # the smallest arena at which a thread of the AdamW launch (2048 x 256 threads) walks a fifth round
MAX_NORMS = {"clipping": 0.5, "not clipping": 1.0e6, "off": 0.0}       # (every arena's norm is >= sqrt(15): 0.5 clips)
STEPS = (0, 9, 12344, 10 ** 7)
LRS = (3e-4, 1.0, 0.0)
HYPERS = tuple(dict(weight_decay=wd, betas=b, eps=e) for wd in (0.0, 0.01) for b in ((0.9, 0.999), (0.5, 0.9)) for e in (1e-8, 1e-5))
DEFAULT = dict(weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
CROSS_SHAPE = (4100, 3)             # (n, n_partial) of the full cross of max_norm x step x hyper-parameters x lr


def f32(x):
    """The double that equals float32(x)."""
    return float(F32(x))


def _scalars64(t, lr, betas, eps, wd):
    lr = f32(lr)
    b1, b2 = float(betas[0]), float(betas[1])
    return dict(keep=1.0 - lr * wd, w1=1.0 - b1, b2=b2, w2=1.0 - b2, bc2_sqrt=float(np.sqrt(1.0 - b2 ** t)), neg_step=-(lr / (1.0 - b1 ** t)),
                eps=float(eps))


def step64(p, g, m, v, t, lr, betas, eps, wd, max_norm, grad_scale):
    """One clip-and-AdamW step in float64 from float32 inputs widened exactly; ``t`` is the number of this step (1 for the first).
    -> dict(p, g, m, v, total, coef, update): the arena holds gradient / grad_scale; total = sqrt(sum g^2) * grad_scale;
    coef = min(max_norm / (total + 1e-6), 1) for max_norm > 0, else 1 -- a NaN total gives a NaN coef, the rule of
    ``torch.clamp(coef, max=1)`` -- times grad_scale; ``update`` is the AdamW increment -lr / (1 - b1^t) * m' / denom."""
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))   # (float64 state of an earlier step passes as it is)
    s = _scalars64(int(t), lr, betas, eps, float(wd))
    max_norm, grad_scale = f32(max_norm), f32(grad_scale)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        total = np.sqrt(np.sum(g * g)) * grad_scale
        coef = np.float64(1.0)
        if max_norm > 0.0:
            coef = np.minimum(max_norm / (total + 1e-6), 1.0)              # (np.minimum hands a NaN on)
        coef = coef * grad_scale
        g2 = g * coef
        p2 = p * s["keep"]
        m2 = m + s["w1"] * (g2 - m)
        v2 = s["b2"] * v + s["w2"] * g2 * g2
        denom = np.sqrt(v2) / s["bc2_sqrt"] + s["eps"]
        update = s["neg_step"] * m2 / denom
        p2 = p2 + update
    return dict(p=p2, g=g2, m=m2, v=v2, total=float(total), coef=float(coef), update=update)


def step32(p, g, m, v, t, lr, betas, eps, wd, max_norm, grad_scale):
    """The step of ``step64`` in float32 arithmetic, each operation rounded on its own -> dict(p, g, m, v, total, coef), float32."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    s = {k: F32(x) for k, x in _scalars64(int(t), lr, betas, eps, float(wd)).items()}
    max_norm, grad_scale = F32(max_norm), F32(grad_scale)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        total = F32(np.sqrt(np.sum(g * g, dtype=F32)) * grad_scale)
        coef = F32(1.0)
        if max_norm > F32(0.0):
            coef = np.minimum(F32(max_norm / F32(total + F32(1e-6))), F32(1.0))
        coef = F32(coef * grad_scale)
        g2 = g * coef
        p2 = p * s["keep"]
        m2 = m + s["w1"] * (g2 - m)
        v2 = v * s["b2"] + (s["w2"] * g2) * g2
        denom = np.sqrt(v2) / s["bc2_sqrt"] + s["eps"]
        p2 = p2 + (s["neg_step"] * m2) / denom
    out = dict(p=p2, g=g2, m=m2, v=v2)
    assert all(a.dtype == F32 for a in out.values())
    return dict(out, total=total, coef=coef)


def group_norms64(flat, seg_start, seg_len, member):
    """sqrt(member @ q), q[s] = sum of squares of flat[seg_start[s] : seg_start[s] + seg_len[s]] in float64 -> (norms [G], q [S])."""
    flat = np.asarray(flat, dtype=F32).astype(np.float64)
    q = np.array([np.sum(flat[a: a + n] ** 2) for a, n in zip(np.asarray(seg_start).tolist(), np.asarray(seg_len).tolist())], dtype=np.float64)
    return np.sqrt(np.asarray(member, dtype=np.float64) @ q), q


def scale_of(p_start, ref):
    """|p| + |update|: what the parameter error of one step is measured against (``ref`` of ``step64``)."""
    return np.abs(np.asarray(p_start).astype(np.float64)) + np.abs(ref["update"])


def parameter_ratio(p_start, got, ref):
    """max over the elements of |got - ref.p| / (|p| + |update|), NaN-free elements only."""
    err = np.abs(np.asarray(got).astype(np.float64) - ref["p"])
    ok = np.isfinite(ref["p"])
    return float((err[ok] / np.maximum(scale_of(p_start, ref)[ok], 1e-300)).max()) if ok.any() else 0.0


# ------------------------------------------------------------------ the inputs of the GPU tests
def arena(n, seed, span=3, mixed=False):
    """-> dict(p, g, m, v) float32 [n]: g integers in [-span, span] whose first element and last four are non-zero (a dropped float4
    then shows in the norm), p, m normal, v >= 0, and about one element in sixteen with m = v = 0.

    Where g != 0 the first moment has the sign of g (``mixed``: its own sign).  m' = (1 - w) m + w g' loses every leading digit it has
    where the two terms cancel; the increment then carries an error of 2^-24 |m| / |m'| of ITSELF, in any float32 evaluation of the
    formula, and |p| + |update| does not scale with that: with signs drawn freely the reference's own ratio (step32 against step64)
    measures 172 * 2^-24, decided by the few elements in 4100 with |m'| < |m| / 100 and a small |p|.  With equal signs m' lies between
    its terms and every operation of the step is well conditioned.  The bits of g, m and v are asserted on ``mixed`` arenas too."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-span, span + 1, size=n).astype(F32)
    g[0] = -span
    g[-4:] = np.array([1, -2, 3, -1], dtype=F32).clip(-span, span)
    p = (rng.standard_normal(n) * 0.5).astype(F32)
    m = (rng.standard_normal(n) * 0.1).astype(F32)
    if not mixed:
        m = np.where(g != 0, np.abs(m) * np.sign(g), m).astype(F32)
    v = np.square(rng.standard_normal(n) * 0.1).astype(F32)
    fresh = rng.random(n) < 1.0 / 16.0
    m[fresh] = 0.0
    v[fresh] = 0.0
    return dict(p=p, g=g, m=m, v=v)


def exact_sumsq(g):
    """The exact integer sum of squares of an integer-valued gradient."""
    gi = np.asarray(g).astype(np.int64)
    assert np.array_equal(gi.astype(F32), g)
    return int(np.sum(gi * gi))


def shape_cases():
    """Every (n, n_partial) of the grid with the remaining parameters walking through their values, so that each value of each meets
    several shapes -> list of dict(n, n_partial, seed, max_norm, step, lr, grad_scale, **hyper)."""
    out = []
    modes = list(MAX_NORMS.values())
    for i, n in enumerate(NS):
        for j, n_partial in enumerate(N_PARTIALS):
            k = i * len(N_PARTIALS) + j
            out.append(dict(n=n, n_partial=n_partial, seed=1000 + k, span=3, max_norm=modes[k % 3], step=STEPS[(k // 3) % 4],
                            lr=LRS[(k // 2) % 3], grad_scale=1.0, **HYPERS[k % 8]))
    return out


def cap_case():
    return dict(n=N_CAP, n_partial=1024, seed=77, span=1, max_norm=MAX_NORMS["clipping"], step=9, lr=3e-4, grad_scale=1.0, **DEFAULT)


def cross_cases(mode, lr):
    """step x hyper-parameters at one max_norm mode and one lr, on CROSS_SHAPE."""
    n, n_partial = CROSS_SHAPE
    return [dict(n=n, n_partial=n_partial, seed=2000 + 10 * a + b, span=3, max_norm=MAX_NORMS[mode], step=step, lr=lr, grad_scale=1.0, **hyper)
            for a, step in enumerate(STEPS) for b, hyper in enumerate(HYPERS)]


def element_cases():
    """Every case in which the GPU test compares parameters with ``step64`` after one step on integer gradients."""
    return shape_cases() + [c for mode in MAX_NORMS for lr in LRS for c in cross_cases(mode, lr)] + [cap_case()]


def reference_pair(case, data=None):
    """(arena, step32 result, step64 result) of one case."""
    a = data if data is not None else arena(case["n"], case["seed"], case["span"])
    args = (a["p"], a["g"], a["m"], a["v"], case["step"] + 1, case["lr"], case["betas"], case["eps"], case["weight_decay"], case["max_norm"],
            case["grad_scale"])
    return a, step32(*args), step64(*args)
