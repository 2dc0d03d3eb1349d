"""Exact and float64 restatements of the two running normalisations (``normalize_observations`` / ``normalize_rewards``), shared by
tests/test_normalization_host.py and tests/test_normalization_gpu.py.  No product code is imported here.

* Statistics are compared against EXACT rational arithmetic: a float32 / float64 input is an exact rational, so count, mean and
  M2 = sum (x - mean)^2 of any data set are exact ``fractions.Fraction`` values.
* The fp32 table entries (mean, rstd = 1 / sqrt(M2 / count + epsilon)) are the exact values rounded to float32 (the square root with
  50 decimal digits).
* Applying the table and scaling the rewards are float32 numpy expressions with every operation rounded on its own.
"""
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

# bound on the kernels' float64 triples against the exact ones: the worst case of an ordered double summation of n <= 16,384 terms is
# n * 2^-53 ~ 1.8e-12 relative; 1e-10 is roughly 50 times that
TRIPLE_REL = 1e-10


def exact_triple(values):
    """-> (count, mean, M2) of a 1-D float32 / float64 array, mean and M2 as Fractions.  (float32: the values times 2^149 are
    integers, exactly representable in float64 -- sums of Python integers.)"""
    v = np.asarray(values)
    n = int(v.size)
    if n == 0:
        return 0, Fraction(0), Fraction(0)
    if v.dtype == np.float32:
        ints = [int(i) for i in (v.astype(np.float64) * 2.0 ** 149).tolist()]
        s1, s2 = sum(ints), sum(i * i for i in ints)
        return n, Fraction(s1, n << 149), Fraction(s2 * n - s1 * s1, n << 298)
    assert v.dtype == np.float64
    fr = [Fraction(float(i)) for i in v.tolist()]
    s1, s2 = sum(fr), sum(f * f for f in fr)
    return n, s1 / n, s2 - s1 * s1 / n


def exact_triples_per_feature(x):
    """[R, F] -> list of F exact triples."""
    x = np.asarray(x)
    return [exact_triple(np.ascontiguousarray(x[:, f])) for f in range(x.shape[1])]


def round_to_f32(q):
    """A Fraction or Decimal rounded to float32 (through 50 decimal digits and float64: at most a rounding tie away from the exact
    rounding, which the tests' 1-ulp bound allows)."""
    getcontext().prec = 50
    d = q if isinstance(q, Decimal) else Decimal(q.numerator) / Decimal(q.denominator)
    return np.float32(float(d))


def exact_rstd_f32(count, m2, epsilon):
    """fp32(1 / sqrt(M2 / count + epsilon)) from the exact triple; 1 for an empty one.  ``epsilon`` is the double the config holds."""
    if count == 0:
        return np.float32(1.0)
    getcontext().prec = 50
    var = m2 / count + Fraction(float(epsilon))
    return round_to_f32(Decimal(1) / (Decimal(var.numerator) / Decimal(var.denominator)).sqrt())


def ulps32(a, b):
    """Distance of two float32 arrays in units in the last place (their positions on the ordered line of float32 values)."""
    def line(x):
        i = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(line(a) - line(b))


def triple_error(got, ref, scale):
    """Relative error of a float64 value against an exact Fraction; for a zero reference, the error relative to ``scale``."""
    err = abs(Fraction(float(got)) - ref)
    return float(err / abs(ref)) if ref != 0 else float(err / Fraction(float(scale)))


def merge_float64(a, b):
    """The update of Chan et al. on float64 triples (count, mean, M2), as the issue's rule states it."""
    (na, ma, qa), (nb, mb, qb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    d = mb - ma
    return n, ma + d * nb / n, qa + qb + d * d * na * nb / n


def obs_rule_float64(batches, epsilon, clip):
    """The observation rule restated in float64: the table frozen for batch k is derived from the triple of batches 0 .. k - 1
    (identity for k = 0) -> list of (mean [F], rstd [F], normalised batch) per batch, all float64 except the fp32-rounded table."""
    F = batches[0].shape[1]
    trip = [(0.0, 0.0, 0.0)] * F
    out = []
    for x in batches:
        mean = np.array([np.float32(t[1]) if t[0] else np.float32(0) for t in trip], dtype=np.float32)
        rstd = np.array([np.float32(1.0 / np.sqrt(t[2] / t[0] + epsilon)) if t[0] else np.float32(1) for t in trip], dtype=np.float32)
        out.append((mean, rstd, obs_normalize_f32(x, mean, rstd, clip)))
        x64 = x.astype(np.float64)
        trip = [merge_float64(trip[f], (float(x.shape[0]), float(x64[:, f].mean()), float(((x64[:, f] - x64[:, f].mean()) ** 2).sum())))
                for f in range(F)]
    return out, trip


def obs_normalize_f32(x, mean, rstd, clip):
    """np.clip((x - mean) * rstd, -clip, clip) in float32: subtraction and product each rounded to float32."""
    x, mean, rstd = (np.asarray(a, dtype=np.float32) for a in (x, mean, rstd))
    return np.clip((x - mean) * rstd, np.float32(-clip), np.float32(clip)).astype(np.float32)


def return_recurrence(rewards, dones, carry, gamma):
    """R_t = gamma * R_{t-1} + r_t in float64 (product and sum rounded separately), R = 0 AFTER a step whose done is set, continued
    from ``carry`` [W] -> (R [W, S] float64, the carry after the last step)."""
    r = np.asarray(rewards, dtype=np.float32).astype(np.float64)
    d = np.asarray(dones).astype(bool)
    R = np.array(carry, dtype=np.float64, copy=True)
    g = np.float64(gamma)
    out = np.empty(r.shape, dtype=np.float64)
    for t in range(r.shape[1]):
        R = g * R
        R = R + r[:, t]
        out[:, t] = R
        R = np.where(d[:, t], 0.0, R)
    return out, R


def return_rule_exact(rewards, dones, carry, returns_before, gamma, epsilon, clip):
    """The reward rule on one rollout: the float64 recurrence, the EXACT triple of all returns seen so far (``returns_before``: flat
    float64 array of the earlier rollouts' returns, this rollout's included in the statistics), the scale rounded to float32 and the
    scaled rewards in float32 -> dict(R, carry, count, mean, m2, scale, scaled)."""
    R, carry_out = return_recurrence(rewards, dones, carry, gamma)
    every = np.concatenate([np.asarray(returns_before, dtype=np.float64).reshape(-1), R.reshape(-1)])
    n, mean, m2 = exact_triple(every)
    scale = exact_rstd_f32(n, m2, epsilon)
    scaled = np.clip(np.asarray(rewards, dtype=np.float32) * scale, np.float32(-clip), np.float32(clip)).astype(np.float32)
    return dict(R=R, carry=carry_out, count=n, mean=mean, m2=m2, scale=scale, scaled=scaled, every=every)
