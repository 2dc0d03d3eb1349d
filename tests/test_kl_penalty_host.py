"""The KL penalty (``kl_penalty``) on the host: the gradients of the two exact KLs (utils.categorical_kl_grad / gaussian_kl_grad) against
central differences of utils.categorical_kl / gaussian_kl, their exact values, the adaptation step (utils.kl_penalty_step), the key's
parser and every refusal, and the config / ABI plumbing.  No GPU.

The central differences: f is evaluated in float64 at x +- h, h = 1e-4, one sample at a time.  The error of (f(x + h) - f(x - h)) / 2h
against f'(x) is at most  h^2 / 6 * max |f'''|  +  (rounding of one f) / h.
  categorical, d / d logit_k: f'' = p_k (1 - p_k), f''' = p_k (1 - p_k)(1 - 2 p_k), |f'''| <= 1 / (6 sqrt 3) for every p_k in [0, 1].
      One f is B sums of terms t_j = p_j - p_old_j + p_old_j d_j >= 0 formed from l_j = logit_j - lse; its rounding is bounded by
      16 eps (2 B + D + 4 B (X + ln A)), D = sum_j p_old_j |d_j| and X = max |logit| over the sample's valid columns, both taken from the
      inputs: every term's own operations (a handful, <= 16 eps of p_j + p_old_j (1 + |d_j|), which sum to 2 B + D) and the error of
      l_j (<= 4 eps (X + ln A + X)) carried through |d t_j / d l_j| = |p_j - p_old_j|, which sums to <= 2 per branch.
  Gaussian, d / d mean: f is quadratic in the mean, f''' = 0.  d / d log_std_a: f''' = -4 (exp(2 d_a) + q^2), bounded on [l - h, l + h]
      by 4 exp(2 h) (exp(2 d_a) + q^2), summed over the samples.  Rounding of one f: 16 eps sum_a (|expm1(2 d_a)| / 2 + |d_a| + q^2 / 2).
Both are computed per case below from the inputs alone; nothing is tuned to the result."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from utils import (categorical_kl, categorical_kl_grad, gaussian_kl, gaussian_kl_grad, kl_penalty_section, kl_penalty_step)  # noqa: E402

H = 1.0e-4
EPS64 = float(np.finfo(np.float64).eps)
M3_CATEGORICAL = 1.0 / (6.0 * np.sqrt(3.0))
LAYOUTS = [(2,), (8,), (3, 3), (2, 1, 5), (31, 32)]


def _offsets(sizes):
    return [sum(sizes[:b]) for b in range(len(sizes))]


def _pack(valid):
    return np.array([sum(1 << j for j in range(valid.shape[1]) if row[j]) for row in valid], dtype=np.int64)


def _log_softmax(x, sizes, valid, dt):
    """The log-softmax of utils.categorical_kl, operation for operation, in ``dt``; -inf on invalid columns."""
    x = np.asarray(x, dtype=dt)
    out = np.full(x.shape, -np.inf, dtype=dt)
    with np.errstate(all="ignore"):
        for off, a in zip(_offsets(sizes), sizes):
            l = np.where(valid[:, off:off + a], x[:, off:off + a], dt(-np.inf))
            mx = l.max(axis=1, keepdims=True)
            out[:, off:off + a] = l - (mx + np.log(np.exp(l - mx).sum(axis=1, keepdims=True, dtype=dt)))
    return out


def _case(sizes, masked, seed=0, N=5):
    """logits, old rows and validity [N, A]: sample 0's first branch has a single valid action (masked); sample 1 has a column with
    old - new < -60 (its old log-prob is about -200); sample 2 has a VALID column whose old log-prob is -inf (a clear mask bit when
    the sample was drawn: the old row is normalised over the other columns); both in the largest branch."""
    rng = np.random.default_rng(1000 * sum(sizes) + 10 * len(sizes) + seed)
    A = sum(sizes)
    logits = rng.normal(size=(N, A)) * 1.5
    valid = np.ones((N, A), dtype=bool)
    if masked:
        valid = rng.random((N, A)) < 0.6
        for off, a in zip(_offsets(sizes), sizes):
            valid[np.arange(N), off + rng.integers(0, a, N)] = True
        valid[0, :sizes[0]] = False
        valid[0, 0] = True
    pert = logits + 0.4 * rng.normal(size=(N, A))
    big = max(range(len(sizes)), key=lambda b: sizes[b])           # (a branch with more than one action)
    off, a = _offsets(sizes)[big], sizes[big]
    valid[1:3, off:off + 2] = True                                  # (samples 1 and 2 keep at least two of its actions)
    old_valid = valid.copy()
    cols = lambda n: off + np.flatnonzero(valid[n, off:off + a])
    if len(cols(1)) > 1:
        pert[1, cols(1)[-1]] = pert[1, cols(1)[:-1]].max() - 200.0
    if len(cols(2)) > 1:
        old_valid[2, cols(2)[0]] = False
    old = _log_softmax(pert, sizes, old_valid, np.float64)
    return logits, old, valid, (_pack(valid) if masked else None)


def _categorical_bounds(logits, old, valid, sizes):
    """Per sample: the bound of the header for d / d logit_k."""
    B, A = len(sizes), logits.shape[1]
    new = _log_softmax(logits, sizes, valid, np.float64)
    with np.errstate(all="ignore"):
        d = np.where(valid & np.isfinite(old), np.abs(old - new), 0.0)
        D = (np.where(np.isfinite(old), np.exp(old), 0.0) * d).sum(axis=1)
    X = np.where(valid, np.abs(logits), 0.0).max(axis=1)
    rounding = 16.0 * EPS64 * (2 * B + D + 4 * B * (X + np.log(A)))
    return M3_CATEGORICAL * H * H / 6.0 + rounding / H


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("sizes", LAYOUTS, ids=lambda s: "x".join(map(str, s)))
def test_categorical_gradient_against_central_differences(sizes, masked):
    logits, old, valid, words = _case(sizes, masked)
    N, A, B = logits.shape[0], logits.shape[1], len(sizes)
    with np.errstate(all="ignore"):
        d = old - _log_softmax(logits, sizes, valid, np.float64)
    assert (d[1][valid[1]] < -60).any(), "the case holds a d < -60 column"
    assert (np.isneginf(old[2]) & valid[2]).any(), "the case holds a valid column with old = -inf under a set mask bit"
    if masked:
        assert valid[0, :sizes[0]].sum() == 1
    grad = categorical_kl_grad(old, logits, sizes, words, np.float64)
    assert grad.shape == (N, A) and grad.dtype == np.float64
    bound = _categorical_bounds(logits, old, valid, sizes)
    worst = 0.0
    for n in range(N):
        w = None if words is None else words[n:n + 1]
        f = lambda x: B * float(categorical_kl(old[n:n + 1], x[None, :], sizes, w, np.float64))       # sum_b KL_nb
        for k in range(A):
            e = np.zeros(A)
            e[k] = H
            num = (f(logits[n] + e) - f(logits[n] - e)) / (2 * H)
            err = abs(num - grad[n, k])
            worst = max(worst, err / bound[n])
            assert err <= bound[n], (n, k, num, grad[n, k], bound[n])
    print(f"[categorical {sizes} masked={masked}] h {H:g}, bounds {bound.min():.2e} .. {bound.max():.2e}, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("A", [1, 3, 8])
def test_gaussian_gradient_against_central_differences(A):
    rng = np.random.default_rng(40 + A)
    N = 6
    mean, old_mean = rng.normal(size=(N, A)), rng.normal(size=(N, A))
    log_std, old_log_std = 0.5 * rng.normal(size=A), 0.5 * rng.normal(size=A)
    d_mean, d_ls = gaussian_kl_grad(old_mean, old_log_std, mean, log_std, np.float64)
    assert d_mean.shape == (N, A) and d_ls.shape == (A,)
    d = old_log_std - log_std
    q = (old_mean - mean) / np.exp(log_std)
    size = (0.5 * np.abs(np.expm1(2 * d))[None, :] + np.abs(d)[None, :] + 0.5 * q * q).sum(axis=1)       # [N]: the terms of one KL_n
    # d / d mean: no truncation (f is quadratic), rounding of one sample's f
    for n in range(N):
        f = lambda m: float(gaussian_kl(old_mean[n:n + 1], old_log_std, m[None, :], log_std, np.float64))
        bound = 16.0 * EPS64 * size[n] / H
        for a in range(A):
            e = np.zeros(A)
            e[a] = H
            num = (f(mean[n] + e) - f(mean[n] - e)) / (2 * H)
            assert abs(num - d_mean[n, a]) <= bound, (n, a, num, d_mean[n, a], bound)
    # d / d log_std: the sum over the samples
    f = lambda ls: N * float(gaussian_kl(old_mean, old_log_std, mean, ls, np.float64))
    for a in range(A):
        e = np.zeros(A)
        e[a] = H
        third = 4.0 * np.exp(2 * H) * (N * np.exp(2 * d[a]) + (q[:, a] ** 2).sum())
        bound = third * H * H / 6.0 + 16.0 * EPS64 * size.sum() / H
        num = (f(log_std + e) - f(log_std - e)) / (2 * H)
        assert abs(num - d_ls[a]) <= bound, (a, num, d_ls[a], bound)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("sizes", LAYOUTS, ids=lambda s: "x".join(map(str, s)))
def test_categorical_exact_values(sizes, masked, dt):
    logits, old, valid, words = _case(sizes, masked, seed=1)
    logits = logits.astype(dt)
    # equal policies: the old rows are the function's own log-softmax, in its own arithmetic -> exactly 0 everywhere
    same = _log_softmax(logits, sizes, valid, dt)
    g0 = categorical_kl_grad(same, logits, sizes, words, dt)
    assert g0.dtype == dt and np.all(g0 == 0), "equal policies"
    g = categorical_kl_grad(old.astype(dt), logits, sizes, words, dt)
    assert np.all(g[~valid] == 0), "masked-out columns"
    eps = float(np.finfo(dt).eps)
    new = _log_softmax(logits, sizes, valid, dt)
    with np.errstate(all="ignore"):
        p_new, p_old = np.where(valid, np.exp(new), 0).astype(np.float64), np.exp(old.astype(dt)).astype(np.float64)
    for off, a in zip(_offsets(sizes), sizes):
        one = valid[:, off:off + a].sum(axis=1) == 1
        # a branch with one valid action: 1 - 1 (where its old row gave that action everything: not the -inf case of sample 2)
        rows = one & (np.where(valid[:, off:off + a], old[:, off:off + a], -np.inf).max(axis=1) == 0)
        assert np.all(g[rows, off:off + a] == 0), "a one-valid-action branch"
        # every branch's gradient sums to sum p - sum p_old, of rounding size
        want = p_new[:, off:off + a].sum(axis=1) - p_old[:, off:off + a].sum(axis=1)
        assert np.all(np.abs(g[:, off:off + a].astype(np.float64).sum(axis=1) - want) <= 4 * a * eps)
        assert np.all(np.abs(want) <= 8 * a * eps), "the rows are normalised: the sum itself is of rounding size"
    if masked:
        assert np.all(g[0, :sizes[0]] == 0), "sample 0's first branch has one valid action"


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_gaussian_exact_values(A, dt):
    rng = np.random.default_rng(7 + A)
    mean, log_std = rng.normal(size=(9, A)).astype(dt), (0.5 * rng.normal(size=A)).astype(dt)
    d_mean, d_ls = gaussian_kl_grad(mean, log_std, mean, log_std, dt)
    assert d_mean.dtype == dt and d_ls.dtype == dt
    assert np.all(d_mean == 0) and np.all(d_ls == 0), "equal policies"
    # equal log-stds: the expm1 part vanishes exactly, d log_std is -sum_n q^2
    old_mean = (mean + rng.normal(size=mean.shape)).astype(dt)
    _, d_ls = gaussian_kl_grad(old_mean, log_std, mean, log_std, dt)
    q = (old_mean - mean) / np.exp(log_std)
    assert np.array_equal(d_ls, (-(q * q)).sum(axis=0, dtype=dt))


RULE = kl_penalty_section({"kl_penalty": {"coef": 0.2, "target": 0.01}})


def test_section_defaults_and_float32_constants():
    assert kl_penalty_section({}) is None
    fixed = kl_penalty_section({"kl_penalty": 0.2})
    assert fixed["coef"] == float(np.float32(0.2)) and fixed["adaptive"] is False and fixed["target"] is None
    assert kl_penalty_section({"kl_penalty": 0})["coef"] == 0.0 and kl_penalty_section({"kl_penalty": {"coef": 0.0}})["adaptive"] is False
    r = RULE
    assert r["adaptive"] and (r["high"], r["low"], r["up"], r["down"]) == (2.0, 0.5, 1.5, 0.5)
    assert r["min"] == float(np.float32(1.0e-4)) and r["max"] == 100.0 and r["coef"] == float(np.float32(0.2))
    assert r["kl_high"] == float(np.float32(2.0 * 0.01)) and r["kl_low"] == float(np.float32(0.5 * 0.01))
    full = {"coef": 0.2, "target": 0.01, "high": 2.0, "low": 0.5, "up": 1.5, "down": 0.5, "min": 1.0e-4, "max": 100.0}
    assert kl_penalty_section({"kl_penalty": full}) == r


def test_step_table_around_limits_and_clamps():
    f32 = np.float32
    hi, lo = f32(RULE["kl_high"]), f32(RULE["kl_low"])
    up, down = f32(1.5), f32(0.5)
    c = f32(0.2)
    table = [
        (c, hi, c, 0),                                              # exactly at the upper limit: nothing moves
        (c, np.nextafter(hi, f32(1)), f32(c * up), 1),
        (c, np.nextafter(hi, f32(0)), c, 0),
        (c, lo, c, 0),                                              # exactly at the lower limit
        (c, np.nextafter(lo, f32(0)), f32(c * down), -1),
        (c, np.nextafter(lo, f32(1)), c, 0),
        (c, f32(0), f32(c * down), -1),
        (c, f32(np.inf), f32(c * up), 1),
        (c, f32(np.nan), c, 0),                                     # a NaN moves nothing
        (f32(80), f32(1), f32(100), 1),                             # 120 -> max
        (f32(100), f32(1), f32(100), 1),                            # at the clamp: decided, the value stays
        (f32(1.5e-4), f32(0), f32(1.0e-4), -1),                     # 7.5e-5 -> min
        (f32(1.0e-4), f32(0), f32(1.0e-4), -1),
    ]
    for coef, kl, want, moved in table:
        got, m = kl_penalty_step(coef, kl, RULE)
        assert isinstance(got, np.float32) and got == want and m == moved, (coef, kl, got, want, m, moved)


def test_steps_from_the_default_start_to_both_clamps():
    c, cuts = np.float32(RULE["coef"]), 0
    while c != np.float32(RULE["min"]):
        c, m = kl_penalty_step(c, 0.0, RULE)
        cuts += 1
        assert m == -1 and cuts < 100
    c, raises = np.float32(RULE["coef"]), 0
    while c != np.float32(RULE["max"]):
        c, m = kl_penalty_step(c, 1.0, RULE)
        raises += 1
        assert m == 1 and raises < 100
    # 0.2 / 2^11 = 9.8e-5 < 1e-4 <= 0.2 / 2^10;   0.2 * 1.5^16 = 131 > 100 >= 0.2 * 1.5^15 = 87.6
    assert (cuts, raises) == (11, 16)


REFUSALS = [
    ({"coef": -0.1}, r"kl_penalty.coef must be a finite number >= 0.*remove the key"),
    ({"coef": float("nan")}, r"kl_penalty.coef must be a finite number >= 0"),
    ({"coef": float("inf")}, r"kl_penalty.coef must be a finite number >= 0"),
    ({"coef": "0.2"}, r"kl_penalty.coef must be a finite number >= 0"),
    ({"coef": True}, r"kl_penalty.coef must be a finite number >= 0"),
    ({"coef": 1e60}, r"kl_penalty.coef must be a finite number >= 0 \(also as a float32\)"),
    ({"target": 0.01}, r"kl_penalty: the section needs `coef`.*add it, or remove the key"),
    ({"coef": 0, "target": 0.01}, r"coef 0 with `target`: a multiplication never leaves 0.*start at a positive coef.*or remove target"),
    ({"coef": 0.2, "target": 0}, r"kl_penalty.target must be a finite number > 0.*remove it for a fixed coefficient"),
    ({"coef": 0.2, "target": float("inf")}, r"kl_penalty.target must be a finite number > 0"),
    ({"coef": 0.2, "target": 0.01, "high": -2}, r"kl_penalty.high must be a finite number > 0.*leave it out for the default 2.0"),
    ({"coef": 0.2, "target": 0.01, "low": 0}, r"kl_penalty.low must be a finite number > 0.*default 0.5"),
    ({"coef": 0.2, "target": 0.01, "up": float("nan")}, r"kl_penalty.up must be a finite number > 0.*default 1.5"),
    ({"coef": 0.2, "target": 0.01, "down": 0}, r"kl_penalty.down must be a finite number > 0.*default 0.5"),
    ({"coef": 0.2, "target": 0.01, "min": 0}, r"kl_penalty.min must be a finite number > 0.*default 0.0001"),
    ({"coef": 0.2, "target": 0.01, "max": "big"}, r"kl_penalty.max must be a finite number > 0.*default 100.0"),
    ({"coef": 0.2, "target": 0.01, "low": 2.0, "high": 2.0}, r"float32\(low \* target\).*must lie below float32\(high \* target\).*choose low < high"),
    ({"coef": 0.2, "target": 0.01, "low": 1.0, "high": 1.0 + 1e-9}, r"must lie below float32\(high \* target\)"),
    ({"coef": 0.2, "target": 0.01, "up": 1.0}, r"kl_penalty.up must be > 1.*default 1.5"),
    ({"coef": 0.2, "target": 0.01, "up": 1.0 + 1e-9}, r"kl_penalty.up must be > 1 \(also as a float32"),
    ({"coef": 0.2, "target": 0.01, "down": 1.0}, r"kl_penalty.down must be < 1.*default 0.5"),
    ({"coef": 0.2, "target": 0.01, "min": 2.0, "max": 1.0}, r"kl_penalty.min = 2.0 must not exceed kl_penalty.max = 1.0.*exchange them"),
    ({"coef": 200.0, "target": 0.01}, r"the start value float32\(coef\) = 200.0 lies outside \[min, max\].*move coef into the range, or widen"),
    ({"coef": 1e-5, "target": 0.01}, r"the start value float32\(coef\).*lies outside \[min, max\]"),
    ({"coef": 0.2, "high": 2.0}, r"\['high'\] belong to the adaptive coefficient and need `target`.*add it, or remove them"),
    ({"coef": 0.2, "min": 0.1, "up": 2.0}, r"\['min', 'up'\] belong to the adaptive coefficient and need `target`"),
    ({"coef": 0.2, "target": 0.01, "factor": 1.5}, r"kl_penalty: unknown keys \['factor'\].*remove them"),
]


@pytest.mark.parametrize("section,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_section_refusals(section, message):
    with pytest.raises(ValueError, match=message):
        kl_penalty_section({"kl_penalty": section})


def test_plain_number_refusals():
    for bad in (-1, float("nan"), "x", True):
        with pytest.raises(ValueError, match=r"kl_penalty.coef must be a finite number >= 0"):
            kl_penalty_section({"kl_penalty": bad})


def test_trainer_level_refusals_and_untouched_neighbours():
    from trainer import check_exact_kl_config, check_kl_estimator_config, check_kl_penalty_config
    assert check_kl_penalty_config({}) is None
    assert check_kl_penalty_config({"kl_penalty": 0.2})["coef"] == float(np.float32(0.2))
    assert check_kl_penalty_config({"kl_penalty": 0.2, "exact_kl": True, "kl_estimator": "analytic"}) is not None
    with pytest.raises(ValueError, match=r"kl_penalty next to exact_kl: false.*contradict.*remove exact_kl, or remove kl_penalty"):
        check_kl_penalty_config({"kl_penalty": 0.2, "exact_kl": False})
    with pytest.raises(ValueError, match=r"kl_penalty next to kl_estimator: k3.*contradict.*remove kl_estimator, or remove kl_penalty"):
        check_kl_penalty_config({"kl_penalty": 0.2, "kl_estimator": "k3"})
    with pytest.raises(ValueError, match=r"kl_penalty in a data-parallel run.*remove the key, or train on one device"):
        check_kl_penalty_config({"kl_penalty": 0.2}, world=2)
    with pytest.raises(ValueError, match=r"kl_penalty: unknown keys \['goal'\]"):
        check_kl_penalty_config({"kl_penalty": {"coef": 0.2, "goal": 0.01}})
    # the two neighbours keep their behaviour with the key next to them
    assert check_exact_kl_config({"kl_penalty": 0.2}) is False and check_exact_kl_config({"kl_penalty": 0.2, "exact_kl": True}) is True
    assert check_kl_estimator_config({"kl_penalty": 0.2}) == "k3"


@pytest.mark.parametrize("new,base,want", [
    ("synthetic_cartpole_kl_penalty.yaml", "synthetic_cartpole.yaml",
     {"coef": 0.2, "target": 0.01, "high": 2.0, "low": 0.5, "up": 1.5, "down": 0.5, "min": 1.0e-4, "max": 100.0}),
    ("synthetic_continuous_kl_penalty.yaml", "synthetic_continuous.yaml", 0.2)])
def test_each_new_config_is_its_base_plus_the_key(new, base, want):
    from trainer import check_kl_penalty_config
    from yaml_parser import YamlParser
    cfgs = os.path.join(PKG, "configs")
    b, n = YamlParser(os.path.join(cfgs, base)).get_config(), YamlParser(os.path.join(cfgs, new)).get_config()
    assert check_kl_penalty_config(n)["adaptive"] is isinstance(want, dict)
    assert n.pop("kl_penalty") == want
    assert n == b


def test_the_evaluator_drops_the_key():
    from evaluation import evaluation_config
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(PKG, "configs", "synthetic_cartpole_kl_penalty.yaml")).get_config()
    out = evaluation_config(cfg, 4, 8)
    assert "kl_penalty" not in out and "exact_kl" not in out and isinstance(cfg["kl_penalty"], dict)


def test_the_abi_grows_additively_at_version_61():
    from etm import lib
    assert lib.ABI_VERSION == 61
    S = lib.SIGNATURES
    names = ("etm_heads_loss_kl", "etm_heads_loss_branched_kl", "etm_heads_loss_gaussian_kl", "etm_ppo_loss_kl")
    for name in names:
        res, args = S[name]
        assert S[name + "_penalty"] == (res, args[:-1] + [lib._P] + args[-1:]), name
    header = open(os.path.join(REPO, "include", "etm_hip.h")).read()
    for name in names:
        assert f" {name}_penalty(" in header, name
        # the declaration is the twin's with `const float *kl_coef` in front of the stream
        decl = lambda n: " ".join(header.split(f"int {n}(", 1)[1].split(");", 1)[0].split())
        twin, mine = decl(name), decl(name + "_penalty")
        assert twin.endswith(", void *stream") and mine == twin[:-len("void *stream")] + "const float *kl_coef, void *stream", name
    if os.path.exists(lib.LIB_PATH):                       # (a built tree: the library exports them and still answers 61)
        handle = lib.load()
        assert handle.etm_abi_version() == 61
        for name in names:
            assert hasattr(handle, name + "_penalty")
