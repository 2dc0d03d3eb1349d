"""The exact categorical KL (``exact_kl: true``) on the host, no GPU: ``utils.categorical_kl`` against the plain definition in 50-digit
arithmetic, its ``d < -60`` case, the masked forms and the branch-mean convention, every refusal of ``check_exact_kl_config``, the new
config file, the evaluator's context and the additive ABI."""
import os
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

getcontext().prec = 50


def _exact_old_rows():
    """Hand-picked old distributions as exact fractions (each row sums to 1 exactly) with the branch layout and the new logits."""
    F = Fraction
    return [
        ((2,), [F(1, 2), F(1, 2)], [0.25, -0.5]),
        ((3,), [F(1, 4), F(1, 4), F(1, 2)], [1.0, 0.0, -1.0]),
        ((3,), [F(1, 1024), F(1023, 2048), F(1023, 2048)], [3.0, -2.0, 0.5]),
        ((2, 3), [F(1, 8), F(7, 8), F(1, 3), F(1, 3), F(1, 3)], [0.1, 0.2, -0.3, 0.4, 2.5]),
        ((4, 1, 3), [F(1, 10), F(2, 10), F(3, 10), F(4, 10), F(1), F(1, 16), F(5, 16), F(10, 16)], [0.0, 1.5, -1.5, 0.75, 9.0, -4.0, 0.0, 4.0]),
    ]


def _plain_definition_50_digits(sizes, p_old, logits):
    """sum_b sum_j p_old (log p_old - log p_new) / B with Decimal at 50 digits; log p_old is the logarithm of the exact fraction."""
    total, off = Decimal(0), 0
    for a in sizes:
        lg = [Decimal(repr(float(x))) for x in logits[off:off + a]]
        lse = sum(x.exp() for x in lg).ln()
        for j in range(a):
            po = Decimal(p_old[off + j].numerator) / Decimal(p_old[off + j].denominator)
            total += po * (po.ln() - (lg[j] - lse))
        off += a
    return total / len(sizes)


def test_categorical_kl_float64_matches_the_plain_definition_at_50_digits():
    from utils import categorical_kl
    for sizes, p_old, logits in _exact_old_rows():
        old = np.log(np.array([float(p) for p in p_old], dtype=np.float64))[None, :]
        got = float(categorical_kl(old, np.asarray(logits, dtype=np.float64)[None, :], sizes))
        # the reference takes the float64 old log-probs as they are handed over (their rounding is the caller's, not the rule's)
        total, off = Decimal(0), 0
        for a in sizes:
            lg = [Decimal(repr(float(x))) for x in logits[off:off + a]]
            lse = sum(x.exp() for x in lg).ln()
            for j in range(a):
                lo = Decimal(repr(float(old[0, off + j])))
                total += lo.exp() * (lo - (lg[j] - lse))
            off += a
        want = total / len(sizes)
        # `sum p_old (old - new)` of the handed-over numbers: the rule adds sum (p_new - p_old), which is 0 only up to the rounding
        # of the old log-probs (sum exp(old) = 1 +- a few 1e-16)
        assert abs(Decimal(got) - want) <= Decimal("1e-15") * max(Decimal(1), abs(want)), (sizes, got, want)
        exact = _plain_definition_50_digits(sizes, p_old, logits)
        assert abs(Decimal(got) - exact) <= Decimal("1e-15") * max(Decimal(1), abs(exact)), (sizes, got, exact)
        assert got >= 0.0


def _log_softmax(x, sizes, dtype, valid=None):
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=dt)
    out, off = np.full_like(x, dt(-np.inf)), 0
    for a in sizes:
        v = np.ones((x.shape[0], a), dtype=bool) if valid is None else valid[:, off:off + a]
        s = np.where(v, x[:, off:off + a], dt(-np.inf))
        m = s.max(axis=1, keepdims=True)
        out[:, off:off + a] = s - (m + np.log(np.exp(s - m).sum(axis=1, keepdims=True, dtype=dt)))
        off += a
    return out


def test_equal_policies_give_exactly_zero_in_float32():
    from utils import categorical_kl
    rng = np.random.default_rng(0)
    for sizes in ((3,), (2, 3), (4, 1, 3), (63,), (31, 32)):
        lg = (3.0 * rng.normal(size=(257, sum(sizes)))).astype(np.float32)
        got = categorical_kl(_log_softmax(lg, sizes, np.float32), lg, sizes, dtype=np.float32)
        assert got.dtype == np.float32 and got.view(np.uint32) == 0, (sizes, got)


def test_never_negative_on_ten_thousand_random_rows():
    from utils import categorical_kl
    rng = np.random.default_rng(1)
    sizes = (2, 3)
    for dtype in (np.float64, np.float32):
        lg = (2.0 * rng.normal(size=(10000, 5))).astype(dtype)
        old = _log_softmax(lg + 0.3 * rng.normal(size=lg.shape).astype(dtype), sizes, dtype)
        rows = np.array([categorical_kl(old[i:i + 1], lg[i:i + 1], sizes, dtype=dtype) for i in range(lg.shape[0])])
        assert (rows >= 0).all(), (dtype, rows.min())
        assert abs(float(categorical_kl(old, lg, sizes, dtype=dtype)) - float(rows.astype(np.float64).mean())) <= 1e-5


def test_the_limit_case_below_minus_sixty():
    from utils import categorical_kl
    # one branch of two actions: the old policy gave action 0 the log-prob -200 (p = e^-200), the current one -0.1
    l0 = -0.1
    l1 = float(np.log(-np.expm1(l0)))
    logits = np.array([[l0, l1]])
    old = np.array([[-200.0, float(np.log1p(-np.exp(-200.0)))]])
    got = float(categorical_kl(old, logits, (2,)))
    new = _log_softmax(logits, (2,), np.float64)
    d1 = old[0, 1] - new[0, 1]
    want = np.exp(new[0, 0]) + np.exp(old[0, 1]) * (np.expm1(-d1) + d1)       # t_0 = exp(l_0): the limit; t_1: the general term
    assert got == pytest.approx(want, rel=1e-15) and got > 0.9
    # the dropped part is below e^-60 |d|
    full = np.exp(-200.0) * (-200.0 - new[0, 0]) + np.exp(old[0, 1]) * (old[0, 1] - new[0, 1])
    assert abs(got - full) < 1e-12
    # -inf (a probability of exactly zero) takes the same case
    old[0, 0] = -np.inf
    old[0, 1] = 0.0
    assert np.isfinite(categorical_kl(old, logits, (2,)))
    # finite results at logits of +-1e4, in both directions and both types
    for dtype in (np.float64, np.float32):
        big = np.array([[1e4, -1e4, 0.0], [-1e4, 1e4, 0.0]], dtype=dtype)
        for old_src, new_src in ((big, big[::-1]), (big, big), (big, np.zeros_like(big))):
            got = categorical_kl(_log_softmax(old_src, (3,), dtype), new_src, (3,), dtype=dtype)
            assert np.isfinite(got) and got >= 0, (dtype, got)


def _words(valid):
    return np.array([sum(1 << j for j in range(valid.shape[1]) if row[j]) for row in valid], dtype=np.int64)


def test_masked_columns_are_skipped_and_one_valid_action_gives_zero():
    from utils import categorical_kl
    rng = np.random.default_rng(2)
    sizes = (4, 1, 3)
    N, A = 64, 8
    valid = rng.random((N, A)) < 0.6
    valid[:, 4] = True
    valid[np.arange(N), rng.integers(0, 4, N)] = True
    valid[np.arange(N), 5 + rng.integers(0, 3, N)] = True
    lg = rng.normal(size=(N, A))
    old = _log_softmax(lg + 0.5 * rng.normal(size=lg.shape), sizes, np.float64, valid)
    assert np.isneginf(old[~valid]).all()
    got = float(categorical_kl(old, lg, sizes, _words(valid)))
    # the plain definition over the valid columns, per branch, mean over samples and branches
    new = _log_softmax(lg, sizes, np.float64, valid)
    want = np.where(valid, np.exp(old) * (np.where(valid, old, 0.0) - np.where(valid, new, 0.0)), 0.0).sum() / (N * len(sizes))
    assert got == pytest.approx(want, rel=1e-12, abs=1e-15)
    # garbage at the masked columns changes nothing: they are skipped, not multiplied
    lg2, old2 = lg.copy(), old.copy()
    lg2[~valid] = 1e30
    old2[~valid] = np.nan
    assert float(categorical_kl(old2, lg2, sizes, _words(valid))) == got
    # a constant mask is the unmasked rule on the compacted branches
    keep = np.array([True, False, True, True, True, False, True, True])
    const = np.broadcast_to(keep, (N, A))
    oldc = _log_softmax(lg + 0.2, sizes, np.float64, const)
    a = float(categorical_kl(oldc, lg, sizes, _words(const)))
    b = float(categorical_kl(oldc[:, keep], lg[:, keep], (3, 1, 2)))
    assert a == b
    # a branch with one valid action contributes exactly 0: here every branch has one
    one = np.zeros((N, A), dtype=bool)
    one[:, [1, 4, 7]] = True
    old1 = _log_softmax(lg, sizes, np.float64, one)
    assert float(categorical_kl(old1, lg + rng.normal(size=lg.shape), sizes, _words(one))) == 0.0
    with pytest.raises(ValueError, match="without a valid action"):
        categorical_kl(old, lg, sizes, np.zeros(N, dtype=np.int64))


def test_the_statistic_is_the_mean_over_samples_and_branches():
    from utils import categorical_kl
    rng = np.random.default_rng(3)
    lg = rng.normal(size=(50, 5))
    old = _log_softmax(rng.normal(size=(50, 5)), (2, 3), np.float64)
    both = float(categorical_kl(old, lg, (2, 3)))
    first = float(categorical_kl(old[:, :2], lg[:, :2], (2,)))
    second = float(categorical_kl(old[:, 2:], lg[:, 2:], (3,)))
    assert both == pytest.approx((first + second) / 2, rel=1e-14)            # the joint KL of a sample's branches is B times the statistic
    with pytest.raises(ValueError, match="old_logps and logits"):
        categorical_kl(old, lg, (2, 2))


# ------------------------------------------------------------------ the key
def test_exact_kl_section_and_every_refusal_of_the_config_check():
    from trainer import check_exact_kl_config, check_kl_estimator_config
    from utils import exact_kl_section
    assert exact_kl_section({}) is False and exact_kl_section({"exact_kl": False}) is False and exact_kl_section({"exact_kl": True}) is True
    assert check_exact_kl_config({}) is False and check_exact_kl_config({"exact_kl": False, "kl_estimator": "k3"}) is False
    for box in (False, True):
        assert check_exact_kl_config({"exact_kl": True}, box) is True
    assert check_exact_kl_config({"exact_kl": True, "kl_estimator": "analytic"}, True) is True
    for bad in (1, 0, "true", "yes", None, 1.0, [True]):
        with pytest.raises(ValueError, match=r"exact_kl must be true or false.*write `exact_kl: true`.*or remove the key"):
            check_exact_kl_config({"exact_kl": bad})
    with pytest.raises(ValueError, match=r"exact_kl: true next to kl_estimator: k3.*contradict.*remove kl_estimator.*or remove exact_kl"):
        check_exact_kl_config({"exact_kl": True, "kl_estimator": "k3"})
    with pytest.raises(ValueError, match=r"exact_kl: true in a data-parallel run.*remove the key, or train on one device"):
        check_exact_kl_config({"exact_kl": True}, False, world=2)
    # check_kl_estimator_config keeps its behaviour; its categorical refusal now also names the new key, behind the old wording
    assert check_kl_estimator_config({"exact_kl": True}) == "k3"
    with pytest.raises(ValueError, match=r"analytic without a Box .*categorical policies keep k3: remove the key, or replace it with `exact_kl: true`"):
        check_kl_estimator_config({"kl_estimator": "analytic"}, False)
    with pytest.raises(ValueError, match=r"kl_estimator must be one of \['k3', 'analytic'\]"):
        check_kl_estimator_config({"kl_estimator": "exact"})


def test_the_new_config_is_its_base_plus_the_key():
    from yaml_parser import YamlParser
    cfgs = os.path.join(PKG, "configs")
    base = YamlParser(os.path.join(cfgs, "synthetic_cartpole_target_kl.yaml")).get_config()
    new = YamlParser(os.path.join(cfgs, "synthetic_cartpole_target_kl_exact.yaml")).get_config()
    assert new.pop("exact_kl") is True
    assert new == base


def test_the_evaluator_drops_the_key():
    from evaluation import evaluation_config
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(PKG, "configs", "synthetic_cartpole_target_kl_exact.yaml")).get_config()
    out = evaluation_config(cfg, 4, 8)
    assert "exact_kl" not in out and "kl_estimator" not in out and cfg["exact_kl"] is True


def test_the_abi_grows_additively_at_version_61():
    from etm import lib
    assert lib.ABI_VERSION == 61
    S = lib.SIGNATURES
    for name in ("etm_rollout_sample_branched", "etm_rollout_policy_branched", "etm_rollout_trxl_branched", "etm_rollout_trxl_group_branched"):
        res, args = S[name + "_masked"]
        assert S[name + "_logps"] == (res, args[:-1] + [lib._P] + args[-1:]), name
    for name, twin, extra in (("etm_heads_loss_kl", "etm_heads_loss_masked", [lib._P, lib._L]),
                              ("etm_heads_loss_branched_kl", "etm_heads_loss_branched_masked", [lib._P, lib._L]),
                              ("etm_ppo_loss_kl", "etm_ppo_loss_masked", [lib._P, lib._L, lib._I])):
        res, args = S[twin]
        assert S[name] == (res, args[:-1] + extra + args[-1:]), name
    assert S["etm_heads_loss_kl_row_floats"] == S["etm_heads_loss_row_floats"]
    assert S["etm_heads_loss_kl_workspace_bytes"] == S["etm_heads_loss_workspace_bytes"]
    header = open(os.path.join(REPO, "include", "etm_hip.h")).read()
    for name in ("etm_rollout_sample_branched_logps", "etm_rollout_policy_branched_logps", "etm_rollout_trxl_branched_logps",
                 "etm_rollout_trxl_group_branched_logps", "etm_heads_loss_kl", "etm_heads_loss_branched_kl", "etm_ppo_loss_kl",
                 "etm_heads_loss_kl_row_floats", "etm_heads_loss_kl_workspace_bytes"):
        assert f" {name}(" in header, name
    if os.path.exists(lib.LIB_PATH):                       # (a built tree: the library exports them and still answers 61)
        handle = lib.load()
        assert handle.etm_abi_version() == 61
        assert handle.etm_heads_loss_kl_row_floats(64, 3) == handle.etm_heads_loss_row_floats(64, 3) + 1
