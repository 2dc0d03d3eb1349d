"""CPU-side checks of the exact Gaussian KL (``kl_estimator: analytic``): ``utils.gaussian_kl`` in float64 against the formula in exact
/ 50-digit arithmetic at hand-picked values, its exact zero at equal policies in float32, its agreement with rsl_rl's expression, the
section parser, every refusal of ``trainer.check_kl_estimator_config``, the config file and the ABI mirror."""
import os
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CFG_DIR = os.path.join(HERE, "..", "episodic-transformer-memory-ppo_amd", "configs")
EPS64 = float(np.finfo(np.float64).eps)


def _expm1_exact(x: Fraction, terms: int = 60) -> Fraction:
    """expm1 of a rational by its series: 60 terms leave a remainder below 1e-40 relative for |x| <= 8 (8^61 / 61! < 1e-28, and the
    callers reduce the argument by halving: expm1(2y) = expm1(y) (expm1(y) + 2))."""
    halvings = 0
    while abs(x) > Fraction(1, 4):
        x, halvings = x / 2, halvings + 1
    term, total = Fraction(1), Fraction(0)
    for k in range(1, terms + 1):
        term = term * x / k
        total += term
    for _ in range(halvings):
        total = total * (total + 2)
    return total


def _reference(old_mean, old_log_std, mean, log_std):
    """-> (mean_n KL_n, the sum of the magnitudes of every intermediate term per sample averaged over n) as floats, from 50-digit
    arithmetic (mpmath where it is installed, else the rational series above with exp(log_std) through the same series)."""
    try:
        import mpmath as mp
        mp.mp.dps = 50
        f = lambda v: mp.mpf(Fraction(float(v)).numerator) / mp.mpf(Fraction(float(v)).denominator)
        expm1, exp = mp.expm1, mp.exp
    except ImportError:
        f = lambda v: Fraction(float(v))
        expm1, exp = _expm1_exact, lambda v: _expm1_exact(v) + 1
    total = mag = 0
    for n in range(len(old_mean)):
        for a in range(len(log_std)):
            d = f(old_log_std[a]) - f(log_std[a])
            q = (f(old_mean[n][a]) - f(mean[n][a])) / exp(f(log_std[a]))
            e = expm1(2 * d) / 2
            total += (e - d) + q * q / 2
            mag += abs(e) + abs(d) + q * q / 2
    return float(total / len(old_mean)), float(mag / len(old_mean))


D_VALUES = [0.0, 1e-8, -1e-8, 3.0, -3.0, 0.25, -0.5]


@pytest.mark.parametrize("d", D_VALUES)
def test_gaussian_kl_float64_against_exact_arithmetic(d):
    """Hand-picked values: d = 0, |d| = 1e-8 (where expm1(2d) / 2 - d is d^2 to first order and log1p / exp forms lose every digit),
    d = +-3, with mean differences of 0, a rounding-sized one and whole sigmas.  Tolerance: every operation of the formula is correctly
    rounded or within an ulp or two (expm1, exp), so the error is a few eps times the MAGNITUDES of the terms it adds -- 8 eps of their
    sum is asserted.  (Near d = 1e-8 that is an absolute 1e-23 on a value of 1e-16: the subtraction of d is exact there, the error is
    expm1's own.)"""
    from utils import gaussian_kl
    log_std = np.array([0.0, -1.5, 0.75])
    old_log_std = log_std + np.array([d, 0.0, -d])
    sigma = np.exp(log_std)
    mean = np.array([[0.5, -2.0, 1.0], [0.0, 0.25, -3.0], [1e3, -1e-3, 0.0]])
    old_mean = mean + np.array([[0.0, 0.0, 0.0], [1.0, -2.0, 0.5], [1e-13, 3.0, -1e-7]]) * sigma
    got = gaussian_kl(old_mean, old_log_std, mean, log_std, np.float64)
    assert got.dtype == np.float64
    ref, mag = _reference(old_mean, old_log_std, mean, log_std)
    print(f"d = {d!r}: gaussian_kl {float(got)!r}, exact {ref!r}, error {abs(float(got) - ref):.3e}, allowed {8 * EPS64 * mag:.3e}")
    assert abs(float(got) - ref) <= 8 * EPS64 * mag
    assert ref >= 0.0
    # the log-std part alone (equal means): at |d| = 1e-8 a value of 2e-16 that the quadratic part above would hide
    got0 = gaussian_kl(mean, old_log_std, mean, log_std, np.float64)
    ref0, mag0 = _reference(mean, old_log_std, mean, log_std)
    print(f"d = {d!r}, equal means: gaussian_kl {float(got0)!r}, exact {ref0!r}, error {abs(float(got0) - ref0):.3e}, allowed {8 * EPS64 * mag0:.3e}")
    assert abs(float(got0) - ref0) <= 8 * EPS64 * mag0
    assert (float(got0) == 0.0) == (d == 0.0) and ref0 >= 0.0


def test_series_fallback_agrees_with_the_library_expm1():
    """The rational series used where mpmath is absent, against numpy's expm1 at the test's arguments."""
    for x in (0.0, 2e-8, -2e-8, 6.0, -6.0, 0.5, -1.0):
        exact = float(_expm1_exact(Fraction(x)))
        assert abs(exact - float(np.expm1(x))) <= 4 * EPS64 * abs(exact)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_equal_policies_give_exactly_zero(dtype):
    from utils import gaussian_kl
    rng = np.random.default_rng(0)
    mean = (rng.normal(size=(37, 8)) * 3).astype(dtype)
    log_std = rng.uniform(-5, 2, size=8).astype(dtype)
    kl = gaussian_kl(mean, log_std, mean.copy(), log_std.copy(), dtype)
    assert kl.dtype == dtype and kl == 0 and not np.signbit(kl)


def test_equal_log_std_is_half_the_scaled_squared_distance():
    from utils import gaussian_kl
    rng = np.random.default_rng(1)
    mean, old = rng.normal(size=(9, 3)).astype(np.float32), rng.normal(size=(9, 3)).astype(np.float32)
    log_std = np.array([-1.0, 0.0, 0.5], dtype=np.float32)
    q = (old - mean) / np.exp(log_std)
    want = np.float32((np.float32(0.5) * q * q).sum(axis=1, dtype=np.float32).sum(dtype=np.float32) / np.float32(9))
    got = gaussian_kl(old, log_std, mean, log_std, np.float32)
    assert got.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32)


def test_equals_rsl_rl_expression_in_float64():
    """rsl_rl: sum_a [log(sigma / sigma_old) + (sigma_old^2 + (mu_old - mu)^2) / (2 sigma^2) - 1/2], mean over the samples (its 1e-5 in
    the logarithm left out)."""
    from utils import gaussian_kl
    rng = np.random.default_rng(2)
    for N, A in ((1, 1), (37, 3), (2059, 8)):
        mean, old = rng.normal(size=(N, A)), rng.normal(size=(N, A))
        log_std, old_log_std = rng.uniform(-2, 1, size=A), rng.uniform(-2, 1, size=A)
        s, so = np.exp(log_std), np.exp(old_log_std)
        rsl = (np.log(s / so) + (so ** 2 + (old - mean) ** 2) / (2.0 * s ** 2) - 0.5).sum(axis=1).mean()
        got = float(gaussian_kl(old, old_log_std, mean, log_std, np.float64))
        assert abs(got - rsl) <= 1e-12 * max(1.0, abs(rsl)), (N, A, got, rsl)


def test_gaussian_kl_refuses_other_shapes():
    from utils import gaussian_kl
    with pytest.raises(ValueError, match=r"means \[N, A\] and log-stds \[A\]"):
        gaussian_kl(np.zeros((4, 3)), np.zeros(2), np.zeros((4, 3)), np.zeros(3))
    with pytest.raises(ValueError, match=r"means \[N, A\] and log-stds \[A\]"):
        gaussian_kl(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3))


# ------------------------------------------------------------------ the section and the refusals
def test_section_parser():
    from utils import kl_estimator_section
    assert kl_estimator_section({}) == "k3"
    assert kl_estimator_section({"kl_estimator": "k3"}) == "k3"
    assert kl_estimator_section({"kl_estimator": "analytic"}) == "analytic"
    for bad in ("exact", "K3", "", None, True, 3, ["analytic"]):
        with pytest.raises(ValueError, match=r"kl_estimator must be one of \['k3', 'analytic'\].*write `k3` \(or remove the key\)"):
            kl_estimator_section({"kl_estimator": bad})


def test_check_kl_estimator_config_and_every_refusal():
    from trainer import check_kl_estimator_config
    # key absent / k3: as ever, whatever the policy and the world
    for cfg in ({}, {"kl_estimator": "k3"}):
        for box in (False, True):
            for world in (1, 4):
                assert check_kl_estimator_config(cfg, box, world) == "k3"
    assert check_kl_estimator_config({"kl_estimator": "analytic"}, True, 1) == "analytic"
    with pytest.raises(ValueError, match=r"kl_estimator must be one of .*write `k3` \(or remove the key\)"):
        check_kl_estimator_config({"kl_estimator": "exact"}, True, 1)
    with pytest.raises(ValueError, match=r"analytic without a Box .*categorical policies keep k3: remove the key"):
        check_kl_estimator_config({"kl_estimator": "analytic"}, False, 1)
    with pytest.raises(ValueError, match=r"analytic in a data-parallel run.*remove the key, or train on one device"):
        check_kl_estimator_config({"kl_estimator": "analytic"}, True, 2)
    # (no Box AND data parallel: the kind of policy is named first)
    with pytest.raises(ValueError, match=r"analytic without a Box"):
        check_kl_estimator_config({"kl_estimator": "analytic"}, False, 2)


def test_config_file_is_the_adaptive_one_plus_the_key():
    from trainer import check_adaptive_lr_config, check_box_policy, check_kl_estimator_config
    from yaml_parser import YamlParser
    base = YamlParser(os.path.join(CFG_DIR, "synthetic_continuous_adaptive_lr.yaml")).get_config()
    cfg = YamlParser(os.path.join(CFG_DIR, "synthetic_continuous_adaptive_lr_analytic.yaml")).get_config()
    assert "kl_estimator" not in base and cfg["kl_estimator"] == "analytic"
    assert {k: v for k, v in cfg.items() if k != "kl_estimator"} == base
    assert check_kl_estimator_config(cfg, check_box_policy(cfg) is not None, 1) == "analytic"
    assert check_adaptive_lr_config(cfg)["desired_kl"] == 0.01


def test_evaluation_context_drops_the_key():
    from evaluation import evaluation_config
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(CFG_DIR, "synthetic_continuous_adaptive_lr_analytic.yaml")).get_config()
    assert "kl_estimator" not in evaluation_config(cfg, 4, 8) and cfg["kl_estimator"] == "analytic"


# ------------------------------------------------------------------ the ABI mirror
def test_abi_61_and_the_new_entries():
    from etm import lib
    assert lib.ABI_VERSION == 61
    handle = lib.load()
    assert handle.etm_abi_version() == 61
    for twin in ("etm_rollout_sample_gaussian", "etm_rollout_policy_gaussian", "etm_rollout_trxl_gaussian", "etm_rollout_trxl_group_gaussian"):
        res, args = lib.SIGNATURES[twin]
        res_m, args_m = lib.SIGNATURES[twin + "_means"]
        assert res_m is res and args_m == args[:-1] + [lib._P] + args[-1:], twin        # st_means in front of the stream
        assert hasattr(handle, twin + "_means")
    res, args = lib.SIGNATURES["etm_heads_loss_gaussian"]
    res_k, args_k = lib.SIGNATURES["etm_heads_loss_gaussian_kl"]
    assert res_k is res and args_k == args[:-1] + [lib._P, lib._L, lib._P] + args[-1:]  # old_mean, its row stride, old_log_std
    # host-only entries: the row gains one float behind d log_std, every other offset keeps its value
    for hid, A in ((64, 1), (384, 3), (512, 8)):
        assert handle.etm_heads_loss_gaussian_kl_row_floats(hid, A) == handle.etm_heads_loss_gaussian_row_floats(hid, A) + 1
        assert handle.etm_heads_loss_gaussian_row_floats(hid, A) == (3 + A) * hid + A + 1 + 5 + A
        for N in (1, 8, 9, 2059):
            rows = (N + 7) // 8
            assert handle.etm_heads_loss_gaussian_kl_workspace_bytes(N, hid, A) == rows * 4 * handle.etm_heads_loss_gaussian_kl_row_floats(hid, A)
    assert handle.etm_heads_loss_gaussian_kl_workspace_bytes(8, 100, 3) == 0 and handle.etm_heads_loss_gaussian_kl_workspace_bytes(8, 64, 9) == 0
