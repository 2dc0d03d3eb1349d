"""CPU-side checks of the KL-adaptive learning rate (``adaptive_lr``): the config surface and every refusal, the single rounding of the
band's limits, the rule ``utils.adaptive_lr_step`` against exact rational arithmetic rounded once, the config file and the ABI mirror."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CFG_DIR = os.path.join(HERE, "..", "episodic-transformer-memory-ppo_amd", "configs")
SCHED = {"learning_rate_schedule": {"initial": 3e-4, "final": 3e-4, "power": 1.0, "max_decay_steps": 10}}
F32 = lambda x: float(np.float32(x))
DEFAULT_RULE = {"desired_kl": 0.01, "low": 0.5, "high": 2.0, "factor": 1.5, "min": F32(1e-5), "max": F32(1e-2),
                "kl_low": F32(0.01 * 0.5), "kl_high": F32(0.01 * 2.0)}


def _round32(q: Fraction) -> np.float32:
    """The float32 nearest to the exact rational ``q`` > 0 (ties to even), found without any floating-point arithmetic on q: the double
    nearest to q is taken first only to find the neighbourhood, the choice among its float32 neighbours is made in exact arithmetic."""
    near = np.float32(float(q))
    cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
    errs = [abs(Fraction(float(c)) - q) for c in cands]
    best = min(errs)
    winners = [c for c, e in zip(cands, errs) if e == best]
    if len(winners) > 1:                                       # a tie: the even mantissa
        winners = [c for c in winners if int(np.float32(c).view(np.uint32)) % 2 == 0]
    return np.float32(winners[0])


def _exact_step(lr, kl, rule):
    """The rule restated in exact rationals: every product / quotient is formed exactly and rounded once to float32."""
    lr, kl = np.float32(lr), np.float32(kl)
    q, factor = Fraction(float(lr)), Fraction(float(np.float32(rule["factor"])))
    lo, hi = np.float32(rule["min"]), np.float32(rule["max"])
    if np.isnan(kl):
        return lr, 0
    if np.isposinf(kl) or (np.isfinite(kl) and Fraction(float(kl)) > Fraction(float(np.float32(rule["kl_high"])))):
        return max(lo, _round32(q / factor)), -1
    if np.isfinite(kl) and 0 < Fraction(float(kl)) < Fraction(float(np.float32(rule["kl_low"]))):
        return min(hi, _round32(q * factor)), 1
    return lr, 0


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------ the section
def test_key_absent_is_none():
    from trainer import check_adaptive_lr_config
    from utils import adaptive_lr_section
    assert adaptive_lr_section({}) is None and check_adaptive_lr_config({}) is None
    assert check_adaptive_lr_config({}, world=4) is None, "without the key a data-parallel run is as ever"


def test_scalar_form_and_the_defaults():
    from trainer import check_adaptive_lr_config
    from utils import adaptive_lr_section
    assert adaptive_lr_section({"adaptive_lr": 0.01}) == DEFAULT_RULE
    full = {"desired_kl": 0.01, "factor": 1.5, "low": 0.5, "high": 2.0, "min": 1.0e-5, "max": 1.0e-2}
    assert adaptive_lr_section({"adaptive_lr": full}) == DEFAULT_RULE
    assert check_adaptive_lr_config({"adaptive_lr": 0.01, **SCHED}) == DEFAULT_RULE
    out = adaptive_lr_section({"adaptive_lr": {"desired_kl": 0.02, "factor": 2, "low": 0, "high": 1.5, "min": 1e-6, "max": 1}})
    assert out == {"desired_kl": 0.02, "low": 0.0, "high": 1.5, "factor": 2.0, "min": F32(1e-6), "max": 1.0, "kl_low": 0.0,
                   "kl_high": F32(0.02 * 1.5)}
    wide = adaptive_lr_section({"adaptive_lr": {"desired_kl": 1.5e38, "low": 0, "high": 2.0}})
    assert wide["kl_low"] == 0.0 and wide["kl_high"] == F32(3e38), "a band nothing leaves"


@pytest.mark.parametrize("desired,low,high", [(0.01, 0.5, 2.0), (0.1, 0.3, 1.7), (1e-3, 0.9, 1.1), (0.7, 0.1, 1.9), (3.3e-5, 0.45, 2.2),
                                              (1 / 3, 1 / 3, 3.0)])
def test_the_limits_are_rounded_once(desired, low, high):
    from utils import adaptive_lr_section
    rule = adaptive_lr_section({"adaptive_lr": {"desired_kl": desired, "low": low, "high": high}})
    for key, mult in (("kl_low", low), ("kl_high", high)):
        product = float(desired) * float(mult)
        assert rule[key] == float(np.float32(product)) and np.float32(rule[key]) == rule[key]
        assert _bits(rule[key]) == _bits(_round32(Fraction(product)))
    for key in ("factor", "min", "max"):
        assert np.float32(rule[key]) == rule[key], key + " is a float32 held exactly"


def test_double_rounding_would_differ_somewhere():
    from utils import adaptive_lr_section
    rng = np.random.default_rng(0)
    differ = 0
    for desired, high in zip(rng.uniform(1e-3, 0.2, 200), rng.uniform(1.0, 3.0, 200)):
        got = adaptive_lr_section({"adaptive_lr": {"desired_kl": float(desired), "high": float(high)}})["kl_high"]
        differ += got != float(np.float32(np.float32(desired) * np.float32(high)))
    assert differ > 0


@pytest.mark.parametrize("bad", [0, -0.01, float("nan"), float("inf"), True, "0.01", [0.01]])
def test_bad_desired_kl_is_refused(bad):
    from trainer import check_adaptive_lr_config
    for sec in (bad, {"desired_kl": bad}):
        with pytest.raises(ValueError, match=r"adaptive_lr\.desired_kl must be a finite number > 0.*remove the key"):
            check_adaptive_lr_config({"adaptive_lr": sec, **SCHED})


@pytest.mark.parametrize("bad", [1, 1.0, 1.0 + 1e-9, 0.5, 0, -1.5, float("nan"), float("inf"), 1e39, False, "1.5"])
def test_bad_factor_is_refused(bad):
    """(1 + 1e-9 is 1 as a float32: the kernel's rule would never move the rate)"""
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr\.factor must be a finite number > 1.*leave it out for the default 1\.5"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, "factor": bad}, **SCHED})


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), True, "0.5"])
def test_bad_low_is_refused(bad):
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr\.low must be a finite number >= 0.*leave it out for the default 0\.5"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, "low": bad}, **SCHED})


@pytest.mark.parametrize("bad", [0, -2.0, float("nan"), float("inf"), True, "2"])
def test_bad_high_is_refused(bad):
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr\.high must be a finite number > 0.*leave it out for the default 2\.0"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, "high": bad}, **SCHED})


@pytest.mark.parametrize("sec", [{"low": 2.0, "high": 2.0}, {"low": 3.0, "high": 2.0}, {"low": 1.0, "high": 1.0 + 1e-12},
                                 {"desired_kl": 1e38, "high": 10.0}])
def test_a_band_that_is_empty_or_overflows_is_refused(sec):
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr: float32\(desired_kl \* low\).*must lie below.*choose low < high"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, **sec}, **SCHED})


@pytest.mark.parametrize("key", ["min", "max"])
@pytest.mark.parametrize("bad", [0, -1e-5, 1e-60, 1e39, float("nan"), float("inf"), True, "1e-5"])
def test_bad_min_or_max_is_refused(key, bad):
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=rf"adaptive_lr\.{key} must be a finite number > 0.*leave it out for the default"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, key: bad}, **SCHED})


def test_min_above_max_is_refused():
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr\.min = 0\.001 must not exceed adaptive_lr\.max = 0\.0005.*exchange them"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, "min": 1e-3, "max": 5e-4}, **SCHED})


def test_unknown_sub_keys_are_refused():
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr: unknown keys \['kl_low', 'schedule'\].*remove them"):
        check_adaptive_lr_config({"adaptive_lr": {"desired_kl": 0.01, "schedule": "adaptive", "kl_low": 1.0}, **SCHED})
    with pytest.raises(ValueError, match=r"adaptive_lr: the section needs `desired_kl`.*add it"):
        check_adaptive_lr_config({"adaptive_lr": {"factor": 1.5}, **SCHED})


def test_start_value_outside_the_range_is_refused():
    from trainer import check_adaptive_lr_config
    for initial in (1e-6, 0.5):
        sched = {"learning_rate_schedule": {"initial": initial, "final": initial, "power": 1.0, "max_decay_steps": 10}}
        with pytest.raises(ValueError, match=r"adaptive_lr: the start value float32\(learning_rate_schedule\.initial\).*outside \[min, max\].*"
                                             r"move initial into the range, or widen"):
            check_adaptive_lr_config({"adaptive_lr": 0.01, **sched})
    # the limits themselves are inside: float32(initial) is what is compared
    for initial in (1e-5, 1e-2):
        sched = {"learning_rate_schedule": {"initial": initial, "final": initial, "power": 1.0, "max_decay_steps": 10}}
        assert check_adaptive_lr_config({"adaptive_lr": 0.01, **sched}) == DEFAULT_RULE


def test_a_decaying_schedule_is_refused():
    from trainer import check_adaptive_lr_config
    sched = {"learning_rate_schedule": {"initial": 3e-4, "final": 1e-4, "power": 1.0, "max_decay_steps": 10}}
    with pytest.raises(ValueError, match=r"adaptive_lr with a decaying learning_rate_schedule.*set learning_rate_schedule\.final to initial.*"
                                         r"or remove the key adaptive_lr"):
        check_adaptive_lr_config({"adaptive_lr": 0.01, **sched})


def test_data_parallel_run_is_refused():
    from trainer import check_adaptive_lr_config
    with pytest.raises(ValueError, match=r"adaptive_lr in a data-parallel run.*remove the key, or train on one device"):
        check_adaptive_lr_config({"adaptive_lr": 0.01, **SCHED}, world=2)
    assert check_adaptive_lr_config({"adaptive_lr": 0.01, **SCHED}, world=1)["desired_kl"] == 0.01


def test_config_file_sets_the_key_on_synthetic_continuous_normalized():
    from trainer import check_adaptive_lr_config
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(CFG_DIR, "synthetic_continuous_adaptive_lr.yaml")).get_config()
    base = YamlParser(os.path.join(CFG_DIR, "synthetic_continuous_normalized.yaml")).get_config()
    assert "adaptive_lr" not in base
    assert cfg["learning_rate_schedule"] == dict(base["learning_rate_schedule"], final=base["learning_rate_schedule"]["initial"])
    drop = ("adaptive_lr", "learning_rate_schedule")
    assert {k: v for k, v in cfg.items() if k not in drop} == {k: v for k, v in base.items() if k not in drop}
    assert check_adaptive_lr_config(cfg) == DEFAULT_RULE
    with pytest.raises(ValueError, match="decaying learning_rate_schedule"):
        check_adaptive_lr_config(dict(base, adaptive_lr=0.01))


# ------------------------------------------------------------------ the rule
def test_the_rule_on_the_stated_table():
    from utils import adaptive_lr_step
    rule, lr = DEFAULT_RULE, np.float32(3e-4)
    kl_low, kl_high = np.float32(rule["kl_low"]), np.float32(rule["kl_high"])
    for kl in (0.0, -1e-9, float("nan"), kl_low, kl_high, -0.0, float("-inf")):
        got, way = adaptive_lr_step(lr, kl, rule)
        assert (_bits(got), way) == (_bits(lr), 0), kl
    for kl in (1e-12, 0.004, np.nextafter(kl_low, np.float32(0)), np.float32(1e-45)):
        got, way = adaptive_lr_step(lr, kl, rule)
        assert (_bits(got), way) == (_bits(np.float32(4.5000002e-4)), 1), kl
    for kl in (np.nextafter(kl_high, np.float32(1)), 0.5, float("inf")):
        got, way = adaptive_lr_step(lr, kl, rule)
        assert (_bits(got), way) == (_bits(np.float32(2.0000001e-4)), -1), kl


def test_the_rule_against_exact_rationals_rounded_once():
    from utils import adaptive_lr_section, adaptive_lr_step
    rng = np.random.default_rng(5)
    seen = set()
    for trial in range(600):
        factor = float(rng.choice([1.5, 2.0, 1.1, 1.0 + 2.0 ** -20, 3.3333333]))
        rule = adaptive_lr_section({"adaptive_lr": {"desired_kl": float(rng.uniform(1e-3, 0.1)), "factor": factor,
                                                    "low": float(rng.uniform(0, 1)), "high": float(rng.uniform(1, 3)),
                                                    "min": 1e-5, "max": 1e-2}})
        lr = np.float32(np.exp(rng.uniform(np.log(5e-6), np.log(2e-2))))           # also outside [min, max]
        kl = np.float32(rng.choice([0.0, rule["kl_low"], rule["kl_high"], float(rng.uniform(0, 0.3)), float(rng.uniform(0, 0.01)),
                                    float("nan"), float("inf"), -1e-3]))
        got, way = adaptive_lr_step(lr, kl, rule)
        want, want_way = _exact_step(lr, kl, rule)
        assert isinstance(got, np.float32) and (_bits(got), way) == (_bits(want), want_way), (lr, kl, rule)
        seen.add((way, bool(got == np.float32(rule["min"])), bool(got == np.float32(rule["max"]))))
    assert {(0, False, False), (1, False, False), (-1, False, False), (-1, True, False), (1, False, True)} <= seen


def test_both_clamps_and_a_rate_that_arrives_outside_the_range():
    from utils import adaptive_lr_step
    rule = DEFAULT_RULE
    lo, hi = np.float32(rule["min"]), np.float32(rule["max"])
    assert adaptive_lr_step(lo, 0.5, rule) == (lo, -1) and adaptive_lr_step(hi, 0.001, rule) == (hi, 1)
    assert adaptive_lr_step(np.float32(1.2e-5), 0.5, rule) == (lo, -1), "one cut above min lands on min"
    assert adaptive_lr_step(np.float32(8e-3), 0.001, rule) == (hi, 1), "one raise below max lands on max"
    # the clamps act on a change only: a rate from a checkpoint outside [min, max] stays until the rule moves it
    for lr in (np.float32(1e-6), np.float32(0.5)):
        assert adaptive_lr_step(lr, 0.01, rule) == (lr, 0) and adaptive_lr_step(lr, float("nan"), rule) == (lr, 0)
    assert adaptive_lr_step(np.float32(0.5), 0.5, rule) == (np.float32(np.float32(0.5) / np.float32(1.5)), -1)
    assert adaptive_lr_step(np.float32(0.5), 0.001, rule) == (hi, 1) and adaptive_lr_step(np.float32(1e-6), 0.5, rule) == (lo, -1)


def test_nine_cuts_reach_min_and_nine_raises_reach_max():
    from utils import adaptive_lr_step
    rule = DEFAULT_RULE
    for kl, end in ((0.5, rule["min"]), (0.001, rule["max"])):
        lr, trail = np.float32(3e-4), []
        for _ in range(9):
            want, _ = _exact_step(lr, kl, rule)
            lr, way = adaptive_lr_step(lr, kl, rule)
            assert _bits(lr) == _bits(want) and way == (-1 if kl == 0.5 else 1)
            trail.append(float(lr))
        assert trail[-1] == end and trail[-2] != end, trail
        assert adaptive_lr_step(lr, kl, rule)[0] == np.float32(end)


# ------------------------------------------------------------------ the ABI mirror
def test_abi_mirror_lists_the_new_entry():
    from etm import lib
    handle = lib.load()
    assert handle.etm_abi_version() == lib.ABI_VERSION >= 59
    restype, argtypes = lib.SIGNATURES["etm_grad_sqnorm_adaptive"]
    P, L, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert restype is I and argtypes == [P, L, P, I, P, P, P, F, F, F, F, F, P, F, P, P, P]
    fn = handle.etm_grad_sqnorm_adaptive
    assert fn.argtypes == argtypes and fn.restype is restype
    # the entry refuses before it touches the device: NULL everything
    assert fn(0, 4, 0, 1, 0, 0, 0, 0.005, 0.02, 1.5, 1e-5, 1e-2, 0, 0.0, 0, 0, 0) != 0
    header = open(os.path.join(HERE, "..", "include", "etm_hip.h")).read()
    assert "int etm_grad_sqnorm_adaptive(const float *g, int64_t n, float *partial, int n_partial, int64_t *step" in header
