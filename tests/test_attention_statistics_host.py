"""No GPU: the host side of ``attention_statistics`` -- the key's reader and its refusals, the evaluator's config, the summary of the
table, the ABI mirror, and the float64 reference the GPU tests compare against (tests/attention_statistics_reference.py) checked
against a loop written per row."""
import math
import os
import re

import numpy as np
import pytest

import attention_statistics_reference as ar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the key
def test_reader_accepts_bools_and_refuses_everything_else():
    from utils import attention_statistics_section
    assert attention_statistics_section({}) is False
    assert attention_statistics_section({"attention_statistics": False}) is False
    assert attention_statistics_section({"attention_statistics": True}) is True
    assert attention_statistics_section({"attention_statistics": np.bool_(True)}) is True
    for bad in (1, 0, "true", "yes", None, 1.0, {"every": 2}, [True]):
        with pytest.raises(ValueError, match=r"attention_statistics must be true or false.*`attention_statistics: true`"):
            attention_statistics_section({"attention_statistics": bad})


def test_data_parallel_run_is_refused():
    from trainer import check_attention_statistics_config
    assert check_attention_statistics_config({}) is False and check_attention_statistics_config({}, world=4) is False
    assert check_attention_statistics_config({"attention_statistics": False}, world=2) is False
    assert check_attention_statistics_config({"attention_statistics": True}) is True
    with pytest.raises(ValueError, match=r"attention_statistics: true in a data-parallel run.*remove the key, or train on one device"):
        check_attention_statistics_config({"attention_statistics": True}, world=2)
    with pytest.raises(ValueError, match="must be true or false"):
        check_attention_statistics_config({"attention_statistics": "on"}, world=2)


def test_evaluation_drops_the_key():
    from evaluation import evaluation_config
    cfg = {"attention_statistics": True, "n_workers": 8, "worker_steps": 16, "n_mini_batch": 4,
           "environment": {"type": "Synthetic"}, "evaluation": {"interval": 1}}
    out = evaluation_config(cfg, 4, 32)
    assert "attention_statistics" not in out and cfg["attention_statistics"] is True


# ------------------------------------------------------------------ the summary
def _empty_table(B=1, H=1):
    return np.zeros((B, H, ar.WORDS), dtype=np.float64)


def test_summary_of_one_row_at_age_three():
    from utils import attention_statistics_summary
    L = 8
    t = _empty_table()
    t[0, 0, 0] = t[0, 0, 1] = 1.0
    t[0, 0, 6] = 1.0
    t[0, 0, ar.AGE0 + 2] = 1.0               # age 3
    t[0, 0, ar.INDEX0 + 4] = 1.0             # v = 7: entry 7 - 3
    s = attention_statistics_summary(t, L)
    assert s["mean_age"][0, 0] == 3.0 and s["rows"][0, 0] == 1 and s["empty"][0, 0] == 0 and s["irregular"][0, 0] == 0
    assert np.array_equal(s["age_hist"][0, 0], np.eye(L)[2]) and np.array_equal(s["index_hist"][0, 0], np.eye(L)[4])
    assert s["entropy"][0, 0] == 0.0 and s["normalised_entropy"][0, 0] == 0.0 and s["max_prob"][0, 0] == 1.0
    assert s["age_hist"].shape == (1, 1, L) and s["mean_age"].shape == (1, 1)


def test_summary_means_are_per_row_and_per_their_own_count():
    from utils import attention_statistics_summary
    t = _empty_table(2, 3)
    t[1, 2, 0], t[1, 2, 1], t[1, 2, 2], t[1, 2, 3] = 4.0, 2.0, 5.0, 1.0
    t[1, 2, 4], t[1, 2, 5], t[1, 2, 6] = 2.0, 1.5, 3.0
    t[1, 2, ar.AGE0: ar.AGE0 + 2] = (3.0, 1.0)
    t[1, 2, ar.INDEX0: ar.INDEX0 + 2] = (1.0, 3.0)
    s = attention_statistics_summary(t, 2)
    assert s["entropy"][1, 2] == 0.5 and s["normalised_entropy"][1, 2] == 0.75 and s["max_prob"][1, 2] == 0.75
    assert s["mean_age"][1, 2] == 1.25 and s["empty"][1, 2] == 5 and s["irregular"][1, 2] == 1
    assert np.array_equal(s["age_hist"][1, 2], [0.75, 0.25]) and np.array_equal(s["index_hist"][1, 2], [0.25, 0.75])
    assert np.isnan(s["entropy"][0, 0]) and s["rows"][0, 0] == 0


def test_summary_of_zero_rows_is_nan_without_an_exception():
    from utils import attention_statistics_summary
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = attention_statistics_summary(_empty_table(2, 2), 16)
    for key in ("entropy", "normalised_entropy", "max_prob", "mean_age", "age_hist", "index_hist"):
        assert np.isnan(s[key]).all(), key
    for key in ("rows", "empty", "irregular"):
        assert (s[key] == 0).all(), key
    t = _empty_table()
    t[0, 0, 0], t[0, 0, 6], t[0, 0, ar.AGE0], t[0, 0, ar.INDEX0] = 2.0, 2.0, 2.0, 2.0      # two rows with v = 1: none with v >= 2
    s = attention_statistics_summary(t, 4)
    assert np.isnan(s["normalised_entropy"][0, 0]) and s["entropy"][0, 0] == 0.0 and s["mean_age"][0, 0] == 1.0


def test_summary_ignores_the_padding_words():
    from utils import attention_statistics_summary
    L = 5
    t = _empty_table()
    t[0, 0, 0] = 1.0
    t[0, 0, ar.AGE0: ar.AGE0 + L] = (0.5, 0.25, 0.25, 0.0, 0.0)
    t[0, 0, ar.INDEX0: ar.INDEX0 + L] = (0.0, 0.0, 0.25, 0.25, 0.5)
    clean = attention_statistics_summary(t, L)
    t[0, 0, ar.AGE0 + L: ar.AGE0 + 128] = 7.0
    t[0, 0, ar.INDEX0 + L: ar.INDEX0 + 128] = 9.0
    t[0, 0, 7] = 11.0
    dirty = attention_statistics_summary(t, L)
    for key in clean:
        assert np.array_equal(clean[key], dirty[key], equal_nan=True), key
    assert clean["mean_age"][0, 0] == 1.75 and clean["age_hist"].shape == (1, 1, L)
    for bad in (np.zeros((1, 264)), np.zeros((1, 1, 263))):
        with pytest.raises(ValueError):
            attention_statistics_summary(bad, L)
    with pytest.raises(ValueError):
        attention_statistics_summary(_empty_table(), 129)


# ------------------------------------------------------------------ the ABI mirror
def test_abi_mirror_declares_both_entries_at_version_61():
    from etm import lib
    assert lib.ABI_VERSION == 61 and lib.ATTN_STATS_WORDS == ar.WORDS == 264
    header = open(os.path.join(REPO, "include", "etm_hip.h")).read()
    assert re.search(r"#define\s+ETM_ATTN_STATS_WORDS\s+264\b", header)
    for name in ("etm_attn_stats_workspace_bytes", "etm_attn_stats"):
        m = re.search(r"^(int64_t|int)\s+" + name + r"\s*\(([^;]*)\);", header, re.M | re.S)
        assert m, name
        res, args = lib.SIGNATURES[name]
        assert res is (lib._L if m.group(1) == "int64_t" else lib._I), name
        assert len(args) == len(m.group(2).split(",")), name
    handle = lib.load()                       # dlopen works without a GPU; no kernel is launched here
    wb = handle.etm_attn_stats_workspace_bytes
    assert wb(1, 1, 1) == 264 * 8 and wb(256, 4, 128) == 4 * 4 * 264 * 8 and wb(257, 4, 31) == 5 * 4 * 264 * 8      # (chunks of 64 samples)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 33, 1), (1, 1, 0), (1, 1, 129), (-3, 2, 8)):
        assert wb(*bad) == 0, bad
    assert handle.etm_attn_stats(None, None, None, None, 0, 1, 1, 1, None) == -1


# ------------------------------------------------------------------ the reference
def _brute_force(att, mask):
    N, H, L = att.shape
    table = np.zeros((H, ar.WORDS), dtype=np.float64)
    for n in range(N):
        bits = [int(b != 0) for b in mask[n]]
        v = sum(bits)
        prefix = bits == [1] * v + [0] * (L - v)
        for h in range(H):
            if not prefix:
                table[h, 3] += 1
                continue
            if v == 0:
                table[h, 2] += 1
                continue
            table[h, 0] += 1
            ent, top = 0.0, 0.0
            for l in range(v):
                p = float(att[n, h, l])
                if p > 0:
                    ent -= p * math.log(p)
                top = max(top, p)
                table[h, ar.AGE0 + (v - l) - 1] += p
                table[h, ar.INDEX0 + l] += p
            table[h, 4] += ent
            table[h, 6] += top
            if v >= 2:
                table[h, 1] += 1
                table[h, 5] += ent / math.log(v)
    return table


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 3, 2), (40, 2, 31), (33, 2, 65), (25, 1, 128)], ids=str)
def test_reference_equals_a_loop_per_row(shape):
    att, mask = ar.attention_statistics_inputs(*shape, seed=3)
    ref, brute = ar.attention_statistics_reference(att, mask), _brute_force(att, mask)
    assert np.array_equal(ref[:, :4], brute[:, :4])
    assert np.allclose(ref, brute, rtol=1e-12, atol=0.0)
    assert (ref[:, 7] == 0).all() and (ref[:, ar.AGE0 + shape[2]: ar.INDEX0] == 0).all() and (ref[:, ar.INDEX0 + shape[2]:] == 0).all()


@pytest.mark.parametrize("shape", [(7, 3, 2), (257, 4, 31), (64, 3, 33), (257, 2, 63), (33, 1, 127), (257, 4, 128)], ids=str)
def test_inputs_cover_what_the_kernel_tests_need(shape):
    N, H, L = shape
    att, mask = ar.attention_statistics_inputs(N, H, L, seed=1)
    v, counted, empty, irregular = ar.row_classes(mask)
    assert att.dtype == np.float32 and mask.dtype == np.uint8
    assert empty.any() and (counted & (v == 1)).any() and (counted & (v == L)).any()
    assert irregular.any() or N < 20
    off = (mask == 0)[:, None, :] & ~empty[:, None, None]           # outside the mask of a row that has one: exact zeros
    assert (att[np.broadcast_to(off, att.shape)] == 0).all()
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((att > 0) & (att < tiny)).any() and ((att == 1).sum(axis=2) == 1).any()
    mass = att[counted].astype(np.float64).sum(axis=2)             # (a subnormal replaces an entry that was not the row's largest)
    assert (mass <= 1 + 1e-5).all() and (mass >= 0.5).all() and np.isclose(mass, 1.0, atol=1e-5).mean() > 0.8


def test_wrong_variants_differ_from_the_reference():
    att, mask = ar.attention_statistics_inputs(64, 2, 33, seed=2)
    ref = ar.attention_statistics_reference(att, mask)
    for kw in ({"age_shift": 1}, {"swap_halves": True}):
        assert np.abs(ar.attention_statistics_reference(att, mask, **kw) - ref).max() > 100 * ar.entropy_bound(ref[0, 0], 33), kw
