"""Host-side checks of the training-side block epilogues (csrc/block_train.hip) that need no GPU: the width dispatch of the row kernels
as a truth table (etm_block_row_groups evaluates the launches' own dispatch_nj on the host), the workspace and partial-row queries
against their documented formulas, and the cover of the case list that tests/test_block_kernels_vs_float64.py runs on the GPU."""
import pytest

EINVAL, EUNSUPPORTED = -1, -2
NJS = (1, 2, 4, 6, 8, 12, 16)


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()                     # dlopen works without a GPU; nothing here launches


def test_row_groups_truth_table(lib):
    """D = 1 .. 1024: the smallest NJ of {1, 2, 4, 6, 8, 12, 16} with 64 NJ >= D; beyond, and for D <= 0, a refusal."""
    for D in range(1, 1025):
        nj = lib.etm_block_row_groups(D)
        need = -(-D // 64)
        assert nj in NJS and nj >= need, (D, nj)
        assert nj == min(m for m in NJS if m >= need), (D, nj)
    for D in range(1025, 1101):
        assert lib.etm_block_row_groups(D) == EUNSUPPORTED, D
    for D in (0, -1, -64, -2 ** 31):
        assert lib.etm_block_row_groups(D) == EINVAL, D
    assert {lib.etm_block_row_groups(D) for D in range(1, 1025)} == set(NJS)


def test_workspace_and_partial_row_queries(lib):
    """ceil(N / 8) partial rows of 3 D (LayerNorm) and D (gate) floats, ceil(N / 64) rows of C floats (relu_bwd_colsum); 0 for
    non-positive arguments."""
    for N in (1, 7, 8, 9, 63, 64, 65, 2048):
        p8, p64 = -(-N // 8), -(-N // 64)
        assert lib.etm_ln_train_bwd_partial_rows(N) == p8 == lib.etm_gate_train_bwd_partial_rows(N)
        assert lib.etm_relu_bwd_colsum_partial_rows(N) == p64
        for D in (1, 63, 64, 65, 384, 1000, 1024):
            assert lib.etm_ln_train_bwd_workspace_bytes(N, D) == p8 * 3 * D * 4, (N, D)
            assert lib.etm_gate_train_bwd_workspace_bytes(N, D) == p8 * D * 4, (N, D)
            assert lib.etm_relu_bwd_colsum_workspace_bytes(N, D) == p64 * D * 4, (N, D)
    for bad in (0, -1, -8):
        assert lib.etm_ln_train_bwd_partial_rows(bad) == 0 and lib.etm_gate_train_bwd_partial_rows(bad) == 0
        assert lib.etm_relu_bwd_colsum_partial_rows(bad) == 0
        for fn in (lib.etm_ln_train_bwd_workspace_bytes, lib.etm_gate_train_bwd_workspace_bytes, lib.etm_relu_bwd_colsum_workspace_bytes):
            assert fn(bad, 64) == 0 and fn(8, bad) == 0 and fn(bad, bad) == 0, (fn, bad)


def test_gpu_case_list_reaches_every_instantiation(lib):
    """The case list of the GPU module (a plain constant): every NJ at the top of its bucket, one past the bucket below and at a
    ragged width, the two widths whose last column group is masked off entirely, each with the plain LayerNorm, the LayerNorm with
    bias + ReLU + residual + fork, and gate_bwd1; row counts below the 4 waves, off the 8 rows of a backward workgroup, and 8."""
    import test_block_kernels_vs_float64 as gpu
    nj = lib.etm_block_row_groups

    def widths(**sel):
        return {c["D"] for c in gpu.CASES if all(c.get(k) == v for k, v in sel.items())}
    plain = widths(kernel="ln", **gpu.LN_PLAIN)
    full = widths(kernel="ln", bias=True, relu=True, res=True, fork=True)
    gate = widths(kernel="gate")
    assert gpu.LN_PLAIN == dict(bias=False, relu=False, res=False, fork=False)
    need = set()
    below = 0
    for m in NJS:
        need |= {64 * m, 64 * below + 1}
        assert nj(64 * m) == m and nj(64 * below + 1) == m
        ragged = {D for D in plain & full & gate if nj(D) == m and D % 64 != 0}
        assert ragged, f"no ragged width for NJ = {m}"
        below = m
    need |= {320, 704}
    assert nj(320) == 6 and -(-320 // 64) == 5 and nj(704) == 12 and -(-704 // 64) == 11
    for name, have in (("plain LayerNorm", plain), ("LayerNorm with bias + ReLU + residual + fork", full), ("gate_bwd1", gate)):
        assert need <= have, f"{name}: widths {sorted(need - have)} are not run"
    for D in need:
        for sel in (dict(kernel="ln", **gpu.LN_PLAIN), dict(kernel="ln", bias=True, relu=True, res=True, fork=True), dict(kernel="gate")):
            ns = {c["N"] for c in gpu.CASES if c["D"] == D and all(c.get(k) == v for k, v in sel.items())}
            assert any(n < 4 for n in ns) and any(n % 8 for n in ns) and 8 in ns, (D, sel, sorted(ns))
    assert all(1 <= c["D"] <= 1024 and c["N"] >= 1 for c in gpu.CASES)
    assert set(gpu.WIDTHS) == plain == gate and set(gpu.ROWS) == {c["N"] for c in gpu.CASES}
