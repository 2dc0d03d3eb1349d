"""Host-side checks of the grouped weight-gradient launches (csrc/grouped_dw.hip) that need no GPU: the workgroup -> tile map the
kernels number their tiles with (etm_grouped_dw_tile_map evaluates the kernels' own function on the host), the shape predicate as
a truth table, and the two problem limits."""
import numpy as np
import pytest

T_MAX = 4096


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()                     # dlopen works without a GPU; nothing here launches


@pytest.fixture(scope="module")
def tile_maps(lib):
    """{T: tile of every workgroup of a launch with T tiles}, T = 1 .. 4096, computed once."""
    maps = {}
    for T in range(1, T_MAX + 1):
        out = np.full(T, -1, dtype=np.int32)
        assert lib.etm_grouped_dw_tile_map(T, out.ctypes.data) == 0
        maps[T] = out
    return maps


def test_tile_map_is_a_bijection_for_every_tile_count(tile_maps):
    """Every tile is computed by exactly one workgroup: a wrong map writes one tile twice and leaves another unwritten."""
    for T, m in tile_maps.items():
        assert np.array_equal(np.sort(m), np.arange(T, dtype=np.int32)), T


def test_tile_map_places_each_die_on_its_own_run(tile_maps):
    """The placement the kernel's comment states: workgroup b runs on die x = b % 8, whose run of tiles is [x T / 8, (x + 1) T / 8) and
    which the dispatcher gives wgs = T / 8 + (x < T % 8) workgroups.  Every workgroup whose slot b / 8 is below min(run, wgs) computes
    tile lo + slot; the others (a die with one workgroup more than its run has tiles) are at most two, none when 8 divides T."""
    for T, m in tile_maps.items():
        b = np.arange(T)
        x, slot = b % 8, b // 8
        lo, hi = x * T // 8, (x + 1) * T // 8
        wgs = T // 8 + (x < T % 8)
        assert np.array_equal(np.bincount(x, minlength=8)[x], wgs), T       # (wgs is indeed what round-robin dealing gives die x)
        placed = slot < np.minimum(hi - lo, wgs)
        assert np.array_equal(m[placed], (lo + slot)[placed]), T
        left = int((~placed).sum())
        assert left <= 2, (T, left)
        if T % 8 == 0:
            assert left == 0, T
        # the leftover workgroups take tiles of other dies' runs, inside the launch
        assert ((m[~placed] >= 0) & (m[~placed] < T)).all(), T


def test_tile_map_rejects_bad_arguments(lib):
    out = np.zeros(4, dtype=np.int32)
    assert lib.etm_grouped_dw_tile_map(0, out.ctypes.data) == -1
    assert lib.etm_grouped_dw_tile_map(-3, out.ctypes.data) == -1
    assert lib.etm_grouped_dw_tile_map(4, None) == -1
    assert not out.any()


def test_supported_truth_table(lib):
    ok = lib.etm_grouped_dw_supported
    assert ok(2048, 384, 384, 384, 384, 384) == 1 and ok(2, 96, 128, 96, 128, 128) == 1
    assert ok(7, 96, 128, 100, 132, 136) == 1 and ok(50, 768, 768, 768, 768, 768) == 1
    # N < 2
    for N in (1, 0, -1):
        assert ok(N, 96, 128, 96, 128, 128) == 0, N
    # whole 96 x 128 tiles only
    for Ma in (0, -96, 1, 64, 95, 97, 128, 100):
        assert ok(64, Ma, 128, 384, 128, 128) == 0, Ma
    for Nb in (0, -128, 1, 64, 96, 127, 129, 192):
        assert ok(64, 96, Nb, 96, 256, 256) == 0, Nb
    # strides below the extent
    assert ok(64, 96, 128, 92, 128, 128) == 0 and ok(64, 192, 128, 96, 128, 128) == 0
    assert ok(64, 96, 128, 96, 124, 128) == 0 and ok(64, 96, 256, 96, 128, 256) == 0
    assert ok(64, 96, 128, 96, 128, 124) == 0 and ok(64, 96, 256, 96, 256, 128) == 0
    # strides that are no multiple of 4 floats
    for r in (1, 2, 3):
        assert ok(64, 96, 128, 96 + r, 128, 128) == 0 and ok(64, 96, 128, 96, 128 + r, 128) == 0 and ok(64, 96, 128, 96, 128, 128 + r) == 0
        assert ok(64, 96, 128, 96 + 4 * r, 128 + 4 * r, 128 + 4 * r) == 1
    # 32-bit byte offsets: (N + 2) * ld * 4 >= 2^31 - 1 is refused, for lda and for ldb
    lim = 2 ** 31 - 1
    for N in (2, 3, 7, 30, 31, 49, 2048, 2560):
        over = -(-lim // (4 * (N + 2)))
        over += -over % 4                                       # the smallest stride (a multiple of 4 floats) over that bound
        assert (N + 2) * over * 4 >= lim > (N + 2) * (over - 4) * 4
        assert ok(N, 96, 128, over, 128, 128) == 0 and ok(N, 96, 128, 96, over, 128) == 0, N
    # ... and so is a stride at which an offset of any load that a wave ISSUES leaves 31 bits: the wave with the most rows
    # (rows_w = ((N + 3) / 4 + 1) & ~1, at most N) runs whole rounds of 6 k-steps of 2 rows and refills the 6 slots once more, so its
    # offsets reach 12 * (rounds + 1) rows -- more than N + 2 for N < 22.  (Beyond the wave's rows a load reads zeros; wrapped round
    # 2^32 it would land inside them again: N = 2 at a stride of 2^27 - 4 floats would add the padding columns of row 1 to C.)
    def issued_rows(N):
        ksteps = (min(((N + 3) // 4 + 1) & ~1, N) + 1) // 2
        return 12 * (-(-ksteps // 6) + 1)

    assert [issued_rows(N) for N in (2, 30, 31, 48, 49, 2048)] == [24, 24, 24, 24, 36, 528]
    assert ok(2, 96, 128, 2 ** 27 - 4, 128, 128) == 0
    for N in (2, 3, 7, 30, 31, 49, 2048, 2560):
        top = (lim - 1) // (4 * max(N + 2, issued_rows(N))) // 4 * 4          # the largest admitted stride: a multiple of 4 floats
        assert ok(N, 96, 128, top, 128, 128) == 1 and ok(N, 96, 128, top + 4, 128, 128) == 0, N
        assert ok(N, 96, 128, 96, top, 128) == 1 and ok(N, 96, 128, 96, top + 4, 128) == 0, N
        assert ok(N, 96, 128, 96, 128, top + 4) == 1, N      # (C is addressed with 64-bit pointers: ldc has no such bound)
    assert ok(2048, 96, 128, 261000, 128, 128) == 1 and ok(2048, 96, 128, 262000, 128, 128) == 0
    assert ok(2048, 96, 128, 96, 261000, 128) == 1 and ok(2048, 96, 128, 96, 262000, 128) == 0


def test_problem_limits(lib):
    assert lib.etm_grouped_dw_max_problems() == 84
    assert lib.etm_grouped_dw_tail_max_problems() == 52
