"""-m gpu: the grouped weight-gradient launches (csrc/grouped_dw.hip: etm_grouped_dw, etm_grouped_dw_tail) and their collector
(ops.DeferredDw) against the float64 product of the same fp32 operands, through the C ABI, at every row split, tile count, stride
and limit the kernel's code distinguishes.

Two kinds of operands:
  exact    integers drawn from [-8, 8] stored as fp32.  Every product is an integer of at most 64 and every partial sum stays below
           2560 * 64 < 2^24, so fp32 addition is exact in any order and the result must EQUAL the float64 product: one dropped or
           doubled row, one tile computed from another tile's operands or written to another place fails, with no tolerance.
  rounded  standard-normal operands.  |C - want| <= gamma_N (|A|^T |B|) elementwise, gamma_N = N u / (1 - N u), u = 2^-24: the
           textbook bound of N fused multiply-adds summed in any order (a derived bound, not a measured one).  The same launch run
           twice must give the same bits.

Everything a launch must not read or write is NaN beforehand: the columns of A and B outside the operand windows (two cases say
where other problems' operands stand there instead), the sample rows beyond N, C itself and the rows and columns of C's storage
around the destination -- the outputs with a NaN of a payload of their own, checked bit for bit afterwards.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
NAN = float("nan")
SENT_BITS = 0x7FC5A5A5            # the outputs' sentinel: a NaN whose payload no arithmetic on the operands' (canonical) NaN produces
U = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda", 0)


def _lib():
    from etm import lib
    return lib.load()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _ints(shape, dev, gen):
    return torch.randint(-8, 9, shape, generator=gen, device=dev).float()


def _randn(shape, dev, gen):
    return torch.randn(shape, generator=gen, device=dev)


def _nans(shape, dev):
    """Operand padding: canonical NaN."""
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _wipe(t):
    """Every element of the (contiguous) output storage ``t`` to the sentinel's bits."""
    t.view(torch.int32).fill_(SENT_BITS)
    return t


def _sentinel(shape, dev):
    return _wipe(torch.empty(shape, dtype=torch.float32, device=dev))


def _args(probs):
    """The table arguments of both entry points for ``probs`` = [(A view [N, Ma], B view [N, Nb], C view [Ma, Nb])]: unit column
    strides, the views' own row strides and addresses."""
    k = len(probs)
    assert all(a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1 and c.shape == (a.shape[1], b.shape[1]) for a, b, c in probs)
    ptrs = [(ctypes.c_void_p * k)(*[p[i].data_ptr() for p in probs]) for i in range(3)]
    dims = (ctypes.c_int32 * (5 * k))(*[v for a, b, c in probs for v in (a.shape[1], b.shape[1], a.stride(0), b.stride(0), c.stride(0))])
    return (*ptrs, dims, k)


def _launch(lib, probs, N, dev):
    from etm import lib as etm_lib
    etm_lib.check(lib.etm_grouped_dw(*_args(probs), N, _stream(dev)), "etm_grouped_dw")


def _want(a, b):
    return a.double().t() @ b.double()


def _assert_exact(got, want, what):
    w32 = want.float()
    assert torch.equal(w32.double(), want), "the float64 product is no fp32 number: the operands are not the exact kind"
    if not torch.equal(got, w32):
        bad = (got != w32) | torch.isnan(got)
        where = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ from the float64 product; rows "
                             f"{int(where[:, 0].min())}..{int(where[:, 0].max())}, columns {int(where[:, 1].min())}..{int(where[:, 1].max())}; "
                             f"first {where[0].tolist()}: got {float(got[tuple(where[0])])} want {float(w32[tuple(where[0])])}")


def _assert_untouched(store, dest, what):
    """Every element of ``store`` outside the index ``dest`` still holds the sentinel bits it was filled with (a NaN with a payload
    of its own: a stray store of anything computed, from NaN padding included, has other bits)."""
    bits = store.view(torch.int32).clone()
    bits[dest] = SENT_BITS
    assert bool((bits == SENT_BITS).all()), f"{what}: {int((bits != SENT_BITS).sum())} elements around the destination were written"


def _bound_ratio(got, a, b, want, N):
    """max |got - want| / (gamma_N |a|^T |b|)  (NaN if ``got`` has one)."""
    gamma = N * U / (1.0 - N * U)
    return float(((got.double() - want).abs() / (gamma * (a.double().abs().t() @ b.double().abs()))).max())


class _Prob:
    """One problem with NaN all round it: A = columns [a_off, a_off + Ma) of a NaN-filled [N, lda] tensor, B = columns
    [b_off, b_off + Nb) of a [N, ldb] one, C = rows [c_row, c_row + Ma) x columns [c_col, c_col + Nb) of a [Ma + 2, Nb + 8] one."""

    def __init__(self, N, Ma, Nb, dev, gen, draw=_ints, a_off=3, lda=None, b_off=4, ldb=None, c_row=1, c_col=4):
        lda, ldb = Ma + 8 if lda is None else lda, Nb + 8 if ldb is None else ldb
        self.a_store, self.b_store, self.c_store = _nans((N, lda), dev), _nans((N, ldb), dev), _sentinel((Ma + 2, Nb + 8), dev)
        self.a, self.b = self.a_store[:, a_off:a_off + Ma], self.b_store[:, b_off:b_off + Nb]
        self.a.copy_(draw((N, Ma), dev, gen))
        self.b.copy_(draw((N, Nb), dev, gen))
        self.dest = (slice(c_row, c_row + Ma), slice(c_col, c_col + Nb))
        self.c = self.c_store[self.dest]
        self.want = _want(self.a, self.b)
        self.what = f"[{Ma}, {Nb}] N={N} A+{a_off}/{lda} B+{b_off}/{ldb} C+({c_row},{c_col})"

    @property
    def views(self):
        return (self.a, self.b, self.c)

    def reset(self):
        _wipe(self.c_store)

    def check_exact(self, what=""):
        _assert_exact(self.c, self.want, what + self.what)
        _assert_untouched(self.c_store, self.dest, what + self.what)


# ------------------------------------------------------------------------------------------------------------------------------
# a. the row split over the four waves and the edges of the 6-slot load pipeline
SPLIT_N = list(range(2, 65)) + list(range(95, 106)) + [2047, 2048, 2049, 2560]
ROUNDED_N = (2, 3, 5, 49, 2049)


def test_every_row_split_and_pipeline_edge():
    """rows_w = ((N + 3) / 4 + 1) & ~1 rows per wave: waves without rows (N = 2: three of them), an odd last k-step, k-step counts
    on both sides of the multiples of the pipeline depth 6 (N = 48 -> 49), the training sizes.  Per N one launch of a [96, 128], a
    [192, 256] (tm, tn in {0, 1}) and a head fold (head N % 4: its columns of a [N, 384] matrix, its plane of [4, N, 128], its rows
    of a [384, 128] gradient).  The operands are the first N rows of one set of allocations whose rows from N on hold NaN."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 1)
    NM = max(SPLIT_N)
    shapes = dict(a1=(NM, 96), b1=(NM, 128), a2=(NM, 192), b2=(NM, 256), q=(NM, 384), pl=(4, NM, 128))
    source = {"exact": {k: _ints(s, dev, gen) for k, s in shapes.items()}, "rounded": {k: _randn(s, dev, gen) for k, s in shapes.items()}}
    w = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
    c1, c2, c3 = _sentinel((96, 128), dev), _sentinel((192, 256), dev), _sentinel((384, 128), dev)
    worst = {}
    for N in SPLIT_N:
        for kind in ("exact", "rounded") if N in ROUNDED_N else ("exact",):
            for k in w:
                w[k].copy_(source[kind][k])
                w[k][..., N:, :] = NAN
            h = N % 4
            rows3 = slice(96 * h, 96 * h + 96)
            w["q"][:, :96 * h] = NAN                              # the other heads' columns of q and planes: outside the windows
            w["q"][:, 96 * h + 96:] = NAN
            w["pl"][:h] = NAN
            w["pl"][h + 1:] = NAN
            probs = [(w["a1"][:N], w["b1"][:N], c1), (w["a2"][:N], w["b2"][:N], c2), (w["q"][:N, rows3], w["pl"][h, :N], c3[rows3])]
            for c in (c1, c2, c3):
                _wipe(c)
            _launch(lib, probs, N, dev)
            _assert_untouched(c3, rows3, f"N={N} {kind} head fold")
            if kind == "exact":
                for i, (a, b, c) in enumerate(probs):
                    _assert_exact(c, _want(a, b), f"N={N} problem {i}")
                continue
            first = [c.clone() for _, _, c in probs]
            for c in (c1, c2, c3):
                _wipe(c)
            _launch(lib, probs, N, dev)
            for i, ((a, b, c), c0) in enumerate(zip(probs, first)):
                assert torch.equal(c.view(torch.int32), c0.view(torch.int32)), f"N={N} problem {i}: two runs of one launch differ"
                ratio = _bound_ratio(c, a, b, _want(a, b), N)
                worst[N] = max(worst.get(N, 0.0), ratio)
                assert ratio <= 1.0, f"N={N} problem {i}: |err| / (gamma_N |A|^T |B|) = {ratio}"
    print("[grouped dW rounded] worst |err| / (gamma_N |A|^T |B|) per N: " + ", ".join(f"N={n}: {r:.3f}" for n, r in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------------------------------------
# b. tile counts: the workgroup -> tile renumbering (gd_tile_of_block) at every residue mod 8, on the device
def test_every_tile_count_of_single_tile_problems():
    """T problems of one [96, 128] tile each, T = 1 .. 64 and 84 (the most a launch carries), N = 6: problem k reads its own windows of
    one wide A (pitch 100 floats, first column 1) and one wide B (pitch 132) with NaN between the windows, and writes its own C."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 2)
    N, K = 6, 84
    assert K == lib.etm_grouped_dw_max_problems()
    A, B, Cs = _nans((N, 100 * K), dev), _nans((N, 132 * K), dev), _sentinel((K, 96, 128), dev)
    av = [A[:, 100 * k + 1: 100 * k + 97] for k in range(K)]
    bv = [B[:, 132 * k: 132 * k + 128] for k in range(K)]
    for k in range(K):
        av[k].copy_(_ints((N, 96), dev, gen))
        bv[k].copy_(_ints((N, 128), dev, gen))
    want = torch.stack([_want(av[k], bv[k]) for k in range(K)])
    flat_want = want.view(K * 96, 128)
    for T in list(range(1, 65)) + [K]:
        _wipe(Cs)
        _launch(lib, [(av[k], bv[k], Cs[k]) for k in range(T)], N, dev)
        _assert_exact(Cs[:T].view(T * 96, 128), flat_want[:T * 96], f"T={T} (rows = 96 * problem + row)")
        _assert_untouched(Cs, slice(0, T), f"T={T}")


GRIDS = [(1, 1), (1, 3), (3, 1), (2, 2), (4, 3)]                # tm x tn tiles of 96 x 128: 23 tiles


def test_ragged_tables_at_every_residue_of_the_tile_count():
    """Tables that mix 1 x 1, 1 x 3, 3 x 1, 2 x 2 and 4 x 3 tile grids with e = 0 .. 7 further single tiles between them: 23 + e tiles,
    every residue mod 8 (the tile -> problem search and the tm / tn split under a renumbering that has leftover blocks)."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 3)
    N = 6
    grid = [_Prob(N, 96 * tm, 128 * tn, dev, gen) for tm, tn in GRIDS]
    extra = [_Prob(N, 96, 128, dev, gen, a_off=k % 4) for k in range(7)]
    residues = set()
    for e in range(8):
        table = []
        for i, p in enumerate(grid):                            # the extras go between the grids, round robin
            table += [p] + extra[i:e:5]
        assert len(table) == 5 + e
        tiles = sum((p.a.shape[1] // 96) * (p.b.shape[1] // 128) for p in table)
        assert tiles == 23 + e
        residues.add(tiles % 8)
        for p in grid + extra:
            p.reset()
        _launch(lib, [p.views for p in table], N, dev)
        for p in table:
            p.check_exact(f"{tiles} tiles: ")
        for p in extra:
            if not any(p is t for t in table):
                _assert_untouched(p.c_store, slice(0, 0), f"{tiles} tiles: a problem outside the table")
    assert residues == set(range(8))


def test_full_launch_of_84_square_layers():
    """84 x [384, 384] in one launch: 1008 tiles, the largest table.  Problem k reads the windows [91 k, 91 k + 384) of one wide A and
    [124 k, 124 k + 384) of one wide B (overlapping windows of different data: every tile's operands are its own).  Unlike the other cases there is no NaN
    beside a window here -- the neighbouring columns are other problems' integers, which a shifted window would still get wrong."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 4)
    N, K, D = 6, 84, 384
    A, B = _ints((N, 91 * (K - 1) + D + 3), dev, gen), _ints((N, 124 * (K - 1) + D + 4), dev, gen)      # (row strides: multiples of 4)
    C = _sentinel((K + 1, D, D), dev)
    probs = [(A[:, 91 * k: 91 * k + D], B[:, 124 * k: 124 * k + D], C[k]) for k in range(K)]
    want = torch.einsum("nkm,nkj->kmj", A.unfold(1, D, 91)[:, :K].double(), B.unfold(1, D, 124)[:, :K].double())
    assert want.shape == (K, D, D)
    _launch(lib, probs, N, dev)
    _assert_exact(C[:K].view(K * D, D), want.view(K * D, D), "84 x [384, 384] (rows = 384 * problem + row)")
    _assert_untouched(C, slice(0, K), "84 x [384, 384]")


# ------------------------------------------------------------------------------------------------------------------------------
# c. tile grids beyond the 4 x 3 of a [384, 384] layer
def test_wide_layer_and_its_head_folds():
    """D = 768 at N = 50: one [768, 768] problem (8 x 6 tiles) and the eight head folds of such a layer (hd = 96: the head's columns of
    q [N, 768], its plane of [8, N, 768], its rows of the gradient).  q has the layer's own pitch (lda = D): the columns beside a
    head's window are the other heads' integers, not NaN; the planes and the [768, 768] problem are padded with NaN."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 5)
    N, D, H = 50, 768, 8
    full = _Prob(N, D, D, dev, gen)
    q = _ints((N, D), dev, gen)
    planes = _nans((H, N, D + 8), dev)
    planes[:, :, 4:4 + D] = _ints((H, N, D), dev, gen)
    c_store = _sentinel((D + 2, D + 8), dev)
    folds = [(q[:, 96 * h: 96 * h + 96], planes[h, :, 4:4 + D], c_store[1 + 96 * h: 97 + 96 * h, 4:4 + D]) for h in range(H)]
    _launch(lib, [full.views] + folds, N, dev)
    full.check_exact()
    for h, (a, b, c) in enumerate(folds):
        _assert_exact(c, _want(a, b), f"head {h} of [768, 768]")
    _assert_untouched(c_store, (slice(1, 1 + D), slice(4, 4 + D)), "head folds of [768, 768]")


# ------------------------------------------------------------------------------------------------------------------------------
# d. strides and offsets
def test_strides_and_offsets():
    """N = 7: A at the column offsets 0, 1, 2, 3 (any 4-byte aligned address) and 2 Ma of [N, Ma + 4] / [N, 3 Ma] tensors, B at column
    offset 4 of [N, Nb + 4], C at row 1 / column 4 of [Ma + 2, Nb + 8] -- one launch of all of them, for one tile and for 2 x 2."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 6)
    N = 7
    probs = []
    for Ma, Nb in ((96, 128), (192, 256)):
        for lda, offs in ((Ma + 4, (0, 1, 2, 3)), (3 * Ma, (0, 1, 2, 3, 2 * Ma))):
            probs += [_Prob(N, Ma, Nb, dev, gen, a_off=off, lda=lda, b_off=4, ldb=Nb + 4) for off in offs]
    assert len(probs) == 18
    _launch(lib, [p.views for p in probs], N, dev)
    for p in probs:
        p.check_exact()


# ------------------------------------------------------------------------------------------------------------------------------
# e. the largest stride the predicate admits at the training size
def test_largest_admitted_stride():
    """N = 2048 with A = the columns 4 .. 100 of a [2048, 261000] tensor (2.1 GB, written in the window only): byte offsets just below
    2^31, the edge of etm_grouped_dw_supported.  lda = 262000 is refused by the argument check (nothing is launched)."""
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 7)
    N, lda = 2048, 261000
    assert lib.etm_grouped_dw_supported(N, 96, 128, lda, 128, 128) == 1 and lib.etm_grouped_dw_supported(N, 96, 128, 262000, 128, 128) == 0
    big = torch.empty((N, lda), dtype=torch.float32, device=dev)
    a = big[:, 4:100]
    a.copy_(_ints((N, 96), dev, gen))
    b, c = _ints((N, 128), dev, gen), _sentinel((98, 128), dev)
    _launch(lib, [(a, b, c[1:97])], N, dev)
    _assert_exact(c[1:97], _want(a, b), f"lda = {lda}")
    _assert_untouched(c, slice(1, 97), f"lda = {lda}")
    _wipe(c)
    pa, pb, pc, dims, k = _args([(a, b, c[1:97])])
    dims[2] = 262000
    assert lib.etm_grouped_dw(pa, pb, pc, dims, k, N, _stream(dev)) == EUNSUPPORTED
    torch.cuda.synchronize(dev)
    _assert_untouched(c, slice(0, 0), "refused lda = 262000")


# ------------------------------------------------------------------------------------------------------------------------------
# f. the tail launch: tiles + column-sum jobs on further workgroups
TAIL_TABLES = {1: [(1, 1)], 7: [(1, 3), (2, 2)], 8: [(2, 2), (2, 2)], 9: [(3, 3)], 12: [(4, 3)], 52: [(1, 1)] * 52}
CS_C = (1, 63, 64, 65, 130)
CS_P = (1, 2, 3, 4, 5, 31, 32, 33, 36, 37)


class _Colsum:
    """One column-sum job: the partial rows are the columns [5, 5 + C) of a NaN-filled [P, C + 9] tensor of integers, the destination
    the elements [1, 1 + C) of a NaN-filled vector."""

    def __init__(self, P, C, dev, gen):
        self.P, self.C, self.ld = P, C, C + 9
        self.store = _nans((P, self.ld), dev)
        self.part = self.store[:, 5:5 + C]
        self.part.copy_(_ints((P, C), dev, gen))
        self.out_store = _sentinel((C + 2,), dev)
        self.out = self.out_store[1:1 + C]
        self.want = self.part.double().sum(0)


def _cs_args(jobs):
    n = len(jobs)
    return ((ctypes.c_void_p * n)(*[j.part.data_ptr() for j in jobs]), (ctypes.c_int * n)(*[j.P for j in jobs]),
            (ctypes.c_int * n)(*[j.C for j in jobs]), (ctypes.c_int * n)(*[j.ld for j in jobs]),
            (ctypes.c_void_p * n)(*[j.out.data_ptr() for j in jobs]), n)


def test_tail_launch_tiles_and_column_sums():
    """etm_grouped_dw_tail on tile tables of 1, 7, 8, 9 and 12 tiles and on the full table of 52 problems, each with 1 and with 64
    column-sum jobs (C in {1, 63, 64, 65, 130} x P in {1 .. 5, 31, 32, 33, 36, 37}: every pair among the 64, ld > C, a first-column
    offset): the tiles and the sums are exact against float64, and every byte of every output's storage equals what etm_grouped_dw
    and etm_colsum_reduce_grouped leave on the same tables.  Around every destination, and in the outputs of the jobs a launch does not name, the sentinel stays."""
    from etm import lib as etm_lib
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 8)
    N = 6
    assert lib.etm_grouped_dw_tail_max_problems() == 52
    pairs = [(P, C) for C in CS_C for P in CS_P]
    jobs = [_Colsum(P, C, dev, gen) for P, C in (pairs + pairs)[:64]]
    for ti, (T, grids) in enumerate(TAIL_TABLES.items()):
        probs = [_Prob(N, 96 * tm, 128 * tn, dev, gen, a_off=i % 4) for i, (tm, tn) in enumerate(grids)]
        assert sum(tm * tn for tm, tn in grids) == T
        for cs in (jobs[7 * ti: 7 * ti + 1], jobs):
            outputs = [p.c_store for p in probs] + [j.out_store for j in jobs]

            def reset():
                for t in outputs:
                    _wipe(t)

            reset()
            etm_lib.check(lib.etm_grouped_dw_tail(*_args([p.views for p in probs]), N, *_cs_args(cs), _stream(dev)), "etm_grouped_dw_tail")
            for p in probs:
                p.check_exact(f"tail, {T} tiles, {len(cs)} column sums: ")
            for j in jobs:
                mine = any(j is c for c in cs)
                if mine:
                    assert torch.equal(j.out, j.want.float()), f"tail, {T} tiles: column sum P={j.P} C={j.C}"
                _assert_untouched(j.out_store, slice(1, 1 + j.C) if mine else slice(0, 0), f"tail, {T} tiles: column sum P={j.P} C={j.C}")
            got = [t.view(torch.int32).clone() for t in outputs]
            reset()
            etm_lib.check(lib.etm_colsum_reduce_grouped(*_cs_args(cs), _stream(dev)), "etm_colsum_reduce_grouped")
            _launch(lib, [p.views for p in probs], N, dev)
            for g, t in zip(got, outputs):
                assert torch.equal(g, t.view(torch.int32)), f"tail, {T} tiles, {len(cs)} column sums: not the separate launches' bits"


# ------------------------------------------------------------------------------------------------------------------------------
# g. refusals: argument checks that return before any launch
def test_refusals_leave_the_outputs_alone():
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 9)
    N = 6
    st = _stream(dev)
    probs = [_Prob(N, 96, 128, dev, gen) for _ in range(3)]
    jobs = [_Colsum(3, 65, dev, gen) for _ in range(2)]
    small = _Prob(N, 64, 128, dev, gen)
    plain, tail = lib.etm_grouped_dw, lib.etm_grouped_dw_tail
    table = lambda n: _args([probs[i % 3].views for i in range(n)])
    jobs_n = lambda n: _cs_args([jobs[i % 2] for i in range(n)])

    def cs_with(field, value):
        part, P, C, ld, out, n = _cs_args(jobs)
        {"P": P, "C": C, "ld": ld}[field][1] = value
        if field == "C":
            ld[1] = value                                       # (ld < C would be the other refusal)
        return part, P, C, ld, out, n

    def shifted(which):                                         # B or C of problem 1 four bytes off its 16-byte alignment
        pa, pb, pc, dims, k = table(3)
        (pb if which == "B" else pc)[1] += 4
        return pa, pb, pc, dims, k

    def null_entry(which):
        pa, pb, pc, dims, k = table(3)
        {"A": pa, "B": pb, "C": pc}[which][2] = None
        return pa, pb, pc, dims, k

    pa, pb, pc, dims, k = table(3)
    cases = [("85 problems", EUNSUPPORTED, lambda: plain(*table(85), N, st)),
             ("53 problems in the tail", EUNSUPPORTED, lambda: tail(*table(53), N, *jobs_n(2), st)),
             ("65 column sums", EUNSUPPORTED, lambda: tail(*table(3), N, *jobs_n(65), st)),
             ("P = 65536", EUNSUPPORTED, lambda: tail(*table(3), N, *cs_with("P", 65536), st)),
             ("C = 65536", EUNSUPPORTED, lambda: tail(*table(3), N, *cs_with("C", 65536), st)),
             ("ld = 65536", EUNSUPPORTED, lambda: tail(*table(3), N, *cs_with("ld", 65536), st)),
             ("Ma = 64", EUNSUPPORTED, lambda: plain(*_args([probs[0].views, small.views]), N, st)),
             ("Ma = 64 in the tail", EUNSUPPORTED, lambda: tail(*_args([probs[0].views, small.views]), N, *jobs_n(2), st)),
             ("N = 1", EUNSUPPORTED, lambda: plain(*table(3), 1, st)),
             ("B off 16 bytes", EINVAL, lambda: plain(*shifted("B"), N, st)),
             ("C off 16 bytes", EINVAL, lambda: plain(*shifted("C"), N, st)),
             ("B off 16 bytes in the tail", EINVAL, lambda: tail(*shifted("B"), N, *jobs_n(2), st)),
             ("C off 16 bytes in the tail", EINVAL, lambda: tail(*shifted("C"), N, *jobs_n(2), st)),
             ("a NULL A", EINVAL, lambda: plain(*null_entry("A"), N, st)),
             ("a NULL B", EINVAL, lambda: plain(*null_entry("B"), N, st)),
             ("a NULL C in the tail", EINVAL, lambda: tail(*null_entry("C"), N, *jobs_n(2), st)),
             ("no A table", EINVAL, lambda: plain(None, pb, pc, dims, k, N, st)),
             ("no dims", EINVAL, lambda: tail(pa, pb, pc, None, k, N, *jobs_n(2), st)),
             ("no column-sum table", EINVAL, lambda: tail(pa, pb, pc, dims, k, N, None, *jobs_n(2)[1:], st)),
             ("no problems", EINVAL, lambda: plain(pa, pb, pc, dims, 0, N, st)),
             ("no column sums", EINVAL, lambda: tail(pa, pb, pc, dims, k, N, *jobs_n(2)[:5], 0, st))]
    for name, code, call in cases:
        assert call() == code, name
    torch.cuda.synchronize(dev)
    for p in probs + [small]:
        _assert_untouched(p.c_store, slice(0, 0), "a refused call")
    for j in jobs:
        _assert_untouched(j.out_store, slice(0, 0), "a refused call")
    # (and the same tables are accepted once nothing is wrong with them)
    assert tail(*table(3), N, *jobs_n(2), st) == 0
    torch.cuda.synchronize(dev)
    probs[2].check_exact("after the refusals: ")


# ------------------------------------------------------------------------------------------------------------------------------
# h. the collector's chunking of more problems than one launch carries
@pytest.mark.parametrize("tail", [True, False])
def test_collector_chunks_150_layers(monkeypatch, tail):
    """150 independent [96, 128] layers (ops.linear_nobias) and one ops.linear_relu_train whose bias gradient leaves a column sum
    pending, N = 6, integers: DeferredDw.flush() launches 52 (tail launch) + 84 + 14 problems, or 84 + 66 with the column sums in a
    launch of their own; every arena view holds the float64 g_i^T x_i exactly.  A second collector meets a [64, 128] layer among
    them: refused, its gradient comes from autograd."""
    from etm import ops
    dev, lib = _dev(), _lib()
    gen = _gen(dev, 10)
    N, K = 6, 150
    X, G = _ints((K, N, 128), dev, gen), _ints((K, N, 96), dev, gen)
    W = _ints((K, 96, 128), dev, gen)
    ws = [W[i].detach().requires_grad_(True) for i in range(K)]
    xr, gr = _ints((N, 128), dev, gen), _ints((N, 96), dev, gen)
    wr, br = _ints((96, 128), dev, gen).requires_grad_(True), _ints((96,), dev, gen).requires_grad_(True)
    x64, g64, w64 = _ints((N, 128), dev, gen), _ints((N, 64), dev, gen), _ints((64, 128), dev, gen).requires_grad_(True)
    want = torch.einsum("knm,knj->kmj", G.double(), X.double())
    gm = gr.double() * ((xr.double() @ wr.detach().double().t() + br.detach().double()) > 0)

    def loss(extra=False):
        total = sum((ops.linear_nobias(X[i], ws[i]) * G[i]).sum() for i in range(K))
        total = total + (ops.linear_relu_train(xr, wr, br) * gr).sum()
        return total + (ops.linear_nobias(x64, w64) * g64).sum() if extra else total

    calls = []
    for name in ("etm_grouped_dw", "etm_grouped_dw_tail"):
        def wrapped(*args, _name=name, _fn=getattr(lib, name)):
            calls.append((_name, args[4]))
            return _fn(*args)
        monkeypatch.setattr(lib, name, wrapped)

    def run(extra):
        arena, db = _sentinel((K + 1, 96, 128), dev), _sentinel((98,), dev)
        dest = {w.data_ptr(): arena[i] for i, w in enumerate(ws)}
        dest[br.data_ptr()] = db[1:97]
        if extra:
            dest[w64.data_ptr()] = _sentinel((64, 128), dev)
        del calls[:]
        for t in ws + [wr, br, w64]:
            t.grad = None
        with ops.DeferredDw(dest, tail=tail) as col:
            loss(extra).backward()
        assert col.written == {w.data_ptr() for w in ws} | {br.data_ptr()}
        assert all(w.grad is None for w in ws) and br.grad is None
        if tail:
            assert calls == [("etm_grouped_dw_tail", 52), ("etm_grouped_dw", 84), ("etm_grouped_dw", 14)], calls
        else:
            assert calls == [("etm_grouped_dw", 84), ("etm_grouped_dw", 66)], calls
        _assert_exact(arena[:K].view(K * 96, 128), want.view(K * 96, 128), "arena (rows = 96 * layer + row)")
        _assert_untouched(arena, slice(0, K), "arena")
        assert torch.equal(db[1:97], gm.sum(0).float()), "the pending column sum (bias gradient)"
        _assert_untouched(db, slice(1, 97), "bias gradient")
        _assert_exact(wr.grad, gm.t() @ xr.double(), "the layer outside the collector's table")
        return dest

    run(False)
    dest = run(True)
    _assert_exact(w64.grad, _want(g64, x64), "the refused [64, 128] layer (autograd)")
    _assert_untouched(dest[w64.data_ptr()], slice(0, 0), "the refused layer's arena view")
