"""-m gpu: the training-side block epilogues (csrc/block_train.hip: ln_train_fwd_kernel<NJ>, ln_train_bwd_kernel<NJ, TWO>, the four
GRU gate kernels, relu_bwd_colsum_kernel, the fixed-order column-sum reduction) and their rollout twins (csrc/rollout_glue.hip:
add_layernorm_kernel, gru_gate_rz_kernel, gru_gate_out_kernel) through the C ABI, against the same formula in float64 on the same
fp32 operands.  The operands are made here: no library GEMM stands between them and a kernel.  CASES walks every NJ
instantiation of the row kernels (etm_block_row_groups) at the top of its bucket, one past the bucket below, at a ragged width and
at the two widths whose last column group is masked off entirely (320, 704); tests/test_block_kernels_host.py checks that cover.

Operands
  grid      multiples of 2^-8 below 8 in magnitude (a, bias, res, dy, dy2, the gate's A, B, C, bg, x, d out).  a + bias and
            relu(a + bias) + res are then exact in fp32: the saved s must EQUAL the float64 value, the ReLU mask is the same in both
            precisions (a share of a + bias is exactly 0: the tie, gradient 0), and d beta -- sums of at most 520 multiples of 2^-8
            below 16, far below 2^24 units -- must equal the float64 column sum with no tolerance.
  integers  in [-8, 8] for etm_relu_bwd_colsum: gm and the bias gradient must equal the float64 result.
  edges     _ln_edge_rows / _ln_edge_gains of test_gpu_parity.py: constant rows, zero rows, +-1e3 offsets, zero and tiny gains.
  The gate's pre-activations hold +-30 and +-100 in a few places: sigmoid is exactly 1 from 20 up and exactly 0 at -90 and below
  (expf overflows), tanh exactly +-1 from |20|; nothing may come out non-finite.

Metrics (one wrong row or column fails)
  row tensors   per row max |got - want| / max |want| over the row (a row that vanishes in float64 is measured against its
                companion's scale, as _edge_check of test_gpu_parity.py does); the worst row counts.
  column sums   per column |got - want| / sum |terms| with the terms in float64; the worst column counts.
Bounds: max(floor, 2 x e32), e32 = the same metric of the same formula evaluated by torch in fp32 on the CPU.  No error of a kernel
under test sets a bound.  FLOORS holds the floors; the module prints the worst error and the worst e32 per quantity at its end
("Training-side block epilogues", carries that table).

Every output and workspace is a block inside a larger flat buffer filled with a NaN of a payload of its own (SENT_BITS): the floats
in front of and behind the block -- for a workspace: beyond *_workspace_bytes -- must still hold those bits afterwards, as must the
column blocks of dA / dB that a launch is documented not to write.  The inputs are followed by canonical NaN: a read past row N
poisons a sum.  Every launch runs twice and must give the same bits.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAN = float("nan")
SENT_BITS = 0x7FC5A5A5            # the outputs' sentinel: a NaN whose payload no arithmetic on the operands' (canonical) NaN produces
PAD = 32                          # floats of sentinel in front of and behind every output block
EPS = float(torch.tensor(1e-5, dtype=torch.float32))       # the fp32 number the kernels receive

# ---- the case list (plain constants: tests/test_block_kernels_host.py imports them without a GPU)
WIDTHS = (1, 63, 64, 65, 128, 129, 200, 256, 257, 320, 384, 385, 512, 513, 704, 768, 769, 1000, 1024)
ROWS = (1, 3, 8, 9, 37)           # one below the 4 waves, the 8 rows of a backward workgroup, one more, a ragged last workgroup
LN_PLAIN = dict(bias=False, relu=False, res=False, fork=False)          # norm1(query) / norm2(h) of the pre-LN layout
LN_FULL = dict(bias=True, relu=True, res=True, fork=True)               # the post-LN block's norm2(relu(fc) + h), output forked
VARIANTS = ((True, False, True), (True, True, True), (False, False, False), (False, False, True), (True, False, False))   # bias, relu, res
CROSS_WIDTHS = (65, 256, 320, 512, 1024)
EDGE_WIDTHS = (65, 256, 320, 512)
CASES = ([dict(kernel="ln", D=D, N=N, **v) for D in WIDTHS for N in ROWS for v in (LN_PLAIN, LN_FULL)]
         + [dict(kernel="gate", D=D, N=N) for D in WIDTHS for N in ROWS])
CASES += [c for c in (dict(kernel="ln", D=D, N=37, bias=b, relu=r, res=s, fork=f) for D in CROSS_WIDTHS for b, r, s in VARIANTS for f in (False, True))
          if c not in CASES]
COLSUM_D, COLSUM_P = 129, (1, 3, 4, 5, 31, 32, 33, 65)      # N = 8 P partial rows: the edges of colsum_reduce's 8 x 4 unrolled loop
RELU_N, RELU_C = (1, 63, 64, 65, 130), (1, 63, 64, 65, 384)
TWIN_ROWS = (1, 3, 37)
WRAPPER_WIDTHS = (63, 128, 200, 320, 512, 704, 1000)        # one per NJ bucket

# ---- floors.  The project's own numbers for these kernels (test_gpu_parity.py): 2e-5 for LayerNorm outputs and gradients
# (test_fused_layernorm_at_value_edges_vs_float64), 2e-6 of sum |terms| for column sums (the norm_kv column check), 2e-6 per row for
# the gate's forward outputs (test_fused_gru_gate_vs_module_ops), 3e-5 for its gradients (test_gru_gate_train_fwd_bwd_vs_torch); the
# rollout twins and the wrappers take their training kernels'.  Where such a number stood more than about 10 x above the larger of
# the worst error measured on the MI355X and 2 x the worst e32, it is LOWERED to 4 x that larger value (marked; the table in
# DESIGN.md has the measurements).  None is raised.
FLOORS = {
    "ln y": 2e-5, "ln mean": 2.6e-6, "ln rstd": 1.4e-6, "ln ds": 2e-5, "ln da": 2e-5,   # mean, rstd: lowered from 2e-5
    "ln dgamma": 2e-6, "ln dbias": 2e-6, "gate dbg": 2e-6,
    "gate r": 7.2e-7, "gate z": 7.3e-7, "gate rx": 2e-6, "gate hh": 3.7e-7, "gate out": 2e-6,      # r, z, hh: lowered from 2e-6
    "gate dA_h": 3e-5, "gate dA_z": 1.6e-6, "gate dx1": 7.3e-7, "gate dA_r": 1.1e-6, "gate dx2": 7.2e-6,   # all but dA_h: lowered from 3e-5
    "add_ln y": 2.0e-6, "gru rx": 2e-6, "gru z": 7.0e-7, "gru out": 2e-6,               # add_ln y: lowered from 2e-5, gru z: from 2e-6
    "wrap ln y": 1.3e-6, "wrap ln grads": 1.6e-6, "wrap ln colsums": 2e-6,               # ops.fused_layernorm(fork=True); y, grads: lowered from 2e-5
    "wrap gate out": 2e-6, "wrap gate grads": 3e-5,                                      # ops.gru_gate_train (library GEMMs inside)
}
WORST = {}


def _judge(q, err, e32, where):
    """Record, then assert err <= max(floor, 2 x e32)."""
    bound = max(FLOORS[q], 2 * e32)
    rec = WORST.setdefault(q, dict(err=0.0, e32=0.0, where=""))
    if not err <= rec["err"]:
        rec["err"], rec["where"] = err, where
    rec["e32"] = max(rec["e32"], e32)
    assert err <= bound, f"{q} at {where}: {err:.3e} from float64 (bound {bound:.3e}: floor {FLOORS[q]:.1e}, torch fp32 CPU {e32:.3e})"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\n[block kernels f64] per quantity: worst error, worst torch-fp32-CPU error (e32), floor; bound = max(floor, 2 x e32)")
    for q in FLOORS:
        if q in WORST:
            r = WORST[q]
            print(f"  {q:<16} {r['err']:.3e}  e32 {r['e32']:.3e}  floor {FLOORS[q]:.1e}  worst at {r['where']}")


# ---- plumbing
def _dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda", 0)


def _lib():
    from etm import lib
    return lib.load()


def _ok(rc, what):
    from etm import lib
    lib.check(rc, what)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(shape, gen):
    return torch.randint(-2047, 2048, shape, generator=gen).float() / 256.0


def _ints(shape, gen):
    return torch.randint(-8, 9, shape, generator=gen).float()


def _inp(t, dev):
    """An operand on the device, followed by two rows (elements, for a vector) of canonical NaN."""
    store = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), NAN, dtype=torch.float32)
    store[:t.shape[0]] = t
    return store.to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Out:
    """A block of ``shape`` inside a flat sentinel-filled buffer, PAD floats in front of and behind it."""

    def __init__(self, dev, *shape):
        self.n = math.prod(shape)
        self.store = torch.empty(self.n + 2 * PAD, dtype=torch.float32, device=dev)
        self.t = self.store[PAD:PAD + self.n].view(shape)
        self.wipe()

    def wipe(self):
        self.store.view(torch.int32).fill_(SENT_BITS)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def bits(self):
        return self.store.view(torch.int32).clone()

    def cpu(self):
        return self.t.cpu()

    def margins_kept(self, what):
        b = self.store.view(torch.int32)
        bad = int((b[:PAD] != SENT_BITS).sum()) + int((b[PAD + self.n:] != SENT_BITS).sum())
        assert bad == 0, f"{what}: {bad} floats outside the block were written"

    def all_kept(self, what):
        bad = int((self.store.view(torch.int32) != SENT_BITS).sum())
        assert bad == 0, f"{what}: {bad} floats were written, none should be"

    def cols_kept(self, lo, hi, what):
        """The columns [lo, hi) of the (2-D) block still hold the sentinel."""
        bad = int((self.t[:, lo:hi].contiguous().view(torch.int32) != SENT_BITS).sum())
        assert bad == 0, f"{what}: {bad} floats of the columns [{lo}, {hi}) were written"


def _twice(dev, outs, call, what):
    """Wipe ``outs``, ``call()``, again; both runs must leave the same bits in the whole storage of every output."""
    first = None
    for _ in range(2):
        for o in outs:
            o.wipe()
        call()
        torch.cuda.synchronize(dev)
        now = [o.bits() for o in outs]
        if first is not None:
            for i, (x, y) in enumerate(zip(first, now)):
                assert torch.equal(x, y), f"{what}: two runs of one launch differ in output {i}"
        first = now
    for o in outs:
        o.margins_kept(what)


def _row_err(got, want, comp=None):
    """Worst row of max |got - want| / max |want| (rows whose float64 value vanishes against ``comp``'s row: over comp's scale)."""
    got, want = got.double().reshape(want.shape[0], -1), want.reshape(want.shape[0], -1)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    scale = want.abs().amax(1)
    if comp is not None:
        c = comp.double().abs().reshape(want.shape[0], -1).amax(1)
        scale = torch.where(scale < 1e-6 * c, c, scale)
    return float(((got - want).abs().amax(1) / scale.clamp(min=1e-300)).max())


def _col_err(got, terms):
    """Worst column of |got - sum terms| / sum |terms| (terms [N, C] in float64)."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - terms.sum(0)).abs() / terms.abs().sum(0).clamp(min=1e-300)).max())


def _exact(got, want64, what):
    w32 = want64.float()
    assert torch.equal(w32.double(), want64), f"{what}: the float64 value is no fp32 number (the operands are not the exact kind)"
    if not torch.equal(got, w32):
        bad = ((got != w32) | torch.isnan(got)).reshape(-1).nonzero()
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ from float64, first at flat index {int(bad[0])}: "
                             f"got {float(got.reshape(-1)[bad[0]])} want {float(w32.reshape(-1)[bad[0]])}")


def _reduce_deferred(lib, dev, ws, P, C, what):
    """The partial rows a producer left in ``ws`` through etm_colsum_reduce_grouped (one launch, one problem) -> an _Out of [C]."""
    out = _Out(dev, C)
    args = ((ctypes.c_void_p * 1)(ws.ptr), (ctypes.c_int * 1)(P), (ctypes.c_int * 1)(C), (ctypes.c_int * 1)(C), (ctypes.c_void_p * 1)(out.ptr), 1)
    _twice(dev, [out], lambda: _ok(lib.etm_colsum_reduce_grouped(*args, _stream(dev)), "etm_colsum_reduce_grouped"), what + " deferred column sums")
    return out


# ---- LayerNorm: the same formula in the precision ``dt``
def _ln_fwd_ref(a, bias, relu, res, gamma, beta, dt):
    s = a.to(dt)
    if bias is not None:
        s = s + bias.to(dt)
    if relu:
        s = torch.relu(s)
    if res is not None:
        s = s + res.to(dt)
    mean = s.mean(1, keepdim=True)
    d = s - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
    return d * rstd * gamma.to(dt) + beta.to(dt), s, mean[:, 0], rstd[:, 0]


def _ln_bwd_ref(dy, dy2, s, mean, rstd, gamma, pre, dt):
    """ds, da (= ds where pre > 0; pre None: no ReLU, da = ds), and the terms of the three column sums.  The terms of d gamma and d beta
    are the products dy xhat and dy themselves (a rounding or two each, as in the norm_kv column check the 2e-6 floor comes from).  An
    element of da is itself the sum rstd (dy g - m1 - xhat m2), whose addends cancel: the third sum's terms are those ADDENDS, three
    per row [3 N, D] -- against sum |da| an element that cancels to nearly nothing would be asked for more digits than fp32 has."""
    d = dy.to(dt) if dy2 is None else dy.to(dt) + dy2.to(dt)
    rs = rstd.to(dt)[:, None]
    xh = (s.to(dt) - mean.to(dt)[:, None]) * rs
    gg = d * gamma.to(dt)
    m1, m2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    ds = rs * (gg - m1 - xh * m2)
    live = torch.ones_like(ds) if pre is None else (pre.to(dt) > 0).to(dt)
    da = ds * live
    return ds, da, d * xh, d, torch.cat((rs * gg * live, -(rs * m1) * live, -(rs * xh * m2) * live))


def _ln_operands(D, N, bias, relu, res, fork, seed, a=None, gamma=None):
    gen = _gen(seed)
    a = _grid((N, D), gen) if a is None else a
    o = dict(a=a, bias=_grid((D,), gen) if bias else None, res=_grid((N, D), gen) if res else None,
             gamma=1 + 0.1 * torch.randn((D,), generator=gen) if gamma is None else gamma, beta=0.1 * torch.randn((D,), generator=gen),
             dy=_grid((N, D), gen), dy2=_grid((N, D), gen) if fork else None, relu=relu)
    if relu or bias:
        tie = torch.rand((N, D), generator=gen) < 0.1           # a + bias == 0 exactly: the tie of the ReLU
        o["a"] = torch.where(tie, -o["bias"].expand(N, D) if bias else torch.zeros(()), a)
    return o


def _run_ln(lib, dev, D, N, bias, relu, res, fork, seed, label, **given):
    """One forward launch and one backward launch (direct, then deferred) of the training LayerNorm; everything compared."""
    what = f"{label} D={D} N={N} bias={int(bias)} relu={int(relu)} res={int(res)} fork={int(fork)}"
    st = _stream(dev)
    o = _ln_operands(D, N, bias, relu, res, fork, seed, **given)
    y64, s64, mean64, rstd64 = _ln_fwd_ref(o["a"], o["bias"], relu, o["res"], o["gamma"], o["beta"], torch.float64)
    y32, _, mean32, rstd32 = _ln_fwd_ref(o["a"], o["bias"], relu, o["res"], o["gamma"], o["beta"], torch.float32)
    d = {k: _inp(v, dev) if isinstance(v, torch.Tensor) else None for k, v in o.items()}
    y, s, stats = _Out(dev, N, D), _Out(dev, N, D), _Out(dev, N, 2)
    _twice(dev, [y, s, stats], lambda: _ok(lib.etm_ln_train_fwd(_ptr(d["a"]), _ptr(d["bias"]), int(relu), _ptr(d["res"]), _ptr(d["gamma"]),
                                                                _ptr(d["beta"]), EPS, y.ptr, s.ptr, stats.ptr, N, D, st), "etm_ln_train_fwd"), what)
    _exact(s.cpu(), s64, what + ": saved s")
    comp_y = (o["gamma"].abs().max() + o["beta"].abs().max()).expand(N, 1)
    _judge("ln y", _row_err(y.cpu(), y64, comp_y), _row_err(y32, y64, comp_y), what)
    smax = s64.abs().amax(1).clamp(min=1e-300)
    got_stats = stats.cpu().double()
    assert bool(torch.isfinite(got_stats).all()), what + ": non-finite statistics"
    _judge("ln mean", float(((got_stats[:, 0] - mean64).abs() / smax).max()), float(((mean32.double() - mean64).abs() / smax).max()), what)
    _judge("ln rstd", float(((got_stats[:, 1] - rstd64).abs() / rstd64).max()), float(((rstd32.double() - rstd64).abs() / rstd64).max()), what)
    y_bits = y.bits()
    _twice(dev, [y], lambda: _ok(lib.etm_ln_train_fwd(_ptr(d["a"]), _ptr(d["bias"]), int(relu), _ptr(d["res"]), _ptr(d["gamma"]),
                                                      _ptr(d["beta"]), EPS, y.ptr, None, None, N, D, st), "etm_ln_train_fwd"), what + " (no s, no stats)")
    assert torch.equal(y.bits(), y_bits), what + ": y differs without s_out / stats"

    # backward on operands of the test's own: s (exact), the float64 statistics rounded to fp32
    mean_r, rstd_r = mean64.float(), rstd64.float()
    pre = (o["a"].double() + o["bias"].double()) if relu else None
    r64 = _ln_bwd_ref(o["dy"], o["dy2"], s64, mean_r, rstd_r, o["gamma"], pre, torch.float64)
    r32 = _ln_bwd_ref(o["dy"], o["dy2"], s64.float(), mean_r, rstd_r, o["gamma"], pre, torch.float32)
    ds_in, st_in = _inp(s64.float(), dev), _inp(torch.stack((mean_r, rstd_r), 1), dev)
    nbytes = lib.etm_ln_train_bwd_workspace_bytes(N, D)
    P = lib.etm_ln_train_bwd_partial_rows(N)
    assert nbytes == P * 3 * D * 4
    ds, da, sums, ws = _Out(dev, N, D), _Out(dev, N, D), _Out(dev, 3, D), _Out(dev, P, 3 * D)

    def bwd(dest):
        _ok(lib.etm_ln_train_bwd(_ptr(d["dy"]), _ptr(d["dy2"]), _ptr(ds_in), _ptr(st_in), _ptr(d["gamma"]), _ptr(d["a"]) if relu else None,
                                 _ptr(d["bias"]) if relu else None, int(relu), ds.ptr, da.ptr, dest, ws.ptr, nbytes, N, D, st), "etm_ln_train_bwd")
    _twice(dev, [ds, da, sums, ws], lambda: bwd(sums.ptr), what + " backward")
    comp = o["dy"] if o["dy2"] is None else o["dy"].double() + o["dy2"].double()
    _judge("ln ds", _row_err(ds.cpu(), r64[0], comp), _row_err(r32[0], r64[0], comp), what)
    if relu:
        _judge("ln da", _row_err(da.cpu(), r64[1], comp), _row_err(r32[1], r64[1], comp), what)
    else:
        da.all_kept(what + ": da without ReLU")
    got = sums.cpu()
    _judge("ln dgamma", _col_err(got[0], r64[2]), _col_err(r32[2].sum(0), r64[2]), what)
    _exact(got[1], r64[3].sum(0), what + ": d beta")
    _judge("ln dbias", _col_err(got[2], r64[4]), _col_err(r32[1].sum(0), r64[4]), what)
    direct = [x.bits() for x in (ds, da, ws)]
    sum_bits = sums.t.view(torch.int32).clone()
    _twice(dev, [ds, da, sums, ws], lambda: bwd(None), what + " backward, deferred")
    sums.all_kept(what + ": the deferred route's absent destination")
    for x, b in zip((ds, da, ws), direct):
        assert torch.equal(x.bits(), b), what + ": the deferred route's first launch differs from the direct route's"
    later = _reduce_deferred(lib, dev, ws, P, 3 * D, what)
    assert torch.equal(later.t.view(torch.int32), sum_bits.reshape(-1)), what + ": deferred column sums are not the direct route's bits"


def _ln_cases(**sel):
    return [c for c in CASES if c["kernel"] == "ln" and all(c[k] == v for k, v in sel.items())]


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_plain_and_forked_full_at_every_width_and_row_count(D):
    """ln_train_fwd_kernel<NJ>, ln_train_bwd_kernel<NJ, false> (plain) and <NJ, true> with bias + ReLU + residual (what every post-LN
    block runs) at every width of WIDTHS x every row count of ROWS.  (D = 1 is the hardest row for d s: it is exactly 0 in float64,
    and the kernel's contracted dy g - m1 leaves the rounding residue of the product, up to 2^-24 |dy g| x rstd = 1 / sqrt(eps) = 316:
    1.5e-5 of |dy| measured, against 2e-5.)"""
    lib, dev = _lib(), _dev()
    assert lib.etm_block_row_groups(D) >= (D + 63) // 64
    for v in (LN_PLAIN, LN_FULL):
        cases = _ln_cases(D=D, **v)
        assert [c["N"] for c in cases] == list(ROWS)
        for c in cases:
            _run_ln(lib, dev, D, c["N"], c["bias"], c["relu"], c["res"], c["fork"], 1000 * D + c["N"], "rows")


@pytest.mark.parametrize("D", CROSS_WIDTHS)
def test_layernorm_every_variant_forked_and_not(D):
    """(bias, relu, res) in VARIANTS x fork in {no, yes} at N = 37."""
    lib, dev = _lib(), _dev()
    for b, r, s in VARIANTS:
        for f in (False, True):
            assert len(_ln_cases(D=D, N=37, bias=b, relu=r, res=s, fork=f)) == 1
            _run_ln(lib, dev, D, 37, b, r, s, f, 77 * D + 8 * b + 4 * r + 2 * s + f, "variants")


@pytest.mark.parametrize("gains", ["mixed", "zero"])
@pytest.mark.parametrize("D", EDGE_WIDTHS)
def test_layernorm_at_value_edges(D, gains):
    """Constant rows, zero rows, +-1e3 offsets; exact zeros, tiny and negative gains, an all-zero gain vector: s = a (exact), plain
    and forked."""
    from test_gpu_parity import _ln_edge_gains, _ln_edge_rows
    lib, dev = _lib(), _dev()
    g = _gen(31 * D + (gains == "zero"))
    a, w = _ln_edge_rows(37, D, g), _ln_edge_gains(D, g, gains)
    for fork in (False, True):
        _run_ln(lib, dev, D, 37, False, False, False, fork, D + fork, f"edges ({gains} gains)", a=a, gamma=w)


# ---- the gate
def _gate_operands(D, N, seed):
    gen = _gen(seed)
    o = dict(A=_grid((N, 3 * D), gen), B=_grid((N, 2 * D), gen) / 4, C=_grid((N, D), gen) / 4, bg=_grid((D,), gen) / 4, x=_grid((N, D), gen),
             dout=_grid((N, D), gen), dout2=_grid((N, D), gen), drx=_grid((N, D), gen))
    o["A"] /= 4                                                                    # pre-activations within +-6, then the saturated ones:
    for blk in range(3):
        for i, v in enumerate((30.0, -30.0, 100.0, -100.0)):
            o["A"][(i + blk) % N, blk * D + (7 * i + blk) % D] = v
    return o


def _normal(t):
    """Subnormal fp32 values to 0: sigmoid(-100) is 4e-44 in float64, the kernel's own z there is exactly 0 (expf overflows), and a
    subnormal operand has too few bits to measure a relative error against."""
    return torch.where(t.abs() < 2.0 ** -126, torch.zeros_like(t), t)


def _gate_fwd_ref(o, dt, z_in=None):
    D = o["x"].shape[1]
    A, B, C, bg, x = (o[k].to(dt) for k in ("A", "B", "C", "bg", "x"))
    r = torch.sigmoid(A[:, :D] + B[:, :D])
    z = torch.sigmoid(A[:, D:2 * D] + B[:, D:] - bg)
    hh = torch.tanh(A[:, 2 * D:] + C)
    zz = z if z_in is None else z_in.to(dt)
    return dict(r=r, z=z, rx=r * x, hh=hh, out=(1.0 - zz) * x + zz * hh)


def _gate_bwd_ref(o, z, hh, r, dx1_in, fork, dt):
    g = o["dout"].to(dt) + o["dout2"].to(dt) if fork else o["dout"].to(dt)
    z, hh, r, x, drx = z.to(dt), hh.to(dt), r.to(dt), o["x"].to(dt), o["drx"].to(dt)
    dph = g * z * (1.0 - hh * hh)
    dpz = g * (hh - x) * z * (1.0 - z)
    dx1 = g * (1.0 - z)
    dpr = drx * x * r * (1.0 - r)
    return dict(dA_h=dph, dA_z=dpz, dx1=dx1, dA_r=dpr, dx2=(dx1 if dx1_in is None else dx1_in.to(dt)) + drx * r, g=g)


def _run_gate(lib, dev, D, N, seed, label, fork=True):
    what = f"{label} D={D} N={N} fork={int(fork)}"
    st = _stream(dev)
    o = _gate_operands(D, N, seed)
    f64 = _gate_fwd_ref(o, torch.float64)
    z_in, hh_in, r_in = (_normal(f64[k].float()) for k in ("z", "hh", "r"))        # the later kernels' operands: made here
    f64 = _gate_fwd_ref(o, torch.float64, z_in)
    f32 = _gate_fwd_ref(o, torch.float32, z_in)
    d = {k: _inp(v, dev) for k, v in o.items()}
    dz, dhh, dr = _inp(z_in, dev), _inp(hh_in, dev), _inp(r_in, dev)
    r, z, rx, hh, out = (_Out(dev, N, D) for _ in range(5))
    _twice(dev, [r, z, rx], lambda: _ok(lib.etm_gate_train_rz(_ptr(d["A"]), _ptr(d["B"]), _ptr(d["bg"]), _ptr(d["x"]), r.ptr, z.ptr, rx.ptr, N, D, st),
                                        "etm_gate_train_rz"), what + " rz")
    _twice(dev, [hh, out], lambda: _ok(lib.etm_gate_train_out(_ptr(d["A"]), _ptr(d["C"]), _ptr(dz), _ptr(d["x"]), hh.ptr, out.ptr, N, D, st),
                                       "etm_gate_train_out"), what + " out")
    got = dict(r=r.cpu(), z=z.cpu(), rx=rx.cpu(), hh=hh.cpu(), out=out.cpu())
    for k in ("r", "z", "rx", "hh", "out"):
        comp = o["x"] if k in ("rx", "out") else torch.ones((N, 1))
        _judge("gate " + k, _row_err(got[k], f64[k], comp), _row_err(f32[k], f64[k], comp), what)
    A, B = o["A"].double(), o["B"].double()
    some = N * D >= 3                                      # (fewer elements: the four planted values overwrite each other)
    for k, pre in (("r", A[:, :D] + B[:, :D]), ("z", A[:, D:2 * D] + B[:, D:] - o["bg"].double())):
        assert not some or (bool((pre >= 20).any()) and bool((pre <= -90).any()))
        assert bool((got[k][pre >= 20] == 1).all()) and bool((got[k][pre <= -90] == 0).all()), f"{what}: {k} is not saturated to exactly 0 / 1"
    pre = A[:, 2 * D:] + o["C"].double()
    assert bool((pre.abs() >= 20).any())
    assert bool((got["hh"][pre.abs() >= 20] == torch.sign(pre[pre.abs() >= 20]).float()).all()), f"{what}: tanh is not saturated to exactly +-1"

    # backward, first kernel: dA[:, D:3D], dB[:, D:2D], dx1, d bg; the columns [0, D) stay alone
    b64 = _gate_bwd_ref(o, z_in, hh_in, r_in, None, fork, torch.float64)
    dx1_in = b64["dx1"].float()
    b64 = _gate_bwd_ref(o, z_in, hh_in, r_in, dx1_in, fork, torch.float64)
    b32 = _gate_bwd_ref(o, z_in, hh_in, r_in, dx1_in, fork, torch.float32)
    nbytes = lib.etm_gate_train_bwd_workspace_bytes(N, D)
    P = lib.etm_gate_train_bwd_partial_rows(N)
    assert nbytes == P * D * 4
    dA, dB, dx1, dbg, ws = _Out(dev, N, 3 * D), _Out(dev, N, 2 * D), _Out(dev, N, D), _Out(dev, D), _Out(dev, P, D)

    def bwd1(dest):
        _ok(lib.etm_gate_train_bwd1(_ptr(d["dout"]), _ptr(d["dout2"]) if fork else None, _ptr(dz), _ptr(dhh), _ptr(d["x"]), dA.ptr, dB.ptr, dx1.ptr,
                                    dest, ws.ptr, nbytes, N, D, st), "etm_gate_train_bwd1")
    _twice(dev, [dA, dB, dx1, dbg, ws], lambda: bwd1(dbg.ptr), what + " bwd1")
    dA.cols_kept(0, D, what + " bwd1: dA")
    dB.cols_kept(0, D, what + " bwd1: dB")
    gA, gB = dA.cpu(), dB.cpu()
    _judge("gate dA_h", _row_err(gA[:, 2 * D:], b64["dA_h"], b64["g"]), _row_err(b32["dA_h"], b64["dA_h"], b64["g"]), what)
    _judge("gate dA_z", _row_err(gA[:, D:2 * D], b64["dA_z"], b64["g"]), _row_err(b32["dA_z"], b64["dA_z"], b64["g"]), what)
    assert torch.equal(gA[:, D:2 * D].contiguous().view(torch.int32), gB[:, D:].contiguous().view(torch.int32)), what + ": dB[:, D:2D] is not dA[:, D:2D]"
    _judge("gate dx1", _row_err(dx1.cpu(), b64["dx1"], b64["g"]), _row_err(b32["dx1"], b64["dx1"], b64["g"]), what)
    _judge("gate dbg", _col_err(dbg.cpu(), -b64["dA_z"]), _col_err(-b32["dA_z"].sum(0), -b64["dA_z"]), what)
    direct = [x.bits() for x in (dA, dB, dx1, ws)]
    dbg_bits = dbg.t.view(torch.int32).clone()
    _twice(dev, [dA, dB, dx1, dbg, ws], lambda: bwd1(None), what + " bwd1, deferred")
    dbg.all_kept(what + ": the deferred route's absent destination")
    for x, b in zip((dA, dB, dx1, ws), direct):
        assert torch.equal(x.bits(), b), what + ": the deferred route's first launch differs from the direct route's"
    later = _reduce_deferred(lib, dev, ws, P, D, what)
    assert torch.equal(later.t.view(torch.int32), dbg_bits), what + ": deferred d bg is not the direct route's bits"

    # second kernel: exactly the columns [0, D) of dA and dB, and dx2
    ddx1 = _inp(dx1_in, dev)
    dx2 = _Out(dev, N, D)
    _twice(dev, [dA, dB, dx2], lambda: _ok(lib.etm_gate_train_bwd2(_ptr(d["drx"]), _ptr(d["x"]), _ptr(dr), _ptr(ddx1), dA.ptr, dB.ptr, dx2.ptr, N, D, st),
                                           "etm_gate_train_bwd2"), what + " bwd2")
    dA.cols_kept(D, 3 * D, what + " bwd2: dA")
    dB.cols_kept(D, 2 * D, what + " bwd2: dB")
    gA, gB = dA.cpu(), dB.cpu()
    comp = o["drx"].double() * o["x"].double()
    _judge("gate dA_r", _row_err(gA[:, :D], b64["dA_r"], comp), _row_err(b32["dA_r"], b64["dA_r"], comp), what)
    assert torch.equal(gA[:, :D].contiguous().view(torch.int32), gB[:, :D].contiguous().view(torch.int32)), what + ": dB[:, 0:D] is not dA[:, 0:D]"
    _judge("gate dx2", _row_err(dx2.cpu(), b64["dx2"], o["drx"]), _row_err(b32["dx2"], b64["dx2"], o["drx"]), what)


@pytest.mark.parametrize("D", WIDTHS)
def test_gate_kernels_at_every_width_and_row_count(D):
    """gate_rz_train, gate_out_train, gate_bwd1_kernel<NJ> (forked: d out + d out2 on load; N = 9 also unforked), gate_bwd2."""
    lib, dev = _lib(), _dev()
    ns = [c["N"] for c in CASES if c["kernel"] == "gate" and c["D"] == D]
    assert ns == list(ROWS)
    for N in ns:
        _run_gate(lib, dev, D, N, 500 * D + N, "gate")
    _run_gate(lib, dev, D, 9, 500 * D, "gate", fork=False)


# ---- the second stage of the column sums
@pytest.mark.parametrize("P", COLSUM_P)
def test_column_sum_second_stage_at_the_edges_of_its_unrolled_loop(P):
    """N = 8 P rows at D = 129: the backward kernels leave P partial rows, colsum_reduce_kernel (direct) and colsum_reduce_block
    (deferred) add them 32 at a time with a tail -- P on both sides of 4, of 32 and of 64."""
    lib, dev = _lib(), _dev()
    assert lib.etm_ln_train_bwd_partial_rows(8 * P) == P == lib.etm_gate_train_bwd_partial_rows(8 * P)
    _run_ln(lib, dev, COLSUM_D, 8 * P, True, True, True, True, 9000 + P, "colsum")
    _run_gate(lib, dev, COLSUM_D, 8 * P, 9500 + P, "colsum")


@pytest.mark.parametrize("C", RELU_C)
def test_relu_bwd_colsum_exact(C):
    """gm = g (y > 0) and its column sums on integers: equal to float64, for N in RELU_N, with y and gm, without y, without both;
    direct and deferred."""
    lib, dev = _lib(), _dev()
    st = _stream(dev)
    for N in RELU_N:
        gen = _gen(100 * C + N)
        g, y = _ints((N, C), gen), _ints((N, C), gen)                      # (y == 0 about once in 17: the tie, gradient 0)
        dg, dy_ = _inp(g, dev), _inp(y, dev)
        nbytes, P = lib.etm_relu_bwd_colsum_workspace_bytes(N, C), lib.etm_relu_bwd_colsum_partial_rows(N)
        assert nbytes == P * C * 4
        for has_y, has_gm in ((True, True), (False, True), (False, False)):
            what = f"relu_bwd_colsum N={N} C={C} y={int(has_y)} gm={int(has_gm)}"
            want = g.double() * (y.double() > 0) if has_y else g.double()
            gm, db, ws = _Out(dev, N, C), _Out(dev, C), _Out(dev, P, C)

            def run(dest):
                _ok(lib.etm_relu_bwd_colsum(_ptr(dg), _ptr(dy_) if has_y else None, gm.ptr if has_gm else None, dest, ws.ptr, nbytes, N, C, st),
                    "etm_relu_bwd_colsum")
            _twice(dev, [gm, db, ws], lambda: run(db.ptr), what)
            if has_gm:
                _exact(gm.cpu(), want, what + ": gm")
            else:
                gm.all_kept(what + ": gm")
            _exact(db.cpu(), want.sum(0), what + ": db")
            direct = [gm.bits(), ws.bits(), db.t.view(torch.int32).clone()]
            _twice(dev, [gm, db, ws], lambda: run(None), what + " deferred")
            db.all_kept(what + ": the deferred route's absent destination")
            assert torch.equal(gm.bits(), direct[0]) and torch.equal(ws.bits(), direct[1]), what + ": the deferred route's first launch differs"
            later = _reduce_deferred(lib, dev, ws, P, C, what)
            assert torch.equal(later.t.view(torch.int32), direct[2]), what + ": deferred db is not the direct route's bits"


# ---- refusals: argument checks that return before any launch
def test_refusals_leave_the_outputs_alone():
    lib, dev = _lib(), _dev()
    st = _stream(dev)
    N, D, DX = 5, 65, 1025
    gen = _gen(4)
    t = {k: _inp(_grid((N, DX), gen), dev) for k in ("a", "res", "dy", "s", "z", "hh", "x")}
    v = {k: _inp(_grid((DX,), gen), dev) for k in ("bias", "gamma", "beta")}
    stats = _inp(torch.ones((N, 2)), dev)
    outs = [_Out(dev, N, 3 * DX) for _ in range(5)]
    y, s, da, dA, dB = outs
    ws = _Out(dev, N * 3 * DX)
    big = 4 * N * 3 * DX
    p = {k: _ptr(x) for k, x in {**t, **v}.items()}
    assert lib.etm_block_row_groups(DX) == EUNSUPPORTED

    def fwd(a=p["a"], bias=p["bias"], relu=0, gamma=p["gamma"], out=y.ptr, n=N, d=D):
        return lib.etm_ln_train_fwd(a, bias, relu, p["res"], gamma, p["beta"], EPS, out, s.ptr, None, n, d, st)

    def bwd(dy=p["dy"], a=p["a"], bias=p["bias"], relu=0, dda=da.ptr, w=ws.ptr, nb=big, n=N, d=D):
        return lib.etm_ln_train_bwd(dy, None, p["s"], _ptr(stats), p["gamma"], a, bias, relu, y.ptr, dda, s.ptr, w, nb, n, d, st)

    def bwd1(dout=p["dy"], w=ws.ptr, nb=big, n=N, d=D):
        return lib.etm_gate_train_bwd1(dout, None, p["z"], p["hh"], p["x"], dA.ptr, dB.ptr, y.ptr, s.ptr, w, nb, n, d, st)

    def add_ln(b=p["res"], relu=0, bias=p["bias"], n=N, d=D):
        return lib.etm_add_layernorm(p["a"], bias, relu, b, p["gamma"], p["beta"], EPS, y.ptr, n, d, st)

    def colsum(yy=None, gm=None, w=ws.ptr, nb=big, n=N, c=D):
        return lib.etm_relu_bwd_colsum(p["dy"], yy, gm, s.ptr, w, nb, n, c, st)

    cases = [("ln fwd at D = 1025", EUNSUPPORTED, lambda: fwd(d=DX)), ("ln bwd at D = 1025", EUNSUPPORTED, lambda: bwd(d=DX)),
             ("gate bwd1 at D = 1025", EUNSUPPORTED, lambda: bwd1(d=DX)), ("add_layernorm at D = 1025", EUNSUPPORTED, lambda: add_ln(d=DX)),
             ("ln fwd: relu without a_bias", EINVAL, lambda: fwd(bias=None, relu=1)),
             ("ln bwd: relu without a", EINVAL, lambda: bwd(a=None, relu=1)), ("ln bwd: relu without a_bias", EINVAL, lambda: bwd(bias=None, relu=1)),
             ("ln bwd: relu without da", EINVAL, lambda: bwd(dda=None, relu=1)),
             ("relu_bwd_colsum: y without gm", EINVAL, lambda: colsum(yy=p["s"])),
             ("ln fwd N = 0", EINVAL, lambda: fwd(n=0)), ("ln fwd D = 0", EINVAL, lambda: fwd(d=0)), ("ln fwd no a", EINVAL, lambda: fwd(a=None)),
             ("ln fwd no gamma", EINVAL, lambda: fwd(gamma=None)), ("ln fwd no y", EINVAL, lambda: fwd(out=None)),
             ("ln bwd N = 0", EINVAL, lambda: bwd(n=0)), ("ln bwd D = 0", EINVAL, lambda: bwd(d=0)), ("ln bwd no dy", EINVAL, lambda: bwd(dy=None)),
             ("ln bwd no workspace", EINVAL, lambda: bwd(w=None)),
             ("gate bwd1 N = 0", EINVAL, lambda: bwd1(n=0)), ("gate bwd1 D = 0", EINVAL, lambda: bwd1(d=0)), ("gate bwd1 no dout", EINVAL, lambda: bwd1(dout=None)),
             ("gate bwd1 no workspace", EINVAL, lambda: bwd1(w=None)),
             ("gate rz no x", EINVAL, lambda: lib.etm_gate_train_rz(p["a"], p["res"], p["bias"], None, y.ptr, s.ptr, da.ptr, N, D, st)),
             ("gate rz N = 0", EINVAL, lambda: lib.etm_gate_train_rz(p["a"], p["res"], p["bias"], p["x"], y.ptr, s.ptr, da.ptr, 0, D, st)),
             ("gate out no hh", EINVAL, lambda: lib.etm_gate_train_out(p["a"], p["res"], p["z"], p["x"], None, y.ptr, N, D, st)),
             ("gate out D = 0", EINVAL, lambda: lib.etm_gate_train_out(p["a"], p["res"], p["z"], p["x"], s.ptr, y.ptr, N, 0, st)),
             ("gate bwd2 no dx2", EINVAL, lambda: lib.etm_gate_train_bwd2(p["dy"], p["x"], p["z"], p["s"], dA.ptr, dB.ptr, None, N, D, st)),
             ("gate bwd2 N = 0", EINVAL, lambda: lib.etm_gate_train_bwd2(p["dy"], p["x"], p["z"], p["s"], dA.ptr, dB.ptr, y.ptr, 0, D, st)),
             ("add_layernorm no b", EINVAL, lambda: add_ln(b=None)), ("add_layernorm N = 0", EINVAL, lambda: add_ln(n=0)),
             ("gru_gate_rz no z", EINVAL, lambda: lib.etm_gru_gate_rz(p["a"], p["res"], p["bias"], p["x"], y.ptr, None, N, D, st)),
             ("gru_gate_out D = 0", EINVAL, lambda: lib.etm_gru_gate_out(p["a"], p["res"], p["z"], p["x"], y.ptr, N, 0, st)),
             ("relu_bwd_colsum N = 0", EINVAL, lambda: colsum(n=0)), ("relu_bwd_colsum C = 0", EINVAL, lambda: colsum(c=0)),
             ("relu_bwd_colsum no workspace", EINVAL, lambda: colsum(w=None)),
             ("ln bwd: workspace 4 bytes short", EWORKSPACE, lambda: bwd(nb=lib.etm_ln_train_bwd_workspace_bytes(N, D) - 4)),
             ("gate bwd1: workspace 4 bytes short", EWORKSPACE, lambda: bwd1(nb=lib.etm_gate_train_bwd_workspace_bytes(N, D) - 4)),
             ("relu_bwd_colsum: workspace 4 bytes short", EWORKSPACE, lambda: colsum(nb=lib.etm_relu_bwd_colsum_workspace_bytes(N, D) - 4))]
    for name, code, call in cases:
        assert call() == code, name
    torch.cuda.synchronize(dev)
    for o in outs + [ws]:
        o.all_kept("a refused call")


# ---- the rollout twins
@pytest.mark.parametrize("D", WIDTHS)
def test_rollout_twins(D):
    """etm_add_layernorm (no bias; bias; bias + ReLU -- the residual is not optional there) and etm_gru_gate_rz / _out at every width,
    N in TWIN_ROWS: against float64 by the training kernels' metrics and floors, and EQUAL to the training kernels' y / z, rx, out
    on the same operands: the expressions are the same, the zeros that add_layernorm_kernel adds for its column groups beyond NJ
    change no sum (x + 0 = x, and no partial sum is -0: they start from +0)."""
    lib, dev = _lib(), _dev()
    st = _stream(dev)
    for N in TWIN_ROWS:
        for bias, relu in ((False, False), (True, False), (True, True)):
            what = f"add_layernorm D={D} N={N} bias={int(bias)} relu={int(relu)}"
            o = _ln_operands(D, N, bias, relu, True, False, 300 * D + 10 * N + 2 * bias + relu)
            d = {k: _inp(v, dev) if isinstance(v, torch.Tensor) else None for k, v in o.items()}
            y64 = _ln_fwd_ref(o["a"], o["bias"], relu, o["res"], o["gamma"], o["beta"], torch.float64)[0]
            y32 = _ln_fwd_ref(o["a"], o["bias"], relu, o["res"], o["gamma"], o["beta"], torch.float32)[0]
            out, y = _Out(dev, N, D), _Out(dev, N, D)
            _twice(dev, [out], lambda: _ok(lib.etm_add_layernorm(_ptr(d["a"]), _ptr(d["bias"]), int(relu), _ptr(d["res"]), _ptr(d["gamma"]), _ptr(d["beta"]),
                                                                 EPS, out.ptr, N, D, st), "etm_add_layernorm"), what)
            comp = (o["gamma"].abs().max() + o["beta"].abs().max()).expand(N, 1)
            _judge("add_ln y", _row_err(out.cpu(), y64, comp), _row_err(y32, y64, comp), what)
            _ok(lib.etm_ln_train_fwd(_ptr(d["a"]), _ptr(d["bias"]), int(relu), _ptr(d["res"]), _ptr(d["gamma"]), _ptr(d["beta"]), EPS, y.ptr, None, None,
                                     N, D, st), "etm_ln_train_fwd")
            torch.cuda.synchronize(dev)
            assert torch.equal(out.bits(), y.bits()), what + ": not the training kernel's bits"
        what = f"gru_gate D={D} N={N}"
        o = _gate_operands(D, N, 700 * D + N)
        z_in = _normal(_gate_fwd_ref(o, torch.float64)["z"].float())
        f64, f32 = _gate_fwd_ref(o, torch.float64, z_in), _gate_fwd_ref(o, torch.float32, z_in)
        d = {k: _inp(v, dev) for k, v in o.items()}
        dz = _inp(z_in, dev)
        rx, z, out = _Out(dev, N, D), _Out(dev, N, D), _Out(dev, N, D)
        _twice(dev, [rx, z], lambda: _ok(lib.etm_gru_gate_rz(_ptr(d["A"]), _ptr(d["B"]), _ptr(d["bg"]), _ptr(d["x"]), rx.ptr, z.ptr, N, D, st),
                                         "etm_gru_gate_rz"), what)
        _twice(dev, [out], lambda: _ok(lib.etm_gru_gate_out(_ptr(d["A"]), _ptr(d["C"]), _ptr(dz), _ptr(d["x"]), out.ptr, N, D, st), "etm_gru_gate_out"), what)
        for k, t in (("rx", rx), ("z", z), ("out", out)):
            comp = torch.ones((N, 1)) if k == "z" else o["x"]
            _judge("gru " + k, _row_err(t.cpu(), f64[k], comp), _row_err(f32[k], f64[k], comp), what)
        assert bool(torch.isfinite(torch.stack((rx.cpu(), z.cpu(), out.cpu()))).all()), what
        tr, tz, trx, thh, tout = (_Out(dev, N, D) for _ in range(5))
        _ok(lib.etm_gate_train_rz(_ptr(d["A"]), _ptr(d["B"]), _ptr(d["bg"]), _ptr(d["x"]), tr.ptr, tz.ptr, trx.ptr, N, D, st), "etm_gate_train_rz")
        _ok(lib.etm_gate_train_out(_ptr(d["A"]), _ptr(d["C"]), _ptr(dz), _ptr(d["x"]), thh.ptr, tout.ptr, N, D, st), "etm_gate_train_out")
        torch.cuda.synchronize(dev)
        for k, mine, theirs in (("rx", rx, trx), ("z", z, tz), ("out", out, tout)):
            assert torch.equal(mine.bits(), theirs.bits()), f"{what}: {k} is not the training kernel's bits"


# ---- the wrappers, once per NJ bucket
@pytest.mark.parametrize("D", WRAPPER_WIDTHS)
def test_wrappers_plumbing_once_per_bucket(D):
    """ops.fused_layernorm(bias, res, relu, fork=True) and ops.gru_gate_train at N = 9 against float64 autograd of the module
    formulas: the two outputs of the fork share one storage, its consumers' gradients are added on load, every gradient lands in its
    place.  (The gate's five products are library GEMMs here, so its bounds are mostly their e32.)"""
    from etm import ops
    from transformer import GRUGate
    lib, dev = _lib(), _dev()
    assert D in WIDTHS and len({lib.etm_block_row_groups(d) for d in WRAPPER_WIDTHS}) == len(WRAPPER_WIDTHS) == 7
    N = 9
    o = _ln_operands(D, N, True, True, True, True, 40 * D)
    names = ("a", "bias", "res", "gamma", "beta")

    def ln_ref(dt):
        t = [o[k].to(dt).clone().requires_grad_(True) for k in names]
        y = torch.nn.functional.layer_norm(torch.relu(t[0] + t[1]) + t[2], (D,), t[3], t[4], EPS)
        return [y.detach()] + list(torch.autograd.grad(y, t, (o["dy"] + o["dy2"]).to(dt)))
    r64, r32 = ln_ref(torch.float64), ln_ref(torch.float32)
    norm = torch.nn.LayerNorm(D, eps=EPS).to(dev)
    with torch.no_grad():
        norm.weight.copy_(o["gamma"])
        norm.bias.copy_(o["beta"])
    a, bias, res = (o[k].to(dev).requires_grad_(True) for k in ("a", "bias", "res"))
    y1, y2 = ops.fused_layernorm(a, norm, bias=bias, res=res, relu=True, fork=True)
    assert y1.data_ptr() == y2.data_ptr()
    got = [y1.detach().cpu()] + [g.cpu() for g in torch.autograd.grad([y1, y2], [a, bias, res, norm.weight, norm.bias], [o["dy"].to(dev), o["dy2"].to(dev)])]
    what = f"fused_layernorm(fork=True) D={D}"
    go = (o["dy"] + o["dy2"]).double()
    _judge("wrap ln y", _row_err(got[0], r64[0]), _row_err(r32[0], r64[0]), what)
    for i in (1, 3):
        _judge("wrap ln grads", _row_err(got[i], r64[i], go), _row_err(r32[i], r64[i], go), f"{what} d {names[i - 1]}")
    _, s64, mean64, rstd64 = _ln_fwd_ref(o["a"], o["bias"], True, o["res"], o["gamma"], o["beta"], torch.float64)
    xh = (s64 - mean64[:, None]) * rstd64[:, None]
    addends = _ln_bwd_ref(o["dy"], o["dy2"], s64, mean64, rstd64, o["gamma"], o["a"].double() + o["bias"].double(), torch.float64)[4]
    for i, terms in ((2, addends), (4, go * xh), (5, go)):
        _judge("wrap ln colsums", _col_err(got[i], terms), _col_err(r32[i], terms), f"{what} d {names[i - 1]}")
    _exact(got[5], go.sum(0), what + ": d beta")

    torch.manual_seed(D)
    gate = GRUGate(D, 2.0).to(dev)
    gen = _gen(41 * D)
    x, yv, g1, g2 = (torch.randn((N, D), generator=gen) for _ in range(4))
    params = [(n, p.detach().cpu()) for n, p in gate.named_parameters()]

    def gate_ref(dt):
        w = {n: p.to(dt).clone().requires_grad_(True) for n, p in params}
        xx, yy = x.to(dt).clone().requires_grad_(True), yv.to(dt).clone().requires_grad_(True)
        lin = lambda name, v: v @ w[name + ".weight"].t()
        r = torch.sigmoid(lin("Wr", yy) + lin("Ur", xx))
        z = torch.sigmoid(lin("Wz", yy) + lin("Uz", xx) - w["bg"])
        out = (1 - z) * xx + z * torch.tanh(lin("Wg", yy) + lin("Ug", r * xx))
        return [out.detach()] + list(torch.autograd.grad(out, [xx, yy] + [w[n] for n, _ in params], (g1 + g2).to(dt)))
    assert {n for n, _ in params} == {"bg"} | {f"{m}.weight" for m in ("Wr", "Ur", "Wz", "Uz", "Wg", "Ug")}, [n for n, _ in params]
    r64, r32 = gate_ref(torch.float64), gate_ref(torch.float32)
    xd, yd = x.to(dev).requires_grad_(True), yv.to(dev).requires_grad_(True)
    o1, o2 = ops.gru_gate_train(gate, xd, yd, fork=True)
    assert o1.data_ptr() == o2.data_ptr()
    got = [o1.detach().cpu()] + [g.cpu() for g in torch.autograd.grad([o1, o2], [xd, yd] + list(gate.parameters()), [g1.to(dev), g2.to(dev)])]
    what = f"gru_gate_train(fork=True) D={D}"
    _judge("wrap gate out", _row_err(got[0], r64[0], x), _row_err(r32[0], r64[0], x), what)
    for i, name in enumerate(["x", "y"] + [n for n, _ in params], start=1):
        w64 = r64[i].reshape(r64[i].shape[0], -1) if r64[i].dim() == 2 else r64[i].reshape(1, -1)
        shape = w64.shape
        _judge("wrap gate grads", _row_err(got[i].reshape(shape), w64), _row_err(r32[i].reshape(shape), w64), f"{what} d {name}")
