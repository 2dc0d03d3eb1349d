"""The KL penalty (``kl_penalty``) on the device: the three categorical loss routes and the Box route with ``coef * KL`` in the loss and its
gradient in d logits, the refusals of the four entries, and the trainer in all three forms of the step.

Bounds.  Every comparison of a device gradient with float64 uses the project's rule for the exact-KL statistic (tests/test_exact_kl_gpu.py):
4 x the largest error, over the whole case list of the route, of the same loss evaluated by torch autograd in float32 on the same operands
-- measured again by every run of this file (the fixtures ``fused_runs`` / ``box_runs`` / ``ppo_runs``; nothing is fixed in advance); the
margin of 4 covers another, equally valid summation order.  An error is max |x - ref| over a quantity's elements, in the quantity's own
units as that rule's is; every quantity (gm_p, d Wb, d bb, d log_std, d_logits) has a bound of its own, one for the total gradient and
one for the difference (penalty run) - (twin), which carries the rounding of the two totals.  Both errors are printed per case, next to
the largest of them relative to the largest element of the float64 total (information only).
The separate-heads kernel forms the penalty's p_j as exp((logit_j - max) - log(sum)), not from the l_j = logit_j - lse of its other
terms: a first version reused l_j, as the fused kernels do, and missed this bound on one case (N = 1, (12,), unmasked, coef 7: 9.56e-7
against 4 x 2.33e-7) -- the largest logit is 4.04 and lse 4.32 there, half a spacing of lse (2.4e-7) goes into p_j = 0.757 next to
p_old_j = 0.780 and coef multiplies it, while torch's log-softmax is exact at the largest column.  With the sampler's rows of equal
logits that route's term is therefore of rounding size, bounded from the number format in the test below, and exactly 0 only in the
fused kernels, where the issue asks for it.
The float64 reference of the penalty's part is ``utils.categorical_kl_grad`` /
``utils.gaussian_kl_grad`` on the kernel's own ``logits`` output times ``coef * scale``, pushed through ``Wb`` and the ReLU mask in float64;
the float32 torch evaluation differentiates ``L_ppo + coef * sum p_old (log p_old - log p)`` (Box: the closed form) as written.
The value term sends no gradient to the policy head: ``gm_v`` and ``d_value`` are held to the twin's under ``==`` instead.
N = 1: the advantage statistics of one sample have no standard deviation (NaN in every policy gradient, with or without the key), so the
N = 1 cases hand the kernels the statistics of a larger minibatch (count 2, mean 0, M2 1), as a data-parallel run does.
profiles/r19/kl_penalty.txt records the pairs as measured on the MI355X."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import resume_helpers as rh
import test_analytic_kl_gpu as ak
import test_exact_kl_gpu as ek

pytestmark = pytest.mark.gpu

SENTINEL, EINVAL = ek.SENTINEL, ek.EINVAL
CLIP, VF, BETA = ek.CLIP, ek.VF, ek.BETA
HALF_LOG_2PI = 0.918938533204672742
COEFS = (0.2, 7.0)
_dev, _offsets, _pack = ek._dev, ek._offsets, ek._pack


@pytest.fixture(autouse=True)
def _collect_between_tests():
    gc.collect()
    yield
    gc.collect()


def _eq(a, b):
    """``==`` on every element (a -0 equals a +0), no NaN anywhere."""
    a, b = (t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in (a, b))
    return a.shape == b.shape and not bool(torch.isnan(a).any()) and bool(torch.equal(a, b))


def _c32(c):
    return float(np.float32(c))


def _coef_word(c):
    return torch.tensor([c], dtype=torch.float32, device=_dev())


def _normalised(adv, stats3, dt):
    """The kernels' normalised advantage from the statistics they are handed: (a - mean) / (sqrt(M2 / (count - 1)) + 1e-8)."""
    cnt, mean, m2 = (stats3[i].to(dt) for i in range(3))
    return (adv.to(dt) - mean) / (torch.sqrt(m2 / (cnt - 1.0)) + 1e-8)


def _given_stats(p):
    if p.N == 1:
        p.stats3 = torch.tensor([2.0, 0.0, 1.0], device=_dev())


def _surrogate(ratio, a_n):
    return torch.min(ratio * a_n, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * a_n)


def _cat_terms(logits, br, valid, actions, old_logp, a_n, old_logps):
    """(the policy and entropy terms of the loss, K = sum_n sum_b sum_{valid j, p_old_j > 0} p_old_j (log p_old_j - log p_j) / (N B)) in
    the dtype of ``logits``, as plain torch operations."""
    N, B = logits.shape[0], len(br)
    pol = ent = kl = 0.0
    zero = torch.zeros((), dtype=logits.dtype, device=logits.device)
    for b, (off, a) in enumerate(zip(_offsets(br), br)):
        v = valid[:, off:off + a]
        lsm = torch.log_softmax(logits[:, off:off + a].masked_fill(~v, float("-inf")), dim=-1)
        lp = lsm.gather(1, actions[:, b:b + 1])[:, 0]
        pol = pol + _surrogate(torch.exp(lp - old_logp[:, b]), a_n).sum()
        ent = ent - (lsm.exp() * lsm.masked_fill(~v, 0.0)).sum()
        old = old_logps[:, off:off + a].to(logits.dtype)
        use = v & (old > float("-inf"))
        kl = kl + torch.where(use, old.exp() * (torch.where(use, old, zero) - torch.where(use, lsm, zero)), zero).sum()
    return -(pol / (N * B) + BETA * ent / N), kl / (N * B)


def _err(x, ref):
    return float((x.double() - ref).abs().max())


def _rel(x, ref, scale):
    return _err(x, ref) / scale


def _scale(ref):
    s = float(ref.abs().max())
    return s if s > 0 else 1.0


def _loss_rounding(twin8, pen8, c):
    """out8[2] of the penalty run against the twin's out8[2] + c * out8[4] in float64 -> (error, bound).  The kernel rounds the product
    and the sum once each (or the two as one fused operation): at most half a spacing of c * kl plus half a spacing of the result."""
    t2, t4, got = float(twin8[2]), float(twin8[4]), float(pen8[2])
    want = t2 + _c32(c) * t4
    bound = 0.5 * float(np.spacing(np.float32(abs(_c32(c) * t4)))) + 0.5 * float(np.spacing(np.float32(abs(want))))
    return abs(got - want), bound, want


# ================================================================== 1. the fused route, categorical
FUSED_CASES = ek.FUSED_CASES


class _Fused(ek._Fused):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        _given_stats(self)

    def pen(self, c, old_logps=None, coef_ptr=None, expect=0):
        lib = self.lib
        old = self.old_logps if old_logps is None else old_logps
        o = self._outputs(lib.etm_heads_loss_kl_row_floats(self.hid, self.A))
        ws = torch.full((max(lib.etm_heads_loss_kl_workspace_bytes(self.N, self.hid, self.A), 4),), 0x5A, dtype=torch.uint8, device=_dev())
        word = _coef_word(c)
        entry = lib.etm_heads_loss_kl_penalty if self.B == 1 else lib.etm_heads_loss_branched_kl_penalty
        rc = entry(*self._head(o, ws), *self._shape(), self.words.data_ptr() if self.masked else None, old.data_ptr(), old.stride(0),
                   word.data_ptr() if coef_ptr is None else coef_ptr, torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, expect)
        torch.cuda.synchronize()
        o["ws"] = ws
        return o

    def grads(self, o):
        """(gm_p, d Wb, d bb) of an output set."""
        hid, A = self.hid, self.A
        return o["gm_p"], o["sums"][3 * hid:(3 + A) * hid].view(A, hid), o["sums"][(3 + A) * hid:(3 + A) * hid + A]

    def _leaves(self, dt):
        return [t.detach().to(dt).requires_grad_(True) for t in (self.pre_p, self.wb, self.bb)]

    def _terms(self, leaves, dt):
        pre_p, wb, bb = leaves
        hp = torch.relu(pre_p + self.b_lp.to(dt))
        logits = hp @ wb.t() + bb
        v = torch.as_tensor(self.valid, device=_dev())
        return _cat_terms(logits, self.br, v, self.actions, self.old_logp.to(dt), _normalised(self.adv, self.stats3, dt), self.old_logps), hp

    def float64(self, logits_kernel, c):
        """(total, difference) of (gm_p, d Wb, d bb) in float64."""
        from utils import categorical_kl_grad
        leaves = self._leaves(torch.float64)
        (L, _), hp = self._terms(leaves, torch.float64)
        twin = torch.autograd.grad(L, leaves)
        G = torch.as_tensor(categorical_kl_grad(self.old_logps.cpu().numpy(), logits_kernel.cpu().numpy(), self.br,
                                                _pack(self.valid) if self.masked else None, np.float64), device=_dev())
        s = _c32(c) / (self.N * self.B)
        relu = ((self.pre_p + self.b_lp) > 0).double()                 # (the kernel's own mask: the float32 sum's sign)
        diff = (s * (G @ leaves[1].detach()) * relu, s * (G.t() @ hp.detach()), s * G.sum(0))
        return [t + d for t, d in zip(twin, diff)], diff, G

    def float32(self, c):
        leaves = self._leaves(torch.float32)
        (L, K), _ = self._terms(leaves, torch.float32)
        twin = torch.autograd.grad(L, leaves, retain_graph=True)
        total = torch.autograd.grad(L + _c32(c) * K, leaves)
        return total, [a - b for a, b in zip(total, twin)]


QUANTITIES = ("gm_p", "d Wb", "d bb", "d log_std")


def _gradient_errors(p, twin, pen, ref_total, ref_diff, t_total, t_diff):
    """-> {quantity: dict(k_total, k_diff, t_total, t_diff, scale)}: the kernel's and the float32 torch evaluation's largest |error| of
    the total gradient and of the difference to the twin, and the largest |element| of the float64 total."""
    k_total, k_diff = p.grads(pen), [a - b for a, b in zip(p.grads(pen), p.grads(twin))]
    return {name: dict(k_total=_err(k_total[i], ref_total[i]), k_diff=_err(k_diff[i], ref_diff[i]), t_total=_err(t_total[i], ref_total[i]),
                       t_diff=_err(t_diff[i], ref_diff[i]), scale=_scale(ref_total[i])) for i, name in zip(range(len(ref_total)), QUANTITIES)}


def _bounds(out):
    """{(quantity, 'total' | 'diff'): 4 x the largest float32 torch error over the case list} and the kernel's largest errors."""
    recs = [r["coefs"][c]["grad"] for r in out.values() for c in COEFS]
    names = [n for n in QUANTITIES if n in recs[0]]
    bound = {(n, kind): 4.0 * max(g[n]["t_" + kind] for g in recs) for n in names for kind in ("total", "diff")}
    worst = {(n, kind): max(g[n]["k_" + kind] for g in recs) for n in names for kind in ("total", "diff")}
    return bound, worst


def _grad_line(grad):
    rel = lambda key: max(g[key] / g["scale"] for g in grad.values())
    return (f"total: torch fp32 {rel('t_total'):.3e} kernel {rel('k_total'):.3e}; difference: torch fp32 {rel('t_diff'):.3e} kernel "
            f"{rel('k_diff'):.3e} (largest over the quantities, relative to the largest element of the float64 total)")


def _assert_gradients(grad, bound, what):
    for name, g in grad.items():
        for kind in ("diff", "total"):
            assert g["k_" + kind] <= bound[(name, kind)], (what, name, kind, g, bound[(name, kind)])


def _fid(c):
    return ek._fid(c)


@pytest.fixture(scope="module")
def fused_runs():
    """Every case once: the twin (etm_heads_loss_kl / _branched_kl), the penalty entry at coef 0 and at both coefficients, the float64
    and float32 references -> ({case: record of small values}, the bound for the totals, the bound for the differences)."""
    out = {}
    for case in FUSED_CASES:
        p = _Fused(*case)
        twin, zero = p.kl(), p.pen(0.0)
        assert bool(torch.isfinite(twin["gm_p"]).all()) and bool(torch.isfinite(twin["sums"]).all()), case
        rec = dict(zero={k: _eq(twin[k], zero[k]) for k in ("gm_p", "gm_v", "sums", "logits", "value")},
                   zero8=_eq(twin["out8"][:7], zero["out8"][:7]), zero7=float(zero["out8"][7]), coefs={})
        never = torch.as_tensor(~p.valid.any(axis=0), device=_dev())       # columns that no sample of the case allows
        for c in COEFS:
            pen = p.pen(c)
            ref_total, ref_diff, G = p.float64(pen["logits"], c)
            t_total, t_diff = p.float32(c)
            grad = _gradient_errors(p, twin, pen, ref_total, ref_diff, t_total, t_diff)
            lerr, lbound, _ = _loss_rounding(twin["out8"], pen["out8"], c)
            t8, p8 = ek._bits(twin["out8"]), ek._bits(pen["out8"])
            _, wb_t, bb_t = p.grads(twin)
            _, wb_p, bb_p = p.grads(pen)
            rec["coefs"][c] = dict(same8=bool(np.array_equal(t8[[0, 1, 3, 4, 5, 6]], p8[[0, 1, 3, 4, 5, 6]])), out7=float(pen["out8"][7]),
                                   loss_err=lerr, loss_bound=lbound, grad=grad,
                                   same_rest=all(_eq(twin[k], pen[k]) for k in ("gm_v", "logits", "value")),
                                   same_stat_sums=ek._same(twin["sums"][(3 + p.A) * p.hid + p.A:], pen["sums"][(3 + p.A) * p.hid + p.A:]),
                                   never=int(never.sum()), never_same=_eq(wb_t[never], wb_p[never]) and _eq(bb_t[never], bb_p[never]),
                                   invalid_zero=bool((G[torch.as_tensor(~p.valid, device=_dev())] == 0).all()),
                                   moved=not _eq(twin["gm_p"], pen["gm_p"]))
            print(f"[fused {_fid(case)} c={c}] {_grad_line(grad)}; loss {lerr:.2e} (bound {lbound:.2e})")
        out[case] = rec
        del p, twin, zero, pen
    bound, worst = _bounds(out)
    for key in bound:
        print(f"[fused] {key[0]} {key[1]}: bound 4 x {bound[key] / 4:.3e}, largest kernel error {worst[key]:.3e}")
    return out, bound


@pytest.mark.parametrize("case", FUSED_CASES, ids=[_fid(c) for c in FUSED_CASES])
def test_fused_coefficient_zero_reproduces_the_twin(fused_runs, case):
    r = fused_runs[0][case]
    assert all(r["zero"].values()), r["zero"]
    assert r["zero8"], "out8[0..6]"
    assert r["zero7"] == 0.0


@pytest.mark.parametrize("c", COEFS)
@pytest.mark.parametrize("case", FUSED_CASES, ids=[_fid(c) for c in FUSED_CASES])
def test_fused_penalty_gradient_against_float64(fused_runs, case, c):
    r = fused_runs[0][case]["coefs"][c]
    assert r["same8"], "out8[0, 1, 3, 4, 5, 6] are the twin's bits"
    assert r["out7"] == _c32(c)
    assert r["loss_err"] <= r["loss_bound"], (r["loss_err"], r["loss_bound"])
    assert r["same_rest"], "gm_v, logits, value"
    assert r["same_stat_sums"], "d bv and the statistic sums of the row"
    assert r["invalid_zero"] and r["never_same"], "a masked-out column gains exactly 0"
    _assert_gradients(r["grad"], fused_runs[1], (case, c))
    if case[0] > 1 or not case[3]:
        assert r["moved"], "the penalty reached the gradient"


@pytest.mark.parametrize("hid", [64, 512])
@pytest.mark.parametrize("N", [37, 2059])
def test_fused_columns_masked_in_every_sample_keep_the_twins_rows(N, hid):
    """A constant mask: the rows of d Wb and the elements of d bb of its invalid columns are the twin's (zeros), exactly."""
    br = (2, 1, 5)
    keep = np.array([True, False, True, True, False, True, True, False])
    p = _Fused(N, hid, br, True)
    p.valid = np.broadcast_to(keep, (N, 8)).copy()
    p.words = torch.as_tensor(_pack(p.valid), device=_dev())
    idx = [np.flatnonzero(keep[off:off + a]) for off, a in zip(_offsets(br), br)]
    g = torch.Generator().manual_seed(5)
    comp = torch.stack([torch.randint(0, len(ix), (N,), generator=g) for ix in idx], dim=1)
    p.actions = torch.stack([torch.as_tensor(ix)[comp[:, b]] for b, ix in enumerate(idx)], dim=1).to(_dev()).contiguous()
    p.old_logps = ek._old_rows(p.logits, br, p.valid, g, _dev())
    twin, pen = p.kl(), p.pen(7.0)
    _, wb_t, bb_t = p.grads(twin)
    _, wb_p, bb_p = p.grads(pen)
    dead = torch.as_tensor(~keep, device=_dev())
    assert _eq(wb_t[dead], wb_p[dead]) and _eq(bb_t[dead], bb_p[dead])
    assert not bool(wb_p[dead].any()) and not bool(bb_p[dead].any())
    assert not _eq(wb_t[~dead], wb_p[~dead]), "the other rows moved"


@pytest.mark.parametrize("c", [0.2, 7.0, 100.0])
@pytest.mark.parametrize("case", [(1, 64, (2,), False), (9, 512, (2, 1, 5), True), (2059, 64, (3, 3), False), (37, 512, (8,), True)], ids=_fid)
def test_fused_equal_policies_add_exactly_nothing(case, c):
    """The old rows are what the sampler stages for the kernel's own logits (one arithmetic: every p_j - p_old_j is exactly 0)."""
    p = _Fused(*case)
    old = ek._sampler_rows(p.logits, p.br, p.words if p.masked else None)
    twin, pen = p.kl(old_logps=old), p.pen(c, old_logps=old)
    for k in ("gm_p", "gm_v", "sums", "logits", "value"):
        assert _eq(twin[k], pen[k]), k
    assert _eq(twin["out8"][:7], pen["out8"][:7]) and float(pen["out8"][7]) == _c32(c) and float(pen["out8"][4]) == 0.0


# ================================================================== 2. the fused route, Box
BOX_CASES = [(N, hid, A) for A in (1, 3, 8) for N in (1, 9, 37, 2059) for hid in (64, 384, 512)]


class _Box(ak._Loss):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        _given_stats(self)

    def pen(self, c, old_mean=None, old_log_std=None, coef_ptr=None, expect=0):
        lib = self.lib
        old_mean = self.old_mean if old_mean is None else old_mean
        old_log_std = self.old_log_std if old_log_std is None else old_log_std
        o = self._outputs(lib.etm_heads_loss_gaussian_kl_row_floats(self.hid, self.A))
        ws = torch.full((max(lib.etm_heads_loss_gaussian_kl_workspace_bytes(self.N, self.hid, self.A), 4),), 0x5A, dtype=torch.uint8, device=_dev())
        word = _coef_word(c)
        rc = lib.etm_heads_loss_gaussian_kl_penalty(*self._head(o, ws), old_mean.data_ptr(), old_mean.stride(0), old_log_std.data_ptr(),
                                                    word.data_ptr() if coef_ptr is None else coef_ptr, torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, expect)
        torch.cuda.synchronize()
        o["ws"] = ws
        return o

    def grads(self, o):
        """(gm_p, d Wb, d bb, d log_std) of an output set."""
        hid, A = self.hid, self.A
        base = (3 + A) * hid
        return o["gm_p"], o["sums"][3 * hid:base].view(A, hid), o["sums"][base:base + A], o["sums"][base + A + 6:base + 2 * A + 6]

    def _leaves(self, dt):
        return [t.detach().to(dt).requires_grad_(True) for t in (self.pre_p, self.wb, self.bb, self.log_std)]

    def _terms(self, leaves, dt, old_mean, old_log_std):
        pre_p, wb, bb, log_std = leaves
        hp = torch.relu(pre_p + self.b_lp.to(dt))
        mu = hp @ wb.t() + bb
        sigma = log_std.exp()
        z = (self.xact.to(dt) - mu) / sigma
        lp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(1)
        pol = _surrogate(torch.exp(lp - self.old_logp.to(dt)), _normalised(self.adv, self.stats3, dt)).mean()
        ent = (0.5 + HALF_LOG_2PI + log_std).sum()
        d = old_log_std.to(dt) - log_std
        q = (old_mean.to(dt) - mu) / sigma
        K = (0.5 * torch.expm1(2.0 * d) - d).sum() + (0.5 * q * q).sum(1).mean()
        return -(pol + BETA * ent), K, hp

    def float64(self, mu_kernel, c, old_mean, old_log_std):
        from utils import gaussian_kl_grad
        leaves = self._leaves(torch.float64)
        L, _, hp = self._terms(leaves, torch.float64, old_mean, old_log_std)
        twin = torch.autograd.grad(L, leaves)
        gm, gl = gaussian_kl_grad(old_mean.cpu().numpy(), old_log_std.cpu().numpy(), mu_kernel.cpu().numpy(), self.log_std.cpu().numpy(), np.float64)
        G, gl = torch.as_tensor(gm, device=_dev()), torch.as_tensor(gl, device=_dev())
        s = _c32(c) / self.N
        relu = ((self.pre_p + self.b_lp) > 0).double()
        diff = (s * (G @ leaves[1].detach()) * relu, s * (G.t() @ hp.detach()), s * G.sum(0), s * gl)
        return [t + d for t, d in zip(twin, diff)], diff

    def float32(self, c, old_mean, old_log_std):
        leaves = self._leaves(torch.float32)
        L, K, _ = self._terms(leaves, torch.float32, old_mean, old_log_std)
        twin = torch.autograd.grad(L, leaves, retain_graph=True)
        total = torch.autograd.grad(L + _c32(c) * K, leaves)
        return total, [a - b for a, b in zip(total, twin)]


def _bid(c):
    return f"N{c[0]}_hid{c[1]}_A{c[2]}"


@pytest.fixture(scope="module")
def box_runs():
    """As ``fused_runs`` against etm_heads_loss_gaussian_kl, the d log_std elements of the row included.  Every case twice: with another
    old log-std (the case's own) and with equal log-stds."""
    out = {}
    for case in BOX_CASES:
        p = _Box(*case)
        for name, ols in (("other log_std", p.old_log_std), ("equal log_std", p.log_std.clone())):
            twin, zero = p.kl(old_log_std=ols), p.pen(0.0, old_log_std=ols)
            assert bool(torch.isfinite(twin["gm_p"]).all()) and bool(torch.isfinite(twin["sums"]).all()), case
            rec = dict(zero={k: _eq(twin[k], zero[k]) for k in ("gm_p", "gm_v", "sums", "logits", "value")},
                       zero8=_eq(twin["out8"][:7], zero["out8"][:7]), zero7=float(zero["out8"][7]), coefs={})
            for c in COEFS:
                pen = p.pen(c, old_log_std=ols)
                ref_total, ref_diff = p.float64(pen["logits"], c, p.old_mean, ols)
                t_total, t_diff = p.float32(c, p.old_mean, ols)
                grad = _gradient_errors(p, twin, pen, ref_total, ref_diff, t_total, t_diff)
                lerr, lbound, _ = _loss_rounding(twin["out8"], pen["out8"], c)
                t8, p8 = ek._bits(twin["out8"]), ek._bits(pen["out8"])
                base = (3 + p.A) * p.hid + p.A
                rec["coefs"][c] = dict(same8=bool(np.array_equal(t8[[0, 1, 3, 4, 5, 6]], p8[[0, 1, 3, 4, 5, 6]])), out7=float(pen["out8"][7]),
                                       loss_err=lerr, loss_bound=lbound, grad=grad,
                                       same_rest=all(_eq(twin[k], pen[k]) for k in ("gm_v", "logits", "value")),
                                       same_stat_sums=ek._same(twin["sums"][base:base + 6], pen["sums"][base:base + 6])
                                       and ek._same(twin["sums"][-1], pen["sums"][-1]))
                print(f"[box {_bid(case)} {name} c={c}] {_grad_line(grad)}; loss {lerr:.2e} (bound {lbound:.2e})")
            out[case + (name,)] = rec
        del p, twin, zero, pen
    bound, worst = _bounds(out)
    for key in bound:
        print(f"[box] {key[0]} {key[1]}: bound 4 x {bound[key] / 4:.3e}, largest kernel error {worst[key]:.3e}")
    return out, bound


@pytest.mark.parametrize("log_stds", ["other log_std", "equal log_std"])
@pytest.mark.parametrize("case", BOX_CASES, ids=[_bid(c) for c in BOX_CASES])
def test_box_coefficient_zero_reproduces_the_twin(box_runs, case, log_stds):
    r = box_runs[0][case + (log_stds,)]
    assert all(r["zero"].values()), r["zero"]
    assert r["zero8"] and r["zero7"] == 0.0


@pytest.mark.parametrize("c", COEFS)
@pytest.mark.parametrize("log_stds", ["other log_std", "equal log_std"])
@pytest.mark.parametrize("case", BOX_CASES, ids=[_bid(c) for c in BOX_CASES])
def test_box_penalty_gradient_against_float64(box_runs, case, log_stds, c):
    r = box_runs[0][case + (log_stds,)]["coefs"][c]
    assert r["same8"] and r["out7"] == _c32(c)
    assert r["loss_err"] <= r["loss_bound"], (r["loss_err"], r["loss_bound"])
    assert r["same_rest"] and r["same_stat_sums"]
    _assert_gradients(r["grad"], box_runs[1], (case, log_stds, c))


@pytest.mark.parametrize("c", [0.2, 7.0])
@pytest.mark.parametrize("case", [(1, 64, 1), (9, 512, 8), (2059, 384, 8), (37, 64, 3)], ids=_bid)
def test_box_equal_policies_add_exactly_nothing(case, c):
    """Equal means and equal log-stds: q = 0 and expm1(0) = 0, so d logits and d log_std gain exactly 0."""
    p = _Box(*case)
    same = dict(old_mean=p.mu.clone(), old_log_std=p.log_std.clone())
    twin, pen = p.kl(**same), p.pen(c, **same)
    for k in ("gm_p", "gm_v", "sums", "logits", "value"):
        assert _eq(twin[k], pen[k]), k
    assert _eq(twin["out8"][:7], pen["out8"][:7]) and float(pen["out8"][7]) == _c32(c) and float(pen["out8"][4]) == 0.0


@pytest.mark.parametrize("case", [(8, 384, 3), (2059, 64, 1), (37, 512, 1), (9, 64, 8)], ids=_bid)
def test_box_means_shifted_by_a_constant_number_of_sigmas(box_runs, case):
    """old_mean = mean + 0.75 sigma, equal log-stds: every sample's d mean gains -c ent_scale 0.75 / sigma_a, so d bb gains
    -c 0.75 / sigma_a, and d log_std gains -c 0.75^2 -- its expm1 part is exactly 0.  Held to float64 on the rounded operands with the
    differences' bound, and to the closed form with the rounding of the shift added."""
    N, hid, A = case
    c, delta = 7.0, 0.75
    p = _Box(*case)
    sigma = p.log_std.exp()
    old_mean = (p.mu + delta * sigma).contiguous()
    ols = p.log_std.clone()
    twin, pen = p.kl(old_mean=old_mean, old_log_std=ols), p.pen(c, old_mean=old_mean, old_log_std=ols)
    ref_total, ref_diff = p.float64(pen["logits"], c, old_mean, ols)
    got = [a - b for a, b in zip(p.grads(pen), p.grads(twin))]
    for name, x, r in zip(QUANTITIES, got, ref_diff):
        assert _err(x, r) <= box_runs[1][(name, "diff")], (name, _err(x, r), box_runs[1][(name, "diff")])
    want_bb, want_ls = -_c32(c) * delta / sigma.double(), torch.full((A,), -_c32(c) * delta * delta, dtype=torch.float64, device=_dev())
    for name, x, want, r in (("d bb", got[2], want_bb, ref_diff[2]), ("d log_std", got[3], want_ls, ref_diff[3])):
        slack = float((r - want).abs().max())                          # (the shift as it was rounded into old_mean)
        print(f"[shift {_bid(case)}] {name}: kernel {x.tolist()} closed form {want.tolist()}")
        assert _err(x, want) <= box_runs[1][(name, "diff")] + slack, name


# ================================================================== 3. the separate-heads route
PPO_CASES = [(N, br, masked) for N in (1, 37, 2059) for br in ((12,), (63,), (5, 9), (31, 32)) for masked in (False, True)]


class _Ppo(ek._Ppo):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        _given_stats(self)

    def pen_branch(self, b, c, coef_ptr=None, expect=0):
        lib, dev, N = self.lib, _dev(), self.N
        off, a = _offsets(self.br)[b], self.br[b]
        lg = self.logits[:, off:off + a].contiguous()
        nbytes = lib.etm_ppo_loss_workspace_bytes(N)
        o = dict(out8=torch.full((8,), SENTINEL, device=dev), d_logits=torch.full((N, a), SENTINEL, device=dev),
                 d_value=torch.full((N,), SENTINEL, device=dev), ws=torch.full((nbytes // 4,), SENTINEL, device=dev))
        p = lambda t: t.data_ptr()
        word = _coef_word(c)
        rc = lib.etm_ppo_loss_kl_penalty(p(lg), p(self.actions) + 8 * b, self.B, p(self.old_logp) + 4 * b, self.B, p(self.adv), p(self.old_value),
                                         p(self.value), p(self.stats3), CLIP, VF, BETA, 1.0 / (N * self.B), 1.0 / N, 1.0 / N, 1 if b == 0 else 0,
                                         p(o["out8"]), p(o["d_logits"]), p(o["d_value"]), p(o["ws"]), nbytes, None, N, a,
                                         p(self.words) if self.masked else None, off if self.masked else 0, p(self.old_logps),
                                         self.old_logps.stride(0), off, p(word) if coef_ptr is None else coef_ptr,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, expect)
        torch.cuda.synchronize()
        return o

    def references(self, c):
        """d loss / d logits [N, A] over all branches: (float64 total, float64 penalty part, float32 torch total)."""
        from utils import categorical_kl_grad
        v = torch.as_tensor(self.valid, device=_dev())
        out = []
        for dt in (torch.float64, torch.float32):
            lg = self.logits.detach().to(dt).requires_grad_(True)
            L, K = _cat_terms(lg, self.br, v, self.actions, self.old_logp.to(dt), _normalised(self.adv, self.stats3, dt), self.old_logps)
            out.append(torch.autograd.grad(L if dt == torch.float64 else L + _c32(c) * K, lg)[0])
        G = torch.as_tensor(categorical_kl_grad(self.old_logps.cpu().numpy(), self.logits.cpu().numpy(), self.br,
                                                _pack(self.valid) if self.masked else None, np.float64), device=_dev())
        part = _c32(c) / (self.N * self.B) * G
        return out[0] + part, part, out[1]


def _pid(c):
    return f"N{c[0]}_{'x'.join(map(str, c[1]))}_{'masked' if c[2] else 'plain'}"


@pytest.fixture(scope="module")
def ppo_runs():
    out = {}
    for case in PPO_CASES:
        p = _Ppo(*case)
        twins = [p.branch(b, True) for b in range(p.B)]
        zeros = [p.pen_branch(b, 0.0) for b in range(p.B)]
        cat = lambda os_: torch.cat([o["d_logits"] for o in os_], dim=1)
        assert bool(torch.isfinite(cat(twins)).all()), case
        rec = dict(zero=all(_eq(t[k], z[k]) for t, z in zip(twins, zeros) for k in ("d_logits", "ws"))
                   and _eq(twins[0]["d_value"], zeros[0]["d_value"]) and all(_eq(t["out8"][:7], z["out8"][:7]) for t, z in zip(twins, zeros)),
                   zero7=[float(z["out8"][7]) for z in zeros], coefs={})
        invalid = torch.as_tensor(~p.valid, device=_dev())
        for c in COEFS:
            pens = [p.pen_branch(b, c) for b in range(p.B)]
            ref, part, t32 = p.references(c)
            s = _scale(ref)
            loss = [_loss_rounding(t["out8"], q["out8"], c) for t, q in zip(twins, pens)]
            rec["coefs"][c] = dict(
                k_total=_err(cat(pens), ref), k_diff=_err(cat(pens) - cat(twins), part), t_total=_err(t32, ref), scale=s,
                same8=all(np.array_equal(ek._bits(t["out8"])[[0, 1, 3, 4, 5, 6]], ek._bits(q["out8"])[[0, 1, 3, 4, 5, 6]]) for t, q in zip(twins, pens)),
                out7=[float(q["out8"][7]) for q in pens], loss_ok=all(e <= bnd for e, bnd, _ in loss), loss_err=max(e for e, _, _ in loss),
                same_rest=_eq(twins[0]["d_value"], pens[0]["d_value"]) and all(ek._same(t["ws"], q["ws"]) for t, q in zip(twins, pens)),
                invalid_zero=not bool(cat(pens)[invalid].any()))
            r = rec["coefs"][c]
            print(f"[ppo {_pid(case)} c={c}] d_logits total: torch fp32 {r['t_total']:.3e} kernel {r['k_total']:.3e}; difference: kernel "
                  f"{r['k_diff']:.3e} (relative to the largest element {s:.3e}: {r['t_total'] / s:.3e}, {r['k_total'] / s:.3e}, "
                  f"{r['k_diff'] / s:.3e}); loss {r['loss_err']:.2e}")
        out[case] = rec
    bound = 4.0 * max(r["coefs"][c]["t_total"] for r in out.values() for c in COEFS)
    print(f"[ppo] bound 4 x {bound / 4:.3e}; largest kernel error: totals {max(r['coefs'][c]['k_total'] for r in out.values() for c in COEFS):.3e}, "
          f"differences {max(r['coefs'][c]['k_diff'] for r in out.values() for c in COEFS):.3e}")
    return out, bound


@pytest.mark.parametrize("case", PPO_CASES, ids=[_pid(c) for c in PPO_CASES])
def test_ppo_route_against_float64(ppo_runs, case):
    """d_logits element-wise against float64 (the total, and the part the penalty adds); coefficient 0 equals the twin under ==.  The
    second branch of (31, 32) reads its columns at logps_off = 31 of rows with stride 63."""
    r = ppo_runs[0][case]
    assert r["zero"] and all(z == 0.0 for z in r["zero7"])
    for c in COEFS:
        q = r["coefs"][c]
        assert q["same8"] and all(x == _c32(c) for x in q["out7"]) and q["loss_ok"], (c, q)
        assert q["same_rest"], "d_value and the partial slots"
        assert q["invalid_zero"], "an invalid column's d logit is exactly 0"
        assert q["k_total"] <= ppo_runs[1] and q["k_diff"] <= ppo_runs[1], (c, q, ppo_runs[1])


def test_ppo_route_equal_policies_and_the_op_over_branches(ppo_runs):
    from etm import ops
    # equal policies (the sampler's rows of the same logits): K is exactly 0, so every statistic is the twin's; the gradient's term is
    # coef pol_scale (exp(l') - exp(l)) with l = fl(logit - fl(max + L)) the sampler's log-prob and l' = fl(fl(logit - max) - L) the
    # penalty's, L = log(sum): |l' - l| <= (sp(lse) + sp(logit - max)) / 2 + sp(l) (sp: a float32 spacing; the four roundings), each
    # expf within one spacing of p, and the sum with the twin's d logit rounds once more
    sp = lambda x: np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)
    for e in (_Ppo(2059, (31, 32), False), _Ppo(37, (5, 9), True), _Ppo(1, (63,), False)):
        e.old_logps = ek._sampler_rows(e.logits, e.br, e.words if e.masked else None)
        for b, (off, a) in enumerate(zip(_offsets(e.br), e.br)):
            t, q = e.branch(b, True), e.pen_branch(b, 7.0)
            assert _eq(t["out8"][:7], q["out8"][:7]) and float(q["out8"][7]) == 7.0 and float(q["out8"][4]) == 0.0
            v = e.valid[:, off:off + a]
            lg = np.where(v, e.logits[:, off:off + a].cpu().numpy().astype(np.float64), -np.inf)
            mx = lg.max(axis=1, keepdims=True)
            lse = mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True))
            with np.errstate(all="ignore"):
                l = np.where(v, lg - lse, 0.0)
                gap = 0.5 * (sp(lse) + sp(np.where(v, lg - mx, 0.0))) + sp(l)
            pj = np.where(v, np.exp(l), 0.0)
            base = t["d_logits"].cpu().numpy().astype(np.float64)
            bound = np.where(v, 7.0 / (e.N * e.B) * (pj * gap + 2 * sp(pj)) + sp(base), 0.0)
            diff = np.abs(q["d_logits"].cpu().numpy().astype(np.float64) - base)
            assert (diff <= bound).all(), (e.N, e.br, b, float((diff - bound).max()))
            assert not diff[~v].any(), "an invalid column's d logit is exactly the twin's 0"
    # the op: the branches' losses add up; None is the call of ever; the word is read in place
    p = _Ppo(37, (5, 9), True)
    word = _coef_word(0.2)
    lgs = lambda: [p.logits[:, :5].contiguous().requires_grad_(True), p.logits[:, 5:].contiguous().requires_grad_(True)]
    args = (p.value, p.actions, p.old_logp, p.adv, p.old_value, CLIP, VF, BETA)
    a = ops.ppo_loss(lgs(), *args, action_mask=p.words, old_logps=p.old_logps)
    la, lb = lgs(), lgs()
    b = ops.ppo_loss(lb, *args, action_mask=p.words, old_logps=p.old_logps, kl_coef=word)
    a2 = ops.ppo_loss(la, *args, action_mask=p.words, old_logps=p.old_logps, kl_coef=None)
    assert ek._same(a[0], a2[0]) and ek._same(a[1], a2[1])
    assert ek._same(a[1][[0, 1, 3, 4, 5]], b[1][[0, 1, 3, 4, 5]])
    want = float(a[0]) + _c32(0.2) * float(a[1][4])
    assert abs(float(b[0]) - want) <= 4 * float(np.spacing(np.float32(abs(want))))
    a2[0].backward()
    b[0].backward()
    ref, part, _ = p.references(0.2)
    got = torch.cat([t.grad for t in lb], dim=1) - torch.cat([t.grad for t in la], dim=1)
    assert _err(got, part) <= ppo_runs[1], (_err(got, part), ppo_runs[1])
    word.fill_(7.0)
    c = ops.ppo_loss(lgs(), *args, action_mask=p.words, old_logps=p.old_logps, kl_coef=word)
    assert float(c[0]) != float(b[0])
    with pytest.raises(ValueError, match=r"ppo_loss: kl_coef without old_logps"):
        ops.ppo_loss(lgs(), *args, action_mask=p.words, kl_coef=word)
    with pytest.raises(ValueError, match=r"kl_coef must be a device tensor of one float32"):
        ops.ppo_loss(lgs(), *args, old_logps=p.old_logps, action_mask=p.words, kl_coef=torch.zeros(2, device=_dev()))


# ================================================================== 4. refusals
def _untouched(o):
    return all(bool((t == (0x5A if t.dtype == torch.uint8 else SENTINEL)).all()) for t in o.values())


def test_a_null_or_misaligned_coefficient_is_refused_and_nothing_is_written():
    word = _coef_word(0.2)
    bad = (0, word.data_ptr() + 2, word.data_ptr() + 1)
    for prob in (_Fused(9, 64, (8,), False), _Fused(9, 64, (3, 3), True)):
        for ptr in bad:
            assert _untouched(prob.pen(0.2, coef_ptr=ptr, expect=EINVAL)), ptr
    box = _Box(9, 64, 3)
    for ptr in bad:
        assert _untouched(box.pen(0.2, coef_ptr=ptr, expect=EINVAL)), ptr
    ppo = _Ppo(37, (5, 9), True)
    for ptr in bad:
        assert _untouched(ppo.pen_branch(1, 0.2, coef_ptr=ptr, expect=EINVAL)), ptr
    # the twin's refusals stay: a misaligned table of old log-probs
    lib = ppo.lib
    assert hasattr(lib, "etm_heads_loss_kl_penalty") and hasattr(lib, "etm_heads_loss_branched_kl_penalty")


def test_the_ops_take_the_word_and_refuse_it_without_the_old_policy():
    from etm import ops
    dev = _dev()
    p = _Fused(9, 64, (3, 3), True)
    lin = lambda i, o_: torch.nn.Linear(i, o_).to(dev)
    h = torch.randn((9, 64), device=dev)
    mods = (lin(64, 64), lin(64, 64), [lin(64, 3), lin(64, 3)], lin(64, 1))
    args = (h, *mods, p.actions, p.old_logp, p.adv, p.old_value, CLIP, VF, BETA)
    word = _coef_word(0.2)
    with pytest.raises(ValueError, match=r"heads_ppo_loss: kl_coef without old_logps"):
        ops.heads_ppo_loss(*args, action_mask=p.words, kl_coef=word)
    with pytest.raises(ValueError, match=r"kl_coef must be a device tensor of one float32"):
        ops.heads_ppo_loss(*args, action_mask=p.words, old_logps=p.old_logps, kl_coef=word.double())
    loss_t, st_t = ops.heads_ppo_loss(*args, action_mask=p.words, old_logps=p.old_logps)
    loss_n, st_n = ops.heads_ppo_loss(*args, action_mask=p.words, old_logps=p.old_logps, kl_coef=None)
    assert ek._same(loss_t, loss_n) and ek._same(st_t, st_n)
    loss, st = ops.heads_ppo_loss(*args, action_mask=p.words, old_logps=p.old_logps, kl_coef=word)
    assert st.shape == (6,) and ek._same(st[[0, 1, 3, 4, 5]], st_t[[0, 1, 3, 4, 5]])
    err, bound, _ = _loss_rounding(st_t, st, 0.2)
    assert err <= bound and float(loss) == float(st[2])
    # unit_grad / loss.backward(): the branch heads' gradients carry the penalty
    for m in mods[2]:
        m.zero_grad()
    loss.backward()
    g_pen = [m.bias.grad.clone() for m in mods[2]]
    for m in mods[2]:
        m.zero_grad()
    loss_t.backward()
    assert any(not _eq(a, m.bias.grad) for a, m in zip(g_pen, mods[2]))
    box = _Box(9, 64, 3)
    bargs = (h, lin(64, 64), lin(64, 64), lin(64, 3), box.log_std, lin(64, 1), box.xact, box.old_logp, box.adv, box.old_value, CLIP, VF, BETA)
    with pytest.raises(ValueError, match=r"heads_ppo_loss_gaussian: kl_coef without old_mean"):
        ops.heads_ppo_loss_gaussian(*bargs, kl_coef=word)
    lt, stt = ops.heads_ppo_loss_gaussian(*bargs, old_mean=box.old_mean, old_log_std=box.old_log_std)
    lp, stp = ops.heads_ppo_loss_gaussian(*bargs, old_mean=box.old_mean, old_log_std=box.old_log_std, kl_coef=word)
    assert ek._same(stt[[0, 1, 3, 4, 5]], stp[[0, 1, 3, 4, 5]])
    err, bound, _ = _loss_rounding(stt, stp, 0.2)
    assert err <= bound


# ================================================================== 5. the trainer
FORMS, SCHED = ek.FORMS, ek.SCHED
SEED, UPDATES, EPOCHS, N_MB = ek.SEED, ek.UPDATES, ek.EPOCHS, ek.N_MB
POLICIES = {k: ek.POLICIES[k] for k in ("discrete", "masked multidiscrete")}
TRAINER_CASES = [(p, f) for p in POLICIES for f in FORMS]
_CACHE = {}


def _config(policy, form, **over):
    return ek._config(policy, form, **over)


def _values_equal(a, b):
    """``==`` on two recordings (rh.state): the keys that differ in a value."""
    assert a.keys() == b.keys()
    return [k for k in a if a[k].shape != b[k].shape or np.isnan(a[k]).any() or not np.array_equal(a[k], b[k])]


def _run(policy, form, key, updates=UPDATES, box=False):
    name = (policy, form, repr(sorted(key.items())), updates, box)
    if name not in _CACHE:
        tr = None
        try:
            tr = rh.trainer(_box_config(form, **key) if box else _config(policy, form, **key), seed=SEED, run_id="klp_run")
            rows, pens, words = [], [], []
            for _ in range(updates):
                rows.append(ek._update(tr)[0])
                pens.append(None if tr.last_kl_penalty is None else dict(tr.last_kl_penalty))
                words.append(None if tr._kl_coef is None else float(tr._kl_coef.item()))
            assert (tr._train_graph is not None) == (form != "eager")
            _CACHE[name] = dict(rows=rows, state=rh.state(tr), pens=pens, words=words, exact=(tr._kl_exact_cat, tr._kl_analytic))
        finally:
            rh.release(tr)
    return _CACHE[name]


def _box_config(form="captured, tables", **over):
    env = dict(type="Synthetic", obs_shape=[rh.F_OBS], continuous_actions=2, max_episode_steps=16, seed=2, p_done=0.1, pool=4)
    return rh.config(**{"environment": env, "learning_rate_schedule": dict(SCHED), "n_mini_batch": N_MB, "epochs": EPOCHS, **FORMS[form], **over})


@pytest.mark.parametrize("policy,form", TRAINER_CASES)
def test_coefficient_zero_is_the_exact_kl_trainer(policy, form):
    """(a) ``kl_penalty: 0`` and no other KL key: two updates equal an ``exact_kl: true`` trainer's under ==."""
    a, b = _run(policy, form, {"exact_kl": True}), _run(policy, form, {"kl_penalty": 0})
    assert b["exact"] == (True, False) and a["exact"] == (True, False)
    assert _values_equal(a["state"], b["state"]) == [] and int(b["state"]["step"]) == UPDATES * EPOCHS * N_MB
    for u in range(UPDATES):
        assert a["rows"][u].shape == (EPOCHS * N_MB, 6) and np.array_equal(a["rows"][u], b["rows"][u]), u
        assert b["pens"][u]["coef"] == 0.0 and b["pens"][u]["next_coef"] == 0.0 and b["pens"][u]["moved"] == 0 and b["words"][u] == 0.0
        assert np.float32(b["pens"][u]["kl"]) == np.float32(b["rows"][u][:, 4].astype(np.float64).mean())
    assert a["pens"] == [None] * UPDATES and a["words"] == [None] * UPDATES


def _full_loss(logits_list, value, mb, br, valid, clip, vf_coef, beta, coef, dt, rule_gradient):
    """L_ppo + coef K of one minibatch in ``dt`` from the model outputs (the trainer's normalisation: mean and unbiased std of the
    minibatch's advantages).  ``rule_gradient``: K enters through utils.categorical_kl_grad's expression (p - p_old on the valid
    columns, held constant) times the logits, whose gradient is the rule's exactly; else as sum p_old (log p_old - log p)."""
    logits = torch.cat(logits_list, dim=1)
    N, B = logits.shape[0], len(br)
    adv = mb["advantages"].to(dt)
    a_n = (adv - adv.mean()) / (adv.std() + 1e-8)
    actions = mb["actions"].reshape(N, B)
    pol = ent = kl = 0.0
    zero = torch.zeros((), dtype=dt, device=logits.device)
    for b, (off, a) in enumerate(zip(_offsets(br), br)):
        v = valid[:, off:off + a]
        lsm = torch.log_softmax(logits[:, off:off + a].masked_fill(~v, float("-inf")), dim=-1)
        lp = lsm.gather(1, actions[:, b:b + 1])[:, 0]
        ratio = torch.exp(lp - mb["log_probs"].reshape(N, B)[:, b].to(dt))
        pol = pol + torch.min(ratio * a_n, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_n).sum()
        ent = ent - (lsm.exp() * lsm.masked_fill(~v, 0.0)).sum()
        old = mb["old_logps"][:, off:off + a].to(dt)
        if rule_gradient:
            kl = kl + (torch.where(v, lsm.exp() - old.exp(), zero).detach() * logits[:, off:off + a]).sum()
        else:
            use = v & (old > float("-inf"))
            kl = kl + torch.where(use, old.exp() * (torch.where(use, old, zero) - torch.where(use, lsm, zero)), zero).sum()
    vo = mb["values"].to(dt)
    ret = vo + adv
    vc = vo + (value - vo).clamp(min=-clip, max=clip)
    val = torch.max((value - ret) ** 2, (vc - ret) ** 2).mean()
    return -(pol / (N * B) - vf_coef * val + beta * ent / N) + coef * kl / (N * B)


def _box_full_loss(mean, value, log_std, mb, old_log_std, clip, vf_coef, beta, coef, dt, rule_gradient):
    N, A = mean.shape
    adv = mb["advantages"].to(dt)
    a_n = (adv - adv.mean()) / (adv.std() + 1e-8)
    sigma = log_std.exp()
    z = (mb["actions"].reshape(N, A).to(dt) - mean) / sigma
    lp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(1)
    ratio = torch.exp(lp - mb["log_probs"].reshape(N).to(dt))
    pol = torch.min(ratio * a_n, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_n).mean()
    ent = (0.5 + HALF_LOG_2PI + log_std).sum()
    d = old_log_std.to(dt) - log_std
    q = (mb["means"].reshape(N, A).to(dt) - mean) / sigma
    if rule_gradient:
        kl = ((-q / sigma).detach() * mean).sum() / N + ((-torch.expm1(2.0 * d)[None, :] - q * q).sum(0).detach() * log_std).sum() / N
    else:
        kl = (0.5 * torch.expm1(2.0 * d) - d).sum() + (0.5 * q * q).sum(1).mean()
    vo = mb["values"].to(dt)
    ret = vo + adv
    vc = vo + (value - vo).clamp(min=-clip, max=clip)
    val = torch.max((value - ret) ** 2, (vc - ret) ** 2).mean()
    return -(pol - vf_coef * val + beta * ent) + coef * kl


def _first_step_gradients(cfg, box):
    """One update of a ``kl_penalty: 0.2`` trainer with the gradient arena of its FIRST optimisation step caught in front of the
    optimiser (tests/test_action_masks_gpu.py: the whole-trainer test), recomputed through the float64 oracle model and through the same
    model in float32 -> (device gradients, float64, float32 torch, names, the update's statistic rows, coef)."""
    from oracle import ref_model as rm
    tr = rh.trainer(cfg, seed=SEED, run_id="klp_arena")
    try:
        coef = float(tr._kl_coef.item())
        before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        names = [n for n, p in tr.model.arena_parameters()]
        state = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()
        first, step0 = {}, tr.optimizer.step

        def spy(*a, **k):
            if not first and not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
                first["g"] = [p.grad.detach().clone() for p in tr.params]
            return step0(*a, **k)

        tr.optimizer.step = spy
        lr, beta, clip = tr.schedules(0)
        perms = ek._perms(0)
        rows, _ = tr._train_epochs(lr, clip, beta, perms=perms)
        torch.cuda.synchronize()
        rows = np.stack(rows)
        b, sf = tr.buffer, tr.buffer.samples_flat
        mbs = b.batch_size // N_MB
        idx = torch.as_tensor(perms[0][:mbs], device=tr.device, dtype=torch.long).sort().values
        mb = {k: sf[k].index_select(0, idx) for k in ("actions", "log_probs", "advantages", "values") + (("means",) if box else ("old_logps",))}
        br = tr.action_space_shape
        A = sum(br)
        if box:
            valid = None
        elif "action_masks" in sf:
            valid = torch.as_tensor(ek._valid(sf["action_masks"].index_select(0, idx).cpu().numpy(), A), device=tr.device)
        else:
            valid = torch.ones((mbs, A), dtype=torch.bool, device=tr.device)
        ep, ind = sf["memory_index"].index_select(0, idx), sf["memory_indices"].index_select(0, idx)
        pos = tr.model.transformer._pos()
        ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
        refs = []
        for dt, rule in ((torch.float64, True), (torch.float32, False)):
            sd = {k: v.to(dt).requires_grad_(k in names) for k, v in before.items()}
            for k, v in state.items():
                sd.setdefault(k, v.to(dt) if v.is_floating_point() else v)
            win = b.memories[ep[:, None], ind].to(dt)
            if pos is not None:
                win = win + pos.to(dt)[ind].unsqueeze(2)
            logits, value, _ = rm.actor_critic(sd, ocfg, sf["obs"].index_select(0, idx).to(dt), win, sf["memory_mask"].index_select(0, idx), ind,
                                               tr.max_episode_length)
            if box:
                loss = _box_full_loss(logits[0], value, sd["policy_log_std"].reshape(-1), mb, b.old_log_std, clip, cfg["value_loss_coefficient"],
                                      beta, coef, dt, rule)
            else:
                loss = _full_loss(logits, value, mb, br, valid, clip, cfg["value_loss_coefficient"], beta, coef, dt, rule)
            refs.append(torch.autograd.grad(loss, [sd[n] for n in names]))
        return first["g"], refs[0], refs[1], names, rows, coef
    finally:
        rh.release(tr)


def _check_first_step(got, ref64, ref32, names, rows, coef, beta, vf_coef, what):
    """The arena against float64 with the bound formed as for the loss routes: the largest |x - ref| over the arena's elements, against
    4 x that of the float32 torch evaluation (the largest per-tensor figures relative to the tensor's largest element are printed
    too).  Column 2 = columns 0, 1, 3, 4 combined."""
    k_abs, t_abs = max(_err(g, r) for g, r in zip(got, ref64)), max(_err(g, r) for g, r in zip(ref32, ref64))
    k_rel = {n: _rel(g, r, _scale(r)) for n, g, r in zip(names, got, ref64)}
    t_rel = {n: _rel(g, r, _scale(r)) for n, g, r in zip(names, ref32, ref64)}
    worst = max(k_rel, key=k_rel.get)
    print(f"[{what}] first-step arena: largest float32 torch error {t_abs:.3e}, largest kernel error {k_abs:.3e}, bound {4.0 * t_abs:.3e}; "
          f"per tensor, relative to its largest element: torch {max(t_rel.values()):.3e}, kernel {k_rel[worst]:.3e} ({worst})")
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert k_abs <= 4.0 * t_abs, (k_abs, t_abs)
    for row in rows:
        pol, val, loss, ent, kl = (float(row[i]) for i in range(5))
        terms = (pol, vf_coef * val, beta * ent, _c32(coef) * kl)
        want = -(pol - vf_coef * val + beta * ent) + _c32(coef) * kl
        # four float32 operations on values no larger than twice the largest term: half a spacing each
        bound_l = 4 * 0.5 * float(np.spacing(np.float32(2 * max(abs(t) for t in terms + (want,)))))
        assert abs(loss - want) <= bound_l, (loss, want, bound_l)
    assert float(rows[-1][4]) > 0, "the policy moved within the update"


@pytest.mark.parametrize("policy,form", TRAINER_CASES)
def test_first_step_arena_against_float64(policy, form):
    """(b) ``kl_penalty: 0.2``: the gradient arena of the first optimisation step against a float64 recomputation of L_ppo + coef K."""
    cfg = _config(policy, form, kl_penalty=0.2, normalize_observations=False, normalize_rewards=False)
    got, r64, r32, names, rows, coef = _first_step_gradients(cfg, False)
    assert coef == _c32(0.2)
    _check_first_step(got, r64, r32, names, rows, coef, cfg["beta_schedule"]["initial"], cfg["value_loss_coefficient"], f"{policy} / {form}")


def _target_from_key_off(policy):
    """How ``target`` is chosen: m0 = float32(mean of the column-4 rows of the FIRST update of the key-off (``exact_kl: true``) trainer),
    the number the rule would have seen there.  The band sits just under it: high 0.9, low 0.8 (as float32 of the products), so an
    update whose KL is about m0 raises.  The factors are large on purpose (up 50, down 0.02): after a raise the penalty (coef 10) holds
    the next update's KL far below the band, which cuts.  The three updates must show a raise and a cut; every decision is checked
    against utils.kl_penalty_step on the run's own rows, whichever way it went."""
    m0 = float(np.float32(_run(policy, "captured, tables", {"exact_kl": True})["rows"][0][:, 4].astype(np.float64).mean()))
    assert m0 > 0
    return {"coef": 0.2, "target": m0, "high": 0.9, "low": 0.8, "up": 50.0, "down": 0.02, "min": 1.0e-4, "max": 100.0}


@pytest.mark.parametrize("policy,form", TRAINER_CASES)
def test_adaptive_coefficient_follows_the_host_rule(policy, form):
    """(c) ``last_kl_penalty`` and the coefficient word after each of three updates equal utils.kl_penalty_step walked over the returned
    column-4 rows."""
    from utils import kl_penalty_section, kl_penalty_step
    key = _target_from_key_off(policy)
    rule = kl_penalty_section({"kl_penalty": key})
    run = _run(policy, form, {"kl_penalty": key}, updates=3)
    coef, moves = np.float32(rule["coef"]), []
    for u in range(3):
        kl = np.float32(run["rows"][u][:, 4].astype(np.float64).mean())
        nxt, moved = kl_penalty_step(coef, kl, rule)
        print(f"{policy} / {form}: update {u} kl rows {run['rows'][u][:, 4].tolist()} mean {float(kl)!r} band [{rule['kl_low']!r}, {rule['kl_high']!r}] "
              f"coef {float(coef)!r} -> {float(nxt)!r} ({moved:+d})")
        assert run["pens"][u] == {"coef": float(coef), "next_coef": float(np.float32(nxt)), "kl": float(kl), "moved": int(moved)}, u
        assert ek._bits32(run["words"][u]) == ek._bits32(nxt), u
        coef = np.float32(nxt)
        moves.append(moved)
    assert 1 in moves and -1 in moves, moves


def test_checkpoint_carries_the_coefficient(tmp_path, monkeypatch):
    """(d) A checkpoint saved after a moved coefficient resumes bit for bit, in place and through ``resume=``, coefficient included; a
    key-absent checkpoint has no entry and a resume with the key starts at ``coef``."""
    import checkpoint as ck
    monkeypatch.chdir(tmp_path)
    policy = "masked multidiscrete"
    key = _target_from_key_off(policy)
    cfg = _config(policy, "captured, tables", kl_penalty=key)
    tr = fresh = plain = late = None
    try:
        tr = rh.trainer(cfg, seed=SEED, run_id="klp_ckpt")
        ek._update(tr)
        assert tr.last_kl_penalty["moved"] != 0 and tr.last_kl_penalty["next_coef"] != tr.last_kl_penalty["coef"]
        moved_to = float(tr._kl_coef.item())
        path = tr.save_checkpoint()
        saved = ck.read_checkpoint(path)
        assert saved["format"] == 1 and isinstance(saved["kl_coef"], np.float32) and float(saved["kl_coef"]) == moved_to
        tr.restart_episodes(1)
        rec_a, pen_a, word_a = rh.update(tr), dict(tr.last_kl_penalty), float(tr._kl_coef.item())
        assert pen_a["coef"] == moved_to
        tr._kl_coef.fill_(0.5)                          # (the load puts the stored word back)
        tr.load_checkpoint(path)
        assert float(tr._kl_coef.item()) == moved_to and tr.last_kl_penalty is None
        rec_b = rh.update(tr)
        assert rh.differing(rec_a, rec_b) == [] and tr.last_kl_penalty == pen_a and ek._bits32(tr._kl_coef.item()) == ek._bits32(word_a)
        fresh = rh.trainer(cfg, seed=999, run_id="klp_fresh", resume=path)
        assert fresh.update_index == 1 and float(fresh._kl_coef.item()) == moved_to
        rec_c = rh.update(fresh)
        assert rh.differing(rec_a, rec_c) == [] and fresh.last_kl_penalty == pen_a and ek._bits32(fresh._kl_coef.item()) == ek._bits32(word_a)
        # a key-absent checkpoint: no entry; resumed with the key it starts at coef
        plain = rh.trainer(_config(policy, "captured, tables"), seed=SEED, run_id="klp_plain")
        ek._update(plain)
        path2 = plain.save_checkpoint()
        assert "kl_coef" not in ck.read_checkpoint(path2)
        late = rh.trainer(cfg, seed=SEED, run_id="klp_late", resume=path2)
        assert float(late._kl_coef.item()) == _c32(0.2)
    finally:
        rh.release(tr, fresh, plain, late)


def test_box_policy_under_the_key():
    """(e) ``kl_penalty`` on a Box config, the captured form with tables: coefficient 0 equals ``exact_kl: true`` under ==, and the first
    step's arena at 0.2 against float64 (``policy_log_std`` among the tensors)."""
    a, b = _run("box", "captured, tables", {"exact_kl": True}, box=True), _run("box", "captured, tables", {"kl_penalty": 0}, box=True)
    assert a["exact"] == (False, True) and b["exact"] == (False, True)
    assert _values_equal(a["state"], b["state"]) == []
    for u in range(UPDATES):
        assert np.array_equal(a["rows"][u], b["rows"][u]) and b["pens"][u]["coef"] == 0.0
    cfg = _box_config(kl_penalty=0.2, normalize_observations=False, normalize_rewards=False)
    got, r64, r32, names, rows, coef = _first_step_gradients(cfg, True)
    assert "policy_log_std" in names
    _check_first_step(got, r64, r32, names, rows, coef, cfg["beta_schedule"]["initial"], cfg["value_loss_coefficient"], "box / captured, tables")


def test_refusals_raise_at_construction():
    """(f)"""
    from trainer import PPOTrainer

    def build(cfg, **kw):
        return PPOTrainer(cfg, run_id="klp_refused", device=rh.dev(), tensorboard=False, **kw)

    cfg = lambda **over: _config("discrete", "captured, tables", **over)
    with pytest.raises(ValueError, match=r"kl_penalty.coef must be a finite number >= 0"):
        build(cfg(kl_penalty=-1.0))
    with pytest.raises(ValueError, match=r"coef 0 with `target`"):
        build(cfg(kl_penalty={"coef": 0, "target": 0.01}))
    with pytest.raises(ValueError, match=r"kl_penalty: unknown keys \['goal'\]"):
        build(cfg(kl_penalty={"coef": 0.2, "goal": 0.01}))
    with pytest.raises(ValueError, match=r"need `target`"):
        build(cfg(kl_penalty={"coef": 0.2, "up": 2.0}))
    with pytest.raises(ValueError, match=r"kl_penalty next to exact_kl: false"):
        build(cfg(kl_penalty=0.2, exact_kl=False))
    with pytest.raises(ValueError, match=r"kl_penalty next to kl_estimator: k3"):
        build(cfg(kl_penalty=0.2, kl_estimator="k3"))
    dp = type("DP", (), {"world": 2, "rank": 0})()
    with pytest.raises(ValueError, match=r"kl_penalty in a data-parallel run.*remove the key, or train on one device"):
        build(cfg(kl_penalty=0.2, normalize_observations=False, normalize_rewards=False), dp=dp)


def test_the_other_kl_rules_see_the_same_column_next_to_the_key():
    """``target_kl`` and ``adaptive_lr`` next to the key construct and run; the key's record is filled from the rows the phase returns."""
    tr = None
    try:
        tr = rh.trainer(_config("discrete", "captured, tables", kl_penalty={"coef": 0.2, "target": 0.01}, target_kl=1.0e-4), seed=SEED,
                        run_id="klp_with_stop")
        rows, _ = ek._update(tr)
        stop, pen = tr.last_kl_stop, tr.last_kl_penalty
        assert rows.shape[0] == (stop["steps_applied"] + 1 if stop["stopped"] else EPOCHS * N_MB)
        assert np.float32(pen["kl"]) == np.float32(rows[:, 4].astype(np.float64).mean()) and ek._bits32(stop["kl"]) == ek._bits32(rows[-1, 4])
    finally:
        rh.release(tr)
