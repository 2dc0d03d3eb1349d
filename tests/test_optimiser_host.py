"""CPU: tests/optimiser_reference.py against torch -- ``step64`` is ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False,
fused=False)`` on float64 parameters to 1e-12 (finite and non-finite gradients), ``group_norms64`` is upstream's concatenated norm,
and the distance of ``step32`` from ``step64`` on the inputs of tests/test_optimiser_vs_float64.py is measured, printed and bounded:
that figure (E_ref) is the reference's own float32 error, which the GPU test's parameter tolerance is built from."""
import numpy as np
import pytest
import torch

import optimiser_reference as orf

REL = 1e-12
SHAPES = [(3, 5), (7,), (1,), (2, 2, 3)]
N = sum(int(np.prod(s)) for s in SHAPES)
E_REF_BOUND = 16 * 2.0 ** -24


def _torch_run(p0, grads, lrs, max_norms, hyper, grad_scale):
    """clip_grad_norm_ (where max_norm > 0) + AdamW on float64 tensors -> per step dict(p, g after clipping, m, v, total), flat float64."""
    splits = np.cumsum([int(np.prod(s)) for s in SHAPES])[:-1]
    params = [torch.nn.Parameter(torch.from_numpy(a.reshape(s).astype(np.float64))) for a, s in zip(np.split(p0, splits), SHAPES)]
    opt = torch.optim.AdamW(params, lr=1.0, betas=hyper["betas"], eps=hyper["eps"], weight_decay=hyper["weight_decay"], foreach=False, fused=False)
    flat = lambda ts: np.concatenate([t.detach().numpy().reshape(-1) for t in ts])
    out = []
    for g, lr, max_norm in zip(grads, lrs, max_norms):
        scaled = g.astype(np.float64) * orf.f32(grad_scale)               # data parallel: torch sees the averaged gradient
        for q, a, s in zip(params, np.split(scaled, splits), SHAPES):
            q.grad = torch.from_numpy(a.reshape(s).copy())
        total = float("nan")
        if max_norm > 0.0:
            total = float(torch.nn.utils.clip_grad_norm_(params, max_norm=orf.f32(max_norm)))
        for group in opt.param_groups:
            group["lr"] = orf.f32(lr)
        opt.step()
        out.append(dict(p=flat(params), g=flat([q.grad for q in params]), m=flat([opt.state[q]["exp_avg"] for q in params]),
                        v=flat([opt.state[q]["exp_avg_sq"] for q in params]), total=total))
    return out


def _reference_run(p0, grads, lrs, max_norms, hyper, grad_scale):
    p, m, v = p0.astype(np.float64), np.zeros(N), np.zeros(N)
    out = []
    for i, g in enumerate(grads):
        out.append(orf.step64(p, g, m, v, i + 1, lrs[i], hyper["betas"], hyper["eps"], hyper["weight_decay"], max_norms[i], grad_scale))
        p, m, v = out[-1]["p"], out[-1]["m"], out[-1]["v"]
    return out


def _close(got, want, what):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    with np.errstate(invalid="ignore"):
        bad = ~((np.abs(got[ok] - want[ok]) <= REL * np.abs(want[ok])) | (got[ok] == want[ok]))
    assert not bad.any(), (what, got[ok][bad][:4], want[ok][bad][:4])


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 3.0], ids=["scale1", "scale1/3"])
@pytest.mark.parametrize("hyper", orf.HYPERS, ids=lambda h: "wd{weight_decay}-b{betas[0]}-eps{eps}".format(**h))
def test_step64_is_clip_grad_norm_and_torch_adamw_in_float64(hyper, grad_scale):
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(N).astype(np.float32)
    steps = 6
    grads = [(rng.standard_normal(N) * (10.0 if i % 2 == 0 else 0.01) / grad_scale).astype(np.float32) for i in range(steps)]
    lrs = [3e-4 * (1 - 0.1 * i) for i in range(steps)]
    for max_norms in ([0.5] * steps, [0.0] * steps):                      # with the clip call (steps 0, 2, 4 clip) and without it
        want = _torch_run(p0, grads, lrs, max_norms, hyper, grad_scale)
        got = _reference_run(p0, grads, lrs, max_norms, hyper, grad_scale)
        for i in range(steps):
            if max_norms[i] > 0:
                assert (got[i]["coef"] < orf.f32(grad_scale)) == (i % 2 == 0), "steps 0, 2, 4 must clip and the others not"
                _close(got[i]["total"], want[i]["total"], f"total norm, step {i}")
            else:
                assert got[i]["coef"] == orf.f32(grad_scale)
            for k in ("p", "g", "m", "v"):
                _close(got[i][k], want[i][k], f"{k}, step {i}")


@pytest.mark.parametrize("where", [0, N // 2, N - 1])
def test_step64_hands_a_non_finite_norm_on_as_clip_grad_norm_does(where):
    """One finite step (so that the moments are not zero), then a gradient with one NaN -- everything NaN -- or one +inf -- NaN at that
    element; elsewhere the clipped gradient is 0 and decay and the old momentum alone move the parameter.  Without the clip call
    (max_norm 0) a NaN stays in its element."""
    rng = np.random.default_rng(9)
    hyper = orf.DEFAULT
    p0 = rng.standard_normal(N).astype(np.float32)
    g0 = rng.standard_normal(N).astype(np.float32)
    for bad in (np.nan, np.inf):
        g1 = rng.standard_normal(N).astype(np.float32)
        g1[where] = bad
        for max_norm in (0.5, 0.0):
            args = (p0, [g0, g1], [3e-4, 3e-4], [max_norm, max_norm], hyper, 1.0)
            want, got = _torch_run(*args)[1], _reference_run(*args)[1]
            for k in ("p", "g", "m", "v"):
                _close(got[k], want[k], f"{k}, {bad}, max_norm {max_norm}")
            others = np.arange(N) != where
            if max_norm > 0 and np.isnan(bad):
                assert np.isnan(got["total"]) and np.isnan(want["total"])
                assert all(np.isnan(got[k]).all() for k in ("p", "g", "m", "v"))
            elif max_norm > 0:
                assert got["total"] == np.inf and want["total"] == np.inf
                assert all(np.isnan(got[k][where]) for k in ("p", "g", "m", "v"))
                assert np.all(got["g"][others] == 0.0) and np.isfinite(got["p"][others]).all()
                first = _reference_run(*args)[0]
                keep = 1.0 - orf.f32(3e-4) * hyper["weight_decay"]
                m2 = hyper["betas"][0] * first["m"]
                v2 = hyper["betas"][1] * first["v"]
                moved = first["p"] * keep - orf.f32(3e-4) / (1 - hyper["betas"][0] ** 2) * m2 / (np.sqrt(v2) / np.sqrt(1 - hyper["betas"][1] ** 2) + hyper["eps"])
                _close(got["p"][others], moved[others], "decay and the old momentum alone")
            else:
                assert np.isnan(got["p"][where]) and not any(np.isfinite(got[k][where]) for k in ("g", "m", "v"))   # (+inf: m = v = +inf)
                assert all(np.isfinite(got[k][others]).all() for k in ("p", "g", "m", "v"))


def test_group_norms64_is_the_norm_of_the_concatenated_gradients():
    """Upstream concatenates the gradients of a group's modules (a parameter listed twice counts twice) and takes one norm."""
    rng = np.random.default_rng(3)
    flat = rng.standard_normal(40).astype(np.float32)
    start, length = np.array([1, 9, 20, 33]), np.array([5, 7, 9, 4])
    member = np.array([[1, 0, 2, 0], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=np.float32)
    got, q = orf.group_norms64(flat, start, length, member)
    t = torch.from_numpy(flat.astype(np.float64))
    pieces = [t[a: a + n] for a, n in zip(start.tolist(), length.tolist())]
    for g in range(3):
        listed = [pieces[s] for s in range(4) for _ in range(int(member[g, s]))]
        want = float(torch.linalg.norm(torch.cat(listed))) if listed else 0.0
        assert abs(got[g] - want) <= REL * want
    assert got[1] == 0.0 and np.allclose(q, [float(x.square().sum()) for x in pieces], rtol=REL, atol=0)


def test_step32_stays_within_the_recorded_ratio_of_step64_on_the_gpu_tests_inputs():
    """E_ref: the largest |step32.p - step64.p| / (|p| + |update|) over every one-step case of tests/test_optimiser_vs_float64.py.  The
    reference alone, on the CPU.  Also: with integer gradients step32's norm is the exact one."""
    worst, at = 0.0, None
    for case in orf.element_cases():
        a, r32, r64 = orf.reference_pair(case)
        s = orf.exact_sumsq(a["g"])
        assert s < 2 ** 24 and float(r32["total"]) == float(np.sqrt(np.float32(s)) * np.float32(case["grad_scale"]))
        ratio = orf.parameter_ratio(a["p"], r32["p"], r64)
        if ratio > worst:
            worst, at = ratio, {k: v for k, v in case.items() if k != "seed"}
    print(f"\nE_ref = {worst:.6e} = {worst * 2 ** 24:.3f} * 2^-24 at {at}")
    assert 0.0 < worst < E_REF_BOUND, (worst, at)
    assert worst <= orf.E_REF, "tests/optimiser_reference.py: E_REF must record (not undercut) the measured ratio"
