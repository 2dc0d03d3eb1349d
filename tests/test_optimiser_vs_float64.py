"""-m gpu: the optimiser step (etm_grad_sqnorm + etm_adamw_clip) and the monitored gradient norms (etm_group_norms) of csrc/optim.hip
through the C ABI against tests/optimiser_reference.py -- plain numpy: ``step64`` (float64, checked against torch on the CPU by
tests/test_optimiser_host.py), ``step32`` (the same formulas in float32, each operation rounded once) and ``group_norms64``.

* Norm: integer gradients make every square and partial sum an integer below 2^24, so the sum of the ``partial`` buffer is asserted
  exactly (prefilled with NaN: a workgroup that writes nothing shows) and ``norm_out`` bit for bit, at n in {4 .. 40004} x n_partial in
  {1 .. 4096} and past the 2048-workgroup cap of the AdamW launch.
* Elements: the clip coefficient follows exactly from the integer sum, so g, m and v are asserted bit for bit against ``step32``.  p is
  asserted against ``step64`` to (4 E_ref + 2^-23) (|p| + |update|): E_ref = 2.946490e-07 = 4.943 * 2^-24 is ``step32``'s own distance
  from ``step64`` on these inputs, measured on the CPU by tests/test_optimiser_host.py (optimiser_reference.E_REF records 2.95e-7); the
  factor 4 and the added unit in the last place cover the two double ``pow`` results, whose last bit may differ between the device's
  and the host's maths library.
* Identities (lr 0, zero gradient, grad_scale = 1 / w on w g), five consecutive steps, non-finite gradients (the rule of
  ``clip_grad_norm_``: a NaN norm gives a NaN coefficient), and the monitored norms: the kernel pair on crafted segments, exactly, and
  ``_grad_group_norms`` of two small trainers against the definition over ``model._grad_groups()``.
"""
import math

import numpy as np
import pytest
import torch

import optimiser_reference as orf
import resume_helpers as rh

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
P_TOL = 4 * orf.E_REF + 2.0 ** -23                  # relative to |p| + |update|


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _run(a, n_partial, step, lr, hyper, max_norm, grad_scale, gate_kl=None):
    """The two launches on the arena ``a`` (numpy; copied) -> dict of numpy results.  ``gate_kl``: the gated twins, gate clear, with
    this kl under a limit of 1."""
    from etm import lib
    h = lib.load()
    dev = rh.dev()
    st = torch.cuda.current_stream(dev).cuda_stream
    t = {k: torch.from_numpy(np.ascontiguousarray(a[k], dtype=np.float32)).to(dev) for k in ("p", "g", "m", "v")}
    n = t["p"].numel()
    partial = torch.full((n_partial,), float("nan"), device=dev)
    stepd = torch.tensor(int(step), dtype=torch.int64, device=dev)
    lrd = torch.tensor(float(lr), dtype=torch.float32, device=dev)
    norm = torch.full((), float("nan"), device=dev)
    tail = (lrd.data_ptr(), stepd.data_ptr(), float(hyper["betas"][0]), float(hyper["betas"][1]), float(hyper["eps"]), float(hyper["weight_decay"]),
            float(max_norm), float(grad_scale), norm.data_ptr())
    if gate_kl is None:
        lib.check(h.etm_grad_sqnorm(t["g"].data_ptr(), n, partial.data_ptr(), n_partial, stepd.data_ptr(), st), "etm_grad_sqnorm")
        lib.check(h.etm_adamw_clip(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), n, partial.data_ptr(), n_partial,
                                   *tail, st), "etm_adamw_clip")
    else:
        kl = torch.tensor([gate_kl], dtype=torch.float32, device=dev)
        words = torch.zeros(3, dtype=torch.int64, device=dev)
        lib.check(h.etm_grad_sqnorm_gated(t["g"].data_ptr(), n, partial.data_ptr(), n_partial, stepd.data_ptr(), kl.data_ptr(), 1.0,
                                          words.data_ptr(), 0, st), "etm_grad_sqnorm_gated")
        lib.check(h.etm_adamw_clip_gated(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), n, partial.data_ptr(),
                                         n_partial, *tail, words.data_ptr(), st), "etm_adamw_clip_gated")
    torch.cuda.synchronize()
    out = {k: x.cpu().numpy() for k, x in t.items()}
    out.update(partial=partial.cpu().numpy(), norm=np.float32(norm.item()), step=int(stepd.item()), lr=np.float32(lrd.item()))
    return out


def _run_case(case, a):
    return _run(a, case["n_partial"], case["step"], case["lr"], case, case["max_norm"], case["grad_scale"])


def _check_norm(case, a, out, what):
    """Exact: every element counted once, the norm's bits, the step count."""
    s = orf.exact_sumsq(a["g"])
    assert s < 2 ** 24
    part = out["partial"]
    assert not np.isnan(part).any(), (what, "a workgroup wrote no partial sum", int(np.isnan(part).sum()))
    assert np.array_equal(part, np.rint(part)) and int(part.astype(np.int64).sum()) == s, (what, int(part.astype(np.int64).sum()), s)
    want = np.float32(np.sqrt(np.float32(s)) * np.float32(case["grad_scale"]))
    assert _bits(out["norm"]) == _bits(want), (what, float(out["norm"]), float(want))
    assert out["step"] == case["step"] + 1, (what, out["step"])
    assert _bits(out["lr"]) == _bits(np.float32(case["lr"]))


def _check_parameters(p_start, got, ref, what, factor=1.0):
    finite = np.isfinite(ref["p"])
    assert np.array_equal(np.isfinite(got), finite), what
    err = np.abs(got.astype(np.float64) - ref["p"])[finite]
    tol = (factor * P_TOL * orf.scale_of(p_start, ref))[finite]
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(tol, 1e-300)).max()))


def _check_elements(case, a, out, r32, r64, what):
    """g, m, v: the bits of step32 (the coefficient is exact); p: step64 under the recorded tolerance."""
    for k in ("g", "m", "v"):
        diff = np.flatnonzero(_bits(out[k]) != _bits(r32[k]))
        assert diff.size == 0, (what, k, diff.size, diff[:4].tolist(), out[k][diff[:4]].tolist(), r32[k][diff[:4]].tolist())
    _check_parameters(a["p"], out["p"], r64, what)


def _what(case):
    return {k: v for k, v in case.items() if k != "seed"}


# ------------------------------------------------------------------ the pair of launches, one step
@pytest.mark.parametrize("n", orf.NS)
def test_norm_is_exact_and_elements_follow_the_references_at_every_shape(n):
    cases = [c for c in orf.shape_cases() if c["n"] == n]
    assert [c["n_partial"] for c in cases] == list(orf.N_PARTIALS)
    for case in cases:
        a, r32, r64 = orf.reference_pair(case)
        out = _run_case(case, a)
        _check_norm(case, a, out, _what(case))
        _check_elements(case, a, out, r32, r64, _what(case))
        clipped = not np.array_equal(out["g"], a["g"])
        assert clipped == (case["max_norm"] == orf.MAX_NORMS["clipping"]), _what(case)


def test_past_the_workgroup_cap_of_the_adamw_launch():
    """n / 4 = 2048 * 1024 + 257: 2048 workgroups, and the first 257 threads walk a fifth round."""
    case = orf.cap_case()
    assert case["n"] // 4 > 2048 * 256 * 4 and case["n"] // 4 - 2048 * 256 * 4 == 257
    a, r32, r64 = orf.reference_pair(case)
    out = _run_case(case, a)
    _check_norm(case, a, out, "cap")
    _check_elements(case, a, out, r32, r64, "cap")
    assert not np.array_equal(out["g"], a["g"])


@pytest.mark.parametrize("lr", orf.LRS)
@pytest.mark.parametrize("mode", list(orf.MAX_NORMS))
def test_every_max_norm_start_step_hyper_parameter_and_lr(mode, lr):
    cases = orf.cross_cases(mode, lr)
    assert len(cases) == len(orf.STEPS) * len(orf.HYPERS)
    for case in cases:
        a, r32, r64 = orf.reference_pair(case)
        out = _run_case(case, a)
        _check_norm(case, a, out, _what(case))
        _check_elements(case, a, out, r32, r64, _what(case))
        assert np.array_equal(out["g"], a["g"]) == (mode != "clipping")
        if lr == 0.0:                                                   # the parameters do not move; the moments and the gradient do
            assert np.array_equal(_bits(out["p"]), _bits(a["p"]))
        else:
            assert not np.array_equal(out["p"], a["p"])
        assert not np.array_equal(out["m"], a["m"]) and not np.array_equal(out["v"], a["v"])


def test_mixed_signs_of_moment_and_gradient_keep_the_bits_of_the_float32_reference():
    """Arenas whose first moment does not share the gradient's sign (optimiser_reference.arena: there the increment is ill conditioned
    and |p| + |update| is no scale for it): the norm exactly, g, m, v bit for bit."""
    for i, (n, n_partial) in enumerate(((4100, 3), (40004, 257))):
        for mode in orf.MAX_NORMS:
            case = dict(n=n, n_partial=n_partial, seed=3000 + i, span=3, max_norm=orf.MAX_NORMS[mode], step=9, lr=3e-4, grad_scale=1.0, **orf.DEFAULT)
            a = orf.arena(n, case["seed"], 3, mixed=True)
            assert (a["m"] * a["g"] < 0).mean() > 0.3
            _, r32, _ = orf.reference_pair(case, a)
            out = _run_case(case, a)
            _check_norm(case, a, out, _what(case))
            for k in ("g", "m", "v"):
                assert np.array_equal(_bits(out[k]), _bits(r32[k])), (_what(case), k)


# ------------------------------------------------------------------ exact identities
def test_lr_zero_leaves_the_parameters_and_moves_everything_else():
    case = dict(n=4100, n_partial=257, seed=41, span=3, max_norm=0.5, step=9, lr=0.0, grad_scale=1.0, **orf.DEFAULT)
    a = orf.arena(case["n"], case["seed"])
    out = _run_case(case, a)
    assert torch.equal(torch.from_numpy(out["p"]), torch.from_numpy(a["p"]))
    assert all(not np.array_equal(out[k], a[k]) for k in ("g", "m", "v")) and out["step"] == 10


@pytest.mark.parametrize("hyper", [orf.DEFAULT, orf.HYPERS[-1]], ids=["default", "b0.5-eps1e-5"])
def test_zero_gradient_on_zero_moments_only_decays(hyper):
    n = 4100
    a = orf.arena(n, 42)
    a = dict(p=a["p"], g=np.zeros(n, np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    for lr in (3e-4, 1.0):
        out = _run(a, 257, 0, lr, hyper, 0.5, 1.0)
        keep = np.float32(1.0 - orf.f32(lr) * hyper["weight_decay"])
        assert np.array_equal(_bits(out["p"]), _bits(a["p"] * keep)), "p' == float32(p * keep)"
        assert _bits(out["norm"]) == _bits(np.float32(0.0)) and not out["g"].any() and not out["m"].any() and not out["v"].any()
        assert (out["partial"] == 0).all()


@pytest.mark.parametrize("w", [2, 8])
def test_grad_scale_one_over_w_on_w_times_the_gradient_is_the_unscaled_step(w):
    """Data parallel: the arena holds the sum over w ranks.  Powers of two are exact, so every output bit equals the unscaled run's."""
    for mode in ("clipping", "not clipping"):
        case = dict(n=4100, n_partial=257, seed=43 + w, span=3, max_norm=orf.MAX_NORMS[mode], step=9, lr=3e-4, grad_scale=1.0, **orf.DEFAULT)
        a = orf.arena(case["n"], case["seed"])
        plain = _run_case(case, a)
        scaled = _run_case(dict(case, grad_scale=1.0 / w), dict(a, g=a["g"] * np.float32(w)))
        for k in ("p", "g", "m", "v", "norm"):
            assert np.array_equal(_bits(scaled[k]), _bits(plain[k])), (w, mode, k)
        assert scaled["step"] == plain["step"] == 10 and np.array_equal(scaled["partial"], plain["partial"] * np.float32(w * w))
        assert (mode == "clipping") == (not np.array_equal(plain["g"], a["g"]))


def test_grad_scale_one_third_on_three_times_the_gradient():
    for mode in ("clipping", "not clipping", "off"):
        case = dict(n=4100, n_partial=257, seed=47, span=3, max_norm=orf.MAX_NORMS[mode], step=9, lr=3e-4, grad_scale=1.0 / 3.0, **orf.DEFAULT)
        a = orf.arena(case["n"], case["seed"])
        a["g"] = a["g"] * np.float32(3.0)
        _, r32, r64 = orf.reference_pair(case, a)
        out = _run_case(case, a)
        _check_norm(case, a, out, mode)
        _check_elements(case, a, out, r32, r64, mode)
        third = orf.step64(a["p"], a["g"] / np.float32(3.0), a["m"], a["v"], 10, 3e-4, case["betas"], case["eps"], case["weight_decay"],
                           case["max_norm"], 1.0)
        assert np.allclose(r64["p"], third["p"], rtol=1e-6, atol=0) and np.allclose(r64["g"], third["g"], rtol=1e-6, atol=0), "the averaged gradient's step"


# ------------------------------------------------------------------ five consecutive steps
def test_five_consecutive_steps_against_five_float64_steps():
    """Random (non-integer) gradients, a changing lr, alternately clipped and not.  Norm: the longest chain of additions at this shape --
    a thread's rounds of four squares, the wave and workgroup trees (24 covers both launches' 8 + 8 levels, the root and the scale),
    a thread's share of the partial sums -- each adding 2^-24 relative.  Parameters: each step adds one step's tolerance."""
    n, n_partial, hyper = 40004, 1024, orf.DEFAULT
    n4 = n // 4
    norm_tol = (4 * math.ceil(n4 / (256 * n_partial)) + math.ceil(n_partial / 256) + 24) * U
    rng = np.random.default_rng(51)
    a = orf.arena(n, 51)
    state = dict(p=a["p"], m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    ref = {k: x.astype(np.float64) for k, x in state.items()}
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)          # an element's gradients share a sign: no cancelling moment (optimiser_reference.arena)
    for it in range(5):
        lr = 3e-4 * (1 - 0.1 * it)
        g = (np.abs(rng.standard_normal(n)) * sign * (10.0 if it % 2 == 0 else 1e-3)).astype(np.float32)   # norm 2000 / 0.2 against max_norm 0.5
        out = _run(dict(state, g=g), n_partial, it, lr, hyper, 0.5, 1.0)
        p_before = ref["p"]
        r64 = orf.step64(ref["p"], g, ref["m"], ref["v"], it + 1, lr, hyper["betas"], hyper["eps"], hyper["weight_decay"], 0.5, 1.0)
        assert (r64["coef"] < 1.0) == (it % 2 == 0)
        assert out["step"] == it + 1 and abs(float(out["norm"]) - r64["total"]) <= norm_tol * r64["total"], (it, float(out["norm"]), r64["total"])
        assert np.array_equal(out["g"], g) == (it % 2 == 1)
        assert np.all(np.abs(out["g"] - r64["g"]) <= (norm_tol + 4 * U) * np.abs(r64["g"])), it
        _check_parameters(p_before, out["p"], r64, f"step {it}", factor=it + 1)
        for k, mag in (("m", np.abs(r64["m"]) + np.abs(r64["g"])), ("v", np.abs(r64["v"]))):
            assert np.all(np.abs(out[k] - r64[k]) <= (it + 1) * 2 * (norm_tol + 4 * U) * mag), (it, k)
        state = {k: out[k] for k in ("p", "m", "v")}
        ref = {k: r64[k] for k in ("p", "m", "v")}


# ------------------------------------------------------------------ non-finite gradients
@pytest.mark.parametrize("where", [0, 2049, 4099], ids=["first", "middle", "last"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradient_follows_the_rule_of_clip_grad_norm(bad, where):
    """max_norm > 0: one NaN makes the norm, the coefficient and with them everything NaN; one +inf makes the coefficient 0: NaN at that
    element, gradient 0 elsewhere, where decay and the old momentum alone move the parameter.  The gated twin gives the same bits.
    max_norm 0: nothing is clipped and the NaN stays in its element."""
    case = dict(n=4100, n_partial=257, seed=61, span=3, max_norm=0.5, step=9, lr=3e-4, grad_scale=1.0, **orf.DEFAULT)
    a = orf.arena(case["n"], case["seed"])
    a["g"][where] = bad
    for max_norm in (0.5, 0.0):
        c = dict(case, max_norm=max_norm)
        _, r32, r64 = orf.reference_pair(c, a)
        out = _run_case(c, a)
        assert out["step"] == 10
        assert np.isnan(out["norm"]) if math.isnan(bad) else out["norm"] == np.inf
        for k in ("p", "g", "m", "v"):
            assert np.array_equal(np.isnan(out[k]), np.isnan(r64[k])), (max_norm, k, int(np.isnan(out[k]).sum()), int(np.isnan(r64[k]).sum()))
        ok = ~np.isnan(r64["g"])
        for k in ("g", "m", "v"):
            assert np.array_equal(_bits(out[k])[ok], _bits(r32[k])[ok]), (max_norm, k)
        _check_parameters(a["p"], out["p"], r64, (bad, where, max_norm))
        others = np.arange(case["n"]) != where
        if max_norm > 0 and math.isnan(bad):
            assert all(np.isnan(out[k]).all() for k in ("p", "g", "m", "v"))
        elif max_norm > 0:
            assert not out["g"][others].any() and np.isfinite(out["p"][others]).all() and np.isnan(out["p"][where])
        else:
            assert np.isnan(out["p"][where]) and all(np.isfinite(out[k][others]).all() for k in ("p", "g", "m", "v"))
            assert np.array_equal(out["g"][others], a["g"][others])
        gated = _run(a, c["n_partial"], c["step"], c["lr"], c, max_norm, 1.0, gate_kl=0.5)
        for k in ("p", "g", "m", "v"):
            assert np.array_equal(np.isnan(gated[k]), np.isnan(out[k])) and np.array_equal(_bits(gated[k])[ok], _bits(out[k])[ok]), ("gated", k)


# ------------------------------------------------------------------ monitored norms: the kernel pair
SEG_LENS = (1, 3, 255, 256, 257, 4095, 4096)


def _segments(lengths, seed):
    """Segments of {-1, 0, 1} at odd offsets with gaps of 1000.0 between them -> (flat, starts, lens)."""
    rng = np.random.default_rng(seed)
    starts, pos = [], 1
    for n in lengths:
        if pos % 2 == 0:
            pos += 1
        starts.append(pos)
        pos += n + 1
    flat = np.full(pos + 3, 1000.0, dtype=np.float32)
    for s, n in zip(starts, lengths):
        flat[s: s + n] = rng.integers(-1, 2, size=n).astype(np.float32)
        flat[s + n - 1] = 1.0                                           # (the last element counts: a short read shows)
    return flat, np.asarray(starts, dtype=np.int64), np.asarray(lengths, dtype=np.int32)


def _group_norms(flat, starts, lens, member):
    from etm import lib
    dev = rh.dev()
    f, s, n, mem = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (flat, starts, lens, member))
    partial = torch.full((len(lens),), float("nan"), device=dev)
    out = torch.full((member.shape[0],), float("nan"), device=dev)
    lib.check(lib.load().etm_group_norms(f.data_ptr(), s.data_ptr(), n.data_ptr(), len(lens), mem.data_ptr(), member.shape[0], partial.data_ptr(),
                                         out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "etm_group_norms")
    torch.cuda.synchronize()
    return partial.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("n_groups", [1, 12])
@pytest.mark.parametrize("n_segs", [1, 255, 256, 257, 700])
def test_group_norms_are_exact_on_integer_segments(n_segs, n_groups):
    rng = np.random.default_rng(100 * n_segs + n_groups)
    layouts = [[n] for n in SEG_LENS] if n_segs == 1 else [[SEG_LENS[i] for i in rng.integers(0, len(SEG_LENS), size=n_segs)]]
    for lengths in layouts:
        if n_segs > 1:
            lengths[:len(SEG_LENS)] = SEG_LENS                            # (every length is there)
        flat, starts, lens = _segments(lengths, seed=n_segs + n_groups)
        assert (starts % 2 == 1).all() and (starts[1:] > starts[:-1] + lens[:-1]).all()
        members = [rng.integers(0, 3, size=(n_groups, n_segs)).astype(np.float32)]
        members[0][:, -1] = np.maximum(members[0][:, -1], 1.0)           # (the last segment counts: a short sum over the segments shows)
        if n_groups == 12:
            members[0][5] = 0.0
        else:
            members.append(np.zeros((1, n_segs), dtype=np.float32))      # one group: the all-zero row as a run of its own
        for member in members:
            want, q = orf.group_norms64(flat, starts, lens, member)
            sums = member.astype(np.float64) @ q
            assert sums.max() < 2 ** 24 and np.array_equal(q, np.rint(q))
            partial, out = _group_norms(flat, starts, lens, member)
            assert np.array_equal(partial.astype(np.float64), q), (lengths[:8], np.flatnonzero(partial != q)[:4])
            assert np.array_equal(_bits(out), _bits(np.sqrt(sums.astype(np.float32)))), (out, want)
            if not member.any(axis=1).all():
                assert _bits(out[np.flatnonzero(~member.any(axis=1))[0]]) == 0, "an all-zero row's norm is +0.0"


# ------------------------------------------------------------------ monitored norms: through the trainer
TRAINERS = {
    "trxl post-LN, image, two branches": dict(
        environment=dict(type="Synthetic", obs_shape=[3, 84, 84], num_actions=[2, 3], max_episode_steps=16, seed=2, p_done=0.1, pool=4),
        normalize_observations=None),
    "gtrxl pre-LN, vector": dict(
        transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative", layer_norm="pre", gtrxl=True,
                         gtrxl_bias=1.0)),
}


@pytest.mark.parametrize("name", list(TRAINERS))
def test_monitored_norms_of_a_trainer_match_the_definition_over_grad_groups(name):
    over = dict(TRAINERS[name])
    cfg = rh.config(**rh.modes(False), **over)
    if cfg.get("normalize_observations", 0) is None:
        del cfg["normalize_observations"]                                # (the table is for vector observations)
    tr = None
    try:
        tr = rh.trainer(cfg, seed=11, run_id="optnorms")
        assert cfg["hidden_layer_size"] == 64 and len(tr.model.policy_branches) == (2 if "two branches" in name else 1)
        lr, beta, clip = tr.schedules(0)
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        idx = torch.arange(0, rh.W_T * rh.S_T, 2, device=tr.device)
        tr._train_mini_batch(tr.buffer.gather(idx), float(lr), clip, beta)
        got = tr._grad_group_norms().cpu().numpy()
        torch.cuda.synchronize()
        groups = tr.model._grad_groups()
        assert list(groups) == tr._grad_keys and got.shape == (len(groups),)
        n_segs = int(tr._seg_start.numel())
        tol = (math.ceil(n_segs / 256) + 40) * U
        for i, (key, modules) in enumerate(groups.items()):
            want = math.sqrt(sum(float(p.grad.detach().double().square().sum()) for m in modules for p in m.parameters()))
            assert want > 0.0 and abs(float(got[i]) - want) <= tol * want, (key, float(got[i]), want)
        # the segment table: inside one parameter, <= 4096, every parameter element once, nothing of the padding
        opt = tr.optimizer
        base, total, padded = opt.flat_grads.data_ptr(), opt.total, opt.flat_grads.numel()
        assert tr.flat_grads.data_ptr() == base and tr.flat_grads.numel() == total
        starts, lens = tr._seg_start.cpu().numpy(), tr._seg_len.cpu().numpy()
        seg_member, grad_member = tr._seg_member.cpu().numpy(), tr._grad_member.cpu().numpy()
        assert seg_member.shape == (len(groups), n_segs) and grad_member.shape == (len(groups), len(tr.params))
        first = np.array([(v.data_ptr() - base) // 4 for v in tr._grad_views])
        size = np.array([v.numel() for v in tr._grad_views])
        assert [v.data_ptr() for v in tr._grad_views] == [p.grad.data_ptr() for p in tr.params] and int(size.sum()) == total
        assert (lens >= 1).all() and (lens <= 4096).all() and (size == 4096).any(), "a 64 x 64 weight is one full segment"
        cover = np.zeros(padded, dtype=np.int64)
        for s in range(n_segs):
            owner = np.flatnonzero((first <= starts[s]) & (starts[s] + lens[s] <= first + size))
            assert owner.size == 1, (s, int(starts[s]), int(lens[s]))
            cover[starts[s]: starts[s] + lens[s]] += 1
            assert np.array_equal(seg_member[:, s], grad_member[:, owner[0]]), s
        assert (cover[:total] == 1).all() and not cover[total:].any()
    finally:
        rh.release(tr)
