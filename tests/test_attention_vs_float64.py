"""-m gpu: every instantiation of the training window attention against a float64 evaluation (oracle/ref_model.py).

Kernel #1 of training has two families behind ``ops.mha``: the folded window pass (csrc/window_attn.hip,
``window_pass_kernel<NJ, RW, NW, HAS_LN, HAS_POS, FULLD>``, forward and backward) and the dense fp32-MFMA kernels
(csrc/mha_fwd.hip ``mha_fwd_kernel<HT, LN, POS>``, csrc/mha_bwd.hip ``bwd_dw_kernel<LN, POS>`` / ``bwd_dx_kernel<LN>``).  norm_kv's
gain / bias gradients of the folded pass take one of three routes (``_WindowFn.backward`` in etm/ops.py): "outputs"
(``ln_grad_from_outputs_kernel<NJ>`` + the guarded ``window_ln_grad_kernel<NJ, HMAX>``), "rows" (``window_ln_grad_kernel``) or the
generic ``etm_window_dx`` (``bwd_dx_kernel``).  The functions below restate the host dispatch; the case list is generated from
the cell sets (one case per folded cell, its shape picked to reach the dense and norm_kv cells too) plus named edge cases, and
``test_attention_matrix_covers_every_instantiation`` checks that nothing is left out.

Each case: a block-major bank (3 blocks, the middle one used) read through the episode indirection, positional rows gathered
at ``pidx != win``, N not a multiple of 8, mask prefixes of 0 (fully masked: uniform attention), 1, L and random counts, LayerNorm
gains / biases away from 1 / 0, a learned (grad) or fixed positional table.  The oracle is ``ref_model.mha`` run on the device in
float64 on the same fp32 values, gradients by float64 autograd with the same upstream gradient.  Error metric: max |got - ref| /
max |ref| per tensor, and per sample row for ctx and att.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

CAP_FWD, CAP_GRAD = 1e-5, 1e-4
# About 4x the worst error measured over the whole matrix on the MI355X (second column: worst, and the case), within the caps
# CAP_FWD (ctx, att, cached_*) and CAP_GRAD (gradients).
BOUNDS = {
    "ctx": 1.0e-5,           # 3.0e-6  hot_D256H4L32/dense (4x would pass the cap)
    "att": 1.0e-5,           # 2.6e-6  hot_D768H6L64/dense (4x would pass the cap)
    "dq": 1.3e-5,            # 3.3e-6  hot_D768H6L64/dense
    "dwk": 1.1e-5,           # 2.7e-6  hot_D256H4L32/dense
    "dwv": 8.5e-6,           # 2.1e-6  hot_D768H6L64/dense
    "dln_g": 7.5e-6,         # 1.8e-6  hot_D256H4L32/folded/rows
    "dln_b": 3.5e-6,         # 8.2e-7  hot_D768H6L64/folded
    "dpos": 6.2e-6,          # 1.5e-6  hot_D512H4L128/dense
    "cached_ctx": 1.3e-6,    # 3.2e-7  nj1_r8x8_ln_learned_part_D96H1L48
    "cached_att": 1.65e-6,   # 4.1e-7  nj1_r8x8_ln_learned_part_D96H1L48
}
WORST = {}   # quantity -> (error, case): printed at the end of the module


# ------------------------------------------------------------------ dispatch rules (python restatement of the host code)
def _nj(D):
    """window_attn.hip ``dispatch``: NJ = ceil(D / 128); 5 runs as 6 and 7 as 8."""
    nj = -(-D // 128)
    return {5: 6, 7: 8}.get(nj, nj)


def _folded_inst(D, L, ln, pos):
    """window_attn.hip: ``dispatch`` (NJ), ``dispatch_rows<NJ>`` (RW, NW: (8,4) L <= 32, (8,8) L <= 64, (16,8) L <= 128 for
    NJ <= 4 only), ``launch_pass`` (HAS_LN = ln_g given, HAS_POS = pos given), ``launch_pass2`` (FULLD = D == 128 NJ)."""
    nj = _nj(D)
    if L <= 32:
        rw, nw = 8, 4
    elif L <= 64:
        rw, nw = 8, 8
    else:
        assert nj <= 4, (D, L)
        rw, nw = 16, 8
    return ("pass", nj, rw, nw, bool(ln), bool(pos), D == 128 * nj)


def _dense_insts(D, H, ln, pos, wants_dx):
    """mha_fwd.hip ``etm_mha_fwd`` / ``launch_fwd<HT>`` (HT = hd / 32, LN, POS); mha_bwd.hip ``etm_mha_bwd``: ``bwd_dw_kernel<LN,
    POS>`` always, ``bwd_dx_kernel<LN>`` (step B3) only when d_ln_g or d_pos is asked for."""
    cells = {("fwd", (D // H) // 32, bool(ln), bool(pos)), ("dw", bool(ln), bool(pos))}
    if wants_dx:
        cells.add(("dx", bool(ln)))
    return cells


def _ln_grad_route(D, H, L, pos_grad, fused_ln_grad):
    """etm/ops.py ``_WindowFn.backward`` (route) and window_ln_grad.hip ``window_ln_grad_launch`` (``switch (D / 128)``, HMAX 4 if
    H <= 4 else 8) / ``etm_window_ln_grad_from_outputs`` (NJ = D / 128) -> (route, cells)."""
    if fused_ln_grad and not pos_grad and D % 128 == 0 and D <= 512 and H <= 8 and L <= 128:
        rows_cell = ("ln_rows", D // 128, 4 if H <= 4 else 8)
        if fused_ln_grad == "rows":
            return "rows", {rows_cell}
        return "outputs", {("ln_outputs", D // 128), rows_cell}
    return "generic", {("dx", True)}


ALL_FOLDED = {("pass", nj, rw, nw, ln, pos, full) for nj in (1, 2, 3, 4, 6, 8) for rw, nw in ((8, 4), (8, 8), (16, 8))
              for ln in (False, True) for pos in (False, True) for full in (False, True) if nj <= 4 or rw == 8}
ALL_DENSE = ({("fwd", ht, ln, pos) for ht in (1, 2, 3, 4) for ln in (False, True) for pos in (False, True)}
             | {("dw", ln, pos) for ln in (False, True) for pos in (False, True)} | {("dx", False), ("dx", True)})
ALL_LN_GRAD = {("ln_rows", nj, hm) for nj in (1, 2, 3, 4) for hm in (4, 8)} | {("ln_outputs", nj) for nj in (1, 2, 3, 4)}
ALL_ROUTES = {"outputs", "rows", "generic"}


def _dw_plan(N, L, D):
    """mha_bwd.hip ``plan_dw``: (splits, chunks, chunks_per_split) of the split-K dW contraction (RB = 32, 128 x 128 tiles)."""
    lp = -(-L // 32) * 32
    chunks = N * lp // 32
    tiles = -(-2 * D // 128) * -(-D // 128)
    splits = max(1, min(256 // tiles, chunks))
    cps = -(-chunks // splits)
    return -(-chunks // cps), chunks, cps


def _ln_settings(c):
    """fused_ln_grad settings whose routes differ for this case (one setting when they all take the generic route)."""
    if not c["ln"]:
        return [True]
    if _ln_grad_route(c["D"], c["H"], c["L"], c["pos"] == "learned", True)[0] == "generic":
        return [True]
    return ["outputs", "rows", False]


def _impls(c):
    from etm import ops
    pos_grad = c["pos"] == "learned"
    got = []
    if ops.attention_supported(c["D"], c["H"], c["L"], c["ln"], pos_grad, impl="folded") == "folded":
        got.append("folded")
    if ops.dense_supported(c["D"], c["L"], c["H"]):
        got.append("dense")
    return got


def _cells(c):
    """Every instantiation a case reaches: (folded forward cells, folded backward cells, dense cells, norm_kv cells, routes)."""
    ln, pos, pos_grad = c["ln"], c["pos"] != "none", c["pos"] == "learned"
    fwd, bwd, dense, lng, routes = set(), set(), set(), set(), set()
    impls = _impls(c)
    if "folded" in impls:
        fwd.add(_folded_inst(c["D"], c["L"], ln, pos))
        bwd.add(_folded_inst(c["D"], c["L"], ln, pos))
        for s in _ln_settings(c) if ln or pos_grad else []:
            route, cells = _ln_grad_route(c["D"], c["H"], c["L"], pos_grad, s) if ln else ("generic", {("dx", ln)})
            routes.add(route)
            (dense if route == "generic" else lng).update(cells)
    if "dense" in impls:
        dense |= _dense_insts(c["D"], c["H"], ln, pos, ln or pos_grad)
    return fwd, bwd, dense, lng, routes


# ------------------------------------------------------------------ the case matrix
_N_CYCLE = (13, 5, 21, 3, 37, 7, 11, 29, 6, 19)
_L_BY_ROWS = {(8, 4): (32, 9, 24), (8, 8): (64, 33, 48), (16, 8): (128, 65, 100)}
_DH_FULL = {1: ((128, 4), (128, 1), (128, 2), (128, 8)), 2: ((256, 2), (256, 8), (256, 4)), 3: ((384, 3), (384, 6), (384, 12), (384, 4)),
            4: ((512, 4), (512, 8), (512, 16)), 6: ((768, 6), (768, 8), (768, 12)), 8: ((1024, 8), (1024, 16), (1024, 32))}
_DH_PART = {1: ((96, 1), (96, 3), (64, 2), (32, 1)), 2: ((160, 5), (192, 2), (192, 6), (224, 7)), 3: ((352, 11), (288, 3), (320, 5), (288, 9)),
            4: ((480, 15), (480, 5), (448, 7), (416, 13)), 6: ((640, 5), (576, 6), (704, 22), (544, 17), (672, 7)),
            8: ((896, 7), (960, 10), (928, 29), (800, 25), (992, 31))}


def _case(name, D, H, L, N, ln, pos, hot=False):
    return dict(name=name, D=D, H=H, L=L, N=N, ln=ln, pos=pos, hot=hot)


def _generate():
    """One case per folded cell.  Its L comes from the cell's row tiling, (D, H) from the cell's NJ / FULLD: the candidate that
    reaches the most dense / norm_kv cells not reached yet (first candidate in rotation on a tie).  Positional cells alternate
    between a learned table (gradient) and a fixed one."""
    cases, seen = [], set()
    for i, (_, nj, rw, nw, ln, pos, full) in enumerate(sorted(ALL_FOLDED)):
        L = _L_BY_ROWS[(rw, nw)][i % 3]
        posk = ("learned" if (i // 2) % 2 else "relative") if pos else "none"
        opts = (_DH_FULL if full else _DH_PART)[nj]
        best = None
        for k in range(len(opts)):
            D, H = opts[(i + k) % len(opts)]
            c = _case("", D, H, L, _N_CYCLE[i % len(_N_CYCLE)], ln, posk)
            if "folded" not in _impls(c):
                continue
            _, _, dense, lng, routes = _cells(c)
            gain = len((dense | lng | routes) - seen)
            if best is None or gain > best[0]:
                best = (gain, c)
        c = best[1]
        seen |= set().union(*_cells(c)[2:])
        c["name"] = f"nj{nj}_r{rw}x{nw}_{'ln' if ln else 'noln'}_{posk}_{'full' if full else 'part'}_D{c['D']}H{c['H']}L{L}"
        cases.append(c)
    return cases


EDGE_CASES = [
    _case("splitk_ragged_D384H4L64N37", 384, 4, 64, 37, True, "learned"),     # dense dW: 13 splits of 6 chunks, the last of 2
    _case("splitk_D128H4L128N45", 128, 4, 128, 45, False, "relative"),
    _case("n1_D256H8L17", 256, 8, 17, 1, True, "relative"),
    _case("n2_D1024H8L64", 1024, 8, 64, 2, True, "learned"),
    _case("hd2_D64H32L20", 64, 32, 20, 11, True, "none"),                       # folded only: hd 2
    _case("hot_D256H4L32", 256, 4, 32, 13, True, "relative", hot=True),
    _case("hot_D512H4L128", 512, 4, 128, 9, False, "learned", hot=True),
    _case("hot_D768H6L64", 768, 6, 64, 7, True, "none", hot=True),
]
CASES = _generate() + EDGE_CASES


# ------------------------------------------------------------------ one case
def _record(name, err, case):
    if name not in WORST or err > WORST[name][0]:
        WORST[name] = (err, case)


def _rel(got, ref, rows=False):
    got, ref = got.detach().double(), ref.detach().double()
    if rows:
        d = (got - ref).abs().reshape(ref.shape[0], -1).amax(dim=1)
        return float((d / ref.abs().reshape(ref.shape[0], -1).amax(dim=1).clamp(min=1e-30)).max())
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def _check(name, got, ref, case, rows=False):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{case}: {name} not finite"
    err = _rel(got, ref, rows)
    _record(name, err, case)
    assert err <= BOUNDS[name], f"{case}: {name} error {err:.3e} > bound {BOUNDS[name]:.1e}"


def _inputs(c, dev):
    D, H, L, N = c["D"], c["H"], c["L"], c["N"]
    g = torch.Generator().manual_seed(1000 * D + 10 * L + N + 7 * H)
    E, T, nb = 5, L + 11, 3
    bank = torch.randn((nb, E, T, D), generator=g)                                  # block-major memory, viewed as [E, T, nb, D]
    ep = torch.randint(0, E, (N,), generator=g)
    win = (torch.randint(0, T - L + 1, (N,), generator=g)[:, None] + torch.arange(L)[None, :]).long()
    pidx = (win + 1 + torch.randint(0, 10, (N, 1), generator=g)) % T                # != win (Q5)
    cnt = torch.randint(0, L + 1, (N,), generator=g)
    cnt[: min(N, 3)] = torch.tensor([0, 1, L])[: min(N, 3)]
    mask = torch.arange(L)[None, :] < cnt[:, None]
    sgn = lambda n: torch.where(torch.rand((n,), generator=g) < 0.5, -1.0, 1.0)
    x = dict(
        wk=torch.randn((D, D), generator=g) / D ** 0.5, wv=torch.randn((D, D), generator=g) / D ** 0.5,
        lg=sgn(D) * (0.5 + 1.5 * torch.rand((D,), generator=g)), lb=sgn(D) * (0.2 + 0.8 * torch.rand((D,), generator=g)),
        table=torch.randn((T, D), generator=g) * 0.5, q=torch.randn((N, D), generator=g), gout=torch.randn((N, D), generator=g))
    dv = {k: v.to(dev) for k, v in x.items()}
    dv.update(bank=bank.to(dev).permute(1, 2, 0, 3), ep=ep.to(dev), win=win.to(dev), pidx=pidx.to(dev), mask=mask.to(dev), cnt=cnt)
    if c["hot"]:
        dv["q"] = dv["q"] * _hot_scale(c, dv)
    return dv


def _window_rows(c, t, dtype):
    """Window rows of block 1 (+ positional rows, LayerNorm) in ``dtype``: [N, L, D] and the leaves that need gradients."""
    from oracle import ref_model as rm
    leaves = {k: t[k].to(dtype).requires_grad_(True) for k in ("q", "wk", "wv", "lg", "lb", "table")}
    x = t["bank"].to(dtype)[t["ep"][:, None], t["win"]][:, :, 1]
    if c["pos"] != "none":
        x = x + (leaves["table"] if c["pos"] == "learned" else leaves["table"].detach())[t["pidx"]]
    if c["ln"]:
        x = rm._ln({"n.weight": leaves["lg"], "n.bias": leaves["lb"]}, "n", x, 1e-5)
    return x, leaves


def _oracle(c, t, with_grad=True):
    from oracle import ref_model as rm
    D, H = c["D"], c["H"]
    x, lv = _window_rows(c, t, torch.float64)
    eye = torch.eye(D, dtype=torch.float64, device=x.device)
    sd = {"a.values.weight": lv["wv"], "a.keys.weight": lv["wk"], "a.queries.weight": eye, "a.fc_out.weight": eye,
          "a.fc_out.bias": torch.zeros(D, dtype=torch.float64, device=x.device)}
    ctx3, a4 = rm.mha(sd, "a", H, x, x, lv["q"].unsqueeze(1), t["mask"])
    ref = dict(ctx=ctx3[:, 0].detach(), att=a4[:, :, 0].detach())
    if with_grad:
        (ctx3[:, 0] * t["gout"].double()).sum().backward()
        ref.update(dq=lv["q"].grad, dwk=lv["wk"].grad, dwv=lv["wv"].grad)
        if c["ln"]:
            ref.update(dln_g=lv["lg"].grad, dln_b=lv["lb"].grad)
        if c["pos"] == "learned":
            ref["dpos"] = lv["table"].grad
    return ref


def _hot_scale(c, t):
    """Query scale that makes the median (over samples with >= 2 unmasked rows and heads) score spread max - min, after the
    1 / sqrt(D), equal to 30: most samples attend nearly one-hot, the rest keep finite softmax gradients."""
    D, H, hd = c["D"], c["H"], c["D"] // c["H"]
    with torch.no_grad():
        x, lv = _window_rows(dict(c, hot=False), t, torch.float64)
        k = (x @ lv["wk"].t()).reshape(x.shape[0], x.shape[1], H, hd)
        e = torch.einsum("nhd,nlhd->nhl", lv["q"].reshape(-1, H, hd), k) / D ** 0.5
        m = t["mask"][:, None, :]
        spread = e.masked_fill(~m, -float("inf")).amax(dim=2) - e.masked_fill(~m, float("inf")).amin(dim=2)
        sel = (t["cnt"] >= 2).to(spread.device)
        return float(30.0 / spread[sel].median())


def _run(c, t, impl):
    """ops.mha forward + backward on the device -> {quantity: tensor}."""
    from etm import ops
    N, H = c["N"], c["H"]
    lv = {k: t[k].clone().requires_grad_(k != "table" or c["pos"] == "learned") for k in ("q", "wk", "wv", "lg", "lb", "table")}
    spec = ops.WindowSpec.from_bank(t["bank"], t["ep"], t["win"], t["pidx"] if c["pos"] != "none" else None, t["mask"])
    ln = (lv["lg"], lv["lb"]) if c["ln"] else (None, None)
    out, att = ops.mha(lv["q"], lv["wk"], lv["wv"], spec, 1, H, *ln, lv["table"] if c["pos"] != "none" else None, impl=impl)
    (out * t["gout"]).sum().backward()
    got = dict(ctx=out.detach(), att=att.detach(), dq=lv["q"].grad, dwk=lv["wk"].grad, dwv=lv["wv"].grad)
    if c["ln"]:
        got.update(dln_g=lv["lg"].grad, dln_b=lv["lb"].grad)
    if c["pos"] == "learned":
        got["dpos"] = lv["table"].grad
    torch.cuda.synchronize()
    return got


def _skip_applies(c, cnt):
    """Some sample with an unmasked row has a wave all of whose rows are masked (or past L): the masked-wave skip runs."""
    _, _, rw, nw, *_ = _folded_inst(c["D"], c["L"], c["ln"], c["pos"] != "none")
    return any(1 <= int(n) <= (nw - 1) * rw for n in cnt)


def _compare(got, ref, label):
    for k, want in ref.items():
        _check(k, got[k], want, label, rows=k in ("ctx", "att"))


def _attention_properties(got, t, label):
    att, L = got["att"], got["att"].shape[-1]
    for n, k in enumerate(t["cnt"].tolist()):
        if k == 0:
            assert float((att[n] - 1.0 / L).abs().max()) <= 1e-6, f"{label}: fully masked sample {n} is not uniform"
        else:
            masked = att[n][:, k:]
            assert bool((masked == 0).all()), f"{label}: sample {n} (count {k}) has nonzero weight at masked slots"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\n[attention f64] worst error per quantity (max |got - ref| / max |ref|):")
    for k in BOUNDS:
        if k in WORST:
            print(f"  {k:<11} {WORST[k][0]:.3e}  bound {BOUNDS[k]:.1e}  {WORST[k][1]}")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_attention_vs_float64(case):
    from etm import lib as etm_lib
    from etm import ops
    c = case
    dev = torch.device("cuda", 0)
    t = _inputs(c, dev)
    ref = _oracle(c, t)
    impls = _impls(c)
    assert impls, c["name"]
    for impl in impls:
        settings = _ln_settings(c) if impl == "folded" else [True]
        runs = []
        try:
            for s in settings:
                ops.set_ln_grad_kernel(s)
                got = _run(c, t, impl)
                label = f"{c['name']}/{impl}/fused_ln_grad={s}"
                _compare(got, ref, label)
                _attention_properties(got, t, label)
                runs.append(got)
        finally:
            ops.set_ln_grad_kernel(True)
        if impl == "folded" and _skip_applies(c, t["cnt"]):
            lib = etm_lib.load()
            try:
                lib.etm_window_set_skip_masked(0)
                full = _run(c, t, impl)
            finally:
                lib.etm_window_set_skip_masked(1)
            # etm_window_dx accumulates its gradients with atomics (order varies run to run): those are held to the bounds instead
            atomic = {"dpos"} | ({"dln_g", "dln_b"} if _ln_grad_route(c["D"], c["H"], c["L"], c["pos"] == "learned", True)[0] == "generic"
                                 else set())
            for k, v in runs[0].items():
                if k in atomic:
                    _check(k, full[k], ref[k], f"{c['name']}/folded/no_skip")
                else:
                    assert torch.equal(v, full[k]), f"{c['name']}: {k} differs with the masked-wave skip off"
    if not c["hot"] and c["D"] // c["H"] % 4 == 0 and c["D"] // c["H"] <= 256:
        _cached_vs_float64(c, t)


def _cached_vs_float64(c, t):
    """ops.attn_cached (rollout path) over a K | V cache built from the fp32 projections of every bank row (its positional row
    is the row's own step, as in the rollout), against float64 attention over the same cached values."""
    from etm import ops
    from oracle import ref_model as rm
    D, H, L = c["D"], c["H"], c["L"]
    bank = t["bank"]
    E, T, nb, _ = bank.shape
    with torch.no_grad():
        x = bank + (t["table"][None, :, None, :] if c["pos"] != "none" else 0.0)
        if c["ln"]:
            x = torch.nn.functional.layer_norm(x, (D,), t["lg"], t["lb"], 1e-5)
        cache = torch.zeros((nb, E, T, 2 * D), device=bank.device).permute(1, 2, 0, 3)      # block-major like the bank
        cache[..., :D] = x @ t["wk"].t()
        cache[..., D:] = x @ t["wv"].t()
        spec = ops.WindowSpec.from_bank(cache, t["ep"], t["win"], None, t["mask"])
        ctx, att = ops.attn_cached(t["q"], spec, 1, H, want_att=True)
        kv = cache.double()[t["ep"][:, None], t["win"]][:, :, 1]
        eye = torch.eye(D, dtype=torch.float64, device=bank.device)
        sd = {"a.values.weight": eye, "a.keys.weight": eye, "a.queries.weight": eye, "a.fc_out.weight": eye,
              "a.fc_out.bias": torch.zeros(D, dtype=torch.float64, device=bank.device)}
        ref_ctx, ref_att = rm.mha(sd, "a", H, kv[..., D:], kv[..., :D], t["q"].double().unsqueeze(1), t["mask"])
    label = f"{c['name']}/attn_cached"
    _check("cached_ctx", ctx, ref_ctx[:, 0], label, rows=True)
    _check("cached_att", att, ref_att[:, :, 0], label, rows=True)
    _attention_properties(dict(att=att), t, label)


def test_attention_matrix_covers_every_instantiation():
    """Every reachable folded cell runs forward and backward, every dense and norm_kv cell and route runs, every case is a shape
    its path supports, and the dense dW split-K runs with several splits and a ragged last one."""
    from etm import ops
    for k, b in BOUNDS.items():
        assert b <= (CAP_FWD if k in ("ctx", "att", "cached_ctx", "cached_att") else CAP_GRAD), k
    fwd, bwd, dense, lng, routes = set(), set(), set(), set(), set()
    for c in CASES:
        f, b, d, l_, r = _cells(c)
        fwd |= f; bwd |= b; dense |= d; lng |= l_; routes |= r
        for impl in _impls(c):
            assert ops.attention_supported(c["D"], c["H"], c["L"], c["ln"], c["pos"] == "learned", impl=impl) == impl, c["name"]
        assert c["N"] % 8 != 0, c["name"]
    assert not ALL_FOLDED - fwd, sorted(ALL_FOLDED - fwd)
    assert not ALL_FOLDED - bwd, sorted(ALL_FOLDED - bwd)
    assert not ALL_DENSE - dense, sorted(ALL_DENSE - dense)
    assert not ALL_LN_GRAD - lng, sorted(ALL_LN_GRAD - lng)
    assert routes == ALL_ROUTES, routes
    plans = [_dw_plan(c["N"], c["L"], c["D"]) for c in CASES if "dense" in _impls(c)]
    assert any(s > 1 and ch % cps for s, ch, cps in plans), plans
    assert any(c["N"] < 8 for c in CASES) and any(c["hot"] and "folded" in _impls(c) for c in CASES)
    assert any(c["hot"] and "dense" in _impls(c) for c in CASES)


# ------------------------------------------------------------------ shape support at the limits
_SUPPORT_GRID = [(D, H, L) for D in (512, 768, 1024) for H in (4, 8, 16, 24, 32) for L in (32, 64, 65, 128) if D % H == 0] + [
    (512, 128, 128), (512, 256, 128), (512, 256, 64)]      # folded pass at large H: launch_pass3's LDS budget


@pytest.mark.parametrize("impl", ("folded", "dense"))
def test_attention_shape_support_is_consistent(impl):
    """At every point either the forward and the backward both complete, or ops.mha refuses the shape with a ValueError before
    any launch, as ops.attention_supported says (the trainer checks the same predicate when it is built)."""
    from etm import ops
    dev = torch.device("cuda", 0)
    refused, ran = [], 0
    for (D, H, L), (ln, posk) in itertools.product(_SUPPORT_GRID, ((False, "none"), (True, "none"), (False, "learned"))):
        c = _case("", D, H, L, 2, ln, posk)
        t = _inputs(c, dev)
        family = ops.attention_supported(D, H, L, ln, posk == "learned", impl=impl)
        if family is None:
            with pytest.raises(ValueError, match="attention_supported"):
                _run(c, t, impl)
            refused.append((D, H, L, ln, posk))
            continue
        got = _run(c, t, impl)
        for k, v in got.items():
            assert v is not None and bool(torch.isfinite(v).all()), (D, H, L, ln, posk, k)
        ran += 1
    print(f"\n[attention support] {impl}: {ran} shapes ran forward + backward, {len(refused)} refused: {refused}")
    if impl == "folded":
        assert (1024, 16, 64, True, "none") in refused and (1024, 16, 64, False, "none") not in refused
