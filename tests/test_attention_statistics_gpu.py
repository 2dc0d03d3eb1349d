"""-m gpu: etm_attn_stats (csrc/attn_stats.hip) through the C ABI against the float64 reference on the same fp32 inputs
(tests/attention_statistics_reference.py), and ops.attn_stats on what ops.mha itself returns.

Bounds.  Words 0 .. 3 (counts): equal.  Histogram words and word 6 are double sums of fp32 values: rtol 1e-11, and exactly 0 where the
reference is 0 (the words beyond L among them).  Words 4 and 5: the absolute bound ``entropy_bound`` of the reference module -- derived
there from logf's and the fp32 row sum's rounding, not measured.  That the bounds are not vacuous is checked per case: the reference
with every age shifted by one, and with the two lane halves exchanged, each miss the reference by more than 100 x the bound."""
import numpy as np
import pytest
import torch

import attention_statistics_reference as ar

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1), (7, 3, 2), (257, 4, 31), (5, 1, 32), (64, 3, 33), (257, 2, 63), (9, 4, 64), (1031, 3, 65), (33, 1, 127), (257, 4, 128)]
EINVAL = -1
SENTINEL = -12345.6789


def _dev():
    return torch.device("cuda", 0)


def _to(x):
    return torch.from_numpy(np.array(x)).to(_dev())             # (a copy: the shared inputs are read-only)


def _lib():
    from etm import lib
    return lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_inputs = {}


def _case(shape):
    """(att, mask, reference table) of a case, computed once and never written."""
    if shape not in _inputs:
        att, mask = ar.attention_statistics_inputs(*shape, seed=17 + sum(shape))
        ref = ar.attention_statistics_reference(att, mask)
        for a in (att, mask, ref):
            a.setflags(write=False)
        _inputs[shape] = (att, mask, ref)
    return _inputs[shape]


def _call(att_d, mask_d, table_d, ws_d, N, H, L, ws_bytes=None):
    rc = _lib().etm_attn_stats(att_d.data_ptr(), mask_d.data_ptr(), table_d.data_ptr(), ws_d.data_ptr(),
                               ws_d.numel() if ws_bytes is None else ws_bytes, N, H, L, _stream())
    torch.cuda.synchronize()
    return rc


def _run(shape, calls=1, heads_beside=0):
    """The table after ``calls`` calls on a zeroed table of H (+ heads_beside sentinel) heads, and the workspace's bytes."""
    N, H, L = shape
    att, mask, _ = _case(shape)
    table = torch.zeros((H + heads_beside, ar.WORDS), dtype=torch.float64, device=_dev())
    table[H:] = SENTINEL
    ws = torch.zeros(int(_lib().etm_attn_stats_workspace_bytes(N, H, L)), dtype=torch.uint8, device=_dev())
    att_d, mask_d = _to(att), _to(mask)
    for _ in range(calls):
        assert _call(att_d, mask_d, table, ws, N, H, L) == 0
    return table.cpu().numpy(), ws.cpu().numpy()


def _check_table(got, ref, L, tag):
    """``got`` [H, 264] against the reference, each figure printed before it is asserted on."""
    assert np.array_equal(got[:, :4], ref[:, :4]), (tag, got[:, :4], ref[:, :4])
    exact = np.r_[6, ar.AGE0: ar.WORDS]
    zero = ref[:, exact] == 0
    rel = np.abs(got[:, exact] - ref[:, exact])[~zero] / np.abs(ref[:, exact])[~zero]
    bound = np.array([ar.entropy_bound(r, L) for r in ref[:, 0]])
    err4, err5 = np.abs(got[:, 4] - ref[:, 4]), np.abs(got[:, 5] - ref[:, 5])
    print(f"\n[attention statistics] {tag}: histogram / max rel {rel.max() if rel.size else 0.0:.3g} (1e-11); entropy err "
          f"{err4.max():.3g}, normalised {err5.max():.3g} (bound {bound.min():.3g})", flush=True)
    assert (got[:, exact][zero] == 0).all(), tag
    assert (got[:, 7] == 0).all(), tag
    assert (rel <= 1e-11).all(), (tag, rel.max())
    assert (err4 <= bound).all() and (err5 <= bound).all(), (tag, err4, err5, bound)


@pytest.mark.parametrize("shape", CASES, ids=str)
def test_table_against_float64(shape):
    N, H, L = shape
    _, _, ref = _case(shape)
    got, _ = _run(shape)
    _check_table(got, ref, L, f"N={N} H={H} L={L}")


@pytest.mark.parametrize("shape", [c for c in CASES if c[2] >= 2], ids=str)
def test_bounds_are_not_vacuous(shape):
    N, H, L = shape
    att, mask, ref = _case(shape)
    v, counted, empty, _ = ar.row_classes(mask)
    assert empty.any() and (counted & (v == 1)).any() and (counted & (v == L)).any()
    bound = max(ar.entropy_bound(r, L) for r in ref[:, 0])
    for kw in ({"age_shift": 1}, {"swap_halves": True}):
        wrong = ar.attention_statistics_reference(att, mask, **kw)
        assert np.abs(wrong - ref).max() > 100 * bound, (kw, np.abs(wrong - ref).max(), bound)
        assert (np.abs(wrong - ref) > 1e-11 * np.abs(ref)).any()


@pytest.mark.parametrize("shape", [(7, 3, 2), (257, 4, 31), (1031, 3, 65), (257, 4, 128)], ids=str)
def test_call_adds_and_leaves_the_next_heads_alone(shape):
    H = shape[1]
    once, _ = _run(shape, calls=1, heads_beside=H)
    twice, _ = _run(shape, calls=2, heads_beside=H)
    assert np.allclose(twice[:H], 2 * once[:H], rtol=1e-11, atol=0.0)
    assert np.array_equal(twice[:H, :4], 2 * once[:H, :4])
    assert (once[H:] == SENTINEL).all() and (twice[H:] == SENTINEL).all()


@pytest.mark.parametrize("shape", [(257, 4, 31), (1031, 3, 65), (257, 4, 128)], ids=str)
def test_equal_state_gives_equal_bytes(shape):
    (t0, w0), (t1, w1) = _run(shape, calls=2), _run(shape, calls=2)
    assert np.array_equal(t0.view(np.uint64), t1.view(np.uint64)) and np.array_equal(w0, w1)


def test_refusals_launch_nothing():
    lib = _lib()
    N, H, L = 40, 2, 16
    att, mask = ar.attention_statistics_inputs(N, H, L, seed=5)
    att_d, mask_d = _to(att), _to(mask)
    need = int(lib.etm_attn_stats_workspace_bytes(N, H, L))
    assert need == H * ar.WORDS * 8
    table = torch.full((H * ar.WORDS + 1,), SENTINEL, dtype=torch.float64, device=_dev())
    ws = torch.full((need + 8,), 0x5A, dtype=torch.uint8, device=_dev())
    a, m, t, w, s = att_d.data_ptr(), mask_d.data_ptr(), table.data_ptr(), ws.data_ptr(), _stream()
    assert t % 8 == 0 and w % 8 == 0
    bad = {"null att": (None, m, t, w, need, N, H, L), "null mask": (a, None, t, w, need, N, H, L),
           "null table": (a, m, None, w, need, N, H, L), "null workspace": (a, m, t, None, need, N, H, L),
           "N = 0": (a, m, t, w, need, 0, H, L), "N < 0": (a, m, t, w, need, -1, H, L),
           "H = 0": (a, m, t, w, need, N, 0, L), "H = 33": (a, m, t, w, need + 8, N, 33, L),
           "L = 0": (a, m, t, w, need, N, H, 0), "L = 129": (a, m, t, w, need, N, H, 129),
           "table misaligned": (a, m, t + 4, w, need, N, H, L), "workspace misaligned": (a, m, t, w + 4, need, N, H, L),
           "workspace short": (a, m, t, w, need - 1, N, H, L), "workspace empty": (a, m, t, w, 0, N, H, L)}
    for name, args in bad.items():
        assert lib.etm_attn_stats(*args, s) == EINVAL, name
    for shape in ((0, H, L), (N, 0, L), (N, 33, L), (N, H, 0), (N, H, 129)):
        assert lib.etm_attn_stats_workspace_bytes(*shape) == 0, shape
    torch.cuda.synchronize()
    assert (table == SENTINEL).all().item() and (ws == 0x5A).all().item()
    assert lib.etm_attn_stats(a, m, t, w, need, N, H, L, s) == 0          # the same operands, accepted
    torch.cuda.synchronize()
    assert (table[: H * ar.WORDS] != SENTINEL).any().item() and table[H * ar.WORDS].item() == SENTINEL and (ws[need:] == 0x5A).all().item()


def test_checked_call_refuses_wrong_operands():
    from etm import ops
    N, H, L = 6, 2, 8
    att, mask = ar.attention_statistics_inputs(N, H, L, seed=6)
    att_d, mask_d = _to(att), _to(mask)
    table = torch.zeros((H, ar.WORDS), dtype=torch.float64, device=_dev())
    ws = torch.empty(int(_lib().etm_attn_stats_workspace_bytes(N, H, L)), dtype=torch.uint8, device=_dev())
    with pytest.raises(TypeError):
        ops.attn_stats(att_d.double(), mask_d, table, ws)
    with pytest.raises(TypeError):
        ops.attn_stats(att_d.transpose(0, 1), mask_d, table, ws)
    with pytest.raises(TypeError):
        ops.attn_stats(att_d, mask_d.bool(), table, ws)
    with pytest.raises(TypeError):
        ops.attn_stats(att_d, mask_d, table.float(), ws)
    with pytest.raises(TypeError):
        ops.attn_stats(att_d, mask_d, table[:1], ws)
    with pytest.raises(TypeError):
        ops.attn_stats(att_d, mask_d, table, ws[:-1])
    with pytest.raises(RuntimeError):
        ops.attn_stats(att_d.cpu(), mask_d, table, ws)
    torch.cuda.synchronize()
    assert (table == 0).all().item()
    ops.attn_stats(att_d, mask_d, table, ws)
    _check_table(table.cpu().numpy(), ar.attention_statistics_reference(att, mask), L, "ops.attn_stats")


def test_owner_class_holds_fixed_addresses():
    from etm import ops
    st = ops.AttentionStatistics(2, 3, 300, 16, _dev())
    assert tuple(st.table.shape) == (2, 3, ar.WORDS) and st.table.dtype == torch.float64
    assert st.workspace.numel() == _lib().etm_attn_stats_workspace_bytes(300, 3, 16)
    ptrs = (st.table.data_ptr(), st.workspace.data_ptr())
    att, mask = ar.attention_statistics_inputs(300, 3, 16, seed=8)
    ops.attn_stats(_to(att), _to(mask), st.table[1], st.workspace)
    got = st.read()
    assert isinstance(got, np.ndarray) and got.shape == (2, 3, ar.WORDS) and (got[0] == 0).all()
    _check_table(got[1], ar.attention_statistics_reference(att, mask), 16, "owner")
    st.reset()
    assert (st.read() == 0).all() and ptrs == (st.table.data_ptr(), st.workspace.data_ptr())
    for bad in ((0, 3, 300, 16), (2, 33, 300, 16), (2, 3, 0, 16), (2, 3, 300, 129)):
        with pytest.raises(ValueError):
            ops.AttentionStatistics(*bad, _dev())


def test_statistics_of_what_mha_returns():
    """Both attention implementations the project selects between, on a small bank: the table of the att and mask ``ops.mha`` itself
    hands back equals the reference computed from that att."""
    from etm import ops
    dev = _dev()
    N, L, D, H, T, nb = 37, 16, 64, 2, 24, 2
    g = torch.Generator().manual_seed(1)
    bank = torch.randn((3, T, nb, D), generator=g)
    ep = torch.randint(0, 3, (N,), generator=g)
    win = (torch.randint(0, T - L + 1, (N,), generator=g)[:, None] + torch.arange(L)[None, :]).long()
    v = torch.randint(0, L + 1, (N,), generator=g)
    v[:5] = torch.tensor([0, 1, 5, L - 1, L])
    mask = torch.arange(L)[None, :] < v[:, None]
    wk, wv = (torch.randn((D, D), generator=g) * 0.1).to(dev), (torch.randn((D, D), generator=g) * 0.1).to(dev)
    q = torch.randn((N, D), generator=g).to(dev)
    spec = ops.WindowSpec.from_bank(bank.to(dev), ep.to(dev), win.to(dev), None, mask.to(dev))
    assert len(ops.ATTENTION_IMPLS) >= 2
    for impl in ops.ATTENTION_IMPLS:
        _, att = ops.mha(q, wk, wv, spec, 1, H, impl=impl)
        assert att.dtype == torch.float32 and tuple(att.shape) == (N, H, L) and att.is_contiguous()
        table = torch.zeros((H, ar.WORDS), dtype=torch.float64, device=dev)
        ws = torch.empty(int(_lib().etm_attn_stats_workspace_bytes(N, H, L)), dtype=torch.uint8, device=dev)
        ops.attn_stats(att, spec.mask, table, ws)
        ref = ar.attention_statistics_reference(att.cpu().numpy(), spec.mask.cpu().numpy())
        got = table.cpu().numpy()
        _check_table(got, ref, L, f"mha {impl}")
        assert got[0, 2] == int((v == 0).sum()) and got[0, 3] == 0 and got[0, 0] == N - int((v == 0).sum())
        # the attention kernels' own fp32 softmax: a counted row's mass is 1 within their rounding
        assert np.allclose(got[:, ar.AGE0: ar.AGE0 + L].sum(axis=1), got[:, 0], atol=1e-4 * N)
