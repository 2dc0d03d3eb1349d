"""The refusals of the 24 launching draw entries of a rollout step (6 sample, 6 policy, 6 + 6 step kernel), through the C ABI.  A
refused call returns the code of the tables below -- literals, read off include/etm_hip.h and the entries' checks, not asked of the
library -- and launches nothing: every output buffer keeps its sentinel.

Sample and policy entries: one accepted call each at W = 2, A = 3 (sizes (2, 1) when branched), hid = 4, S = 2, then every defect the
entry's header comment names, one at a time, and pairs of defects that fix which refusal wins.

Step entries: refused calls only (the value tests own the accepted paths), on the smallest admitted shapes -- D = 128, H = 1, L = 32,
nb = 1, hid = 128, A = 3, W = 1, with gtrxl = 1 for the group form --, every call built from a complete operand set: real buffers
sized for the largest A a defective call names (64), zero-filled index / window / slot tables, a valid block-pointer table, zeroed
scratch.  An entry that wrongly accepted a defective call would compute rubbish inside these buffers and read nothing outside them.
The order of the checks, hence the code of a pair: the mandatory mask (masked entries) or the Box table (Gaussian entries: A <= 0
ETM_EINVAL, A > 8 ETM_EUNSUPPORTED) first; st_means / st_logps; the window operands; the mandatory pointers; the shape integers
(a bad branch table makes A = 0 here); flag without actions; the mask's alignment, then its 63 columns; the tail; h_splits; the
shape predicate (ETM_EUNSUPPORTED); the scratch size (ETM_EWORKSPACE); the block-pointer table."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -7.25, -7
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -3
VARIANTS = ("", "_branched", "_branched_masked", "_branched_logps", "_gaussian", "_gaussian_means")


def _family(stem):
    return tuple(f"etm_rollout_{stem}{v}" for v in VARIANTS)


SAMPLE, POLICY, WORKER, GROUP = _family("sample"), _family("policy"), _family("trxl"), _family("trxl_group")
DRAW, STEP = SAMPLE + POLICY, WORKER + GROUP


def _of(entries, *suffixes):
    return tuple(e for e in entries if e.endswith(suffixes))


def _is(entry):
    box = "_gaussian" in entry
    return dict(box=box, branched="_branched" in entry, masked=entry.endswith("_masked"), logps=entry.endswith("_logps"),
                means=entry.endswith("_means"), plain=not box and "_branched" not in entry)


W_DRAW, A, SIZES, HID_DRAW, S = 2, 3, (2, 1), 4, 2
A_MAX = 64                                       # the largest number of columns a defective call names
D, H, L, NB, HID, W_STEP, T, SLOTS = 128, 1, 32, 1, 128, 1, 40, 2
D_BAD = 126                                      # no multiple of 4: neither form of the step kernel takes it, and every buffer covers it

STEP_HEAD = ["h_in", "wemb_t", "bemb", "blocks", "nb", "kv", "kv_worker_stride", "kv_row_stride", "win", "mask", "items", "wh_t", "bh",
             "wp", "bp", "wv", "bv"]
STEP_MIDDLE = ["host_actions", "host_flag", "sync_counter", "ln_eps", "scratch", "scratch_bytes", "wkv", "pos", "step_l", "slot_l", "bank",
               "bank_slot_stride", "bank_row_stride", "bank_block_stride", "h_bias", "h_splits", "ss", "mask_table", "index_table", "st_mask",
               "st_idx", "latch", "t_row", "mask_t", "win_t", "kv_init", "T", "pre_ln", "gtrxl", "W", "D", "H", "L", "hid"]
OPTIONAL = {"forced", "h_bias", "host_actions", "host_flag", "action_mask", "st_logps", "st_means", "low", "high", "branch_sizes", "stream",
            "wkv", "pos", "step_l", "slot_l", "bank", "ss", "mask_table", "index_table", "st_mask", "st_idx", "latch", "t_row", "mask_t", "win_t",
            "kv_init", "win", "mask"}
POINTERS = {"logits", "mean", "value", "h", "wp", "bp", "wv", "bv", "log_std", "normals", "uniforms", "t_dev", "actions", "st_actions", "st_logp",
            "st_values", "sync_counter", "h_in", "wemb_t", "bemb", "blocks", "kv", "items", "wh_t", "bh", "scratch"}


def _order(entry):
    """The entry's argument names in the order of its declaration in include/etm_hip.h."""
    k = _is(entry)
    draw = (["log_std", "normals"] if k["box"] else ["uniforms"]) + ["forced", "t_dev", "actions", "st_actions", "st_logp", "st_values"]
    if entry in SAMPLE:
        order = ["mean" if k["box"] else "logits", "value"] + draw
        order += ["low", "high", "W", "A"] if k["box"] else ["W", "branch_sizes", "n_branches"] if k["branched"] else ["W", "A"]
    elif entry in POLICY:
        order = ["h", "h_bias", "wp", "bp", "wv", "bv"] + draw + ["host_actions", "host_flag", "sync_counter"]
        order += (["low", "high", "W", "A", "hid", "stage_W"] if k["box"] else
                  ["W", "hid", "stage_W", "branch_sizes", "n_branches"] if k["branched"] else ["W", "A", "hid", "stage_W"])
    else:
        order = STEP_HEAD + draw + STEP_MIDDLE
        order += ["A", "stage_W", "low", "high"] if k["box"] else ["stage_W", "branch_sizes", "n_branches"] if k["branched"] else ["A", "stage_W"]
    return order + ["action_mask"] * (k["masked"] or k["logps"]) + ["st_logps"] * k["logps"] + ["st_means"] * k["means"] + ["stream"]


def _mandatory(entry):
    return [n for n in _order(entry) if n in POINTERS and n not in OPTIONAL]


def null(*names):
    return {n: None for n in names}


def off2(name):
    return {name: ("+2", name)}


FLAG_ALONE = dict(host_flag=("use", "host_flag_buf"))
COLUMNS_64 = dict(sizes=(32, 32))
BAD_SIZES = (("NULL branch_sizes", dict(sizes=None)), ("a branch of size 0", dict(sizes=(2, 0, 1))), ("17 branches", dict(sizes=(1,) * 17)))

# (defect, overrides of the good call's named arguments, the entries it is tried on, the code) -- one defect per row unless it says "+"
DRAW_DEFECTS = [
    ("NULL st_logps", null("st_logps"), _of(DRAW, "_logps"), EINVAL),
    ("st_logps off by 2 bytes", off2("st_logps"), _of(DRAW, "_logps"), EINVAL),
    ("NULL st_means", null("st_means"), _of(DRAW, "_means"), EINVAL),
    ("st_means off by 2 bytes", off2("st_means"), _of(DRAW, "_means"), EINVAL),
    ("NULL mandatory action_mask", null("action_mask"), _of(DRAW, "_masked"), EINVAL),
    ("NULL optional action_mask", null("action_mask"), _of(DRAW, "_logps"), OK),
    ("action_mask off by 2 bytes", off2("action_mask"), _of(DRAW, "_masked", "_logps"), EINVAL),
    ("host_flag without host_actions", FLAG_ALONE, POLICY, EINVAL),
    ("stage_W < W", dict(stage_W=W_DRAW - 1), POLICY, EINVAL),
    ("W 0", dict(W=0), DRAW, EINVAL),
    ("W -1", dict(W=-1), DRAW, EINVAL),
    ("A 0", dict(A=0), (SAMPLE[0], POLICY[0]), EINVAL),
    ("hid 0", dict(hid=0), POLICY, EINVAL),
    ("64 mask columns", COLUMNS_64, _of(DRAW, "_masked", "_logps"), EUNSUPPORTED),
    ("Box A 0", dict(A=0), _of(DRAW, "_gaussian", "_means"), EINVAL),
    ("Box A 9", dict(A=9), _of(DRAW, "_gaussian", "_means"), EUNSUPPORTED),
    # ---- two defects at once
    ("action_mask off by 2 bytes + 64 mask columns", dict(COLUMNS_64, **off2("action_mask")), _of(DRAW, "_masked", "_logps"), EINVAL),
    ("NULL t_dev + 64 mask columns", dict(COLUMNS_64, t_dev=None), _of(DRAW, "_masked", "_logps"), EINVAL),
    ("NULL st_logps + 64 mask columns", dict(COLUMNS_64, st_logps=None), _of(DRAW, "_logps"), EINVAL),
    ("stage_W < W + 64 mask columns", dict(COLUMNS_64, stage_W=W_DRAW - 1), _of(POLICY, "_masked", "_logps"), EINVAL),
    ("NULL st_means + Box A 9", dict(A=9, st_means=None), _of(DRAW, "_means"), EINVAL),
    ("NULL t_dev + Box A 9", dict(A=9, t_dev=None), _of(DRAW, "_gaussian", "_means"), EINVAL),
    ("host_flag without host_actions + Box A 9", dict(FLAG_ALONE, A=9), _of(POLICY, "_gaussian", "_means"), EINVAL),
]
DRAW_DEFECTS += [(what, over, tuple(e for e in DRAW if "_branched" in e), EINVAL) for what, over in BAD_SIZES]
DRAW_DEFECTS += [(f"NULL {n}", null(n), (e,), EINVAL) for e in DRAW for n in _mandatory(e)]

UNSUPPORTED_D = dict(D=D_BAD)
STEP_BRANCHED, STEP_BOX = tuple(e for e in STEP if "_branched" in e), _of(STEP, "_gaussian", "_means")
STEP_MASK = _of(STEP, "_masked", "_logps")
STEP_DEFECTS = [
    # ---- the first checks
    ("NULL st_means", null("st_means"), _of(STEP, "_means"), EINVAL),
    ("st_means off by 2 bytes", off2("st_means"), _of(STEP, "_means"), EINVAL),
    ("NULL st_logps", null("st_logps"), _of(STEP, "_logps"), EINVAL),
    ("st_logps off by 2 bytes", off2("st_logps"), _of(STEP, "_logps"), EINVAL),
    ("NULL mandatory action_mask", null("action_mask"), _of(STEP, "_masked"), EINVAL),
    ("action_mask off by 2 bytes", off2("action_mask"), STEP_MASK, EINVAL),
    ("64 mask columns", COLUMNS_64, STEP_MASK, EUNSUPPORTED),
    # ---- the window operands
    ("ss with T 0", dict(T=0), STEP, EINVAL),
    ("neither ss nor win", null("ss", "win"), STEP, EINVAL),
    ("neither ss nor mask", null("ss", "mask"), STEP, EINVAL),
    # ---- the shape integers
    ("W 0", dict(W=0), STEP, EINVAL),
    ("nb 0", dict(nb=0), STEP, EINVAL),
    ("D 0", dict(D=0), STEP, EINVAL),
    ("H 0", dict(H=0), STEP, EINVAL),
    ("L 0", dict(L=0), STEP, EINVAL),
    ("hid 0", dict(hid=0), STEP, EINVAL),
    ("A 0", dict(A=0), (WORKER[0], GROUP[0]) + STEP_BOX, EINVAL),
    ("stage_W < W", dict(stage_W=W_STEP - 1), STEP, EINVAL),
    ("D % H != 0", dict(H=3), STEP, EINVAL),
    ("host_flag without host_actions", FLAG_ALONE, STEP, EINVAL),
    # ---- tail, h_splits, shape predicate, scratch, block table
    ("tail without step_l", null("step_l"), STEP, EINVAL),
    ("tail without slot_l", null("slot_l"), STEP, EINVAL),
    ("tail without bank", null("bank"), STEP, EINVAL),
    ("h_splits -1", dict(h_splits=-1), STEP, EINVAL),
    ("h_splits 65", dict(h_splits=65), STEP, EINVAL),
    ("h_splits 1 without h_bias", dict(h_splits=1, h_bias=None), STEP, EINVAL),
    ("unsupported D", UNSUPPORTED_D, STEP, EUNSUPPORTED),
    ("group form without gates", dict(gtrxl=0), GROUP, EUNSUPPORTED),
    ("scratch one byte short", dict(short=1), STEP, EWORKSPACE),
    ("NULL block pointer 4", dict(block={4: None}), STEP, EINVAL),
    ("NULL gate pointer 12 with gtrxl", dict(gtrxl=1, block={12: None}), STEP, EINVAL),
    ("norm_kv gain without bias", dict(block={18: None}), STEP, EINVAL),
    ("norm_kv bias without gain", dict(block={17: None}), STEP, EINVAL),
    ("Box A 9", dict(A=9), STEP_BOX, EUNSUPPORTED),
    # ---- two defects at once
    ("NULL st_logps + unsupported D", dict(UNSUPPORTED_D, st_logps=None), _of(STEP, "_logps"), EINVAL),
    ("NULL st_means + unsupported D", dict(UNSUPPORTED_D, st_means=None), _of(STEP, "_means"), EINVAL),
    ("NULL mandatory action_mask + unsupported D", dict(UNSUPPORTED_D, action_mask=None), _of(STEP, "_masked"), EINVAL),
    ("action_mask off by 2 bytes + unsupported D", dict(UNSUPPORTED_D, **off2("action_mask")), STEP_MASK, EINVAL),
    ("NULL h_in + unsupported D", dict(UNSUPPORTED_D, h_in=None), STEP, EINVAL),
    ("tail without bank + unsupported D", dict(UNSUPPORTED_D, bank=None), STEP, EINVAL),
    ("h_splits 65 + unsupported D", dict(UNSUPPORTED_D, h_splits=65), STEP, EINVAL),
    ("unsupported D + scratch one byte short", dict(UNSUPPORTED_D, short=1), STEP, EUNSUPPORTED),
    ("scratch one byte short + NULL block pointer 4", dict(short=1, block={4: None}), STEP, EWORKSPACE),
    ("scratch one byte short + NULL branch_sizes", dict(short=1, sizes=None), STEP_BRANCHED, EINVAL),
    ("NULL block pointer 4 + NULL branch_sizes", dict(block={4: None}, sizes=None), STEP_BRANCHED, EINVAL),
    ("Box A 9 + NULL h_in", dict(A=9, h_in=None), STEP_BOX, EUNSUPPORTED),
    ("Box A 9 + NULL st_means", dict(A=9, st_means=None), _of(STEP, "_means"), EUNSUPPORTED),
    ("Box A 0 + scratch one byte short", dict(A=0, short=1), STEP_BOX, EINVAL),
]
STEP_DEFECTS += [(f"ss without {n}", null(n), STEP, EINVAL) for n in ("mask_table", "index_table", "st_mask", "st_idx", "latch", "mask_t", "win_t")]
STEP_DEFECTS += [(what, over, STEP_BRANCHED, EINVAL) for what, over in BAD_SIZES]
STEP_DEFECTS += [(f"NULL {n}", null(n), (e,), EINVAL) for e in STEP for n in _mandatory(e)]


def _dev():
    return torch.device("cuda", 0)


def _pinned(t):
    return t.pin_memory()


def _lib():
    from etm import lib
    return lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _zeros(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device=_dev())


def _full(n, dtype=torch.float32):
    return torch.full((n,), SENTINEL if dtype == torch.float32 else ISENTINEL if dtype == torch.int64 else 0xA5, dtype=dtype, device=_dev())


def _draw_inputs():
    """The operands the sample and policy calls read."""
    g = torch.Generator().manual_seed(5)
    rnd = lambda n: (torch.randn(n, generator=g) * 0.5).to(_dev())
    return dict(logits=rnd(W_DRAW * A_MAX), mean=rnd(W_DRAW * A_MAX), value=rnd(W_DRAW), h=rnd(W_DRAW * 2 * HID_DRAW), wp=rnd(A_MAX * HID_DRAW),
                bp=rnd(A_MAX), wv=rnd(HID_DRAW), bv=rnd(1), log_std=_zeros(A_MAX), normals=_zeros(S * W_DRAW * A_MAX),
                uniforms=torch.full((S * W_DRAW * A_MAX,), 0.5, device=_dev()),
                action_mask=torch.full((W_DRAW,), (1 << 62) - 1, dtype=torch.int64, device=_dev()))


def _step_inputs():
    """The operands the step calls would read: weights (every block pointer the same buffer, as long as the longest matrix), zero-filled
    index / window / slot tables."""
    g = torch.Generator().manual_seed(7)
    rnd = lambda n: (torch.randn(n, generator=g) * 0.05).to(_dev())
    i64 = lambda n: _zeros(n, torch.int64)
    weights = rnd(3 * D * D + 3 * D)
    return dict(h_in=rnd(W_STEP * D), wemb_t=rnd(D * D), bemb=rnd(D), weights=weights, wh_t=rnd(D * 2 * HID), bh=rnd(2 * HID), wp=rnd(A_MAX * HID),
                bp=rnd(A_MAX), wv=rnd(HID), bv=rnd(1), log_std=_zeros(A_MAX), normals=_zeros(S * W_STEP * A_MAX),
                uniforms=torch.full((S * W_STEP * A_MAX,), 0.5, device=_dev()), win=i64(W_STEP * L), mask=_zeros(W_STEP * L, torch.uint8),
                wkv=rnd(NB * D * 2 * D), pos=rnd(T * D), step_l=i64(W_STEP), slot_l=i64(W_STEP), h_bias=rnd(D), ss=i64(2 * W_STEP),
                mask_table=_zeros(L * L, torch.uint8), index_table=i64(T * L), kv_init=_zeros(T * NB * 2 * D),
                action_mask=torch.full((W_STEP,), (1 << 62) - 1, dtype=torch.int64, device=_dev()))


@pytest.fixture(scope="module")
def draw_inputs():
    return _draw_inputs()         # shared and left unchanged


@pytest.fixture(scope="module")
def step_inputs():
    return _step_inputs()


def _draw_outputs():
    n = S * W_DRAW * A_MAX
    return dict(t_dev=_zeros(1, torch.int64), actions_i=_full(W_DRAW * A_MAX, torch.int64), actions_f=_full(W_DRAW * A_MAX),
                st_actions_i=_full(n, torch.int64), st_actions_f=_full(n), st_logp=_full(n), st_values=_full(S * W_DRAW), st_logps=_full(n),
                st_means=_full(n), sync_counter=_zeros(1, torch.int32),
                host_flag_buf=_pinned(torch.full((1,), ISENTINEL, dtype=torch.int64)))


def _step_outputs(lib):
    n = S * W_STEP * A_MAX
    scratch_bytes = max(lib.etm_rollout_trxl_scratch_bytes(W_STEP, D, H, NB), lib.etm_rollout_trxl_group_scratch_bytes(NB))
    return dict(_draw_outputs(), actions_i=_full(W_STEP * A_MAX, torch.int64), actions_f=_full(W_STEP * A_MAX), st_actions_i=_full(n, torch.int64),
                st_actions_f=_full(n), st_logp=_full(n), st_values=_full(S * W_STEP), st_logps=_full(n), st_means=_full(n),
                items=_full(NB * W_STEP * D), kv=_full(W_STEP * T * NB * 2 * D), bank=_full(SLOTS * T * NB * D),
                st_mask=_full(S * W_STEP * L, torch.uint8), st_idx=_full(S * W_STEP * L, torch.int64), latch=_full(2 * W_STEP, torch.int64),
                t_row=_full(1, torch.int64), mask_t=_full(W_STEP * L, torch.uint8), win_t=_full(W_STEP * L, torch.int64),
                scratch=_zeros((scratch_bytes + 7) // 8, torch.int64))


def _snapshot(out):
    return {k: t.clone() for k, t in out.items()}


def _untouched(out, before):
    return [k for k, t in out.items() if not torch.equal(t, before[k])]


def _call(lib, entry, inp, out, over):
    """The entry with the good call's arguments, `over` replacing some by name; -> the return code."""
    over = dict(over)
    k = _is(entry)
    step = entry in STEP
    short, block = over.pop("short", 0), over.pop("block", {})
    sizes = over.pop("sizes", SIZES)
    kind = "_f" if k["box"] else "_i"
    a = dict(inp, **out)
    a.update(actions=out["actions" + kind], st_actions=out["st_actions" + kind], forced=None, host_actions=None, host_flag=None, h_bias=None,
             low=None, high=None, stream=_stream(), A=A, W=W_DRAW, hid=HID_DRAW, stage_W=W_DRAW,
             branch_sizes=None if sizes is None else (ctypes.c_int32 * len(sizes))(*sizes), n_branches=len(SIZES if sizes is None else sizes))
    if step:
        group = entry in GROUP
        ptrs = [inp["weights"].data_ptr()] * 19
        for i, v in block.items():
            ptrs[i] = v
        whole = lib.etm_rollout_trxl_group_scratch_bytes(NB) if group else lib.etm_rollout_trxl_scratch_bytes(W_STEP, D, H, NB)
        assert 0 < whole <= out["scratch"].numel() * 8
        a.update(blocks=(ctypes.c_void_p * 19)(*ptrs), nb=NB, kv_worker_stride=T * NB * 2 * D, kv_row_stride=NB * 2 * D, ln_eps=1e-5,
                 scratch_bytes=whole - short, bank_slot_stride=T * NB * D, bank_row_stride=NB * D, bank_block_stride=D, h_bias=inp["h_bias"],
                 h_splits=0, T=T, pre_ln=0, gtrxl=int(group), W=W_STEP, D=D, H=H, L=L, hid=HID, stage_W=W_STEP)
    else:
        assert not block and not short
    order = _order(entry)
    for name, v in over.items():
        assert name in order, (entry, name)
        a[name] = (a[v[1]].data_ptr() + 2 if v[0] == "+2" else a[v[1]]) if isinstance(v, tuple) else v
    ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v
    rc = getattr(lib, entry)(*[ptr(a[name]) for name in order])
    torch.cuda.synchronize()
    return rc


def test_the_tables_cover_every_entry():
    assert len(set(DRAW)) == 12 and len(set(STEP)) == 12
    for table, entries in ((DRAW_DEFECTS, DRAW), (STEP_DEFECTS, STEP)):
        assert all(code in (OK, EINVAL, EUNSUPPORTED, EWORKSPACE) and set(es) <= set(entries) and es for _, _, es, code in table)
        for entry in entries:
            names = {d[0] for d in table if entry in d[2]}
            assert "W 0" in names and len([n for n in names if n.startswith("NULL")]) >= 8, entry
    assert all(code != OK for _, _, _, code in STEP_DEFECTS), "the refusal test launches no step kernel"
    for entry in STEP:
        names = {d[0] for d in STEP_DEFECTS if entry in d[2]}
        assert {"scratch one byte short", "unsupported D", "NULL block pointer 4"} <= names, entry


def test_the_step_shapes_are_admitted():
    lib = _lib()
    tab = (ctypes.c_int32 * len(SIZES))(*SIZES)
    assert sum(SIZES) == A
    assert lib.etm_rollout_trxl_supported(D, H, L, HID, A, NB) == 1
    assert lib.etm_rollout_trxl_supported_branched(D, H, L, HID, tab, len(SIZES), NB) == 1
    assert lib.etm_rollout_trxl_supported_gaussian(D, H, L, HID, A, NB) == 1
    assert lib.etm_rollout_trxl_group_supported(D, H, L, HID, A, NB, W_STEP, 1) == 1
    assert lib.etm_rollout_trxl_group_supported_branched(D, H, L, HID, tab, len(SIZES), NB, W_STEP, 1) == 1
    assert lib.etm_rollout_trxl_group_supported_gaussian(D, H, L, HID, A, NB, W_STEP, 1) == 1
    assert 0 < lib.etm_rollout_trxl_grid(W_STEP, H) <= 256 and lib.etm_rollout_trxl_team(H) == 1
    assert lib.etm_rollout_trxl_supported(D_BAD, H, L, HID, A, NB) == 0 and lib.etm_rollout_trxl_group_supported(D_BAD, H, L, HID, A, NB, W_STEP, 1) == 0
    assert lib.etm_rollout_trxl_scratch_bytes(W_STEP, D, H, NB) > 0 and lib.etm_rollout_trxl_group_scratch_bytes(NB) > 0


def _accepted(out, before, entry):
    """An accepted sample / policy call advanced the step counter and staged row 0 of its tables."""
    k = _is(entry)
    assert int(out["t_dev"]) == 1, entry
    assert bool(torch.isfinite(out["st_values"][:W_DRAW]).all()) and not bool((out["st_values"][:W_DRAW] == SENTINEL).any()), entry
    assert bool(torch.equal(out["st_values"][W_DRAW:], before["st_values"][W_DRAW:])), entry
    if k["logps"]:
        assert not bool((out["st_logps"][:W_DRAW * A] == SENTINEL).any()), entry
    if k["means"]:
        assert not bool((out["st_means"][:W_DRAW * A] == SENTINEL).any()), entry


@pytest.mark.parametrize("entry", DRAW)
def test_good_sample_and_policy_calls_are_accepted(draw_inputs, entry):
    out = _draw_outputs()
    before = _snapshot(out)
    assert _call(_lib(), entry, draw_inputs, out, {}) == OK
    _accepted(out, before, entry)


@pytest.mark.parametrize("entry", DRAW)
def test_defective_sample_and_policy_calls_return_the_tables_code_and_write_nothing(draw_inputs, entry):
    lib = _lib()
    rows = [d for d in DRAW_DEFECTS if entry in d[2]]
    assert rows
    for what, over, _, code in rows:
        out = _draw_outputs()
        before = _snapshot(out)
        rc = _call(lib, entry, draw_inputs, out, over)
        assert rc == code, (entry, what, rc, code)
        if code == OK:
            _accepted(out, before, entry)
        else:
            assert _untouched(out, before) == [], (entry, what)


@pytest.mark.parametrize("entry", STEP)
def test_defective_step_calls_return_the_tables_code_and_write_nothing(step_inputs, entry):
    lib = _lib()
    rows = [d for d in STEP_DEFECTS if entry in d[2]]
    assert rows
    out = _step_outputs(lib)
    before = _snapshot(out)
    for what, over, _, code in rows:
        rc = _call(lib, entry, step_inputs, out, over)
        assert rc == code, (entry, what, rc, code)
        assert _untouched(out, before) == [], (entry, what)
