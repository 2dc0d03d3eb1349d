"""The refusals of the 15 launching loss entries (11 heads + loss, 4 PPO loss), through the C ABI: per entry one accepted call at the
smallest shapes, every defect its header comment names one at a time, and pairs of defects that fix which refusal wins.  A refused
call returns the code of the table below -- literals, read off include/etm_hip.h, not asked of the library -- and launches nothing:
every output buffer keeps its sentinel.

Shapes: heads + loss N = 9 (two workgroups of 8 samples, one of them partial), hid = 64, A = 8 (unbranched), sizes (3, 3) (branched),
A = 3 (Box); PPO loss N = 37, A = 5, the branch's bits and log-prob columns starting at 3.  The buffers are allocated for the largest
hid / A a defective call names, so that even an entry that wrongly accepted one would stay inside them."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
OK, EINVAL, EUNSUPPORTED, EWORKSPACE = 0, -1, -2, -3

H, HM, HB, HBM = "etm_heads_loss", "etm_heads_loss_masked", "etm_heads_loss_branched", "etm_heads_loss_branched_masked"
HK, HBK, HKP, HBKP = "etm_heads_loss_kl", "etm_heads_loss_branched_kl", "etm_heads_loss_kl_penalty", "etm_heads_loss_branched_kl_penalty"
HG, HGK, HGKP = "etm_heads_loss_gaussian", "etm_heads_loss_gaussian_kl", "etm_heads_loss_gaussian_kl_penalty"
P, PM, PK, PKP = "etm_ppo_loss", "etm_ppo_loss_masked", "etm_ppo_loss_kl", "etm_ppo_loss_kl_penalty"

UNBRANCHED, BRANCHED, BOX = (H, HM, HK, HKP), (HB, HBM, HBK, HBKP), (HG, HGK, HGKP)
CATEGORICAL = UNBRANCHED + BRANCHED
HEADS, PPO = CATEGORICAL + BOX, (P, PM, PK, PKP)
ENTRIES = HEADS + PPO

N_HEADS, HID, N_PPO, A_PPO, SHIFT = 9, 64, 37, 5, 3
HID_MAX, A_MAX, ROW_STRIDE = 576, 9, 16          # the largest a defective call names; the row stride of old_logps / old_mean / xact

HEADS_POINTERS = ("pre_p", "pre_v", "b_lp", "b_lv", "wb", "bb", "wv", "bv", "old_logp", "adv", "old_value", "adv_stats3", "gm_p", "gm_v",
                  "sums", "out8", "workspace")
PPO_POINTERS = ("logits", "actions", "old_logp", "adv", "adv_stats3", "out8", "d_logits", "partials")


def null(*names):
    return {n: None for n in names}


def off2(name):
    return {name: ("+2", name)}


# (defect, overrides of the good call's named arguments, the entries it is tried on, the code) -- one defect per row unless it says "+"
DEFECTS = [
    # ---- heads + loss: the entry-specific pointers
    ("NULL kl_coef", null("kl_coef"), (HKP, HBKP, HGKP), EINVAL),
    ("kl_coef off by 2 bytes", off2("kl_coef"), (HKP, HBKP, HGKP), EINVAL),
    ("NULL old_logps", null("old_logps"), (HK, HBK, HKP, HBKP), EINVAL),
    ("old_logps off by 2 bytes", off2("old_logps"), (HK, HBK, HKP, HBKP), EINVAL),
    ("NULL mandatory action_mask", null("action_mask"), (HM, HBM), EINVAL),
    ("NULL optional action_mask", null("action_mask"), (HK, HBK, HKP, HBKP), OK),
    ("action_mask off by 2 bytes", off2("action_mask"), (HM, HBM, HK, HBK, HKP, HBKP), EINVAL),
    ("NULL xact", null("xact"), BOX, EINVAL),
    ("NULL log_std", null("log_std"), BOX, EINVAL),
    ("NULL old_mean", null("old_mean"), (HGK, HGKP), EINVAL),
    ("old_mean off by 2 bytes", off2("old_mean"), (HGK, HGKP), EINVAL),
    ("NULL old_log_std", null("old_log_std"), (HGK, HGKP), EINVAL),
    ("old_log_std off by 2 bytes", off2("old_log_std"), (HGK, HGKP), EINVAL),
    ("NULL actions", null("actions"), CATEGORICAL, EINVAL),
    ("NULL branch_sizes", null("branch_sizes"), BRANCHED, EUNSUPPORTED),
    # ---- heads + loss: each stride one below its minimum
    ("old_logps_stride A - 1", dict(old_logps_stride=7), (HK, HKP), EINVAL),
    ("old_logps_stride sum(sizes) - 1", dict(old_logps_stride=5), (HBK, HBKP), EINVAL),
    ("action_stride n_branches - 1", dict(action_stride=1), BRANCHED, EINVAL),
    ("logp_stride n_branches - 1", dict(logp_stride=1), BRANCHED, EINVAL),
    ("action_stride A - 1", dict(action_stride=2), BOX, EINVAL),
    ("logp_stride 0", dict(logp_stride=0), BOX, EINVAL),
    ("old_mean_stride A - 1", dict(old_mean_stride=2), (HGK, HGKP), EINVAL),
    # ---- heads + loss: shapes
    ("hid 100", dict(hid=100), HEADS, EUNSUPPORTED),
    ("hid 576", dict(hid=576), HEADS, EUNSUPPORTED),
    ("A 9", dict(A=9), UNBRANCHED + BOX, EUNSUPPORTED),
    ("A 9", dict(sizes=(4, 5)), BRANCHED, EUNSUPPORTED),
    ("workspace one byte short", dict(short=1), HEADS, EWORKSPACE),
    # ---- heads + loss: two defects at once
    ("NULL old_logps + hid 100", dict(old_logps=None, hid=100), (HK, HBK, HKP, HBKP), EINVAL),
    ("NULL old_mean + hid 100", dict(old_mean=None, hid=100), (HGK, HGKP), EINVAL),
    ("NULL mandatory action_mask + hid 100", dict(action_mask=None, hid=100), (HM, HBM), EINVAL),
    ("hid 100 + action_stride n_branches - 1", dict(hid=100, action_stride=1), BRANCHED, EUNSUPPORTED),
    ("hid 100 + old_logps_stride sum(sizes) - 1", dict(hid=100, old_logps_stride=5), (HBK, HBKP), EUNSUPPORTED),
    ("hid 100 + old_logps_stride A - 1", dict(hid=100, old_logps_stride=7), (HK, HKP), EINVAL),
    ("hid 100 + action_stride A - 1", dict(hid=100, action_stride=2), BOX, EINVAL),
    ("NULL pre_p + hid 100", dict(pre_p=None, hid=100), BRANCHED, EUNSUPPORTED),
    ("NULL pre_p + hid 100", dict(pre_p=None, hid=100), UNBRANCHED + BOX, EINVAL),
    ("hid 100 + workspace one byte short", dict(hid=100, short=1), HEADS, EUNSUPPORTED),
    ("NULL pre_p + workspace one byte short", dict(pre_p=None, short=1), HEADS, EINVAL),
    ("action_mask off by 2 bytes + hid 100", dict(hid=100, **off2("action_mask")), (HM, HK, HKP), EINVAL),
    ("action_mask off by 2 bytes + hid 100", dict(hid=100, **off2("action_mask")), (HBM, HBK, HBKP), EUNSUPPORTED),
    ("NULL kl_coef + old_logps off by 2 bytes", dict(kl_coef=None, **off2("old_logps")), (HKP, HBKP), EINVAL),
    ("NULL kl_coef + hid 100", dict(kl_coef=None, hid=100), (HKP, HBKP, HGKP), EINVAL),
    # ---- PPO loss
    ("NULL kl_coef", null("kl_coef"), (PKP,), EINVAL),
    ("kl_coef off by 2 bytes", off2("kl_coef"), (PKP,), EINVAL),
    ("NULL old_logps", null("old_logps"), (PK, PKP), EINVAL),
    ("old_logps off by 2 bytes", off2("old_logps"), (PK, PKP), EINVAL),
    ("logps_off -1", dict(logps_off=-1), (PK, PKP), EINVAL),
    ("old_logps_stride logps_off + A - 1", dict(old_logps_stride=7), (PK, PKP), EINVAL),
    ("NULL mandatory action_mask", null("action_mask"), (PM,), EINVAL),
    ("NULL optional action_mask", null("action_mask"), (PK, PKP), OK),
    ("NULL optional action_mask + shift 60 (ignored)", dict(action_mask=None, mask_shift=60), (PK, PKP), OK),
    ("action_mask off by 2 bytes", off2("action_mask"), (PM, PK, PKP), EINVAL),
    ("shift 60 with A 5", dict(mask_shift=60), (PM, PK, PKP), EUNSUPPORTED),
    ("shift -1", dict(mask_shift=-1), (PM, PK, PKP), EUNSUPPORTED),
    ("N 0", dict(N=0), PPO, EINVAL),
    ("A 0", dict(A=0), (P, PM), EINVAL),
    ("NULL value with include_value", null("value"), PPO, EINVAL),
    ("NULL old_value with include_value", null("old_value"), PPO, EINVAL),
    ("NULL d_value with include_value", null("d_value"), PPO, EINVAL),
    ("workspace one byte short", dict(short=1), PPO, EWORKSPACE),
    ("NULL old_logps + shift 60", dict(old_logps=None, mask_shift=60), (PK, PKP), EINVAL),
    ("NULL mandatory action_mask + shift 60", dict(action_mask=None, mask_shift=60), (PM,), EINVAL),
    ("NULL logits + shift 60", dict(logits=None, mask_shift=60), (PM, PK, PKP), EINVAL),
    ("shift 60 + action_mask off by 2 bytes", dict(mask_shift=60, **off2("action_mask")), (PM, PK, PKP), EUNSUPPORTED),
    ("shift 60 + workspace one byte short", dict(mask_shift=60, short=1), (PM, PK, PKP), EUNSUPPORTED),
    ("NULL kl_coef + old_logps off by 2 bytes", dict(kl_coef=None, **off2("old_logps")), (PKP,), EINVAL),
    ("NULL kl_coef + shift 60", dict(kl_coef=None, mask_shift=60), (PKP,), EINVAL),
]
DEFECTS += [(f"NULL {n}", null(n), HEADS, EINVAL) for n in HEADS_POINTERS]
DEFECTS += [(f"NULL {n}", null(n), PPO, EINVAL) for n in PPO_POINTERS]


def _dev():
    return torch.device("cuda", 0)


def _lib():
    from etm import lib
    return lib.load()


@pytest.fixture(scope="module")
def inputs():
    """The operands every call reads, shared and left unchanged."""
    dev, g = _dev(), torch.Generator().manual_seed(11)
    rnd = lambda *s: (torch.randn(s, generator=g) * 0.5).to(dev)
    n = max(N_HEADS, N_PPO)
    return dict(pre_p=rnd(N_HEADS * HID_MAX), pre_v=rnd(N_HEADS * HID_MAX), b_lp=rnd(HID_MAX), b_lv=rnd(HID_MAX), wb=rnd(A_MAX * HID_MAX),
                bb=rnd(A_MAX), wv=rnd(HID_MAX), bv=rnd(1), logits=rnd(N_PPO * A_PPO), value=rnd(N_PPO),
                actions=(torch.arange(2 * n) % 3).to(dev), xact=rnd(N_HEADS * ROW_STRIDE), log_std=rnd(A_MAX),
                old_logp=(-1.0 - torch.rand(2 * n, generator=g)).to(dev), adv=rnd(n), old_value=rnd(n),
                adv_stats3=torch.tensor([float(n), 0.0, float(n - 1)], device=dev),
                old_logps=(-1.0 - torch.rand(n * ROW_STRIDE, generator=g)).to(dev), old_mean=rnd(N_HEADS * ROW_STRIDE), old_log_std=rnd(A_MAX),
                kl_coef=torch.tensor([0.2], device=dev),
                mask_unbranched=torch.full((n,), 0xFF, dtype=torch.int64, device=dev),
                mask_branched=torch.full((n,), 0x3F, dtype=torch.int64, device=dev),
                mask_ppo=torch.full((n,), 0x1F << SHIFT, dtype=torch.int64, device=dev))


def _outputs(entry):
    full = lambda k: torch.full((k,), SENTINEL, device=_dev())
    if entry in PPO:
        return dict(out8=full(8), d_logits=full(N_PPO * A_PPO), d_value=full(N_PPO), partials=full(64))
    return dict(gm_p=full(N_HEADS * HID_MAX), gm_v=full(N_HEADS * HID_MAX), sums=full((3 + A_MAX) * HID_MAX + 3 * A_MAX + 8), out8=full(8),
                logits_out=full(N_HEADS * A_MAX), value_out=full(N_HEADS), workspace=full(2 * ((3 + A_MAX) * HID_MAX + 3 * A_MAX + 8)))


def _untouched(o):
    return all(bool((t == SENTINEL).all()) for t in o.values())


def _heads_workspace_bytes(lib, entry, N, hid, A):
    kind = "gaussian_kl_" if entry in (HGK, HGKP) else "gaussian_" if entry == HG else "kl_" if "_kl" in entry else ""
    return getattr(lib, f"etm_heads_loss_{kind}workspace_bytes")(N, hid, A)


def _call(lib, entry, inp, out, over):
    """The entry with the good call's arguments, `over` replacing some by name; -> the return code."""
    over = dict(over)
    short, sizes = over.pop("short", 0), over.pop("sizes", (3, 3))
    ppo, box, branched = entry in PPO, entry in BOX, entry in BRANCHED
    kl, pen = "_kl" in entry, entry.endswith("_penalty")
    masked = entry.endswith("_masked") or (kl and not box)
    a = dict(inp, **out)
    a.update(stream=torch.cuda.current_stream().cuda_stream, clip=0.2, vf_coef=0.5, beta=0.01, dyn=None)
    if ppo:
        N, A = N_PPO, A_PPO
        a.update(action_stride=1, logp_stride=1, pol_scale=1.0 / N, ent_scale=1.0 / N, val_scale=1.0 / N, include_value=1, N=N, A=A,
                 partials_bytes=lib.etm_ppo_loss_workspace_bytes(N) - short, action_mask=inp["mask_ppo"], mask_shift=SHIFT,
                 old_logps_stride=SHIFT + A, logps_off=SHIFT)
        order = ["logits", "actions", "action_stride", "old_logp", "logp_stride", "adv", "old_value", "value", "adv_stats3", "clip", "vf_coef",
                 "beta", "pol_scale", "ent_scale", "val_scale", "include_value", "out8", "d_logits", "d_value", "partials", "partials_bytes",
                 "dyn", "N", "A"]
        order += ["action_mask", "mask_shift"] * masked + ["old_logps", "old_logps_stride", "logps_off"] * kl
    else:
        N, A, nbr = N_HEADS, (3 if box else 8), (len(sizes) if branched else 1)
        total = sum(sizes) if branched else A
        a.update(logits=out["logits_out"], value=out["value_out"], N=N, hid=HID, A=A, n_branches=nbr,
                 branch_sizes=(ctypes.c_int32 * len(sizes))(*sizes), action_stride=ROW_STRIDE if box else nbr, logp_stride=nbr,
                 pol_scale=1.0 / (N * nbr), ent_scale=1.0 / N, val_scale=1.0 / N, action_mask=inp["mask_branched" if branched else "mask_unbranched"],
                 old_logps_stride=ROW_STRIDE, old_mean_stride=ROW_STRIDE,
                 workspace_bytes=_heads_workspace_bytes(lib, entry, N, HID, 6 if branched else A) - short)
        assert a["workspace_bytes"] + short > 0 and total <= A_MAX
        order = ["pre_p", "pre_v", "b_lp", "b_lv", "wb", "bb", "wv", "bv"]
        order += ["xact", "action_stride", "log_std", "old_logp", "logp_stride"] if box else ["actions", "action_stride", "old_logp", "logp_stride"]
        order += ["adv", "old_value", "adv_stats3", "clip", "vf_coef", "beta", "pol_scale", "ent_scale", "val_scale", "dyn", "gm_p", "gm_v", "sums",
                  "out8", "logits", "value", "workspace", "workspace_bytes", "N", "hid"]
        order += ["branch_sizes", "n_branches"] if branched else ["A"]
        order += ["action_mask"] * masked + ["old_logps", "old_logps_stride"] * (kl and not box)
        order += ["old_mean", "old_mean_stride", "old_log_std"] * (kl and box)
    order += ["kl_coef"] * pen + ["stream"]
    for name, v in over.items():
        assert name in order, (entry, name)
        a[name] = a[v[1]].data_ptr() + 2 if isinstance(v, tuple) else v
    ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v
    rc = getattr(lib, entry)(*[ptr(a[name]) for name in order])
    torch.cuda.synchronize()
    return rc


def test_the_table_covers_every_entry():
    assert len(set(ENTRIES)) == 15
    for entry in ENTRIES:
        names = {d[0] for d in DEFECTS if entry in d[2]}
        assert "workspace one byte short" in names and any(n.startswith("NULL") for n in names), entry
    assert all(code in (OK, EINVAL, EUNSUPPORTED, EWORKSPACE) for _, _, _, code in DEFECTS)


@pytest.mark.parametrize("entry", ENTRIES)
def test_good_call_is_accepted_and_writes_out8(inputs, entry):
    out = _outputs(entry)
    assert _call(_lib(), entry, inputs, out, {}) == OK
    assert bool(torch.isfinite(out["out8"]).all()) and not bool((out["out8"] == SENTINEL).any()), out["out8"].tolist()


@pytest.mark.parametrize("entry", ENTRIES)
def test_defective_calls_return_the_tables_code_and_write_nothing(inputs, entry):
    lib = _lib()
    rows = [d for d in DEFECTS if entry in d[2]]
    assert rows
    for what, over, _, code in rows:
        out = _outputs(entry)
        rc = _call(lib, entry, inputs, out, over)
        assert rc == code, (entry, what, rc, code)
        if code == OK:
            assert not bool((out["out8"] == SENTINEL).any()), (entry, what)
        else:
            assert _untouched(out), (entry, what)
