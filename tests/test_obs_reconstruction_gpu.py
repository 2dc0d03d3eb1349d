"""Observation reconstruction (``obs_reconstruction``) on the device: the fused last layer + loss kernel, the data-gradient kernel and the
reused weight-gradient entry through the C ABI against float64, the autograd node, and the trainer in its three forms of the step.

The bound, everywhere: a result may miss its float64 reference by at most 4 x the largest error of a float32 torch evaluation of the same
expression on the same operands (measured again in every run, on the device), with a floor of two float32 spacings of the result's
largest term for the cases where float32 torch is exact.  The reference is float64 ``conv_transpose2d`` and the host rule
(utils.obs_reconstruction_loss) on the kernel's own float32 inputs.  The largest term: of the loss, the largest l / M; of dz, its largest
element; of db, the largest |dz|; of da2 and dW (sums of products of dz with a weight / an activation), the product of the two largest
magnitudes -- an upper bound of the largest product, used by the floor only.

The shapes are the smallest at which tiling, the 2 x 2 overlap, the edges and the gather can each go wrong: (Hi, Wi) = (1, 1) has no
overlap, (2, 2) every overlap class once, (3, 2) is not square, (20, 20) is the real geometry (N = 2 only: 882 blocks, four workgroups);
N = 33 with (3, 2) fills more than one workgroup of both kernels (33 * 4 * 3 = 396 blocks of 4 x 4 pixels)."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resume_helpers as rh

pytestmark = pytest.mark.gpu

EINVAL, SENTINEL = -1, -7.25
BANK = 40


@pytest.fixture(autouse=True)
def _collect_between_tests():
    gc.collect()
    yield
    gc.collect()


def _dev():
    return torch.device("cuda", 0)


def _lib():
    from etm import lib
    return lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _eq(a, b):
    return a.shape == b.shape and not bool(torch.isnan(a).any()) and bool(torch.equal(a, b))


def _sp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


# ================================================================== 1. the kernels through the C ABI
class _Problem:
    """One call's operands on the device.  ``byte``: a uint8 bank; ``gather``: a bank of 40 images behind a permuted index with one
    repeated entry (else the N images themselves)."""

    def __init__(self, N, Hi, Wi, C, byte, gather, seed=0):
        g = torch.Generator().manual_seed(1000 * N + 100 * Hi + 10 * Wi + C + seed)
        self.N, self.Hi, self.Wi, self.C, self.Ho, self.Wo = N, Hi, Wi, C, 4 * Hi + 4, 4 * Wi + 4
        self.a2 = torch.relu(torch.randn((N, Hi, Wi, 32), generator=g)).to(_dev())
        self.w = (torch.randn((32, C, 8, 8), generator=g) * 0.15).to(_dev())
        self.b = (torch.randn((C,), generator=g) * 0.1).to(_dev())
        images = BANK if gather else N
        raw = torch.randint(0, 256, (images, self.Ho, self.Wo, C), generator=g, dtype=torch.uint8)
        self.index = None
        if gather:
            idx = torch.randperm(BANK, generator=g)[:N]
            if N > 1:
                idx[-1] = idx[0]
            self.index = idx.to(_dev())
        from etm.ops import byte_unit_table
        self.x_u8 = raw.to(_dev())
        self.x_f32 = torch.from_numpy(byte_unit_table())[raw.long()].to(_dev())
        self.x = self.x_u8 if byte else self.x_f32
        self.byte = byte
        self.target = self.x_f32 if self.index is None else self.x_f32.index_select(0, self.index)      # [N, Ho, Wo, C] float32
        self.M = N * self.Ho * self.Wo * C

    def outputs(self):
        d = _dev()
        return dict(dz=torch.full((self.N, self.Ho, self.Wo, self.C), SENTINEL, device=d), out=torch.full((4,), SENTINEL, device=d),
                    db=torch.full((self.C,), SENTINEL, device=d))

    def fwd(self, coef, expect=0, bank=None, **ptr):
        """etm_obs_recon_fwd_loss -> its outputs.  ``ptr``: argument name -> a replacement address / value."""
        lib = _lib()
        x = self.x if bank is None else bank
        o = self.outputs()
        nbytes = max(lib.etm_obs_recon_workspace_bytes(self.N, self.C, self.Hi, self.Wi), 64)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=_dev())
        word = torch.tensor([coef], dtype=torch.float32, device=_dev())
        a = dict(a2=self.a2.data_ptr(), w=self.w.data_ptr(), bias=self.b.data_ptr(), x=x.data_ptr(), u8=int(x.dtype == torch.uint8),
                 x_index=None if self.index is None else self.index.data_ptr(), x_images=x.shape[0], word=word.data_ptr(),
                 dz=o["dz"].data_ptr(), out=o["out"].data_ptr(), db=o["db"].data_ptr(), ws=ws.data_ptr(), nbytes=nbytes, N=self.N, C=self.C,
                 Hi=self.Hi, Wi=self.Wi)
        a.update({k: (v(a) if callable(v) else v) for k, v in ptr.items()})
        rc = lib.etm_obs_recon_fwd_loss(*a.values(), _st())
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect, ptr)
        return o

    def dgrad(self, grad, expect=0, **ptr):
        da2 = torch.full_like(self.a2, SENTINEL)
        a = dict(dz=grad.data_ptr(), w=self.w.data_ptr(), a2=self.a2.data_ptr(), da2=da2.data_ptr(), N=self.N, C=self.C, Hi=self.Hi, Wi=self.Wi)
        a.update({k: (v(a) if callable(v) else v) for k, v in ptr.items()})
        rc = _lib().etm_obs_recon_dgrad(*a.values(), _st())
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect, ptr)
        return da2

    def reference(self, coef, dt):
        """(loss, dz, db, da2, dW) in ``dt``: float64 on the host with the host rule, float32 as torch operations on the device."""
        from utils import obs_reconstruction_loss
        c32 = float(np.float32(coef))
        if dt == torch.float64:
            a2, w, b, t = (v.detach().cpu().double() for v in (self.a2, self.w, self.b, self.target))
            z = F.conv_transpose2d(a2.permute(0, 3, 1, 2), w, b, stride=4).permute(0, 2, 3, 1)
            loss, dl = obs_reconstruction_loss(z.numpy(), t.numpy(), np.float64)
            loss, dz = torch.tensor(loss), torch.from_numpy(dl) * c32
            self.largest_l = float((torch.clamp_min(z, 0) - z * t + torch.log1p(torch.exp(-z.abs()))).max()) / self.M
        else:
            a2, w, b, t = self.a2, self.w, self.b, self.target
            z = F.conv_transpose2d(a2.permute(0, 3, 1, 2), w, b, stride=4).permute(0, 2, 3, 1)
            e = torch.exp(-z.abs())
            loss = (torch.clamp_min(z, 0) - z * t + torch.log1p(e)).mean()
            r = 1.0 / (1.0 + e)
            dz = (torch.where(z >= 0, r, e * r) - t) / self.M * c32
        db = dz.sum(dim=(0, 1, 2))
        wv = w.clone().requires_grad_(True)
        y = F.conv2d(dz.permute(0, 3, 1, 2), wv, stride=4)                      # the first encoder layer's forward on the gradient image
        da2 = (y.permute(0, 2, 3, 1) * (a2 > 0)).detach()
        (dW,) = torch.autograd.grad(y, wv, a2.permute(0, 3, 1, 2))
        return [v.detach().double().cpu() for v in (loss, dz, db, da2, dW)]


GRID = [(N, Hi, Wi, C) for (Hi, Wi) in ((1, 1), (2, 2), (3, 2)) for C in (1, 3) for N in (1, 3, 33)] + [(2, 20, 20, C) for C in (1, 3)]


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gathered"])
@pytest.mark.parametrize("byte", [False, True], ids=["float32", "uint8"])
@pytest.mark.parametrize("N,Hi,Wi,C", GRID, ids=lambda v: str(v))
def test_kernels_against_float64(N, Hi, Wi, C, byte, gather):
    from etm import ops
    p = _Problem(N, Hi, Wi, C, byte, gather)
    coef = 0.75
    o = p.fwd(coef)
    da2 = p.dgrad(o["dz"])
    dW = ops.obs_recon_wgrad(o["dz"], p.a2)
    torch.cuda.synchronize()
    assert float(o["out"][1]) == coef and float(o["out"][3]) == 0.0
    assert float(o["out"][2]) == float(np.float32(coef) * np.float32(float(o["out"][0])))
    ref, t32 = p.reference(coef, torch.float64), p.reference(coef, torch.float32)
    got = [o["out"][0], o["dz"], o["db"], da2, dW]
    dz_max, w_max, a_max = float(ref[1].abs().max()), float(p.w.abs().max()), float(p.a2.max())
    largest = [p.largest_l, dz_max, dz_max, dz_max * w_max, dz_max * a_max]
    for name, g, r, t, term in zip(("loss", "dz", "db", "da2", "dW"), got, ref, t32, largest):
        err, terr = float((g.double().cpu() - r).abs().max()), float((t - r).abs().max())
        bound = max(4.0 * terr, 2.0 * _sp(term))
        print(f"[N {N} {Hi}x{Wi} C {C} {'u8' if byte else 'f32'} {'gathered' if gather else 'plain'}] {name}: kernel {err:.3e}, "
              f"float32 torch {terr:.3e}, bound {bound:.3e}, largest |reference| {float(r.abs().max()):.3e}")
        assert bool(torch.isfinite(g).all()) and err <= bound, (name, err, bound)
    assert bool((da2[p.a2 <= 0] == 0).all()) and bool((p.a2 <= 0).any()), "elements of da2 where a2 <= 0 are exactly 0"


@pytest.mark.parametrize("N,Hi,Wi,C,gather", [(3, 2, 2, 3, True), (33, 3, 2, 1, False), (2, 20, 20, 3, True)], ids=str)
def test_exact_properties(N, Hi, Wi, C, gather):
    p = _Problem(N, Hi, Wi, C, True, gather)
    one, again = p.fwd(0.3), p.fwd(0.3)
    for k in one:
        assert _eq(one[k], again[k]), f"two calls give equal bits: {k}"
    assert _eq(p.dgrad(one["dz"]), p.dgrad(one["dz"]))
    # uint8 and float32 targets of equal value give equal bits
    flt = p.fwd(0.3, bank=p.x_f32)
    for k in one:
        assert _eq(one[k], flt[k]), f"uint8 against float32 targets: {k}"
    # *coef = 0: dz exactly 0, the loss unchanged
    zero = p.fwd(0.0)
    assert bool((zero["dz"] == 0).all()) and bool((zero["db"] == 0).all())
    assert float(zero["out"][0]) == float(one["out"][0]) and float(zero["out"][1]) == 0.0 and float(zero["out"][2]) == 0.0
    assert bool((p.dgrad(zero["dz"]) == 0).all())
    # doubling coef doubles dz bit for bit
    two = p.fwd(0.6)
    assert _eq(two["dz"], one["dz"] * 2.0) and float(two["out"][0]) == float(one["out"][0])


def _untouched(*tensors):
    return all(bool((t == SENTINEL).all()) for t in tensors)


def test_every_refusal_leaves_sentinels():
    p = _Problem(3, 2, 2, 3, False, True)
    pb = _Problem(3, 2, 2, 3, True, False)
    lib = _lib()
    assert lib.etm_obs_recon_supported(3, 2, 2) == 1 and lib.etm_obs_recon_supported(0, 2, 2) == 0 and lib.etm_obs_recon_supported(5, 2, 2) == 0
    word = torch.tensor([0.5], dtype=torch.float32, device=_dev())
    cases = [dict(a2=None), dict(w=None), dict(bias=None), dict(x=None), dict(word=None), dict(dz=None), dict(out=None), dict(db=None), dict(ws=None),
             dict(a2=p.a2.data_ptr() + 4), dict(x=p.x.data_ptr() + 4), dict(w=p.w.data_ptr() + 2), dict(bias=p.b.data_ptr() + 2),
             dict(word=word.data_ptr() + 2), dict(word=word.data_ptr() + 1), dict(x_index=p.index.data_ptr() + 4),
             dict(N=0), dict(N=-1), dict(C=0), dict(C=5), dict(x_images=0), dict(x_images=-3)]
    for ptr in cases:
        o = p.fwd(0.5, expect=EINVAL, **ptr)
        assert _untouched(*o.values()), ptr
    # a misaligned output or workspace (of the call's own tensors: a callable moves the address inside the argument table)
    for key, by in (("dz", 4), ("out", 2), ("db", 2), ("ws", 4)):
        o = p.fwd(0.5, expect=EINVAL, **{key: lambda a, key=key, by=by: a[key] + by})
        assert _untouched(*o.values()), key
    o = pb.fwd(0.5, expect=EINVAL, x=pb.x_u8.data_ptr() + 2)          # a byte image needs 4-byte alignment
    assert _untouched(*o.values())
    good = p.fwd(0.5)
    for ptr in (dict(dz=None), dict(w=None), dict(a2=None), dict(da2=None), dict(dz=good["dz"].data_ptr() + 4), dict(a2=p.a2.data_ptr() + 8),
                dict(da2=lambda a: a["da2"] + 4), dict(w=p.w.data_ptr() + 1), dict(N=0), dict(C=0), dict(C=5)):
        assert _untouched(p.dgrad(good["dz"], expect=EINVAL, **ptr)), ptr


# ================================================================== 2. the node
def _decoder_loss(sd, h, obs_nchw, coef, hw3):
    """coef * (the mean sigmoid cross-entropy of the decoder's logits against ``obs_nchw``), the logits' shape, as plain torch operations in
    the dtype of ``h``: dec_hidden + ReLU viewed as the NHWC feature map, the three transposed layers, the rule's expression."""
    n = h.shape[0]
    x = torch.relu(h @ sd["dec_hidden.weight"].t() + sd["dec_hidden.bias"]).view(n, hw3[0], hw3[1], 64).permute(0, 3, 1, 2)
    x = torch.relu(F.conv_transpose2d(x, sd["dec_conv3.weight"], sd["dec_conv3.bias"], stride=1))
    x = torch.relu(F.conv_transpose2d(x, sd["dec_conv2.weight"], sd["dec_conv2.bias"], stride=2))
    z = F.conv_transpose2d(x, sd["dec_conv1.weight"], sd["dec_conv1.bias"], stride=4)
    t = obs_nchw.to(z.dtype)
    return coef * (torch.clamp_min(z, 0) - z * t + torch.log1p(torch.exp(-z.abs()))).mean()


DEC = ["dec_hidden.weight", "dec_hidden.bias", "dec_conv3.weight", "dec_conv3.bias", "dec_conv2.weight", "dec_conv2.bias", "dec_conv1.weight", "dec_conv1.bias"]


@pytest.mark.parametrize("byte", [False, True], ids=["float32", "uint8"])
def test_node_against_float64_autograd(byte):
    from etm import ops
    from model import ActorCriticModel, IndexedObservations
    cfg = dict(hidden_layer_size=64, obs_reconstruction=0.1,
               transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative", layer_norm="post",
                                gtrxl=False, gtrxl_bias=0.0))
    torch.manual_seed(3)
    m = ActorCriticModel(cfg, type("Space", (), {"shape": (3, 36, 36)})(), (3,), 16).to(_dev())
    g = torch.Generator().manual_seed(4)
    N = 37
    h = torch.randn((N, 64), generator=g).to(_dev()).requires_grad_(True)
    raw = torch.randint(0, 256, (BANK, 36, 36, 3), generator=g, dtype=torch.uint8)
    index = torch.randperm(BANK, generator=g)[:N].to(_dev())
    bank = raw.to(_dev()) if byte else (raw.float() / 255).to(_dev())
    coef = torch.tensor([0.25], dtype=torch.float32, device=_dev())
    params = [dict(m.named_parameters())[k] for k in DEC]
    term, out = ops.obs_reconstruction_loss(m.reconstruct(h), m.dec_conv1, IndexedObservations(bank, index), coef, with_out=True)
    got = torch.autograd.grad(term, [h] + params)
    torch.cuda.synchronize()
    target = (raw.float() / 255).to(_dev()).index_select(0, index).permute(0, 3, 1, 2)
    refs = []
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dt).requires_grad_(True) for k, v in m.named_parameters() if k in DEC}
        hh = h.detach().to(dt).requires_grad_(True)
        loss = _decoder_loss(sd, hh, target, 0.25, m._dec_hw3)
        refs.append((loss.detach(), torch.autograd.grad(loss, [hh] + [sd[k] for k in DEC])))
    (l64, g64), (l32, g32) = refs
    lerr, lterr = abs(float(term) - float(l64)), abs(float(l32) - float(l64))
    print(f"[node {'u8' if byte else 'f32'}] coef * loss {float(term):.6f}: kernel {lerr:.3e}, float32 torch {lterr:.3e}; out {out.tolist()}")
    assert lerr <= max(4.0 * lterr, 2.0 * _sp(float(l64)))
    assert float(out[2]) == float(term) and float(out[1]) == 0.25
    k_abs = max(float((a.double() - r).abs().max()) for a, r in zip(got, g64))
    t_abs = max(float((a.double() - r).abs().max()) for a, r in zip(g32, g64))
    for name, a, r, t in zip(["h"] + DEC, got, g64, g32):
        print(f"    d {name}: kernel {float((a.double() - r).abs().max()):.3e}, float32 torch {float((t.double() - r).abs().max()):.3e}, "
              f"largest |reference| {float(r.abs().max()):.3e}")
    print(f"    largest over all tensors: kernel {k_abs:.3e}, float32 torch {t_abs:.3e}, bound {4 * t_abs:.3e}")
    assert k_abs <= 4.0 * t_abs, (k_abs, t_abs)


# ================================================================== 3. the trainer
FORMS = {"captured, tables": {}, "captured, no tables": {"step_ends_fused": False}, "eager": rh.modes(False)}
SCHED = dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10)
SEED, EPOCHS, N_MB, SIDE = 11, 2, 2, 36


def _config(form="captured, tables", byte=False, **over):
    env = dict(type="Synthetic", obs_shape=[3, SIDE, SIDE], num_actions=3, max_episode_steps=16, seed=2, p_done=0.1, pool=4)
    if byte:
        env.update(observation_levels=256, observation_dtype="uint8")
    cfg = rh.config(**{"environment": env, "learning_rate_schedule": dict(SCHED), "n_mini_batch": N_MB, "epochs": EPOCHS, **FORMS[form], **over})
    cfg.pop("normalize_observations")
    cfg.pop("normalize_rewards")
    return cfg


def _perms(update):
    rng = np.random.default_rng(4 + update)
    return [rng.permutation(rh.W_T * rh.S_T) for _ in range(EPOCHS)]


def _update(tr):
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    rows, norms = tr._train_epochs(lr, clip, beta, perms=_perms(tr.update_index))
    tr.update_index += 1
    torch.cuda.synchronize()
    return np.stack(rows), norms


def _full_loss(sd, cfg, tr, idx, mb, clip, beta, coef, dt):
    """L_ppo + coef * loss of one minibatch in ``dt`` through the oracle's model (oracle/ref_model.py, restated up to h) and the decoder."""
    from oracle import ref_model as rm
    b, sf = tr.buffer, tr.buffer.samples_flat
    ep, ind = sf["memory_index"].index_select(0, idx), sf["memory_indices"].index_select(0, idx)
    pos = tr.model.transformer._pos()
    win = b.memories[ep[:, None], ind].to(dt)
    if pos is not None:
        win = win + pos.to(dt)[ind].unsqueeze(2)
    tcfg = dict(cfg["transformer"], positional_encoding="none")
    obs = sf["obs"].index_select(0, idx)
    obs = (obs.float() / 255 if obs.dtype == torch.uint8 else obs).to(dt)
    x = obs
    for i, s in ((1, 4), (2, 2), (3, 1)):
        x = torch.relu(F.conv2d(x, sd[f"conv{i}.weight"], sd[f"conv{i}.bias"], stride=s))
    x = torch.relu(x.reshape(x.shape[0], -1) @ sd["lin_hidden.weight"].t() + sd["lin_hidden.bias"])
    h, _, _ = rm.transformer(sd, tcfg, tr.max_episode_length, x, win, sf["memory_mask"].index_select(0, idx), ind)
    h_pi = torch.relu(h @ sd["lin_policy.weight"].t() + sd["lin_policy.bias"])
    h_v = torch.relu(h @ sd["lin_value.weight"].t() + sd["lin_value.bias"])
    value = (h_v @ sd["value.weight"].t() + sd["value.bias"]).reshape(-1)
    lsm = torch.log_softmax(h_pi @ sd["policy_branches.0.weight"].t() + sd["policy_branches.0.bias"], dim=-1)
    adv = mb["advantages"].to(dt)
    a_n = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lsm.gather(1, mb["actions"].reshape(-1, 1))[:, 0] - mb["log_probs"].reshape(-1).to(dt))
    pol = torch.min(ratio * a_n, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_n).mean()
    ent = -(lsm.exp() * lsm).sum(1).mean()
    vo = mb["values"].to(dt)
    ret = vo + adv
    vc = vo + (value - vo).clamp(min=-clip, max=clip)
    val = torch.max((value - ret) ** 2, (vc - ret) ** 2).mean()
    return -(pol - cfg["value_loss_coefficient"] * val + beta * ent) + _decoder_loss(sd, h, obs, coef, tr.model._dec_hw3)


@pytest.mark.parametrize("form,separate", [(f, False) for f in FORMS] + [("captured, tables", True)],
                         ids=list(FORMS) + ["captured, tables, separate heads"])
def test_first_step_arena_against_float64(form, separate):
    over = {"fused_heads_loss": False} if separate else {}
    cfg = _config(form, byte=(form == "captured, tables"), obs_reconstruction=0.5, **over)
    tr = rh.trainer(cfg, seed=SEED, run_id="recon_arena")
    try:
        coef = float(tr._recon_coef.item())
        assert coef == 0.5
        before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        names = [n for n, p in tr.model.arena_parameters()]
        assert names[-8:] == DEC
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
        perms = _perms(0)
        rows, _ = tr._train_epochs(lr, clip, beta, perms=perms)
        torch.cuda.synchronize()
        assert (tr._train_graph is not None) == (form != "eager")
        sf = tr.buffer.samples_flat
        mbs = tr.buffer.batch_size // N_MB
        idx = torch.as_tensor(perms[0][:mbs], device=tr.device, dtype=torch.long).sort().values
        mb = {k: sf[k].index_select(0, idx) for k in ("actions", "log_probs", "advantages", "values")}
        refs = []
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt).requires_grad_(True) for k, v in before.items()}
            refs.append(torch.autograd.grad(_full_loss(sd, cfg, tr, idx, mb, clip, beta, coef, dt), [sd[n] for n in names]))
        got, r64, r32 = first["g"], refs[0], refs[1]
        k_abs = max(float((g.double() - r).abs().max()) for g, r in zip(got, r64))
        t_abs = max(float((g.double() - r).abs().max()) for g, r in zip(r32, r64))
        dec = max(float(r.abs().max()) for n, r in zip(names, r64) if n in DEC)
        print(f"[{form}{', separate heads' if separate else ''}] first-step arena: kernel {k_abs:.3e}, float32 torch {t_abs:.3e}, bound {4 * t_abs:.3e}; "
              f"largest decoder gradient {dec:.3e}")
        assert all(bool(torch.isfinite(g).all()) for g in got) and dec > 0
        assert k_abs <= 4.0 * t_abs, (k_abs, t_abs)
        # the public surface: the float32 of the float64 mean over the returned steps
        tab = tr._recon_tab[:len(rows)].cpu().numpy()
        assert len(rows) == EPOCHS * N_MB and np.all(np.isfinite(tab)) and np.all(tab > 0)
        assert tr.last_obs_reconstruction == {"loss": float(np.float32(tab.astype(np.float64).mean())), "coef": 0.5}
        assert 0.3 < tr.last_obs_reconstruction["loss"] < 1.5, "a fresh decoder starts near ln 2"
        norms = tr._grad_keys
        assert "decoder" in norms
    finally:
        rh.release(tr)


def test_coefficient_zero_leaves_every_other_gradient_and_the_key_absent_trainer_allocates_nothing():
    sched = {"initial": 0.5, "final": 0.0, "power": 1.0, "max_decay_steps": 1}
    a = b = None
    try:
        a = rh.trainer(_config("eager", obs_reconstruction=sched), seed=SEED, run_id="recon_zero")
        b = rh.trainer(_config("eager"), seed=SEED, run_id="recon_absent")
        assert b._recon is None and b._recon_coef is None and b._recon_tab is None and b.last_obs_reconstruction is None
        assert b.model.recon_cfg is None and not any("dec_" in k for k in b.model.state_dict()) and "decoder" not in b._grad_keys
        assert [k for k in a.model.state_dict()][:-8] == [k for k in b.model.state_dict()]
        for k, v in b.model.state_dict().items():
            assert _eq(v, a.model.state_dict()[k]), k
        for tr in (a, b):
            torch.manual_seed(SEED)              # (the device's generator is shared: both rollouts draw the same uniforms)
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
        torch.cuda.synchronize()
        assert _eq(a.buffer.obs, b.buffer.obs) and _eq(a.buffer.advantages, b.buffer.advantages) and _eq(a.buffer.actions, b.buffer.actions)
        idx = np.sort(_perms(0)[0][: a.buffer.batch_size // N_MB])
        lr, beta, clip = a.schedules(1)
        a.update_index = 1                       # the schedule's coefficient is exactly 0 from update 1 on
        ga, gb = a.minibatch_gradients(idx, clip, beta), b.minibatch_gradients(idx, clip, beta)
        torch.cuda.synchronize()
        assert float(a._recon_coef.item()) == 0.0
        other = {k: float((ga[k].double() - v.double()).abs().max()) for k, v in gb.items() if not _eq(ga[k], v)}
        print(f"[coef = 0] tensors whose gradient differs from the key-absent trainer's: {other}")
        assert other == {}, "coef = 0: every other gradient is the key-absent trainer's"
        for k in DEC:
            assert bool((ga[k] == 0).all()), f"coef = 0: the gradient of {k} is exactly 0"
        a.update_index = 0
        g0 = a.minibatch_gradients(idx, clip, beta)
        assert float(a._recon_coef.item()) == 0.5 and all(float(g0[k].abs().max()) > 0 for k in DEC)
    finally:
        rh.release(a, b)


def test_checkpoint_resumes_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sched = {"initial": 0.5, "final": 0.1, "power": 1.0, "max_decay_steps": 4}
    cfg = _config("eager", obs_reconstruction=sched)
    tr = fresh = None
    try:
        tr = rh.trainer(cfg, seed=SEED, run_id="recon_ckpt")
        rh.update(tr)
        assert tr.last_obs_reconstruction["coef"] == 0.5
        path = tr.save_checkpoint()
        tr.restart_episodes(1)
        rec_a, pub_a = rh.update(tr), dict(tr.last_obs_reconstruction)
        assert pub_a["coef"] == float(np.float32(0.4)) and any(k.startswith("param:dec_conv1") for k in rec_a)
        tr.load_checkpoint(path)
        rec_b = rh.update(tr)
        print(f"[resume in place] differing: {rh.differing(rec_a, rec_b)}")
        assert rh.differing(rec_a, rec_b) == [] and tr.last_obs_reconstruction == pub_a
        fresh = rh.trainer(cfg, seed=999, run_id="recon_fresh", resume=path)
        assert fresh.update_index == 1
        rec_c = rh.update(fresh)
        assert rh.differing(rec_a, rec_c) == [] and fresh.last_obs_reconstruction == pub_a
    finally:
        rh.release(tr, fresh)


def test_refusals_raise_at_construction():
    from trainer import PPOTrainer

    def build(cfg, **kw):
        return PPOTrainer(cfg, run_id="recon_refused", device=rh.dev(), tensorboard=False, **kw)

    with pytest.raises(ValueError, match=r"obs_reconstruction must be a number > 0"):
        build(_config(obs_reconstruction=0))
    with pytest.raises(ValueError, match=r"exactly the keys"):
        build(_config(obs_reconstruction={"initial": 0.1}))
    with pytest.raises(ValueError, match=r"obs_reconstruction is for image observations"):
        build(dict(_config(obs_reconstruction=0.1), environment=dict(type="Synthetic", obs_shape=[5], num_actions=3, max_episode_steps=16, seed=2,
                                                                     p_done=0.1, pool=4)))
    with pytest.raises(ValueError, match=r"does not map a side of 40 pixels back"):
        build(dict(_config(obs_reconstruction=0.1), environment=dict(type="Synthetic", obs_shape=[3, 40, 40], num_actions=3, max_episode_steps=16,
                                                                     seed=2, p_done=0.1, pool=4)))
    dp = type("DP", (), {"world": 2, "rank": 0})()
    with pytest.raises(ValueError, match=r"obs_reconstruction in a data-parallel run.*remove the key, or train on one device"):
        build(_config(obs_reconstruction=0.1), dp=dp)
