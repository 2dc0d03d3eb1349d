"""The exact Gaussian KL (``kl_estimator: analytic``) on the device: the four Gaussian sampling sites with the means staged, the
Gaussian heads + loss kernel with the KL sum, and the trainer in all three forms of the step.

Measured on the MI355X over the loss cases below (profiles/r17/analytic_kl.txt has the same two figures over the full 5 x 3 x 3 product):
  largest |float32 torch evaluation of rsl_rl's expression - float64|: 1.288e-07  (N 2059, hid 384, A 8; a KL of 0.759)
  largest |out8[4] of etm_heads_loss_gaussian_kl - float64|:            4.398e-08  (N 2059, hid 512, A 3; 1.48 ulp of 0.346)
The bound every comparison of a device KL with float64 uses is 4 x the first, measured again by every run of this file on its own
inputs (the fixture ``loss_cases``: nothing is fixed in advance), or 4 ulp of the value where that is larger.  The trainer's column 4
against float64 on eagerly recomputed means: worst 4.0e-10 on KLs of 2e-5 .. 3e-3."""
import gc
import math

import numpy as np
import pytest
import torch

import resume_helpers as rh

pytestmark = pytest.mark.gpu

LOGP_BOUND = 9.0e-7                      # tests/test_continuous_vs_float64.py: BOUNDS["logp"], the rollout log-prob against float64
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
SENTINEL = -7.25
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(autouse=True)
def _collect_between_tests():
    gc.collect()
    yield
    gc.collect()


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ================================================================== the sampler, per site
SITE_CASES = [(A, W) for A in (1, 3, 8) for W in (1, 8)]
LOG_STD = (-1.0, 0.0, 0.5)
LOW, HIGH = -1.0, 1.5
S_SITE = 3                               # rows 0 / 1 or 1 / 2 are written by the two steps, the third keeps its sentinel


def _log_std(A):
    return torch.tensor([LOG_STD[a % 3] for a in range(A)], dtype=torch.float32)


def _draws(A, W, seed):
    """(normals [S, W, A], forced [S, W, A]: NaN but one row -- worker W - 1 of the second step written, partly outside the bounds)."""
    g = torch.Generator().manual_seed(seed)
    normals = torch.randn((S_SITE, W, A), generator=g)
    forced = torch.full((S_SITE, W, A), float("nan"))
    return normals, forced, 3.0 * torch.randn((A,), generator=g)


def _tables(A, W, means):
    dev = _dev()
    t = dict(actions=torch.full((S_SITE, W, A), SENTINEL, device=dev), log_probs=torch.full((S_SITE, W, 1), SENTINEL, device=dev),
             values=torch.full((S_SITE, W), SENTINEL, device=dev))
    if means:
        t["means"] = torch.full((S_SITE, W, A), SENTINEL, device=dev)
    return t


def _direct_site(site, A, W, means, normals, forced, first_row):
    """Two steps (rows first_row, first_row + 1) of the ``sample`` / ``policy`` site through etm/ops.py on fixed random operands ->
    every output as host arrays."""
    from etm import ops
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * A + W)
    hid = 64
    st = _tables(A, W, means)
    t_dev = torch.full((), first_row, dtype=torch.int64, device=dev)
    act = torch.full((W, A), SENTINEL, device=dev)
    log_std = _log_std(A).to(dev)
    kw = dict(st_means=st["means"]) if means else {}
    mean_head, value_head = torch.nn.Linear(hid, A), torch.nn.Linear(hid, 1)
    with torch.no_grad():
        for m in (mean_head, value_head):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) / hid ** 0.5)
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    mean_head, value_head = mean_head.to(dev), value_head.to(dev)
    h_bias = (0.1 * torch.randn(2 * hid, generator=g)).to(dev)
    clipped = []
    for step in range(2):
        if site == "sample":
            mu, value = torch.randn((W, A), generator=g).to(dev), torch.randn(W, generator=g).to(dev)
            ops.rollout_sample_gaussian(mu, value, log_std, normals.to(dev), forced.to(dev), t_dev, act, st["actions"], st["log_probs"],
                                        st["values"], low=LOW, high=HIGH, **kw)
        else:
            h2 = torch.randn((W, 2 * hid), generator=g).to(dev)
            ops.rollout_policy_gaussian(h2, mean_head, value_head, log_std, normals.to(dev), forced.to(dev), t_dev, act, st["actions"],
                                        st["log_probs"], st["values"], low=LOW, high=HIGH, h_bias=h_bias, **kw)
        torch.cuda.synchronize()
        clipped.append(act.cpu().numpy().copy())
    out = {k: v.cpu().numpy() for k, v in st.items()}
    out.update(clipped=np.stack(clipped), t=int(t_dev.item()))
    return out


def _site_config(site, A, W, analytic):
    gated = site == "group"
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[7], continuous_actions=A, action_low=LOW, action_high=HIGH,
                                max_episode_steps=37, seed=3, p_done=0.01, pool=4),
               gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=W, worker_steps=S_SITE, n_mini_batch=1,
               value_loss_coefficient=0.5, hidden_layer_size=384, max_grad_norm=0.5, rollout_groups=1, rollout_min_group_size=2,
               hip_graph_rollout=False, hip_graph_train=False, tunable_gemm=False,
               transformer=dict(num_blocks=2, embed_dim=384, num_heads=4, memory_length=32, positional_encoding="relative",
                                layer_norm="pre" if gated else "post", gtrxl=gated, gtrxl_bias=1.0 if gated else 0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    if analytic:
        cfg["kl_estimator"] = "analytic"
    return cfg


def _trainer_site_passes(site, A, W, analytic, passes):
    """The step kernel of a worker (``worker``: post-LN) or of a group (``group``: GRU-gated pre-LN) through a trainer's own eager step,
    two steps per pass on fixed observations at episode steps 0 and 1, the staging tables pre-filled with the sentinel.  ``passes``:
    (normals, forced) each -> one output dict per pass."""
    from etm import ops
    from trainer import PPOTrainer
    torch.manual_seed(31)
    tr = PPOTrainer(_site_config(site, A, W, analytic), run_id="akl_site", device=_dev(), tensorboard=False)
    outs = []
    try:
        assert tr.box is not None and tr._kl_analytic == analytic and ("means" in tr._stage) == analytic and (tr.buffer.means is not None) == analytic
        with torch.no_grad():
            tr.model.policy_log_std.copy_(_log_std(A))
        obs = np.random.default_rng(5).normal(size=(2, W, 7)).astype(np.float32)
        g = tr._group_all
        main = torch.cuda.current_stream(tr.device)
        for normals, forced in passes:
            tr.worker_current_episode_step[:] = 0
            tr.obs[:] = obs[0]
            # (the tables of _begin_rollout are [W, S, A]: worker-major, as the buffer's)
            plan, groups = tr._begin_rollout(main, forced.transpose(0, 1).contiguous(), None, normals.transpose(0, 1).contiguous())
            assert groups == [g] and not plan.graph
            for table in tr._stage.values():
                if table.dtype == torch.float32:
                    table.fill_(SENTINEL)
            clipped = []
            for step in range(2):
                tr.worker_current_episode_step[:] = step
                tr.obs[:] = obs[step]
                tr._launch_eager(g, plan)
                torch.cuda.synchronize()
                clipped.append(tr._act_pin.numpy().copy())
            assert g.rf_scratch is not None and g.group_kernel == (site == "group"), "the step kernel of the site did not run"
            assert int(ops.rollout_trxl_error(g.rf_scratch).item()) == 0
            out = {k: tr._stage[k].cpu().numpy() for k in ("actions", "log_probs", "values") + (("means",) if analytic else ())}
            out.update(clipped=np.stack(clipped), t=int(g.t_dev.item()))
            outs.append(out)
            tr._forced_tab.fill_(float("nan"))
    finally:
        tr.close()
        del tr
        gc.collect()
        torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("A,W", SITE_CASES)
@pytest.mark.parametrize("site", ["sample", "policy", "worker", "group"])
def test_site_stages_the_means_and_keeps_every_other_bit(site, A, W):
    normals, forced, forced_row = _draws(A, W, 7 * A + W)
    w_f = W - 1
    direct = site in ("sample", "policy")
    first = 1 if direct else 0                       # (the trainer's step counter restarts at 0)
    rows = (first, first + 1)
    spare = ({0, 1, 2} - set(rows)).pop()
    forced[rows[1], w_f] = forced_row
    zero, nan = torch.zeros_like(normals), torch.full_like(forced, float("nan"))
    if direct:
        on = _direct_site(site, A, W, True, normals, forced, first)
        off = _direct_site(site, A, W, False, normals, forced, first)
        mode = _direct_site(site, A, W, True, zero, nan, first)
    else:
        on, mode = _trainer_site_passes(site, A, W, True, [(normals, forced), (zero, nan)])
        off, = _trainer_site_passes(site, A, W, False, [(normals, forced)])
    # 1. the twin's bits: staged actions, log-probs, values, the clipped actions of both steps, the step counter
    for k in ("actions", "log_probs", "values", "clipped"):
        assert _same(on[k], off[k]), (site, k)
    assert on["t"] == off["t"] == first + 2
    assert np.array_equal(on["clipped"][1], np.clip(on["actions"][rows[1]], LOW, HIGH))
    assert np.array_equal(on["actions"][rows[1], w_f], forced_row.numpy()), "the forced row was honoured"
    # 2. a zero normals table: x = mu + sigma * 0 is the mean, bit for bit
    for r in rows:
        assert _same(mode["means"][r], mode["actions"][r]), (site, r)
    # 3. forced or not, the stored mean is the policy's: the means of the same call without forcing (and with other normals)
    for r in rows:
        assert _same(on["means"][r], mode["means"][r]), (site, r)
    assert not np.array_equal(on["means"][rows[1], w_f], on["actions"][rows[1], w_f])
    # 4. the rows of other steps are untouched
    for out in (on, mode):
        for k in ("actions", "log_probs", "values", "means"):
            assert np.all(out[k][spare] == np.float32(SENTINEL)), (site, k)
    assert np.all(off["actions"][spare] == np.float32(SENTINEL))
    # 5. the staged log-prob from the stored means and actions in float64, within the rollout log-prob's bound
    ls = _log_std(A).double().numpy()
    x, mu = on["actions"][list(rows)].astype(np.float64), on["means"][list(rows)].astype(np.float64)
    z = (x - mu) / np.exp(ls)
    lp_ref = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(axis=-1)
    lp = on["log_probs"][list(rows), :, 0].astype(np.float64)
    err = np.abs(lp - lp_ref) / np.maximum(np.abs(lp_ref), 1.0)
    print(f"[site {site} A={A} W={W}] log-prob from the stored means: worst relative error {err.max():.2e} (bound {LOGP_BOUND:.1e})")
    assert err.max() <= LOGP_BOUND


def test_means_entries_refuse_a_missing_or_misaligned_table():
    """NULL / misaligned st_means at the two entries that can be called without a model: ETM_EINVAL and nothing written."""
    from etm import lib as etm_lib
    lib = etm_lib.load()
    dev = _dev()
    A, W = 3, 4
    st = _tables(A, W, True)
    mean, value = torch.randn((W, A), device=dev), torch.randn(W, device=dev)
    log_std, normals = _log_std(A).to(dev), torch.randn((S_SITE, W, A), device=dev)
    t_dev = torch.zeros((), dtype=torch.int64, device=dev)
    act = torch.full((W, A), SENTINEL, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for bad in (0, st["means"].data_ptr() + 2):
        rc = lib.etm_rollout_sample_gaussian_means(mean.data_ptr(), value.data_ptr(), log_std.data_ptr(), normals.data_ptr(), None,
                                                   t_dev.data_ptr(), act.data_ptr(), st["actions"].data_ptr(), st["log_probs"].data_ptr(),
                                                   st["values"].data_ptr(), None, None, W, A, bad, stream)
        assert rc == EINVAL
        h2, wp, bp = torch.randn((W, 128), device=dev), torch.randn((A, 64), device=dev), torch.randn(A, device=dev)
        wv, bv, sync = torch.randn((1, 64), device=dev), torch.randn(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.etm_rollout_policy_gaussian_means(h2.data_ptr(), None, wp.data_ptr(), bp.data_ptr(), wv.data_ptr(), bv.data_ptr(),
                                                   log_std.data_ptr(), normals.data_ptr(), None, t_dev.data_ptr(), act.data_ptr(),
                                                   st["actions"].data_ptr(), st["log_probs"].data_ptr(), st["values"].data_ptr(), None, None,
                                                   sync.data_ptr(), None, None, W, A, 64, W, bad, stream)
        assert rc == EINVAL
    torch.cuda.synchronize()
    assert int(t_dev.item()) == 0 and bool((act == SENTINEL).all()) and all(bool((t == SENTINEL).all()) for t in st.values())


# ================================================================== the loss
# a thin cross over N (one wave's pair, a full workgroup, a second workgroup with one sample, a ragged tail, more than 256 workgroup
# rows), hid (HC 1, 6, 8) and A: every N, every A and every HC at least twice
LOSS_CASES = [(1, 64, 1), (8, 384, 3), (9, 512, 8), (37, 64, 3), (2059, 384, 8), (2059, 64, 1), (37, 512, 1), (8, 512, 3), (9, 64, 8),
              (1, 384, 8), (2059, 512, 3)]
CLIP, VF, BETA = 0.2, 0.5, 0.01


class _Loss:
    """The operands of one heads + loss problem on the device and the two entries through the C ABI."""

    def __init__(self, N, hid, A, seed=None):
        from etm import lib as etm_lib
        from etm import ops
        self.lib, self.N, self.hid, self.A = etm_lib.load(), N, hid, A
        dev = _dev()
        g = torch.Generator().manual_seed(seed if seed is not None else 13 * N + 5 * hid + A)
        r = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev)
        self.pre_p, self.pre_v = r(N, hid), r(N, hid)
        self.b_lp, self.b_lv = r(hid, s=0.1), r(hid, s=0.1)
        self.wb, self.bb, self.wv, self.bv = r(A, hid, s=hid ** -0.5), r(A, s=0.1), r(hid, s=hid ** -0.5), r(1, s=0.1)
        self.log_std = torch.tensor([(-0.5, 0.0, 0.7)[a % 3] for a in range(A)], device=dev)
        self.adv, self.old_value = r(N), r(N)
        self.stats3 = ops.adv_stats(self.adv)
        self.xact, self.old_logp = torch.zeros((N, A), device=dev), torch.zeros(N, device=dev)
        mu = self.twin()["logits"]                                 # the kernel's own means (they do not depend on the actions)
        sigma = self.log_std.exp()
        self.xact = (mu + sigma * r(N, A)).contiguous()
        lp = (-0.5 * ((self.xact - mu) / sigma) ** 2 - self.log_std - HALF_LOG_2PI).sum(1)
        self.old_logp = (lp - r(N, s=0.05)).contiguous()
        self.old_mean = (mu + 0.4 * sigma * r(N, A)).contiguous()
        self.old_log_std = (self.log_std + r(A, s=0.15)).contiguous()
        self.mu = mu

    def _outputs(self, row):
        dev, N, hid, A = _dev(), self.N, self.hid, self.A
        f = lambda *shape: torch.full(shape, SENTINEL, device=dev)
        return dict(gm_p=f(N, hid), gm_v=f(N, hid), sums=f(row), out8=f(8), logits=f(N, A), value=f(N))

    def _head(self, o, ws):
        p = lambda t: t.data_ptr()
        return (p(self.pre_p), p(self.pre_v), p(self.b_lp), p(self.b_lv), p(self.wb), p(self.bb), p(self.wv), p(self.bv), p(self.xact), self.A,
                p(self.log_std), p(self.old_logp), 1, p(self.adv), p(self.old_value), p(self.stats3), CLIP, VF, BETA, 1.0 / self.N,
                1.0 / self.N, 1.0 / self.N, None, p(o["gm_p"]), p(o["gm_v"]), p(o["sums"]), p(o["out8"]), p(o["logits"]), p(o["value"]),
                p(ws), ws.numel(), self.N, self.hid, self.A)

    def twin(self):
        lib = self.lib
        o = self._outputs(lib.etm_heads_loss_gaussian_row_floats(self.hid, self.A))
        ws = torch.empty(lib.etm_heads_loss_gaussian_workspace_bytes(self.N, self.hid, self.A), dtype=torch.uint8, device=_dev())
        rc = lib.etm_heads_loss_gaussian(*self._head(o, ws), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return o

    def kl(self, old_mean=None, old_log_std=None, stride=None, expect=0, hid=None, A=None, raw_ptrs=None):
        lib = self.lib
        old_mean = self.old_mean if old_mean is None else old_mean
        old_log_std = self.old_log_std if old_log_std is None else old_log_std
        o = self._outputs(lib.etm_heads_loss_gaussian_kl_row_floats(self.hid, self.A))
        ws = torch.full((max(lib.etm_heads_loss_gaussian_kl_workspace_bytes(self.N, self.hid, self.A), 4),), 0x5A, dtype=torch.uint8, device=_dev())
        head = list(self._head(o, ws))
        if hid is not None:
            head[-2] = hid
        if A is not None:
            head[-1] = A
        pm, pl = raw_ptrs if raw_ptrs is not None else (old_mean.data_ptr(), old_log_std.data_ptr())
        rc = lib.etm_heads_loss_gaussian_kl(*head, pm, old_mean.stride(0) if stride is None else stride, pl,
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, expect)
        torch.cuda.synchronize()
        o["ws"] = ws
        return o

    def kl64(self, mu, old_mean=None, old_log_std=None):
        from utils import gaussian_kl
        old_mean = self.old_mean if old_mean is None else old_mean
        old_log_std = self.old_log_std if old_log_std is None else old_log_std
        return float(gaussian_kl(old_mean.cpu().numpy(), old_log_std.cpu().numpy(), mu.cpu().numpy(), self.log_std.cpu().numpy(), np.float64))

    def rsl32(self, mu):
        """rsl_rl's expression as plain float32 torch operations (without its 1e-5)."""
        s, so = self.log_std.exp(), self.old_log_std.exp()
        kl = torch.sum(torch.log(s / so) + (so.square() + (self.old_mean - mu).square()) / (2.0 * s.square()) - 0.5, dim=-1)
        return float(kl.mean().item())


@pytest.fixture(scope="module")
def loss_cases():
    """Every case once: the two entries' outputs, the float64 KL on the kernel's own means, the error of the float32 torch evaluation of
    rsl_rl's expression and of the kernel -> ({case: record}, the bound's first term: 4 x the largest torch error)."""
    out = {}
    for case in LOSS_CASES:
        p = _Loss(*case)
        twin, kl = p.twin(), p.kl()
        ref = p.kl64(kl["logits"])
        out[case] = dict(p=p, twin=twin, kl=kl, ref=ref, torch_err=abs(p.rsl32(kl["logits"]) - ref), kernel_err=abs(float(kl["out8"][4]) - ref))
    worst_torch, worst_kernel = max(r["torch_err"] for r in out.values()), max(r["kernel_err"] for r in out.values())
    for case, r in out.items():
        print(f"[loss N={case[0]} hid={case[1]} A={case[2]}] kl64 {r['ref']:.9e} torch fp32 rsl_rl error {r['torch_err']:.3e} kernel error "
              f"{r['kernel_err']:.3e} ({r['kernel_err'] / _ulp32(r['ref']):.2f} ulp)")
    print(f"[loss] largest float32 torch error {worst_torch:.3e}, largest kernel error {worst_kernel:.3e}; bound = max(4 x {worst_torch:.3e}, 4 ulp)")
    return out, 4.0 * worst_torch


def _bound(loss_cases, value):
    return max(loss_cases[1], 4.0 * _ulp32(value))


@pytest.mark.parametrize("case", LOSS_CASES, ids=[f"N{n}_hid{h}_A{a}" for n, h, a in LOSS_CASES])
def test_loss_keeps_the_twins_bits_and_reduces_the_exact_kl(loss_cases, case):
    N, hid, A = case
    r = loss_cases[0][case]
    twin, kl = r["twin"], r["kl"]
    row = (3 + A) * hid + A + 1 + 5 + A
    assert twin["sums"].numel() == row and kl["sums"].numel() == row + 1
    for k in ("gm_p", "gm_v", "logits", "value"):
        assert _same(twin[k], kl[k]), k
    assert _same(twin["sums"], kl["sums"][:row]), "every element of the old row"
    t8, k8 = _bits(twin["out8"]), _bits(kl["out8"])
    assert np.array_equal(t8[[0, 1, 2, 3, 5, 7]], k8[[0, 1, 2, 3, 5, 7]]), "policy, value, loss, entropy, clip fraction"
    assert k8[6] == t8[4], "the k3 value moves to out8[6]"
    assert float(twin["out8"][6]) == 0.0
    got = float(kl["out8"][4])
    assert abs(got - r["ref"]) <= _bound(loss_cases, r["ref"]), (got, r["ref"], _bound(loss_cases, r["ref"]))
    # the raw sum at the end of the row is what out8[4] scales (ent_scale = 1 / N)
    assert abs(float(kl["sums"][row]) / N - got) <= 2 * _ulp32(got)


@pytest.mark.parametrize("case", [(1, 64, 1), (9, 512, 8), (2059, 384, 8), (37, 64, 3)])
def test_loss_equal_policies_give_exactly_zero(case):
    p = _Loss(*case)
    o = p.kl(old_mean=p.mu.clone(), old_log_std=p.log_std.clone())
    assert _same(o["logits"], p.mu)
    assert _bits(o["out8"])[4] == 0, float(o["out8"][4])
    assert float(o["sums"][-1]) == 0.0


@pytest.mark.parametrize("case", [(8, 384, 3), (2059, 64, 1), (37, 512, 1), (9, 64, 8)])
def test_loss_means_shifted_by_a_constant_number_of_sigmas(loss_cases, case):
    N, hid, A = case
    delta = 0.75
    p = _Loss(*case)
    old_mean = (p.mu + delta * p.log_std.exp()).contiguous()
    o = p.kl(old_mean=old_mean, old_log_std=p.log_std.clone())
    want = 0.5 * A * delta * delta
    got = float(o["out8"][4])
    # (the shift is rounded into old_mean: the float64 value on the operands themselves is what the kernel is held to as well)
    ref = p.kl64(o["logits"], old_mean, p.log_std)
    print(f"[shift N={N} hid={hid} A={A}] kernel {got!r}, A delta^2 / 2 = {want!r}, float64 on the rounded operands {ref!r}")
    assert abs(got - ref) <= _bound(loss_cases, ref)
    assert abs(got - want) <= _bound(loss_cases, want) + abs(ref - want)


def test_loss_refusals_write_nothing():
    p = _Loss(9, 64, 3)
    dev = _dev()
    tries = [dict(raw_ptrs=(0, p.old_log_std.data_ptr()), expect=EINVAL), dict(raw_ptrs=(p.old_mean.data_ptr(), 0), expect=EINVAL),
             dict(raw_ptrs=(p.old_mean.data_ptr() + 2, p.old_log_std.data_ptr()), expect=EINVAL),
             dict(raw_ptrs=(p.old_mean.data_ptr(), p.old_log_std.data_ptr() + 1), expect=EINVAL),
             dict(stride=2, expect=EINVAL),
             dict(hid=100, expect=EUNSUPPORTED), dict(hid=576, expect=EUNSUPPORTED)]
    for kw in tries:
        o = p.kl(**kw)
        for k, t in o.items():
            want = 0x5A if k == "ws" else SENTINEL
            assert bool((t == want).all()), (kw, k)
    # and the op: the two operands come together, with the minibatch's shape
    from etm import ops
    lin = lambda i, o_: torch.nn.Linear(i, o_).to(dev)
    h = torch.randn((9, 64), device=dev)
    args = (h, lin(64, 64), lin(64, 64), lin(64, 3), p.log_std, lin(64, 1), p.xact, p.old_logp, p.adv, p.old_value, CLIP, VF, BETA)
    with pytest.raises(ValueError, match="old_mean and old_log_std come together"):
        ops.heads_ppo_loss_gaussian(*args, old_mean=p.old_mean)
    with pytest.raises(ValueError, match=r"old_mean must be float32 \[9, 3\]"):
        ops.heads_ppo_loss_gaussian(*args, old_mean=p.old_mean[:, :2], old_log_std=p.old_log_std)
    loss, st = ops.heads_ppo_loss_gaussian(*args, old_mean=p.old_mean, old_log_std=p.old_log_std)
    loss_t, st_t = ops.heads_ppo_loss_gaussian(*args)
    assert st.shape == (6,) and _same(loss, loss_t) and _same(st[[0, 1, 2, 3, 5]], st_t[[0, 1, 2, 3, 5]])


# ================================================================== the trainer
FORMS = {"captured, tables": {}, "captured, no tables": {"step_ends_fused": False}, "eager": rh.modes(False)}
SCHED = dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10)
SEED, UPDATES, EPOCHS, N_MB = 11, 2, 3, 2
A_T = 2
KEY = {"kl_estimator": "analytic"}
_CACHE = {}


def _config(form="captured, tables", **over):
    """The tiny trainer of tests/resume_helpers.py as a Box policy of two dimensions."""
    env = dict(type="Synthetic", obs_shape=[rh.F_OBS], continuous_actions=A_T, max_episode_steps=16, seed=2, p_done=0.1, pool=4)
    return rh.config(**{"environment": env, "learning_rate_schedule": dict(SCHED), "n_mini_batch": N_MB, "epochs": EPOCHS, **FORMS[form], **over})


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


def _eager_means(tr, idx):
    """The Gaussian means of the minibatch ``idx`` on the trainer's current weights, by the model's own eager forward."""
    from etm.ops import WindowSpec
    mb = tr.buffer.gather(idx)
    m = tr.model
    with torch.no_grad():
        spec = WindowSpec.from_bank(mb["memories"], mb["memory_index"], mb["memory_indices"], mb["memory_indices"], mb["memory_mask"])
        h, _ = m.forward_state(mb["obs"], spec)
        hp = torch.relu(torch.nn.functional.linear(h, m.lin_policy.weight, m.lin_policy.bias))
        mu = torch.nn.functional.linear(hp, m.policy_branches[0].weight, m.policy_branches[0].bias)
    return mu, mb


def _stepwise_update(tr):
    """The update ``_update`` would run, one minibatch step at a time from outside ``_train_epochs`` (as
    tests/test_adaptive_lr_gpu.py::_single_steps), with the float64 KL of every step taken BEFORE it on the pre-step weights ->
    (statistics rows, float64 KL per row)."""
    from utils import gaussian_kl
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    perms = _perms(tr.update_index)
    mbs = tr.buffer.batch_size // N_MB
    with torch.no_grad():
        tr._bank_pos = tr._bank_with_positions()
        tr._obs_train = tr._training_observations()
    monitor = tr.config.get("monitor_gradients", True)
    rows, ref = [], []
    for i in range(EPOCHS * N_MB):
        perm = torch.as_tensor(perms[i // N_MB], device=tr.device, dtype=torch.long).view(-1, mbs).sort(dim=1).values
        idx = perm[i % N_MB].contiguous()
        mu, mb = _eager_means(tr, idx)
        ref.append(float(gaussian_kl(mb["means"].cpu().numpy(), tr.buffer.old_log_std.cpu().numpy(), mu.cpu().numpy(),
                                     tr.model.policy_log_std.detach().cpu().numpy(), np.float64)))
        if tr._use_train_graph:
            st, _ = tr._train_step_graph(idx, float(lr), clip, beta, monitor)
        else:
            st = tr._train_mini_batch(tr.buffer.gather(idx), float(lr), clip, beta)
        rows.append(st.cpu().numpy())
    if tr.model.obs_norm is not None:
        tr._update_obs_norm()
    tr._bank_pos = tr._row_stats = None
    tr.update_index += 1
    torch.cuda.synchronize()
    return np.stack(rows), np.asarray(ref)


def _plain_run(form, key):
    """Two updates of the key-absent (``key`` False) or key-on trainer without a KL rule -> (rows per update, norms, state, extras)."""
    name = ("plain", form, key)
    if name not in _CACHE:
        tr = None
        try:
            tr = rh.trainer(_config(form, **(KEY if key else {})), seed=SEED, run_id="akl_plain")
            assert tr.box is not None and tr._kl_analytic == key
            rows, norms, extra = [], [], []
            for _ in range(UPDATES):
                ls_before = tr.model.policy_log_std.detach().cpu().numpy().copy()
                r, n = _update(tr)
                rows.append(r), norms.append(n)
                if key:
                    extra.append(dict(ls_before=ls_before, ls_after=tr.model.policy_log_std.detach().cpu().numpy().copy(),
                                      old_log_std=tr.buffer.old_log_std.cpu().numpy().copy(), means=tr.buffer.means.cpu().numpy().copy(),
                                      stage=tr._stage["means"].cpu().numpy().copy(), flat=tr.buffer.samples_flat["means"].cpu().numpy().copy()))
            assert (tr._train_graph is not None) == (form != "eager")
            assert (getattr(tr, "_tg_idx_table", None) is not None) == (form == "captured, tables")
            if not key:
                assert tr.buffer.means is None and tr.buffer.old_log_std is None and "means" not in tr._stage and "means" not in tr.buffer.samples_flat
            _CACHE[name] = (rows, norms, rh.state(tr), extra)
        finally:
            rh.release(tr)
    return _CACHE[name]


@pytest.mark.parametrize("form", list(FORMS))
def test_key_on_without_a_rule_changes_column_4_only(loss_cases, form):
    rows_a, norms_a, state_a, _ = _plain_run(form, False)
    rows_b, norms_b, state_b, extra = _plain_run(form, True)
    assert rh.differing(state_a, state_b) == [] and int(state_b["step"]) == UPDATES * EPOCHS * N_MB
    others = [0, 1, 2, 3, 5]
    for u in range(UPDATES):
        assert rows_a[u].shape == rows_b[u].shape == (EPOCHS * N_MB, 6) and norms_a[u] == norms_b[u]
        assert np.array_equal(rh.bits(rows_a[u][:, others]), rh.bits(rows_b[u][:, others])), u
        assert not np.array_equal(rh.bits(rows_a[u][:, 4]), rh.bits(rows_b[u][:, 4])), "column 4 holds another statistic"
        e = extra[u]
        assert np.array_equal(rh.bits(e["means"]), rh.bits(e["stage"].transpose(1, 0, 2))), "buffer.means is the staging table transposed"
        assert np.array_equal(rh.bits(e["flat"]), rh.bits(e["means"].reshape(-1, A_T)))
        assert np.array_equal(rh.bits(e["old_log_std"]), rh.bits(e["ls_before"])) and not np.array_equal(e["old_log_std"], e["ls_after"])
    # column 4 against float64 on the update's own buffer, the new means by an eager forward on the pre-step weights: update 0 as the
    # run above ran it, update 1 one step at a time (the same bits as the run's rows)
    tr = None
    try:
        tr = rh.trainer(_config(form, **KEY), seed=SEED, run_id="akl_stepwise")
        for u in range(UPDATES):
            rows_s, ref = _stepwise_update(tr)
            assert np.array_equal(rh.bits(rows_s), rh.bits(rows_b[u])), (form, u)
            err = np.abs(rows_s[:, 4].astype(np.float64) - ref)
            print(f"{form}: update {u} exact kl rows {rows_s[:, 4].tolist()} float64 {ref.tolist()} k3 rows {rows_a[u][:, 4].tolist()} "
                  f"worst error {err.max():.3e}")
            for got, want in zip(rows_s[:, 4], ref):
                assert abs(float(got) - want) <= _bound(loss_cases, want), (form, u, float(got), want)
        assert rh.differing(rh.state(tr), state_b) == []
    finally:
        rh.release(tr)


def _walk(kl_rows, lr, rule, limit=None):
    """The host model of tests/test_adaptive_lr_gpu.py over one update's kl rows."""
    from utils import adaptive_lr_step
    rates, raises, cuts, applied, stopped = [], 0, 0, 0, False
    for kl in np.asarray(kl_rows, dtype=np.float32):
        lr, way = adaptive_lr_step(lr, kl, rule)
        raises, cuts = raises + (way == 1), cuts + (way == -1)
        if limit is not None and not kl <= np.float32(limit):
            stopped = True
            break
        rates.append(np.float32(lr))
        applied += 1
    return rates, np.float32(lr), raises, cuts, applied, stopped


def _band():
    """A band from the key-on probe's column-4 rows of its first update (the method of test_adaptive_lr_gpu._band): row 1 -- the first
    real KL -- lies below kl_low and raises the rate, kl_high lies between it and the largest later row."""
    if "band" not in _CACHE:
        kl = _plain_run("captured, tables", True)[0][0][:, 4]
        print("probe exact kl (n_mini_batch 2, epochs 3):", kl.tolist())
        later = float(kl[2:].max())
        assert 0 < float(kl[1]) < later, f"row 1 must be a real kl below a later row's: {kl.tolist()} (another seed is needed)"
        kl_low = np.float32(float(kl[1]) + 0.25 * (later - float(kl[1])))
        kl_high = np.float32(float(kl[1]) + 0.5 * (later - float(kl[1])))
        assert float(kl[1]) < kl_low < kl_high < later
        _CACHE["band"] = {"desired_kl": 1.0, "low": float(kl_low), "high": float(kl_high)}
    return _CACHE["band"]


def _bits32(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("form", list(FORMS))
def test_adaptive_lr_decides_on_the_exact_kl(form):
    """The run equals utils.adaptive_lr_step walked over the run's own column-4 rows, in the counters and the bits of lr_dev."""
    tr = None
    try:
        tr = rh.trainer(_config(form, adaptive_lr=_band(), **KEY), seed=SEED, run_id="akl_alr")
        rule = dict(tr._adapt.rule)
        lr = np.float32(SCHED["initial"])
        moved = set()
        for u in range(UPDATES):
            rows, _ = _update(tr)
            last = dict(tr.last_adaptive_lr)
            rates, lr, raises, cuts, applied, stopped = _walk(rows[:, 4], lr, rule)
            print(f"{form}: update {u} exact kl rows {rows[:, 4].tolist()} -> {last}")
            assert applied == EPOCHS * N_MB and not stopped
            assert last == {"lr": float(lr), "raised": raises, "lowered": cuts, "kl_low": rule["kl_low"], "kl_high": rule["kl_high"]}, u
            assert _bits32(tr.optimizer.lr_dev.item()) == _bits32(lr)
            moved |= {_bits32(r) for r in rates}
        assert len(moved) >= 2, "the rate moved"
    finally:
        rh.release(tr)


def test_target_kl_stops_on_the_exact_kl_in_the_middle_of_an_epoch():
    rows = _plain_run("captured, tables", True)[0]
    kl = rows[0][:, 4]
    records = [r for r in (1, 2, 3, 4, 5) if kl[r] > kl[:r].max() and r % N_MB == 0]
    assert records, f"no first minibatch of an epoch has a kl above all earlier rows: {kl.tolist()} (another seed is needed)"
    r = records[0]
    limit = float(np.float32((float(kl[:r].max()) + float(kl[r])) / 2))
    assert float(kl[:r].max()) < limit < float(kl[r])
    tr = None
    try:
        tr = rh.trainer(_config(target_kl={"value": limit, "factor": 1.0, "host_check": "epoch"}, **KEY), seed=SEED, run_id="akl_stop")
        rows_g, _ = _update(tr)
        stop, state = dict(tr.last_kl_stop), rh.state(tr)
    finally:
        rh.release(tr)
    print(f"stop at row {r} of {kl.tolist()}, limit {limit}: {stop}")
    assert stop["stopped"] and stop["steps_applied"] == r and stop["steps_launched"] == r + N_MB and _bits32(stop["kl"]) == _bits32(kl[r])
    assert rows_g.shape == (r + 1, 6) and np.array_equal(rh.bits(rows_g), rh.bits(rows[0][: r + 1]))
    assert int(state["step"]) == r


def test_checkpoint_with_the_key_resumes_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = _config(**KEY)
    tr = fresh = None
    try:
        tr = rh.trainer(cfg, seed=SEED, run_id="akl_ckpt")
        _update(tr)
        path = tr.save_checkpoint()
        tr.restart_episodes(1)
        rec_a = rh.update(tr)
        means_a, old_a = tr.buffer.means.cpu().numpy().copy(), tr.buffer.old_log_std.cpu().numpy().copy()
        tr.load_checkpoint(path)
        rec_b = rh.update(tr)
        assert rh.differing(rec_a, rec_b) == []
        assert _same(tr.buffer.means, means_a) and _same(tr.buffer.old_log_std, old_a)
        fresh = rh.trainer(cfg, seed=999, run_id="akl_fresh", resume=path)
        assert fresh.update_index == 1 and fresh._kl_analytic
        rec_c = rh.update(fresh)
        assert rh.differing(rec_a, rec_c) == []
        assert _same(fresh.buffer.means, means_a) and _same(fresh.buffer.old_log_std, old_a)
    finally:
        rh.release(tr, fresh)


def test_refusals_raise_at_construction():
    from trainer import PPOTrainer

    def build(cfg, **kw):
        return PPOTrainer(cfg, run_id="akl_refused", device=rh.dev(), tensorboard=False, **kw)

    with pytest.raises(ValueError, match=r"kl_estimator must be one of .*write `k3` \(or remove the key\)"):
        build(_config(kl_estimator="exact"))
    with pytest.raises(ValueError, match=r"analytic without a Box .*categorical policies keep k3: remove the key"):
        build(rh.config(**KEY))
    dp = type("DP", (), {"world": 2, "rank": 0})()
    with pytest.raises(ValueError, match=r"analytic in a data-parallel run.*remove the key, or train on one device"):
        build(_config(normalize_observations=False, normalize_rewards=False, **KEY), dp=dp)
