"""The exact categorical KL (``exact_kl: true``) on the device: the four categorical sampling sites with every column's log-prob staged,
the three categorical loss routes with the KL sum, and the trainer in all three forms of the step.

Every comparison of a device KL with float64 (``utils.categorical_kl`` on the kernel's own logits) uses 4 x the largest error, over the
whole case list of the route, of a plain float32 torch evaluation of ``(p_old * (logp_old - logp_new)).sum(-1).mean() / B`` on the same
operands, measured again by every run of this file (the fixtures ``fused_cases`` / ``ppo_cases``: nothing is fixed in advance); both
errors are printed per case.  profiles/r18/exact_kl.txt records them as measured on the MI355X."""
import gc

import numpy as np
import pytest
import torch

import resume_helpers as rh

pytestmark = pytest.mark.gpu

LOGP_BOUND = 1.1e-6                      # tests/test_rollout_step_vs_float64.py: BOUNDS["logp"], a staged log-prob against float64
SENTINEL = -7.25
EINVAL, EUNSUPPORTED = -1, -2
NEG_INF = float("-inf")


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


def _offsets(sizes):
    return [sum(sizes[:b]) for b in range(len(sizes))]


def _valid(words, A):
    w = np.asarray(words).astype(np.int64).reshape(-1, 1)
    return ((w >> np.arange(A, dtype=np.int64)[None, :]) & 1).astype(bool)


def _pack(valid):
    return np.array([sum(1 << j for j in range(valid.shape[1]) if row[j]) for row in valid], dtype=np.int64)


def _log_softmax64(logits, sizes, valid=None):
    """float64 log-softmax per branch over the valid columns; -inf elsewhere."""
    x = np.asarray(logits, dtype=np.float64)
    out = np.full_like(x, -np.inf)
    for off, a in zip(_offsets(sizes), sizes):
        v = np.ones(x[..., off:off + a].shape, dtype=bool) if valid is None else valid[..., off:off + a]
        s = np.where(v, x[..., off:off + a], -np.inf)
        m = s.max(axis=-1, keepdims=True)
        out[..., off:off + a] = s - (m + np.log(np.exp(s - m).sum(axis=-1, keepdims=True)))
    return out


# ================================================================== the sampler, per site
LAYOUTS = [(3,), (2, 3), (4, 1, 3), (63,), (31, 32)]
S_SITE = 3                               # rows 0 / 1 or 1 / 2 are written by the two steps, the third keeps its sentinel
# the smallest shapes tests/test_rollout_step_vs_float64.py admits per site: the per-worker step kernel at D = 128, two heads, L = 32
# (its case a63); the group kernel at D = 128, one head, L = 32, GRU-gated pre-LN (g4_64) -- it takes at most 15 columns
# (the other two sites take their operands directly, through etm/ops.py)
SITE_MODEL = {"worker": dict(D=128, H=2, ln="post", gtrxl=False), "group": dict(D=128, H=1, ln="pre", gtrxl=True)}
SITE_CASES = [(site, br, masked, W) for site in ("sample", "policy", "worker", "group") for br in LAYOUTS for masked in (False, True)
              for W in (1, 8) if not (site == "group" and sum(br) > 15)]


def _site_words(br, W):
    """[W, S_SITE] words of the workers' three observations: all valid / one valid action per branch / first action invalid / last
    action invalid / random (tests/test_action_masks_gpu.py: crafted_words); worker 0's second observation leaves every branch one
    valid action."""
    import test_action_masks_gpu as mg
    return mg.crafted_words(br, range(W), S_SITE).view(np.int64)


def _site_draws(br, W, words, seed):
    """uniforms [W, S, B] (worker 0 of the second step greedy: -1) and forced [W, S, B] (-1 but worker W - 1 of the second step: the
    LAST valid action of every branch -- another action than a small uniform draws)."""
    g = torch.Generator().manual_seed(seed)
    B, A = len(br), sum(br)
    u = torch.rand((W, S_SITE, B), generator=g)
    forced = torch.full((W, S_SITE, B), -1, dtype=torch.int64)
    return u, forced


def _site_config(site, br, W, masked, key):
    m = SITE_MODEL[site]
    env = dict(type="Synthetic", obs_shape=[7], num_actions=list(br) if len(br) > 1 else int(br[0]), max_episode_steps=37, seed=3,
               p_done=0.01, pool=4)
    cfg = dict(environment=env, gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=W, worker_steps=S_SITE, n_mini_batch=1,
               value_loss_coefficient=0.5, hidden_layer_size=128, max_grad_norm=0.5, rollout_groups=1, rollout_min_group_size=2,
               hip_graph_rollout=False, hip_graph_train=False, tunable_gemm=False,
               transformer=dict(num_blocks=2, embed_dim=m["D"], num_heads=m["H"], memory_length=32, positional_encoding="relative",
                                layer_norm=m["ln"], gtrxl=m["gtrxl"], gtrxl_bias=1.0 if m["gtrxl"] else 0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    if masked:
        cfg["action_masks"] = True
    if key:
        cfg["exact_kl"] = True
    return cfg


def _site_passes(site, br, W, masked, key, passes, words):
    """The sampling site through a trainer's own eager step: two steps per pass on fixed observations at episode steps 0 and 1, the
    staging tables pre-filled with the sentinel.  ``passes``: (uniforms, forced) each -> one output dict per pass."""
    import test_action_masks_gpu as mg
    from etm import ops
    from trainer import PPOTrainer
    cfg = _site_config(site, br, W, masked, key)
    env = mg._crafted_env(br, W, 0, cfg["environment"], S_SITE + 1, words=words.view(np.uint64)) if masked else None
    torch.manual_seed(31)
    tr = PPOTrainer(cfg, run_id="ekl_site", device=_dev(), tensorboard=False, env=env)
    outs = []
    B, A = len(br), sum(br)
    try:
        assert tr.box is None and tr._kl_exact_cat == key and ("logps" in tr._stage) == key and (tr.buffer.old_logps is not None) == key
        assert tr._masked == masked and not tr._kl_analytic
        with torch.no_grad():
            for prm in tr.model.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
        obs = np.random.default_rng(5).normal(size=(2, W, 7)).astype(np.float32)
        g = tr._group_all
        main = torch.cuda.current_stream(tr.device)
        for uniforms, forced in passes:
            tr.worker_current_episode_step[:] = 0
            tr.obs[:] = obs[0]
            if masked:
                tr._am_np[:] = words[:, 0]
            sq = (lambda t: t[:, :, 0]) if B == 1 else (lambda t: t)
            plan, groups = tr._begin_rollout(main, sq(forced).contiguous(), sq(uniforms).contiguous(), None)
            assert groups == [g] and not plan.graph
            for table in tr._stage.values():
                if table.dtype == torch.float32:
                    table.fill_(SENTINEL)
            tr._stage["actions"].fill_(-5)
            host = []
            for step in range(2):
                tr.worker_current_episode_step[:] = step
                tr.obs[:] = obs[step]
                if masked:
                    tr._am_np[:] = words[:, step]
                tr._launch_eager(g, plan)
                torch.cuda.synchronize()
                host.append(tr._act_pin.numpy().copy())
            assert g.rf_scratch is not None and g.group_kernel == (site == "group"), "the step kernel of the site did not run"
            assert int(ops.rollout_trxl_error(g.rf_scratch).item()) == 0
            out = {k: tr._stage[k].cpu().numpy() for k in ("actions", "log_probs", "values") + (("logps",) if key else ())}
            out.update(host=np.stack(host), t=int(g.t_dev.item()))
            outs.append(out)
            tr._forced_tab.fill_(-1)
    finally:
        tr.close()
        del tr
        gc.collect()
        torch.cuda.synchronize()
    return outs


def _direct(site, br, W, masked, key, uniforms, forced, words, first_row):
    """Two steps (rows first_row, first_row + 1) of the ``sample`` / ``policy`` entries through etm/ops.py on fixed random operands ->
    every output as host arrays, and the kernel's own logits of both steps."""
    from etm import ops
    dev = _dev()
    B, A = len(br), sum(br)
    g = torch.Generator().manual_seed(1000 * A + W)
    hid = 64
    tm = lambda t: t.transpose(0, 1).contiguous().to(dev)          # [W, S, B] -> time-major
    st = dict(actions=torch.full((S_SITE, W, B), -5, dtype=torch.int64, device=dev), log_probs=torch.full((S_SITE, W, B), SENTINEL, device=dev),
              values=torch.full((S_SITE, W), SENTINEL, device=dev))
    if key:
        st["logps"] = torch.full((S_SITE, W, A), SENTINEL, device=dev)
    kw = dict(st_logps=st["logps"]) if key else {}
    t_dev = torch.full((), first_row, dtype=torch.int64, device=dev)
    act = torch.full((W, B), -5, dtype=torch.int64, device=dev)
    head, value_head = torch.nn.Linear(hid, A), torch.nn.Linear(hid, 1)
    with torch.no_grad():
        for m in (head, value_head):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) / hid ** 0.5 * 3.0)
            m.bias.copy_(0.5 * torch.randn(m.bias.shape, generator=g))
    head, value_head = head.to(dev), value_head.to(dev)
    u_t, f_t = tm(uniforms), tm(forced)
    host, logits = [], []
    for step in range(2):
        am = torch.as_tensor(words[:, first_row + step].copy(), device=dev) if masked else None
        if site == "sample":
            lg, value = (2.0 * torch.randn((W, A), generator=g)).to(dev), torch.randn(W, generator=g).to(dev)
            ops.rollout_sample(lg, value, u_t, f_t, t_dev, act, st["actions"], st["log_probs"], st["values"], branches=br, action_mask=am, **kw)
        else:
            h2 = torch.randn((W, 2 * hid), generator=g).to(dev)
            ops.rollout_policy(h2, head, value_head, u_t, f_t, t_dev, act, st["actions"], st["log_probs"], st["values"], branches=br,
                               action_mask=am, **kw)
            lg = ops.rollout_heads(h2, head, value_head)[0]          # the same dot products, wave by wave
        torch.cuda.synchronize()
        host.append(act.cpu().numpy().copy())
        logits.append(lg.reshape(W, A).cpu().numpy().copy())
    out = {k: v.cpu().numpy() for k, v in st.items()}
    out.update(host=np.stack(host), t=int(t_dev.item()), logits=np.stack(logits))
    return out


@pytest.mark.parametrize("site,br,masked,W", SITE_CASES,
                         ids=[f"{s}-{'_'.join(map(str, b))}-{'masked' if m else 'plain'}-W{w}" for s, b, m, w in SITE_CASES])
def test_site_stages_every_log_prob_and_keeps_every_other_bit(site, br, masked, W):
    B, A = len(br), sum(br)
    direct = site in ("sample", "policy")
    first = 1 if direct else 0                        # (the trainer's step counter restarts at 0)
    rows = (first, first + 1)
    spare = ({0, 1, 2} - set(rows)).pop()
    words = _site_words(br, W) if masked else np.full((W, S_SITE), (1 << A) - 1, dtype=np.int64)
    valid = _valid(words.reshape(-1), A).reshape(W, S_SITE, A)
    u, forced = _site_draws(br, W, words, 7 * A + W)
    # the second step: worker 0 greedy, worker W - 1 forced to the LAST valid action of every branch (W = 1: forced wins)
    w_f, step2 = W - 1, (1 if not direct else rows[1])
    u[0, rows[1]] = -1.0
    for b, (off, a) in enumerate(zip(_offsets(br), br)):
        # (the words of the direct sites are indexed by the staging row, the trainer sites' by the step)
        v = valid[w_f, step2, off:off + a]
        forced[w_f, rows[1], b] = int(np.flatnonzero(v)[-1])
    u2 = torch.rand(u.shape, generator=torch.Generator().manual_seed(99))
    free = torch.full_like(forced, -1)
    if direct:
        on = _direct(site, br, W, masked, True, u, forced, words, first)
        off_ = _direct(site, br, W, masked, False, u, forced, words, first)
        other = _direct(site, br, W, masked, True, u2, free, words, first)
        vrow = {r: valid[:, r] for r in rows}
    else:
        on, other = _site_passes(site, br, W, masked, True, [(u, forced), (u2, free)], words)
        off_, = _site_passes(site, br, W, masked, False, [(u, forced)], words)
        vrow = {r: valid[:, r] for r in rows}
    # 1. the twin's bits: staged actions, log-probs, values, the host's actions of both steps, the step counter
    for k in ("actions", "log_probs", "values", "host"):
        assert _same(on[k], off_[k]), (site, k)
    assert on["t"] == off_["t"] == first + 2
    acts = on["actions"].reshape(S_SITE, W, B)
    assert np.array_equal(acts[rows[1], w_f], forced[w_f, rows[1]].numpy()), "the forced row was honoured"
    lps, logp = on["logps"], on["log_probs"].reshape(S_SITE, W, B)
    for r in rows:
        for b, (off, a) in enumerate(zip(_offsets(br), br)):
            taken = acts[r, :, b]
            assert ((taken >= 0) & (taken < a)).all()
            # 2. the entry at the taken action is the staged log-prob, bit for bit
            assert _same(lps[r, np.arange(W), off + taken], logp[r, :, b]), (site, r, b)
        # 3. invalid columns are exactly -inf, valid ones finite
        assert np.isneginf(lps[r][~vrow[r]]).all() and np.isfinite(lps[r][vrow[r]]).all(), (site, r)
        # 4. a forced row and a greedy row store the policy's row: the rows of the same states under other draws, nothing forced
        assert _same(lps[r], other["logps"][r]), (site, r)
    # 5. the rows of other steps keep their sentinel
    for out in (on, other):
        assert np.all(out["logps"][spare] == np.float32(SENTINEL)) and np.all(out["log_probs"][spare] == np.float32(SENTINEL))
        assert np.all(out["values"][spare] == np.float32(SENTINEL)) and np.all(out["actions"][spare] == -5)
    # 6. every finite entry against a float64 log-softmax of the kernel's own logits.  The two entries that take or expose their logits
    # are held to those; a step kernel keeps its logits to itself, and what it stores is logit - lse, the logits up to one shift per
    # branch: the float64 log-softmax (which no shift changes) of the stored row itself
    worst = 0.0
    for i, r in enumerate(rows):
        src = on["logits"][i] if direct else np.where(vrow[r], lps[r], 0.0)
        ref = _log_softmax64(src, br, vrow[r])
        err = np.abs(lps[r].astype(np.float64)[vrow[r]] - ref[vrow[r]]) / np.maximum(np.abs(ref[vrow[r]]), 1.0)
        worst = max(worst, float(err.max()))
    print(f"[site {site} {br} masked={masked} W={W}] stored log-probs against float64: worst relative error {worst:.2e} (bound {LOGP_BOUND:.1e})")
    assert worst <= LOGP_BOUND


def test_logps_entries_refuse_a_missing_or_misaligned_table():
    """NULL / misaligned st_logps at the two entries that can be called without a model: ETM_EINVAL and nothing written; and the
    existence of all four entries."""
    from etm import lib as etm_lib
    lib = etm_lib.load()
    for name in ("etm_rollout_sample_branched_logps", "etm_rollout_policy_branched_logps", "etm_rollout_trxl_branched_logps",
                 "etm_rollout_trxl_group_branched_logps"):
        assert hasattr(lib, name), name
    dev = _dev()
    A, W = 5, 4
    import ctypes
    tab = (ctypes.c_int32 * 2)(2, 3)
    st_a, st_l = torch.full((S_SITE, W, 2), -5, dtype=torch.int64, device=dev), torch.full((S_SITE, W, 2), SENTINEL, device=dev)
    st_v, st_p = torch.full((S_SITE, W), SENTINEL, device=dev), torch.full((S_SITE, W, A), SENTINEL, device=dev)
    lg, value, u = torch.randn((W, A), device=dev), torch.randn(W, device=dev), torch.rand((S_SITE, W, 2), device=dev)
    t_dev = torch.zeros((), dtype=torch.int64, device=dev)
    act = torch.full((W, 2), -5, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    h2, wp, bp = torch.randn((W, 128), device=dev), torch.randn((A, 64), device=dev), torch.randn(A, device=dev)
    wv, bv, sync = torch.randn((1, 64), device=dev), torch.randn(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for bad in (0, st_p.data_ptr() + 2):
        rc = lib.etm_rollout_sample_branched_logps(lg.data_ptr(), value.data_ptr(), u.data_ptr(), None, t_dev.data_ptr(), act.data_ptr(),
                                                   st_a.data_ptr(), st_l.data_ptr(), st_v.data_ptr(), W, tab, 2, None, bad, stream)
        assert rc == EINVAL
        rc = lib.etm_rollout_policy_branched_logps(h2.data_ptr(), None, wp.data_ptr(), bp.data_ptr(), wv.data_ptr(), bv.data_ptr(),
                                                   u.data_ptr(), None, t_dev.data_ptr(), act.data_ptr(), st_a.data_ptr(), st_l.data_ptr(),
                                                   st_v.data_ptr(), None, None, sync.data_ptr(), W, 64, W, tab, 2, None, bad, stream)
        assert rc == EINVAL
    torch.cuda.synchronize()
    assert int(t_dev.item()) == 0 and bool((act == -5).all()) and bool((st_a == -5).all())
    assert all(bool((t == SENTINEL).all()) for t in (st_l, st_v, st_p))


# ================================================================== the loss
CLIP, VF, BETA = 0.2, 0.5, 0.01
NS = (1, 8, 9, 37, 2059)
FUSED_CASES = [(N, hid, br, masked) for N in NS for hid in (64, 512) for br in ((2,), (8,), (3, 3), (2, 1, 5)) for masked in (False, True)]
PPO_CASES = [(N, br, masked) for N in NS for br in ((12,), (63,), (5, 9), (31, 32)) for masked in (False, True)]


def _random_valid(N, br, g):
    """bool [N, A]: every branch keeps at least one action; sample 0's first branch keeps exactly one."""
    A = sum(br)
    v = torch.rand((N, A), generator=g) < 0.6
    for off, a in zip(_offsets(br), br):
        keep = torch.randint(0, a, (N,), generator=g)
        v[torch.arange(N), off + keep] = True
    v[0, :br[0]] = False
    v[0, 0] = True
    return v.numpy()


def _masked_log_softmax32(logits, br, valid):
    """float32 torch log-softmax per branch over the valid columns (-inf elsewhere): what a plain torch evaluation computes."""
    out = torch.full_like(logits, NEG_INF)
    v = torch.as_tensor(valid, device=logits.device)
    for off, a in zip(_offsets(br), br):
        out[:, off:off + a] = torch.log_softmax(logits[:, off:off + a].masked_fill(~v[:, off:off + a], NEG_INF), dim=-1)
    return out


def _torch_kl32(old_logps, logits, br, valid):
    """(p_old * (logp_old - logp_new)).sum(-1).mean() / B as plain float32 torch operations (invalid columns left out)."""
    v = torch.as_tensor(valid, device=logits.device)
    new = _masked_log_softmax32(logits, br, valid)
    zero = torch.zeros_like(new)
    term = torch.where(v, old_logps.exp() * (torch.where(v, old_logps, zero) - torch.where(v, new, zero)), zero)
    return float((term.sum(-1).mean() / len(br)).item())


def _old_rows(logits, br, valid, g, dev):
    """Old log-probs [N, A]: the float32 log-softmax of perturbed logits over the valid columns (normalised rows: the rule and the
    plain definition agree only on those); sample N - 1 carries the d < -60 case -- the last valid column of its first branch, where
    it has another one, lies 200 below the branch's largest perturbed logit, so its old log-prob is about -200."""
    pert = logits + (0.4 * torch.randn(logits.shape, generator=g)).to(dev)
    n = logits.shape[0] - 1
    cols = np.flatnonzero(valid[n, :br[0]])
    if len(cols) > 1:
        pert[n, int(cols[-1])] = float(pert[n, cols[:-1].tolist()].max()) - 200.0
    return _masked_log_softmax32(pert, br, valid).contiguous()


def _sampler_rows(logits, br, words):
    """Every column's log-prob of the rows ``logits`` [N, A] as the SAMPLER stores it (one rollout_sample launch with W = N workers):
    lg[j] - lse in the arithmetic the loss kernels repeat on equal logits."""
    from etm import ops
    dev = logits.device
    N, A, B = logits.shape[0], logits.shape[1], len(br)
    st = dict(a=torch.zeros((1, N, B), dtype=torch.int64, device=dev), l=torch.zeros((1, N, B), device=dev), v=torch.zeros((1, N), device=dev),
              p=torch.full((1, N, A), SENTINEL, device=dev))
    ops.rollout_sample(logits.contiguous(), torch.zeros(N, device=dev), torch.full((1, N, B), 0.5, device=dev), None,
                       torch.zeros((), dtype=torch.int64, device=dev), torch.zeros((N, B), dtype=torch.int64, device=dev), st["a"], st["l"],
                       st["v"], branches=br, action_mask=words, st_logps=st["p"])
    torch.cuda.synchronize()
    return st["p"][0].contiguous()


class _Fused:
    """The operands of one categorical heads + loss problem on the device and its entries through the C ABI."""

    def __init__(self, N, hid, br, masked, seed=None):
        from etm import lib as etm_lib
        from etm import ops
        import ctypes
        self.lib, self.N, self.hid, self.br, self.masked = etm_lib.load(), N, hid, tuple(br), masked
        self.A, self.B = sum(br), len(br)
        dev = _dev()
        g = torch.Generator().manual_seed(seed if seed is not None else 13 * N + 5 * hid + 7 * self.A + self.B)
        self.g = g
        r = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev)
        A, B = self.A, self.B
        self.pre_p, self.pre_v = r(N, hid), r(N, hid)
        self.b_lp, self.b_lv = r(hid, s=0.1), r(hid, s=0.1)
        self.wb, self.bb, self.wv, self.bv = r(A, hid, s=2.0 * hid ** -0.5), r(A, s=0.3), r(hid, s=hid ** -0.5), r(1, s=0.1)
        self.adv, self.old_value = r(N), r(N)
        self.stats3 = ops.adv_stats(self.adv)
        self.valid = _random_valid(N, br, g) if masked else np.ones((N, A), dtype=bool)
        self.words = torch.as_tensor(_pack(self.valid), device=dev)
        acts = torch.zeros((N, B), dtype=torch.int64)
        for b, (off, a) in enumerate(zip(_offsets(br), br)):        # a valid action per branch
            score = torch.rand((N, a), generator=g) + torch.as_tensor(self.valid[:, off:off + a]).float()
            acts[:, b] = score.argmax(dim=1)
        self.actions = acts.to(dev).contiguous()
        self.old_logp = torch.zeros((N, B), device=dev)
        self.tab = (ctypes.c_int32 * B)(*br)
        self.logits = self.twin()["logits"]                          # the kernel's own logits (they do not depend on the log-probs)
        self.new32 = _masked_log_softmax32(self.logits, br, self.valid)
        lp = torch.stack([self.new32[torch.arange(N), off + self.actions[:, b]] for b, off in enumerate(_offsets(br))], dim=1)
        self.old_logp = (lp - r(N, B, s=0.05)).contiguous()
        self.old_logps = _old_rows(self.logits, br, self.valid, g, dev)

    def _outputs(self, row):
        dev, N, hid, A = _dev(), self.N, self.hid, self.A
        f = lambda *shape: torch.full(shape, SENTINEL, device=dev)
        return dict(gm_p=f(N, hid), gm_v=f(N, hid), sums=f(row), out8=f(8), logits=f(N, A), value=f(N))

    def _head(self, o, ws):
        p = lambda t: t.data_ptr()
        B = self.B
        return (p(self.pre_p), p(self.pre_v), p(self.b_lp), p(self.b_lv), p(self.wb), p(self.bb), p(self.wv), p(self.bv), p(self.actions), B,
                p(self.old_logp), B, p(self.adv), p(self.old_value), p(self.stats3), CLIP, VF, BETA, 1.0 / (self.N * B), 1.0 / self.N,
                1.0 / self.N, None, p(o["gm_p"]), p(o["gm_v"]), p(o["sums"]), p(o["out8"]), p(o["logits"]), p(o["value"]), p(ws), ws.numel(),
                self.N, self.hid)

    def _shape(self):
        return (self.A,) if self.B == 1 else (self.tab, self.B)

    def twin(self):
        lib = self.lib
        o = self._outputs(lib.etm_heads_loss_row_floats(self.hid, self.A))
        ws = torch.empty(lib.etm_heads_loss_workspace_bytes(self.N, self.hid, self.A), dtype=torch.uint8, device=_dev())
        stream = torch.cuda.current_stream().cuda_stream
        head = self._head(o, ws) + self._shape()
        if self.masked:
            entry = lib.etm_heads_loss_masked if self.B == 1 else lib.etm_heads_loss_branched_masked
            rc = entry(*head, self.words.data_ptr(), stream)
        else:
            entry = lib.etm_heads_loss if self.B == 1 else lib.etm_heads_loss_branched
            rc = entry(*head, stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return o

    def kl(self, old_logps=None, stride=None, expect=0, hid=None, raw_ptr=None):
        lib = self.lib
        old_logps = self.old_logps if old_logps is None else old_logps
        o = self._outputs(lib.etm_heads_loss_kl_row_floats(self.hid, self.A))
        ws = torch.full((max(lib.etm_heads_loss_kl_workspace_bytes(self.N, self.hid, self.A), 4),), 0x5A, dtype=torch.uint8, device=_dev())
        head = list(self._head(o, ws))
        if hid is not None:
            head[-1] = hid
        entry = lib.etm_heads_loss_kl if self.B == 1 else lib.etm_heads_loss_branched_kl
        rc = entry(*head, *self._shape(), self.words.data_ptr() if self.masked else None,
                   old_logps.data_ptr() if raw_ptr is None else raw_ptr, old_logps.stride(0) if stride is None else stride,
                   torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, expect)
        torch.cuda.synchronize()
        o["ws"] = ws
        return o

    def kl64(self, logits, old_logps=None):
        from utils import categorical_kl
        old = self.old_logps if old_logps is None else old_logps
        return float(categorical_kl(old.cpu().numpy(), logits.cpu().numpy(), self.br, _pack(self.valid) if self.masked else None, np.float64))


@pytest.fixture(scope="module")
def fused_cases():
    """Every case once: the two entries' outputs, the float64 KL on the kernel's own logits, the error of the float32 torch evaluation
    and of the kernel -> ({case: record}, the bound: 4 x the largest torch error over the list)."""
    out = {}
    for case in FUSED_CASES:
        p = _Fused(*case)
        twin, kl = p.twin(), p.kl()
        ref = p.kl64(kl["logits"])
        out[case] = dict(p=p, twin=twin, kl=kl, ref=ref, torch_err=abs(_torch_kl32(p.old_logps, kl["logits"], p.br, p.valid) - ref),
                         kernel_err=abs(float(kl["out8"][4]) - ref))
    worst_torch, worst_kernel = max(r["torch_err"] for r in out.values()), max(r["kernel_err"] for r in out.values())
    for case, r in out.items():
        print(f"[fused N={case[0]} hid={case[1]} br={case[2]} masked={case[3]}] kl64 {r['ref']:.9e} torch fp32 error {r['torch_err']:.3e} "
              f"kernel error {r['kernel_err']:.3e}")
    print(f"[fused] largest float32 torch error {worst_torch:.3e}, largest kernel error {worst_kernel:.3e}; bound = 4 x {worst_torch:.3e}")
    return out, 4.0 * worst_torch


def _fid(c):
    return f"N{c[0]}_hid{c[1]}_{'x'.join(map(str, c[2]))}_{'masked' if c[3] else 'plain'}"


@pytest.mark.parametrize("case", FUSED_CASES, ids=[_fid(c) for c in FUSED_CASES])
def test_fused_loss_keeps_the_twins_bits_and_reduces_the_exact_kl(fused_cases, case):
    N, hid, br, masked = case
    A, B = sum(br), len(br)
    r = fused_cases[0][case]
    twin, kl = r["twin"], r["kl"]
    row = (3 + A) * hid + A + 1 + 5
    assert twin["sums"].numel() == row and kl["sums"].numel() == row + 1
    for k in ("gm_p", "gm_v", "logits", "value"):
        assert _same(twin[k], kl[k]), k
    assert _same(twin["sums"], kl["sums"][:row]), "every element of the old row"
    t8, k8 = _bits(twin["out8"]), _bits(kl["out8"])
    assert np.array_equal(t8[[0, 1, 2, 3, 5, 7]], k8[[0, 1, 2, 3, 5, 7]]), "policy, value, loss, entropy, clip fraction"
    assert k8[6] == t8[4], "the k3 value moves to out8[6]"
    assert float(twin["out8"][6]) == 0.0
    got = float(kl["out8"][4])
    assert got >= 0.0
    assert abs(got - r["ref"]) <= fused_cases[1], (got, r["ref"], fused_cases[1])
    # the raw sum at the end of the row is what out8[4] scales (pol_scale = 1 / (N B))
    assert abs(float(kl["sums"][row]) / (N * B) - got) <= 2 * float(np.spacing(np.float32(got)))


@pytest.mark.parametrize("case", [(1, 64, (2,), False), (9, 512, (2, 1, 5), True), (2059, 64, (3, 3), False), (37, 512, (8,), True)],
                         ids=_fid)
def test_fused_loss_equal_policies_give_exactly_zero(case):
    """The old rows are what the sampler stages for the loss kernel's own logits: the two repeat one arithmetic (max, sum of exp in
    column order, log, lg[j] - lse), so every d_j is exactly 0 and so is the statistic."""
    p = _Fused(*case)
    old = _sampler_rows(p.logits, p.br, p.words if p.masked else None)
    assert np.isneginf(old.cpu().numpy()[~p.valid]).all() and np.isfinite(old.cpu().numpy()[p.valid]).all()
    o = p.kl(old_logps=old)
    assert _same(o["logits"], p.logits)
    assert _bits(o["out8"])[4] == 0, float(o["out8"][4])
    assert float(o["sums"][-1]) == 0.0


@pytest.mark.parametrize("hid", [64, 512])
def test_fused_loss_constant_mask_equals_the_compacted_call(hid):
    """A constant mask gives the bits of the unmasked call on the compacted branches."""
    N, br = 37, (2, 1, 5)
    keep = np.array([True, False, True, True, False, True, True, False])
    br_c = (1, 1, 3)
    p = _Fused(N, hid, br, True)
    p.valid = np.broadcast_to(keep, (N, 8)).copy()
    p.words = torch.as_tensor(_pack(p.valid), device=_dev())
    # actions inside the kept columns, old rows over them
    idx = [np.flatnonzero(keep[off:off + a]) for off, a in zip(_offsets(br), br)]
    g = torch.Generator().manual_seed(5)
    comp = torch.stack([torch.randint(0, len(ix), (N,), generator=g) for ix in idx], dim=1)
    p.actions = torch.stack([torch.as_tensor(ix)[comp[:, b]] for b, ix in enumerate(idx)], dim=1).to(_dev()).contiguous()
    p.old_logps = _masked_log_softmax32(p.logits + 0.3, br, p.valid).contiguous()
    full = p.kl()
    q = _Fused(N, hid, br_c, False)
    kcols = torch.as_tensor(np.flatnonzero(keep), device=_dev())
    q.pre_p, q.pre_v, q.b_lp, q.b_lv, q.wv, q.bv = p.pre_p, p.pre_v, p.b_lp, p.b_lv, p.wv, p.bv
    q.wb, q.bb = p.wb[kcols].contiguous(), p.bb[kcols].contiguous()
    q.adv, q.old_value, q.stats3, q.old_logp = p.adv, p.old_value, p.stats3, p.old_logp
    q.actions = comp.to(_dev()).contiguous()
    q.old_logps = p.old_logps[:, kcols].contiguous()
    small = q.kl()
    assert _same(full["out8"], small["out8"]) and _same(full["gm_p"], small["gm_p"]) and _same(full["gm_v"], small["gm_v"])
    assert _same(full["sums"][-1], small["sums"][-1])


def test_fused_loss_refusals_write_nothing():
    p = _Fused(9, 64, (3, 3), True)
    tries = [dict(raw_ptr=0, expect=EINVAL), dict(raw_ptr=p.old_logps.data_ptr() + 2, expect=EINVAL), dict(stride=5, expect=EINVAL),
             dict(hid=100, expect=EUNSUPPORTED), dict(hid=576, expect=EUNSUPPORTED)]
    q = _Fused(9, 64, (8,), False)
    for prob, kws in ((p, tries), (q, tries[:3] + [dict(stride=7, expect=EINVAL)] + tries[3:])):
        for kw in kws:
            o = prob.kl(**kw)
            for k, t in o.items():
                assert bool((t == (0x5A if k == "ws" else SENTINEL)).all()), (kw, k)
    # and the op: the rows come with the minibatch's shape; None is the call of ever
    from etm import ops
    dev = _dev()
    lin = lambda i, o_: torch.nn.Linear(i, o_).to(dev)
    h = torch.randn((9, 64), device=dev)
    args = (h, lin(64, 64), lin(64, 64), [lin(64, 3), lin(64, 3)], lin(64, 1), p.actions, p.old_logp, p.adv, p.old_value, CLIP, VF, BETA)
    with pytest.raises(ValueError, match=r"old_logps must be float32 \[9, 6\]"):
        ops.heads_ppo_loss(*args, old_logps=p.old_logps[:, :5])
    loss, st = ops.heads_ppo_loss(*args, action_mask=p.words, old_logps=p.old_logps)
    loss_t, st_t = ops.heads_ppo_loss(*args, action_mask=p.words)
    assert st.shape == (6,) and _same(loss, loss_t) and _same(st[[0, 1, 2, 3, 5]], st_t[[0, 1, 2, 3, 5]])


# ------------------------------------------------------------------ the separate-heads route (etm_ppo_loss_kl, one branch per call)
class _Ppo:
    def __init__(self, N, br, masked):
        from etm import lib as etm_lib
        from etm import ops
        self.lib, self.N, self.br, self.masked = etm_lib.load(), N, tuple(br), masked
        self.A, self.B = sum(br), len(br)
        dev = _dev()
        g = torch.Generator().manual_seed(17 * N + 3 * self.A + self.B)
        r = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev)
        N, A, B = self.N, self.A, self.B
        self.logits = r(N, A, s=1.5)
        self.value, self.old_value, self.adv = r(N), r(N), r(N)
        self.stats3 = ops.adv_stats(self.adv)
        self.valid = _random_valid(N, br, g) if masked else np.ones((N, A), dtype=bool)
        self.words = torch.as_tensor(_pack(self.valid), device=dev)
        acts = torch.zeros((N, B), dtype=torch.int64)
        for b, (off, a) in enumerate(zip(_offsets(br), br)):
            score = torch.rand((N, a), generator=g) + torch.as_tensor(self.valid[:, off:off + a]).float()
            acts[:, b] = score.argmax(dim=1)
        self.actions = acts.to(dev).contiguous()
        new32 = _masked_log_softmax32(self.logits, br, self.valid)
        lp = torch.stack([new32[torch.arange(N), off + self.actions[:, b]] for b, off in enumerate(_offsets(br))], dim=1)
        self.old_logp = (lp - r(N, B, s=0.05)).contiguous()
        self.old_logps = _old_rows(self.logits, br, self.valid, g, dev)

    def branch(self, b, kl, raw_ptr=None, stride=None, off_arg=None, expect=0):
        """One branch through etm_ppo_loss / _masked (kl False) or etm_ppo_loss_kl -> outputs."""
        lib, dev, N = self.lib, _dev(), self.N
        off, a = _offsets(self.br)[b], self.br[b]
        lg = self.logits[:, off:off + a].contiguous()
        nbytes = lib.etm_ppo_loss_workspace_bytes(N)
        o = dict(out8=torch.full((8,), SENTINEL, device=dev), d_logits=torch.full((N, a), SENTINEL, device=dev),
                 d_value=torch.full((N,), SENTINEL, device=dev), ws=torch.full((nbytes // 4,), SENTINEL, device=dev))
        p = lambda t: t.data_ptr()
        args = (p(lg), p(self.actions) + 8 * b, self.B, p(self.old_logp) + 4 * b, self.B, p(self.adv), p(self.old_value), p(self.value),
                p(self.stats3), CLIP, VF, BETA, 1.0 / (N * self.B), 1.0 / N, 1.0 / N, 1 if b == 0 else 0, p(o["out8"]), p(o["d_logits"]),
                p(o["d_value"]), p(o["ws"]), nbytes, None, N, a)
        stream = torch.cuda.current_stream().cuda_stream
        am = p(self.words) if self.masked else None
        if kl:
            rc = lib.etm_ppo_loss_kl(*args, am, off if self.masked else 0, p(self.old_logps) if raw_ptr is None else raw_ptr,
                                     self.old_logps.stride(0) if stride is None else stride, off if off_arg is None else off_arg, stream)
        elif self.masked:
            rc = lib.etm_ppo_loss_masked(*args, am, off, stream)
        else:
            rc = lib.etm_ppo_loss(*args, stream)
        assert rc == expect, (rc, expect)
        torch.cuda.synchronize()
        return o


@pytest.fixture(scope="module")
def ppo_cases():
    from utils import categorical_kl
    out = {}
    for case in PPO_CASES:
        p = _Ppo(*case)
        twins = [p.branch(b, False) for b in range(p.B)]
        kls = [p.branch(b, True) for b in range(p.B)]
        got = float(sum(float(o["out8"][4]) for o in kls))            # (ops.ppo_loss adds the branches' statistics the same way)
        ref = float(categorical_kl(p.old_logps.cpu().numpy(), p.logits.cpu().numpy(), p.br, _pack(p.valid) if p.masked else None, np.float64))
        out[case] = dict(p=p, twins=twins, kls=kls, ref=ref, got=got, torch_err=abs(_torch_kl32(p.old_logps, p.logits, p.br, p.valid) - ref),
                         kernel_err=abs(got - ref))
    worst_torch, worst_kernel = max(r["torch_err"] for r in out.values()), max(r["kernel_err"] for r in out.values())
    for case, r in out.items():
        print(f"[ppo N={case[0]} br={case[1]} masked={case[2]}] kl64 {r['ref']:.9e} torch fp32 error {r['torch_err']:.3e} kernel error {r['kernel_err']:.3e}")
    print(f"[ppo] largest float32 torch error {worst_torch:.3e}, largest kernel error {worst_kernel:.3e}; bound = 4 x {worst_torch:.3e}")
    return out, 4.0 * worst_torch


@pytest.mark.parametrize("case", PPO_CASES, ids=[f"N{c[0]}_{'x'.join(map(str, c[1]))}_{'masked' if c[2] else 'plain'}" for c in PPO_CASES])
def test_ppo_loss_keeps_the_twins_bits_and_reduces_the_exact_kl(ppo_cases, case):
    r = ppo_cases[0][case]
    for b, (twin, kl) in enumerate(zip(r["twins"], r["kls"])):
        assert _same(twin["d_logits"], kl["d_logits"]), b
        if b == 0:
            assert _same(twin["d_value"], kl["d_value"])
        t8, k8 = _bits(twin["out8"]), _bits(kl["out8"])
        assert np.array_equal(t8[[0, 1, 2, 3, 5, 7]], k8[[0, 1, 2, 3, 5, 7]]), b
        assert k8[6] == t8[4] and float(twin["out8"][6]) == 0.0
        n_blocks = (case[0] + 255) // 256
        tw, kw = twin["ws"].view(n_blocks, 8), kl["ws"].view(n_blocks, 8)
        assert _same(tw[:, :5], kw[:, :5]), "partial slots 0..4"
        assert bool((tw[:, 5:] == SENTINEL).all()) and bool((kw[:, 6:] == SENTINEL).all()), "slot 5 is the KL's, 6 and 7 stay free"
        assert float(kl["out8"][4]) >= 0.0
    assert abs(r["got"] - r["ref"]) <= ppo_cases[1], (r["got"], r["ref"], ppo_cases[1])


def test_ppo_loss_equal_policies_constant_mask_and_refusals():
    # the op over branches: None is the call of ever; with the rows, stats[4] is the sum of the branches' exact KLs
    from etm import ops
    p = _Ppo(37, (5, 9), True)
    lgs = [p.logits[:, :5].contiguous().requires_grad_(True), p.logits[:, 5:].contiguous().requires_grad_(True)]
    a = ops.ppo_loss(lgs, p.value, p.actions, p.old_logp, p.adv, p.old_value, CLIP, VF, BETA, action_mask=p.words)
    b = ops.ppo_loss(lgs, p.value, p.actions, p.old_logp, p.adv, p.old_value, CLIP, VF, BETA, action_mask=p.words, old_logps=p.old_logps)
    assert _same(a[0], b[0]) and _same(a[1][[0, 1, 2, 3, 5]], b[1][[0, 1, 2, 3, 5]]) and not _same(a[1][4], b[1][4])
    want = float(p.branch(0, True)["out8"][4]) + float(p.branch(1, True)["out8"][4])
    assert abs(float(b[1][4]) - want) <= float(np.spacing(np.float32(want)))
    # a constant mask gives the bits of the unmasked call on the compacted branch
    N = 37
    q = _Ppo(N, (12,), True)
    keep = np.zeros(12, dtype=bool)
    keep[[0, 3, 4, 7, 11]] = True
    q.valid = np.broadcast_to(keep, (N, 12)).copy()
    q.words = torch.as_tensor(_pack(q.valid), device=_dev())
    g = torch.Generator().manual_seed(3)
    comp = torch.randint(0, 5, (N, 1), generator=g)
    q.actions = torch.as_tensor(np.flatnonzero(keep))[comp].to(_dev()).contiguous()
    q.old_logps = _masked_log_softmax32(q.logits * 0.7, (12,), q.valid).contiguous()
    full = q.branch(0, True)
    c = _Ppo(N, (5,), False)
    kcols = torch.as_tensor(np.flatnonzero(keep), device=_dev())
    c.logits, c.value, c.old_value, c.adv, c.stats3, c.old_logp = q.logits[:, kcols].contiguous(), q.value, q.old_value, q.adv, q.stats3, q.old_logp
    c.actions, c.old_logps = comp.to(_dev()).contiguous(), q.old_logps[:, kcols].contiguous()
    small = c.branch(0, True)
    assert _same(full["out8"], small["out8"]) and _same(full["d_logits"][:, kcols], small["d_logits"]) and _same(full["d_value"], small["d_value"])
    # equal policies (the sampler's rows of the same logits, see the fused test): exactly 0, masked or not
    for e in (_Ppo(2059, (31, 32), False), _Ppo(37, (5, 9), True), _Ppo(1, (63,), False)):
        e.old_logps = _sampler_rows(e.logits, e.br, e.words if e.masked else None)
        for b_ in range(e.B):
            assert _bits(e.branch(b_, True)["out8"])[4] == 0, (e.N, e.br, b_)
    # refusals: nothing is written
    for kw in (dict(raw_ptr=0), dict(raw_ptr=p.old_logps.data_ptr() + 1), dict(stride=13), dict(off_arg=-1), dict(off_arg=6)):
        o = p.branch(1, True, expect=EINVAL, **kw)
        assert all(bool((t == SENTINEL).all()) for t in o.values()), kw


# ================================================================== the trainer
FORMS = {"captured, tables": {}, "captured, no tables": {"step_ends_fused": False}, "eager": rh.modes(False)}
SCHED = dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10)
SEED, UPDATES, EPOCHS, N_MB = 11, 2, 3, 2
KEY = {"exact_kl": True}
POLICIES = {
    "discrete": dict(br=(3,), over={}),
    "masked multidiscrete": dict(br=(2, 3), over={"action_masks": True}, env={"num_actions": [2, 3], "action_mask_p": 0.3}),
    "discrete, separate heads": dict(br=(3,), over={"fused_heads_loss": False}),
}
_CACHE = {}


def _config(policy="discrete", form="captured, tables", **over):
    """The tiny trainer of tests/resume_helpers.py with the policy's action space."""
    pol = POLICIES[policy]
    env = dict(type="Synthetic", obs_shape=[rh.F_OBS], num_actions=3, max_episode_steps=16, seed=2, p_done=0.1, pool=4)
    env.update(pol.get("env", {}))
    return rh.config(**{"environment": env, "learning_rate_schedule": dict(SCHED), "n_mini_batch": N_MB, "epochs": EPOCHS, **FORMS[form],
                        **pol["over"], **over})


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


def _eager_logits(tr, idx):
    """The logits of the minibatch ``idx`` on the trainer's current weights, by the model's own eager forward."""
    from etm.ops import WindowSpec
    mb = tr.buffer.gather(idx)
    m = tr.model
    with torch.no_grad():
        spec = WindowSpec.from_bank(mb["memories"], mb["memory_index"], mb["memory_indices"], mb["memory_indices"], mb["memory_mask"])
        h, _ = m.forward_state(mb["obs"], spec)
        hp = torch.relu(torch.nn.functional.linear(h, m.lin_policy.weight, m.lin_policy.bias))
        lg = torch.cat([torch.nn.functional.linear(hp, br.weight, br.bias) for br in m.policy_branches], dim=1)
    return lg, mb


def _stepwise_update(tr, br):
    """The update ``_update`` would run, one minibatch step at a time from outside ``_train_epochs``, with the float64 KL and the float32
    torch evaluation of every step taken BEFORE it on the pre-step weights -> (statistics rows, float64 KL per row, torch error per row)."""
    from utils import categorical_kl
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    perms = _perms(tr.update_index)
    mbs = tr.buffer.batch_size // N_MB
    with torch.no_grad():
        tr._bank_pos = tr._bank_with_positions()
        tr._obs_train = tr._training_observations()
    monitor = tr.config.get("monitor_gradients", True)
    rows, ref, terr = [], [], []
    for i in range(EPOCHS * N_MB):
        perm = torch.as_tensor(perms[i // N_MB], device=tr.device, dtype=torch.long).view(-1, mbs).sort(dim=1).values
        idx = perm[i % N_MB].contiguous()
        lg, mb = _eager_logits(tr, idx)
        words = mb["action_masks"].cpu().numpy() if "action_masks" in mb else None
        valid = _valid(words, sum(br)) if words is not None else np.ones(tuple(lg.shape), dtype=bool)
        ref.append(float(categorical_kl(mb["old_logps"].cpu().numpy(), lg.cpu().numpy(), br, words, np.float64)))
        terr.append(abs(_torch_kl32(mb["old_logps"], lg, br, valid) - ref[-1]))
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
    return np.stack(rows), np.asarray(ref), np.asarray(terr)


def _plain_run(policy, form, key):
    """Two updates of the key-absent (``key`` False) or key-on trainer without a KL rule -> (rows per update, norms, state, extras)."""
    name = ("plain", policy, form, key)
    if name not in _CACHE:
        tr = None
        try:
            tr = rh.trainer(_config(policy, form, **(KEY if key else {})), seed=SEED, run_id="ekl_plain")
            assert tr.box is None and tr._kl_exact_cat == key and tr.action_space_shape == POLICIES[policy]["br"]
            rows, norms, extra = [], [], []
            for _ in range(UPDATES):
                r, n = _update(tr)
                rows.append(r), norms.append(n)
                if key:
                    extra.append(dict(old=tr.buffer.old_logps.cpu().numpy().copy(), stage=tr._stage["logps"].cpu().numpy().copy(),
                                      flat=tr.buffer.samples_flat["old_logps"].cpu().numpy().copy(),
                                      actions=tr.buffer.actions.cpu().numpy().copy(), log_probs=tr.buffer.log_probs.cpu().numpy().copy()))
            assert (tr._train_graph is not None) == (form != "eager")
            if not key:
                assert tr.buffer.old_logps is None and "logps" not in tr._stage and "old_logps" not in tr.buffer.samples_flat
            _CACHE[name] = (rows, norms, rh.state(tr), extra)
        finally:
            rh.release(tr)
    return _CACHE[name]


PLAIN = [(p, f) for p in ("discrete", "masked multidiscrete") for f in FORMS] + [("discrete, separate heads", "captured, tables")]


@pytest.mark.parametrize("policy,form", PLAIN)
def test_key_on_without_a_rule_changes_column_4_only(fused_cases, policy, form):
    br = POLICIES[policy]["br"]
    A, B = sum(br), len(br)
    rows_a, norms_a, state_a, _ = _plain_run(policy, form, False)
    rows_b, norms_b, state_b, extra = _plain_run(policy, form, True)
    assert rh.differing(state_a, state_b) == [] and int(state_b["step"]) == UPDATES * EPOCHS * N_MB
    others = [0, 1, 2, 3, 5]
    for u in range(UPDATES):
        assert rows_a[u].shape == rows_b[u].shape == (EPOCHS * N_MB, 6) and norms_a[u] == norms_b[u]
        assert np.array_equal(rh.bits(rows_a[u][:, others]), rh.bits(rows_b[u][:, others])), u
        assert not np.array_equal(rh.bits(rows_a[u][:, 4]), rh.bits(rows_b[u][:, 4])), "column 4 holds another statistic"
        e = extra[u]
        assert np.array_equal(rh.bits(e["old"]), rh.bits(e["stage"].transpose(1, 0, 2))), "buffer.old_logps is the staging table transposed"
        assert np.array_equal(rh.bits(e["flat"]), rh.bits(e["old"].reshape(-1, A)))
        # the entry at the taken action is the buffer's log-prob, bit for bit
        acts, lps = e["actions"].reshape(rh.W_T, rh.S_T, B), e["log_probs"].reshape(rh.W_T, rh.S_T, B)
        for b, off in enumerate(_offsets(br)):
            picked = np.take_along_axis(e["old"], (off + acts[:, :, b])[:, :, None], axis=2)[:, :, 0]
            assert np.array_equal(rh.bits(picked), rh.bits(lps[:, :, b])), (u, b)
    # the first step of every update sees the rollout's own policy: the exact KL of equal policies
    first = [float(rows_b[u][0, 4]) for u in range(UPDATES)]
    print(f"{policy} / {form}: first-step exact kl of each update {first} (k3 {[float(rows_a[u][0, 4]) for u in range(UPDATES)]})")
    # column 4 against float64 on the update's own buffer, the new logits by an eager forward on the pre-step weights
    tr = None
    try:
        tr = rh.trainer(_config(policy, form, **KEY), seed=SEED, run_id="ekl_stepwise")
        for u in range(UPDATES):
            rows_s, ref, terr = _stepwise_update(tr, br)
            assert np.array_equal(rh.bits(rows_s), rh.bits(rows_b[u])), (policy, form, u)
            err = np.abs(rows_s[:, 4].astype(np.float64) - ref)
            bound = fused_cases[1]                # (4 x the float32 torch error observed over the loss list, as every device KL here)
            print(f"{policy} / {form}: update {u} exact kl rows {rows_s[:, 4].tolist()} float64 {ref.tolist()} k3 rows {rows_a[u][:, 4].tolist()} "
                  f"worst error {err.max():.3e}, float32 torch error on these rows {terr.max():.3e} (bound {bound:.3e})")
            assert (rows_s[:, 4] >= 0).all()
            assert err.max() <= bound, (policy, form, u, err.max(), bound)
        assert rh.differing(rh.state(tr), state_b) == []
    finally:
        rh.release(tr)


def _walk(kl_rows, lr, rule):
    """The host model of tests/test_adaptive_lr_gpu.py over one update's kl rows."""
    from utils import adaptive_lr_step
    rates, raises, cuts = [], 0, 0
    for kl in np.asarray(kl_rows, dtype=np.float32):
        lr, way = adaptive_lr_step(lr, kl, rule)
        raises, cuts = raises + (way == 1), cuts + (way == -1)
        rates.append(np.float32(lr))
    return rates, np.float32(lr), raises, cuts


def _band(policy):
    """A band from the key-on probe's column-4 rows of its first update (the method of tests/test_adaptive_lr_gpu.py): row 1 -- the first
    real KL -- lies below kl_low and raises the rate, kl_high lies between it and the largest later row."""
    if ("band", policy) not in _CACHE:
        kl = _plain_run(policy, "captured, tables", True)[0][0][:, 4]
        print("probe exact kl (n_mini_batch 2, epochs 3):", kl.tolist())
        later = float(kl[2:].max())
        assert 0 < float(kl[1]) < later, f"row 1 must be a real kl below a later row's: {kl.tolist()} (another seed is needed)"
        kl_low = np.float32(float(kl[1]) + 0.25 * (later - float(kl[1])))
        kl_high = np.float32(float(kl[1]) + 0.5 * (later - float(kl[1])))
        assert float(kl[1]) < kl_low < kl_high < later
        _CACHE[("band", policy)] = {"desired_kl": 1.0, "low": float(kl_low), "high": float(kl_high)}
    return _CACHE[("band", policy)]


def _bits32(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("policy,form", [("discrete", "captured, tables"), ("discrete", "eager"), ("masked multidiscrete", "captured, no tables")])
def test_adaptive_lr_decides_on_the_exact_kl(policy, form):
    """The run equals utils.adaptive_lr_step walked over the run's own column-4 rows, in the counters and the bits of lr_dev."""
    tr = None
    try:
        tr = rh.trainer(_config(policy, form, adaptive_lr=_band(policy), **KEY), seed=SEED, run_id="ekl_alr")
        rule = dict(tr._adapt.rule)
        lr = np.float32(SCHED["initial"])
        moved = set()
        for u in range(UPDATES):
            rows, _ = _update(tr)
            last = dict(tr.last_adaptive_lr)
            rates, lr, raises, cuts = _walk(rows[:, 4], lr, rule)
            print(f"{policy} / {form}: update {u} exact kl rows {rows[:, 4].tolist()} -> {last}")
            assert last == {"lr": float(lr), "raised": raises, "lowered": cuts, "kl_low": rule["kl_low"], "kl_high": rule["kl_high"]}, u
            assert _bits32(tr.optimizer.lr_dev.item()) == _bits32(lr)
            moved |= {_bits32(r) for r in rates}
        assert len(moved) >= 2, "the rate moved"
    finally:
        rh.release(tr)


@pytest.mark.parametrize("policy", ["discrete", "masked multidiscrete"])
def test_target_kl_stops_on_the_exact_kl_in_the_middle_of_an_epoch(policy):
    rows = _plain_run(policy, "captured, tables", True)[0]
    kl = rows[0][:, 4]
    records = [r for r in (1, 2, 3, 4, 5) if kl[r] > kl[:r].max() and r % N_MB == 0]
    assert records, f"no first minibatch of an epoch has a kl above all earlier rows: {kl.tolist()} (another seed is needed)"
    r = records[0]
    limit = float(np.float32((float(kl[:r].max()) + float(kl[r])) / 2))
    assert float(kl[:r].max()) < limit < float(kl[r])
    tr = None
    try:
        tr = rh.trainer(_config(policy, target_kl={"value": limit, "factor": 1.0, "host_check": "epoch"}, **KEY), seed=SEED, run_id="ekl_stop")
        rows_g, _ = _update(tr)
        stop, state = dict(tr.last_kl_stop), rh.state(tr)
    finally:
        rh.release(tr)
    print(f"{policy}: stop at row {r} of {kl.tolist()}, limit {limit}: {stop}")
    assert stop["stopped"] and stop["steps_applied"] == r and stop["steps_launched"] == r + N_MB and _bits32(stop["kl"]) == _bits32(kl[r])
    assert rows_g.shape == (r + 1, 6) and np.array_equal(rh.bits(rows_g), rh.bits(rows[0][: r + 1]))
    assert int(state["step"]) == r


def test_checkpoint_with_the_key_resumes_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = _config("masked multidiscrete", **KEY)
    tr = fresh = None
    try:
        tr = rh.trainer(cfg, seed=SEED, run_id="ekl_ckpt")
        _update(tr)
        path = tr.save_checkpoint()
        tr.restart_episodes(1)
        rec_a = rh.update(tr)
        old_a = tr.buffer.old_logps.cpu().numpy().copy()
        tr.load_checkpoint(path)
        rec_b = rh.update(tr)
        assert rh.differing(rec_a, rec_b) == []
        assert _same(tr.buffer.old_logps, old_a)
        fresh = rh.trainer(cfg, seed=999, run_id="ekl_fresh", resume=path)
        assert fresh.update_index == 1 and fresh._kl_exact_cat
        rec_c = rh.update(fresh)
        assert rh.differing(rec_a, rec_c) == []
        assert _same(fresh.buffer.old_logps, old_a)
    finally:
        rh.release(tr, fresh)


def test_the_key_on_a_box_policy_is_kl_estimator_analytic_in_every_bit():
    env = dict(type="Synthetic", obs_shape=[rh.F_OBS], continuous_actions=2, max_episode_steps=16, seed=2, p_done=0.1, pool=4)
    base = dict(environment=env, learning_rate_schedule=dict(SCHED), n_mini_batch=N_MB, epochs=EPOCHS)
    runs = {}
    for name, key in (("analytic", {"kl_estimator": "analytic"}), ("exact", KEY), ("both", {"kl_estimator": "analytic", **KEY})):
        tr = None
        try:
            tr = rh.trainer(rh.config(**base, **key), seed=SEED, run_id="ekl_box")
            assert tr.box is not None and tr._kl_analytic and not tr._kl_exact_cat and tr.buffer.means is not None and tr.buffer.old_logps is None
            rows = [_update(tr)[0] for _ in range(UPDATES)]
            runs[name] = (rows, rh.state(tr))
        finally:
            rh.release(tr)
    for name in ("exact", "both"):
        assert rh.differing(runs["analytic"][1], runs[name][1]) == []
        for a, b in zip(runs["analytic"][0], runs[name][0]):
            assert np.array_equal(rh.bits(a), rh.bits(b)), name


def test_refusals_raise_at_construction():
    from trainer import PPOTrainer

    def build(cfg, **kw):
        return PPOTrainer(cfg, run_id="ekl_refused", device=rh.dev(), tensorboard=False, **kw)

    with pytest.raises(ValueError, match=r"exact_kl must be true or false"):
        build(_config(exact_kl="yes"))
    with pytest.raises(ValueError, match=r"exact_kl: true next to kl_estimator: k3"):
        build(_config(kl_estimator="k3", **KEY))
    dp = type("DP", (), {"world": 2, "rank": 0})()
    with pytest.raises(ValueError, match=r"exact_kl: true in a data-parallel run.*remove the key, or train on one device"):
        build(_config(normalize_observations=False, normalize_rewards=False, **KEY), dp=dp)
