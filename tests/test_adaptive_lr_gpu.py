"""-m gpu: the KL-adaptive learning rate (``adaptive_lr``) -- etm_grad_sqnorm_adaptive (csrc/optim.hip) and everything built on it.
Nothing here has a tolerance: the rule is three float32 operations with one host definition (utils.adaptive_lr_step, itself checked
against exact rationals in tests/test_adaptive_lr_host.py), a step that applies runs the ungated arithmetic with the rate the rule
gave, a dropped step writes nothing -- so every comparison is of bits.

Kernel level: n in {4, 2052, 40004} floats x n_partial in {1, 7, 1024} (one float4, a grid-stride tail, many workgroups), ``step`` at 0
and at 12345, ``max_norm`` clipping and not, eleven kl values around the band's limits x five starting rates around the clamps;
the reference is the UNGATED pair run with ``lr_dev`` preset to the model's rate.  With a gate: stopped, tripping, clear.  Every refusal.
Trainer level, on the tiny trainer of tests/resume_helpers.py with ``learning_rate_schedule.final = initial``, in the three forms of the
step:
1. a band nothing leaves: two updates equal a key-absent trainer's in every bit;
2. a band taken from a key-absent probe's kl rows: the run sees a raise and a cut;
3. that run against the host model walked over the run's own rows: counters and the final ``lr_dev`` bits;
4. that run against a key-absent trainer driven step by step from outside with the model's rate: rows and state, every bit;
5. with ``target_kl`` as well, a stop in the middle of an epoch; 6. checkpoint and resume; 7. the refusals at construction.
"""
import struct

import numpy as np
import pytest
import torch

import resume_helpers as rh

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.01
F32 = lambda x: float(np.float32(x))


def _bits32(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _rule(desired_kl=0.01, **over):
    from utils import adaptive_lr_section
    return adaptive_lr_section({"adaptive_lr": dict(desired_kl=desired_kl, **over)})


# ------------------------------------------------------------------ kernel level
def _problem(n, n_partial, step, seed, lr=3e-4):
    gen = torch.Generator().manual_seed(seed)
    dev = rh.dev()
    r = lambda: torch.randn(n, generator=gen)
    return dict(p=r().to(dev), g=(r() * 0.3).to(dev), m=(r() * 0.1).to(dev), v=(r() * 0.1).square().to(dev),
                partial=torch.full((n_partial,), -1.0, device=dev), step=torch.tensor(step, dtype=torch.int64, device=dev),
                lr=torch.tensor(float(lr), dtype=torch.float32, device=dev), norm=torch.full((), -1.0, device=dev), n=n, n_partial=n_partial)


def _clone(prob):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in prob.items()}


def _sqnorm_adaptive(q, kl_tensor, rule, counters, gating=None, **ptr):
    """The new entry on ``q`` -> its return code.  ``gating`` = (limit, gate words, host word or None).  ``ptr``: raw pointer / value
    overrides by argument name (the refusal test)."""
    from etm import lib
    h = lib.load()
    st = torch.cuda.current_stream(rh.dev()).cuda_stream
    limit, words, host = gating if gating is not None else (0.0, None, None)
    a = dict(g=q["g"].data_ptr(), n=q["n"], partial=q["partial"].data_ptr(), n_partial=q["n_partial"], step=q["step"].data_ptr(),
             kl=kl_tensor.data_ptr(), lr_dev=q["lr"].data_ptr(), kl_low=rule["kl_low"], kl_high=rule["kl_high"], factor=rule["factor"],
             lr_min=rule["min"], lr_max=rule["max"], lr_state=counters.data_ptr(), kl_limit=float(limit),
             gate=words.data_ptr() if words is not None else 0, host_word=host.data_ptr() if host is not None else 0)
    a.update(ptr)
    return h.etm_grad_sqnorm_adaptive(a["g"], a["n"], a["partial"], a["n_partial"], a["step"], a["kl"], a["lr_dev"], a["kl_low"], a["kl_high"],
                                      a["factor"], a["lr_min"], a["lr_max"], a["lr_state"], a["kl_limit"], a["gate"], a["host_word"], st)


def _run(q, max_norm, adaptive=None):
    """The pair of launches on ``q`` (in place): the ungated pair, or -- ``adaptive`` = (kl tensor, rule, counters, gate or None) -- the
    new norm entry followed by etm_adamw_clip (no gate) / etm_adamw_clip_gated, the existing entries as they are."""
    from etm import lib
    h = lib.load()
    st = torch.cuda.current_stream(rh.dev()).cuda_stream
    tail = (q["p"].data_ptr(), q["g"].data_ptr(), q["m"].data_ptr(), q["v"].data_ptr(), q["n"], q["partial"].data_ptr(), q["n_partial"],
            q["lr"].data_ptr(), q["step"].data_ptr(), BETAS[0], BETAS[1], EPS, WD, float(max_norm), 1.0, q["norm"].data_ptr())
    if adaptive is None:
        lib.check(h.etm_grad_sqnorm(q["g"].data_ptr(), q["n"], q["partial"].data_ptr(), q["n_partial"], q["step"].data_ptr(), st), "sqnorm")
        lib.check(h.etm_adamw_clip(*tail, st), "adamw")
    else:
        kl, rule, counters, gate = adaptive
        lib.check(_sqnorm_adaptive(q, kl, rule, counters, gate), "sqnorm_adaptive")
        if gate is None:
            lib.check(h.etm_adamw_clip(*tail, st), "adamw")
        else:
            lib.check(h.etm_adamw_clip_gated(*tail, gate[1].data_ptr(), st), "adamw_gated")
    torch.cuda.synchronize()


def _same(a, b, keys):
    return [k for k in keys if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


ARENAS = ("p", "g", "m", "v", "step")
EVERYTHING = ARENAS + ("partial", "norm", "lr")


def _kl_values(rule):
    lo, hi = np.float32(rule["kl_low"]), np.float32(rule["kl_high"])
    return [0.0, -1e-9, 1e-12, float(np.nextafter(lo, np.float32(0))), float(lo), 0.01, float(hi), float(np.nextafter(hi, np.float32(1))), 0.5,
            float("nan"), float("inf")]


def _start_rates(rule):
    # mid-range, at min, at max, one cut above min (a cut lands on the clamp), one raise below max
    return [3e-4, rule["min"], rule["max"], F32(1.2e-5), F32(8e-3)]


@pytest.mark.parametrize("n_partial", [1, 7, 1024])
@pytest.mark.parametrize("n", [4, 2052, 40004])
def test_adaptive_norm_launch_moves_the_rate_as_the_host_rule_and_the_step_runs_the_ungated_bits(n, n_partial):
    from utils import adaptive_lr_step
    dev = rh.dev()
    rule = _rule()
    ways = set()
    for step in (0, 12345):
        for max_norm in (0.05, 1.0e6):                                  # |g| ~ 0.3 sqrt(n) >= 0.6: 0.05 clips, 1e6 does not
            base = _problem(n, n_partial, step, seed=n + n_partial + step)
            wants = {}                                                  # the ungated pair per rate the model can ask for
            for lr0 in _start_rates(rule):
                for kl_value in _kl_values(rule):
                    lr1, way = adaptive_lr_step(np.float32(lr0), np.float32(kl_value), rule)
                    ways.add((way, bool(lr1 == np.float32(lr0))))
                    key = _bits32(lr1)
                    if key not in wants:
                        want = _clone(base)
                        want["lr"].fill_(float(lr1))
                        _run(want, max_norm)
                        assert int(want["step"]) == step + 1 and not torch.equal(want["p"], base["p"])
                        assert (not torch.equal(want["g"], base["g"])) == (max_norm == 0.05), "max_norm clips in one case and not in the other"
                        wants[key] = want
                    got = _clone(base)
                    got["lr"].fill_(float(lr0))
                    kl = torch.tensor([kl_value], dtype=torch.float32, device=dev)
                    counters = torch.tensor([5, 9], dtype=torch.int64, device=dev)
                    _run(got, max_norm, (kl, rule, counters, None))
                    case = (step, max_norm, lr0, kl_value)
                    assert _bits32(got["lr"].item()) == key, (case, float(got["lr"]), float(lr1))
                    assert counters.tolist() == [5 + (way == 1), 9 + (way == -1)], (case, counters.tolist())
                    assert _same(got, wants[key], EVERYTHING) == [], case
            assert len(wants) >= 9, "the rates the model asks for differ: the AdamW launch must have read the new one"
    assert ways == {(0, True), (1, False), (-1, False), (1, True), (-1, True)}, "kept, moved both ways, and both clamps holding the rate"


@pytest.mark.parametrize("n,n_partial", [(2052, 7), (40004, 1024)])
def test_adaptive_norm_launch_with_a_gate(n, n_partial):
    from utils import adaptive_lr_step
    dev = rh.dev()
    rule = _rule()
    limit = F32(0.03)                                                   # above kl_high = 0.02
    for step, max_norm in ((0, 0.05), (12345, 1.0e6)):
        base = _problem(n, n_partial, step, seed=7 + n + step)
        plain = _clone(base)
        _run(plain, max_norm)                                           # (for the partial sums and the norm a dropped step still files)
        # 1. an already-stopped gate: nothing changes, rate and counters included, whatever the kl says
        for kl_value in (0.001, 0.5, float("nan")):
            got = _clone(base)
            kl = torch.tensor([kl_value], dtype=torch.float32, device=dev)
            counters = torch.tensor([5, 9], dtype=torch.int64, device=dev)
            words = torch.tensor([1, 3, 77], dtype=torch.int64, device=dev)
            host = torch.full((1,), 4, dtype=torch.int64).pin_memory()
            _run(got, max_norm, (kl, rule, counters, (limit, words, host)))
            assert _same(got, base, ARENAS + ("lr",)) == [] and counters.tolist() == [5, 9], kl_value
            assert words.tolist() == [1, 3, 77] and int(host[0]) == 4
            assert _same(got, plain, ("partial", "norm")) == []
        # 2. a tripping step: the rule runs first (a kl above kl_high has cut the rate), then the step is dropped
        for kl_value, way in ((0.5, -1), (float("inf"), -1), (float("nan"), 0)):
            lr1, model_way = adaptive_lr_step(np.float32(3e-4), np.float32(kl_value), rule)
            assert model_way == way
            got = _clone(base)
            kl = torch.tensor([kl_value], dtype=torch.float32, device=dev)
            counters = torch.tensor([5, 9], dtype=torch.int64, device=dev)
            words = torch.tensor([0, 3, 0], dtype=torch.int64, device=dev)
            host = torch.zeros(1, dtype=torch.int64).pin_memory()
            _run(got, max_norm, (kl, rule, counters, (limit, words, host)))
            assert _same(got, base, ARENAS) == [], kl_value
            assert _bits32(got["lr"].item()) == _bits32(lr1) and counters.tolist() == [5, 9 + (way == -1)], kl_value
            assert words.tolist() == [1, 3, int(kl.view(torch.int32).item()) & 0xFFFFFFFF] and int(host[0]) == 4
            assert _same(got, plain, ("partial", "norm")) == []
        # (a limit below kl_low: the tripping step raises the rate, and is dropped)
        got = _clone(base)
        kl = torch.tensor([0.004], dtype=torch.float32, device=dev)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        words = torch.zeros(3, dtype=torch.int64, device=dev)
        _run(got, max_norm, (kl, rule, counters, (F32(0.001), words, None)))
        assert _same(got, base, ARENAS) == [] and counters.tolist() == [1, 0] and words.tolist() == [1, 0, _bits32(F32(0.004))]
        assert _bits32(got["lr"].item()) == _bits32(np.float32(3e-4) * np.float32(1.5))
        # 3. a clear gate with kl <= limit (kl == limit included): the gate-free adaptive call, and gate[1] advanced
        for kl_value in (0.0, 1e-12, 0.004, 0.01, float(np.nextafter(np.float32(rule["kl_high"]), np.float32(1))), limit):
            free = _clone(base)
            kl = torch.tensor([kl_value], dtype=torch.float32, device=dev)
            counters_free = torch.tensor([5, 9], dtype=torch.int64, device=dev)
            _run(free, max_norm, (kl, rule, counters_free, None))
            got = _clone(base)
            counters = torch.tensor([5, 9], dtype=torch.int64, device=dev)
            words = torch.tensor([0, 3, 0], dtype=torch.int64, device=dev)
            host = torch.zeros(1, dtype=torch.int64).pin_memory()
            _run(got, max_norm, (kl, rule, counters, (limit, words, host)))
            assert _same(got, free, EVERYTHING) == [] and counters.tolist() == counters_free.tolist(), kl_value
            assert words.tolist() == [0, 4, 0] and int(host[0]) == 0 and int(got["step"]) == step + 1


def test_adaptive_entry_refuses_and_launches_nothing():
    from etm import lib
    h = lib.load()
    dev = rh.dev()
    q = _problem(2052, 7, 5, seed=1)
    start = _clone(q)
    rule = _rule()
    kl = torch.tensor([0.5], dtype=torch.float32, device=dev)           # (a kl that would cut: a launch would show)
    store = torch.zeros(12, dtype=torch.int32, device=dev)              # int64 words at +4 bytes are misaligned
    counters, words = store[:4].view(torch.int64), store[4:10].view(torch.int64)
    bytes_ = torch.zeros(16, dtype=torch.uint8, device=dev)             # a float at +1 / +2 bytes is misaligned
    host = torch.zeros(2, dtype=torch.int64).pin_memory()
    st = torch.cuda.current_stream(dev).cuda_stream
    einval = h.etm_grad_sqnorm(0, q["n"], q["partial"].data_ptr(), q["n_partial"], 0, st)
    assert einval != 0
    gate = (0.03, words, host)
    call = lambda gating=None, **ptr: _sqnorm_adaptive(q, kl, rule, counters, gating, **ptr)
    refused = {
        "kl NULL": call(kl=0), "kl misaligned": call(kl=bytes_.data_ptr() + 2), "lr_dev NULL": call(lr_dev=0),
        "lr_dev misaligned": call(lr_dev=bytes_.data_ptr() + 1), "lr_state NULL": call(lr_state=0),
        "lr_state misaligned": call(lr_state=counters.data_ptr() + 4), "gate misaligned": call(gate, gate=words.data_ptr() + 4),
        "host_word misaligned": call(gate, host_word=host.data_ptr() + 4), "host_word without gate": call(host_word=host.data_ptr()),
        "factor 1": call(factor=1.0), "factor below 1": call(factor=0.5), "factor NaN": call(factor=float("nan")),
        "factor Inf": call(factor=float("inf")), "kl_low negative": call(kl_low=-1e-3), "kl_low == kl_high": call(kl_low=rule["kl_high"]),
        "kl_low above kl_high": call(kl_low=0.03), "kl_low NaN": call(kl_low=float("nan")), "kl_high Inf": call(kl_high=float("inf")),
        "kl_high NaN": call(kl_high=float("nan")), "lr_min 0": call(lr_min=0.0), "lr_min negative": call(lr_min=-1e-5),
        "lr_min above lr_max": call(lr_min=0.1), "lr_min NaN": call(lr_min=float("nan")), "lr_max Inf": call(lr_max=float("inf")),
        "lr_max NaN": call(lr_max=float("nan")),
        # and whatever etm_grad_sqnorm refuses
        "g NULL": call(g=0), "g misaligned": call(g=q["g"].data_ptr() + 4), "n not a multiple of 4": call(n=q["n"] - 1), "n 0": call(n=0),
        "partial NULL": call(partial=0), "n_partial 0": call(n_partial=0), "n_partial above 4096": call(n_partial=4097),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in refused.items() if v != einval} == {}
    assert _same(q, start, EVERYTHING) == [] and not bool(store.any()) and host.tolist() == [0, 0], "a refused call launches nothing"
    # the same arguments unharmed are taken (kl_low 0 and lr_min == lr_max are inside the ranges)
    assert call(kl_low=0.0, lr_min=rule["max"]) == 0 and call(gate) == 0
    torch.cuda.synchronize()
    assert counters.tolist() == [0, 2] and words.tolist() == [1, 0, _bits32(0.5)] and int(host[0]) == 1


# ------------------------------------------------------------------ FlatAdamW.step(adapt=)
def _optimiser(lr=3e-4):
    from etm.optim import FlatAdamW
    torch.manual_seed(3)
    dev = rh.dev()
    return FlatAdamW([torch.nn.Parameter(torch.randn(37, 5, device=dev)), torch.nn.Parameter(torch.randn(11, device=dev))], lr=lr)


def _opt_state(opt):
    return [t.clone() for t in (opt.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.flat_grads, opt.step_dev, opt.lr_dev, opt.total_norm)]


def test_flat_adamw_step_takes_the_rule():
    """keep, raise, cut, keep against a plain optimiser whose ``set_lr`` is fed the model's rate; then the gate as well."""
    from etm.optim import AdaptiveLr, KlGate
    from utils import adaptive_lr_step
    dev = rh.dev()
    rule = _rule()
    plain, adaptive = _optimiser(), _optimiser()
    adapt = AdaptiveLr(rule, dev)
    adapt.reset()
    stats = torch.zeros(6, device=dev)
    adapt.kl = stats[4:5]
    gen = torch.Generator().manual_seed(8)
    lr = np.float32(3e-4)
    for kl_value, way in ((0.01, 0), (0.001, 1), (0.3, -1), (0.0, 0)):
        grad = torch.randn(plain.flat_grads.numel(), generator=gen).to(dev)
        stats[4] = kl_value
        lr, model_way = adaptive_lr_step(lr, np.float32(kl_value), rule)
        assert model_way == way
        plain.set_lr(float(lr))
        plain.flat_grads.copy_(grad)
        plain.step(0.5)
        adaptive.flat_grads.copy_(grad)
        adaptive.step(0.5, adapt=adapt)
        for a, b in zip(_opt_state(plain), _opt_state(adaptive)):
            assert torch.equal(a, b), kl_value
    assert adapt.read() == (1, 1) and int(adaptive.step_dev) == 4 and _bits32(adaptive.lr_dev.item()) == _bits32(lr)
    adapt.reset()
    assert adapt.read() == (0, 0) and _bits32(adaptive.lr_dev.item()) == _bits32(lr), "the counters are per update, the rate is never reset"
    # with a gate: a tripping step cuts and is dropped, a later one does nothing at all
    gate = KlGate(F32(0.03), dev)
    gate.reset()
    gate.kl = stats[4:5]
    stats[4] = 0.2
    before = _opt_state(adaptive)
    adaptive.step(0.5, gate=gate, adapt=adapt)
    after = _opt_state(adaptive)
    cut = adaptive_lr_step(lr, np.float32(0.2), rule)[0]
    assert all(torch.equal(a, b) for a, b in zip(before[:5], after[:5])) and _bits32(after[5].item()) == _bits32(cut)
    stats[4] = 0.001
    adaptive.step(0.5, gate=gate, adapt=adapt)
    assert all(torch.equal(a, b) for a, b in zip(after[:6], _opt_state(adaptive)[:6]))
    torch.cuda.synchronize()
    assert adapt.read() == (0, 1) and gate.read() == (True, 0, F32(0.2)) and int(adaptive.step_dev) == 4
    with pytest.raises(RuntimeError, match="the device owns lr_dev"):
        adaptive.set_lr(1e-3)
    with pytest.raises(ValueError, match="the same element"):
        gate.kl = stats[3:4]
        adaptive.step(0.5, gate=gate, adapt=adapt)
    with pytest.raises(ValueError, match="adapt.kl"):
        adapt.kl = None
        adaptive.step(0.5, adapt=adapt)


def test_flat_adamw_state_round_trips_the_adapted_rate():
    from etm.optim import AdaptiveLr
    dev = rh.dev()
    rule = _rule()
    a = _optimiser()
    adapt = AdaptiveLr(rule, dev)
    a.attach_adaptive(adapt)
    kl = torch.tensor([0.3], device=dev)
    adapt.kl = kl
    for _ in range(3):
        a.flat_grads.normal_()
        a.step(0.5, adapt=adapt)
    sd = a.state_dict()
    want = np.float32(np.float32(np.float32(np.float32(3e-4) / np.float32(1.5)) / np.float32(1.5)) / np.float32(1.5))
    assert _bits32(sd["lr"]) == _bits32(want) == _bits32(a.lr_dev.item()) and float(np.float32(sd["lr"])) == sd["lr"] and sd["step"] == 3
    b = _optimiser(lr=1e-3)
    b.attach_adaptive(AdaptiveLr(rule, dev))
    address = b.lr_dev.data_ptr()
    b.load_state_dict(sd)
    assert b.lr_dev.data_ptr() == address and _bits32(b.lr_dev.item()) == _bits32(want) and b._lr_host == sd["lr"]
    assert _bits32(b.state_dict()["lr"]) == _bits32(want)
    # without a rule the stored value is what it is today: the python float set_lr was last given
    c = _optimiser(lr=2.8e-4)
    assert c.state_dict()["lr"] == 2.8e-4
    # ... and a rule-carrying optimiser continues from such a stored value
    b.load_state_dict(dict(sd, lr=2.8e-4))
    assert _bits32(b.lr_dev.item()) == _bits32(np.float32(2.8e-4)) and _bits32(b.state_dict()["lr"]) == _bits32(np.float32(2.8e-4))


# ------------------------------------------------------------------ trainer level
FORMS = {"captured, tables": {}, "captured, no tables": {"step_ends_fused": False}, "eager": rh.modes(False)}
SCHED = dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10)
SEED = 11
UPDATES = 2


def _config(form="captured, tables", **over):
    return rh.config(**{"learning_rate_schedule": dict(SCHED), "n_mini_batch": 2, "epochs": 3, **FORMS[form], **over})


def _perms(update, epochs=3, batch=rh.W_T * rh.S_T):
    rng = np.random.default_rng(4 + update)
    return [rng.permutation(batch) for _ in range(epochs)]


def _update(tr):
    """Update ``tr.update_index`` as ``run_training`` runs it, on ``_perms`` and the trainer's own draws -> (statistics rows, norm rows)."""
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    rows, norms = tr._train_epochs(lr, clip, beta, perms=_perms(tr.update_index))
    tr.update_index += 1
    torch.cuda.synchronize()
    return np.stack(rows), norms


def _single_steps(tr, rates):
    """The first ``len(rates)`` minibatch steps of the update ``_update`` would run, asked for one by one from outside ``_train_epochs``
    with the rate of each step passed in -- no code of this feature runs -- and with what ``_train_epochs`` does around its steps."""
    _, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    perms = _perms(tr.update_index)
    n_mb = tr.buffer.n_mini_batches
    mbs = tr.buffer.batch_size // n_mb
    with torch.no_grad():
        tr._bank_pos = tr._bank_with_positions()
        tr._obs_train = tr._training_observations()
    monitor = tr.config.get("monitor_gradients", True)
    rows = []
    for i, lr in enumerate(rates):
        perm = torch.as_tensor(perms[i // n_mb], device=tr.device, dtype=torch.long).view(-1, mbs).sort(dim=1).values
        idx = perm[i % n_mb].contiguous()
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
    return np.stack(rows)


def _walk(kl_rows, lr, rule, limit=None):
    """The host model over one update's kl rows -> (rate per step: the one the step's AdamW launch uses, raises, cuts, steps applied,
    stopped).  ``limit``: ``target_kl`` as well -- a dropped step moves nothing, the tripping step has run the rule."""
    from utils import adaptive_lr_step
    rates, raises, cuts, applied, stopped = [], 0, 0, 0, False
    for kl in np.asarray(kl_rows, dtype=np.float32):
        if stopped:
            break
        lr, way = adaptive_lr_step(lr, kl, rule)
        raises, cuts = raises + (way == 1), cuts + (way == -1)
        if limit is not None and not kl <= np.float32(limit):
            stopped = True
            break
        rates.append(np.float32(lr))
        applied += 1
    return rates, np.float32(lr), raises, cuts, applied, stopped


@pytest.mark.parametrize("form", list(FORMS))
def test_a_band_nothing_leaves_changes_no_bit(form):
    """low 0 and kl_high = 3e38: two updates through the adaptive norm launch equal a key-absent trainer's in every bit."""
    results = []
    for key in ({}, {"adaptive_lr": {"desired_kl": 1.5e38, "low": 0, "high": 2.0}}):
        tr = None
        try:
            tr = rh.trainer(_config(form, **key), seed=SEED, run_id="alr_never")
            out = [_update(tr) for _ in range(2)]
            results.append((out, rh.state(tr), tr.last_adaptive_lr))
            assert (tr._train_graph is not None) == (form != "eager")
            assert (getattr(tr, "_tg_idx_table", None) is not None) == (form == "captured, tables")
        finally:
            rh.release(tr)
    (out_a, state_a, last_a), (out_b, state_b, last_b) = results
    assert last_a is None
    assert last_b == {"lr": F32(3e-4), "raised": 0, "lowered": 0, "kl_low": 0.0, "kl_high": F32(3e38)}
    assert rh.differing(state_a, state_b) == [] and int(state_b["step"]) == 12
    for (rows_a, norms_a), (rows_b, norms_b) in zip(out_a, out_b):
        assert rows_a.shape == (6, 6) and np.array_equal(rh.bits(rows_a), rh.bits(rows_b)) and norms_a == norms_b


_CACHE = {}


def _band():
    """The band, from a key-absent probe's kl rows of its first update (as test_target_kl_gpu._stop_row derives its limit): row 1 -- the
    kl after one step, the smallest real one -- lies below kl_low and raises the rate; kl_high lies between row 1 and the largest later
    row, so that a later step of the probe would cut.  -> the ``adaptive_lr`` section (desired_kl 1: low and high ARE the limits)."""
    if "band" not in _CACHE:
        tr = None
        try:
            tr = rh.trainer(_config(), seed=SEED, run_id="alr_probe")
            rows, _ = _update(tr)
        finally:
            rh.release(tr)
        kl = rows[:, 4]
        print("probe kl (n_mini_batch 2, epochs 3):", kl.tolist())
        later = float(kl[2:].max())
        assert 0 < float(kl[1]) < later, f"row 1 must be a real kl below a later row's: {kl.tolist()} (another seed is needed)"
        kl_low = np.float32(float(kl[1]) + 0.25 * (later - float(kl[1])))
        kl_high = np.float32(float(kl[1]) + 0.5 * (later - float(kl[1])))
        assert float(kl[1]) < kl_low < kl_high < later
        _CACHE["band"] = {"desired_kl": 1.0, "low": float(kl_low), "high": float(kl_high)}
    return _CACHE["band"]


def _adaptive_run(form):
    """``UPDATES`` updates of the trainer with the probe's band -> (rows per update, norms per update, ``last_adaptive_lr`` per update,
    state, rule)."""
    if ("run", form) not in _CACHE:
        tr = None
        try:
            tr = rh.trainer(_config(form, adaptive_lr=_band()), seed=SEED, run_id="alr_run")
            rows, norms, last = [], [], []
            for _ in range(UPDATES):
                r, n = _update(tr)
                rows.append(r), norms.append(n), last.append(dict(tr.last_adaptive_lr))
            _CACHE[("run", form)] = (rows, norms, last, rh.state(tr), dict(tr._adapt.rule))
            assert (tr._train_graph is not None) == (form != "eager")
        finally:
            rh.release(tr)
    return _CACHE[("run", form)]


@pytest.mark.parametrize("form", list(FORMS))
def test_a_run_that_raises_and_cuts_equals_the_host_model_and_single_steps_at_the_models_rate(form):
    rows, norms, last, state, rule = _adaptive_run(form)
    assert rule["kl_low"] == _band()["low"] and rule["kl_high"] == _band()["high"]
    for u in range(UPDATES):
        print(f"{form}: update {u} kl rows {rows[u][:, 4].tolist()} -> {last[u]}")
    # 2. the run sees a raise and a cut
    assert sum(x["raised"] for x in last) >= 1 and sum(x["lowered"] for x in last) >= 1, last
    # 3. the host model over the run's own rows
    lr, schedule = np.float32(SCHED["initial"]), []
    for u in range(UPDATES):
        assert rows[u].shape == (6, 6)
        rates, lr, raises, cuts, applied, stopped = _walk(rows[u][:, 4], lr, rule)
        assert applied == 6 and not stopped
        assert last[u] == {"lr": float(lr), "raised": raises, "lowered": cuts, "kl_low": rule["kl_low"], "kl_high": rule["kl_high"]}, u
        schedule.append(rates)
    assert _bits32(state["lr"]) == _bits32(lr) and int(state["step"]) == 6 * UPDATES
    assert len({_bits32(r) for rates in schedule for r in rates}) >= 3, "the rate moved both ways"
    # 4. a key-absent trainer driven step by step from outside with the model's rate per step: code that runs nothing new
    tr = None
    try:
        tr = rh.trainer(_config(form), seed=SEED, run_id="alr_single")
        for u in range(UPDATES):
            rows_s = _single_steps(tr, schedule[u])
            assert np.array_equal(rh.bits(rows_s), rh.bits(rows[u])), u
        assert tr.last_adaptive_lr is None and rh.differing(rh.state(tr), state) == []
    finally:
        rh.release(tr)


def test_with_target_kl_a_stop_in_the_middle_of_an_epoch():
    """Both keys: the rows of the run without the stop hold up to the stop, so its limit is taken from them."""
    rows, _, _, _, rule = _adaptive_run("captured, tables")
    kl = rows[0][:, 4]
    # the first minibatch of an epoch stops (r in {2, 4}: the second one is launched and must do nothing), the stopping kl above all earlier
    records = [r for r in (2, 4) if kl[r] > kl[:r].max()]
    assert records, f"no first minibatch of an epoch has a kl above all earlier rows: {kl.tolist()} (another seed is needed)"
    r = records[0]
    limit = float(np.float32((float(kl[:r].max()) + float(kl[r])) / 2))
    assert float(kl[:r].max()) < limit < float(kl[r])
    rates, lr_end, raises, cuts, applied, stopped = _walk(kl, np.float32(SCHED["initial"]), rule, limit=limit)
    assert stopped and applied == r and len(rates) == r
    print(f"stop at row {r} of {kl.tolist()}, limit {limit}; the stopping step's rule: {lr_end} after {rates}")
    key = {"adaptive_lr": _band(), "target_kl": {"value": limit, "factor": 1.0, "host_check": "epoch"}}
    tr = None
    try:
        tr = rh.trainer(_config(**key), seed=SEED, run_id="alr_stop")
        rows_g, _ = _update(tr)
        state, stop, last = rh.state(tr), dict(tr.last_kl_stop), dict(tr.last_adaptive_lr)
    finally:
        rh.release(tr)
    assert stop["stopped"] and stop["steps_applied"] == r and stop["steps_launched"] == r + 2 and _bits32(stop["kl"]) == _bits32(kl[r])
    assert rows_g.shape == (r + 1, 6) and np.array_equal(rh.bits(rows_g), rh.bits(rows[0][: r + 1]))
    assert int(state["step"]) == r, "step_dev counts applied steps only"
    assert last == {"lr": float(lr_end), "raised": raises, "lowered": cuts, "kl_low": rule["kl_low"], "kl_high": rule["kl_high"]}
    assert _bits32(state["lr"]) == _bits32(lr_end)
    tr = None
    try:                       # a key-absent trainer driven for exactly r single steps at the model's rates: everything but the rate itself
        tr = rh.trainer(_config(), seed=SEED, run_id="alr_stop_single")
        rows_s = _single_steps(tr, rates)
        assert np.array_equal(rh.bits(rows_s), rh.bits(rows_g[:r]))
        ref = rh.state(tr)
        assert [k for k in rh.differing(ref, state) if k != "lr"] == []
        assert _bits32(ref["lr"]) == _bits32(rates[-1])
    finally:
        rh.release(tr)


def test_checkpoint_after_an_adaptive_update_resumes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = _config(adaptive_lr=_band())
    tr = fresh = None
    try:
        tr = rh.trainer(cfg, seed=SEED, run_id="alr_ckpt")
        _update(tr)
        saved_lr = tr.last_adaptive_lr["lr"]
        assert _bits32(saved_lr) != _bits32(F32(SCHED["initial"])), "the checkpoint carries a rate the rule has moved"
        path = tr.save_checkpoint()
        tr.restart_episodes(1)
        rec_a = rh.update(tr)
        last_a, graph = dict(tr.last_adaptive_lr), tr._train_graph
        assert graph is not None
        tr.load_checkpoint(path)
        assert _bits32(tr.optimizer.lr_dev.item()) == _bits32(saved_lr) and tr.optimizer._lr_host == saved_lr and tr.update_index == 1
        rec_b = rh.update(tr)
        assert rh.differing(rec_a, rec_b) == [] and tr.last_adaptive_lr == last_a
        assert tr._train_graph is graph, "the captured graphs keep replaying, with the restored rate"
        fresh = rh.trainer(cfg, seed=999, run_id="alr_fresh", resume=path)
        assert _bits32(fresh.optimizer.lr_dev.item()) == _bits32(saved_lr) and fresh.update_index == 1
        rec_c = rh.update(fresh)
        assert rh.differing(rec_a, rec_c) == [] and fresh.last_adaptive_lr == last_a
    finally:
        rh.release(tr, fresh)


def test_checkpoint_of_a_key_absent_run_resumed_with_the_key_continues_from_its_rate(tmp_path, monkeypatch):
    """A key-absent run with a decaying schedule, resumed with the key (the current config wins): the rule starts from the stored rate."""
    monkeypatch.chdir(tmp_path)
    plain = late = None
    try:
        plain = rh.trainer(rh.config(n_mini_batch=2, epochs=3), seed=SEED, run_id="alr_plain")
        for _ in range(2):
            rh.update(plain)
        stored = plain.optimizer.state_dict()["lr"]
        assert stored == plain.schedules(1)[0] != SCHED["initial"]
        path_plain = plain.save_checkpoint()
        late = rh.trainer(_config(adaptive_lr={"desired_kl": 1.5e38, "low": 0, "high": 2.0}), seed=5, run_id="alr_late", resume=path_plain)
        assert _bits32(late.optimizer.lr_dev.item()) == _bits32(np.float32(stored)) and late.update_index == 2
        rh.update(late)
        assert late.last_adaptive_lr["lr"] == F32(stored) and _bits32(late.optimizer.lr_dev.item()) == _bits32(np.float32(stored))
    finally:
        rh.release(plain, late)


def test_refusals_raise_at_construction():
    from trainer import PPOTrainer

    def build(**over):
        return PPOTrainer(_config(**over), run_id="alr_refused", device=rh.dev(), tensorboard=False)

    with pytest.raises(ValueError, match=r"adaptive_lr\.desired_kl must be a finite number > 0"):
        build(adaptive_lr=-0.01)
    with pytest.raises(ValueError, match=r"adaptive_lr\.factor must be a finite number > 1"):
        build(adaptive_lr={"desired_kl": 0.01, "factor": 1.0})
    with pytest.raises(ValueError, match=r"choose low < high"):
        build(adaptive_lr={"desired_kl": 0.01, "low": 2.0, "high": 0.5})
    with pytest.raises(ValueError, match=r"adaptive_lr\.min = .* must not exceed"):
        build(adaptive_lr={"desired_kl": 0.01, "min": 1e-3, "max": 5e-4})
    with pytest.raises(ValueError, match=r"adaptive_lr: unknown keys \['schedule'\]"):
        build(adaptive_lr={"desired_kl": 0.01, "schedule": "adaptive"})
    with pytest.raises(ValueError, match=r"outside \[min, max\]"):
        build(adaptive_lr={"desired_kl": 0.01, "min": 1e-3})
    with pytest.raises(ValueError, match=r"decaying learning_rate_schedule.*set learning_rate_schedule\.final to initial"):
        build(adaptive_lr=0.01, learning_rate_schedule=dict(SCHED, final=1e-4))
    dp = type("DP", (), {"world": 2, "rank": 0})()
    with pytest.raises(ValueError, match=r"adaptive_lr in a data-parallel run"):
        PPOTrainer(_config(adaptive_lr=0.01, normalize_observations=False, normalize_rewards=False), run_id="alr_refused", device=rh.dev(),
                   dp=dp, tensorboard=False)
