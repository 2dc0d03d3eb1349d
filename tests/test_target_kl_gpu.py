"""-m gpu: the KL early stop (``target_kl``) -- etm_grad_sqnorm_gated / etm_adamw_clip_gated (csrc/optim.hip) and everything built on them.
Nothing here has a tolerance: a step that applies runs the ungated arithmetic, a dropped step writes nothing, so every comparison is
of bits.

Kernel level: n in {4, 2052, 40004} floats x n_partial in {1, 7, 1024} (one float4, a grid-stride tail, several workgroups), ``step`` at
0 and at 12345, ``max_norm`` clipping and not; the gate clear with kl <= limit (kl == limit included), and kl above the limit, NaN, +Inf.
Trainer level, on the tiny trainer of tests/resume_helpers.py:
1. limit 3e38: two updates equal a key-absent trainer's in every bit, in the three forms of the step.
2. ``n_mini_batch: 1, epochs: 4``: the stop at row r of a probe; rows, ``step_dev`` and the state of a key-absent ``epochs: r`` run.
3. ``n_mini_batch: 2, epochs: 3``: a stop in the middle of an epoch; ``host_check`` epoch and none; r single steps from outside.
   (The parent commit's single-step wiring and ``_train_epochs`` give equal bits on this config -- the assertion below is of equal bits.)
4. A checkpoint saved after a stopped update resumes.
"""
import struct

import numpy as np
import pytest
import torch

import resume_helpers as rh

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.01


def _bits32(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


# ------------------------------------------------------------------ kernel level
def _problem(n, n_partial, step, seed):
    gen = torch.Generator().manual_seed(seed)
    dev = rh.dev()
    r = lambda: torch.randn(n, generator=gen)
    return dict(p=r().to(dev), g=(r() * 0.3).to(dev), m=(r() * 0.1).to(dev), v=(r() * 0.1).square().to(dev),
                partial=torch.full((n_partial,), -1.0, device=dev), step=torch.tensor(step, dtype=torch.int64, device=dev),
                lr=torch.tensor(3e-4, dtype=torch.float32, device=dev), norm=torch.full((), -1.0, device=dev), n=n, n_partial=n_partial)


def _clone(prob):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in prob.items()}


def _run(prob, max_norm, gate=None):
    """The pair of launches on ``prob`` (in place): ungated, or gated with ``gate`` = (kl tensor, limit, gate tensor, host word or None)."""
    from etm import lib
    h = lib.load()
    st = torch.cuda.current_stream(rh.dev()).cuda_stream
    q = prob
    tail = (q["lr"].data_ptr(), q["step"].data_ptr(), BETAS[0], BETAS[1], EPS, WD, float(max_norm), 1.0, q["norm"].data_ptr())
    if gate is None:
        lib.check(h.etm_grad_sqnorm(q["g"].data_ptr(), q["n"], q["partial"].data_ptr(), q["n_partial"], q["step"].data_ptr(), st), "sqnorm")
        lib.check(h.etm_adamw_clip(q["p"].data_ptr(), q["g"].data_ptr(), q["m"].data_ptr(), q["v"].data_ptr(), q["n"], q["partial"].data_ptr(),
                                   q["n_partial"], *tail, st), "adamw")
    else:
        kl, limit, words, host = gate
        lib.check(h.etm_grad_sqnorm_gated(q["g"].data_ptr(), q["n"], q["partial"].data_ptr(), q["n_partial"], q["step"].data_ptr(),
                                          kl.data_ptr(), float(limit), words.data_ptr(), host.data_ptr() if host is not None else 0, st),
                  "sqnorm_gated")
        lib.check(h.etm_adamw_clip_gated(q["p"].data_ptr(), q["g"].data_ptr(), q["m"].data_ptr(), q["v"].data_ptr(), q["n"],
                                         q["partial"].data_ptr(), q["n_partial"], *tail, words.data_ptr(), st), "adamw_gated")
    torch.cuda.synchronize()


def _same(a, b, keys):
    return [k for k in keys if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


ARENAS = ("p", "g", "m", "v", "step")
LIMIT = float(np.float32(0.03))


@pytest.mark.parametrize("n_partial", [1, 7, 1024])
@pytest.mark.parametrize("n", [4, 2052, 40004])
def test_gated_pair_applies_with_the_ungated_bits_and_drops_without_a_write(n, n_partial):
    dev = rh.dev()
    for step in (0, 12345):
        for max_norm in (0.05, 1.0e6):                                  # |g| ~ 0.3 sqrt(n) >= 0.6: 0.05 clips, 1e6 does not
            start = _problem(n, n_partial, step, seed=n + n_partial + step)
            want = _clone(start)
            _run(want, max_norm)
            assert int(want["step"]) == step + 1
            clipped = not torch.equal(want["g"], start["g"])
            assert clipped == (max_norm == 0.05), "max_norm must clip in one case and not in the other"
            assert not torch.equal(want["p"], start["p"]) and not torch.equal(want["m"], start["m"]) and not torch.equal(want["v"], start["v"])
            # gate clear, kl below the limit and exactly at it (which must apply): the ungated bits, gate[1] advanced
            for kl_value in (0.0, 0.01, LIMIT):
                got = _clone(start)
                kl = torch.tensor([kl_value], dtype=torch.float32, device=dev)
                words = torch.tensor([0, 3, 0], dtype=torch.int64, device=dev)
                host = torch.zeros(1, dtype=torch.int64).pin_memory()
                _run(got, max_norm, (kl, LIMIT, words, host))
                assert _same(got, want, ARENAS + ("partial", "norm")) == [], (step, max_norm, kl_value)
                assert words.tolist() == [0, 4, 0] and int(host[0]) == 0
            # halting values: above the limit, NaN, +Inf
            above = float(np.nextafter(np.float32(LIMIT), np.float32(1.0)))
            for kl_value in (above, 0.5, float("nan"), float("inf")):
                got = _clone(start)
                kl = torch.tensor([kl_value], dtype=torch.float32, device=dev)
                words = torch.tensor([0, 3, 0], dtype=torch.int64, device=dev)
                host = torch.zeros(1, dtype=torch.int64).pin_memory()
                _run(got, max_norm, (kl, LIMIT, words, host))
                assert _same(got, start, ARENAS) == [], (step, max_norm, kl_value)
                assert _same(got, want, ("partial", "norm")) == [], "a dropped step still files the partial sums and the norm"
                tripped = int(kl.view(torch.int32).item()) & 0xFFFFFFFF
                assert words.tolist() == [1, 3, tripped] and int(host[0]) == 4, (words.tolist(), host.tolist())
                # a following call with a small kl stays halted and overwrites neither gate[2] nor the host word
                kl.fill_(0.0)
                got["g"].mul_(2.0)                                     # (the next minibatch's gradient)
                before = _clone(got)
                _run(got, max_norm, (kl, LIMIT, words, host))
                assert _same(got, before, ARENAS) == [] and words.tolist() == [1, 3, tripped] and int(host[0]) == 4
            # no host word: the same decision, nothing stored outside the gate
            got = _clone(start)
            kl = torch.tensor([0.5], dtype=torch.float32, device=dev)
            words = torch.tensor([0, 0, 0], dtype=torch.int64, device=dev)
            _run(got, max_norm, (kl, LIMIT, words, None))
            assert _same(got, start, ARENAS) == [] and words.tolist() == [1, 0, _bits32(0.5)]


def test_gated_entries_refuse_null_and_misaligned_arguments():
    from etm import lib
    h = lib.load()
    dev = rh.dev()
    q = _problem(2052, 7, 5, seed=1)
    start = _clone(q)
    kl = torch.tensor([0.0], dtype=torch.float32, device=dev)
    store = torch.zeros(8, dtype=torch.int32, device=dev)              # (an int64 gate at +4 bytes is misaligned)
    words = store.view(torch.int64)
    st = torch.cuda.current_stream(dev).cuda_stream
    einval = h.etm_grad_sqnorm(0, q["n"], q["partial"].data_ptr(), q["n_partial"], 0, st)
    assert einval != 0
    sq = lambda klp, gp, hp=0: h.etm_grad_sqnorm_gated(q["g"].data_ptr(), q["n"], q["partial"].data_ptr(), q["n_partial"], q["step"].data_ptr(),
                                                      klp, LIMIT, gp, hp, st)
    assert sq(0, words.data_ptr()) == einval and sq(kl.data_ptr(), 0) == einval and sq(kl.data_ptr(), words.data_ptr() + 4) == einval
    assert sq(kl.data_ptr(), words.data_ptr(), words.data_ptr() + 12) == einval, "a misaligned host word"
    ad = lambda gp: h.etm_adamw_clip_gated(q["p"].data_ptr(), q["g"].data_ptr(), q["m"].data_ptr(), q["v"].data_ptr(), q["n"],
                                           q["partial"].data_ptr(), q["n_partial"], q["lr"].data_ptr(), q["step"].data_ptr(), BETAS[0], BETAS[1],
                                           EPS, WD, 0.5, 1.0, q["norm"].data_ptr(), gp, st)
    assert ad(0) == einval and ad(words.data_ptr() + 4) == einval
    torch.cuda.synchronize()
    assert _same(q, start, ARENAS + ("partial", "norm")) == [] and not bool(store.any()), "a refused call launches nothing"


def test_flat_adamw_step_takes_the_gate():
    """FlatAdamW.step(gate=): None is the ungated pair; a KlGate applies, then drops, with ``step_dev`` counting applied steps only."""
    from etm.optim import FlatAdamW, KlGate
    dev = rh.dev()

    def make():
        torch.manual_seed(3)
        params = [torch.nn.Parameter(torch.randn(37, 5, device=dev)), torch.nn.Parameter(torch.randn(11, device=dev))]
        opt = FlatAdamW(params, lr=1e-3)
        return opt

    plain, gated = make(), make()
    gate = KlGate(LIMIT, dev)
    gate.reset()
    stats = torch.zeros(6, device=dev)
    gate.kl = stats[4:5]
    gen = torch.Generator().manual_seed(8)
    for k, kl_value in enumerate((0.0, 0.02, 0.2, 0.0)):
        grad = torch.randn(plain.flat_grads.numel(), generator=gen).to(dev)
        stats[4] = kl_value
        gated.flat_grads.copy_(grad)
        before = [t.clone() for t in (gated.flat_params, gated.exp_avg, gated.exp_avg_sq, gated.flat_grads, gated.step_dev)]
        gated.step(0.5, gate=gate)
        if k < 2:
            plain.flat_grads.copy_(grad)
            plain.step(0.5)
            for a, b in zip((plain.flat_params, plain.exp_avg, plain.exp_avg_sq, plain.flat_grads, plain.step_dev),
                            (gated.flat_params, gated.exp_avg, gated.exp_avg_sq, gated.flat_grads, gated.step_dev)):
                assert torch.equal(a, b)
        else:
            for a, b in zip(before, (gated.flat_params, gated.exp_avg, gated.exp_avg_sq, gated.flat_grads, gated.step_dev)):
                assert torch.equal(a, b)
    torch.cuda.synchronize()
    assert gate.read() == (True, 2, float(np.float32(0.2))) and int(gate.host_word[0]) == 3 and int(gated.step_dev) == 2
    gate.reset()
    assert gate.read() == (False, 0, None) and int(gate.host_word[0]) == 0
    with pytest.raises(ValueError, match="gate.kl"):
        gate.kl = None
        gated.step(0.5, gate=gate)


# ------------------------------------------------------------------ trainer level
FORMS = {"captured, tables": {}, "captured, no tables": {"step_ends_fused": False}, "eager": rh.modes(False)}


def _perms(epochs, batch=rh.W_T * rh.S_T, seed=4):
    rng = np.random.default_rng(seed)
    return [rng.permutation(batch) for _ in range(epochs)]


def _update(tr, perms):
    """One update as ``run_training`` runs it, on explicit permutations and the trainer's own draws -> (statistics rows, norm rows)."""
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    assert tr.buffer.batch_size == len(perms[0])
    rows, norms = tr._train_epochs(lr, clip, beta, perms=perms)
    tr.update_index += 1
    torch.cuda.synchronize()
    return np.stack(rows), norms


def _single_steps(tr, perms, steps):
    """The first ``steps`` minibatch steps of the update ``_update`` would run, asked for one by one from outside ``_train_epochs`` (as
    tests/test_gpu_step_ends.py asks for single steps), with what ``_train_epochs`` does around its steps."""
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    n_mb = tr.buffer.n_mini_batches
    mbs = tr.buffer.batch_size // n_mb
    with torch.no_grad():
        tr._bank_pos = tr._bank_with_positions()
        tr._obs_train = tr._training_observations()
    monitor = tr.config.get("monitor_gradients", True)
    rows = []
    for i in range(steps):
        perm = torch.as_tensor(perms[i // n_mb], device=tr.device, dtype=torch.long).view(-1, mbs).sort(dim=1).values
        st, _ = tr._train_step_graph(perm[i % n_mb].contiguous(), lr, clip, beta, monitor)
        rows.append(st.cpu().numpy())
    if tr.model.obs_norm is not None:
        tr._update_obs_norm()
    tr._bank_pos = tr._row_stats = None
    tr.update_index += 1
    torch.cuda.synchronize()
    return np.stack(rows)


def _kl_key(limit, host_check="epoch"):
    return {"target_kl": {"value": float(limit), "factor": 1.0, "host_check": host_check}}


@pytest.mark.parametrize("form", list(FORMS))
def test_a_limit_never_reached_changes_no_bit(form):
    """Limit 3e38: two updates through the gated launches equal a key-absent trainer of the same seed in every bit of the state."""
    results = []
    for key in ({}, _kl_key(3e38, "none" if form == "eager" else "epoch")):
        tr = None
        try:
            tr = rh.trainer(rh.config(**FORMS[form], **key), run_id="kl_never")
            out = [_update(tr, _perms(2, seed=4 + u)) for u in range(2)]
            results.append((out, rh.state(tr), tr.last_kl_stop))
            assert (tr._train_graph is not None) == (form != "eager")
            assert (getattr(tr, "_tg_idx_table", None) is not None) == (form == "captured, tables")
        finally:
            rh.release(tr)
    (out_a, state_a, stop_a), (out_b, state_b, stop_b) = results
    assert stop_a is None
    assert stop_b == {"stopped": False, "steps_applied": 4, "steps_launched": 4, "kl": None, "limit": float(np.float32(3e38))}
    assert rh.differing(state_a, state_b) == [] and int(state_b["step"]) == 8
    for (rows_a, norms_a), (rows_b, norms_b) in zip(out_a, out_b):
        assert rows_a.shape == (4, 6) and np.array_equal(rh.bits(rows_a), rh.bits(rows_b)) and norms_a == norms_b


_PROBES = {}
SEED = 11          # (of the trainers below: chosen so that the probes' kl rows rise where the two stop tests need them to)


def _probe(n_mini_batch, epochs):
    """A key-absent trainer's first update on ``_perms(epochs)`` -> (statistics rows, norm rows, state)."""
    if (n_mini_batch, epochs) not in _PROBES:
        tr = None
        try:
            tr = rh.trainer(rh.config(n_mini_batch=n_mini_batch, epochs=epochs), seed=SEED, run_id="kl_probe")
            rows, norms = _update(tr, _perms(epochs))
            _PROBES[(n_mini_batch, epochs)] = (rows, norms, rh.state(tr))
        finally:
            rh.release(tr)
    return _PROBES[(n_mini_batch, epochs)]


def _stop_row(kl, allowed):
    """The first row r >= 1 among ``allowed`` whose kl exceeds every earlier row's, and a float32 limit strictly between the two."""
    records = [r for r in range(1, len(kl)) if r in allowed and kl[r] > kl[:r].max()]
    assert records, f"no row of {sorted(allowed)} has a kl above all earlier rows: {kl.tolist()} (another seed is needed)"
    r = records[0]
    limit = float(np.float32((float(kl[:r].max()) + float(kl[r])) / 2))
    assert float(kl[:r].max()) < limit < float(kl[r]), (kl.tolist(), limit)
    return r, limit


def _gated_run(n_mini_batch, epochs, limit, host_check="epoch"):
    tr = None
    try:
        tr = rh.trainer(rh.config(n_mini_batch=n_mini_batch, epochs=epochs, **_kl_key(limit, host_check)), seed=SEED, run_id="kl_gated")
        rows, norms = _update(tr, _perms(epochs))
        return rows, norms, rh.state(tr), tr.last_kl_stop
    finally:
        rh.release(tr)


def test_stop_at_an_epoch_boundary_equals_a_shorter_update():
    rows_p, norms_p, _ = _probe(1, 4)
    kl = rows_p[:, 4]
    print("probe kl (n_mini_batch 1, epochs 4):", kl.tolist())
    # rows 0 and 1 are the eager warm-up steps: from row 2 on the stop falls in a replay of the captured step (and at r = 2 the host
    # check has an epoch left that it must not launch)
    r, limit = _stop_row(kl, allowed={2, 3})
    rows, norms, state, stop = _gated_run(1, 4, limit)
    assert stop["stopped"] and stop["steps_applied"] == r and stop["limit"] == limit
    assert _bits32(stop["kl"]) == _bits32(kl[r]) and stop["steps_launched"] == r + 1
    assert int(state["step"]) == r, "step_dev counts applied steps only"
    assert rows.shape == (r + 1, 6) and np.array_equal(rh.bits(rows), rh.bits(rows_p[: r + 1]))
    for key in norms_p:
        assert len(norms[key]) == r + 1 and norms[key][:r] == norms_p[key][:r], key
    tr = None
    try:                       # the reference runs no gated code: a key-absent trainer with epochs: r on perms[:r]
        tr = rh.trainer(rh.config(n_mini_batch=1, epochs=r), seed=SEED, run_id="kl_short")
        rows_s, _ = _update(tr, _perms(4)[:r])
        assert tr.last_kl_stop is None and np.array_equal(rh.bits(rows_s), rh.bits(rows_p[:r]))
        assert rh.differing(rh.state(tr), state) == []
    finally:
        rh.release(tr)


def test_stop_in_the_middle_of_an_epoch():
    rows_p, _, _ = _probe(2, 3)
    kl = rows_p[:, 4]
    print("probe kl (n_mini_batch 2, epochs 3):", kl.tolist())
    r, limit = _stop_row(kl, allowed={2, 4})               # the first minibatch of an epoch stops: the second one is launched
    rows_e, _, state_e, stop_e = _gated_run(2, 3, limit, "epoch")
    rows_n, _, state_n, stop_n = _gated_run(2, 3, limit, "none")
    for rows, stop in ((rows_e, stop_e), (rows_n, stop_n)):
        assert stop["stopped"] and stop["steps_applied"] == r and _bits32(stop["kl"]) == _bits32(kl[r])
        assert rows.shape == (r + 1, 6) and np.array_equal(rh.bits(rows), rh.bits(rows_p[: r + 1]))
    assert stop_e["steps_launched"] == r + 2 and stop_n["steps_launched"] == 6
    assert rh.differing(state_e, state_n) == [] and int(state_e["step"]) == r
    tr = None
    try:                       # a key-absent trainer driven for exactly r single steps
        tr = rh.trainer(rh.config(n_mini_batch=2, epochs=3), seed=SEED, run_id="kl_single")
        rows_s = _single_steps(tr, _perms(3), r)
        assert np.array_equal(rh.bits(rows_s), rh.bits(rows_p[:r]))
        assert rh.differing(rh.state(tr), state_e) == []
    finally:
        rh.release(tr)


def test_checkpoint_after_a_stopped_update_resumes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rows_p, _, _ = _probe(2, 3)
    r, limit = _stop_row(rows_p[:, 4], allowed={2, 4})
    tr = None
    try:
        tr = rh.trainer(rh.config(n_mini_batch=2, epochs=3, **_kl_key(limit)), seed=SEED, run_id="kl_ckpt")
        _update(tr, _perms(3))
        assert tr.last_kl_stop["stopped"] and tr.last_kl_stop["steps_applied"] == r
        path = tr.save_checkpoint()
        tr.restart_episodes(1)
        rec_a = rh.update(tr)
        stop_a = dict(tr.last_kl_stop)
        assert int(rec_a["step"]) == r + stop_a["steps_applied"]
        tr.load_checkpoint(path)
        assert int(tr.optimizer.step_dev) == r and tr.update_index == 1
        rec_b = rh.update(tr)
        assert rh.differing(rec_a, rec_b) == [] and tr.last_kl_stop == stop_a
    finally:
        rh.release(tr)
