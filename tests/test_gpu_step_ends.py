"""-m gpu: the two ends of the captured optimisation step (etm_step_head, etm_group_norms_step / etm_step_end, the table-driven
``_train_epochs``) against the separate entry points and the wiring they replace.  Nothing here has a tolerance: the new launches
move data and run the old kernels' bodies in the old order, so every comparison is ``torch.equal``.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda", 0)


def _fields(rows, dev, gen):
    """Per-sample fields shaped like the flattened buffer's: scalars, an action row, int64 windows, a bool mask, an odd float row."""
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    return [r(rows) * 3.0 + 0.5,                                                       # advantages
            r(rows), r(rows),                                                          # values, log-probabilities
            torch.randint(0, 7, (rows, 1), generator=gen).to(dev),                     # actions (int64)
            torch.randint(0, 96, (rows, 64), generator=gen).to(dev),                   # memory_indices
            (torch.rand(rows, 64, generator=gen) < 0.5).to(dev),                       # memory_mask (bool, 64 bytes a row)
            torch.randint(0, 40, (rows,), generator=gen).to(dev),                      # memory_index
            r(rows, 5)]


@pytest.mark.parametrize("n", [2048, 1237])
def test_head_launch_gives_the_separate_entry_points_bits(n):
    """etm_step_head against etm_gather_rows and ops.adv_stats at minibatch 2048 and at a size that is a multiple of no tile (1237:
    prime), for every row of the index table the counter can select, with and without the optional jobs."""
    from etm import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(11 + n)
    rows, table_rows = 16384, 8
    fields = _fields(rows, dev, gen)
    table = torch.stack([torch.randperm(rows, generator=gen)[:n].sort().values for _ in range(table_rows)]).to(dev)
    table[3, :5] = torch.tensor([-4, rows, rows + 9, 0, rows - 1], device=dev)        # out of range: clamped like the gather clamps
    counter = torch.zeros(1, dtype=torch.long, device=dev)
    for c in (0, 1, 3, 7, 8, 21):
        counter.fill_(c)
        idx = table[c % table_rows].clone()
        want = ops.gather_rows(fields, idx)
        want_stats = ops.adv_stats(want[0])
        idx_out = torch.full((n,), -1, dtype=torch.long, device=dev)
        got, got_stats = ops.step_head(fields, table, counter, idx_out=idx_out, adv_src=fields[0])
        assert torch.equal(idx_out, idx)
        assert torch.equal(got_stats, want_stats), (c, got_stats, want_stats)
        assert len(got) == len(want) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, want))
        assert int(counter) == c, "the head launch only reads the counter"
    # no counter: row 0; no index copy, no statistics
    got, none = ops.step_head(fields, table, None)
    assert none is None and all(torch.equal(a, b) for a, b in zip(got, ops.gather_rows(fields, table[0].clone())))
    # a field the gather launch does not take (rows of 6 bytes) goes through index_select on the copied indices
    odd = torch.randint(0, 100, (rows, 3), generator=gen).to(torch.int16).to(dev)
    counter.fill_(2)
    idx_out = torch.empty(n, dtype=torch.long, device=dev)
    got, _ = ops.step_head([fields[1], odd], table, counter, idx_out=idx_out)
    assert torch.equal(got[1], odd.index_select(0, table[2])) and torch.equal(got[0], fields[1].index_select(0, table[2]))


def _norm_problem(dev, gen, n_floats=70000, n_groups=5):
    flat = torch.randn(n_floats, generator=gen).to(dev)
    starts, lens = [], []
    off = 0
    while off < n_floats:                           # segments of <= 4096 floats, some short
        ln = min(4096 if len(starts) % 3 else 1000, n_floats - off)
        starts.append(off)
        lens.append(ln)
        off += ln
    member = (torch.rand(n_groups, len(starts), generator=gen) < 0.4).float()
    return (flat, torch.tensor(starts, dtype=torch.int64, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev), member.to(dev),
            torch.empty(len(starts), dtype=torch.float32, device=dev))


def _norms(lib_mod, prob, step=None):
    flat, seg_start, seg_len, member, partial = prob
    out = torch.empty(member.shape[0], dtype=torch.float32, device=flat.device)
    st = torch.cuda.current_stream(flat.device).cuda_stream
    h = lib_mod.load()
    if step is None:
        lib_mod.check(h.etm_group_norms(flat.data_ptr(), seg_start.data_ptr(), seg_len.data_ptr(), seg_start.numel(), member.data_ptr(),
                                        member.shape[0], partial.data_ptr(), out.data_ptr(), st), "etm_group_norms")
    else:
        stats, stats_tab, norm_tab, counter = step
        lib_mod.check(h.etm_group_norms_step(flat.data_ptr(), seg_start.data_ptr(), seg_len.data_ptr(), seg_start.numel(), member.data_ptr(),
                                             member.shape[0], partial.data_ptr(), out.data_ptr(), norm_tab.data_ptr(), stats.data_ptr(),
                                             stats.numel(), stats_tab.data_ptr(), stats_tab.shape[0], counter.data_ptr(), st),
                      "etm_group_norms_step")
    return out


def test_step_end_files_rows_and_advances_the_counter():
    from etm import lib
    dev = _dev()
    gen = torch.Generator().manual_seed(5)
    prob = _norm_problem(dev, gen)
    steps, n_groups = 6, prob[3].shape[0]
    stats_tab = torch.full((steps, 6), -1.0, device=dev)
    norm_tab = torch.full((steps, n_groups), -1.0, device=dev)
    counter = torch.zeros(1, dtype=torch.long, device=dev)
    rows, norms = [], []
    for k in range(steps):
        prob[0].mul_(1.25)
        stats = torch.randn(6, generator=gen).to(dev)
        want = _norms(lib, prob)
        got = _norms(lib, prob, (stats, stats_tab, norm_tab, counter))
        assert torch.equal(got, want)
        assert int(counter) == k + 1
        rows.append(stats)
        norms.append(want)
        assert torch.equal(stats_tab[: k + 1], torch.stack(rows)) and torch.equal(norm_tab[: k + 1], torch.stack(norms))
        assert bool((stats_tab[k + 1:] == -1).all()) and bool((norm_tab[k + 1:] == -1).all())
    # beyond the table: the last row takes it, nothing outside is written (the tables are views into a guarded buffer)
    guard = torch.full((steps + 2, 6), -7.0, device=dev)
    tab = guard[1: steps + 1]
    counter.fill_(steps + 3)
    stats = torch.randn(6, generator=gen).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib.check(lib.load().etm_step_end(stats.data_ptr(), 6, tab.data_ptr(), steps, counter.data_ptr(), st), "etm_step_end")
    assert int(counter) == steps + 4 and torch.equal(tab[steps - 1], stats)
    assert bool((guard[0] == -7).all()) and bool((guard[-1] == -7).all()) and bool((tab[: steps - 1] == -7).all())
    counter.fill_(2)
    lib.check(lib.load().etm_step_end(stats.data_ptr(), 6, tab.data_ptr(), steps, counter.data_ptr(), st), "etm_step_end")
    assert int(counter) == 3 and torch.equal(tab[2], stats)


def test_captured_step_ends_walk_the_tables_in_every_replay():
    """Head and end launches in ONE captured graph, replayed 600 times with nothing in between: replay k must read row k % 8 of the
    index table and file its results in row k, the bits of the eager separate entry points."""
    from etm import lib, ops
    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    rows, n, table_rows, replays = 8192, 1536, 8, 600
    fields = _fields(rows, dev, gen)
    table = torch.stack([torch.randperm(rows, generator=gen)[:n] for _ in range(table_rows)]).to(dev)
    prob = list(_norm_problem(dev, gen, n_floats=n * 5))
    counter = torch.zeros(1, dtype=torch.long, device=dev)
    idx_out = torch.empty(n, dtype=torch.long, device=dev)
    stats = torch.empty(6, device=dev)
    stats_tab = torch.zeros((replays, 6), device=dev)
    norm_tab = torch.zeros((replays, prob[3].shape[0]), device=dev)
    live = {}

    def body():
        got, st3 = ops.step_head(fields, table, counter, idx_out=idx_out, adv_src=fields[0])
        prob[0].copy_(got[7].reshape(-1))                     # the "gradient arena" of this step: a gathered field
        stats[:3].copy_(st3)
        stats[3:].copy_(got[1][:3])
        live["norms"] = _norms(lib, prob, (stats, stats_tab, norm_tab, counter))

    want_stats, want_norms = [], []
    for r in range(table_rows):                                # eager, separate entry points
        idx = table[r].clone()
        g = ops.gather_rows(fields, idx)
        prob[0].copy_(g[7].reshape(-1))
        want_stats.append(torch.cat([ops.adv_stats(g[0]), g[1][:3]]))
        want_norms.append(_norms(lib, prob))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    counter.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    counter.zero_()
    for _ in range(replays):
        graph.replay()
    assert int(counter) == replays
    for k in range(replays):
        assert torch.equal(stats_tab[k], want_stats[k % table_rows]), f"replay {k}: statistics row"
        assert torch.equal(norm_tab[k], want_norms[k % table_rows]), f"replay {k}: norm row"
    assert torch.equal(idx_out, table[(replays - 1) % table_rows])


def _trainer_pair(golden_dir, name, n_mini_batch, epochs):
    """Two trainers of the fixture's model and rollout shape from the same start -- deterministic weights, the fixture's forced
    actions -- one on today's wiring of the step's ends, one on the wiring before it."""
    import detgen as dg
    from trainer import PPOTrainer
    dev = _dev()
    z = np.load(os.path.join(golden_dir, f"rollout_{name}.npz"), allow_pickle=False)
    info = json.loads(str(z["cfg_json"]))
    keys = [str(k) for k in z["keys"]]
    shapes = [tuple(int(x) for x in str(s).split(",") if x) for s in z["shapes"]]
    out = []
    for fused in (True, False):
        cfg = {**info["cfg"], "environment": {"type": "Synthetic", **info["env"]}, "n_mini_batch": n_mini_batch, "epochs": epochs,
               "step_ends_fused": fused}
        tr = PPOTrainer(cfg, run_id="step_ends", device=dev, tensorboard=False)
        gen = dg.det_state_dict("rollout_" + name, keys, shapes)
        sd = tr.model.state_dict()
        tr.model.load_state_dict({k: (torch.from_numpy(gen[k]) if k in gen else sd[k]) for k in keys})
        tr._sample_training_data(forced_actions=z["u0/actions"][:, :, 0])
        tr.buffer.prepare_batch_dict()
        out.append(tr)
    return out


@pytest.mark.parametrize("name,n_mini_batch,epochs", [("cfg3", 4, 3), ("cfg5", 4, 3)])
def test_train_epochs_same_bits_as_the_wiring_before(golden_dir, name, n_mini_batch, epochs):
    """One whole ``_train_epochs`` call (all epochs and minibatches, explicit permutations; two eager warm-up steps, the capture, then
    replays) through the table-driven step and through the wiring before it (``step_ends_fused: false``: index copy in front of every
    replay, clones behind it): every statistics row, every gradient-norm row and every parameter ``torch.equal``, in the same order."""
    new, old = _trainer_pair(golden_dir, name, n_mini_batch, epochs)
    try:
        for k in new.buffer.samples_flat:
            assert torch.equal(new.buffer.samples_flat[k], old.buffer.samples_flat[k]), f"the two rollouts differ in {k}: nothing to compare"
        rng = np.random.default_rng(4)
        perms = [rng.permutation(new.buffer.batch_size) for _ in range(epochs)]
        results = []
        for tr in (new, old):
            stats, norms = tr._train_epochs(3e-4, 0.15, 5e-3, perms=perms)
            torch.cuda.synchronize()
            assert tr._train_graph is not None, "the step must have been captured and replayed"
            results.append((np.stack(stats), norms))
        assert getattr(new, "_tg_idx_table", None) is not None and getattr(old, "_tg_idx_table", None) is None
        assert int(new._tg_counter) == epochs * n_mini_batch
        (s_new, n_new), (s_old, n_old) = results
        assert s_new.shape == (epochs * n_mini_batch, 6) and s_new.dtype == s_old.dtype
        assert np.array_equal(s_new, s_old), np.abs(s_new - s_old).max()
        assert list(n_new) == list(n_old) and len(n_new) > 0
        for key in n_new:
            assert len(n_new[key]) == epochs * n_mini_batch and n_new[key] == n_old[key], key
        for (ka, a), (kb, b) in zip(new.model.state_dict().items(), old.model.state_dict().items()):
            assert ka == kb and torch.equal(a, b), ka
        # a second update on the same tables (counter reset, graph replayed from its first step on)
        perms = [rng.permutation(new.buffer.batch_size) for _ in range(epochs)]
        again = [tr._train_epochs(2e-4, 0.1, 1e-3, perms=perms) for tr in (new, old)]
        assert np.array_equal(np.stack(again[0][0]), np.stack(again[1][0])) and again[0][1] == again[1][1]
        for (ka, a), (kb, b) in zip(new.model.state_dict().items(), old.model.state_dict().items()):
            assert torch.equal(a, b), ka
        # single steps asked for from outside _train_epochs (the parity tests do): same values on both wirings, eager sample included
        idx = torch.as_tensor(perms[0][: new.buffer.batch_size // n_mini_batch], device=new.device).sort().values
        with torch.no_grad():
            for tr in (new, old):
                tr._bank_pos, tr._obs_train = tr._bank_with_positions(), tr._observations_channels_last()
        one = [tr._train_step_graph(idx, 2e-4, 0.1, 1e-3, True) for tr in (new, old)]
        assert torch.equal(one[0][0], one[1][0]) and torch.equal(one[0][1], one[1][1])
        new.profile_sample_every, old.profile_sample_every = 1, 1            # every step eager
        one = [tr._train_step_graph(idx, 2e-4, 0.1, 1e-3, True) for tr in (new, old)]
        assert torch.equal(one[0][0], one[1][0]) and torch.equal(one[0][1], one[1][1])
        for (ka, a), (kb, b) in zip(new.model.state_dict().items(), old.model.state_dict().items()):
            assert torch.equal(a, b), ka
    finally:
        new.close()
        old.close()


def _recorded_step(golden_dir, name):
    """A trainer of the fixture's shape and the problem lists that one real backward pass of it hands to ``DeferredDw.flush``."""
    import detgen as dg
    from etm import ops
    from trainer import PPOTrainer
    dev = _dev()
    z = np.load(os.path.join(golden_dir, f"rollout_{name}.npz"), allow_pickle=False)
    info = json.loads(str(z["cfg_json"]))
    keys = [str(k) for k in z["keys"]]
    shapes = [tuple(int(x) for x in str(s).split(",") if x) for s in z["shapes"]]
    cfg = {**info["cfg"], "environment": {"type": "Synthetic", **info["env"]}}
    tr = PPOTrainer(cfg, run_id="step_tail", device=dev, tensorboard=False)
    gen = dg.det_state_dict("rollout_" + name, keys, shapes)
    sd = tr.model.state_dict()
    tr.model.load_state_dict({k: (torch.from_numpy(gen[k]) if k in gen else sd[k]) for k in keys})
    tr._sample_training_data(forced_actions=z["u0/actions"][:, :, 0])
    tr.buffer.prepare_batch_dict()
    rec = {}
    orig = ops.DeferredDw.flush

    def flush(self):
        rec.update(items=list(self.items), colsums=list(self.colsums), wgrads=list(self.conv_wgrads), N=self.N)
        orig(self)

    mbs = tr.buffer.batch_size // tr.buffer.n_mini_batches
    idx = torch.arange(mbs, device=dev)
    with torch.no_grad():
        tr._bank_pos, tr._obs_train = tr._bank_with_positions(), tr._observations_channels_last()
    ops.DeferredDw.flush = flush
    try:
        tr._train_body_a(idx, 0.2, 1e-2)
    finally:
        ops.DeferredDw.flush = orig
    torch.cuda.synchronize()
    return tr, rec


@pytest.mark.parametrize("name", ["cfg3", "cfg5", "cfg2"])
def test_tail_launch_gives_the_separate_launches_bits(golden_dir, name):
    """etm_grouped_dw_tail against etm_colsum_reduce_grouped + etm_grouped_dw (the slice reduction stays a launch of its own in both:
    ``flush()`` as a whole is compared) on the problem lists of
    a real step of the config-3, config-5 and config-2 shaped models (every destination is a view of the flat gradient arena, which is
    compared whole), eagerly and from a captured graph replayed 600 times."""
    from etm import lib, ops
    tr, rec = _recorded_step(golden_dir, name)
    try:
        assert rec["colsums"], "the step handed no grouped reductions over: nothing to compare"
        # (config 2: D = 128 is no multiple of the grouped kernel's 96-row tiles, its layers multiply their own weight gradients -- no
        # launch for the reductions to ride in, flush() keeps their own; the comparison below still runs on what the step hands over)
        assert bool(rec["items"]) == (name != "cfg2")
        assert bool(rec["wgrads"]) == (name != "cfg2"), "visual configs hand their encoder's slices over"
        flat = tr.flat_grads
        assert lib.load().etm_grouped_dw_tail_max_problems() >= 1

        def run(tail):
            d = ops.DeferredDw({}, tail=tail)
            d.items, d.colsums, d.conv_wgrads, d.N = list(rec["items"]), list(rec["colsums"]), list(rec["wgrads"]), rec["N"]
            d.flush()

        flat.zero_()
        run(False)
        want = flat.clone()
        assert int((want != 0).sum()) > 1000, "the recorded problems wrote next to nothing: nothing to compare"
        flat.fill_(float("nan"))
        run(True)
        got = flat.clone()
        flat.fill_(float("nan"))
        run(False)
        assert torch.equal(torch.isnan(got), torch.isnan(flat)), "the tail launch writes another set of elements"
        written = ~torch.isnan(got)
        assert torch.equal(got[written], want[written]) and bool((want[~written] == 0).all())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(True)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run(True)
        for it in range(600):
            flat.zero_()
            graph.replay()
            assert torch.equal(flat, want), f"replay {it}: the tail launch differs from the separate launches"
    finally:
        tr.close()
