"""-m gpu: ``attention_statistics: true`` through the trainer, on a small vector-observation config (4 workers, 16 steps, a window of
8, two blocks, two heads, two epochs of two minibatches).

1. Observing changes nothing: after two updates the training state, the buffer's values, log-probs and advantages equal the key-off
   trainer's under ``==``, with the optimisation step captured and eager.
2. Key off: nothing hangs on the model, ``last_attention_statistics`` is None.
3. Counts of the last update per block and head: rows + empty + irregular = epochs x batch, no irregular row, the empty rows are the
   buffer's samples without a valid window entry (x epochs), the two histograms carry the same mass, and that mass is the number of
   counted rows within the attention kernels' own fp32 softmax rounding.
4. Values: the eager trainer's table equals the float64 reference accumulated over a copy of every (att, mask) ``ops.attn_stats`` was
   handed, within the bounds of the kernel test (tests/test_attention_statistics_gpu.py).
5. The captured and the eager trainer's tables agree to the same bounds, their counters exactly.

Every trainer runs once per module (four in all) and is shared by the tests."""
import gc

import numpy as np
import pytest
import torch

import attention_statistics_reference as ar

pytestmark = pytest.mark.gpu

W, S, L, BLOCKS, HEADS, EPOCHS, N_MB = 4, 16, 8, 2, 2, 2, 2
BATCH = W * S


def _config(graph, key):
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[4], num_actions=3, max_episode_steps=12, seed=0, p_done=0.05, pool=8),
               gamma=0.99, lamda=0.95, updates=2, epochs=EPOCHS, n_workers=W, worker_steps=S, n_mini_batch=N_MB,
               value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False, hip_graph_train=graph,
               transformer=dict(num_blocks=BLOCKS, embed_dim=64, num_heads=HEADS, memory_length=L, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    if key:
        cfg["attention_statistics"] = True
    return cfg


_runs = {}


def _run(graph, key):
    """Two updates of one trainer -> what the tests look at.  The eager trainer with the key also keeps a copy of every operand pair
    ``ops.attn_stats`` is handed during the last update, and the float64 reference accumulated over them."""
    if (graph, key) in _runs:
        return _runs[(graph, key)]
    from etm import ops
    from trainer import PPOTrainer
    gc.collect()
    torch.manual_seed(5)
    tr = PPOTrainer(_config(graph, key), run_id="attention_statistics", device=torch.device("cuda", 0), tensorboard=False)
    real, seen = ops.attn_stats, []

    def recording(att, mask, table_rows, workspace):
        block = (table_rows.data_ptr() - tr._attn_stats.table.data_ptr()) // (HEADS * ar.WORDS * 8)
        seen.append((int(block), att.detach().cpu().numpy().copy(), mask.cpu().numpy().copy()))
        return real(att, mask, table_rows, workspace)

    out = {}
    try:
        out["off"] = (tr.last_attention_statistics is None, tr.model.transformer.attn_stats is None, tr._attn_stats is None)
        if key and not graph:
            ops.attn_stats = recording
        for upd in range(2):
            torch.manual_seed(9 + upd)
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            del seen[:]
            torch.manual_seed(20 + upd)
            tr._train_epochs(3e-4, 0.1, 1e-3)
        torch.cuda.synchronize()
        out["captured"] = tr._train_graph is not None
        out["digest"] = tr.state_digest()
        out["buffer"] = {k: getattr(tr.buffer, k).cpu().numpy() for k in ("values", "log_probs", "advantages")}
        out["empty_samples"] = int((~tr.buffer.memory_mask.reshape(-1, L).any(dim=1)).sum().item())
        out["summary"] = tr.last_attention_statistics
        out["off_after"] = (tr.last_attention_statistics is None, tr.model.transformer.attn_stats is None)
        if key:
            out["table"] = tr._attn_stats.read()
        if seen:
            ref = np.zeros((BLOCKS, HEADS, ar.WORDS))
            for block, att, mask in seen:
                ref[block] += ar.attention_statistics_reference(att, mask)
            out["reference"], out["calls"] = ref, len(seen)
    finally:
        ops.attn_stats = real
        tr.close()
        del tr
        gc.collect()
        torch.cuda.synchronize()
    _runs[(graph, key)] = out
    return out


def _close(got, ref, tag):
    """Two tables [BLOCKS, HEADS, 264] within the kernel test's bounds: counters equal, double sums of fp32 values to rtol 1e-11,
    the entropy words within ``entropy_bound`` of the rows counted."""
    assert np.array_equal(got[:, :, :4], ref[:, :, :4]), tag
    exact = np.r_[6, ar.AGE0: ar.WORDS]
    print(f"\n[attention statistics] {tag}: max |diff| of the double sums {np.abs(got[:, :, exact] - ref[:, :, exact]).max():.3g}, "
          f"of the entropy words {np.abs(got[:, :, 4:6] - ref[:, :, 4:6]).max():.3g} (bound {ar.entropy_bound(ref[:, :, 0].min(), L):.3g})",
          flush=True)
    assert np.allclose(got[:, :, exact], ref[:, :, exact], rtol=1e-11, atol=0.0), tag
    for b, h in np.ndindex(BLOCKS, HEADS):
        bound = ar.entropy_bound(ref[b, h, 0], L)
        assert abs(got[b, h, 4] - ref[b, h, 4]) <= bound and abs(got[b, h, 5] - ref[b, h, 5]) <= bound, (tag, b, h)


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_observing_changes_nothing(graph):
    off, on = _run(graph, False), _run(graph, True)
    assert off["captured"] == graph and on["captured"] == graph
    for k in off["buffer"]:
        assert np.array_equal(off["buffer"][k], on["buffer"][k]), k
    assert off["digest"] == on["digest"], (off["digest"], on["digest"])


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_key_off_allocates_nothing(graph):
    off, on = _run(graph, False), _run(graph, True)
    assert off["off"] == (True, True, True) and off["off_after"] == (True, True) and off["summary"] is None
    assert on["off"] == (True, False, False) and on["off_after"] == (False, False)


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_counts_of_the_last_update(graph):
    on = _run(graph, True)
    s, table = on["summary"], on["table"]
    assert set(s) == {"rows", "empty", "irregular", "entropy", "normalised_entropy", "max_prob", "mean_age", "age_hist", "index_hist"}
    assert s["rows"].shape == (BLOCKS, HEADS) and s["age_hist"].shape == (BLOCKS, HEADS, L) and s["index_hist"].shape == (BLOCKS, HEADS, L)
    assert on["empty_samples"] >= W                     # (every worker's first step has nothing stored yet)
    age_mass, index_mass = table[:, :, ar.AGE0: ar.AGE0 + L].sum(axis=2), table[:, :, ar.INDEX0: ar.INDEX0 + L].sum(axis=2)
    print(f"\n[attention statistics] rows {s['rows'].tolist()} empty {s['empty'].tolist()} mass - rows {(age_mass - s['rows']).tolist()}", flush=True)
    assert (s["rows"] + s["empty"] + s["irregular"] == EPOCHS * BATCH).all()
    assert (s["irregular"] == 0).all()
    assert (s["empty"] == EPOCHS * on["empty_samples"]).all()
    assert np.allclose(age_mass, index_mass, rtol=1e-11, atol=0.0)
    assert (np.abs(age_mass - s["rows"]) <= s["rows"] * 1e-4).all()
    assert (table[:, :, ar.AGE0 + L: ar.INDEX0] == 0).all() and (table[:, :, ar.INDEX0 + L:] == 0).all() and (table[:, :, 7] == 0).all()
    for key in ("entropy", "normalised_entropy", "max_prob", "mean_age"):
        assert np.isfinite(s[key]).all(), key
    assert ((s["normalised_entropy"] >= 0) & (s["normalised_entropy"] <= 1 + 1e-6)).all()
    assert ((s["mean_age"] >= 1) & (s["mean_age"] <= L)).all() and ((s["max_prob"] > 0) & (s["max_prob"] <= 1 + 1e-6)).all()
    assert np.allclose(s["age_hist"].sum(axis=2), 1.0) and np.allclose(s["index_hist"].sum(axis=2), 1.0)


def test_eager_table_equals_the_reference_over_what_was_handed_over():
    on = _run(False, True)
    assert on["calls"] == EPOCHS * N_MB * BLOCKS
    _close(on["table"], on["reference"], "eager trainer against float64")


def test_captured_table_equals_the_eager_one():
    _close(_run(True, True)["table"], _run(False, True)["table"], "captured against eager")
