"""Measurements behind checkpoint and resume (profiles/r13/resume.txt).

    python tools/resume_measure.py [gap] [digest] [save]

gap:    the largest relative parameter difference between an EAGER and a GRAPH trainer (hip_graph_rollout / hip_graph_train off / on) on
        the tiny config of tests/resume_helpers.py after two updates from identical weights, draws and permutations -- what a freshly
        resumed graph-mode trainer (its first minibatches run as eager warm-up) may differ by from an uninterrupted one that replays.
        Uses nothing of the checkpoint code: the figure is a property of the trainer as it was before it.
digest: ``etm_arena_digest`` at the arena of configs/synthetic_minigrid.yaml (BASELINE config 3) and at 16 x that size, device events
        around 200 calls, three repetitions; the bytes it must read are 4 per float.
save:   ``save_checkpoint`` (three digests, the model file, the training checkpoint) at config 3 next to the update it follows: host clock
        around work that ends in a device synchronise, alternated update / save pairs in one process, files in a temporary directory.
"""
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

dev = torch.device("cuda", 0)
HBM_PEAK = 8.0e12          # bytes / s (MI355X_MICROARCH: 8 TB/s HBM3E)


def gap():
    import resume_helpers as rh
    rng = np.random.default_rng(0)
    draws = [(rng.random((rh.W_T, rh.S_T)).astype(np.float32), [rng.permutation(rh.W_T * rh.S_T) for _ in range(2)]) for _ in range(2)]
    recs = {}
    for graph in (False, True):
        tr = rh.trainer(rh.config(**rh.modes(graph)), seed=11, run_id="gap")
        recs[graph] = [rh.update(tr, uniforms=u, perms=p) for u, p in draws]
        assert (tr._train_graph is not None) == graph and (tr._step_graph is not None) == graph
        rh.release(tr)
    for k, (a, b) in enumerate(zip(recs[False], recs[True])):
        print(f"eager against graph, update {k}: largest relative parameter difference "
              f"{rh.largest_relative_parameter_difference(a, b):.3e}; recorded arrays that differ in a bit: {rh.differing(a, b) or 'none'}", flush=True)


def _config3(**over):
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(REPO, "episodic-transformer-memory-ppo_amd", "configs", "synthetic_minigrid.yaml")).get_config()
    cfg.update(tunable_gemm=False, **over)
    return cfg


def digest(n_config3):
    from etm import ops
    for n in (n_config3, 16 * n_config3):
        x = torch.randn(n, device=dev)
        out, partial = torch.zeros(4, dtype=torch.int64, device=dev), ops.arena_digest_workspace(dev)
        for _ in range(20):
            ops.arena_digest(x, out=out, partial=partial)
        for rep in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(200):
                ops.arena_digest(x, out=out, partial=partial)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / 200 * 1e3
            print(f"etm_arena_digest n={n} ({4 * n / 1e6:.1f} MB) rep {rep}: {us:8.2f} us per call (2 launches, back to back)  "
                  f"{4 * n / us * 1e-6:6.2f} TB/s = {4 * n / (us * 1e-6) / HBM_PEAK * 100:5.1f} % of the HBM peak", flush=True)


def save(pairs=5):
    from trainer import PPOTrainer
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        os.chdir(work)
        try:
            torch.manual_seed(0)
            tr = PPOTrainer(_config3(), run_id="savecost", device=dev, tensorboard=False)
            n = tr.optimizer.flat_params.numel()

            def update():
                lr, beta, clip = tr.schedules(tr.update_index)
                tr._sample_training_data()
                tr.buffer.prepare_batch_dict()
                tr._train_epochs(lr, clip, beta)
                tr.update_index += 1

            def clock(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for _ in range(3):
                update()
            tr.save_checkpoint()
            rows = []
            for pair in range(pairs):
                u, s, d = clock(update), clock(tr.save_checkpoint), clock(tr.state_digest)
                rows.append((u, s, d))
                print(f"pair {pair}: update {u:8.2f} ms   save_checkpoint {s:8.2f} ms   state_digest {d:6.3f} ms", flush=True)
            u, s, d = np.array(rows).T
            size = {f: os.path.getsize(os.path.join("models", f)) for f in sorted(os.listdir("models"))}
            print(f"arena {n} floats; files {size}", flush=True)
            print(f"update {u.min():.1f} - {u.max():.1f} ms, save_checkpoint {s.min():.1f} - {s.max():.1f} ms = {np.mean(s) / np.mean(u) * 100:.1f} % "
                  f"of an update at checkpoint_interval: 1; state_digest {d.min():.3f} - {d.max():.3f} ms", flush=True)
            tr.close()
        finally:
            os.chdir(cwd)
    return n


if __name__ == "__main__":
    what = sys.argv[1:] or ["gap", "digest", "save"]
    n3 = 3_940_000
    if "gap" in what:
        gap()
    if "save" in what:
        n3 = save()
    if "digest" in what:
        digest(n3)
