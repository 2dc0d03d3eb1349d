"""What time-limit bootstrapping (``bootstrap_truncated``) costs on the device.

    python tools/truncation_cost.py [kernel] [pass]

kernel: ``etm_gae_truncated`` next to ``etm_gae`` at config 3's shape (W = 32, S = 512) and at W = 65,536, one step in a hundred
        flagged (about 5 truncations per worker at S = 512), boot NaN elsewhere; the library's per-launch HIP events.  Bytes: 13 per
        (worker, step) for etm_gae, 14 + the boot lines around set flags for etm_gae_truncated.
pass:   the bootstrap pass per update at config 3 (configs/synthetic_minigrid.yaml) with about 5 truncations per worker, in both batch
        forms -- W records per replay on fixed operands (the committed form) and one eager call over all records, at a repeated and at
        a new record count -- next to the rollout phase of the same trainer.  The synthetic environment never reports a truncation, so the
        records are made here from the rollout's own episode ends (slot, length and step are the buffer's; the final observation is a random frame).  Host clock
        around work that ends in a device synchronise.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from etm import ops  # noqa: E402

dev = torch.device("cuda", 0)


def kernel_times():
    from scan_roofline import timed
    for W, S in ((32, 512), (65536, 512)):
        gen = torch.Generator().manual_seed(W)
        r, v, last = torch.randn(W, S, generator=gen).to(dev), torch.randn(W, S, generator=gen).to(dev), torch.randn(W, generator=gen).to(dev)
        tr = torch.rand(W, S, generator=gen) < 0.01
        d = (tr | (torch.rand(W, S, generator=gen) < 0.01))
        boot = torch.full((W, S), float("nan"))
        boot[tr] = torch.randn(int(tr.sum()), generator=gen)
        d, tr, boot = d.to(dev), tr.to(dev), boot.to(dev)
        out = torch.empty_like(v)
        n = 200 if W == 32 else 30
        for rep in range(3):              # alternated
            plain = timed(lambda: ops.gae(r, d, v, last, 0.995, 0.95, out=out), n)["gae_kernel"]
            trunc = timed(lambda: ops.gae(r, d, v, last, 0.995, 0.95, out=out, truncated=tr, boot=boot), n)["gae_kernel"]
            none = timed(lambda: ops.gae(r, d, v, last, 0.995, 0.95, out=out, truncated=torch.zeros_like(tr), boot=boot), n)["gae_kernel"]
            print(f"gae W={W} S={S} rep {rep}: etm_gae {plain:8.2f} us ({13 * W * S / plain * 1e-3:7.1f} GB/s at 13 B)   etm_gae_truncated "
                  f"{trunc:8.2f} us ({int(tr.sum())} flags)   etm_gae_truncated without a flag {none:8.2f} us", flush=True)
        assert torch.isfinite(out).all()


def bootstrap_pass_cost(per_worker=5, repeats=12):
    from trainer import PPOTrainer
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(REPO, "episodic-transformer-memory-ppo_amd", "configs", "synthetic_minigrid.yaml")).get_config()
    cfg["bootstrap_truncated"] = True
    torch.manual_seed(0)
    tr = PPOTrainer(cfg, run_id="trunccost", device=dev, tensorboard=False)
    W, S = tr.num_workers, cfg["worker_steps"]
    rng = np.random.default_rng(0)

    def rollout():
        t0 = time.perf_counter()
        tr._sample_training_data()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(3):
        rollout()
    roll = [rollout() for _ in range(5)]
    print(f"rollout phase (key on, no record: the parent's path + one flag upload): {np.mean(roll) * 1e3:.2f} ms "
          f"(min {np.min(roll) * 1e3:.2f}, max {np.max(roll) * 1e3:.2f}) per update of {W * S} steps", flush=True)
    # records from the last rollout's episode ends: (w, t, slot, s = episode length, a random frame)
    dones, slots = tr.buffer.dones, tr.buffer.memory_index_host
    recs = []
    for w in range(W):
        ends = np.flatnonzero(dones[w])
        picks = [i for i in range(1, len(ends))][:per_worker]
        for i in picks:
            t = int(ends[i])
            frame = rng.integers(0, 256, size=tr.observation_space.shape).astype(np.float32) / np.float32(255)
            if tr.observation_dtype == torch.uint8:
                frame = (frame * 255).astype(np.uint8)
            recs.append((w, t, int(slots[w, t]), int(ends[i] - ends[i - 1]), frame))
    print(f"{len(recs)} records ({len(recs) / W:.1f} per worker), episode lengths {min(r[3] for r in recs)} .. {max(r[3] for r in recs)}", flush=True)
    def committed(records):
        tr._truncations = list(records)
        tr._bootstrap_pass()

    def eager(records):                   # the other batch form: one call over all records (not in the product)
        n, w, t, operands = tr._bootstrap_operands(list(records), len(records))
        with torch.no_grad():
            tr.buffer.bootstrap_values[w, t] = tr._bootstrap_forward(*operands)

    def clock(form, records):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        form(records)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    results = {}
    for rep in range(2):                  # alternated
        for chunked, form in ((True, committed), (False, eager)):
            times = [clock(form, recs) for _ in range(4 + repeats)][4:]
            name = f"{W} records per replay" if chunked else "one eager call over all records"
            results.setdefault(chunked, tr.buffer.bootstrap_values.cpu().numpy().copy())
            print(f"bootstrap pass, {name:32s} rep {rep}: {np.mean(times) * 1e3:7.3f} ms per update (min {np.min(times) * 1e3:.3f}, max "
                  f"{np.max(times) * 1e3:.3f}); replayed graph: {tr._bs.graph is not None}", flush=True)
    # the eager form's shapes follow the record count, which changes from update to update: counts not seen before
    fresh = [clock(eager, recs[:n]) for n in range(len(recs) - 1, len(recs) - 9, -1)]
    print(f"bootstrap pass, one eager call, a record count not seen before (tunable_gemm: {cfg.get('tunable_gemm', 'default on')}): "
          f"{np.mean(fresh) * 1e3:7.3f} ms (min {np.min(fresh) * 1e3:.3f}, max {np.max(fresh) * 1e3:.3f})", flush=True)
    a, b = results[True], results[False]
    print(f"the two forms' values: max |difference| {np.abs(a - b).max():.3e} at max |value| {np.abs(b).max():.3e}", flush=True)
    tr.close()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernel", "pass"]
    if "kernel" in what:
        kernel_times()
    if "pass" in what:
        bootstrap_pass_cost()
