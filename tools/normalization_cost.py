"""What the running normalisations (``normalize_observations`` / ``normalize_rewards``) cost on the device.

    python tools/normalization_cost.py [kernel] [step] [update]

kernel: ``etm_obs_stats_update`` at 4,096 x 4 (configs/synthetic_cartpole.yaml: 16 workers x 256 steps) and 16,384 x 4 rows,
        ``etm_return_scale`` at 16 x 256 and at 65,536 workers x 512 steps next to ``etm_gae`` at the same sizes, ``etm_obs_normalize``
        at 16 x 4 (a rollout step) and 1,024 x 4 (a minibatch); the library's per-launch HIP events around each ENTRY (all of its
        launches), three alternated repetitions.  Bytes each must read or write: 4 per element for the statistics; 4 + 1 (scan) +
        4 + 4 (scaling) = 13 per (worker, step) for the return scaling; 13 for etm_gae.
step:   the captured step graph of one worker group at synthetic_cartpole's shape, replayed back to back, with
        ``normalize_observations`` on against the same config with it off -- five alternated pairs in one process.
update: both keys on: the observation update and the return scaling per update, next to the optimisation phase of the same trainer
        (host clock around work that ends in a device synchronise).
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
HBM_PEAK = 8.0e12          # bytes / s (MI355X_MICROARCH: 8 TB/s HBM3E)


def _config(**over):
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(REPO, "episodic-transformer-memory-ppo_amd", "configs", "synthetic_cartpole.yaml")).get_config()
    cfg.update(over)
    return cfg


def kernel_times():
    from scan_roofline import timed
    key = "running_norm_kernels"
    for R, F in ((4096, 4), (16384, 4)):
        gen = torch.Generator().manual_seed(R)
        x = (torch.randn(R, F, generator=gen) * 3 + 5).to(dev)
        stats, mean, rstd = torch.zeros((3, F), dtype=torch.float64, device=dev), torch.zeros(F, device=dev), torch.ones(F, device=dev)
        for rep in range(3):
            us = timed(lambda: ops.obs_stats_update(x, stats, mean, rstd, 1e-8), 200)[key]
            print(f"obs_stats_update R={R} F={F} rep {rep}: {us:8.2f} us (2 launches)  {4 * R * F / us * 1e-3:8.2f} GB/s = "
                  f"{4 * R * F / (us * 1e-6) / HBM_PEAK * 100:.3f} % of the HBM peak on {4 * R * F} bytes", flush=True)
    for N, F in ((16, 4), (1024, 4)):
        x = torch.randn(N, F).to(dev)
        mean, rstd, out = torch.zeros(F, device=dev), torch.ones(F, device=dev), torch.empty((N, F), device=dev)
        for rep in range(3):
            us = timed(lambda: ops.obs_normalize(x, mean, rstd, 10.0, out=out), 200)[key]
            print(f"obs_normalize N={N} F={F} rep {rep}: {us:8.2f} us", flush=True)
    for W, S in ((16, 256), (65536, 512)):
        gen = torch.Generator().manual_seed(W)
        r, v, last = torch.randn(W, S, generator=gen).to(dev), torch.randn(W, S, generator=gen).to(dev), torch.randn(W, generator=gen).to(dev)
        d = (torch.rand(W, S, generator=gen) < 0.02).to(dev)
        carry, stats = torch.zeros(W, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
        scaled, adv, ws = torch.empty_like(r), torch.empty_like(r), ops.return_scale_workspace(W, dev)
        n = 200 if W == 16 else 30
        for rep in range(3):              # alternated
            ret = timed(lambda: ops.return_scale(r, d, carry, stats, 0.99, 1e-8, 10.0, out=scaled, ws=ws), n)[key]
            gae = timed(lambda: ops.gae(r, d, v, last, 0.99, 0.95, out=adv), n)["gae_kernel"]
            print(f"W={W} S={S} rep {rep}: etm_return_scale {ret:8.2f} us (3 launches; {13 * W * S / ret * 1e-3:7.1f} GB/s at 13 B = "
                  f"{13 * W * S / (ret * 1e-6) / HBM_PEAK * 100:.2f} % of the HBM peak)   etm_gae {gae:8.2f} us "
                  f"({13 * W * S / gae * 1e-3:7.1f} GB/s at 13 B)", flush=True)
        assert torch.isfinite(scaled).all() and torch.isfinite(stats).all()


def _trainer(cfg, run_id):
    from trainer import PPOTrainer
    torch.manual_seed(0)
    tr = PPOTrainer(cfg, run_id=run_id, device=dev, tensorboard=False)
    for _ in range(2):
        tr._sample_training_data()
    torch.cuda.synchronize()
    return tr


def _step_graph_us(tr):
    g0, S = tr._groups[0], tr.config["worker_steps"]
    n = max(1, min(200, S - 8))          # the step counter must stay inside the staging arrays
    g0.t_dev.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(g0.stream):
        e0.record()
        for _ in range(n):
            g0.graphs[0].replay()
        e1.record()
    torch.cuda.synchronize()
    g0.t_dev.zero_()
    return e0.elapsed_time(e1) / n * 1e3


def step_graph_cost(pairs=5):
    off, on = _trainer(_config(), "normcost_off"), _trainer(_config(normalize_observations=True), "normcost_on")
    assert off._step_graph is not None and on._step_graph is not None
    print(f"step graph of one group ({on._groups[0].W} of {on.num_workers} workers, {len(on._groups)} groups), replayed back to back", flush=True)
    rows = []
    for pair in range(pairs):
        a, b = _step_graph_us(off), _step_graph_us(on)
        rows.append((a, b))
        print(f"pair {pair}: key off {a:7.2f} us   normalize_observations on {b:7.2f} us   difference {b - a:+6.2f} us", flush=True)
    a, b = np.array(rows).T
    print(f"key off {a.min():.2f} - {a.max():.2f} us, on {b.min():.2f} - {b.max():.2f} us; difference {np.mean(b - a):+.2f} us "
          f"(pairs {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}); scatter of the off runs {a.max() - a.min():.2f} us", flush=True)

    def rollout(tr):
        t0 = time.perf_counter()
        tr._sample_training_data()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for pair in range(pairs):
        a, b = rollout(off), rollout(on)
        print(f"rollout phase pair {pair}: key off {a:7.2f} ms   on {b:7.2f} ms", flush=True)
    off.close()
    on.close()


def update_cost(repeats=8):
    tr = _trainer(_config(normalize_observations=True, normalize_rewards=True), "normcost_both")
    buf = tr.buffer

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def optimise():
        tr._train_epochs(3e-4, 0.2, 1e-3)

    tr.buffer.prepare_batch_dict()
    for _ in range(3):
        optimise()
    opt = [clock(optimise) for _ in range(repeats)]
    upd = [clock(tr._update_obs_norm) for _ in range(repeats + 4)][4:]
    last = tr.get_last_value()
    adv = [clock(lambda: buf.calc_advantages(last, 0.99, 0.95)) for _ in range(repeats + 4)][4:]
    rn, buf.return_norm = buf.return_norm, None
    adv_off = [clock(lambda: buf.calc_advantages(last, 0.99, 0.95)) for _ in range(repeats + 4)][4:]
    buf.return_norm = rn
    f = lambda v: f"{np.mean(v):7.3f} ms ({np.min(v):.3f} - {np.max(v):.3f})"
    print(f"optimisation phase per update ({tr.config['epochs']} epochs x {tr.config['n_mini_batch']} minibatches, observation update "
          f"included): {f(opt)}", flush=True)
    print(f"observation update alone (host clock, synchronised): {f(upd)}", flush=True)
    print(f"calc_advantages (uploads + return scaling + GAE): {f(adv)}   without the return scaling: {f(adv_off)}", flush=True)
    print(f"both per update: {(np.mean(upd) + np.mean(adv) - np.mean(adv_off)) / np.mean(opt) * 100:.2f} % of the optimisation phase", flush=True)
    tr.close()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernel", "step", "update"]
    if "kernel" in what:
        kernel_times()
    if "step" in what:
        step_graph_cost()
    if "update" in what:
        update_cost()
