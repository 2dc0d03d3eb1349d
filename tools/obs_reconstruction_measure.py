"""Measurements behind the README section on ``obs_reconstruction`` (profiles/r21/obs_reconstruction.txt).  Needs the MI355X.

  python tools/obs_reconstruction_measure.py fused [--n 2048] [--pairs 5] [--iters 10]
      the fused last layer + loss (ops.obs_reconstruction_loss: etm_obs_recon_fwd_loss, etm_obs_recon_dgrad, the reused
      etm_conv_train_wgrad) against the same layer written as library ops (conv_transpose2d + binary_cross_entropy_with_logits on
      channels_last activations and a float32 target that already exists), forward and backward, in alternated pairs: milliseconds per
      pass and torch.cuda.max_memory_allocated above the operands of both.
  python tools/obs_reconstruction_measure.py cost [--pairs 5] [--updates 2]
      configs/synthetic_minigrid_recon.yaml against configs/synthetic_minigrid_u8.yaml (the key absent), both trainers alive in one
      process, alternated pairs: seconds per optimisation phase (the captured step replayed epochs * n_mini_batch times).
  python tools/obs_reconstruction_measure.py behaviour [--updates 50]
      the reconstruction loss per update with the key, and the mean reward per step with the key and without (no assertion).
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")
sys.path[:0] = [REPO, PKG]
os.environ.setdefault("ETM_QUIET", "1")

import numpy as np      # noqa: E402
import torch            # noqa: E402
import torch.nn.functional as F      # noqa: E402


def _config(key, **over):
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(PKG, "configs", "synthetic_minigrid_recon.yaml" if key else "synthetic_minigrid_u8.yaml")).get_config()
    cfg["tunable_gemm"] = False
    cfg.update(over)
    return cfg


def _update(tr):
    """One update -> (seconds of the rollout, seconds of the optimisation phase, mean raw reward per step)."""
    dev = tr.device
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    tr._sample_training_data()
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    reward = float(tr.buffer.rewards.mean())
    tr.buffer.prepare_batch_dict()
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._train_epochs(lr, clip, beta)
    tr.update_index += 1
    torch.cuda.synchronize(dev)
    return t1 - t0, time.perf_counter() - t1, reward


def _timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def fused(args):
    from etm import ops
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = args.n
    a2 = torch.relu(torch.randn((n, 20, 20, 32), device=dev)).requires_grad_(True)
    dec = torch.nn.ConvTranspose2d(32, 3, 8, 4).to(dev)
    obs = torch.randint(0, 256, (n, 84, 84, 3), dtype=torch.uint8, device=dev)
    target = (obs.float() / 255).permute(0, 3, 1, 2)            # (the library twin's target: float32, NCHW view of NHWC memory)
    coef = torch.full((1,), 0.1, device=dev)
    params = [a2, dec.weight, dec.bias]

    def run_fused():
        for p in params:
            p.grad = None
        ops.obs_reconstruction_loss(a2, dec, obs, coef, unit_grad=True).backward()

    def run_library():
        for p in params:
            p.grad = None
        z = F.conv_transpose2d(a2.permute(0, 3, 1, 2), dec.weight, dec.bias, stride=4)
        (coef[0] * F.binary_cross_entropy_with_logits(z, target)).backward()

    peak = {}
    for name, fn in (("fused", run_fused), ("library", run_library)):
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    rows = {"fused": [], "library": []}
    for pair in range(args.pairs):
        for name, fn in ((("fused", run_fused), ("library", run_library)) if pair % 2 == 0 else (("library", run_library), ("fused", run_fused))):
            rows[name].append(_timed(fn, args.iters))
    for name in rows:
        r = np.array(rows[name])
        print(f"N {n} last layer + loss, forward and backward, {name}: ms per pass {np.round(r, 3).tolist()} (median {np.median(r):.3f}, "
              f"range {r.min():.3f} .. {r.max():.3f}); peak memory above the operands {peak[name]:.1f} MiB", flush=True)
    print(f"library / fused, medians: {np.median(rows['library']) / np.median(rows['fused']):.2f}", flush=True)


def cost(args):
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    trainers = {}
    for key in (False, True):
        torch.manual_seed(0)
        trainers[key] = PPOTrainer(_config(key), run_id="cost", device=dev, tensorboard=False)
        for _ in range(2):
            _update(trainers[key])         # eager warm-up steps, graph capture
    rows = {False: [], True: []}
    for pair in range(args.pairs):
        for key in ((False, True) if pair % 2 == 0 else (True, False)):
            rows[key].append(min(_update(trainers[key])[1] for _ in range(args.updates)))
    cfg = trainers[True].config
    steps = cfg["epochs"] * cfg["n_mini_batch"]
    off, on = np.array(rows[False]) * 1e3, np.array(rows[True]) * 1e3
    for key, r in ((False, off), (True, on)):
        print(f"config 3 (uint8) obs_reconstruction={'0.1' if key else 'absent'}: optimisation ms per update {np.round(r, 2).tolist()} "
              f"(median {np.median(r):.2f})", flush=True)
    print(f"key on - key absent, medians: {np.median(on) - np.median(off):+.2f} ms per update = {(np.median(on) - np.median(off)) * 1e3 / steps:+.1f} us "
          f"per minibatch step of {cfg['n_workers'] * cfg['worker_steps'] // cfg['n_mini_batch']} samples; key-absent scatter (max - min) "
          f"{off.max() - off.min():.2f} ms", flush=True)
    for tr in trainers.values():
        tr.close()


def behaviour(args):
    from trainer import PPOTrainer
    for key in (True, False):
        torch.manual_seed(0)
        tr = PPOTrainer(_config(key, n_workers=16, worker_steps=128), run_id="behaviour", device=torch.device("cuda", 0), tensorboard=False)
        rewards, losses = [], []
        for _ in range(args.updates):
            rewards.append(_update(tr)[2])
            if key:
                losses.append(tr.last_obs_reconstruction["loss"])
        if key:
            print(f"obs_reconstruction 0.1 (16 workers x 128 steps per update): loss per update {np.round(losses, 4).tolist()} (ln 2 = {np.log(2):.4f})",
                  flush=True)
        print(f"obs_reconstruction={'0.1' if key else 'absent'}: {args.updates} updates, mean reward per step: first 5 updates {np.mean(rewards[:5]):.4f}, "
              f"last 10 updates {np.mean(rewards[-10:]):.4f}", flush=True)
        tr.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    f = sub.add_parser("fused")
    f.add_argument("--n", type=int, default=2048)
    f.add_argument("--pairs", type=int, default=5)
    f.add_argument("--iters", type=int, default=10)
    c = sub.add_parser("cost")
    c.add_argument("--pairs", type=int, default=5)
    c.add_argument("--updates", type=int, default=2)
    b = sub.add_parser("behaviour")
    b.add_argument("--updates", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible")
    {"fused": fused, "cost": cost, "behaviour": behaviour}[args.mode](args)


if __name__ == "__main__":
    main()
