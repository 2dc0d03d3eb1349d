"""Measurements behind the README section on ``previous_step_input`` (profiles/r20/previous_step_input.txt).  Needs the MI355X.

  python tools/previous_step_measure.py behaviour [--updates 150]
      configs/hidden_arm.yaml with and without the key for the same number of updates: mean reward per step of the first and the
      last updates (no assertion; 0.5 is what a policy that is told nothing can reach with two arms).
  python tools/previous_step_measure.py cost [--config synthetic_cartpole] [--pairs 5] [--updates 3]
      key on against key absent at this commit, in alternated pairs, both trainers alive in one process: seconds per rollout
      (the captured step graph replayed worker_steps times, environments included) and per optimisation phase (the captured step
      replayed epochs * n_mini_batch times), after one warm-up update that captures the graphs.
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


def _config(name, key):
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(PKG, "configs", name + ".yaml")).get_config()
    cfg.pop("previous_step_input", None)
    if key:
        cfg["previous_step_input"] = True
    cfg["tunable_gemm"] = False
    return cfg


def _update(tr, lr=None):
    """One update -> (seconds of the rollout, seconds of the optimisation phase, mean raw reward per step)."""
    dev = tr.device
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    tr._sample_training_data()
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    reward = float(tr.buffer.rewards.mean())
    tr.buffer.prepare_batch_dict()
    sched = tr.config["learning_rate_schedule"]["initial"] if lr is None else lr
    tr._train_epochs(sched, tr.config["clip_range_schedule"]["initial"], tr.config["beta_schedule"]["initial"])
    torch.cuda.synchronize(dev)
    return t1 - t0, time.perf_counter() - t1, reward


def behaviour(args):
    from trainer import PPOTrainer
    for key in (True, False):
        torch.manual_seed(0)
        tr = PPOTrainer(_config("hidden_arm", key), run_id="hidden_arm", device=torch.device("cuda", 0), tensorboard=False)
        rewards = [_update(tr)[2] for _ in range(args.updates)]
        print(f"hidden_arm previous_step_input={key}: {args.updates} updates, mean reward per step: first 5 updates "
              f"{np.mean(rewards[:5]):.3f}, last 10 updates {np.mean(rewards[-10:]):.3f}", flush=True)
        tr.close()


def cost(args):
    from trainer import PPOTrainer
    dev = torch.device("cuda", 0)
    trainers = {}
    for key in (False, True):
        torch.manual_seed(0)
        trainers[key] = PPOTrainer(_config(args.config, key), run_id="cost", device=dev, tensorboard=False)
        for _ in range(2):
            _update(trainers[key])         # eager warm-up steps, graph capture
    rows = {False: [], True: []}
    for pair in range(args.pairs):
        for key in ((False, True) if pair % 2 == 0 else (True, False)):
            t = np.array([_update(trainers[key])[:2] for _ in range(args.updates)])
            rows[key].append(t.min(axis=0))
    for key in (False, True):
        r = np.array(rows[key]) * 1e3
        print(f"{args.config} previous_step_input={key}: rollout ms per update {np.round(r[:, 0], 2).tolist()} (median {np.median(r[:, 0]):.2f}), "
              f"optimisation ms per update {np.round(r[:, 1], 2).tolist()} (median {np.median(r[:, 1]):.2f})", flush=True)
    off, on = np.array(rows[False]) * 1e3, np.array(rows[True]) * 1e3
    cfg = trainers[True].config
    steps, mbs = cfg["worker_steps"], cfg["epochs"] * cfg["n_mini_batch"]
    print(f"{args.config}: key on - key absent, medians: rollout {np.median(on[:, 0]) - np.median(off[:, 0]):+.2f} ms per update = "
          f"{(np.median(on[:, 0]) - np.median(off[:, 0])) * 1e3 / steps:+.2f} us per step; optimisation "
          f"{np.median(on[:, 1]) - np.median(off[:, 1]):+.2f} ms per update = {(np.median(on[:, 1]) - np.median(off[:, 1])) * 1e3 / mbs:+.2f} us per "
          f"minibatch step; key-absent scatter (max - min): rollout {off[:, 0].max() - off[:, 0].min():.2f} ms, optimisation "
          f"{off[:, 1].max() - off[:, 1].min():.2f} ms", flush=True)
    for tr in trainers.values():
        tr.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    b = sub.add_parser("behaviour")
    b.add_argument("--updates", type=int, default=150)
    c = sub.add_parser("cost")
    c.add_argument("--config", default="synthetic_cartpole")
    c.add_argument("--pairs", type=int, default=5)
    c.add_argument("--updates", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible")
    {"behaviour": behaviour, "cost": cost}[args.mode](args)


if __name__ == "__main__":
    main()
