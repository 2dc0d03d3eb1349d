"""What the KL penalty (``kl_penalty``) costs on the device, what it does to a run, and that nothing changes without the key.

    python tools/kl_penalty_measure.py [step] [behaviour] [registers --parent DIR] [absent-outputs --parent DIR]
                                       [absent-bench --parent DIR [--branch-first]]

step:      the captured optimisation step (one graph replay = one minibatch step), replayed back to back, ``kl_penalty: 0.2`` (a fixed
           coefficient) against ``exact_kl: true`` alone, five alternated pairs in one process, at configs/synthetic_cartpole.yaml's and
           synthetic_minigrid.yaml's (BASELINE config 3) shapes; the scatter of the runs without the penalty next to each difference.
behaviour: configs/poc_memory_env.yaml (50 updates) and configs/synthetic_continuous.yaml (40 updates), each with ``exact_kl: true``
           alone and with ``kl_penalty: {coef: 0.2, target: 0.01}``: per update the coefficient, ``other/kl``, the KL of the update's
           last step and the mean reward of the episodes that ended in it; the mean ``other/kl`` and last-step KL of the last 20
           updates.  No assertion.
registers / absent-outputs / absent-bench: as tools/analytic_kl_measure.py, this tree against a checkout of the parent commit in DIR
           (cross-compiled resource numbers and instruction text of every pre-existing heads-loss / ppo-loss / reduce kernel and the
           numbers of the new ones; ``bench.py --dump-outputs`` byte for byte and a trace's kernel names and call counts; the bench
           value of three runs each).
The errors of the new kernels against float64 are measured by tests/test_kl_penalty_gpu.py itself (run it with ``-s``).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
STEP_SHAPES = ("synthetic_cartpole", "synthetic_minigrid")
BEHAVIOUR = (("poc_memory_env", 50), ("synthetic_continuous", 40))
ADAPTIVE = {"kl_penalty": {"coef": 0.2, "target": 0.01}}


def step_cost(pairs=5):
    import target_kl_measure as tk
    for name in STEP_SHAPES:
        off, _, snap_off = tk._prepared(tk._config(name, exact_kl=True), "klp_off")
        on, _, snap_on = tk._prepared(tk._config(name, kl_penalty=0.2), "klp_on")
        assert on._kl_coef is not None and off._kl_coef is None and on._kl_exact_cat and off._kl_exact_cat
        n = off.config["epochs"] * off.config["n_mini_batch"]

        def run(tr, snap):
            snap.restore()
            return tk._replay_us(tr, n)
        rows = []
        for pair in range(pairs):
            a, b = run(off, snap_off), run(on, snap_on)
            rows.append((a, b))
            print(f"{name}, captured optimisation step, {n} replays back to back, pair {pair}: exact_kl alone {a:9.2f} us   kl_penalty 0.2 "
                  f"{b:9.2f} us   difference {b - a:+7.2f} us", flush=True)
        a, b = np.array(rows).T
        print(f"{name}: exact_kl alone {a.min():.2f} - {a.max():.2f} us, kl_penalty {b.min():.2f} - {b.max():.2f} us; difference "
              f"{np.mean(b - a):+.2f} us (pairs {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}), {np.mean(b - a) / np.mean(a) * 100:+.3f} %; "
              f"scatter of the runs without the penalty {a.max() - a.min():.2f} us, pair to pair {np.abs(np.diff(a)).max():.2f} us", flush=True)
        off.close(), on.close()


def behaviour(tail=20):
    import torch
    import target_kl_measure as tk
    from utils import process_episode_info
    for name, updates in BEHAVIOUR:
        for key in ({"exact_kl": True}, ADAPTIVE):
            tr = tk._trainer(tk._config(name, **key), "klp_behaviour")
            label = f"{name} {'kl_penalty' if 'kl_penalty' in key else 'exact_kl alone'}"
            kls, lasts, rewards, coefs = [], [], [], []
            for update in range(updates):
                lr, beta, clip = tr.schedules(update)
                infos = tr._sample_training_data()
                tr.buffer.prepare_batch_dict()
                rows, _ = tr._train_epochs(lr, clip, beta)
                tr.update_index = update + 1
                torch.cuda.synchronize()
                kl = np.stack(rows)[:, 4]
                pen = tr.last_kl_penalty or {}
                reward = process_episode_info(infos).get("reward_mean", float("nan"))
                kls.append(float(kl.mean())), lasts.append(float(kl[-1])), rewards.append(float(reward)), coefs.append(pen.get("coef", 0.0))
                print(f"{label} update {update:3d}: coef {coefs[-1]:.5e} -> {pen.get('next_coef', 0.0):.5e} ({pen.get('moved', 0):+d})  other/kl "
                      f"{kl.mean():.5e}  kl of the last step {kl[-1]:.5e}  mean reward {reward:.4f}", flush=True)
            print(f"{label}: {updates} updates; last {tail}: mean other/kl {np.mean(kls[-tail:]):.5e}, mean kl of the last step "
                  f"{np.mean(lasts[-tail:]):.5e} (min {np.min(lasts[-tail:]):.3e}, max {np.max(lasts[-tail:]):.3e}), mean reward "
                  f"{np.nanmean(rewards[-tail:]):.4f}, coefficient {np.min(coefs[-tail:]):.4e} .. {np.max(coefs[-tail:]):.4e}", flush=True)
            tr.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["step", "behaviour"])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (for `registers`; built, for `absent-*`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "kl_penalty"), help="where `absent-outputs` writes dumps and traces")
    ap.add_argument("--branch-first", action="store_true", help="`absent-bench` in the mirrored order (branch, parent, parent, branch, ...)")
    args = ap.parse_args()
    if {"registers", "absent-outputs", "absent-bench"} & set(args.what) and not args.parent:
        raise SystemExit("registers / absent-outputs / absent-bench need --parent DIR")
    if "registers" in args.what:
        import analytic_kl_measure as akm
        akm.SOURCES = ("heads_loss", "ppo_loss")
        akm.KERNEL_WORDS = ("heads_loss", "heads_reduce", "ppo_loss", "ppo_finalize")
        akm.registers(args.parent)
    if "step" in args.what:
        step_cost()
    if "behaviour" in args.what:
        behaviour()
    if "absent-outputs" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_outputs(args.parent, args.out)
    if "absent-bench" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_bench(args.parent, args.branch_first)
