"""What invalid-action masks (``action_masks: true``) cost, and that nothing changes without the key.

    python tools/action_masks_measure.py [step] [opt] [host] [absent --parent DIR]

step:   the captured rollout step graph of every worker group, replayed ``worker_steps`` times back to back on the group's stream, of
        three trainers of the same seed -- key absent; ``action_masks: true`` with ``environment.action_mask_p: 0.3`` and the words
        read in place from pinned host memory (the trainer's transport); the same with the words' device twin, handed over as the
        (step, slot) block's twin is (``_mask_in_place = False``: a copy node in the step graph where the plan does not stream; in
        the pipelined plan, which reads that block in place, the kernels read device memory and the upload the twin would need per
        step is NOT in the number -- its lower bound) -- five alternated rounds, at configs/synthetic_cartpole.yaml (the group
        kernel) and at configs/synthetic_minigrid.yaml (BASELINE config 3, the per-worker kernel).
opt:    the captured optimisation step (one graph replay = one minibatch step) with the key on against the key absent, five
        alternated pairs at the same two shapes (tools/target_kl_measure.py's replay loop).
host:   the host's cost per rollout step and 32 workers of ``action_masks()`` + the empty-branch check + the copy into the buffer's
        pinned array, for the synthetic front-end in two groups (what the rollout loop adds under the device's step).
absent: the key absent, this tree against a built checkout of the parent commit in DIR (tools/target_kl_measure.py's ``absent``):
        ``bench.py --dump-outputs`` byte for byte, kernel names and call counts of a trace, the bench value of three runs each.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import target_kl_measure as tk      # noqa: E402  (the shared pieces: configs, trainers, the optimisation step's replay loop, `absent`)

SHAPES = ("synthetic_cartpole", "synthetic_minigrid")


def _masked(name, p=0.3):
    cfg = tk._config(name, action_masks=True)
    cfg["environment"] = dict(cfg["environment"], action_mask_p=p)
    return cfg


def _rollout_trainer(cfg, run_id, twin=False):
    """A trainer after one rollout (its step graphs are captured).  ``twin``: the words go through their device twin."""
    import torch
    tr = tk._trainer(cfg, run_id)
    if twin:
        tr._mask_in_place = False
        with torch.no_grad():
            streamed = bool(cfg.get("stream_observations", True)) and tr._use_kv_cache and tr.model._fused_encoder_ok(tr._obs_dev)
        if streamed and all(g.stream is not None for g in tr._groups):      # the pipelined plan would still read in place: point the kernels at device memory
            for g in tr._groups:
                g.am_dev.copy_(g.am_pin)
                g.am_pin = g.am_dev       # (measurement only -- the host's words no longer reach the device)
    tr._sample_training_data()
    torch.cuda.synchronize()
    assert all(g.graphs is not None for g in tr._groups)
    return tr


def _step_graph_us(tr):
    """Every group's captured step, ``worker_steps`` replays back to back on its stream -> us per replay, mean over the groups."""
    import torch
    S, out = tr.config["worker_steps"], []
    for g in tr._groups:
        stream = g.stream if g.stream is not None else torch.cuda.current_stream(tr.device)
        g.restart()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(S):
                g.graphs[0].replay()
            e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / S * 1e3)
    return float(np.mean(out))


def step_cost(rounds=5):
    for name in SHAPES:
        trs = {"absent": _rollout_trainer(tk._config(name), "am_off"), "in place": _rollout_trainer(_masked(name), "am_on"),
               "device twin": _rollout_trainer(_masked(name), "am_twin", twin=True)}
        g0, plan = trs["in place"]._groups[0], trs["in place"]._plan
        print(f"{name}: {len(trs['in place']._groups)} groups of {g0.W}, group kernel {g0.group_kernel}, plan own_stream {plan.own_stream} "
              f"host_flag {plan.host_flag} direct_rows {plan.direct_rows}; valid share {trs['in place'].last_valid_action_share:.3f}", flush=True)
        rows = []
        for r in range(rounds):
            row = [_step_graph_us(trs[k]) for k in trs]
            rows.append(row)
            print(f"{name} round {r}: " + "   ".join(f"{k} {v:8.2f} us" for k, v in zip(trs, row)), flush=True)
        a, b, c = np.array(rows).T
        print(f"{name}: step graph, key absent {a.min():.2f} - {a.max():.2f} us (scatter {a.max() - a.min():.2f}); words in place "
              f"{np.mean(b - a):+.2f} us (rounds {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}); words through the device twin "
              f"{np.mean(c - a):+.2f} us (rounds {np.min(c - a):+.2f} .. {np.max(c - a):+.2f})", flush=True)
        for tr in trs.values():
            tr.close()


def opt_cost(pairs=5):
    for name in SHAPES:
        off, _, snap_off = tk._prepared(tk._config(name), "am_opt_off")
        on, _, snap_on = tk._prepared(_masked(name), "am_opt_on")
        assert "action_masks" in on.buffer.samples_flat and "action_masks" not in off.buffer.samples_flat
        n = off.config["epochs"] * off.config["n_mini_batch"]
        rows = []
        for pair in range(pairs):
            snap_off.restore(), snap_on.restore()
            rows.append((tk._replay_us(off, n), tk._replay_us(on, n)))
            print(f"{name} pair {pair}: key absent {rows[-1][0]:9.2f} us   masked {rows[-1][1]:9.2f} us   difference {rows[-1][1] - rows[-1][0]:+7.2f} us",
                  flush=True)
        a, b = np.array(rows).T
        print(f"{name}: captured optimisation step, {n} replays back to back: key absent {a.min():.2f} - {a.max():.2f} us, masked {b.min():.2f} - "
              f"{b.max():.2f} us; difference {np.mean(b - a):+.2f} us (pairs {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}), "
              f"{np.mean(b - a) / np.mean(a) * 100:+.3f} %; scatter of the key-absent runs {a.max() - a.min():.2f} us", flush=True)
        off.close(), on.close()


def host_cost(steps=2000):
    from environments import branch_bit_masks, empty_mask_branches
    from environments.vec_env import make_vec_env
    for name in ("synthetic_multidiscrete", "synthetic_cartpole"):
        cfg = _masked(name)
        env_cfg = dict(cfg["environment"], pool=4, gen_threads=1, copy_threads=1, obs_shape=[4])      # (the observations are not what is timed)
        W = 32
        env = make_vec_env(env_cfg, W, groups=2)
        branches = tuple(env.action_space_shape)
        bits = branch_bit_masks(branches)
        words, keep = np.zeros(W, dtype=np.int64), np.zeros((W, steps), dtype=np.int64)
        env.reset()
        acts = np.zeros((W, len(branches)), dtype=np.int64)
        spent = 0.0
        for t in range(steps):
            for part, (lo, hi) in zip(env.parts, env.bounds):
                part.step(acts[lo:hi])
                t0 = time.perf_counter()
                part.action_masks(out=words[lo:hi])
                if empty_mask_branches(words[lo:hi], branches, bits).any():
                    raise SystemExit("an empty branch")
                keep[lo:hi, t] = words[lo:hi]
                spent += time.perf_counter() - t0
        print(f"{name} branches {branches}: action_masks() + empty-branch check + buffer copy, {W} workers in 2 groups: "
              f"{spent / steps * 1e6:.2f} us per rollout step ({spent / steps / 2 * 1e6:.2f} us per group and step)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["step", "opt", "host"])
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (for `absent`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "action_masks"), help="where `absent` writes dumps and traces")
    args = ap.parse_args()
    if "host" in args.what:
        host_cost()
    if "step" in args.what:
        step_cost()
    if "opt" in args.what:
        opt_cost()
    if "absent" in args.what:
        if not args.parent:
            raise SystemExit("absent needs --parent DIR")
        tk.key_absent(args.parent, args.out)
