"""What the KL early stop (``target_kl``) costs and saves on the device, and that nothing changes without the key.

    python tools/target_kl_measure.py [step] [host] [absent --parent DIR]

step:   the captured optimisation step (one graph replay = one minibatch step), replayed back to back, of a trainer with
        ``target_kl: {value: 3e38, factor: 1.0, host_check: none}`` (every step applies, through the gated launches) against a key-absent
        trainer of the same seed -- five alternated pairs in one process, at configs/synthetic_minigrid.yaml (BASELINE config 3) and at
        configs/synthetic_cartpole.yaml.  The gate adds no launch, so the difference is reported next to the pairs' scatter.
host:   ``host_check: epoch`` against ``none`` (epochs: 5, the config's minibatches): the optimisation phase per update at the 3e38 limit
        (what four event waits cost), then with a limit taken from a key-absent probe so that the stop falls in epoch 2 of 5 (what
        not launching epochs 3 - 5 saves).  Every timed update starts from the same restored weights, moments and step count and runs
        the same permutations, so that the stop falls on the same step every time; host clock around work that ends in a device
        synchronise.
absent: the key absent, this tree against a built checkout of the parent commit in DIR: ``bench.py --dump-outputs`` byte for byte, kernel
        names and call counts of a rocprofv3 kernel trace, and the bench value of three runs each, alternated.  Every run is a fresh
        child process under a time limit; the first one that fails ends the tool.
"""
import argparse
import glob
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
SHAPES = ("synthetic_minigrid", "synthetic_cartpole")


def _config(name, **over):
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(REPO, "episodic-transformer-memory-ppo_amd", "configs", name + ".yaml")).get_config()
    cfg.update(over)
    return cfg


def _trainer(cfg, run_id):
    import torch
    from trainer import PPOTrainer
    torch.manual_seed(0)
    return PPOTrainer(cfg, run_id=run_id, device=torch.device("cuda", 0), tensorboard=False)


def _kl(limit, host_check):
    return {"target_kl": {"value": float(limit), "factor": 1.0, "host_check": host_check}}


def _perms(tr, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(tr.buffer.batch_size) for _ in range(tr.config["epochs"])]


class _Snapshot:
    """Weights, moments and step count of a trainer, to start every timed update from the same point."""

    def __init__(self, tr):
        o = tr.optimizer
        self.tensors = (o.flat_params, o.exp_avg, o.exp_avg_sq, o.step_dev)
        self.saved = [t.clone() for t in self.tensors]

    def restore(self):
        for t, s in zip(self.tensors, self.saved):
            t.copy_(s)


def _prepared(cfg, run_id, perm_seed=4):
    """A trainer after one rollout, a snapshot of its state right there (the same for every trainer of one shape: same seed), and two
    whole updates on that rollout (the step is captured)."""
    import torch
    tr = _trainer(cfg, run_id)
    tr._sample_training_data()
    tr.buffer.prepare_batch_dict()
    perms, snap = _perms(tr, perm_seed), _Snapshot(tr)
    for _ in range(2):
        tr._train_epochs(3e-4, 0.2, 1e-3, perms=perms)
    torch.cuda.synchronize()
    assert tr._train_graph is not None and tr._train_graph[1] is None, "the single-device captured step is what is measured"
    return tr, perms, snap


def _replay_us(tr, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        tr._bank_pos, tr._obs_train = tr._bank_with_positions(), tr._training_observations()
    tr._tg_counter.zero_()
    if tr._kl_gate is not None:
        tr._kl_gate.reset()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        tr._train_graph[0].replay()
    e1.record()
    torch.cuda.synchronize()
    tr._bank_pos = tr._row_stats = None
    return e0.elapsed_time(e1) / n * 1e3


def step_cost(pairs=5):
    for name in SHAPES:
        off, _, snap_off = _prepared(_config(name), "klm_off")
        on, _, snap_on = _prepared(_config(name, **_kl(3e38, "none")), "klm_on")
        n = off.config["epochs"] * off.config["n_mini_batch"]           # one update's steps: the counter stays inside the tables
        rows = []
        for pair in range(pairs):
            snap_off.restore(), snap_on.restore()
            a, b = _replay_us(off, n), _replay_us(on, n)
            applied = on._kl_gate.read()
            assert applied[:2] == (False, n), applied
            rows.append((a, b))
            print(f"{name} pair {pair}: key absent {a:9.2f} us   gated, limit 3e38 {b:9.2f} us   difference {b - a:+7.2f} us", flush=True)
        a, b = np.array(rows).T
        print(f"{name}: captured step, {n} replays back to back: key absent {a.min():.2f} - {a.max():.2f} us, gated {b.min():.2f} - "
              f"{b.max():.2f} us; difference {np.mean(b - a):+.2f} us (pairs {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}), "
              f"{np.mean(b - a) / np.mean(a) * 100:+.3f} %; scatter of the key-absent runs {a.max() - a.min():.2f} us", flush=True)
        off.close(), on.close()


def _phase_ms(tr, perms, snap, repeats):
    import torch
    out = []
    for _ in range(repeats):
        snap.restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr._train_epochs(3e-4, 0.2, 1e-3, perms=perms)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def host_check_cost(repeats=5):
    f = lambda v: f"{np.mean(v):8.3f} ms ({np.min(v):.3f} - {np.max(v):.3f})"
    for name in SHAPES:
        probe, perms, snap = _prepared(_config(name, epochs=5), "klm_probe")
        n_mb = probe.config["n_mini_batch"]
        snap.restore()
        rows, _ = probe._train_epochs(3e-4, 0.2, 1e-3, perms=perms)
        kl = np.stack(rows)[:, 4]
        absent = _phase_ms(probe, perms, snap, repeats)
        probe.close()
        print(f"{name}: epochs 5 x {n_mb} minibatches; optimisation phase per update, key absent: {f(absent)}", flush=True)
        print(f"{name}: kl of the probe's {len(kl)} steps: " + " ".join(f"{x:.3e}" for x in kl), flush=True)
        # the 3e38 limit: what the four event waits cost (alternated)
        tr_e, p_e, s_e = _prepared(_config(name, epochs=5, **_kl(3e38, "epoch")), "klm_epoch")
        tr_n, p_n, s_n = _prepared(_config(name, epochs=5, **_kl(3e38, "none")), "klm_none")
        e, n = [], []
        for _ in range(repeats):
            e += _phase_ms(tr_e, p_e, s_e, 1)
            n += _phase_ms(tr_n, p_n, s_n, 1)
        assert not tr_e.last_kl_stop["stopped"] and tr_e.last_kl_stop["steps_launched"] == 5 * n_mb
        print(f"{name}: limit 3e38 (no stop): host_check epoch {f(e)}   none {f(n)}   four waits cost {np.mean(e) - np.mean(n):+.3f} ms "
              f"({(np.mean(e) - np.mean(n)) / np.mean(n) * 100:+.2f} %)", flush=True)
        tr_e.close(), tr_n.close()
        # a stop in epoch 2 of 5: a step of the second epoch whose kl exceeds every earlier one -- on other permutations where these
        # have none (a probe of the same seed: same rollout, same start)
        perm_seed, records = 4, [r for r in range(n_mb, 2 * n_mb) if kl[r] > kl[:r].max()]
        if not records:
            probe, _, snap = _prepared(_config(name, epochs=5), "klm_probe2")
            for perm_seed in range(5, 17):
                snap.restore()
                kl = np.stack(probe._train_epochs(3e-4, 0.2, 1e-3, perms=_perms(probe, perm_seed))[0])[:, 4]
                records = [r for r in range(n_mb, 2 * n_mb) if kl[r] > kl[:r].max()]
                if records:
                    print(f"{name}: permutations of seed {perm_seed}: kl " + " ".join(f"{x:.3e}" for x in kl), flush=True)
                    break
            probe.close()
        if not records:
            print(f"{name}: no step of epoch 2 has a kl above all earlier steps on 13 sets of permutations: the saving is not measured", flush=True)
            continue
        r = records[len(records) // 2]
        limit = float(np.float32((float(kl[:r].max()) + float(kl[r])) / 2))
        if not float(kl[:r].max()) < limit < float(kl[r]):
            print(f"{name}: no float32 between the kl of steps {r - 1} and {r}: the saving is not measured", flush=True)
            continue
        tr_e, p_e, s_e = _prepared(_config(name, epochs=5, **_kl(limit, "epoch")), "klm_epoch_stop", perm_seed)
        tr_n, p_n, s_n = _prepared(_config(name, epochs=5, **_kl(limit, "none")), "klm_none_stop", perm_seed)
        e, n = [], []
        for _ in range(repeats):
            e += _phase_ms(tr_e, p_e, s_e, 1)
            n += _phase_ms(tr_n, p_n, s_n, 1)
        se, sn = tr_e.last_kl_stop, tr_n.last_kl_stop
        assert se["stopped"] and sn["stopped"] and se["steps_applied"] == sn["steps_applied"] == r, (se, sn, r)
        print(f"{name}: limit {limit:.6e}: stop at step {r} (epoch 2 of 5); launched {se['steps_launched']} (epoch) / {sn['steps_launched']} "
              f"(none) of {5 * n_mb}: host_check epoch {f(e)}   none {f(n)}   the check saves {np.mean(n) - np.mean(e):+.3f} ms "
              f"({(np.mean(n) - np.mean(e)) / np.mean(n) * 100:+.1f} % of the phase)", flush=True)
        tr_e.close(), tr_n.close()


# ------------------------------------------------------------------ key absent, against a checkout of the parent commit
BENCH = ["bench.py", "--gpus", "1", "--no-rooflines", "--no-cpu-baseline", "--no-worker-processes-run"]


def _child(cmd, cwd, limit):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if r.returncode != 0:
        print(r.stdout[-3000:])
        raise SystemExit(f"{' '.join(cmd)} in {cwd} ended with {r.returncode}: nothing more is started")
    return r.stdout


def _bench_value(out):
    for line in reversed(out.splitlines()):
        if line.startswith("{"):
            return float(json.loads(line)["value"])
    raise SystemExit("no JSON line in the bench output")


def key_absent(parent, out_dir):
    trees = (("parent", os.path.abspath(parent)), ("branch", REPO))
    out_dir = os.path.abspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    sums = {}
    for label, tree in trees:
        dump = os.path.join(out_dir, "dump_" + label)
        _child([sys.executable] + BENCH + ["--steps", "3", "--warmup", "1", "--dump-outputs", dump], tree, 400)
        sums[label] = {os.path.basename(p): hashlib.sha256(open(p, "rb").read()).hexdigest() for p in sorted(glob.glob(os.path.join(dump, "*.npy")))}
    same = sums["parent"] == sums["branch"] and len(sums["parent"]) > 0
    differ = sorted(k for k in set(sums["parent"]) | set(sums["branch"]) if sums["parent"].get(k) != sums["branch"].get(k))
    print(f"bench.py --dump-outputs, sha256 of every file: {'DUMP IDENTICAL' if same else 'DUMP DIFFERS in ' + str(differ)} "
          f"({len(sums['parent'])} files)", flush=True)
    calls = {}
    for label, tree in trees:
        trace = os.path.join(out_dir, "trace_" + label)
        _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--", sys.executable] + BENCH
               + ["--no-profile", "--steps", "3", "--warmup", "1"], tree, 600)
        import csv
        table = {}
        for path in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                table[row["Name"]] = table.get(row["Name"], 0) + int(row["Calls"])
        calls[label] = table
    print(f"rocprofv3 --kernel-trace --stats: parent {len(calls['parent'])} kernel names, {sum(calls['parent'].values())} calls; branch "
          f"{len(calls['branch'])} kernel names, {sum(calls['branch'].values())} calls: "
          f"{'IDENTICAL names and call counts' if calls['parent'] == calls['branch'] and calls['parent'] else 'DIFFERENT'}", flush=True)
    if calls["parent"] != calls["branch"]:
        for k in sorted(set(calls["parent"]) | set(calls["branch"])):
            if calls["parent"].get(k) != calls["branch"].get(k):
                print(f"    {k}: parent {calls['parent'].get(k)} branch {calls['branch'].get(k)}")
    values = {"parent": [], "branch": []}
    for label in ("parent", "branch", "branch", "parent", "parent", "branch"):
        out = _child([sys.executable] + BENCH + ["--steps", "20", "--warmup", "5"], dict(trees)[label], 400)
        values[label].append(_bench_value(out))
        print(f"bench {label}: {values[label][-1]:,.0f} env-steps/s", flush=True)
    p, b = values["parent"], values["branch"]
    inside = min(p) <= np.mean(b) <= max(p)
    print(f"parent {min(p):,.0f} - {max(p):,.0f} (mean {np.mean(p):,.0f}); branch {min(b):,.0f} - {max(b):,.0f} (mean {np.mean(b):,.0f}, "
          f"{(np.mean(b) / np.mean(p) - 1) * 100:+.2f} %); the branch's mean lies {'inside' if inside else 'OUTSIDE'} the parent's range", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["step", "host"])
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (for `absent`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "target_kl"), help="where `absent` writes dumps and traces")
    args = ap.parse_args()
    if "step" in args.what:
        step_cost()
    if "host" in args.what:
        host_check_cost()
    if "absent" in args.what:
        if not args.parent:
            raise SystemExit("absent needs --parent DIR")
        key_absent(args.parent, args.out)
