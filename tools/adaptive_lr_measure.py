"""What the KL-adaptive learning rate (``adaptive_lr``) costs on the device, what it does to a run, and that nothing changes without
the key.

    python tools/adaptive_lr_measure.py [step] [behaviour] [registers --parent DIR] [absent-outputs] [absent-bench --parent DIR]

step:      the captured optimisation step (one graph replay = one minibatch step), replayed back to back, of a trainer with a band
           nothing leaves (``low: 0``, kl_high 3e38: every step runs the adaptive norm launch and keeps its rate) against a key-absent
           trainer of the same seed -- five alternated pairs in one process, at configs/synthetic_minigrid.yaml (BASELINE config 3) and
           at configs/synthetic_cartpole.yaml, both with ``learning_rate_schedule.final = initial``.  No launch is added, so the
           difference is reported next to the pairs' scatter.
behaviour: configs/poc_memory_env.yaml with ``adaptive_lr: 0.01`` for 50 updates: the rate, the counters and ``other/kl`` (the mean of
           the update's kl rows) per update, and the mean kl of the last 20 updates next to desired_kl; then the key absent at a fixed
           3e-4 and a fixed 1e-5, four updates each: how far the kl runs within one update at a fixed rate.  No assertion.
registers: VGPR / SGPR / scratch / LDS of the four existing optimiser kernels, csrc/optim.hip of this tree against the one of a checkout
           of the parent commit in DIR, both cross-compiled for gfx950 (needs no device), and whether their instruction text is the same.
absent-outputs / absent-bench: the key absent, this tree against a built checkout of the parent commit in DIR (the steps of
           tools/target_kl_measure.py: key_absent, in two parts so that each fits a time limit): ``bench.py --dump-outputs`` byte for
           byte and kernel names and call counts of a kernel trace; the bench value of three runs each, alternated.  Every run is a
           fresh child process under a time limit; the first one that fails ends the tool.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
SHAPES = ("synthetic_minigrid", "synthetic_cartpole")
NEVER = {"adaptive_lr": {"desired_kl": 1.5e38, "low": 0, "high": 2.0}}
OLD_KERNELS = ("grad_sqnorm_kernel", "grad_sqnorm_gated_kernel", "adamw_clip_kernel", "adamw_clip_gated_kernel")
NEW_KERNELS = ("grad_sqnorm_adaptive_kernel", "grad_sqnorm_adaptive_gated_kernel")


def _flat_schedule(cfg):
    s = dict(cfg["learning_rate_schedule"])
    s["final"] = s["initial"]
    return s


def step_cost(pairs=5):
    import target_kl_measure as tk
    for name in SHAPES:
        base = tk._config(name)
        base["learning_rate_schedule"] = _flat_schedule(base)
        off, _, snap_off = tk._prepared(dict(base), "alm_off")
        on, _, snap_on = tk._prepared(dict(base, **NEVER), "alm_on")
        n = off.config["epochs"] * off.config["n_mini_batch"]           # one update's steps: the counter stays inside the tables
        rows = []
        for pair in range(pairs):
            snap_off.restore(), snap_on.restore()
            on._adapt.reset()
            a, b = tk._replay_us(off, n), tk._replay_us(on, n)
            assert on._adapt.read() == (0, 0) and float(on.optimizer.lr_dev.item()) == float(np.float32(base['learning_rate_schedule']['initial']))
            rows.append((a, b))
            print(f"{name} pair {pair}: key absent {a:9.2f} us   adaptive, band never left {b:9.2f} us   difference {b - a:+7.2f} us", flush=True)
        a, b = np.array(rows).T
        print(f"{name}: captured step, {n} replays back to back: key absent {a.min():.2f} - {a.max():.2f} us, adaptive {b.min():.2f} - "
              f"{b.max():.2f} us; difference {np.mean(b - a):+.2f} us (pairs {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}), "
              f"{np.mean(b - a) / np.mean(a) * 100:+.3f} %; scatter of the key-absent runs {a.max() - a.min():.2f} us, pair to pair "
              f"{np.abs(np.diff(a)).max():.2f} us", flush=True)
        off.close(), on.close()


def behaviour(updates=50, desired_kl=0.01):
    import torch
    import target_kl_measure as tk
    cfg = tk._config("poc_memory_env", adaptive_lr=desired_kl)
    cfg["learning_rate_schedule"] = _flat_schedule(cfg)
    cfg["environment"] = dict(cfg["environment"], seed=0)
    tr = tk._trainer(cfg, "alm_behaviour")
    kls = []
    for update in range(updates):
        lr, beta, clip = tr.schedules(update)
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        rows, _ = tr._train_epochs(lr, clip, beta)
        tr.update_index = update + 1
        torch.cuda.synchronize()
        kl = float(np.mean(np.stack(rows)[:, 4]))
        kls.append(kl)
        last = tr.last_adaptive_lr
        print(f"update {update:3d}: lr {last['lr']:.6e}  raised {last['raised']:2d}  lowered {last['lowered']:2d}  other/kl {kl:.5e}", flush=True)
    print(f"poc_memory_env, adaptive_lr {desired_kl} (band {last['kl_low']:.4g} .. {last['kl_high']:.4g}), {updates} updates of "
          f"{cfg['epochs'] * cfg['n_mini_batch']} steps: mean other/kl of the last 20 updates {np.mean(kls[-20:]):.5e} (desired_kl {desired_kl}); "
          f"of the first 10 {np.mean(kls[:10]):.5e}; the rate ends at {last['lr']:.6e}", flush=True)
    tr.close()


def fixed_rate_probe(updates=4):
    """poc_memory_env, key absent: the kl of the steps of the first updates at a fixed 3e-4 and a fixed 1e-5."""
    import target_kl_measure as tk
    for lr in (3e-4, 1e-5):
        cfg = tk._config("poc_memory_env")
        cfg["environment"] = dict(cfg["environment"], seed=0)
        cfg["learning_rate_schedule"] = dict(cfg["learning_rate_schedule"], initial=lr, final=lr)
        tr = tk._trainer(cfg, "alm_fixed")
        for update in range(updates):
            rate, beta, clip = tr.schedules(update)
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            rows, _ = tr._train_epochs(rate, clip, beta)
            tr.update_index = update + 1
            kl = np.stack(rows)[:, 4]
            print(f"lr {lr:g} update {update}: kl of step 0 {kl[0]:.3e}, steps 1-7 " + " ".join(f"{x:.2e}" for x in kl[1:8])
                  + f" ... last {kl[-1]:.3e}, mean {kl.mean():.3e}", flush=True)
        tr.close()


def _kernel_table(tree, work):
    """{kernel: {vgpr, sgpr, scratch, lds, text}} of csrc/optim.hip of ``tree``, cross-compiled for gfx950 with the Makefile's flags."""
    src = os.path.join(tree, "episodic-transformer-memory-ppo_amd", "csrc")
    os.makedirs(work, exist_ok=True)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on",
                    "-I" + src, "--save-temps", "-c", os.path.join(src, "optim.hip"), "-o", "optim.o"], cwd=work, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(os.path.join(work, "optim-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, m.group(2)).group(1))
        name = next((k for k in OLD_KERNELS + NEW_KERNELS if re.search(r"\d%s[A-Z]" % k, m.group(1))), None)
        if name is None:
            continue
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata" % re.escape(m.group(1)), asm, re.S | re.M).group(1)
        text = [re.sub(r"\.LBB\d+_\d+", "L", re.sub(r";.*", "", line)).strip() for line in body.splitlines()]
        out[name] = dict(vgpr=field("next_free_vgpr"), sgpr=field("next_free_sgpr"), scratch=field("private_segment_fixed_size"),
                         lds=field("group_segment_fixed_size"), text=[t for t in text if t and not t.startswith(".")])
    return out


def registers(parent):
    with tempfile.TemporaryDirectory() as work:
        old, new = _kernel_table(os.path.abspath(parent), os.path.join(work, "parent")), _kernel_table(REPO, os.path.join(work, "branch"))
    f = lambda k: f"VGPR {k['vgpr']:3d}  SGPR {k['sgpr']:3d}  scratch {k['scratch']} B  LDS {k['lds']} B  {len(k['text'])} instructions"
    for name in OLD_KERNELS:
        same = old[name]["text"] == new[name]["text"]
        print(f"{name:34s} parent: {f(old[name])}\n{'':34s} branch: {f(new[name])}   instruction text {'IDENTICAL' if same else 'DIFFERS'}", flush=True)
    for name in NEW_KERNELS:
        print(f"{name:34s} new:    {f(new[name])}", flush=True)


def absent_outputs(parent, out_dir):
    import csv
    import glob
    import hashlib
    import target_kl_measure as tk
    trees = (("parent", os.path.abspath(parent)), ("branch", REPO))
    out_dir = os.path.abspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    sums, calls = {}, {}
    for label, tree in trees:
        dump = os.path.join(out_dir, "dump_" + label)
        tk._child([sys.executable] + tk.BENCH + ["--steps", "3", "--warmup", "1", "--dump-outputs", dump], tree, 300)
        sums[label] = {os.path.basename(p): hashlib.sha256(open(p, "rb").read()).hexdigest() for p in sorted(glob.glob(os.path.join(dump, "*.npy")))}
    same = sums["parent"] == sums["branch"] and len(sums["parent"]) > 0
    differ = sorted(k for k in set(sums["parent"]) | set(sums["branch"]) if sums["parent"].get(k) != sums["branch"].get(k))
    print(f"bench.py --dump-outputs, sha256 of every file: {'DUMP IDENTICAL' if same else 'DUMP DIFFERS in ' + str(differ)} "
          f"({len(sums['parent'])} files)", flush=True)
    for label, tree in trees:
        trace = os.path.join(out_dir, "trace_" + label)
        tk._child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--", sys.executable] + tk.BENCH
                  + ["--no-profile", "--steps", "3", "--warmup", "1"], tree, 400)
        table = {}
        for path in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                table[row["Name"]] = table.get(row["Name"], 0) + int(row["Calls"])
        calls[label] = table
    same = calls["parent"] == calls["branch"] and len(calls["parent"]) > 0
    print(f"kernel trace: parent {len(calls['parent'])} kernel names, {sum(calls['parent'].values())} calls; branch {len(calls['branch'])} "
          f"kernel names, {sum(calls['branch'].values())} calls: {'IDENTICAL names and call counts' if same else 'DIFFERENT'}", flush=True)
    for k in sorted(set(calls["parent"]) | set(calls["branch"])):
        if calls["parent"].get(k) != calls["branch"].get(k):
            print(f"    {k}: parent {calls['parent'].get(k)} branch {calls['branch'].get(k)}")


def absent_bench(parent, branch_first=False):
    import target_kl_measure as tk
    trees = {"parent": os.path.abspath(parent), "branch": REPO}
    values = {"parent": [], "branch": []}
    order = ("parent", "branch", "branch", "parent", "parent", "branch")
    if branch_first:            # (the mirrored order: whether the place in the series matters)
        order = tuple({"parent": "branch", "branch": "parent"}[x] for x in order)
    for label in order:
        out = tk._child([sys.executable] + tk.BENCH + ["--steps", "20", "--warmup", "5"], trees[label], 300)
        values[label].append(tk._bench_value(out))
        print(f"bench {label}: {values[label][-1]:,.0f} env-steps/s", flush=True)
    p, b = values["parent"], values["branch"]
    inside = min(p) <= np.mean(b) <= max(p)
    print(f"parent {min(p):,.0f} - {max(p):,.0f} (mean {np.mean(p):,.0f}); branch {min(b):,.0f} - {max(b):,.0f} (mean {np.mean(b):,.0f}, "
          f"{(np.mean(b) / np.mean(p) - 1) * 100:+.2f} %); the branch's mean lies {'inside' if inside else 'OUTSIDE'} the parent's range", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["step", "behaviour"])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (for `registers`; built, for `absent-*`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "adaptive_lr"), help="where `absent-outputs` writes dumps and traces")
    ap.add_argument("--branch-first", action="store_true", help="`absent-bench` in the mirrored order (branch, parent, parent, branch, ...)")
    args = ap.parse_args()
    if {"registers", "absent-outputs", "absent-bench"} & set(args.what) and not args.parent:
        raise SystemExit("registers / absent-outputs / absent-bench need --parent DIR")
    if "registers" in args.what:
        registers(args.parent)
    if "step" in args.what:
        step_cost()
    if "behaviour" in args.what:
        behaviour()
        fixed_rate_probe()
    if "absent-outputs" in args.what:
        absent_outputs(args.parent, args.out)
    if "absent-bench" in args.what:
        absent_bench(args.parent, args.branch_first)
