"""What the exact Gaussian KL (``kl_estimator: analytic``) costs on the device, what it does to a run, and that nothing changes
without the key.

    python tools/analytic_kl_measure.py [errors] [step] [rollout] [behaviour] [registers --parent DIR]
                                        [absent-outputs --parent DIR] [absent-bench --parent DIR]

errors:    the heads + loss kernel's KL and a plain float32 torch evaluation of rsl_rl's expression, each against
           ``utils.gaussian_kl`` in float64 on the same operands (the kernel's own means), over N x hid x A; and the host definition in
           float32, the form the kernel computes.
step:      the captured optimisation step (one graph replay = one minibatch step), replayed back to back, key on against key absent,
           five alternated pairs in one process, at configs/synthetic_continuous.yaml's and synthetic_continuous_normalized.yaml's shapes.
rollout:   the captured rollout step graph (head and tail of one worker group, replayed back to back on a parked environment) at the
           same two shapes, key on against key absent, five alternated pairs.
behaviour: configs/synthetic_continuous_adaptive_lr.yaml with and without the key for the same number of updates: raises and cuts per
           update, the KL of each update's first step, the mean ``other/kl`` of the last updates.  No assertion.
registers: VGPR / SGPR / scratch / LDS of every rollout, heads + loss and reduce kernel of csrc/rollout_glue.hip, rollout_fused.hip,
           rollout_group.hip and heads_loss.hip, this tree against a checkout of the parent commit in DIR, both cross-compiled for
           gfx950 (needs no device), and whether the instruction text of each pre-existing kernel is the same.
absent-outputs / absent-bench: the key absent, this tree against a built checkout of the parent commit in DIR: the steps of
           tools/adaptive_lr_measure.py (``bench.py --dump-outputs`` byte for byte, kernel names and call counts of a trace; the bench
           value of three runs each, alternated).
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
SHAPES = ("synthetic_continuous", "synthetic_continuous_normalized")
KEY = {"kl_estimator": "analytic"}
SOURCES = ("rollout_glue", "rollout_fused", "rollout_group", "heads_loss")
KERNEL_WORDS = ("rollout_", "heads_loss", "heads_reduce")
NEW_WORDS = ("_means_kernel", "gaussian_kl_kernel", "heads_reduce_kl_kernel")


# ------------------------------------------------------------------ errors
def errors():
    import ctypes  # noqa: F401
    import torch
    from etm import lib as etm_lib
    from etm import ops
    from utils import gaussian_kl
    lib, dev = etm_lib.load(), torch.device("cuda", 0)
    worst = {"kernel": 0.0, "torch": 0.0, "host32": 0.0}
    for N in (1, 8, 9, 37, 2059):
        for hid in (64, 384, 512):
            for A in (1, 3, 8):
                g = torch.Generator().manual_seed(13 * N + 5 * hid + A)
                r = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev)
                pre_p, pre_v, b_lp, b_lv = r(N, hid), r(N, hid), r(hid, s=0.1), r(hid, s=0.1)
                wb, bb, wv, bv = r(A, hid, s=hid ** -0.5), r(A, s=0.1), r(hid, s=hid ** -0.5), r(1, s=0.1)
                log_std = torch.tensor([(-0.5, 0.0, 0.7)[a % 3] for a in range(A)], device=dev)
                adv, old_value = r(N), r(N)
                stats3 = ops.adv_stats(adv)
                row = lib.etm_heads_loss_gaussian_kl_row_floats(hid, A)
                nbytes = lib.etm_heads_loss_gaussian_kl_workspace_bytes(N, hid, A)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                gm_p, gm_v, sums, out8 = torch.empty((N, hid), device=dev), torch.empty((N, hid), device=dev), torch.empty(row, device=dev), torch.empty(8, device=dev)
                mu, value = torch.empty((N, A), device=dev), torch.empty(N, device=dev)
                xact, old_logp = r(N, A), r(N, s=0.1)
                old_mean, old_log_std = torch.zeros((N, A), device=dev), (log_std + r(A, s=0.15)).contiguous()
                p = lambda t: t.data_ptr()

                def call():
                    etm_lib.check(lib.etm_heads_loss_gaussian_kl(
                        p(pre_p), p(pre_v), p(b_lp), p(b_lv), p(wb), p(bb), p(wv), p(bv), p(xact), A, p(log_std), p(old_logp), 1, p(adv),
                        p(old_value), p(stats3), 0.2, 0.5, 0.01, 1.0 / N, 1.0 / N, 1.0 / N, None, p(gm_p), p(gm_v), p(sums), p(out8), p(mu),
                        p(value), p(ws), nbytes, N, hid, A, p(old_mean), A, p(old_log_std), torch.cuda.current_stream().cuda_stream),
                        "etm_heads_loss_gaussian_kl")
                    torch.cuda.synchronize()

                call()                                     # (the means do not depend on old_mean)
                old_mean.copy_(mu + 0.4 * log_std.exp() * r(N, A))
                call()
                host = [t.cpu().numpy() for t in (old_mean, old_log_std, mu, log_std)]
                ref = float(gaussian_kl(*host, np.float64))
                s, so = log_std.exp(), old_log_std.exp()
                rsl = float(torch.sum(torch.log(s / so) + (so.square() + (old_mean - mu).square()) / (2.0 * s.square()) - 0.5, dim=-1).mean().item())
                e = {"kernel": abs(float(out8[4]) - ref), "torch": abs(rsl - ref), "host32": abs(float(gaussian_kl(*host, np.float32)) - ref)}
                ulp = float(np.spacing(np.float32(ref)))
                print(f"N {N:5d} hid {hid:3d} A {A}: kl64 {ref:.9e}  kernel {e['kernel']:.3e} ({e['kernel'] / ulp:.2f} ulp)  float32 torch rsl_rl "
                      f"{e['torch']:.3e} ({e['torch'] / ulp:.2f} ulp)  gaussian_kl in float32 {e['host32']:.3e}", flush=True)
                for k in worst:
                    worst[k] = max(worst[k], e[k])
    print(f"largest |error| against float64 over 45 cases: kernel {worst['kernel']:.3e}, float32 torch evaluation of rsl_rl's expression "
          f"{worst['torch']:.3e}, utils.gaussian_kl in float32 {worst['host32']:.3e}", flush=True)


# ------------------------------------------------------------------ step / rollout
def _pairs(label, unit, measure_off, measure_on, pairs=5):
    rows = []
    for pair in range(pairs):
        a, b = measure_off(), measure_on()
        rows.append((a, b))
        print(f"{label} pair {pair}: key absent {a:9.2f} {unit}   analytic {b:9.2f} {unit}   difference {b - a:+7.2f} {unit}", flush=True)
    a, b = np.array(rows).T
    print(f"{label}: key absent {a.min():.2f} - {a.max():.2f} {unit}, analytic {b.min():.2f} - {b.max():.2f} {unit}; difference "
          f"{np.mean(b - a):+.2f} {unit} (pairs {np.min(b - a):+.2f} .. {np.max(b - a):+.2f}), {np.mean(b - a) / np.mean(a) * 100:+.3f} %; "
          f"scatter of the key-absent runs {a.max() - a.min():.2f} {unit}, pair to pair {np.abs(np.diff(a)).max():.2f} {unit}", flush=True)


def step_cost():
    import target_kl_measure as tk
    for name in SHAPES:
        off, _, snap_off = tk._prepared(tk._config(name), "akm_off")
        on, _, snap_on = tk._prepared(tk._config(name, **KEY), "akm_on")
        assert on._kl_analytic and not off._kl_analytic
        n = off.config["epochs"] * off.config["n_mini_batch"]

        def run(tr, snap):
            snap.restore()
            return tk._replay_us(tr, n)
        _pairs(f"{name}, captured optimisation step, {n} replays back to back", "us", lambda: run(off, snap_off), lambda: run(on, snap_on))
        off.close(), on.close()


def _step_graph_us(tr):
    """The first group's captured step graph replayed back to back (tools/normalization_cost.py's method: the step counter advances
    and must stay inside the staging arrays; no environment is stepped)."""
    import torch
    g0, S = tr._groups[0], tr.config["worker_steps"]
    n = max(1, min(200, S - 8))
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


def rollout_cost():
    import target_kl_measure as tk
    for name in SHAPES:
        off, on = tk._trainer(tk._config(name), "akm_roll_off"), tk._trainer(tk._config(name, **KEY), "akm_roll_on")
        for tr in (off, on):
            for _ in range(2):
                tr._sample_training_data()
        g = on._groups[0]
        assert off._step_graph is not None and on._step_graph is not None and g.graphs is not None
        form = "group kernel" if g.group_kernel else "per-worker kernel" if g.rf_scratch is not None else "multi-launch"
        _pairs(f"{name}, captured rollout step graph ({len(on._groups)} groups of {g.W} workers, {form}), replayed back to back", "us",
               lambda: _step_graph_us(off), lambda: _step_graph_us(on))
        off.close(), on.close()


# ------------------------------------------------------------------ behaviour
def behaviour(updates=40, tail=15):
    import torch
    import target_kl_measure as tk
    for key in ({}, KEY):
        cfg = tk._config("synthetic_continuous_adaptive_lr", **key)
        tr = tk._trainer(cfg, "akm_behaviour")
        label = "analytic" if key else "k3"
        kls, firsts, raises, cuts = [], [], [], []
        for update in range(updates):
            lr, beta, clip = tr.schedules(update)
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            rows, _ = tr._train_epochs(lr, clip, beta)
            tr.update_index = update + 1
            torch.cuda.synchronize()
            kl = np.stack(rows)[:, 4]
            last = tr.last_adaptive_lr
            kls.append(float(kl.mean())), firsts.append(float(kl[0])), raises.append(last["raised"]), cuts.append(last["lowered"])
            print(f"{label} update {update:3d}: lr {last['lr']:.6e}  raised {last['raised']:2d}  lowered {last['lowered']:2d}  kl of step 0 "
                  f"{kl[0]:+.3e}  other/kl {kl.mean():.5e}", flush=True)
        f = np.asarray(firsts)
        print(f"{label}: {updates} updates of {cfg['epochs'] * cfg['n_mini_batch']} steps, desired_kl {cfg['adaptive_lr']['desired_kl']} (band "
              f"{last['kl_low']:.4g} .. {last['kl_high']:.4g}): raises per update {np.mean(raises):.2f}, cuts per update {np.mean(cuts):.2f}; kl of "
              f"step 0: {int((f > 0).sum())} positive, {int((f < 0).sum())} negative, {int((f == 0).sum())} zero, |.| median {np.median(np.abs(f)):.3e} "
              f"max {np.abs(f).max():.3e}; mean other/kl of the last {tail} updates {np.mean(kls[-tail:]):.5e}, of the first 10 "
              f"{np.mean(kls[:10]):.5e}; the rate ends at {last['lr']:.6e}", flush=True)
        tr.close()


# ------------------------------------------------------------------ registers
def _kernel_table(tree, work):
    """{kernel symbol: {vgpr, sgpr, scratch, lds, text}} of the rollout / heads-loss / reduce kernels of ``tree``, cross-compiled for
    gfx950 with the Makefile's flags."""
    src = os.path.join(tree, "episodic-transformer-memory-ppo_amd", "csrc")
    os.makedirs(work, exist_ok=True)
    out = {}
    for name in SOURCES:
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on",
                        "-I" + src, "--save-temps", "-c", os.path.join(src, name + ".hip"), "-o", name + ".o"], cwd=work, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = open(os.path.join(work, name + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
            symbol = m.group(1)
            if not any(w in symbol for w in KERNEL_WORDS):
                continue
            field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, m.group(2)).group(1))
            body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata" % re.escape(symbol), asm, re.S | re.M).group(1)
            text = [re.sub(r"\.LBB\d+_\d+|\.Lpost_getpc\d+", "L", re.sub(r";.*", "", line)).strip() for line in body.splitlines()]
            out[symbol] = dict(vgpr=field("next_free_vgpr"), sgpr=field("next_free_sgpr"), scratch=field("private_segment_fixed_size"),
                               lds=field("group_segment_fixed_size"), text=[t for t in text if t and not t.startswith(".")])
    return out


def _demangled(symbols):
    r = subprocess.run(["c++filt"], input="\n".join(symbols), stdout=subprocess.PIPE, text=True)
    names = r.stdout.splitlines() if r.returncode == 0 else list(symbols)
    return dict(zip(symbols, (re.sub(r"\(.*", "", re.sub(r"^void ", "", n.replace("(anonymous namespace)::", ""))) for n in names)))


def registers(parent):
    with tempfile.TemporaryDirectory() as work:
        old, new = _kernel_table(os.path.abspath(parent), os.path.join(work, "parent")), _kernel_table(REPO, os.path.join(work, "branch"))
    names = _demangled(sorted(set(old) | set(new)))
    f = lambda k: f"VGPR {k['vgpr']:3d}  SGPR {k['sgpr']:3d}  scratch {k['scratch']:4d} B  LDS {k['lds']:6d} B  {len(k['text']):5d} instr."
    numbers = lambda k: (k["vgpr"], k["sgpr"], k["scratch"], k["lds"])
    missing = sorted(set(old) - set(new))
    same_numbers = same_text = 0
    for s in sorted(old):
        if s in missing:
            continue
        eq_n, eq_t = numbers(old[s]) == numbers(new[s]), old[s]["text"] == new[s]["text"]
        same_numbers, same_text = same_numbers + eq_n, same_text + eq_t
        print(f"{names[s]:62s} {f(new[s])}   numbers {'EQUAL' if eq_n else 'DIFFER from ' + f(old[s])}, text {'IDENTICAL' if eq_t else 'DIFFERS'}",
              flush=True)
    print(f"pre-existing kernels: {len(old)} in the parent, {len(missing)} missing in this tree {missing}; VGPR / SGPR / scratch / LDS equal for "
          f"{same_numbers}, instruction text identical for {same_text}", flush=True)
    for s in sorted(set(new) - set(old)):
        print(f"{names[s]:62s} {f(new[s])}   new", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["errors", "step", "rollout", "behaviour"])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (for `registers`; built, for `absent-*`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "analytic_kl"), help="where `absent-outputs` writes dumps and traces")
    ap.add_argument("--branch-first", action="store_true", help="`absent-bench` in the mirrored order (branch, parent, parent, branch, ...)")
    ap.add_argument("--updates", type=int, default=40, help="updates of each `behaviour` run")
    args = ap.parse_args()
    if {"registers", "absent-outputs", "absent-bench"} & set(args.what) and not args.parent:
        raise SystemExit("registers / absent-outputs / absent-bench need --parent DIR")
    if "registers" in args.what:
        registers(args.parent)
    if "errors" in args.what:
        errors()
    if "step" in args.what:
        step_cost()
    if "rollout" in args.what:
        rollout_cost()
    if "behaviour" in args.what:
        behaviour(args.updates)
    if "absent-outputs" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_outputs(args.parent, args.out)
    if "absent-bench" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_bench(args.parent, args.branch_first)
