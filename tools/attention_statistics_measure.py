"""Measurements behind the README section on attention statistics (profiles/r28/attention_statistics.txt).  Needs the MI355X.
``ETM_DIAG_LIB=<path>`` measures another build of the library.

    python tools/attention_statistics_measure.py [kernel] [step] [absent-outputs --parent DIR] [absent-bench --parent DIR]

kernel:  etm_attn_stats alone, at the minibatch shapes of configs/synthetic_minigrid.yaml (BASELINE config 3: N 2048, H 4, L 64) and
         configs/path_room_device.yaml (N 1024, H 4, L 32) and at a whole config-3 batch (N 16384): device time per call between two
         events around 500 back-to-back calls on one stream, after a warm-up, three rounds, every round printed, beside the bytes a
         call reads (N H L 4 of att, N L of mask per head) and the time those bytes take at the HBM rate.
step:    the captured optimisation step (one graph replay = one minibatch step), replayed back to back, of a trainer with
         ``attention_statistics: true`` against a key-absent trainer of the same seed -- five alternated pairs in one process, at
         configs/synthetic_minigrid.yaml and configs/path_room_device.yaml: the key's share of the step.
absent-outputs / absent-bench: the key absent, this tree against a built checkout of the parent commit in DIR (the steps of
         tools/adaptive_lr_measure.py): ``bench.py --dump-outputs`` byte for byte and kernel names and call counts of a kernel
         trace; the bench value of three runs each, alternated."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
os.environ.setdefault("ETM_QUIET", "1")
SHAPES = ("synthetic_minigrid", "path_room_device")
KERNEL_SHAPES = ((2048, 4, 64, "config 3 minibatch"), (1024, 4, 32, "path_room_device minibatch"), (16384, 4, 64, "config 3 whole batch"))
HBM_BYTES_PER_S = 8.0e12


def kernel(calls=500, rounds=3):
    import torch
    from etm import lib as etm_lib
    if os.environ.get("ETM_DIAG_LIB"):
        etm_lib.LIB_PATH = os.environ["ETM_DIAG_LIB"]
    from etm import ops
    dev = torch.device("cuda", 0)
    for N, H, L, what in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(0)
        v = torch.randint(0, L + 1, (N,), generator=g)
        mask = (torch.arange(L)[None, :] < v[:, None])
        logits = torch.randn((N, H, L), generator=g).masked_fill(~mask[:, None, :], -1e20)
        att = torch.softmax(logits, dim=2).to(dev).contiguous()
        mask = mask.to(torch.uint8).to(dev)
        st = ops.AttentionStatistics(1, H, N, L, dev)
        nbytes = N * H * L * 4 + H * N * L
        print(f"{what}: N {N} H {H} L {L}: a call reads {nbytes / 1e6:.2f} MB ({nbytes / HBM_BYTES_PER_S * 1e6:.2f} us at 8 TB/s; the attention "
              f"kernel has just written them: cache-resident in the step), workspace {st.workspace.numel() / 1e3:.1f} kB", flush=True)
        for _ in range(20):
            ops.attn_stats(att, mask, st.table[0], st.workspace)
        torch.cuda.synchronize()
        for r in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                ops.attn_stats(att, mask, st.table[0], st.workspace)
            e1.record()
            torch.cuda.synchronize()
            print(f"    round {r}: {e0.elapsed_time(e1) / calls * 1e3:8.2f} us per call (two launches), {calls} calls back to back", flush=True)


def step_cost(pairs=5):
    import target_kl_measure as tk
    for name in SHAPES:
        off, _, snap_off = tk._prepared(tk._config(name), "asm_off")
        on, _, snap_on = tk._prepared(tk._config(name, attention_statistics=True), "asm_on")
        n = off.config["epochs"] * off.config["n_mini_batch"]           # one update's steps: the counter stays inside the tables
        blocks = on.num_blocks
        rows = []
        for pair in range(pairs):
            snap_off.restore(), snap_on.restore()
            on._attn_stats.reset()
            a, b = tk._replay_us(off, n), tk._replay_us(on, n)
            counted = on._attn_stats.read()[:, :, (0, 2, 3)].sum(axis=2)       # counted + empty + irregular rows: every row of every replay
            assert (counted == n * on.buffer.batch_size // on.config["n_mini_batch"]).all(), counted
            rows.append((a, b))
            print(f"{name} pair {pair}: key absent {a:9.2f} us   attention_statistics {b:9.2f} us   difference {b - a:+7.2f} us", flush=True)
        a, b = np.array(rows).T
        print(f"{name}: captured step, {n} replays back to back, {blocks} blocks = {blocks} calls (2 launches each) per step: key absent "
              f"{a.min():.2f} - {a.max():.2f} us, with the key {b.min():.2f} - {b.max():.2f} us; difference {np.mean(b - a):+.2f} us (pairs "
              f"{np.min(b - a):+.2f} .. {np.max(b - a):+.2f}), {np.mean(b - a) / np.mean(b) * 100:+.3f} % of the step with the key; scatter of "
              f"the key-absent runs {a.max() - a.min():.2f} us", flush=True)
        off.close(), on.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "step"])
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (for `absent-*`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "attention_statistics"), help="where `absent-outputs` writes dumps and traces")
    args = ap.parse_args()
    if {"absent-outputs", "absent-bench"} & set(args.what) and not args.parent:
        raise SystemExit("absent-outputs / absent-bench need --parent DIR")
    if "kernel" in args.what:
        kernel()
    if "step" in args.what:
        step_cost()
    if "absent-outputs" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_outputs(args.parent, args.out)
    if "absent-bench" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_bench(args.parent)
