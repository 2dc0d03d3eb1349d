"""What the exact categorical KL (``exact_kl: true``) costs on the device, what it does to a run, and that nothing changes without
the key.

    python tools/exact_kl_measure.py [errors] [step] [rollout] [behaviour] [registers --parent DIR]
                                     [absent-outputs --parent DIR] [absent-bench --parent DIR] [--logps-tail]

errors:    the fused heads + loss kernel's KL, a plain float32 torch evaluation of ``(p_old * (logp_old - logp_new)).sum(-1).mean() / B``
           and ``utils.categorical_kl`` in float32, each against ``utils.categorical_kl`` in float64 on the same operands (the kernel's
           own logits), over N x hid x layout, masked and not.
step:      the captured optimisation step (one graph replay = one minibatch step), replayed back to back, key on against key absent,
           five alternated pairs in one process, at configs/synthetic_cartpole.yaml's and synthetic_minigrid.yaml's (BASELINE config 3)
           shapes.
rollout:   the captured rollout step graph (head and tail of one worker group, replayed back to back on a parked environment) with the
           per-worker kernel (synthetic_minigrid.yaml) and the group kernel (synthetic_cartpole.yaml), key on against key absent, five
           alternated pairs.  ``--logps-tail`` loads the diagnostic build of ``make -C csrc diag-logps-tail`` (the log-prob columns
           stored one per thread behind the action's hand-over instead of by the sampling thread as it draws) for the other store
           placement.
behaviour: configs/synthetic_cartpole_target_kl_exact.yaml, and configs/poc_memory_env.yaml with ``adaptive_lr: 0.01``, with and
           without the key for the same number of updates: raises and cuts (or applied steps) per update, the KL of each update's first
           step, the mean ``other/kl`` of the last 20 updates.  No assertion.
registers / absent-outputs / absent-bench: as tools/analytic_kl_measure.py, this tree against a checkout of the parent commit in DIR
           (cross-compiled resource numbers and instruction text of every pre-existing rollout / heads-loss / ppo-loss / reduce kernel;
           ``bench.py --dump-outputs`` byte for byte and a trace's kernel names and call counts; the bench value of three runs each).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
KEY = {"exact_kl": True}
STEP_SHAPES = ("synthetic_cartpole", "synthetic_minigrid")
TAIL_BUILD = os.path.join(REPO, "tools", "scratch", "libetm_hip_logps_tail.so")


# ------------------------------------------------------------------ errors
def errors():
    import ctypes
    import torch
    from etm import lib as etm_lib
    from etm import ops
    from utils import categorical_kl
    lib, dev = etm_lib.load(), torch.device("cuda", 0)
    worst = {"kernel": 0.0, "torch": 0.0, "host32": 0.0}
    cases = 0
    for N in (1, 8, 9, 37, 2059):
        for hid in (64, 384, 512):
            for br in ((2,), (8,), (3, 3), (2, 1, 5)):
                for masked in (False, True):
                    A, B = sum(br), len(br)
                    offs = [sum(br[:b]) for b in range(B)]
                    g = torch.Generator().manual_seed(13 * N + 5 * hid + 7 * A + B)
                    r = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).to(dev)
                    pre_p, pre_v, b_lp, b_lv = r(N, hid), r(N, hid), r(hid, s=0.1), r(hid, s=0.1)
                    wb, bb, wv, bv = r(A, hid, s=2.0 * hid ** -0.5), r(A, s=0.3), r(hid, s=hid ** -0.5), r(1, s=0.1)
                    adv, old_value = r(N), r(N)
                    stats3 = ops.adv_stats(adv)
                    valid = torch.ones((N, A), dtype=torch.bool)
                    if masked:
                        valid = torch.rand((N, A), generator=g) < 0.6
                        for off, a in zip(offs, br):
                            valid[torch.arange(N), off + torch.randint(0, a, (N,), generator=g)] = True
                    words = torch.as_tensor(np.array([sum(1 << j for j in range(A) if row[j]) for row in valid.numpy()], dtype=np.int64), device=dev)
                    actions = torch.stack([(torch.rand((N, a), generator=g) + valid[:, off:off + a].float()).argmax(1) for off, a in zip(offs, br)],
                                          dim=1).to(dev).contiguous()
                    vd = valid.to(dev)

                    def lsm(x):
                        out = torch.full_like(x, float("-inf"))
                        for off, a in zip(offs, br):
                            out[:, off:off + a] = torch.log_softmax(x[:, off:off + a].masked_fill(~vd[:, off:off + a], float("-inf")), dim=-1)
                        return out
                    row, nbytes = lib.etm_heads_loss_kl_row_floats(hid, A), lib.etm_heads_loss_kl_workspace_bytes(N, hid, A)
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                    gm_p, gm_v, sums, out8 = torch.empty((N, hid), device=dev), torch.empty((N, hid), device=dev), torch.empty(row, device=dev), torch.empty(8, device=dev)
                    logits, value = torch.empty((N, A), device=dev), torch.empty(N, device=dev)
                    old_logp, old_logps = r(N, B, s=0.1), torch.zeros((N, A), device=dev)
                    p = lambda t: t.data_ptr()
                    tab = (ctypes.c_int32 * B)(*br)

                    def call():
                        head = (p(pre_p), p(pre_v), p(b_lp), p(b_lv), p(wb), p(bb), p(wv), p(bv), p(actions), B, p(old_logp), B, p(adv), p(old_value),
                                p(stats3), 0.2, 0.5, 0.01, 1.0 / (N * B), 1.0 / N, 1.0 / N, None, p(gm_p), p(gm_v), p(sums), p(out8), p(logits),
                                p(value), p(ws), nbytes, N, hid)
                        tail = (p(words) if masked else None, p(old_logps), A, torch.cuda.current_stream().cuda_stream)
                        rc = lib.etm_heads_loss_kl(*head, A, *tail) if B == 1 else lib.etm_heads_loss_branched_kl(*head, tab, B, *tail)
                        etm_lib.check(rc, "etm_heads_loss_kl")
                        torch.cuda.synchronize()

                    call()                                     # (the logits do not depend on the old rows)
                    old_logps.copy_(lsm(logits + 0.4 * r(N, A)))
                    call()
                    wh = words.cpu().numpy() if masked else None
                    ref = float(categorical_kl(old_logps.cpu().numpy(), logits.cpu().numpy(), br, wh, np.float64))
                    new, zero = lsm(logits), torch.zeros_like(logits)
                    term = torch.where(vd, old_logps.exp() * (torch.where(vd, old_logps, zero) - torch.where(vd, new, zero)), zero)
                    e = {"kernel": abs(float(out8[4]) - ref), "torch": abs(float((term.sum(-1).mean() / B).item()) - ref),
                         "host32": abs(float(categorical_kl(old_logps.cpu().numpy(), logits.cpu().numpy(), br, wh, np.float32)) - ref)}
                    ulp = float(np.spacing(np.float32(ref)))
                    print(f"N {N:5d} hid {hid:3d} branches {str(br):10s} {'masked' if masked else 'plain ':6s}: kl64 {ref:.9e}  kernel {e['kernel']:.3e} "
                          f"({e['kernel'] / ulp:.2f} ulp)  float32 torch {e['torch']:.3e} ({e['torch'] / ulp:.2f} ulp)  categorical_kl in float32 "
                          f"{e['host32']:.3e}", flush=True)
                    cases += 1
                    for k in worst:
                        worst[k] = max(worst[k], e[k])
    print(f"largest |error| against float64 over {cases} cases: kernel {worst['kernel']:.3e}, float32 torch evaluation of the plain definition "
          f"{worst['torch']:.3e}, utils.categorical_kl in float32 {worst['host32']:.3e}", flush=True)


# ------------------------------------------------------------------ step / rollout
def step_cost():
    import analytic_kl_measure as akm
    import target_kl_measure as tk
    for name in STEP_SHAPES:
        off, _, snap_off = tk._prepared(tk._config(name), "ekm_off")
        on, _, snap_on = tk._prepared(tk._config(name, **KEY), "ekm_on")
        assert on._kl_exact_cat and not off._kl_exact_cat
        n = off.config["epochs"] * off.config["n_mini_batch"]

        def run(tr, snap):
            snap.restore()
            return tk._replay_us(tr, n)
        akm._pairs(f"{name}, captured optimisation step, {n} replays back to back (second column: exact_kl)", "us",
                   lambda: run(off, snap_off), lambda: run(on, snap_on))
        off.close(), on.close()


def rollout_cost(placement):
    import analytic_kl_measure as akm
    import target_kl_measure as tk
    for name in ("synthetic_minigrid", "synthetic_cartpole"):
        off, on = tk._trainer(tk._config(name), "ekm_roll_off"), tk._trainer(tk._config(name, **KEY), "ekm_roll_on")
        for tr in (off, on):
            for _ in range(2):
                tr._sample_training_data()
        g = on._groups[0]
        assert off._step_graph is not None and on._step_graph is not None and g.graphs is not None and "logps" in on._stage
        form = "group kernel" if g.group_kernel else "per-worker kernel" if g.rf_scratch is not None else "multi-launch"
        akm._pairs(f"{name}, captured rollout step graph ({len(on._groups)} groups of {g.W} workers, {form}; log-prob columns stored "
                   f"{placement}), replayed back to back (second column: exact_kl)", "us",
                   lambda: akm._step_graph_us(off), lambda: akm._step_graph_us(on))
        off.close(), on.close()


# ------------------------------------------------------------------ behaviour
def behaviour(updates=50, tail=20):
    import torch
    import target_kl_measure as tk
    for name, extra in (("synthetic_cartpole_target_kl", {}), ("poc_memory_env", {"adaptive_lr": 0.01})):
        for key in ({}, KEY):
            cfg = tk._config(name, **extra, **key)
            tr = tk._trainer(cfg, "ekm_behaviour")
            label = f"{name} {'exact_kl' if key else 'k3'}"
            kls, firsts, raises, cuts, applied = [], [], [], [], []
            for update in range(updates):
                lr, beta, clip = tr.schedules(update)
                tr._sample_training_data()
                tr.buffer.prepare_batch_dict()
                rows, _ = tr._train_epochs(lr, clip, beta)
                tr.update_index = update + 1
                torch.cuda.synchronize()
                kl = np.stack(rows)[:, 4]
                last = getattr(tr, "last_adaptive_lr", None) or {}
                stop = getattr(tr, "last_kl_stop", None) or {}
                kls.append(float(kl.mean())), firsts.append(float(kl[0]))
                raises.append(last.get("raised", 0)), cuts.append(last.get("lowered", 0)), applied.append(stop.get("steps_applied", len(kl)))
                print(f"{label} update {update:3d}: raised {raises[-1]:2d}  lowered {cuts[-1]:2d}  steps applied {applied[-1]:2d}  kl of step 0 "
                      f"{kl[0]:+.3e}  other/kl {kl.mean():.5e}", flush=True)
            f = np.asarray(firsts)
            print(f"{label}: {updates} updates: raises per update {np.mean(raises):.2f}, cuts per update {np.mean(cuts):.2f}, steps applied per "
                  f"update {np.mean(applied):.2f}; kl of step 0: {int((f > 0).sum())} positive, {int((f < 0).sum())} negative, "
                  f"{int((f == 0).sum())} zero, |.| median {np.median(np.abs(f)):.3e} max {np.abs(f).max():.3e}; mean other/kl of the last {tail} "
                  f"updates {np.mean(kls[-tail:]):.5e}", flush=True)
            tr.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["errors", "step", "rollout", "behaviour"])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (for `registers`; built, for `absent-*`)")
    ap.add_argument("--out", default=os.path.join(REPO, "tools", "scratch", "exact_kl"), help="where `absent-outputs` writes dumps and traces")
    ap.add_argument("--branch-first", action="store_true", help="`absent-bench` in the mirrored order (branch, parent, parent, branch, ...)")
    ap.add_argument("--updates", type=int, default=50, help="updates of each `behaviour` run")
    ap.add_argument("--logps-tail", action="store_true", help="load the diagnostic build with the other store placement (`rollout`)")
    args = ap.parse_args()
    if {"registers", "absent-outputs", "absent-bench"} & set(args.what) and not args.parent:
        raise SystemExit("registers / absent-outputs / absent-bench need --parent DIR")
    if args.logps_tail:
        from etm import lib as etm_lib
        if not os.path.exists(TAIL_BUILD):
            raise SystemExit(f"{TAIL_BUILD} is missing: run `make -C episodic-transformer-memory-ppo_amd/csrc diag-logps-tail`")
        etm_lib.LIB_PATH = TAIL_BUILD
    if "registers" in args.what:
        import analytic_kl_measure as akm
        akm.SOURCES = ("rollout_glue", "rollout_fused", "rollout_group", "heads_loss", "ppo_loss")
        akm.KERNEL_WORDS = ("rollout_", "heads_loss", "heads_reduce", "ppo_loss", "ppo_finalize")
        akm.registers(args.parent)
    if "errors" in args.what:
        errors()
    if "step" in args.what:
        step_cost()
    if "rollout" in args.what:
        rollout_cost("behind the hand-over" if args.logps_tail else "by the sampling thread, in front of the hand-over")
    if "behaviour" in args.what:
        behaviour(args.updates)
    if "absent-outputs" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_outputs(args.parent, args.out)
    if "absent-bench" in args.what:
        import adaptive_lr_measure as alm
        alm.absent_bench(args.parent, args.branch_first)
