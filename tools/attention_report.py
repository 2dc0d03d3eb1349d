"""Where a policy's attention lands in its memory window while it trains (``attention_statistics: true``).  Needs the MI355X.

    python tools/attention_report.py --config configs/cue_room_device.yaml --updates 200 [--every 10]

Trains the config with the key on and prints, for the first and the last ``--every`` updates (each averaged over its updates' tables,
which are summed first: a mean over rows, not over updates): per block and head the normalised entropy (1 = uniform over the valid
entries), the mean age (1 = the newest stored step) and the mean largest probability; the age histogram in coarse bins; the share of
the attention mass on window entries 0 and 1 beside the share a uniform attention over the same rows would put there.  The uniform
share is computed from the run's own masks: a row with v valid entries gives entries 0 and 1 the share min(v, 2) / v, and the table
does not keep v -- so the tool counts it from the buffer's masks, once per update.  No assertion."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")
sys.path[:0] = [REPO, PKG]
os.environ.setdefault("ETM_QUIET", "1")

import numpy as np      # noqa: E402
import torch            # noqa: E402


def age_bins(L):
    """Coarse age bins [lo, hi] (inclusive, ages from 1): 1, 2, 3-4, 5-8, ... up to L."""
    bins, lo = [(1, 1)], 2
    while lo <= L:
        hi = min(L, max(lo, 2 * (lo - 1)))
        bins.append((lo, hi))
        lo = hi + 1
    return bins


def report(label, table, L, uniform01, episodes):
    from utils import attention_statistics_summary, process_episode_info
    s = attention_statistics_summary(table, L)
    res = process_episode_info(episodes) if episodes else {}
    head = f"== {label}: {int(s['rows'][0, 0])} counted rows per head, {int(s['empty'][0, 0])} empty, {int(s['irregular'][0, 0])} irregular"
    if res:
        head += f"; episodes: reward {res['reward_mean']:.3f}, length {res['length_mean']:.1f}"
        if "success_percent" in res:
            head += f", success {res['success_percent']:.2f}"
    print(head, flush=True)
    bins = age_bins(L)
    print("   block head  norm.entropy  mean age  max prob   mass on entries 0-1 (uniform %.4f)   age histogram %s"
          % (uniform01, " ".join(f"{lo}" if lo == hi else f"{lo}-{hi}" for lo, hi in bins)))
    for b, h in np.ndindex(s["rows"].shape):
        hist = " ".join(f"{s['age_hist'][b, h, lo - 1: hi].sum():.3f}" for lo, hi in bins)
        print(f"   {b:5d} {h:4d}  {s['normalised_entropy'][b, h]:12.4f}  {s['mean_age'][b, h]:8.3f}  {s['max_prob'][b, h]:8.4f}   "
              f"{s['index_hist'][b, h, :2].sum():.4f}                                   {hist}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, help="a config file (a path, or a name under the package's configs/)")
    ap.add_argument("--updates", type=int, required=True)
    ap.add_argument("--every", type=int, default=10, help="how many updates the first and the last report cover")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from trainer import PPOTrainer
    from yaml_parser import YamlParser
    path = args.config if os.path.exists(args.config) else os.path.join(PKG, args.config)
    cfg = YamlParser(path).get_config()
    cfg["attention_statistics"] = True
    cfg["updates"] = args.updates
    cfg["tunable_gemm"] = False
    cfg.pop("evaluation", None)
    cfg.pop("checkpoint_interval", None)
    torch.manual_seed(args.seed)
    tr = PPOTrainer(cfg, run_id="attention_report", device=torch.device("cuda", 0), tensorboard=False)
    L, every = tr.memory_length, max(1, min(args.every, args.updates))
    spans = {"first": range(0, every), "last": range(args.updates - every, args.updates)}
    sums = {k: [None, 0.0, 0.0, []] for k in spans}       # table, uniform mass on entries 0-1, counted samples, episodes
    try:
        for update in range(args.updates):
            lr, beta, clip = tr.schedules(update)
            infos = tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            tr._train_epochs(lr, clip, beta)
            table = tr._attn_stats.read()
            v = tr.buffer.memory_mask.reshape(-1, L).sum(dim=1).cpu().numpy().astype(np.float64)
            for k, span in spans.items():
                if update in span:
                    acc = sums[k]
                    acc[0] = table if acc[0] is None else acc[0] + table
                    acc[1] += float((np.minimum(v[v > 0], 2) / v[v > 0]).sum())
                    acc[2] += float((v > 0).sum())
                    acc[3].extend(infos)
    finally:
        tr.close()
    print(f"{os.path.basename(path)}: {args.updates} updates, memory_length {L}, blocks x heads {sums['first'][0].shape[:2]}, seed {args.seed}")
    for k, span in spans.items():
        table, u, n, eps = sums[k]
        report(f"updates {span.start} .. {span.stop - 1}", table, L, u / max(n, 1.0), eps)


if __name__ == "__main__":
    main()
