"""Evaluate a checkpoint in batches on the fused rollout: many environments, whole episodes, greedy or sampled.

    python evaluate.py --model ./models/run.nn [--episodes-per-worker 4] [--workers 32] [--sample] [--seed N]

Loads the ``pickle((state_dict, config))`` of ``PPOTrainer._save_model``, builds the evaluator's rollout context (no training
context, no optimiser step ever runs), plays ``--episodes-per-worker`` episodes in each of ``--workers`` held-out environments
through the same step kernels and captured step graphs as training -- with the mode of the policy at every step, or sampled with
``--sample`` -- and prints ONE JSON line {"result", "steps", "seconds"}.  Arguments left out take the checkpoint config's
``evaluation`` section (see evaluation.py for the quota rule).
"""
import argparse
import json
import pickle

import torch


def main():
    ap = argparse.ArgumentParser(description="Evaluate a trained model on the MI355X")
    ap.add_argument("--model", default="./models/run.nn", help="Path to the trained model")
    ap.add_argument("--episodes-per-worker", type=int, default=None, help="Episodes every environment contributes (its first ones)")
    ap.add_argument("--workers", type=int, default=None, help="Number of evaluation environments")
    ap.add_argument("--sample", action="store_true", help="Sample the actions instead of taking the mode of the policy")
    ap.add_argument("--seed", type=int, default=None, help="First worker id of the evaluation environments and seed of sampled draws")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible: the MI355X path cannot run (there is no CPU fallback)")
    from evaluation import Evaluator, evaluation_defaults
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    with open(args.model, "rb") as f:
        state_dict, config = pickle.load(f)
    ev = evaluation_defaults(config)
    evaluator = Evaluator(config, device, run_id="evaluate")
    evaluator.load_state_dict(state_dict)
    try:
        out = evaluator.run(episodes_per_worker=ev["episodes_per_worker"] if args.episodes_per_worker is None else args.episodes_per_worker,
                            n_workers=ev["n_workers"] if args.workers is None else args.workers,
                            deterministic=False if args.sample else ev["deterministic"],
                            seed=ev["seed"] if args.seed is None else args.seed, worker_steps=ev["worker_steps"])
    finally:
        evaluator.close()
    print(json.dumps({"result": {k: float(v) for k, v in out["result"].items()}, "steps": int(out["steps"]),
                      "seconds": float(out["seconds"])}), flush=True)


if __name__ == "__main__":
    main()
