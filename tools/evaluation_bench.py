"""One measured evaluation next to the training rollout of the same run (reports, not thresholds).
python tools/evaluation_bench.py [config] [n_workers] [episodes_per_worker]      (defaults: synthetic_minigrid 32 2 = config 3's shape)
Prints the training rollout's env-steps/s (mean of three rollouts after a warm-up update), the first evaluation (it allocates the
evaluator's rollout context and captures its step graphs), a second and a third one (steady state: wall time, env-steps/s), the same
sampled, and the device memory the evaluator's context took from the allocator."""
import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "episodic-transformer-memory-ppo_amd"))
import torch
from yaml_parser import YamlParser
from trainer import PPOTrainer
name = sys.argv[1] if len(sys.argv) > 1 else "synthetic_minigrid"
n_workers = int(sys.argv[2]) if len(sys.argv) > 2 else 32
episodes = int(sys.argv[3]) if len(sys.argv) > 3 else 2
cfg = YamlParser(os.path.join(REPO, "episodic-transformer-memory-ppo_amd", "configs", name + ".yaml")).get_config()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
tr = PPOTrainer(cfg, run_id="evalbench", device=dev, tensorboard=False)
lr, beta, clip = tr.schedules(0)
tr._sample_training_data(); tr.buffer.prepare_batch_dict(); tr._train_epochs(lr, clip, beta); torch.cuda.synchronize()
steps = cfg["n_workers"] * cfg["worker_steps"]
rates = []
for _ in range(3):
    t0 = time.perf_counter(); tr._sample_training_data(); torch.cuda.synchronize()
    rates.append(steps / (time.perf_counter() - t0))
print(f"{name}: training rollout {cfg['n_workers']} workers x {cfg['worker_steps']} steps: " + ", ".join(f"{r:.0f}" for r in rates) + " env-steps/s")
before = torch.cuda.memory_allocated(dev)
for label, det in (("first (allocates, captures)", True), ("greedy", True), ("greedy", True), ("sampled", False), ("sampled", False)):
    out = tr.evaluate(episodes_per_worker=episodes, n_workers=n_workers, deterministic=det)
    r = out["result"]
    print(f"evaluate {label:<28} {len(out['episodes'])} episodes ({n_workers} workers x {episodes}), {out['steps']} env steps in "
          f"{out['seconds']:.3f} s = {out['steps'] / out['seconds']:.0f} env-steps/s; chunk {tr._evaluator._key[1]} steps; "
          f"reward {r.get('reward_mean', float('nan')):.3f} length {r.get('length_mean', float('nan')):.1f}")
print(f"evaluator's rollout context: {tr._evaluator.allocated_bytes / 2 ** 20:.1f} MiB of device memory at construction, "
      f"{(torch.cuda.memory_allocated(dev) - before) / 2 ** 20:.1f} MiB more allocated after the evaluations than before them "
      f"(training context: peak {torch.cuda.max_memory_allocated(dev) / 2 ** 20:.0f} MiB allocated)")
tr.close()
