"""Measurements behind the README section on device-resident environments (profiles/r22/device_env.txt).  Needs the MI355X.

  python tools/device_env_measure.py kernel [--steps 500]
      etm_cue_room_step at 84 x 84 (grid 7, cell 12) and W in {16, 64, 1024}: device time per step between two events around
      ``steps`` back-to-back launches on one stream (frames to device memory, result words to pinned host memory), after a warm-up.
  python tools/device_env_measure.py rollout [--pairs 5] [--rollouts 3]
      the rollout phase of configs/cue_room_device.yaml against configs/cue_room.yaml -- the host twin stepped serially and through
      worker processes (``vectorize: pipe``) -- and against the ``Synthetic`` uint8 config of equal shape, the floor a host environment
      that costs nothing reaches.  All trainers alive in one process, one warm-up rollout each (it captures the step graphs), then
      ``pairs`` alternated rounds of ``rollouts`` rollouts: seconds per rollout and environment steps per second, range and median,
      with the trainer's own split (env.step, waiting for the actions, upload + launch).
  python tools/device_env_measure.py behaviour [--updates 200]
      configs/cue_room_device.yaml for ``updates`` updates with and without ``obs_reconstruction``: success rate of the episodes that
      ended in the first and the last tenth of the run (no assertion; always walking to one corner earns 25 %).
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")
sys.path[:0] = [REPO, PKG]
os.environ.setdefault("ETM_QUIET", "1")

import numpy as np      # noqa: E402
import torch            # noqa: E402


def _config(name, **env_over):
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(PKG, "configs", name + ".yaml")).get_config()
    cfg["environment"].update(env_over)
    cfg["tunable_gemm"] = False
    return cfg


def _trainer(cfg, run_id):
    from trainer import PPOTrainer
    torch.manual_seed(0)
    return PPOTrainer(cfg, run_id=run_id, device=torch.device("cuda", 0), tensorboard=False)


def kernel(args):
    from etm import lib as etm_lib
    lib = etm_lib.load()
    G, P, dev = 7, 12, torch.device("cuda", 0)
    fb = 3 * (G * P) ** 2
    for W in (16, 64, 1024):
        state = torch.zeros(int(lib.etm_cue_room_state_bytes(W)) // 8, dtype=torch.int64, device=dev)
        frames = torch.zeros((W, fb), dtype=torch.uint8, device=dev)
        actions = torch.from_numpy(np.random.default_rng(0).integers(0, 4, size=(8, W))).to(dev)
        words = [torch.zeros(W, dtype=dt).pin_memory() for dt in (torch.float32, torch.uint8, torch.float32, torch.int32, torch.int64)]
        ptrs = [t.data_ptr() for t in words]
        stream = torch.cuda.current_stream(dev).cuda_stream
        etm_lib.check(lib.etm_cue_room_reset(state.data_ptr(), frames.data_ptr(), fb, *ptrs, None, 0, W, G, P, 2, 32, 0, stream), "reset")

        def run(n):
            for i in range(n):
                rc = lib.etm_cue_room_step(state.data_ptr(), actions[i % 8].data_ptr(), 1, frames.data_ptr(), fb, *ptrs, None, 0, W, G, P,
                                           2, 32, 0, stream)
                if rc != 0:
                    etm_lib.check(rc, "etm_cue_room_step")
        run(50)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(args.steps)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1000.0 / args.steps
        print(f"etm_cue_room_step 84x84 W={W}: {us:.2f} us per step over {args.steps} back-to-back launches (events), "
              f"{W * fb / us / 1e3:.1f} GB/s of frame bytes written", flush=True)


def rollout(args):
    base = _config("cue_room")
    W, S = base["n_workers"], base["worker_steps"]
    env = base["environment"]
    synthetic = dict(type="Synthetic", obs_shape=[3, env["grid"] * env["cell"], env["grid"] * env["cell"]], num_actions=4,
                     max_episode_steps=env["max_episode_steps"], seed=0, p_reward=0.05, p_done=0.05, pool=64, observation_levels=256,
                     observation_dtype="uint8")
    floor = dict(base, environment=synthetic)
    runs = [("device", _config("cue_room_device")), ("host serial", _config("cue_room", vectorize="serial")),
            ("host worker processes", _config("cue_room", vectorize="pipe")), ("Synthetic uint8 floor", floor)]
    trainers = [(name, _trainer(cfg, "measure_" + name.split()[0])) for name, cfg in runs]
    times = {name: [] for name, _ in trainers}
    split = {name: [] for name, _ in trainers}
    try:
        for name, tr in trainers:
            tr._sample_training_data()
            torch.cuda.synchronize()
            print(f"{name}: plan {tr._plan}", flush=True)
        for _ in range(args.pairs):
            for name, tr in trainers:
                for _ in range(args.rollouts):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr._sample_training_data()
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
                    t = tr.last_update_timing
                    split[name].append((t["env_s"], t["wait_s"], t["launch_s"]))
    finally:
        for _, tr in trainers:
            tr.close()
    print(f"rollout phase, W = {W}, S = {S}, {args.pairs} alternated rounds of {args.rollouts} rollouts each:")
    for name, _ in trainers:
        x, sp = np.asarray(times[name]), np.median(np.asarray(split[name]), axis=0)
        print(f"  {name:24s} {1e3 * x.min():7.1f} .. {1e3 * x.max():7.1f} ms per rollout, median {1e3 * np.median(x):7.1f} ms = "
              f"{W * S / np.median(x):9.0f} env-steps/s; medians of env.step / wait / launch: {1e3 * sp[0]:.1f} / {1e3 * sp[1]:.1f} / "
              f"{1e3 * sp[2]:.1f} ms", flush=True)


def behaviour(args):
    for recon in (None, 0.1):
        cfg = _config("cue_room_device")
        if recon is not None:
            cfg["obs_reconstruction"] = recon
        tr = _trainer(cfg, "cue_room_behaviour")
        ended = []
        t0 = time.perf_counter()
        for update in range(args.updates):
            lr, beta, clip = tr.schedules(update)
            infos = tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            tr._train_epochs(lr, clip, beta)
            tr.update_index += 1
            ended.append((sum(i["success"] for i in infos), len(infos), sum(i["length"] for i in infos)))
        torch.cuda.synchronize()
        e = np.asarray(ended, dtype=np.float64)
        k = max(1, args.updates // 10)
        first, last = e[:k].sum(axis=0), e[-k:].sum(axis=0)
        extra = "" if tr.last_obs_reconstruction is None else f"; last reconstruction loss {tr.last_obs_reconstruction['loss']:.4f}"
        print(f"cue_room_device obs_reconstruction={recon}: {args.updates} updates in {time.perf_counter() - t0:.0f} s; success rate of the "
              f"first {k} updates {100 * first[0] / first[1]:.1f} % ({int(first[1])} episodes, mean length {first[2] / first[1]:.1f}), of the "
              f"last {k} updates {100 * last[0] / last[1]:.1f} % ({int(last[1])} episodes, mean length {last[2] / last[1]:.1f}); "
              f"one fixed corner earns 25 %{extra}", flush=True)
        tr.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--steps", type=int, default=500)
    r = sub.add_parser("rollout")
    r.add_argument("--pairs", type=int, default=5)
    r.add_argument("--rollouts", type=int, default=3)
    b = sub.add_parser("behaviour")
    b.add_argument("--updates", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    {"kernel": kernel, "rollout": rollout, "behaviour": behaviour}[args.what](args)
