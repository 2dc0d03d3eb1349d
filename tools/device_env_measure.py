"""Measurements behind the README sections on the device-resident environments (profiles/r22/device_env.txt, profiles/r23/command_room.txt,
profiles/r24/device_env_refactor.txt, profiles/r25/path_room.txt, profiles/r26/spot_room.txt).  Needs the MI355X.  ``ETM_DIAG_LIB=<path>`` measures another build of the library.

  python tools/device_env_measure.py kernel [--steps 500] [--rounds 3]
      etm_cue_room_step, etm_command_room_step, etm_path_room_step and etm_spot_room_step side by side in one process, at 84 x 84 (grid 7, cell 12) and W in {16, 64, 1024}:
      device time per step between two events around ``steps`` back-to-back launches on one stream (frames to device memory, result
      words to pinned host memory), after a warm-up; ``rounds`` alternated rounds, every round printed.
  python tools/device_env_measure.py rollout [--type CueRoom|CommandRoom|PathRoom|SpotRoom] [--pairs 5] [--rollouts 3]
      the rollout phase of the type's device config (configs/cue_room_device.yaml, command_room_device.yaml, path_room_device.yaml, spot_room_device.yaml) against its host config
      -- the host twin stepped serially and, for CueRoom, through worker processes (``vectorize: pipe``) -- and against the
      ``Synthetic`` uint8 config of equal shape and action count, the floor a host environment that costs nothing reaches.  All
      trainers alive in one process, one warm-up rollout each (it captures the step graphs), then ``pairs`` alternated rounds of
      ``rollouts`` rollouts: seconds per rollout and environment steps per second, range and median, with the trainer's own split
      (env.step, waiting for the actions, upload + launch).
  python tools/device_env_measure.py behaviour [--type CueRoom|CommandRoom|PathRoom|SpotRoom] [--updates 200]
      the type's device config for ``updates`` updates, twice (no assertion).  CueRoom: with and without ``obs_reconstruction``;
      success rate of the episodes that ended in the first and the last tenth of the run (always walking to one corner earns 25 %).
      CommandRoom: as configured and with ``memory_length`` cut to ``command_count``; success rate and mean commands completed,
      beside what a uniformly random policy reaches.  PathRoom: as configured and with ``memory_length`` cut to 8; mean best / n (the
      share of the path reached), success rate and falls per episode, beside a uniformly random policy stepped on the host twin.
      SpotRoom: as configured, with ``previous_step_input: false`` and with ``memory_length`` cut to 8; mean return, success rate,
      share of deaths, coins and damage per episode of the episodes that ended in the first and the last tenth, beside a uniformly
      random policy stepped on the host twin.
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

if os.environ.get("ETM_DIAG_LIB"):
    from etm import lib as etm_lib      # noqa: E402
    etm_lib.LIB_PATH = os.environ["ETM_DIAG_LIB"]


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
    # (name, reset entry, step entry, state bytes, rule words behind W, actions)
    tasks = [("etm_cue_room_step", lib.etm_cue_room_reset, lib.etm_cue_room_step, lib.etm_cue_room_state_bytes, (G, P, 2, 32, 0), 4),
             ("etm_command_room_step", lib.etm_command_room_reset, lib.etm_command_room_step, lib.etm_command_room_state_bytes,
              (G, P, 8, 1, 1, 0), 5),
             ("etm_path_room_step", lib.etm_path_room_reset, lib.etm_path_room_step, lib.etm_path_room_state_bytes, (G, P, 16, 64, 0), 4),
             ("etm_spot_room_step", lib.etm_spot_room_reset, lib.etm_spot_room_step, lib.etm_spot_room_state_bytes,
              (G, P, 2, 2, 2, 5, 64, 0), 5)]
    for W in (16, 64, 1024):
        frames = torch.zeros((W, fb), dtype=torch.uint8, device=dev)
        words = [torch.zeros(W, dtype=dt).pin_memory() for dt in (torch.float32, torch.uint8, torch.float32, torch.int32, torch.int64)]
        ptrs = [t.data_ptr() for t in words]
        stream = torch.cuda.current_stream(dev).cuda_stream
        runs = []
        for name, reset, step, state_bytes, rule, n_act in tasks:
            state = torch.zeros(int(state_bytes(W)) // 8, dtype=torch.int64, device=dev)
            actions = torch.from_numpy(np.random.default_rng(0).integers(0, n_act, size=(8, W))).to(dev)
            etm_lib.check(reset(state.data_ptr(), frames.data_ptr(), fb, *ptrs, None, 0, W, *rule, stream), name + " (reset)")

            def run(n, step=step, state=state, actions=actions, rule=rule, name=name):
                for i in range(n):
                    rc = step(state.data_ptr(), actions[i % 8].data_ptr(), 1, frames.data_ptr(), fb, *ptrs, None, 0, W, *rule, stream)
                    if rc != 0:
                        etm_lib.check(rc, name)
            run(50)
            torch.cuda.synchronize()
            runs.append((name, run, []))
        for _ in range(args.rounds):
            for name, run, us in runs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(args.steps)
                b.record()
                torch.cuda.synchronize()
                us.append(a.elapsed_time(b) * 1000.0 / args.steps)
        for name, _, us in runs:
            med = float(np.median(us))
            print(f"{name} 84x84 W={W}: {' / '.join(f'{u:.2f}' for u in us)} us per step over {args.steps} back-to-back launches (events, "
                  f"{args.rounds} alternated rounds), median {med:.2f} us = {W * fb / med / 1e3:.1f} GB/s of frame bytes written", flush=True)


# per type: the config names' stem, the action count, and whether the worker-process front-end is among the rollout's runs
TYPES = {"CueRoom": ("cue_room", 4, True), "CommandRoom": ("command_room", 5, False), "PathRoom": ("path_room", 4, False),
         "SpotRoom": ("spot_room", 5, False)}


def rollout(args):
    stem, n_act, with_pipe = TYPES[args.type]
    base = _config(stem)
    W, S = base["n_workers"], base["worker_steps"]
    env = base["environment"]
    if "max_episode_steps" in env:
        longest = env["max_episode_steps"]
    else:
        longest = env["command_count"] * (env["show_steps"] + env["gap_steps"] + 1)
    synthetic = dict(type="Synthetic", obs_shape=[3, env["grid"] * env["cell"], env["grid"] * env["cell"]], num_actions=n_act,
                     max_episode_steps=longest, seed=0, p_reward=0.05, p_done=0.05, pool=64, observation_levels=256,
                     observation_dtype="uint8")
    floor = dict(base, environment=synthetic)
    runs = [("device", _config(stem + "_device")), ("host serial", _config(stem, vectorize="serial"))]
    if with_pipe:
        runs.append(("host worker processes", _config(stem, vectorize="pipe")))
    runs.append(("Synthetic uint8 floor", floor))
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


def _train(cfg, run_id, updates, count, tr=None):
    """``updates`` updates of ``cfg`` (on the trainer ``tr`` where one is given) -> (the trainer, still open; ``count(infos)`` summed
    over the first tenth of the updates and over the last, as float arrays; how many updates a tenth is; seconds)."""
    tr = _trainer(cfg, run_id) if tr is None else tr
    ended = []
    t0 = time.perf_counter()
    for update in range(updates):
        lr, beta, clip = tr.schedules(update)
        infos = tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        tr._train_epochs(lr, clip, beta)
        tr.update_index += 1
        ended.append(count(infos))
    torch.cuda.synchronize()
    e = np.asarray(ended, dtype=np.float64)
    k = max(1, updates // 10)
    return tr, e[:k].sum(axis=0), e[-k:].sum(axis=0), k, time.perf_counter() - t0


def _behaviour_cue_room(args):
    for recon in (None, 0.1):
        cfg = _config("cue_room_device")
        if recon is not None:
            cfg["obs_reconstruction"] = recon
        tr, first, last, k, seconds = _train(cfg, "cue_room_behaviour", args.updates, lambda infos: (
            sum(i["success"] for i in infos), len(infos), sum(i["length"] for i in infos)))
        extra = "" if tr.last_obs_reconstruction is None else f"; last reconstruction loss {tr.last_obs_reconstruction['loss']:.4f}"
        print(f"cue_room_device obs_reconstruction={recon}: {args.updates} updates in {seconds:.0f} s; success rate of the "
              f"first {k} updates {100 * first[0] / first[1]:.1f} % ({int(first[1])} episodes, mean length {first[2] / first[1]:.1f}), of the "
              f"last {k} updates {100 * last[0] / last[1]:.1f} % ({int(last[1])} episodes, mean length {last[2] / last[1]:.1f}); "
              f"one fixed corner earns 25 %{extra}", flush=True)
        tr.close()


def _behaviour_command_room(args):
    K = _config("command_room_device")["environment"]["command_count"]
    # a policy uniform over the five actions answers command e correctly with probability 1 / 5, whatever the command
    chance_n, chance_success = sum(0.2 ** k for k in range(1, K + 1)), 0.2 ** K
    for window in (None, K):
        cfg = _config("command_room_device")
        if window is not None:
            cfg["transformer"]["memory_length"] = window
        tr, first, last, k, seconds = _train(cfg, "command_room_behaviour", args.updates, lambda infos: (
            sum(i["success"] for i in infos), len(infos), sum(round(i["reward"] * 10) for i in infos)))
        print(f"command_room_device memory_length={cfg['transformer']['memory_length']}: {args.updates} updates in "
              f"{seconds:.0f} s; first {k} updates: success {100 * first[0] / first[1]:.2f} %, "
              f"{first[2] / first[1]:.2f} of {K} commands completed on average ({int(first[1])} episodes); last {k} updates: success "
              f"{100 * last[0] / last[1]:.2f} %, {last[2] / last[1]:.2f} commands ({int(last[1])} episodes); a uniformly random policy: "
              f"success {100 * chance_success:.4f} %, {chance_n:.2f} commands", flush=True)
        tr.close()


class _PathRoomRecorder:
    """What PathRoom's infos do not carry, per finished episode: n (from the episode draw: every worker's episodes follow one
    another from 0) and the falls (the mark bits of the state words, read back after every step; a fall in the step that ends an
    episode is not seen, the state is the next episode's by then)."""

    def __init__(self, front_ends):
        self.total = np.zeros(4)                  # sum of best / n, successes, episodes, falls of the episodes that ended
        for env in front_ends:
            self._wrap(env)

    def _wrap(self, env):
        from environments.path_room_env import episode_draw
        results = env._results
        W, G, M = env.num_envs, env.grid, env.path_moves
        episode, falls = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)

        def recorded():
            rewards, dones, infos = results()
            falls[:] += ((env._state.view(W, 4)[:, 3].cpu().numpy() >> 53) & 0x7ff) != 0
            for w in np.flatnonzero(dones):
                n = len(episode_draw(env.stream0 + int(w), int(episode[w]), G, M)[1])
                best = round(infos[w]["reward"] * 10) - 10 * infos[w]["success"]
                self.total += (best / n, infos[w]["success"], 1, falls[w])
                episode[w] += 1
                falls[w] = 0
            return rewards, dones, infos
        env._results = recorded

    def take(self, infos):
        total, self.total = self.total, np.zeros(4)
        return tuple(total)


def _path_room_random_policy(env, episodes=1000):
    """(mean best / n, success rate, falls per episode) of a policy uniform over the four actions, on the host twin."""
    from environments.path_room_env import PathRoomEnv
    e = PathRoomEnv(**{k: v for k, v in env.items() if k in ("grid", "cell", "path_moves", "max_episode_steps", "seed")})
    rng = np.random.default_rng(0)
    share = success = falls = 0.0
    for _ in range(episodes):
        e.reset()
        while True:
            _, _, done, info = e.step(int(rng.integers(0, 4)))
            falls += e.mark is not None and not done      # (as the recorder counts: not in the step that ends the episode)
            if done:
                share += e.best / len(e.moves)
                success += info["success"]
                break
    return share / episodes, success / episodes, falls / episodes


def _behaviour_path_room(args):
    chance = _path_room_random_policy(_config("path_room_device")["environment"])
    for window in (None, 8):
        cfg = _config("path_room_device")
        if window is not None:
            cfg["transformer"]["memory_length"] = window
        recorder = []

        def count(infos):
            return recorder[0].take(infos)
        tr = _trainer(cfg, "path_room_behaviour")
        recorder.append(_PathRoomRecorder(list(getattr(tr.env, "parts", None) or [tr.env])))
        tr, first, last, k, seconds = _train(cfg, "path_room_behaviour", args.updates, count, tr)

        def line(x):
            return (f"best / n {x[0] / x[2]:.3f}, success {100 * x[1] / x[2]:.2f} %, {x[3] / x[2]:.2f} falls per episode "
                    f"({int(x[2])} episodes)")
        print(f"path_room_device memory_length={cfg['transformer']['memory_length']}: {args.updates} updates in {seconds:.0f} s; "
              f"first {k} updates: {line(first)}; last {k} updates: {line(last)}; a uniformly random policy (1000 episodes of the "
              f"host twin): best / n {chance[0]:.3f}, success {100 * chance[1]:.2f} %, {chance[2]:.2f} falls per episode", flush=True)
        tr.close()


def _spot_room_episodes(infos, health):
    """(sum of returns, successes, deaths, coins, damage, episodes) of finished SpotRoom episodes, from their infos alone: the return
    is 5 coin + 10 success - damage tenths; an ending that is neither a success nor a cut is a death and has lost all ``health``
    points, every other episode has lost fewer, so with ``health`` <= 5 (asserted) the sign of 5 coin - damage tells the coin."""
    assert health <= 5, "the coin and the damage are read apart only while the damage stays below the coin's 5 tenths"
    total = np.zeros(6)
    for i in infos:
        tenths = round(i["reward"] * 10) - 10 * i["success"]
        death = not i["success"] and not i.get("truncated", False)
        damage = health if death else (5 - tenths if tenths > 0 else -tenths)
        total += (i["reward"], i["success"], death, (tenths + damage) // 5, damage, 1)
    return tuple(total)


def _spot_room_line(x):
    return (f"return {x[0] / x[5]:.3f}, success {100 * x[1] / x[5]:.2f} %, deaths {100 * x[2] / x[5]:.2f} %, coins {100 * x[3] / x[5]:.2f} %, "
            f"damage {x[4] / x[5]:.2f} per episode ({int(x[5])} episodes)")


def _spot_room_random_policy(env, episodes=1000):
    """``_spot_room_episodes`` of a policy uniform over the five actions, on the host twin."""
    from environments.spot_room_env import SpotRoomEnv
    e = SpotRoomEnv(**{k: v for k, v in env.items() if k not in ("type", "device", "vectorize")})
    rng = np.random.default_rng(0)
    infos = []
    for _ in range(episodes):
        e.reset()
        done = False
        while not done:
            _, _, done, info = e.step(int(rng.integers(0, 5)))
        infos.append(info)
    return _spot_room_episodes(infos, env["health"])


def _behaviour_spot_room(args):
    env = _config("spot_room_device")["environment"]
    print(f"spot_room: a uniformly random policy (1000 episodes of the host twin): {_spot_room_line(_spot_room_random_policy(env))}", flush=True)
    for name, change in (("as configured", {}), ("previous_step_input=false", {"previous_step_input": False}),
                         ("memory_length=8", {"memory_length": 8})):
        cfg = _config("spot_room_device")
        if "previous_step_input" in change:
            cfg["previous_step_input"] = False
        if "memory_length" in change:
            cfg["transformer"]["memory_length"] = change["memory_length"]
        tr, first, last, k, seconds = _train(cfg, "spot_room_behaviour", args.updates, lambda infos: _spot_room_episodes(infos, env["health"]))
        print(f"spot_room_device {name}: {args.updates} updates in {seconds:.0f} s; first {k} updates: {_spot_room_line(first)}; "
              f"last {k} updates: {_spot_room_line(last)}", flush=True)
        tr.close()


def behaviour(args):
    {"CueRoom": _behaviour_cue_room, "CommandRoom": _behaviour_command_room, "PathRoom": _behaviour_path_room,
     "SpotRoom": _behaviour_spot_room}[args.type](args)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--steps", type=int, default=500)
    k.add_argument("--rounds", type=int, default=3)
    r = sub.add_parser("rollout")
    r.add_argument("--type", choices=list(TYPES), default="CueRoom")
    r.add_argument("--pairs", type=int, default=5)
    r.add_argument("--rollouts", type=int, default=3)
    b = sub.add_parser("behaviour")
    b.add_argument("--type", choices=list(TYPES), default="CueRoom")
    b.add_argument("--updates", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    {"kernel": kernel, "rollout": rollout, "behaviour": behaviour}[args.what](args)
