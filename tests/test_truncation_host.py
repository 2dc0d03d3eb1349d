"""CPU: the environment side of time-limit bootstrapping (``bootstrap_truncated``).

* ``SerialVecEnv`` hands the observation of a truncated episode's last step over as ``info["final_observation"]`` -- a copy, in the
  environment's dtype, only next to ``"truncated"`` -- and still returns the reset observation in its rows.
* ``PocMemoryEnv(report_truncation=...)``: off, the info dicts are key for key what they were; on, ``truncated`` marks exactly the
  episodes that were cut at the time limit away from a goal.
* ``worker_processes: true`` with ``bootstrap_truncated: true`` is refused before anything is built.
* ``configs/poc_memory_env_truncation.yaml`` parses to ``poc_memory_env.yaml`` plus the two keys.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")


class _Scripted:
    """One environment whose episodes end after ``lengths[k]`` steps, ``how[k]`` in ("terminated", "truncated"); the observation of
    episode k, step s (0 = the reset) is filled with 10 * k + s."""

    def __init__(self, lengths, how, dtype):
        self.lengths, self.how, self.dtype = lengths, how, dtype
        self.observation_space = SimpleNamespace(shape=(2, 3), dtype=dtype)
        self.action_space = SimpleNamespace(n=2)
        self.max_episode_steps = 8
        self.k, self.s = -1, 0
        self.handed_out = []

    def _obs(self):
        o = np.full((2, 3), 10 * self.k + self.s, dtype=self.dtype)
        self.handed_out.append(o)
        return o

    def reset(self):
        self.k, self.s = self.k + 1, 0
        return self._obs()

    def step(self, action):
        self.s += 1
        done = self.s == self.lengths[self.k]
        info = None
        if done:
            info = {"reward": 1.0, "length": self.s}
            if self.how[self.k] == "truncated":
                info["truncated"] = True
        return self._obs(), 0.5, done, info

    def close(self):
        pass


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float32", "uint8"])
def test_serial_vec_env_hands_over_the_final_observation(dtype):
    from environments.vec_env import SerialVecEnv
    env = _Scripted(lengths=[2, 3, 1, 4], how=["truncated", "terminated", "truncated", "terminated"], dtype=dtype)
    vec = SerialVecEnv([env])
    out = np.zeros((1, 2, 3), dtype=dtype)
    vec.reset(out=out)
    assert out[0, 0, 0] == 0
    seen = []
    for _ in range(6):                                 # episodes 0, 1 and 2 end; episode 3 is running
        rows, rewards, dones, infos = vec.step(np.zeros(1, dtype=np.int64), out=out)
        assert rows is out and rows.dtype == dtype
        seen.append((int(rows[0, 0, 0]), bool(dones[0]), infos[0]))
    values = [v for v, _, _ in seen]
    assert values == [1, 10, 11, 12, 20, 30], "the returned rows of a finished worker are the reset observations"
    ends = [(i, info) for i, (_, done, info) in enumerate(seen) if done]
    assert [i for i, _ in ends] == [1, 4, 5] and all(info is None for _, d, info in seen if not d)
    (_, first), (_, second), (_, third) = ends
    assert first["truncated"] is True and third["truncated"] is True
    assert "truncated" not in second and "final_observation" not in second, "final_observation comes only with truncated"
    for info, value in ((first, 2), (third, 21)):
        fo = info["final_observation"]
        assert isinstance(fo, np.ndarray) and fo.dtype == dtype and fo.shape == (2, 3)
        assert (fo == value).all(), "the observation step() returned for the last step, not the reset one"
        assert not any(np.shares_memory(fo, o) for o in env.handed_out) and not np.shares_memory(fo, out), "a copy"
    assert {k for k in first if k not in ("truncated", "final_observation")} == {"reward", "length"}


def _run_poc(report, seed, policy, episodes=40):
    from environments.poc_memory_env import PocMemoryEnv
    kw = {} if report is None else {"report_truncation": report}
    env = PocMemoryEnv(glob=False, freeze=True, max_episode_steps=32, seed=seed, **kw)
    out = []
    for _ in range(episodes):
        env.reset()
        t, info, trace = 0, None, []
        while True:
            _, r, done, info = env.step([policy(t)])
            trace.append((r, done, None if info is None else dict(info)))
            t += 1
            if done:
                break
        out.append((trace, abs(env._pos) == 1.0))
    return out


def test_poc_memory_env_infos_unchanged_with_the_flag_off():
    dither = lambda t: t % 2                    # never reaches an end: every episode is cut at 32 steps
    left = lambda t: 0
    for policy in (dither, left):
        default, off = _run_poc(None, 5, policy), _run_poc(False, 5, policy)
        assert default == off
        for trace, _ in off:
            info = trace[-1][2]
            assert list(info) == ["success", "reward", "length"], "key for key the info dict of every finished episode so far"
            assert all(i is None for _, _, i in trace[:-1])


def test_poc_memory_env_reports_time_limit_cuts_only():
    dither = lambda t: t % 2
    left = lambda t: 0
    cuts = _run_poc(True, 5, dither)
    assert all(len(trace) == 32 and not at_goal and trace[-1][2].get("truncated") is True for trace, at_goal in cuts)
    goals = _run_poc(True, 5, left)
    assert all(at_goal and len(trace) < 32 and "truncated" not in trace[-1][2] for trace, at_goal in goals)
    # everything else is what the flag-off environment reports
    for (trace_on, _), (trace_off, _) in zip(cuts + goals, _run_poc(False, 5, dither) + _run_poc(False, 5, left)):
        strip = lambda tr: [(r, d, None if i is None else {k: v for k, v in i.items() if k != "truncated"}) for r, d, i in tr]
        assert strip(trace_on) == trace_off
    # a goal reached AT the time limit is a termination: walk so that the last admitted step arrives at an end
    from environments.poc_memory_env import PocMemoryEnv
    for seed in range(16):                       # a start from which the right end is an even number of steps away
        env = PocMemoryEnv(glob=False, freeze=True, max_episode_steps=32, seed=seed, report_truncation=True)
        env.reset()
        steps_to_right = int(round((1.0 - env._pos) / 0.2))
        if steps_to_right % 2 == 0:
            break
    spare = 30 - steps_to_right                  # steps 2 .. 31 move (the first two are frozen)
    assert spare >= 0 and spare % 2 == 0
    plan = [0, 0] + [0, 1] * (spare // 2) + [1] * steps_to_right
    info = None
    for a in plan:
        _, _, done, info = env.step([a])
    assert done and env._t == 32 and abs(env._pos) == 1.0 and "truncated" not in info


def test_create_env_forwards_report_truncation():
    from utils import create_env
    assert create_env({"type": "PocMemoryEnv"}).report_truncation is False
    assert create_env({"type": "PocMemoryEnv", "report_truncation": True}).report_truncation is True


def test_worker_processes_with_bootstrap_truncated_is_refused():
    from trainer import check_truncation_transport
    with pytest.raises(ValueError) as exc:
        check_truncation_transport({"worker_processes": True, "bootstrap_truncated": True})
    msg = str(exc.value)
    assert "worker_processes" in msg and "bootstrap_truncated" in msg and "final observation" in msg and "shared segment" in msg
    check_truncation_transport({"worker_processes": True})
    check_truncation_transport({"worker_processes": True, "bootstrap_truncated": False})
    check_truncation_transport({"worker_processes": False, "bootstrap_truncated": True})
    check_truncation_transport({"worker_processes": True, "bootstrap_truncated": True}, env=object())      # (a supplied environment is in-process)


def test_truncation_config_parses():
    from yaml_parser import YamlParser
    base = YamlParser(os.path.join(PKG, "configs", "poc_memory_env.yaml")).get_config()
    cfg = YamlParser(os.path.join(PKG, "configs", "poc_memory_env_truncation.yaml")).get_config()
    assert cfg["bootstrap_truncated"] is True and cfg["environment"] == {"type": "PocMemoryEnv", "report_truncation": True}
    assert "bootstrap_truncated" not in base and base["environment"] == {"type": "PocMemoryEnv"}
    rest = {k: v for k, v in cfg.items() if k not in ("bootstrap_truncated", "environment")}
    assert rest == {k: v for k, v in base.items() if k != "environment"}
