"""Host-side logic of the evaluator (no GPU): the quota rule, the refusals, environment seeding, the evaluation config."""
import inspect
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")


def _info(tag):
    return {"reward": float(tag), "length": int(tag), "success": bool(tag % 2)}


def test_quota_keeps_each_workers_first_episodes_in_worker_order():
    """Worker w contributes exactly its first E finished episodes -- later ones are dropped, however early they finish -- and the
    result is ordered by (worker, index)."""
    from evaluation import EpisodeQuota
    q = EpisodeQuota(n_workers=3, episodes_per_worker=2, max_episode_steps=10, worker_steps=10)
    q.begin_chunk()
    # worker 2 finishes four short episodes before worker 0 finishes one
    for w, tag in ((2, 1), (2, 2), (2, 3), (1, 4), (2, 5), (0, 6)):
        kept = q.add(w, _info(tag))
        assert kept == (tag not in (3, 5))
    assert not q.done
    q.begin_chunk()
    assert q.add(0, _info(7)) and not q.done
    assert q.add(1, _info(8)) and q.done
    assert not q.add(1, _info(9))
    eps = q.episodes()
    assert [(e["worker"], e["index"], e["length"]) for e in eps] == [(0, 0, 6), (0, 1, 7), (1, 0, 4), (1, 1, 8), (2, 0, 1), (2, 1, 2)]
    assert eps == sorted(eps, key=lambda e: (e["worker"], e["index"]))
    assert all(set(e) == {"reward", "length", "success", "worker", "index"} for e in eps)
    assert q.chunks == 2


def test_quota_chunk_bound_raises():
    """More than ceil(E * T / worker_steps) + 1 chunks: RuntimeError."""
    from evaluation import EpisodeQuota, chunk_bound
    assert chunk_bound(3, 32, 8) == 13 and chunk_bound(3, 32, 40) == 4 and chunk_bound(1, 10, 10) == 2 and chunk_bound(2, 7, 3) == 6
    q = EpisodeQuota(n_workers=2, episodes_per_worker=1, max_episode_steps=10, worker_steps=4)
    assert q.max_chunks == 4
    for _ in range(4):
        q.begin_chunk()
    q.add(0, _info(1))
    with pytest.raises(RuntimeError, match=r"workers \[1\]"):
        q.begin_chunk()
    with pytest.raises(ValueError):
        EpisodeQuota(n_workers=0, episodes_per_worker=1, max_episode_steps=10, worker_steps=4)


def _base_config(**over):
    cfg = dict(environment=dict(type="PocMemoryEnv"), n_workers=16, worker_steps=128, n_mini_batch=8)
    cfg.update(over)
    return cfg


def test_evaluation_section_defaults_and_refusals():
    from trainer import check_evaluation_config
    assert check_evaluation_config(_base_config()) is None
    ev = check_evaluation_config(_base_config(evaluation={}))
    assert ev == dict(interval=0, episodes_per_worker=1, n_workers=16, deterministic=True, seed=100000, worker_steps=None)
    ev = check_evaluation_config(_base_config(evaluation=dict(interval=5, episodes_per_worker=2, n_workers=4, deterministic=False, seed=7)))
    assert (ev["interval"], ev["episodes_per_worker"], ev["n_workers"], ev["deterministic"], ev["seed"]) == (5, 2, 4, False, 7)
    # data parallel + periodic evaluation: refused (the trainer asks before any environment is built); without an interval it is not
    with pytest.raises(ValueError, match="data-parallel"):
        check_evaluation_config(_base_config(evaluation=dict(interval=1)), world=2)
    assert check_evaluation_config(_base_config(evaluation=dict(episodes_per_worker=2)), world=2)["interval"] == 0
    assert check_evaluation_config(_base_config(evaluation=dict(interval=1)), world=1)["interval"] == 1
    with pytest.raises(ValueError, match="unknown"):
        check_evaluation_config(_base_config(evaluation=dict(intervall=1)))
    with pytest.raises(ValueError):
        check_evaluation_config(_base_config(evaluation=dict(episodes_per_worker=0)))


def test_trainer_checks_evaluation_before_building_environments():
    """The constructor asks check_evaluation_config with the data-parallel world before it creates the writer or any environment."""
    import types

    import torch
    import trainer
    from environments import shm_env
    built = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(trainer, "_make_writer", lambda *a, **k: built.append("writer"))
        mp.setattr(trainer, "make_vec_env", lambda *a, **k: built.append("make_vec_env"))
        mp.setattr(shm_env, "ShmVecEnv", lambda *a, **k: built.append("ShmVecEnv"))
        for worker_processes in (False, True):
            cfg = _base_config(evaluation=dict(interval=1), worker_processes=worker_processes, hidden_layer_size=64,
                               transformer=dict(num_blocks=2, embed_dim=64, num_heads=2, memory_length=8, positional_encoding="relative",
                                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
                               **{k: dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10)
                                  for k in ("learning_rate_schedule", "beta_schedule", "clip_range_schedule")})
            with pytest.raises(ValueError, match="evaluation.interval in a data-parallel run"):
                trainer.PPOTrainer(cfg, device=torch.device("cuda", 0), dp=types.SimpleNamespace(world=2, rank=0))      # (no device is touched)
    assert built == []


def test_uniforms_with_deterministic_is_a_value_error():
    """_sample_training_data refuses uniforms= / normals= together with deterministic=True before it touches the device."""
    from trainer import PPOTrainer
    tr = object.__new__(PPOTrainer)            # (no device: the refusal comes first)
    for kw in (dict(uniforms=np.zeros((2, 2), dtype=np.float32)), dict(normals=np.zeros((2, 2, 1), dtype=np.float32))):
        with pytest.raises(ValueError, match="deterministic"):
            tr._sample_training_data(deterministic=True, **kw)
    assert inspect.signature(PPOTrainer._sample_training_data).parameters["deterministic"].default is False


def test_create_env_seeds_poc_memory_env_per_worker():
    """environment.seed present: worker w draws from seed + w (repeatable, different between workers); absent: unseeded."""
    from utils import create_env

    def starts(env, n=12):
        out = []
        for _ in range(n):
            obs = env.reset()
            out.append((float(obs[0]), float(obs[1]), float(obs[2])))
        return out

    cfg = dict(type="PocMemoryEnv", seed=11)
    a, b = starts(create_env(cfg, worker_id=3)), starts(create_env(cfg, worker_id=3))
    assert a == b
    assert a != starts(create_env(cfg, worker_id=4))
    assert a == starts(create_env(dict(type="PocMemoryEnv", seed=10), worker_id=4)), "the stream is seed + worker_id"
    from environments.poc_memory_env import PocMemoryEnv
    assert a == starts(PocMemoryEnv(glob=False, freeze=True, max_episode_steps=32, seed=14))
    # absent: numpy's unseeded generator (fresh entropy) -- two environments disagree somewhere in 40 resets
    free = dict(type="PocMemoryEnv")
    assert starts(create_env(free, worker_id=3), 40) != starts(create_env(free, worker_id=3), 40)


def test_evaluation_config_of_the_second_rollout_context():
    """The evaluator's config copy: evaluation width and chunk length, in-process environments, nothing shared with the original."""
    from evaluation import evaluation_config
    cfg = _base_config(worker_processes=True, episode_bank_capacity=99, evaluation=dict(interval=1))
    ev = evaluation_config(cfg, 4, 8)
    assert (ev["n_workers"], ev["worker_steps"], ev["n_mini_batch"], ev["worker_processes"]) == (4, 8, 1, False)
    assert "evaluation" not in ev and "episode_bank_capacity" not in ev
    assert ev["environment"] == dict(type="PocMemoryEnv", vectorize="serial")
    assert cfg["environment"] == dict(type="PocMemoryEnv") and cfg["n_workers"] == 16 and cfg["worker_processes"] is True
    syn = evaluation_config(_base_config(environment=dict(type="Synthetic", obs_shape=[4])), 4, 8)
    assert "vectorize" not in syn["environment"]


def test_eval_yaml_parses():
    """configs/poc_memory_env_eval.yaml: the PoC config plus a seeded environment and the evaluation section."""
    from trainer import check_evaluation_config
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(PKG, "configs", "poc_memory_env_eval.yaml")).get_config()
    base = YamlParser(os.path.join(PKG, "configs", "poc_memory_env.yaml")).get_config()
    assert cfg["evaluation"] == dict(interval=10, episodes_per_worker=2, n_workers=16, deterministic=True, seed=100000)
    assert cfg["environment"] == dict(type="PocMemoryEnv", seed=0)
    assert {k: v for k, v in cfg.items() if k not in ("evaluation", "environment")} == {k: v for k, v in base.items() if k != "environment"}
    assert "evaluation" not in base and "seed" not in base["environment"]
    ev = check_evaluation_config(cfg)
    assert ev["interval"] == 10 and ev["worker_steps"] is None


def test_evaluate_py_refuses_to_run_without_a_device(monkeypatch):
    """The same no-device SystemExit as train.py, before the checkpoint is opened."""
    import torch
    import evaluate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr("sys.argv", ["evaluate.py", "--model", "/nonexistent/run.nn", "--workers", "4", "--sample"])
    with pytest.raises(SystemExit, match="no HIP device visible"):
        evaluate.main()
