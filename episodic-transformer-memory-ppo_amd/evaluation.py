"""Batched evaluation of the current policy on the fused rollout (``PPOTrainer.evaluate``, evaluate.py).

The evaluator is a SECOND rollout context next to the training one: a ``PPOTrainer`` built from a copy of the config with the
evaluation's ``n_workers`` and a short ``worker_steps``, whose environments, episode steps and slots, bank, K|V cache, staging,
draw tables and captured step graphs are its own.  The only thing it takes from the training context are the parameters: the
flat parameter arena is copied (read only) before every evaluation -- and, with ``normalize_observations``, the model's running
triple and frozen table, which are buffers outside the arena.  Its draws come from its own ``torch.Generator`` and its
construction leaves torch's generators as it found them, so training with evaluations interleaved is bit-identical to training
without them.

Quota rule: worker w contributes exactly its FIRST ``episodes_per_worker`` finished episodes -- not "the first E episodes to
finish", which would favour short episodes.  Chunks of ``worker_steps`` steps run until every worker has met its quota; episodes
and their memories carry over chunk borders exactly as they carry over updates in training.
"""
import copy
import time

import torch

from run_settings import KL_KEYS, check_evaluation_config
from trainer import PPOTrainer
from utils import process_episode_info


def chunk_bound(episodes_per_worker: int, max_episode_steps: int, worker_steps: int) -> int:
    """The largest number of chunks an evaluation may take: a worker needs at most E * T steps for E episodes of at most T steps, i.e.
    ceil(E * T / worker_steps) chunks, plus one."""
    return -(-int(episodes_per_worker) * int(max_episode_steps) // int(worker_steps)) + 1


class EpisodeQuota:
    """The bookkeeping of the quota rule, on the host and without a device: ``begin_chunk()`` before every chunk (RuntimeError past
    ``chunk_bound``), ``add(worker, info)`` for every episode in the order it finished, ``done``, ``episodes()``."""

    def __init__(self, n_workers: int, episodes_per_worker: int, max_episode_steps: int, worker_steps: int):
        if n_workers < 1 or episodes_per_worker < 1 or worker_steps < 1:
            raise ValueError("n_workers, episodes_per_worker and worker_steps must be positive")
        self.n_workers, self.episodes_per_worker = int(n_workers), int(episodes_per_worker)
        self.max_chunks = chunk_bound(episodes_per_worker, max_episode_steps, worker_steps)
        self.chunks = 0
        self._kept = [[] for _ in range(self.n_workers)]

    def begin_chunk(self):
        if self.chunks >= self.max_chunks:
            short = [w for w, k in enumerate(self._kept) if len(k) < self.episodes_per_worker]
            raise RuntimeError(f"evaluation: workers {short} have not finished {self.episodes_per_worker} episodes after {self.chunks} "
                               f"chunks (the bound for episodes of at most max_episode_steps steps): the environment does not end its episodes")
        self.chunks += 1

    def add(self, worker: int, info: dict) -> bool:
        """An episode of ``worker`` finished.  -> whether it counts (one of the worker's first ``episodes_per_worker``)."""
        kept = self._kept[int(worker)]
        if len(kept) >= self.episodes_per_worker:
            return False
        kept.append(dict(info, worker=int(worker), index=len(kept)))
        return True

    @property
    def done(self) -> bool:
        return all(len(k) >= self.episodes_per_worker for k in self._kept)

    def episodes(self) -> list:
        """The counted episodes' info dicts, each with ``worker`` and ``index``, ordered by (worker, index)."""
        return [info for kept in self._kept for info in kept]


def evaluation_config(config: dict, n_workers: int, worker_steps: int) -> dict:
    """The config of the evaluation's rollout context: the training config with the evaluation's width and chunk length, in-process
    environments whatever training uses, no optimisation-phase sizing that depends on the training batch."""
    cfg = copy.deepcopy({k: v for k, v in config.items() if k != "evaluation"})
    cfg.update(n_workers=int(n_workers), worker_steps=int(worker_steps), n_mini_batch=1, worker_processes=False)
    cfg.pop("episode_bank_capacity", None)        # (sized for the training batch; the default never fills)
    cfg.pop("bootstrap_truncated", None)          # (no GAE target is ever used here; the rollout still strips the two info keys)
    cfg.pop("normalize_rewards", None)            # (likewise; normalize_observations stays: the model reads its table)
    for key in KL_KEYS:                           # (kl_estimator, exact_kl, kl_penalty: no update ever reads a KL and no loss is ever formed
        cfg.pop(key, None)                        # here: neither means nor log-prob rows are staged, the sampling entries of ever)
    cfg.pop("attention_statistics", None)         # (only grad-enabled passes are counted, and none ever runs here)
    if cfg["environment"].get("type") != "Synthetic":
        cfg["environment"]["vectorize"] = "serial"
    return cfg


class _EvaluationRollout(PPOTrainer):
    """The rollout context of the evaluator: a trainer that never optimises, remembers which worker finished which episode and can
    start over on fresh environments."""

    def __init__(self, *args, **kwargs):
        self._finished = []
        super().__init__(*args, **kwargs)

    def _hand_over_episodes(self, g, t, dones, infos, episode_infos):
        import numpy as np
        self._finished.extend(g.lo + int(wl) for wl in np.flatnonzero(dones))
        super()._hand_over_episodes(g, t, dones, infos, episode_infos)

    def restart(self, first_worker_id: int):
        """Fresh environments from ``first_worker_id`` on, every worker at step 0 of an empty episode in slot w (the trainer's
        ``_restart_workers``, which ``restart_episodes`` runs on in training)."""
        self._restart_workers(first_worker_id)


class Evaluator:
    """``run()`` behind ``PPOTrainer.evaluate`` and evaluate.py.  ``parameters``: a callable that returns the flat parameter arena to
    evaluate (the training context's, read before every run), or None when the weights come from ``load_state_dict`` (a checkpoint;
    no training context exists then and no optimiser step ever runs).  The rollout context is allocated by the first run (and again
    when ``n_workers`` or ``worker_steps`` change) and released by ``close()``."""

    DEFAULT_WORKER_STEPS = 64         # chunk length when neither the call nor ``evaluation.worker_steps`` gives one (capped by the config's)

    def __init__(self, config: dict, device, run_id: str = "run", parameters=None, buffers=None):
        self.config, self.device, self.run_id, self.parameters = config, torch.device(device), run_id, parameters
        self.buffers = buffers        # with ``parameters``: a callable -> {name: the training model's buffer} (the observation table)
        self.state_dict = None
        self.rollout = None
        self._key = None
        self.allocated_bytes = 0      # device memory the rollout context took from the allocator when it was built

    def load_state_dict(self, state_dict):
        """The weights of a checkpoint (``PPOTrainer._save_model``'s state dict) for the following runs."""
        self.state_dict = state_dict
        if self.rollout is not None:
            self.rollout.model.load_state_dict(state_dict)

    def _context(self, n_workers, worker_steps, seed):
        key = (n_workers, worker_steps)
        if self.rollout is not None and self._key != key:
            self.close()
        if self.rollout is None:
            cfg = evaluation_config(self.config, n_workers, worker_steps)
            torch.cuda.synchronize(self.device)
            before = torch.cuda.memory_allocated(self.device)
            # the model's initialisation draws from torch's generators: leave them as they were (training continues on them)
            with torch.random.fork_rng(devices=[self.device]):
                self.rollout = _EvaluationRollout(cfg, run_id=self.run_id + "_evaluation", device=self.device, first_worker_id=seed,
                                                  tensorboard=False)
            if self.state_dict is not None:
                self.rollout.model.load_state_dict(self.state_dict)       # (in place: the parameters stay views of the arena)
            self._key = key
            self.allocated_bytes = torch.cuda.memory_allocated(self.device) - before
        return self.rollout

    def run(self, episodes_per_worker=1, n_workers=None, deterministic=True, seed=100000, worker_steps=None) -> dict:
        """-> {"episodes": the counted episodes' info dicts with ``worker`` and ``index``, ordered by (worker, index); "result":
        process_episode_info of them; "steps": environment steps run; "seconds": wall time}."""
        n_workers = int(self.config["n_workers"]) if n_workers is None else int(n_workers)
        if worker_steps is None:
            worker_steps = min(int(self.config["worker_steps"]), self.DEFAULT_WORKER_STEPS)
        worker_steps = int(worker_steps)
        ro = self._context(n_workers, worker_steps, int(seed))
        t0 = time.perf_counter()
        if self.parameters is not None:
            # the current weights, read only: both contexts lay the same model out in the same flat arena
            src, dst = self.parameters(), ro.optimizer.flat_params
            if src.numel() != dst.numel():
                raise RuntimeError("evaluation: the parameter arenas of the two rollout contexts differ")
            with torch.no_grad():
                dst.copy_(src)
                # ... and the model's observation-normalisation buffers (they are no part of the arena), in place
                named = self.buffers() if self.buffers is not None else {}
                for name, buf in ro.model.named_buffers():
                    if name.startswith("obs_norm_"):
                        buf.copy_(named[name])
        ro.restart(int(seed))
        # sampled evaluation: its own generator, seeded per call (never torch's global one)
        ro._draw_generator = None if deterministic else torch.Generator(device=self.device).manual_seed(int(seed))
        quota = EpisodeQuota(n_workers, episodes_per_worker, ro.max_episode_length, worker_steps)
        while not quota.done:
            quota.begin_chunk()
            ro._finished = []
            infos = ro._sample_training_data(deterministic=bool(deterministic))
            if len(infos) != len(ro._finished):
                raise RuntimeError("evaluation: finished episodes and their workers do not match")
            for w, info in zip(ro._finished, infos):
                quota.add(w, info)
        torch.cuda.synchronize(self.device)
        episodes = quota.episodes()
        result = process_episode_info([{k: v for k, v in e.items() if k not in ("worker", "index")} for e in episodes])
        return {"episodes": episodes, "result": result, "steps": quota.chunks * n_workers * worker_steps,
                "seconds": time.perf_counter() - t0}

    def close(self):
        if self.rollout is not None:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self.rollout.close()
            self.rollout = None
            self._key = None


def evaluation_defaults(config: dict) -> dict:
    """The ``evaluation`` section of ``config`` with the defaults filled in (also when the section is absent)."""
    return check_evaluation_config(config) or check_evaluation_config(dict(config, evaluation={}))
