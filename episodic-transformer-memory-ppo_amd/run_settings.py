"""Run settings: every optional config key resolved once, outside the trainer.

``RunSettings`` is what ``PPOTrainer`` knows about its optional keys.  It is filled in two stages, and the order in which the stages
refuse a config is a contract (users see the first refusal; tests/test_constructor_refusals_gpu.py pins it through the constructor,
tests/test_run_settings_host.py through this module).  A refusal is a ValueError raised before anything is built from the key.

``RunSettings.before_environment(config, world, env, resume)`` -- from the config alone, before any environment or process exists
(the trainer has refused a non-HIP device with a RuntimeError before it gets here):

 1. ``check_kernel_shapes``: the transformer's shape against the gfx950 kernels.
 2. ``check_box_policy``: a Box the config declares (``environment.continuous_actions``): 1..8 dimensions, ``hidden_layer_size``.
 3. ``check_byte_observation_transport``: ``worker_processes`` with uint8 observations.
 4. ``check_truncation_transport``: ``worker_processes`` with ``bootstrap_truncated``.
 5. ``check_device_env_config`` (environments/device_types.py; only without a supplied ``env``): ``environment.device``.
 6. ``check_action_mask_config``: ``action_masks`` with a declared Box, with more than 63 declared actions, with ``worker_processes``
    (a supplied ``env``: without ``action_masks()``).
 7. ``utils.previous_step_input_section``: the value of ``previous_step_input``; the key with ``worker_processes``.
 8. ``check_evaluation_config``: unknown keys and ranges of ``evaluation``; ``evaluation.interval`` in a data-parallel run.
 9. ``check_normalization_config``: the values of ``normalize_observations`` / ``normalize_rewards``; either in a data-parallel run.
10. ``check_checkpoint_config`` (checkpoint.py): the value of ``checkpoint_interval``; the key, or a resume, in a data-parallel run.
11. ``check_target_kl_config``: the value of ``target_kl``; the key in a data-parallel run.
12. ``check_adaptive_lr_config``: the value of ``adaptive_lr``; the key in a data-parallel run, with a decaying schedule, with a start
    value outside [min, max].
13. ``check_kl_estimator_config``: the value of ``kl_estimator``; ``analytic`` without a declared Box (a supplied ``env`` says what the
    policy is in stage two); ``analytic`` in a data-parallel run.
14. ``check_exact_kl_config``: the value of ``exact_kl``; ``true`` next to ``kl_estimator: k3``; ``true`` in a data-parallel run.
15. ``check_kl_penalty_config``: the value of ``kl_penalty``; the key next to ``exact_kl: false`` or ``kl_estimator: k3``; the key in a
    data-parallel run.
16. ``utils.obs_reconstruction_section``: the value of ``obs_reconstruction``; the key in a data-parallel run.
17. ``check_attention_statistics_config``: the value of ``attention_statistics``; ``true`` in a data-parallel run.

``.with_environment(env, observation_shape, observation_dtype, action_space_shape, box)`` -- once the environment exists and has been
looked at, before the buffer, the model or any device word is allocated:

 1. uint8 observations that are no images.
 2. ``check_normalization_config``: ``normalize_observations`` with image or uint8 observations, or with too many features.
 3. ``check_box_policy``: the environment's Box (``box``): 1..8 dimensions, ``hidden_layer_size``.
 4. ``check_action_mask_config``: ``action_masks`` with the environment's Box, with more than 63 actions, without ``action_masks()``.
 5. ``utils.previous_step_input_section``: ``previous_step_input`` with a Box policy, with a table of more than 64 rows.
 6. ``check_kl_estimator_config``: ``kl_estimator: analytic`` on a categorical environment.
 7. ``utils.obs_reconstruction_section``: ``obs_reconstruction`` on observations the decoder does not map back onto themselves.

A new optional key adds a field to ``RunSettings``, a ``check_*`` function and a line in the list above -- all in this file; a key that
implies the exact KL's plumbing adds itself to ``KL_KEYS`` and ``kl_plumbing``.  trainer.py re-exports every ``check_*`` name.  The
on/off tuning switches (``hip_graph_train``, ``kv_cache_rollout``, ...) are not settings: they are read with ``config.get`` where they
are used, and tools flip them on a live trainer.
"""
from dataclasses import dataclass, replace

import numpy as np
import torch

from checkpoint import check_checkpoint_config
from environments.device_types import check_device_env_config, is_byte_only
from etm import lib as etm_lib
from etm import ops
from utils import (adaptive_lr_section, attention_statistics_section, exact_kl_section, kl_estimator_section, kl_penalty_section,
                   normalization_section, obs_reconstruction_section, previous_step_input_section, target_kl_section)


def world_of(dp) -> int:
    """The number of data-parallel ranks: 1 without ``dp``."""
    return 1 if dp is None else int(getattr(dp, "world", 1))


def check_kernel_shapes(tcfg: dict):
    """Fail early (before any environment or buffer is built) if the transformer shape is outside what the gfx950
    kernels are built for; there is no fallback path."""
    d, h, mem = tcfg["embed_dim"], tcfg["num_heads"], tcfg["memory_length"]
    if d % h != 0:
        raise ValueError("Embedding dimension needs to be divisible by the number of heads")
    hd = d // h
    problems = []
    if d % 32 != 0 or d > 1024:
        problems.append(f"embed_dim={d} (need a multiple of 32, <= 1024)")
    if hd % 32 != 0 or hd > 128:
        problems.append(f"head_dim={hd} (need 32, 64, 96 or 128)")
    if mem > 128:
        problems.append(f"memory_length={mem} (need <= 128)")
    if not problems and ops.attention_supported(d, h, mem, ln=tcfg.get("layer_norm") == "pre",
                                                pos_grad=tcfg.get("positional_encoding") == "learned") is None:
        problems.append(f"attention backward at embed_dim={d}, num_heads={h}, memory_length={mem}, layer_norm="
                        f"{tcfg.get('layer_norm')}, positional_encoding={tcfg.get('positional_encoding')} (LDS: see DESIGN.md section 6)")
    if problems:
        raise ValueError("transformer shape not supported by the MI355X kernels: " + "; ".join(problems))


def check_box_policy(config: dict, A=None):
    """Fail early for a Box (continuous) policy the fused kernels do not take: A = ``environment.continuous_actions`` (or the
    dimension of the environment's Box) must lie in 1..8 and ``hidden_layer_size`` inside the Gaussian heads + loss kernel's
    predicate (etm_heads_loss_supported_gaussian); there is no torch-autograd fallback.  None when the config is not a Box."""
    if A is None:
        A = config.get("environment", {}).get("continuous_actions")
        if A is None:
            return None
    A, hid = int(A), int(config["hidden_layer_size"])
    if not 1 <= A <= 8:
        raise ValueError(f"Box action space of {A} dimensions: the fused Gaussian heads + loss kernel takes 1 to 8")
    if not etm_lib.load().etm_heads_loss_supported_gaussian(1, hid, A):
        raise ValueError(f"Box action space with hidden_layer_size={hid}: the fused Gaussian heads + loss kernel needs a multiple of 64, "
                         "at most 512")
    return A


def check_byte_observation_transport(config, env=None):
    """``worker_processes: true`` with ``observation_dtype: uint8`` is refused, before any environment or process is created: the
    workers' shared segment types its observation rows as float32 (environments/shm_env.py)."""
    env_cfg = config["environment"]
    as_bytes = str(env_cfg.get("observation_dtype", "float32")) == "uint8" or is_byte_only(env_cfg.get("type"))      # (types with no float form)
    if env is None and config.get("worker_processes", False) and as_bytes:
        raise ValueError("worker_processes: true does not carry uint8 observations (the shared segment's rows are float32): "
                         "set worker_processes: false (in-process environments keep the bytes), or let the environment emit float32")


def check_truncation_transport(config, env=None):
    """``worker_processes: true`` with ``bootstrap_truncated: true`` is refused, before any environment or process is created: the
    workers' shared segment has no row for a final observation (environments/shm_env.py; a worker resets in place)."""
    if env is None and config.get("worker_processes", False) and config.get("bootstrap_truncated", False):
        raise ValueError("worker_processes: true does not carry bootstrap_truncated: true (the shared segment has no row for a final "
                         "observation): set worker_processes: false (in-process environments hand it over in their info), or leave "
                         "bootstrap_truncated off")


def check_action_mask_config(config, env=None, action_space_shape=None, box=False):
    """The optional key ``action_masks: true`` (invalid-action masking: one 64-bit word per worker and step, bit j = column j of the
    concatenated policy head is allowed).  -> whether it is on; absent or false: nothing is allocated, no launch is added or exchanged.
    Refused, each before anything is built from it: a Box policy (``environment.continuous_actions``, or ``box`` once the environment
    is known); more than 63 actions over all branches (``action_space_shape``, or a Synthetic environment's ``num_actions``);
    ``worker_processes: true`` without a supplied ``env`` (the workers' shared segment has no row for a mask word, as for
    ``bootstrap_truncated``); an environment front-end without ``action_masks`` (``env``, once it exists).  Data-parallel runs need
    nothing: the masks are per-rank data."""
    if not config.get("action_masks", False):
        return False
    from environments import MAX_MASKED_ACTIONS
    env_cfg = config.get("environment", {})
    if box or env_cfg.get("continuous_actions") is not None:
        raise ValueError("action_masks: true with a Box (continuous) action space: a Gaussian policy has no invalid actions to mask; "
                         "remove the key (the environment's bounds already clip the actions)")
    shape = action_space_shape
    if shape is None and env_cfg.get("type") == "Synthetic" and "num_actions" in env_cfg:
        n = env_cfg["num_actions"]
        shape = tuple(n) if isinstance(n, (list, tuple)) else (int(n),)
    if shape is not None and sum(int(a) for a in shape) > MAX_MASKED_ACTIONS:
        raise ValueError(f"action_masks: true with {sum(int(a) for a in shape)} actions over all branches: a step's mask is one 64-bit word "
                         f"per worker and takes at most {MAX_MASKED_ACTIONS}; remove the key, or reduce the action space")
    if env is None and config.get("worker_processes", False):
        raise ValueError("worker_processes: true does not carry action_masks: true (the shared segment has no row for a mask word): "
                         "set worker_processes: false (in-process environments hand the words over each step), or remove the key")
    if env is not None and not callable(getattr(env, "action_masks", None)):
        raise ValueError(f"action_masks: true, but the environment front-end {type(env).__name__} has no action_masks(): let the "
                         "environments offer action_masks() (environments/vec_env.py: the VecEnv protocol; a Synthetic environment needs "
                         "environment.action_mask_p), or remove the key")
    return True


def check_evaluation_config(config, world: int = 1):
    """The optional ``evaluation`` section (interval, episodes_per_worker, n_workers, deterministic, seed, worker_steps) -> a dict with
    the defaults filled in, or None when the section is absent (never evaluate, allocate nothing).  ``evaluation.interval`` in a
    data-parallel run (``world`` > 1) is refused, before any environment is built: every rank would have to take part in the same
    evaluation -- evaluate the checkpoint with evaluate.py instead."""
    ev = config.get("evaluation")
    if ev is None:
        return None
    known = ("interval", "episodes_per_worker", "n_workers", "deterministic", "seed", "worker_steps")
    unknown = sorted(set(ev) - set(known))
    if unknown:
        raise ValueError(f"evaluation: unknown keys {unknown} (known: {list(known)})")
    out = dict(interval=int(ev.get("interval", 0) or 0), episodes_per_worker=int(ev.get("episodes_per_worker", 1)),
               n_workers=int(ev.get("n_workers", config["n_workers"])), deterministic=bool(ev.get("deterministic", True)),
               seed=int(ev.get("seed", 100000)), worker_steps=ev.get("worker_steps"))
    if out["interval"] < 0 or out["episodes_per_worker"] < 1 or out["n_workers"] < 1:
        raise ValueError("evaluation: interval >= 0, episodes_per_worker >= 1 and n_workers >= 1 are required")
    if out["interval"] > 0 and world > 1:
        raise ValueError("evaluation.interval in a data-parallel run: periodic evaluation runs on one rank's device only; "
                         "evaluate the checkpoint with evaluate.py instead")
    return out


def check_normalization_config(config, world: int = 1, observation_shape=None, observation_dtype=None):
    """The optional keys ``normalize_observations`` and ``normalize_rewards`` (each ``true`` or {clip, epsilon}) -> {"observations":
    section or None, "rewards": section or None} with the defaults filled in.  Refused, each before anything is allocated: unknown
    sub-keys, ``clip <= 0`` or ``epsilon <= 0`` (utils.normalization_section); either key in a data-parallel run (``world`` > 1: the
    ranks' statistics would have to be merged, which this build does not do); ``normalize_observations`` with image or uint8
    observations (``observation_shape`` / ``observation_dtype``, once the environment is known) or with more features than the
    statistics kernel takes."""
    out = {"observations": normalization_section(config, "normalize_observations"), "rewards": normalization_section(config, "normalize_rewards")}
    on = [k for k, key in (("normalize_observations", "observations"), ("normalize_rewards", "rewards")) if out[key] is not None]
    if on and world > 1:
        raise ValueError(f"{' / '.join(on)} in a data-parallel run: every rank would keep statistics of its own workers only (merging "
                         "them over the ranks is not built); remove the key(s), or train on one device")
    if out["observations"] is not None and observation_shape is not None:
        if len(tuple(observation_shape)) != 1 or observation_dtype == torch.uint8:
            raise ValueError(f"normalize_observations with image / uint8 observations of shape {tuple(observation_shape)}: they are already "
                             "in [0, 1] (byte k = k / 255); remove the key -- it is for float32 vector observations")
        if not ops.obs_stats_supported(int(observation_shape[0])):
            raise ValueError(f"normalize_observations with {int(observation_shape[0])} features: the statistics kernel takes 1 to 1024; "
                             "remove the key or reduce the observation")
    return out


def check_target_kl_config(config, world: int = 1):
    """The optional key ``target_kl`` (a number or {value, factor, host_check}; utils.target_kl_section) -> {"value", "factor",
    "host_check", "limit"} or None when the key is absent (nothing is allocated, no launch is added or exchanged).  Refused, each before
    anything is allocated: a value or factor that is no finite number > 0, unknown sub-keys, a ``host_check`` other than "epoch" /
    "none"; the key in a data-parallel run (``world`` > 1): every rank sees the KL of its own minibatch, and agreeing on one is not
    built."""
    out = target_kl_section(config)
    if out is not None and world > 1:
        raise ValueError("target_kl in a data-parallel run: every rank would stop on the KL of its own minibatch and the replicas would "
                         "part (agreeing on one KL over the ranks is not built); remove the key, or train on one device")
    return out


def check_adaptive_lr_config(config, world: int = 1):
    """The optional key ``adaptive_lr`` (a number: the desired KL, or {desired_kl, factor, low, high, min, max};
    utils.adaptive_lr_section) -> the rule with its float32 constants, or None when the key is absent (nothing is allocated, no launch
    is added or exchanged).  Refused, each before anything is allocated and each with what to do instead: values outside their ranges
    and unknown sub-keys (utils.adaptive_lr_section); a start value float32(learning_rate_schedule.initial) outside [min, max]; a
    ``learning_rate_schedule`` that decays (final != initial): two schedules would compete for one number; the key in a data-parallel
    run (``world`` > 1): every rank sees the KL of its own minibatch, and agreeing on one is not built."""
    out = adaptive_lr_section(config)
    if out is None:
        return None
    if world > 1:
        raise ValueError("adaptive_lr in a data-parallel run: every rank would move its learning rate on the KL of its own minibatch and "
                         "the replicas would part (agreeing on one KL over the ranks is not built); remove the key, or train on one device")
    sched = config["learning_rate_schedule"]
    if sched["final"] != sched["initial"]:
        raise ValueError(f"adaptive_lr with a decaying learning_rate_schedule (initial {sched['initial']!r}, final {sched['final']!r}): the "
                         "two schedules compete for one learning rate; set learning_rate_schedule.final to initial (it is the start value "
                         "only), or remove the key adaptive_lr")
    start = float(np.float32(sched["initial"]))
    if not out["min"] <= start <= out["max"]:
        raise ValueError(f"adaptive_lr: the start value float32(learning_rate_schedule.initial) = {start!r} lies outside [min, max] = "
                         f"[{out['min']!r}, {out['max']!r}]; move initial into the range, or widen adaptive_lr.min / adaptive_lr.max")
    return out


def check_kl_estimator_config(config, box: bool = False, world: int = 1):
    """The optional key ``kl_estimator`` (utils.kl_estimator_section) -> "k3" (absent: nothing is allocated, no launch is added or
    exchanged) or "analytic": the statistic ``kl`` -- what ``other/kl`` shows and what ``target_kl`` and ``adaptive_lr`` decide on -- is
    the exact KL of the rollout's and the current Gaussian of a Box policy instead of the sample estimate.  Refused, each before
    anything is built and each with what to do instead: a value other than ``k3`` / ``analytic``; ``analytic`` without a Box policy
    (``box``: a categorical policy's exact KL would need every old logit stored); ``analytic`` in a data-parallel run (``world`` > 1),
    as for the other KL keys."""
    kind = kl_estimator_section(config)
    if kind != "analytic":
        return kind
    if not box:
        raise ValueError("kl_estimator: analytic without a Box (continuous) action space: the exact KL is built for diagonal Gaussian "
                         "policies only (a categorical policy's would need every old logit stored); categorical policies keep k3: "
                         "remove the key, or replace it with `exact_kl: true` (the exact KL of every policy kind)")
    if world > 1:
        raise ValueError("kl_estimator: analytic in a data-parallel run: every rank would see the KL of its own minibatch (agreeing on one "
                         "KL over the ranks is not built); remove the key, or train on one device")
    return kind


def check_exact_kl_config(config, box: bool = False, world: int = 1) -> bool:
    """The optional key ``exact_kl`` (utils.exact_kl_section) -> False (absent or ``false``: nothing is allocated, no launch is added
    or exchanged) or True: the statistic ``kl`` -- what ``other/kl`` shows and what ``target_kl`` and ``adaptive_lr`` decide on -- is the
    exact KL(old || new) of the rollout's and the current policy for EVERY policy kind.  For a Box policy (``box``) that is exactly
    ``kl_estimator: analytic``; for Discrete and MultiDiscrete policies, masked or not, the four categorical sampling sites stage
    every column's log-prob and the loss kernels reduce ``utils.categorical_kl``.  Refused, each before anything is built and each
    with what to do instead: a value that is no bool; ``exact_kl: true`` next to an explicit ``kl_estimator: k3`` (they contradict
    each other); the key in a data-parallel run (``world`` > 1), as for the other KL keys."""
    on = exact_kl_section(config)
    if not on:
        return False
    if "kl_estimator" in config and kl_estimator_section(config) == "k3":
        raise ValueError("exact_kl: true next to kl_estimator: k3: the two keys contradict each other (k3 is the sample estimate); "
                         "remove kl_estimator for the exact KL, or remove exact_kl to keep the sample estimate")
    if world > 1:
        raise ValueError("exact_kl: true in a data-parallel run: every rank would see the KL of its own minibatch (agreeing on one "
                         "KL over the ranks is not built); remove the key, or train on one device")
    return True


def check_kl_penalty_config(config, world: int = 1):
    """The optional key ``kl_penalty`` (a number: a fixed coefficient, or {coef, target, high, low, up, down, min, max};
    utils.kl_penalty_section) -> the section with its float32 constants, or None when the key is absent (nothing is allocated, no launch
    is added or exchanged).  With the key the loss is L + coef * KL(old || new), the exact KL that ``exact_kl: true`` reports -- the key
    implies that plumbing for every policy kind -- and with ``target`` the coefficient adapts once per update (utils.kl_penalty_step).
    Refused, each before anything is built and each with what to do instead: what utils.kl_penalty_section refuses; an explicit
    ``exact_kl: false`` or ``kl_estimator: k3`` next to the key (they contradict it); the key in a data-parallel run (``world`` > 1),
    as for the other KL keys."""
    out = kl_penalty_section(config)
    if out is None:
        return None
    if "exact_kl" in config and not exact_kl_section(config):
        raise ValueError("kl_penalty next to exact_kl: false: the two keys contradict each other (the penalty is a term in the exact KL "
                         "and switches its plumbing on); remove exact_kl, or remove kl_penalty to train without the penalty")
    if "kl_estimator" in config and kl_estimator_section(config) == "k3":
        raise ValueError("kl_penalty next to kl_estimator: k3: the two keys contradict each other (the penalty is a term in the exact KL, "
                         "k3 is the sample estimate); remove kl_estimator, or remove kl_penalty to train without the penalty")
    if world > 1:
        raise ValueError("kl_penalty in a data-parallel run: every rank would penalise and adapt on the KL of its own minibatches "
                         "(agreeing on one KL over the ranks is not built); remove the key, or train on one device")
    return out


def check_attention_statistics_config(config, world: int = 1) -> bool:
    """The optional key ``attention_statistics`` (utils.attention_statistics_section) -> False (absent or ``false``: nothing is
    allocated, launched or changed) or True: every grad-enabled forward pass of an update adds its attention probabilities to a
    per-block, per-head table (etm_attn_stats), read once per update into ``last_attention_statistics``.  Refused, each before
    anything is built and each with what to do instead: a value that is no bool; the key in a data-parallel run (``world`` > 1):
    every rank sees its own minibatches, and merging the ranks' tables is not built."""
    on = attention_statistics_section(config)
    if on and world > 1:
        raise ValueError("attention_statistics: true in a data-parallel run: every rank would count the attention of its own minibatches "
                         "only (merging the tables over the ranks is not built); remove the key, or train on one device")
    return on


# the keys that decide on the KL's plumbing: a context that never forms a loss (evaluation.evaluation_config) drops exactly these
KL_KEYS = ("kl_estimator", "exact_kl", "kl_penalty")


def kl_plumbing(config, continuous: bool):
    """Who stages what for the exact KL -> (kl_analytic, kl_exact_cat), the one statement of the rule for the trainer (staging tables,
    sampling entries, loss entries) and the buffer (fields).  ``exact_kl: true`` and ``kl_penalty`` (it is a term in that very number)
    ask for the exact KL of whatever policy there is.  A Box policy's (``continuous``) is ``kl_estimator: analytic``: the rollout's
    means and a snapshot of the log-std.  A categorical policy's needs every column's log-prob of the rollout.  The values are not
    checked here (the ``check_*_config`` functions do that; ``Buffer`` refuses ``analytic`` without a Box itself)."""
    exact = exact_kl_section(config) or kl_penalty_section(config) is not None
    analytic = kl_estimator_section(config) == "analytic" or (exact and bool(continuous))
    return analytic, exact and not continuous


@dataclass(frozen=True)
class RunSettings:
    """What the optional keys of ``config`` come to for one trainer (module docstring: the two stages and their refusal order)."""
    config: dict
    world: int                          # data-parallel ranks
    worker_processes: bool              # the environments live in worker processes (never with a supplied environment)
    target_kl: dict = None              # check_target_kl_config
    adaptive_lr: dict = None            # check_adaptive_lr_config
    kl_penalty: dict = None             # check_kl_penalty_config
    attention_statistics: bool = False
    evaluation: dict = None             # check_evaluation_config: the section with its defaults, None without it
    checkpoint_interval: int = None
    # known with the environment
    normalization: dict = None          # check_normalization_config: {"observations", "rewards"}
    masked: bool = None
    prev: dict = None                   # previous_step_input: {"action", "reward"} or None
    kl_analytic: bool = None            # kl_plumbing
    kl_exact_cat: bool = None
    recon: dict = None                  # obs_reconstruction: the coefficient's schedule or None

    @classmethod
    def before_environment(cls, config: dict, world: int = 1, env=None, resume: bool = False):
        """Stage one.  ``env``: a supplied environment or None; ``resume``: whether the run continues from a checkpoint."""
        worker_processes = bool(env is None and config.get("worker_processes", False))
        check_kernel_shapes(config["transformer"])
        declared_box = check_box_policy(config) is not None
        check_byte_observation_transport(config, env)
        check_truncation_transport(config, env)
        if env is None:       # environment.device: true (a device-resident type) against the transports and the world size
            check_device_env_config(config, world)
        check_action_mask_config(config, env)
        # previous_step_input: the value itself and the transport (the shared segment of the worker processes has no row for the last
        # reward); the action space is looked at in stage two
        previous_step_input_section(config, worker_processes=worker_processes)
        evaluation = check_evaluation_config(config, world)
        check_normalization_config(config, world)
        checkpoint_interval = check_checkpoint_config(config, world, resume=resume)
        target_kl = check_target_kl_config(config, world)
        adaptive_lr = check_adaptive_lr_config(config, world)
        # (a supplied environment says what the policy is in stage two; else the config does, before anything is built)
        check_kl_estimator_config(config, env is not None or declared_box, world)
        check_exact_kl_config(config, declared_box, world)
        kl_penalty = check_kl_penalty_config(config, world)
        obs_reconstruction_section(config, world=world)      # (the value; the observation's shape in stage two)
        attention_statistics = check_attention_statistics_config(config, world)
        return cls(config=config, world=world, worker_processes=worker_processes, target_kl=target_kl, adaptive_lr=adaptive_lr,
                   kl_penalty=kl_penalty, attention_statistics=attention_statistics, evaluation=evaluation,
                   checkpoint_interval=checkpoint_interval)

    def with_environment(self, env, observation_shape, observation_dtype, action_space_shape, box):
        """Stage two.  ``box``: the environment's ``ActionKind`` when it is a Box, else None."""
        config, world, continuous = self.config, self.world, box is not None
        if observation_dtype == torch.uint8 and len(observation_shape) < 2:
            raise ValueError("uint8 observations are images (byte k = k / 255); a vector observation must be float32")
        normalization = check_normalization_config(config, world, observation_shape, observation_dtype)
        if continuous:
            check_box_policy(config, box.shape[0])
        masked = check_action_mask_config(config, env, action_space_shape, continuous)
        prev = previous_step_input_section(config, action_space_shape, box=continuous)
        check_kl_estimator_config(config, continuous, world)
        kl_analytic, kl_exact_cat = kl_plumbing(config, continuous)
        recon = obs_reconstruction_section(config, observation_shape, world)
        return replace(self, normalization=normalization, masked=masked, prev=prev, kl_analytic=kl_analytic, kl_exact_cat=kl_exact_cat,
                       recon=recon)
