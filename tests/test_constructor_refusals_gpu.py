"""-m gpu: what ``PPOTrainer(...)`` refuses, in which order, and what it binds -- through the constructor itself.

A. The refusal order (run_settings.py states it as a numbered list).  Every case raises before anything is built: ``make_vec_env``,
   ``ShmVecEnv``, ``Buffer`` and ``ActorCriticModel`` are replaced by functions that fail the test.  Two walks peel one fault at a time
   off a single config -- a data-parallel one (every optional key on, ``world`` 2) and a single-device one (shape, Box, the worker
   processes' transports, masks, previous step, evaluation) --, a non-HIP device is refused before any of them, and with a supplied
   stub environment the checks that need the environment give the refusal of the first broken thing.
C. Four tiny trainers (4 workers, 16 steps, embed_dim 64) bind the attributes that bench.py, the tests and the tools read with the
   values recorded from the commit before run_settings.py existed, written here as literals (``host_cpu_plan: false`` pins the host
   plan; its ``budget`` and ``busy_threads`` describe the machine and are left out)."""
import copy
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


class _Built(Exception):
    """Construction went past the checks and started to build something."""


def _boom(*args, **kwargs):
    raise _Built()


@pytest.fixture
def nothing_built(monkeypatch):
    import trainer
    from environments import shm_env
    monkeypatch.setattr(trainer, "make_vec_env", _boom)
    monkeypatch.setattr(shm_env, "ShmVecEnv", _boom)
    monkeypatch.setattr(trainer, "Buffer", _boom)
    monkeypatch.setattr(trainer, "ActorCriticModel", _boom)


def _base(**over):
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[4], num_actions=3, max_episode_steps=16, seed=0, p_done=0.05, pool=8),
               gamma=0.99, lamda=0.95, updates=1, epochs=2, n_workers=4, worker_steps=16, n_mini_batch=2, value_loss_coefficient=0.5,
               hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False, host_cpu_plan=False,
               transformer=dict(num_blocks=2, embed_dim=64, num_heads=2, memory_length=8, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    cfg.update(over)
    return cfg


def _construct(cfg, **kw):
    from trainer import PPOTrainer
    return PPOTrainer(copy.deepcopy(cfg), run_id="refusals", device=kw.pop("device", DEV), tensorboard=False, **kw)


def _refused(cfg, message, **kw):
    with pytest.raises(ValueError) as exc:
        _construct(cfg, **kw)
    assert str(exc.value).startswith(message), str(exc.value)


# ------------------------------------------------------------------ A: the data-parallel walk
def data_parallel_config():
    cfg = _base(evaluation=dict(interval=2), normalize_observations=True, normalize_rewards=True, checkpoint_interval=1, target_kl=0.02,
                adaptive_lr=0.01, kl_estimator="analytic", exact_kl=True, kl_penalty=0.5, obs_reconstruction=0.1, attention_statistics=True)
    cfg["environment"] = dict(cfg["environment"], continuous_actions=2)
    del cfg["environment"]["num_actions"]
    return cfg


# (keys removed before the case, the refusal that must come next)
DATA_PARALLEL_WALK = (
    ((), "evaluation.interval in a data-parallel run"),
    (("evaluation",), "normalize_observations / normalize_rewards in a data-parallel run"),
    (("normalize_observations", "normalize_rewards"), "checkpoint_interval in a data-parallel run"),
    (("checkpoint_interval",), "target_kl in a data-parallel run"),
    (("target_kl",), "adaptive_lr in a data-parallel run"),
    (("adaptive_lr",), "kl_estimator: analytic in a data-parallel run"),
    (("kl_estimator",), "exact_kl: true in a data-parallel run"),
    (("exact_kl",), "kl_penalty in a data-parallel run"),
    (("kl_penalty",), "obs_reconstruction in a data-parallel run"),
    (("obs_reconstruction",), "attention_statistics: true in a data-parallel run"),
)


def test_data_parallel_walk(nothing_built):
    cfg, dp = data_parallel_config(), types.SimpleNamespace(world=2, rank=0)
    for removed, message in DATA_PARALLEL_WALK:
        for key in removed:
            del cfg[key]
        _refused(cfg, message, dp=dp)
    del cfg["attention_statistics"]
    with pytest.raises(_Built):         # (past the settings: the environment is the next thing built)
        _construct(cfg, dp=dp)


# ------------------------------------------------------------------ A: the single-device walk
def single_device_config():
    cfg = _base(worker_processes=True, bootstrap_truncated=True, action_masks=True, previous_step_input=dict(action=False, reward=False),
                evaluation=dict(foo=1))
    cfg["transformer"]["embed_dim"] = 48
    cfg["environment"] = dict(cfg["environment"], continuous_actions=9, observation_dtype="uint8")
    return cfg


def _set(path, value):
    def fix(cfg):
        node = cfg
        for k in path[:-1]:
            node = node[k]
        if value is _set:
            del node[path[-1]]
        else:
            node[path[-1]] = value
    return fix


# (the refusal the config gives, the fix applied after it)
SINGLE_DEVICE_WALK = (
    ("transformer shape not supported by the MI355X kernels: embed_dim=48", _set(("transformer", "embed_dim"), 64)),
    ("Box action space of 9 dimensions", _set(("environment", "continuous_actions"), 2)),
    ("worker_processes: true does not carry uint8 observations", _set(("environment", "observation_dtype"), _set)),
    ("worker_processes: true does not carry bootstrap_truncated: true", _set(("bootstrap_truncated",), _set)),
    ("action_masks: true with a Box (continuous) action space", _set(("environment", "continuous_actions"), _set)),
    ("worker_processes: true does not carry action_masks: true", _set(("action_masks",), _set)),
    ("previous_step_input: both `action` and `reward` are false", _set(("previous_step_input",), True)),
    ("worker_processes: true does not carry previous_step_input", _set(("worker_processes",), False)),
    ("evaluation: unknown keys ['foo']", _set(("evaluation",), _set)),
)


def test_single_device_walk(nothing_built):
    cfg = single_device_config()
    with pytest.raises(RuntimeError, match="needs an MI355X"):      # (a non-HIP device: before any of the config's faults)
        _construct(cfg, device=torch.device("cpu"))
    for message, fix in SINGLE_DEVICE_WALK:
        _refused(cfg, message)
        fix(cfg)
    with pytest.raises(_Built):
        _construct(cfg)


# ------------------------------------------------------------------ A: stage two, on a supplied stub environment
class _StubEnv:
    """What the constructor reads of an environment front-end before it builds anything; stepping it fails the test."""
    max_episode_steps = 16

    def __init__(self, obs_shape=(4,), dtype=np.float32, actions=(3,), box=None):
        from environments import ActionKind
        self.observation_space_shape, self.observation_dtype = tuple(obs_shape), np.dtype(dtype)
        self.action_space_shape = (box,) if box else tuple(actions)
        self.action_kind = ActionKind("box", (box,), -np.ones(box, np.float32), np.ones(box, np.float32)) if box else \
            ActionKind("discrete" if len(actions) == 1 else "multidiscrete", actions)

    reset = step = close = _boom


STAGE_TWO = {
    "uint8 vector observations": (dict(), dict(dtype=np.uint8), "uint8 observations are images"),
    "normalize_observations on images": (dict(normalize_observations=True), dict(obs_shape=(3, 84, 84)),
                                         "normalize_observations with image / uint8 observations of shape (3, 84, 84)"),
    "a Box of 9 dimensions": (dict(), dict(box=9), "Box action space of 9 dimensions"),
    "no action_masks()": (dict(action_masks=True), dict(), "action_masks: true, but the environment front-end _StubEnv has no action_masks()"),
    "analytic, categorical": (dict(kl_estimator="analytic"), dict(), "kl_estimator: analytic without a Box (continuous) action space"),
    "reconstruction of a vector": (dict(obs_reconstruction=0.1), dict(), "obs_reconstruction is for image observations [C, H, W]"),
    # two broken things: the earlier one
    "uint8 vector + analytic": (dict(kl_estimator="analytic"), dict(dtype=np.uint8), "uint8 observations are images"),
    "images normalised + Box 9": (dict(normalize_observations=True), dict(obs_shape=(3, 84, 84), box=9),
                                  "normalize_observations with image / uint8 observations"),
    "no action_masks() + reconstruction": (dict(action_masks=True, obs_reconstruction=0.1), dict(), "action_masks: true, but the environment"),
    "analytic + reconstruction": (dict(kl_estimator="analytic", obs_reconstruction=0.1), dict(), "kl_estimator: analytic without a Box"),
}


@pytest.mark.parametrize("case", sorted(STAGE_TWO))
def test_stage_two(nothing_built, case):
    keys, stub, message = STAGE_TWO[case]
    _refused(_base(**keys), message, env=_StubEnv(**stub))


# ------------------------------------------------------------------ C: the trainer still binds what it bound
def _image_env(**over):
    return dict(dict(type="Synthetic", obs_shape=[3, 84, 84], num_actions=3, max_episode_steps=16, seed=0, p_done=0.05, pool=8), **over)


BOUND_CONFIGS = {
    "discrete": lambda: _base(),
    "masked multidiscrete, exact_kl": lambda: _base(environment=_image_env(num_actions=[3, 2], action_mask_p=0.3), action_masks=True,
                                                    exact_kl=True),
    "box, kl_penalty": lambda: _base(environment=dict(type="Synthetic", obs_shape=[4], continuous_actions=2, max_episode_steps=16, seed=0,
                                                      p_done=0.05, pool=8), kl_penalty=0.5),
    "image, reconstruction, previous step, truncation": lambda: _base(
        environment=_image_env(observation_levels=256, observation_dtype="uint8"), obs_reconstruction=0.1, previous_step_input=True,
        bootstrap_truncated=True),
}

HOST_PLAN_KEYS = ("copy_threads", "copier_spin", "polite_wait", "envs_per_process", "worker_spin", "reason")


def bound(tr):
    """The attributes a reader outside the trainer relies on, as plain Python values."""
    return {"_masked": tr._masked, "_kl_analytic": tr._kl_analytic, "_kl_exact_cat": tr._kl_exact_cat, "_prev_cfg": tr._prev_cfg,
            "_kl_pen": tr._kl_pen, "_kl_cfg": tr._kl_cfg, "_recon": tr._recon, "_host_plan": {k: tr._host_plan[k] for k in HOST_PLAN_KEYS},
            "_env_cfg": tr._env_cfg, "_env_groups": tr._env_groups, "_bootstrap": tr._bootstrap, "_stage": sorted(tr._stage),
            "samples_flat": sorted(tr.buffer.samples_flat)}


_PLAN = {"copy_threads": 1, "copier_spin": True, "polite_wait": False, "envs_per_process": 1, "worker_spin": True,
         "reason": "host_cpu_plan: false"}
_STAGE = ["actions", "log_probs", "memory_indices", "memory_mask", "obs", "values"]
_FLAT = ["actions", "advantages", "log_probs", "memory_index", "memory_indices", "memory_mask", "obs", "values"]
_OFF = {"_masked": False, "_kl_analytic": False, "_kl_exact_cat": False, "_prev_cfg": None, "_kl_pen": None, "_kl_cfg": None, "_recon": None,
        "_host_plan": _PLAN, "_env_groups": 1, "_bootstrap": False, "_stage": _STAGE, "samples_flat": _FLAT}
# recorded from the parent commit's trainers on the MI355X
EXPECTED = {
    "discrete": dict(_OFF, _env_cfg={"type": "Synthetic", "obs_shape": [4], "num_actions": 3, "max_episode_steps": 16, "seed": 0, "p_done": 0.05,
                                     "pool": 8}),
    "masked multidiscrete, exact_kl": dict(
        _OFF, _masked=True, _kl_exact_cat=True, _stage=sorted(_STAGE + ["logps"]), samples_flat=sorted(_FLAT + ["action_masks", "old_logps"]),
        _env_cfg={"type": "Synthetic", "obs_shape": [3, 84, 84], "num_actions": [3, 2], "max_episode_steps": 16, "seed": 0, "p_done": 0.05,
                  "pool": 8, "action_mask_p": 0.3}),
    "box, kl_penalty": dict(
        _OFF, _kl_analytic=True, _stage=sorted(_STAGE + ["means"]), samples_flat=sorted(_FLAT + ["means"]),
        _kl_pen={"coef": 0.5, "adaptive": False, "target": None, "kl_high": None, "kl_low": None, "high": None, "low": None, "up": None,
                 "down": None, "min": None, "max": None},
        _env_cfg={"type": "Synthetic", "obs_shape": [4], "continuous_actions": 2, "max_episode_steps": 16, "seed": 0, "p_done": 0.05, "pool": 8}),
    "image, reconstruction, previous step, truncation": dict(
        _OFF, _prev_cfg={"action": True, "reward": True}, _bootstrap=True, samples_flat=sorted(_FLAT + ["prev_actions", "prev_rewards"]),
        _recon={"initial": 0.1, "final": 0.1, "power": 1.0, "max_decay_steps": 0.0},
        _env_cfg={"type": "Synthetic", "obs_shape": [3, 84, 84], "num_actions": 3, "max_episode_steps": 16, "seed": 0, "p_done": 0.05, "pool": 8,
                  "observation_levels": 256, "observation_dtype": "uint8"}),
}


@pytest.mark.parametrize("name", sorted(BOUND_CONFIGS))
def test_trainer_binds_what_it_bound(name):
    torch.manual_seed(0)
    tr = _construct(BOUND_CONFIGS[name]())
    try:
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()          # (samples_flat exists from here on)
        got = bound(tr)
    finally:
        tr.close()
    assert got == EXPECTED[name], got
