"""Helpers with the upstream names (utils.py): create_env, polynomial_decay, batched_index_select,
process_episode_info, Module; normalization_section reads this build's two normalisation keys, target_kl_section its KL early
stop, target_kl_rows says which rows of an update's result tables a stopped update returns; adaptive_lr_section reads the
KL-adaptive learning rate and adaptive_lr_step is its rule, the one host definition of what the norm kernel decides;
kl_estimator_section reads which KL both rules see and gaussian_kl is the exact KL of a Box policy's Gaussians, the one host
definition of what the Gaussian heads + loss kernel reduces; exact_kl_section reads the key that switches the exact KL on for every
policy kind and categorical_kl is the exact KL of Discrete / MultiDiscrete policies, the one host definition of what the categorical
loss kernels reduce."""
import numpy as np
import torch
from torch import nn


def create_env(config: dict, render: bool = False, worker_id: int = 0):
    """One environment instance for ``config["type"]`` (upstream utils.py:10-30).

    "Synthetic" is this build's workload generator (environments/synthetic.py).  The simulator-backed types need
    third-party packages that are not part of this build; they raise a clear ImportError when absent.
    """
    kind = config["type"]
    if kind == "Synthetic":
        from environments.synthetic import SyntheticEnv
        keys = ("obs_shape", "num_actions", "max_episode_steps", "seed", "p_reward", "p_done", "pool", "continuous_actions", "action_low",
                "action_high", "observation_levels", "observation_dtype")
        kw = {k: config[k] for k in keys if k in config}
        if "obs_shape" in kw:
            kw["obs_shape"] = tuple(kw["obs_shape"])
        return SyntheticEnv(worker_id=worker_id, **kw)
    if kind == "PocMemoryEnv":
        from environments.poc_memory_env import PocMemoryEnv
        # ``environment.seed`` (optional): worker w draws from its own stream seed + w, so a run -- and an evaluation, whose
        # workers start at another id -- can be repeated; absent: unseeded, as ever
        seed = int(config["seed"]) + int(worker_id) if config.get("seed") is not None else None
        # ``environment.report_truncation`` (optional): time-limit cuts carry "truncated": True in their info (bootstrap_truncated)
        return PocMemoryEnv(glob=False, freeze=True, max_episode_steps=32, seed=seed,
                            report_truncation=bool(config.get("report_truncation", False)))
    raise ImportError(f"environment type {kind!r} needs its simulator package (gym / gym-minigrid / memory-gym), which is "
                      "outside this build; use type 'Synthetic' with the same observation shape for throughput runs")


def polynomial_decay(initial: float, final: float, max_decay_steps: int, power: float, current_step: int) -> float:
    """Polynomial schedule; ``final`` once current_step exceeds max_decay_steps (strictly) or if nothing decays."""
    if current_step > max_decay_steps or initial == final:
        return final
    frac = 1 - current_step / max_decay_steps
    return (initial - final) * (frac ** power) + final


def batched_index_select(input, dim, index):
    """input [B, ...], index [B, K] -> input gathered along ``dim`` per batch row: [B, K, ...] for dim == 1.

    Kept for API compatibility; the trainer itself never materialises windows (the kernels gather in place)."""
    view = [index.shape[0]] + [1] * (input.dim() - 1)
    view[dim] = index.shape[1]
    expand = list(input.shape)
    expand[dim] = index.shape[1]
    return torch.gather(input, dim, index.reshape(view).expand(expand))


def process_episode_info(episode_info: list) -> dict:
    """mean/std per key of the finished-episode dicts (plus ``success_percent``)."""
    result = {}
    if not episode_info:
        return result
    for key in episode_info[0].keys():
        vals = [info[key] for info in episode_info]
        if key == "success":
            result[key + "_percent"] = np.sum(vals) / len(vals)
        result[key + "_mean"] = np.mean(vals)
        result[key + "_std"] = np.std(vals)
    return result


def normalization_section(config: dict, key: str):
    """The optional section ``key`` (``normalize_observations`` / ``normalize_rewards``) of ``config`` -> {"clip", "epsilon"} with the
    defaults (10, 1e-8) filled in, or None when the key is absent or false.  ``true`` stands for the defaults."""
    sec = config.get(key)
    if sec is None or sec is False:
        return None
    if sec is True:
        sec = {}
    if not isinstance(sec, dict):
        raise ValueError(f"{key}: expected true or a section with clip / epsilon, got {sec!r}")
    unknown = sorted(set(sec) - {"clip", "epsilon"})
    if unknown:
        raise ValueError(f"{key}: unknown keys {unknown} (known: ['clip', 'epsilon']); remove them")
    out = dict(clip=float(sec.get("clip", 10.0)), epsilon=float(sec.get("epsilon", 1.0e-8)))
    if not out["clip"] > 0 or not np.isfinite(out["clip"]):
        raise ValueError(f"{key}.clip must be a positive number, got {sec.get('clip')!r}; leave it out for the default 10")
    if not out["epsilon"] > 0 or not np.isfinite(out["epsilon"]):
        raise ValueError(f"{key}.epsilon must be a positive number, got {sec.get('epsilon')!r}; leave it out for the default 1e-8")
    return out


def _positive_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and bool(np.isfinite(x)) and x > 0


def target_kl_section(config: dict):
    """The optional key ``target_kl`` (a number, or {value, factor, host_check}) -> {"value", "factor", "host_check", "limit"} with the
    defaults (factor 1.5, stable-baselines3's rule; host_check "epoch") filled in, or None when the key is absent.  ``limit`` is
    float32(factor * value): the product is formed once in double and rounded once."""
    sec = config.get("target_kl")
    if sec is None:
        return None
    if not isinstance(sec, dict):
        sec = {"value": sec}
    known = ("value", "factor", "host_check")
    unknown = sorted(set(sec) - set(known))
    if unknown:
        raise ValueError(f"target_kl: unknown keys {unknown} (known: {list(known)}); remove them")
    if "value" not in sec:
        raise ValueError("target_kl: the section needs `value` (the target KL, e.g. 0.02); add it, or remove the key to train without the stop")
    value, factor, host_check = sec["value"], sec.get("factor", 1.5), sec.get("host_check", "epoch")
    if not _positive_number(value):
        raise ValueError(f"target_kl.value must be a finite number > 0, got {value!r}; remove the key to train without the stop")
    if not _positive_number(factor):
        raise ValueError(f"target_kl.factor must be a finite number > 0, got {factor!r}; leave it out for the default 1.5")
    if host_check not in ("epoch", "none"):
        raise ValueError(f"target_kl.host_check must be 'epoch' or 'none', got {host_check!r}; leave it out for the default 'epoch'")
    return dict(value=float(value), factor=float(factor), host_check=host_check, limit=float(np.float32(float(factor) * float(value))))


def target_kl_rows(stopped: bool, steps_applied: int, steps_launched: int) -> int:
    """How many leading rows of an update's statistics / norm tables are returned: all launched ones, or -- stopped -- rows
    0 ... steps_applied, the stopping row included (its loss statistics are real: the loss on the weights the update ends with).
    Never 0."""
    rows = min(int(steps_applied) + 1, int(steps_launched)) if stopped else int(steps_launched)
    return max(rows, 1)


ADAPTIVE_LR_DEFAULTS = dict(factor=1.5, low=0.5, high=2.0, min=1.0e-5, max=1.0e-2)


def _finite_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and bool(np.isfinite(x))


def _f32(x):
    with np.errstate(over="ignore"):            # (a value beyond float32's range becomes inf, and is refused as such)
        return np.float32(x)


def adaptive_lr_section(config: dict):
    """The optional key ``adaptive_lr`` (a number: the desired KL, or {desired_kl, factor, low, high, min, max}) -> {"desired_kl",
    "factor", "low", "high", "min", "max", "kl_low", "kl_high"} with the defaults (factor 1.5, low 0.5, high 2.0, the band and the
    factor of rsl_rl; min 1e-5, max 1e-2) filled in, or None when the key is absent.  ``kl_low`` = float32(desired_kl * low) and
    ``kl_high`` = float32(desired_kl * high), each product formed once in double and rounded once; ``factor``, ``min`` and ``max`` are
    each rounded to float32.  Every value returned is a python float that holds a float32 exactly, but ``desired_kl``, ``low`` and
    ``high``, which stay as given."""
    sec = config.get("adaptive_lr")
    if sec is None:
        return None
    if not isinstance(sec, dict):
        sec = {"desired_kl": sec}
    known = ("desired_kl", "factor", "low", "high", "min", "max")
    unknown = sorted(set(sec) - set(known))
    if unknown:
        raise ValueError(f"adaptive_lr: unknown keys {unknown} (known: {list(known)}); remove them")
    if "desired_kl" not in sec:
        raise ValueError("adaptive_lr: the section needs `desired_kl` (the KL the learning rate is steered to, e.g. 0.01); add it, or remove "
                         "the key to train with learning_rate_schedule alone")
    desired = sec["desired_kl"]
    if not _positive_number(desired):
        raise ValueError(f"adaptive_lr.desired_kl must be a finite number > 0, got {desired!r}; remove the key to train with "
                         "learning_rate_schedule alone")
    v = {k: sec.get(k, d) for k, d in ADAPTIVE_LR_DEFAULTS.items()}
    if not _finite_number(v["factor"]) or not _f32(v["factor"]) > 1 or not np.isfinite(_f32(v["factor"])):
        raise ValueError(f"adaptive_lr.factor must be a finite number > 1 (also as a float32), got {v['factor']!r}; leave it out for the "
                         "default 1.5")
    if not _finite_number(v["low"]) or not v["low"] >= 0:
        raise ValueError(f"adaptive_lr.low must be a finite number >= 0 (the learning rate rises below low * desired_kl; 0: never), got "
                         f"{v['low']!r}; leave it out for the default 0.5")
    if not _positive_number(v["high"]):
        raise ValueError(f"adaptive_lr.high must be a finite number > 0 (the learning rate falls above high * desired_kl), got "
                         f"{v['high']!r}; leave it out for the default 2.0")
    kl_low, kl_high = _f32(float(desired) * float(v["low"])), _f32(float(desired) * float(v["high"]))
    if not np.isfinite(kl_high) or not kl_low < kl_high:
        raise ValueError(f"adaptive_lr: float32(desired_kl * low) = {float(kl_low)!r} must lie below float32(desired_kl * high) = "
                         f"{float(kl_high)!r}, both finite; choose low < high (the defaults are 0.5 and 2.0)")
    for k in ("min", "max"):
        if not _positive_number(v[k]) or not _f32(v[k]) > 0 or not np.isfinite(_f32(v[k])):
            raise ValueError(f"adaptive_lr.{k} must be a finite number > 0 (also as a float32), got {v[k]!r}; leave it out for the default "
                             f"{ADAPTIVE_LR_DEFAULTS[k]!r}")
    if not np.float32(v["min"]) <= np.float32(v["max"]):
        raise ValueError(f"adaptive_lr.min = {v['min']!r} must not exceed adaptive_lr.max = {v['max']!r}; exchange them, or leave them out "
                         "for the defaults 1e-5 and 1e-2")
    return dict(desired_kl=float(desired), low=float(v["low"]), high=float(v["high"]), factor=float(np.float32(v["factor"])),
                min=float(np.float32(v["min"])), max=float(np.float32(v["max"])), kl_low=float(kl_low), kl_high=float(kl_high))


def adaptive_lr_step(lr32, kl32, rule):
    """The rule of ``adaptive_lr`` for one minibatch step, in numpy float32 (the one host definition of what
    grad_sqnorm_adaptive_kernel decides; csrc/optim.hip): ``lr32`` the learning rate before the step, ``kl32`` the step's own kl,
    ``rule`` of ``adaptive_lr_section`` -> (the learning rate the step's AdamW launch uses, -1 cut | 0 kept | +1 raised).  A NaN kl or
    a kl <= 0 changes nothing, +Inf cuts, a kl at a limit changes nothing; the clamps act on a change only.  The direction says what
    was decided, also where a clamp left the value as it was (a cut at ``min``)."""
    lr, kl = np.float32(lr32), np.float32(kl32)
    factor, lo, hi = np.float32(rule["factor"]), np.float32(rule["min"]), np.float32(rule["max"])
    if kl > np.float32(rule["kl_high"]):
        return np.maximum(lo, np.float32(lr / factor)), -1          # (float32 / float32: correctly rounded, as __fdiv_rn)
    if kl < np.float32(rule["kl_low"]) and kl > np.float32(0):
        return np.minimum(hi, np.float32(lr * factor)), 1
    return lr, 0


KL_ESTIMATORS = ("k3", "analytic")


def kl_estimator_section(config: dict) -> str:
    """The optional key ``kl_estimator`` -> "k3" (absent: the sample estimate mean((ratio - 1) - log ratio) of every policy kind) or
    "analytic" (the exact KL of the two diagonal Gaussians of a Box policy, ``gaussian_kl``).  Any other value is refused."""
    value = config.get("kl_estimator", "k3")
    if not isinstance(value, str) or value not in KL_ESTIMATORS:
        raise ValueError(f"kl_estimator must be one of {list(KL_ESTIMATORS)}, got {value!r}; write `k3` (or remove the key) for the sample "
                         "estimate, `analytic` for the exact KL of a Box policy's Gaussians")
    return value


def gaussian_kl(old_mean, old_log_std, mean, log_std, dtype=np.float64):
    """KL(old || new) of two diagonal Gaussians, the mean over the N samples of the sum over the A dimensions, in numpy ``dtype`` (the
    one host definition of what heads_loss_gaussian_kl_kernel reduces; csrc/heads_loss.hip): ``old_mean`` / ``mean`` [N, A],
    ``old_log_std`` / ``log_std`` [A].
        KL_n = sum_a [(expm1(2 d_a) / 2 - d_a) + ((old_mean_na - mean_na) / sigma_a)^2 / 2],  d_a = old_log_std_a - log_std_a
    -- rsl_rl's log(sigma / sigma_old) + (sigma_old^2 + (mu_old - mu)^2) / (2 sigma^2) - 1/2 written so that nothing cancels (and
    without its 1e-5): equal policies give exactly 0, equal log-stds exactly mean_n sum_a ((mu_old - mu) / sigma)^2 / 2."""
    dt = np.dtype(dtype).type
    mo, mu = np.asarray(old_mean, dtype=dt), np.asarray(mean, dtype=dt)
    lo, ls = np.asarray(old_log_std, dtype=dt).reshape(-1), np.asarray(log_std, dtype=dt).reshape(-1)
    if mo.ndim != 2 or mo.shape != mu.shape or lo.shape != (mo.shape[1],) or ls.shape != lo.shape:
        raise ValueError(f"gaussian_kl: means [N, A] and log-stds [A] expected, got {mo.shape}, {lo.shape}, {mu.shape}, {ls.shape}")
    d = lo - ls
    const = (dt(0.5) * np.expm1(dt(2) * d) - d).sum(dtype=dt)
    q = (mo - mu) / np.exp(ls)
    per_sample = const + (dt(0.5) * q * q).sum(axis=1, dtype=dt)
    return dt(per_sample.sum(dtype=dt) / dt(mo.shape[0]))


def exact_kl_section(config: dict) -> bool:
    """The optional key ``exact_kl`` -> False (absent or ``false``: the KL statistic is what ``kl_estimator`` says, the k3 sample
    estimate by default) or True (the exact KL(old || new) of every policy kind: ``gaussian_kl`` for a Box policy, ``categorical_kl``
    for Discrete and MultiDiscrete ones, masked or not).  A value that is no bool is refused."""
    value = config.get("exact_kl", False)
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"exact_kl must be true or false, got {value!r}; write `exact_kl: true` for the exact KL of the rollout's and "
                         "the current policy, or remove the key for the sample estimate")
    return bool(value)


def categorical_kl(old_logps, logits, sizes, mask_words=None, dtype=np.float64):
    """Exact KL(old || new) of categorical policies, the mean over the N samples AND the B branches (the convention of the k3 column it
    replaces; the joint KL of a sample's branches is B times it), in numpy ``dtype`` -- the one host definition of what the categorical
    loss kernels reduce (etm_categorical_kl_term; csrc/heads_loss.hip, csrc/ppo_loss.hip).  ``old_logps`` [N, sum(sizes)]: every
    column's log-prob under the policy that drew the samples (-inf where the column was masked out); ``logits`` [N, sum(sizes)]: the
    current raw logits, the branches' segments side by side; ``mask_words`` (optional) [N] int64: bit j = column j was allowed.
    Per sample n and branch b with valid columns V (all of them without masks), with l_j = logit_j - lse_V, d_j = old_j - l_j:
        KL_nb = sum_{j in V} t_j,   t_j = exp(old_j) (expm1(-d_j) + d_j)  for d_j >= -60,   t_j = exp(l_j)  for d_j < -60
    -- sum p_old (old - l) with the vanishing sum (p - p_old) added: every term is >= 0 and no term of size 1 cancels, equal policies
    give exactly 0; below d = -60 the limit p_old -> 0 (the dropped part is under e^-60 |d|, and inf * denormal stays out of the
    sum).  Columns outside V are skipped, not multiplied (0 * inf); a branch with one valid action contributes 0."""
    dt = np.dtype(dtype).type
    lo, lg = np.asarray(old_logps, dtype=dt), np.asarray(logits, dtype=dt)
    sizes = tuple(int(a) for a in sizes)
    if lg.ndim != 2 or lo.shape != lg.shape or not sizes or min(sizes) <= 0 or sum(sizes) != lg.shape[1]:
        raise ValueError(f"categorical_kl: old_logps and logits [N, {sum(sizes)}] for branches {sizes} expected, got {lo.shape}, {lg.shape}")
    N, A = lg.shape
    if mask_words is None:
        valid = np.ones((N, A), dtype=bool)
    else:
        if A > 63:
            raise ValueError(f"categorical_kl: a mask word describes at most 63 columns, not {A}")
        words = np.asarray(mask_words).astype(np.int64).reshape(-1)
        if words.shape != (N,):
            raise ValueError(f"categorical_kl: mask_words [{N}] expected, got {words.shape}")
        valid = ((words[:, None] >> np.arange(A, dtype=np.int64)[None, :]) & 1).astype(bool)
    total, off = dt(0), 0
    with np.errstate(all="ignore"):
        for size in sizes:
            v = valid[:, off:off + size]
            if not v.any(axis=1).all():
                raise ValueError("categorical_kl: a branch without a valid action")
            l = np.where(v, lg[:, off:off + size], dt(-np.inf))
            mx = l.max(axis=1, keepdims=True)
            logp = l - (mx + np.log(np.exp(l - mx).sum(axis=1, keepdims=True, dtype=dt)))
            old = lo[:, off:off + size]
            d = old - logp
            t = np.where(d >= dt(-60), np.exp(old) * (np.expm1(-d) + d), np.exp(logp))
            total = dt(total + np.where(v, t, dt(0)).sum(dtype=dt))
            off += size
    return dt(total / dt(N * len(sizes)))


class Module(nn.Module):
    """nn.Module with gradient norm / mean helpers."""

    def _flat_grads(self):
        grads = [p.grad.view(-1) for _, p in self.named_parameters() if p.grad is not None]
        return torch.cat(grads) if grads else None

    def grad_norm(self):
        g = self._flat_grads()
        return torch.linalg.norm(g).item() if g is not None else None

    def grad_mean(self):
        g = self._flat_grads()
        return torch.mean(g).item() if g is not None else None
