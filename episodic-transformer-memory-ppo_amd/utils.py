"""Helpers with the upstream names (utils.py): create_env, polynomial_decay, batched_index_select,
process_episode_info, Module; normalization_section reads this build's two normalisation keys, target_kl_section its KL early
stop, target_kl_rows says which rows of an update's result tables a stopped update returns; adaptive_lr_section reads the
KL-adaptive learning rate and adaptive_lr_step is its rule, the one host definition of what the norm kernel decides;
kl_estimator_section reads which KL both rules see and gaussian_kl is the exact KL of a Box policy's Gaussians, the one host
definition of what the Gaussian heads + loss kernel reduces; exact_kl_section reads the key that switches the exact KL on for every
policy kind and categorical_kl is the exact KL of Discrete / MultiDiscrete policies, the one host definition of what the categorical
loss kernels reduce; kl_penalty_section reads the KL penalty of the loss, kl_penalty_step is the rule that adapts its coefficient once
per update, and categorical_kl_grad / gaussian_kl_grad are the gradients of the two exact KLs, the one host definition of what the
penalty kernels add to d logits; obs_reconstruction_section reads the observation reconstruction loss, obs_reconstruction_loss and
transposed_conv_last are the one host definition of what the fused last decoder layer + loss kernel computes."""
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
    if kind == "HiddenArm":
        from environments.hidden_arm_env import HiddenArmEnv
        seed = int(config["seed"]) + int(worker_id) if config.get("seed") is not None else None
        return HiddenArmEnv(arms=int(config.get("arms", 2)), max_episode_steps=int(config.get("max_episode_steps", 16)), seed=seed)
    from environments.device_types import DEVICE_ENV_TYPES, make_host_env
    if kind in DEVICE_ENV_TYPES:
        # the host twin of an image memory task (environments/cue_room_env.py, command_room_env.py, path_room_env.py, spot_room_env.py);
        # ``device: true`` is the vectorised front-end's key (environments/device_env.py) and means nothing to a single environment
        return make_host_env(config, worker_id=worker_id)
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


def attention_statistics_section(config: dict) -> bool:
    """The optional key ``attention_statistics`` -> False (absent or ``false``: nothing is allocated, launched or changed) or True
    (every grad-enabled forward pass of an update adds its attention probabilities to a per-block, per-head table).  A value that is
    no bool is refused."""
    value = config.get("attention_statistics", False)
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"attention_statistics must be true or false, got {value!r}; write `attention_statistics: true` to record where "
                         "the policy's attention lands in its memory window, or remove the key")
    return bool(value)


ATTENTION_STATISTICS_WORDS = 264      # doubles per head of the table (include/etm_hip.h: etm_attn_stats)


def attention_statistics_summary(table, memory_length: int) -> dict:
    """The accumulator of etm_attn_stats, ``table`` [blocks, heads, 264] float64, as a dict of numpy arrays (a pure host function):
    ``rows``, ``empty``, ``irregular`` [B, H]: the counted rows (a prefix mask with at least one valid entry), the rows without a
    valid entry and the rows whose mask was no prefix; ``entropy`` (nats), ``max_prob``, ``mean_age`` [B, H]: means over the counted
    rows; ``normalised_entropy`` [B, H]: the mean of entropy / ln v over the rows with v >= 2 valid entries -- each NaN where its
    count is 0; ``age_hist``, ``index_hist`` [B, H, L]: the attention mass by age (``age_hist[..., a - 1]``: age a, 1 = the newest
    stored step) and by window entry, each divided by its total mass (NaN without mass).  ``mean_age`` is the age histogram's mean.
    Words beyond ``memory_length`` are padding and are not read."""
    table = np.asarray(table, dtype=np.float64)
    L = int(memory_length)
    if table.ndim != 3 or table.shape[2] != ATTENTION_STATISTICS_WORDS or not 1 <= L <= 128:
        raise ValueError(f"attention_statistics_summary: a table [blocks, heads, {ATTENTION_STATISTICS_WORDS}] and 1 <= memory_length "
                         f"<= 128 are needed, got {table.shape} and {memory_length}")
    rows, rows2 = table[:, :, 0], table[:, :, 1]
    age, index = table[:, :, 8: 8 + L], table[:, :, 136: 136 + L]
    age_mass, index_mass = age.sum(axis=2), index.sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_row = lambda x, n: np.where(n > 0, x / n, np.nan)
        return {"rows": rows.copy(), "empty": table[:, :, 2].copy(), "irregular": table[:, :, 3].copy(),
                "entropy": per_row(table[:, :, 4], rows), "normalised_entropy": per_row(table[:, :, 5], rows2),
                "max_prob": per_row(table[:, :, 6], rows),
                "mean_age": per_row((age * np.arange(1, L + 1, dtype=np.float64)).sum(axis=2), age_mass),
                "age_hist": per_row(age, age_mass[:, :, None]), "index_hist": per_row(index, index_mass[:, :, None])}


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


def _valid_columns(mask_words, N, A, what):
    if mask_words is None:
        return np.ones((N, A), dtype=bool)
    if A > 63:
        raise ValueError(f"{what}: a mask word describes at most 63 columns, not {A}")
    words = np.asarray(mask_words).astype(np.int64).reshape(-1)
    if words.shape != (N,):
        raise ValueError(f"{what}: mask_words [{N}] expected, got {words.shape}")
    return ((words[:, None] >> np.arange(A, dtype=np.int64)[None, :]) & 1).astype(bool)


def categorical_kl_grad(old_logps, logits, sizes, mask_words=None, dtype=np.float64):
    """d (sum_n sum_b KL_nb) / d logits, [N, sum(sizes)] in numpy ``dtype``, KL_nb as in ``categorical_kl`` (whose operands these are;
    that function returns the sum divided by N B) -- the one host definition of what the penalty kernels add to d logits (PEN;
    csrc/heads_loss.hip, csrc/ppo_loss.hip).  Per sample and branch with valid columns V, p_j = exp(l_j), p_old_j = exp(old_j) (+0 at
    -inf):
        d KL_nb / d logit_k = p_k - p_old_k  for k in V,   exactly 0 for k outside V
    -- from sum_{j in V} p_old_j (old_j - l_j) with d l_j / d logit_k = delta_jk - p_k and sum_V p_old = 1.  No case at d < -60: there
    p_old -> 0 and the term's derivative is p_k.  Equal policies give exactly 0, and so does a branch with one valid action (1 - 1)."""
    dt = np.dtype(dtype).type
    lo, lg = np.asarray(old_logps, dtype=dt), np.asarray(logits, dtype=dt)
    sizes = tuple(int(a) for a in sizes)
    if lg.ndim != 2 or lo.shape != lg.shape or not sizes or min(sizes) <= 0 or sum(sizes) != lg.shape[1]:
        raise ValueError(f"categorical_kl_grad: old_logps and logits [N, {sum(sizes)}] for branches {sizes} expected, got {lo.shape}, {lg.shape}")
    N, A = lg.shape
    valid = _valid_columns(mask_words, N, A, "categorical_kl_grad")
    out, off = np.zeros((N, A), dtype=dt), 0
    with np.errstate(all="ignore"):
        for size in sizes:
            v = valid[:, off:off + size]
            if not v.any(axis=1).all():
                raise ValueError("categorical_kl_grad: a branch without a valid action")
            l = np.where(v, lg[:, off:off + size], dt(-np.inf))
            mx = l.max(axis=1, keepdims=True)
            logp = l - (mx + np.log(np.exp(l - mx).sum(axis=1, keepdims=True, dtype=dt)))
            out[:, off:off + size] = np.where(v, np.exp(logp) - np.exp(lo[:, off:off + size]), dt(0))
            off += size
    return out


def gaussian_kl_grad(old_mean, old_log_std, mean, log_std, dtype=np.float64):
    """(d / d mean [N, A], d / d log_std [A]) of sum_n KL_n, KL_n as in ``gaussian_kl`` (which returns the sum divided by N), in numpy
    ``dtype`` -- the one host definition of what heads_loss_gaussian_kl_penalty_kernel adds.  With d_a = old_log_std_a - log_std_a and
    q_na = (old_mean_na - mean_na) / sigma_a:
        d KL_n / d mean_na = -q_na / sigma_a,    d KL_n / d log_std_a = -expm1(2 d_a) - q_na^2
    -- the second is 1 - (sigma_old^2 + (mu_old - mu)^2) / sigma^2, written so that equal policies give exactly 0."""
    dt = np.dtype(dtype).type
    mo, mu = np.asarray(old_mean, dtype=dt), np.asarray(mean, dtype=dt)
    lo, ls = np.asarray(old_log_std, dtype=dt).reshape(-1), np.asarray(log_std, dtype=dt).reshape(-1)
    if mo.ndim != 2 or mo.shape != mu.shape or lo.shape != (mo.shape[1],) or ls.shape != lo.shape:
        raise ValueError(f"gaussian_kl_grad: means [N, A] and log-stds [A] expected, got {mo.shape}, {lo.shape}, {mu.shape}, {ls.shape}")
    sigma = np.exp(ls)
    q = (mo - mu) / sigma
    d_mean = -q / sigma
    d_ls = (-np.expm1(dt(2) * (lo - ls))[None, :] - q * q).sum(axis=0, dtype=dt)
    return d_mean.astype(dt), d_ls.astype(dt)


KL_PENALTY_DEFAULTS = dict(high=2.0, low=0.5, up=1.5, down=0.5, min=1.0e-4, max=100.0)


def kl_penalty_section(config: dict):
    """The optional key ``kl_penalty`` (a number: a fixed coefficient, or {coef, target, high, low, up, down, min, max}) -> {"coef",
    "adaptive", "target", "high", "low", "up", "down", "min", "max", "kl_high", "kl_low"}, or None when the key is absent.  ``coef`` alone
    is a fixed coefficient (0 allowed); with ``target`` the coefficient adapts once per update (``kl_penalty_step``) and the other
    sub-keys default to RLlib's thresholds and factors (high 2.0, low 0.5, up 1.5, down 0.5) and this build's clamps (min 1e-4, max
    100).  ``kl_high`` = float32(high * target) and ``kl_low`` = float32(low * target), each product formed once in double and rounded
    once; ``coef``, ``up``, ``down``, ``min`` and ``max`` are each rounded to float32 (python floats that hold a float32 exactly).
    Without ``target`` the rule's entries are None."""
    sec = config.get("kl_penalty")
    if sec is None:
        return None
    if not isinstance(sec, dict):
        sec = {"coef": sec}
    known = ("coef", "target") + tuple(KL_PENALTY_DEFAULTS)
    unknown = sorted(set(sec) - set(known))
    if unknown:
        raise ValueError(f"kl_penalty: unknown keys {unknown} (known: {list(known)}); remove them")
    if "coef" not in sec:
        raise ValueError("kl_penalty: the section needs `coef` (the coefficient of the KL term, e.g. 0.2); add it, or remove the key to "
                         "train without the penalty")
    coef = sec["coef"]
    if not _finite_number(coef) or not coef >= 0 or not np.isfinite(_f32(coef)):
        raise ValueError(f"kl_penalty.coef must be a finite number >= 0 (also as a float32), got {coef!r}; remove the key to train without "
                         "the penalty")
    coef32 = float(np.float32(coef))
    if "target" not in sec:
        extra = sorted(set(sec) - {"coef"})
        if extra:
            raise ValueError(f"kl_penalty: {extra} belong to the adaptive coefficient and need `target` (the KL the coefficient is steered "
                             "to, e.g. 0.01); add it, or remove them for a fixed coefficient")
        return dict(coef=coef32, adaptive=False, target=None, kl_high=None, kl_low=None, **{k: None for k in KL_PENALTY_DEFAULTS})
    v = {k: sec.get(k, d) for k, d in KL_PENALTY_DEFAULTS.items()}
    v["target"] = sec["target"]
    for k in ("target",) + tuple(KL_PENALTY_DEFAULTS):
        if not _positive_number(v[k]) or not _f32(v[k]) > 0 or not np.isfinite(_f32(v[k])):
            hint = "remove it for a fixed coefficient" if k == "target" else f"leave it out for the default {KL_PENALTY_DEFAULTS[k]!r}"
            raise ValueError(f"kl_penalty.{k} must be a finite number > 0 (also as a float32), got {v[k]!r}; {hint}")
    if coef32 == 0:
        raise ValueError("kl_penalty: coef 0 with `target`: a multiplication never leaves 0, the coefficient could not adapt; start at a "
                         "positive coef (e.g. 0.2), or remove target for a fixed coefficient of 0")
    kl_low, kl_high = _f32(float(v["target"]) * float(v["low"])), _f32(float(v["target"]) * float(v["high"]))
    if not np.isfinite(kl_high) or not kl_low < kl_high:
        raise ValueError(f"kl_penalty: float32(low * target) = {float(kl_low)!r} must lie below float32(high * target) = {float(kl_high)!r}, "
                         "both finite; choose low < high (the defaults are 0.5 and 2.0)")
    if not np.float32(v["up"]) > 1:
        raise ValueError(f"kl_penalty.up must be > 1 (also as a float32; the coefficient rises by it above high * target), got {v['up']!r}; "
                         "leave it out for the default 1.5")
    if not np.float32(v["down"]) < 1:
        raise ValueError(f"kl_penalty.down must be < 1 (also as a float32; the coefficient falls by it below low * target), got "
                         f"{v['down']!r}; leave it out for the default 0.5")
    if not np.float32(v["min"]) <= np.float32(v["max"]):
        raise ValueError(f"kl_penalty.min = {v['min']!r} must not exceed kl_penalty.max = {v['max']!r}; exchange them, or leave them out "
                         "for the defaults 1e-4 and 100")
    if not np.float32(v["min"]) <= np.float32(coef32) <= np.float32(v["max"]):
        raise ValueError(f"kl_penalty: the start value float32(coef) = {coef32!r} lies outside [min, max] = [{float(np.float32(v['min']))!r}, "
                         f"{float(np.float32(v['max']))!r}]; move coef into the range, or widen kl_penalty.min / kl_penalty.max")
    return dict(coef=coef32, adaptive=True, target=float(v["target"]), high=float(v["high"]), low=float(v["low"]),
                up=float(np.float32(v["up"])), down=float(np.float32(v["down"])), min=float(np.float32(v["min"])),
                max=float(np.float32(v["max"])), kl_high=float(kl_high), kl_low=float(kl_low))


def kl_penalty_step(coef32, kl32, rule):
    """The rule of an adaptive ``kl_penalty`` for one update, in numpy float32 (PPO paper section 4; RLlib's thresholds, with clamps):
    ``coef32`` the coefficient the update used, ``kl32`` float32(the mean of the update's returned kl column), ``rule`` of
    ``kl_penalty_section`` -> (the next update's coefficient, -1 cut | 0 kept | +1 raised).  kl > kl_high: min(max, coef * up);
    kl < kl_low: max(min, coef * down); a kl at a limit and a NaN change nothing.  The direction says what was decided, also where a
    clamp left the value as it was."""
    coef, kl = np.float32(coef32), np.float32(kl32)
    if kl > np.float32(rule["kl_high"]):
        return np.minimum(np.float32(rule["max"]), np.float32(coef * np.float32(rule["up"]))), 1
    if kl < np.float32(rule["kl_low"]):
        return np.maximum(np.float32(rule["min"]), np.float32(coef * np.float32(rule["down"]))), -1
    return coef, 0


OBS_RECONSTRUCTION_KEYS = ("initial", "final", "power", "max_decay_steps")


def obs_reconstruction_sizes(limit: int = 200):
    """The image sizes (one side) the decoder maps back onto themselves, up to ``limit``: the three encoder layers must consume the
    side without a remainder -- (H - 8) % 4 == 0, then (h1 - 4) % 2 == 0, then h2 >= 3 -- because the transposed layers produce exactly
    (h - 1) * stride + kernel.  84 -> 20 -> 9 -> 7 -> 9 -> 20 -> 84 is one of them."""
    return [h for h in range(8, limit + 1) if obs_reconstruction_maps_back(h)]


def obs_reconstruction_maps_back(side: int) -> bool:
    h = int(side)
    for k, s in ((8, 4), (4, 2), (3, 1)):
        if h < k or (h - k) % s:
            return False
        h = (h - k) // s + 1
    return True


def obs_reconstruction_section(config: dict, observation_shape=None, world: int = 1):
    """The optional key ``obs_reconstruction`` (a number > 0: a fixed coefficient, or the four keys of the other schedules {initial, final,
    power, max_decay_steps}) -> that schedule as a dict of floats (``polynomial_decay`` gives the coefficient of an update), or None when
    the key is absent.  The training loss is then L_ppo + coef * (the mean sigmoid cross-entropy of the decoder's logits against the
    observation, ``obs_reconstruction_loss``).  Refused, each with what to do instead: a value that is neither a number > 0 nor a dict
    of exactly the four keys with finite values >= 0 and initial > 0; vector observations and image sizes the decoder does not map back
    onto themselves (``observation_shape``, when given); a data-parallel run (``world`` > 1)."""
    value = config.get("obs_reconstruction")
    if value is None:
        return None
    if isinstance(value, dict):
        unknown, missing = sorted(str(k) for k in set(value) - set(OBS_RECONSTRUCTION_KEYS)), [k for k in OBS_RECONSTRUCTION_KEYS if k not in value]
        if unknown or missing:
            raise ValueError(f"obs_reconstruction: a schedule has exactly the keys {list(OBS_RECONSTRUCTION_KEYS)} (unknown: {unknown}, "
                             f"missing: {missing}); write all four, or a single number for a fixed coefficient")
        for k in OBS_RECONSTRUCTION_KEYS:
            if not _finite_number(value[k]) or not value[k] >= 0 or not np.isfinite(_f32(value[k])):
                raise ValueError(f"obs_reconstruction.{k} must be a finite number >= 0, got {value[k]!r}")
        if not value["initial"] > 0 or not _f32(value["initial"]) > 0:
            raise ValueError(f"obs_reconstruction.initial must be > 0 (the coefficient the run starts with), got {value['initial']!r}; "
                             "remove the key to train without the reconstruction loss")
        sec = {k: float(value[k]) for k in OBS_RECONSTRUCTION_KEYS}
    elif _positive_number(value) and np.isfinite(_f32(value)) and _f32(value) > 0:
        sec = dict(initial=float(value), final=float(value), power=1.0, max_decay_steps=0.0)
    else:
        raise ValueError(f"obs_reconstruction must be a number > 0 (a fixed coefficient, e.g. 0.1) or a schedule {{initial, final, power, "
                         f"max_decay_steps}}, got {value!r}; remove the key to train without the reconstruction loss")
    if observation_shape is not None:
        shape = tuple(int(s) for s in observation_shape)
        if len(shape) != 3:
            raise ValueError(f"obs_reconstruction is for image observations [C, H, W] (the decoder mirrors the convolutional encoder), got "
                             f"the observation shape {shape}; remove the key")
        if shape[0] > 4:
            raise ValueError(f"obs_reconstruction: the last decoder layer's kernel carries at most 4 image channels, got {shape[0]}; "
                             "remove the key")
        bad = [s for s in shape[1:] if not obs_reconstruction_maps_back(s)]
        if bad:
            raise ValueError(f"obs_reconstruction: the decoder does not map a side of {bad[0]} pixels back onto itself (the encoder's "
                             f"layers must consume it without a remainder: (H - 8) % 4 == 0 for the first, and so on); sides that work: "
                             f"{obs_reconstruction_sizes(132)} ...; resize the observation, or remove the key")
    if world > 1:
        raise ValueError("obs_reconstruction in a data-parallel run: every rank would report the reconstruction loss of its own "
                         "minibatches (agreeing on one loss over the ranks is not built); remove the key, or train on one device")
    return sec


def obs_reconstruction_coef(section: dict, update: int) -> float:
    """The coefficient of update ``update`` as the float32 the device word holds (a decay of 0 steps: ``initial`` at update 0, then
    ``final``)."""
    if section["max_decay_steps"] <= 0:
        return float(np.float32(section["initial"] if update <= 0 else section["final"]))
    return float(np.float32(polynomial_decay(section["initial"], section["final"], section["max_decay_steps"], section["power"], update)))


def obs_reconstruction_target(target, dtype=np.float64):
    """The observation as the loss's target in [0, 1]: a byte k stands for float32(k) / float32(255) (the one conversion of
    csrc/etm_common.h), then ``dtype``; a float array is taken as it is."""
    t = np.asarray(target)
    if t.dtype == np.uint8:
        t = t.astype(np.float32) / np.float32(255)
    return t.astype(dtype)


def obs_reconstruction_loss(logits, target, dtype=np.float64):
    """(loss, dlogits) of the sigmoid cross-entropy on the logit, in numpy ``dtype`` -- the one host definition of what
    etm_obs_recon_fwd_loss computes.  Per element l = max(z, 0) - z t + log1p(exp(-|z|)) (no sigmoid followed by a log: finite for every
    finite z); loss = the mean of l over all elements; dlogits = (sigma(z) - t) / (number of elements), sigma formed from exp(-|z|) so
    that neither tail overflows.  ``target`` as ``obs_reconstruction_target`` takes it, in the shape of ``logits``."""
    dt = np.dtype(dtype).type
    z = np.asarray(logits, dtype=dt)
    t = obs_reconstruction_target(target, dt)
    if z.shape != t.shape or z.size == 0:
        raise ValueError(f"obs_reconstruction_loss: logits and target of one non-empty shape expected, got {z.shape} and {t.shape}")
    e = np.exp(-np.abs(z))
    l = np.maximum(z, dt(0)) - z * t + np.log1p(e)
    r = dt(1) / (dt(1) + e)
    sigma = np.where(z >= 0, r, e * r)
    count = dt(z.size)
    return dt(l.sum(dtype=dt) / count), ((sigma - t) / count).astype(dt)


def transposed_conv_last(a, w, b, dtype=np.float64):
    """The decoder's last layer in plain numpy ``dtype``: ConvTranspose2d(Cin, C, 8, 4) on ``a`` NHWC [N, Hi, Wi, Cin] with ``w``
    [Cin, C, 8, 8] and ``b`` [C] (the parameters' own layouts) -> the logits NHWC [N, 4 (Hi - 1) + 8, 4 (Wi - 1) + 8, C].  Output pixel
    (Y, X) sums over the at most 2 x 2 input pixels with 0 <= Y - 4 iy < 8, 0 <= X - 4 ix < 8 and over the channels, in ascending
    (iy, ix, ci), the bias last -- the kernel's order."""
    dt = np.dtype(dtype).type
    a, w, b = np.asarray(a, dtype=dt), np.asarray(w, dtype=dt), np.asarray(b, dtype=dt)
    if a.ndim != 4 or w.ndim != 4 or w.shape[0] != a.shape[3] or w.shape[2:] != (8, 8) or b.shape != (w.shape[1],):
        raise ValueError(f"transposed_conv_last: a [N, Hi, Wi, Cin], w [Cin, C, 8, 8], b [C] expected, got {a.shape}, {w.shape}, {b.shape}")
    n, hi, wi, cin = a.shape
    c = w.shape[1]
    z = np.zeros((n, 4 * hi + 4, 4 * wi + 4, c), dtype=dt)
    for iy in range(hi):
        for ix in range(wi):
            for ci in range(cin):       # z[n, 4 iy + ky, 4 ix + kx, c] += a[n, iy, ix, ci] w[ci, c, ky, kx]
                z[:, 4 * iy:4 * iy + 8, 4 * ix:4 * ix + 8, :] += a[:, iy, ix, ci][:, None, None, None] * w[ci].transpose(1, 2, 0)[None]
    return z + b


PREVIOUS_STEP_MAX_ROWS = 64          # rows of the table the kernels carry (csrc/prev_input.hip PI_MAXR; RF_MAXSPLIT of the step kernel)


def previous_step_input_section(config: dict, action_space_shape=None, box=False, worker_processes=False):
    """The optional key ``previous_step_input`` (``true``: both, or {action, reward} with at least one true) -> {"action", "reward"},
    or None when the key is absent or ``false``.  Refused, each with what to do instead: a value that is neither a bool nor a dict of
    the two bools, unknown sub-keys, both sub-keys false; a Box policy (``box``); ``worker_processes: true``; a table of more than 64
    rows (``action_space_shape``, when given: sum A_b, + 1 with ``reward``)."""
    value = config.get("previous_step_input")
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)):
        if not value:
            return None
        sec = dict(action=True, reward=True)
    elif isinstance(value, dict):
        known = ("action", "reward")
        unknown = sorted(str(k) for k in set(value) - set(known))
        if unknown:
            raise ValueError(f"previous_step_input: unknown keys {unknown} (known: {list(known)}); remove them")
        sec = {}
        for k in known:
            v = value.get(k, False)
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"previous_step_input.{k} must be true or false, got {v!r}")
            sec[k] = bool(v)
        if not sec["action"] and not sec["reward"]:
            raise ValueError("previous_step_input: both `action` and `reward` are false, so nothing would be fed back; set at least one "
                             "of them true, or remove the key")
    else:
        raise ValueError(f"previous_step_input must be true or {{action: bool, reward: bool}}, got {value!r}; write "
                         "`previous_step_input: true` for both the previous action and the previous reward, or remove the key")
    if box:
        raise ValueError("previous_step_input does not carry a Box policy (the table has one row per discrete action): use a Discrete or "
                         "MultiDiscrete action space, append the previous action to the observation in a wrapper, or remove the key")
    if worker_processes:
        raise ValueError("worker_processes: true does not carry previous_step_input (the shared segment has no row for the last reward): "
                         "set worker_processes: false (in-process environments hand the reward over each step), or remove the key")
    if action_space_shape is not None:
        rows = previous_step_table_rows(action_space_shape, sec["reward"])
        if rows > PREVIOUS_STEP_MAX_ROWS:
            raise ValueError(f"previous_step_input: the table would have {rows} rows (sum of the action space {tuple(action_space_shape)}"
                             f"{' + the reward row' if sec['reward'] else ''}), the kernels carry {PREVIOUS_STEP_MAX_ROWS}: use a smaller "
                             "action space, or remove the key")
    return sec


def previous_step_table_rows(sizes, reward: bool) -> int:
    """R of the table ``prev_input.weight`` [R, D]: branch b owns rows off_b .. off_b + A_b - 1 (the flat layout of the action masks),
    the reward row, with ``reward`` only, is the last one."""
    sizes = tuple(int(a) for a in sizes)
    if not sizes or min(sizes) <= 0:
        raise ValueError(f"previous_step_table_rows: positive branch sizes expected, got {sizes}")
    return sum(sizes) + (1 if reward else 0)


def _previous_step_operands(table, prev_actions, prev_rewards, sizes, dt):
    T = np.asarray(table, dtype=dt)
    sizes = tuple(int(a) for a in sizes)
    reward = prev_rewards is not None
    if T.ndim != 2 or (sizes and min(sizes) <= 0) or T.shape[0] < sum(sizes) + (1 if reward else 0) or not (sizes or reward):
        raise ValueError(f"previous step rule: a table [R >= {sum(sizes) + (1 if reward else 0)}, D] for branches {sizes} expected, got {T.shape}")
    if sizes:
        a = np.asarray(prev_actions).astype(np.int64)
        a = a.reshape(a.shape[0], -1)
        if a.shape[1] != len(sizes):
            raise ValueError(f"previous step rule: prev_actions [N, {len(sizes)}] expected, got {a.shape}")
        if (a >= np.asarray(sizes, dtype=np.int64)[None, :]).any():
            raise ValueError("previous step rule: an action outside its branch")
        n = a.shape[0]
    else:
        a = None
        n = np.asarray(prev_rewards).reshape(-1).shape[0]
    r = None
    if reward:
        r = np.asarray(prev_rewards, dtype=dt).reshape(-1)
        if r.shape != (n,):
            raise ValueError(f"previous step rule: prev_rewards [{n}] expected, got {r.shape}")
    return T, a, r, sizes, n


def previous_step_rows(table, prev_actions, prev_rewards, sizes, bias=None, dtype=np.float64):
    """The addend of ``previous_step_input`` in numpy ``dtype`` -- the one host definition of what etm_prev_input_rows writes
    (csrc/prev_input.hip; bit for bit in float32).  ``table`` T [R, D]; ``prev_actions`` [N, B] int64, one column per entry of ``sizes``
    (empty ``sizes``: the action rows are not fed back and ``prev_actions`` is not read), a NEGATIVE entry in column 0 = the sample has
    no previous step; ``prev_rewards`` [N] (None: no reward term), the raw reward.
        e_n = sum_b T[off_b + a_nb, :] + r_n T[R - 1, :]
    started at +0, the branches in ascending b, the reward term last, every product and sum rounded on its own; a sample without a
    previous step is exactly +0 in every column.  ``bias`` [D] (optional) is added last, to every row."""
    dt = np.dtype(dtype).type
    T, a, r, sizes, n = _previous_step_operands(table, prev_actions, prev_rewards, sizes, dt)
    out = np.zeros((n, T.shape[1]), dtype=dt)
    has = np.ones(n, dtype=bool) if a is None else a[:, 0] >= 0
    off = 0
    for b, size in enumerate(sizes):
        idx = np.where(has, a[:, b], 0)
        if (idx < 0).any():
            raise ValueError("previous step rule: a negative action behind column 0 of a sample that has a previous step")
        out = np.where(has[:, None], (out + T[off + idx]).astype(dt), out)
        off += size
    if r is not None:
        out = np.where(has[:, None], (out + (r[:, None] * T[-1][None, :]).astype(dt)).astype(dt), out)
    if bias is not None:
        out = (out + np.asarray(bias, dtype=dt).reshape(1, -1)).astype(dt)
    return out


def previous_step_coefficients(prev_actions, prev_rewards, sizes, rows, dtype=np.float64):
    """c [N, R] of the rule above as a matrix: e = c T.  c_nk = 1 at the rows of the sample's previous actions, r_n at the reward row
    (the last), 0 elsewhere, and 0 everywhere for a sample without a previous step."""
    dt = np.dtype(dtype).type
    _, a, r, sizes, n = _previous_step_operands(np.zeros((rows, 1), dtype=dt), prev_actions, prev_rewards, sizes, dt)
    c = np.zeros((n, rows), dtype=dt)
    has = np.ones(n, dtype=bool) if a is None else a[:, 0] >= 0
    off = 0
    for b, size in enumerate(sizes):
        c[np.nonzero(has)[0], off + a[has, b]] += dt(1)
        off += size
    if r is not None:
        c[has, rows - 1] = r[has]
    return c


def previous_step_table_grad(gm, prev_actions, prev_rewards, sizes, rows, dtype=np.float64):
    """d L / d T [R, D] in numpy ``dtype`` -- the host definition of what etm_prev_input_grad sums: dT[k, :] = sum_n c_nk gm[n, :] with
    ``previous_step_coefficients``, ``gm`` [N, D] the gradient at lin_hidden's pre-activation.  The samples are added in ascending n;
    a row that no sample touched is exactly 0."""
    dt = np.dtype(dtype).type
    g = np.asarray(gm, dtype=dt)
    _, a, r, sizes, n = _previous_step_operands(np.zeros((rows, 1), dtype=dt), prev_actions, prev_rewards, sizes, dt)
    if g.ndim != 2 or g.shape[0] != n:
        raise ValueError(f"previous_step_table_grad: gm [{n}, D] expected, got {g.shape}")
    out = np.zeros((rows, g.shape[1]), dtype=dt)
    for i in range(n):
        if a is not None and a[i, 0] < 0:
            continue
        off = 0
        for b, size in enumerate(sizes):
            out[off + a[i, b]] = out[off + a[i, b]] + g[i]
            off += size
        if r is not None:
            out[rows - 1] = out[rows - 1] + (r[i] * g[i]).astype(dt)
    return out


def previous_step_fields(actions, rewards, dones, carry_actions=None, carry_rewards=None, carry_live=None):
    """The buffer fields of ``previous_step_input`` for one rollout -- the host definition of what the trainer builds on the device.
    ``actions`` [W, S, B] int, ``rewards`` [W, S] (raw, as the environment returned them), ``dones`` [W, S] bool (step t ended its
    episode); the carry of the rollout before: ``carry_actions`` [W, B], ``carry_rewards`` [W], ``carry_live`` [W] bool (False or
    None: the worker starts an episode at step 0 -- the first rollout, a resume, or a done at the last step before).
    -> (prev_actions [W, S, B] int64, prev_rewards [W, S] float32, (carry_actions, carry_rewards, carry_live) for the next rollout).
    At an episode's first step prev_actions is -1 in every branch and prev_rewards is 0; elsewhere they are step t - 1's."""
    a = np.asarray(actions).astype(np.int64)
    if a.ndim == 2:
        a = a[:, :, None]
    r = np.asarray(rewards, dtype=np.float32)
    d = np.asarray(dones).astype(bool)
    W, S, B = a.shape
    if r.shape != (W, S) or d.shape != (W, S):
        raise ValueError(f"previous_step_fields: rewards and dones [{W}, {S}] expected, got {r.shape}, {d.shape}")
    live = np.zeros(W, dtype=bool) if carry_live is None else np.asarray(carry_live).astype(bool).reshape(W)
    ca = np.full((W, B), -1, dtype=np.int64) if carry_actions is None else np.asarray(carry_actions).astype(np.int64).reshape(W, B)
    cr = np.zeros(W, dtype=np.float32) if carry_rewards is None else np.asarray(carry_rewards, dtype=np.float32).reshape(W)
    pa = np.empty((W, S, B), dtype=np.int64)
    pr = np.empty((W, S), dtype=np.float32)
    pa[:, 0] = np.where(live[:, None], ca, -1)
    pr[:, 0] = np.where(live, cr, np.float32(0))
    first = d[:, :-1]                                  # step t + 1 starts an episode where step t ended one
    pa[:, 1:] = np.where(first[:, :, None], -1, a[:, :-1])
    pr[:, 1:] = np.where(first, np.float32(0), r[:, :-1])
    return pa, pr, (a[:, -1].copy(), r[:, -1].copy(), ~d[:, -1])


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
