"""Vectorised environment front-ends for the trainer.

``VecEnv`` protocol (what ``PPOTrainer`` steps):
    num_envs, observation_space_shape, action_space_shape, num_actions, max_episode_steps
    observation_dtype (optional; absent = float32): numpy.uint8 for byte image observations -- ``out`` and the returned rows
        are then uint8 and byte k stands for float32(k) / float32(255) (environments.observation_dtype reads it, or else
        ``observation_space.dtype``)
        action_space_shape: one entry per action branch (environments.action_space_shape: ``nvec`` of a MultiDiscrete space,
        ``(n,)`` of a Discrete one, ``(A,)`` of a Box); num_actions: n of a Discrete space, the sum of ``nvec`` (the policy's
        logits), A of a Box
    action_kind (optional; absent = discrete / multidiscrete by action_space_shape): environments.ActionKind, with the bounds of
        a Box (float action rows [W, A], clipped to them before they arrive)
    reset(out=None) -> obs [W, *obs_shape] float32
    step(actions [W] or [W, B], out=None, on_rows=None) -> (obs, rewards [W] f32, dones [W] bool, infos [W] (dict or None))
        on_rows(lo, hi), optional: called as soon as observation rows [lo, hi) of ``out`` are final, in increasing order and
        covering [0, W) -- the trainer starts their upload while the remaining environments still step
with auto-reset: for a finished worker the returned observation is already the first one of the next episode, which
is exactly what upstream's loop does by hand (trainer.py:195-201).
    A finished episode's info dict may carry two more keys (the trainer strips both before it averages the infos):
    "truncated": True -- the episode was only CUT (a time limit); the state after its last step is not terminal.  Absent =
        terminated.  With ``bootstrap_truncated: true`` GAE then bootstraps from the value of the final observation instead of 0.
    "final_observation" -- with "truncated" only: the observation ``step`` returned for the episode's last step (the one the auto-reset
        replaces in the returned rows), a copy in the environment's own dtype (uint8 stays bytes).  ``SerialVecEnv`` and ``PipeVecEnv``
        add it; ``SyntheticVecEnv`` never reports a truncation (its terminal frame is deliberately not drawn: the key is a no-op there),
        and the worker processes' shared segment (``worker_processes: true``) has no row for it -- that combination is refused.
    action_masks(out=None) -> uint64 [W] (optional; needed by ``action_masks: true``): the invalid-action words of the observations
        LAST RETURNED by ``reset`` / ``step`` -- after an auto-reset the new episode's.  Bit j of a worker's word is set when column j
        of the concatenated policy head is allowed: the flat layout of sb3-contrib's ``action_masks()``, branch b of a MultiDiscrete
        space owning bits [off_b, off_b + A_b); bits past the last column are ignored; at most 63 columns; every branch must keep at
        least one action (the trainer raises ValueError on a word with an empty branch before it launches the step).  ``out``:
        an int64 or uint64 [W] array to fill.  A single environment offers ``action_masks() -> bool [sum A_b]`` for its current
        observation (sb3-contrib's name and layout); ``environments.pack_action_masks`` is the one place that packs.
        ``SerialVecEnv`` asks its environments, ``PipeVecEnv`` sends the ``("action_masks", None)`` command to every worker and
        then collects, ``CompositeVecEnv`` fills its parts' slices, ``SyntheticVecEnv`` draws them (``action_mask_p``).  Box spaces
        have no masks, and the worker processes' shared segment has no row for a word (refused, like ``bootstrap_truncated``).

* ``SerialVecEnv``  -- wraps in-process single envs with the upstream env API.
* ``PipeVecEnv``    -- wraps upstream-protocol ``Worker`` subprocesses (worker.py), one pipe round trip per step.
* ``environments.synthetic.SyntheticVecEnv`` implements the protocol natively.
* ``environments.device_env.CueRoomDeviceVecEnv`` / ``CommandRoomDeviceVecEnv`` / ``PathRoomDeviceVecEnv`` / ``SpotRoomDeviceVecEnv`` (the types of environments/device_types.py with
  ``device: true``) implement it over environments that live in device memory, and declare ``device_resident = True``: ``step_device(actions_dev, rows_dev, stream) -> (rewards, dones, infos)`` steps
  them from the device's action table straight into the given device rows (the trainer's streamed plans use it).
"""
import numpy as np

from environments import action_space_kind, observation_dtype, pack_action_masks


class _VecBase:
    ROW_CHUNKS = 2   # on_rows granularity: W / ROW_CHUNKS workers per notification (each notification costs the trainer ~9 us)

    def _alloc(self, out):
        return out if out is not None else np.zeros((self.num_envs,) + self.observation_space_shape, dtype=getattr(self, "observation_dtype", np.float32))

    def _notify(self, on_rows, done_upto, sent_upto):
        """Call on_rows for the complete chunks in [sent_upto, done_upto); returns the new sent_upto."""
        if on_rows is None:
            return sent_upto
        step = max(1, -(-self.num_envs // self.ROW_CHUNKS))
        while sent_upto + step <= done_upto or (done_upto == self.num_envs and sent_upto < done_upto):
            hi = min(sent_upto + step, self.num_envs)
            on_rows(sent_upto, hi)
            sent_upto = hi
        return sent_upto

    def _mask_out(self, out):
        return out if out is not None else np.zeros(self.num_envs, dtype=np.uint64)


class SerialVecEnv(_VecBase):
    def __init__(self, envs):
        self.envs = list(envs)
        self.num_envs = len(self.envs)
        e = self.envs[0]
        self.observation_space_shape = tuple(e.observation_space.shape)
        self.observation_dtype = observation_dtype(e.observation_space)
        self.action_kind = action_space_kind(e.action_space)
        self.action_space_shape = self.action_kind.shape
        self.num_actions = sum(self.action_space_shape)
        self.max_episode_steps = int(e.max_episode_steps)

    def reset(self, out=None):
        out = self._alloc(out)
        for w, e in enumerate(self.envs):
            out[w] = e.reset()
        return out

    def step(self, actions, out=None, on_rows=None):
        out = self._alloc(out)
        actions = np.asarray(actions).reshape(self.num_envs, -1)
        rewards = np.zeros(self.num_envs, dtype=np.float32)
        dones = np.zeros(self.num_envs, dtype=bool)
        infos = [None] * self.num_envs
        sent = 0
        for w, e in enumerate(self.envs):
            obs, rewards[w], dones[w], info = e.step(actions[w])      # (one row [B] per environment: one action per branch)
            if info:
                infos[w] = info
                if info.get("truncated"):
                    info["final_observation"] = np.array(obs)      # (a copy, the environment's dtype)
                obs = e.reset()
            out[w] = obs
            sent = self._notify(on_rows, w + 1, sent)
        return out, rewards, dones, infos

    def action_masks(self, out=None):
        if not all(hasattr(e, "action_masks") for e in self.envs):
            raise AttributeError("action_masks: an environment of this front-end offers no action_masks()")
        rows = np.stack([np.asarray(e.action_masks(), dtype=bool).reshape(-1) for e in self.envs])
        return pack_action_masks(rows, out=self._mask_out(out))

    def close(self):
        for e in self.envs:
            e.close()


class PipeVecEnv(_VecBase):
    """One subprocess per env, upstream (cmd, data) pipe protocol; actions are sent to all workers before any
    result is received so the environments step concurrently."""

    def __init__(self, env_config: dict, num_envs: int, first_worker_id: int = 0):
        from utils import create_env
        from worker import Worker
        probe = create_env(env_config)
        self.observation_space_shape = tuple(probe.observation_space.shape)
        self.observation_dtype = observation_dtype(probe.observation_space)
        self.action_kind = action_space_kind(probe.action_space)
        self.action_space_shape = self.action_kind.shape
        self.num_actions = sum(self.action_space_shape)
        self.max_episode_steps = int(probe.max_episode_steps)
        self._has_masks = hasattr(probe, "action_masks")
        probe.close()
        self.num_envs = num_envs
        self.workers = [Worker(env_config, worker_id=first_worker_id + w) for w in range(num_envs)]

    def reset(self, out=None):
        out = self._alloc(out)
        for wk in self.workers:
            wk.child.send(("reset", None))
        for w, wk in enumerate(self.workers):
            out[w] = self._recv(wk)
        return out

    def step(self, actions, out=None, on_rows=None):
        out = self._alloc(out)
        actions = np.asarray(actions).reshape(self.num_envs, -1)
        for w, wk in enumerate(self.workers):
            wk.child.send(("step", actions[w]))
        rewards = np.zeros(self.num_envs, dtype=np.float32)
        dones = np.zeros(self.num_envs, dtype=bool)
        infos = [None] * self.num_envs
        sent = 0
        for w, wk in enumerate(self.workers):
            obs, rewards[w], dones[w], info = self._recv(wk)
            if info:
                infos[w] = info
                if info.get("truncated"):
                    info["final_observation"] = np.array(obs)      # (a copy, the environment's dtype)
                wk.child.send(("reset", None))
                obs = self._recv(wk)
            out[w] = obs
            sent = self._notify(on_rows, w + 1, sent)
        return out, rewards, dones, infos

    def action_masks(self, out=None):
        if not self._has_masks:
            raise AttributeError("action_masks: the environment of this front-end offers no action_masks()")
        for wk in self.workers:
            wk.child.send(("action_masks", None))
        rows = np.stack([np.asarray(self._recv(wk), dtype=bool).reshape(-1) for wk in self.workers])
        return pack_action_masks(rows, out=self._mask_out(out))

    @staticmethod
    def _recv(wk):
        msg = wk.child.recv()
        if isinstance(msg, Exception):
            raise msg
        return msg

    def close(self):
        for wk in self.workers:
            try:
                wk.child.send(("close", None))
            except Exception:
                pass


class CompositeVecEnv(_VecBase):
    """Several vectorised environments side by side (workers of part p are rows [lo_p, hi_p) of every array).  ``step`` /
    ``reset`` behave like one environment over all workers; the trainer's pipelined rollout steps the ``parts`` one at a time
    (while one part is being stepped on the host the device runs the other part's forward pass).  All state lives in the
    parts, so both ways of stepping can be mixed."""

    def __init__(self, parts):
        self.parts = list(parts)
        self.bounds, lo = [], 0
        for p in self.parts:
            self.bounds.append((lo, lo + p.num_envs))
            lo += p.num_envs
        self.num_envs = lo
        e = self.parts[0]
        self.observation_space_shape = tuple(e.observation_space_shape)
        self.observation_dtype = observation_dtype(e)
        self.action_space_shape = tuple(getattr(e, "action_space_shape", None) or (int(e.num_actions),))
        self.action_kind = getattr(e, "action_kind", None) or (action_space_kind(e.action_space) if hasattr(e, "action_space") else None)
        self.num_actions = int(e.num_actions)
        self.max_episode_steps = int(e.max_episode_steps)

    def reset(self, out=None):
        out = self._alloc(out)
        for p, (lo, hi) in zip(self.parts, self.bounds):
            p.reset(out=out[lo:hi])
        return out

    def step(self, actions, out=None, on_rows=None):
        out = self._alloc(out)
        actions = np.asarray(actions)                          # [W] or [W, B]: the parts take their rows
        rewards = np.zeros(self.num_envs, dtype=np.float32)
        dones = np.zeros(self.num_envs, dtype=bool)
        infos = []
        for p, (lo, hi) in zip(self.parts, self.bounds):
            cb = None if on_rows is None else (lambda a, b, lo=lo: on_rows(lo + a, lo + b))
            _, rewards[lo:hi], dones[lo:hi], inf = p.step(actions[lo:hi], out=out[lo:hi], on_rows=cb)
            infos.extend(inf)
        return out, rewards, dones, infos

    def action_masks(self, out=None):
        out = self._mask_out(out)
        for p, (lo, hi) in zip(self.parts, self.bounds):
            p.action_masks(out=out[lo:hi])
        return out

    def close(self):
        for p in self.parts:
            p.close()


def make_vec_env(env_config: dict, num_envs: int, first_worker_id: int = 0, groups: int = 1):
    """Pick the front-end for ``env_config["type"]``.  ``groups`` > 1: a ``CompositeVecEnv`` of that many equal parts (worker
    ids stay consecutive, so every worker sees the same stream as in a single front-end)."""
    if groups > 1 and num_envs % groups == 0:
        per = num_envs // groups
        return CompositeVecEnv([make_vec_env(env_config, per, first_worker_id + g * per) for g in range(groups)])
    if env_config["type"] == "Synthetic":
        from environments.synthetic import SyntheticVecEnv
        keys = ("obs_shape", "num_actions", "max_episode_steps", "seed", "p_reward", "p_done", "pool", "copy_threads", "row_chunks", "step_cost_us", "gen_threads",
                "continuous_actions", "action_low", "action_high", "observation_levels", "observation_dtype", "action_mask_p")
        kw = {k: env_config[k] for k in keys if k in env_config}
        if "obs_shape" in kw:
            kw["obs_shape"] = tuple(kw["obs_shape"])
        return SyntheticVecEnv(num_envs, first_worker_id=first_worker_id, **kw)
    from environments.device_types import device_env_section, make_device_vec_env
    sec = device_env_section(env_config)        # (None unless the type has a device-resident front-end: environments/device_types.py)
    if sec is not None and sec["device"]:       # the rule as one HIP kernel per step (environments/device_env.py)
        return make_device_vec_env(env_config, num_envs, first_worker_id)
    if env_config.get("vectorize", "pipe") == "serial":
        from utils import create_env
        return SerialVecEnv([create_env(env_config, worker_id=first_worker_id + w) for w in range(num_envs)])
    return PipeVecEnv(env_config, num_envs, first_worker_id)
