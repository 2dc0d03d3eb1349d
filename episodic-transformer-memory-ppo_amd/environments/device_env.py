"""Device-resident vectorised environments: ``CueRoomDeviceVecEnv`` serves CueRoom (environments/cue_room_env.py is the one
definition of the rule), ``CommandRoomDeviceVecEnv`` serves CommandRoom (environments/command_room_env.py),
``PathRoomDeviceVecEnv`` serves PathRoom (environments/path_room_env.py) and ``SpotRoomDeviceVecEnv`` serves SpotRoom
(environments/spot_room_env.py) from device memory -- step, auto-reset and rendering
of all workers are ONE HIP kernel per call (csrc/device_env.hip), bit for bit the host rule.

Two ways of stepping, over the same state:

* the ``VecEnv`` protocol (``reset`` / ``step`` / ``action_masks``, vec_env.py): ``step(actions, out)`` uploads the host actions, runs
  the kernel into a device frame block and copies the frames into ``out`` -- every existing consumer works unchanged;
* ``device_resident = True`` and ``step_device(actions_dev, rows_dev, stream)``: the kernel reads the actions where the sampling
  kernel left them and writes the frames where the next step's encoder reads them; no observation byte crosses the bus.  The trainer
  takes this form in the plans that stream observations (trainer._drive_rollout_host).

Both return the step's rewards, dones and infos from result words the kernel writes into pinned host memory.  The host waits for them
on an EVENT recorded behind the launch, not on a completion word: the step's workgroups have no arrival counter (it would be the
kernel's only atomic), so a word needs a second launch behind the step (the C entry offers it), and the event behind one launch was
the shorter chain.

``DeviceVecEnv`` holds everything that is not one task's: the buffers, the pinned result words, the event wait, both ways of stepping
and the counters, and opens them (``_open``: section, library, the kernel's own refusal, buffers).  A task's class is four attributes
-- its name, its action count, the prefix of its C entries, its section reader -- a constructor with its keys, and ``_rule_of``.
"""
import numpy as np
import torch

from environments.command_room_env import command_room_section
from environments.cue_room_env import cue_room_section
from environments.path_room_env import path_room_section
from environments.spot_room_env import spot_room_section
from etm import lib as etm_lib


class DeviceVecEnv:
    device_resident = True
    observation_dtype = np.uint8
    TASK = None            # the environment type, for messages
    NUM_ACTIONS = None     # Discrete(n)
    ENTRY = None           # the C entries are ENTRY + "_supported", "_state_bytes", "_reset", "_step"
    SECTION = None         # the type's section reader (a staticmethod)

    def _rule_of(self, sec):
        """The checked section -> (the integers both entries take between ``W`` and the stream word, the arguments of the
        ``_supported`` entry, max_episode_steps); keeps the task's own keys as attributes."""
        raise NotImplementedError

    def _open(self, num_envs, first_worker_id, device, **keys):
        """Everything behind a task's constructor: the checked section, the library, the kernel's own refusal, the buffers."""
        from environments import ActionKind
        sec = self.SECTION(keys)
        if int(num_envs) < 1:
            raise ValueError(f"{type(self).__name__} needs at least one environment")
        if not torch.cuda.is_available():
            raise RuntimeError("environment.device: true needs the MI355X (the environments live in device memory): set device: false "
                               "for the host twin")
        self._etm = etm_lib.load()
        rule, supported, max_episode_steps = self._rule_of(sec)
        if not getattr(self._etm, self.ENTRY + "_supported")(*supported):
            raise ValueError(f"{self.TASK}: the kernel does not take {self.ENTRY}_supported{tuple(supported)}")
        self.num_envs = W = int(num_envs)
        self.grid, self.cell = sec["grid"], sec["cell"]
        self.max_episode_steps = int(max_episode_steps)
        side = self.grid * self.cell
        self.observation_space_shape = (3, side, side)
        self.num_actions = num_actions = self.NUM_ACTIONS
        self.action_kind = ActionKind("discrete", (num_actions,))
        self.action_space_shape = (num_actions,)
        self.stream0 = (sec["seed"] + int(first_worker_id)) & ((1 << 64) - 1)
        if self.stream0 >= 1 << 63:
            self.stream0 -= 1 << 64          # (the C entry takes the 64-bit word as int64)
        self.device = dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.frame_bytes = 3 * side * side
        self._entry_names = (self.ENTRY + "_reset", self.ENTRY + "_step")
        self._reset_entry, self._step_entry = (getattr(self._etm, name) for name in self._entry_names)
        self._state = torch.zeros(int(getattr(self._etm, self.ENTRY + "_state_bytes")(W)) // 8, dtype=torch.int64, device=dev)
        self._frames = torch.zeros((W,) + self.observation_space_shape, dtype=torch.uint8, device=dev)
        self._act_dev = torch.zeros(W, dtype=torch.int64, device=dev)
        self._act_pin = torch.zeros(W, dtype=torch.int64).pin_memory()
        # the result words, in pinned host memory: the kernel writes them in place
        self._rewards = torch.zeros(W, dtype=torch.float32).pin_memory()
        self._flags = torch.zeros(W, dtype=torch.uint8).pin_memory()
        self._returns = torch.zeros(W, dtype=torch.float32).pin_memory()
        self._lengths = torch.zeros(W, dtype=torch.int32).pin_memory()
        self._masks = torch.zeros(W, dtype=torch.int64).pin_memory()
        self._rewards_np, self._flags_np, self._returns_np = self._rewards.numpy(), self._flags.numpy(), self._returns.numpy()
        self._lengths_np, self._masks_np = self._lengths.numpy(), self._masks.numpy()
        self._words = tuple(t.data_ptr() for t in (self._rewards, self._flags, self._returns, self._lengths, self._masks))
        self._rule = (W,) + tuple(rule) + (self.stream0,)
        self._done_event = torch.cuda.Event()
        self.device_steps = 0          # calls of step_device (the trainer's fast path), for tests and tools
        self.protocol_steps = 0        # calls of step

    # ---------------------------------------------------------------- launches
    def _run(self, actions_ptr, act_stride, frames_ptr, stream):
        """One launch on ``stream`` (a torch stream), then the host waits for its result words."""
        args = self._words + (None, 0) + self._rule + (stream.cuda_stream,)
        if actions_ptr is None:
            rc = self._reset_entry(self._state.data_ptr(), frames_ptr, self.frame_bytes, *args)
        else:
            rc = self._step_entry(self._state.data_ptr(), actions_ptr, act_stride, frames_ptr, self.frame_bytes, *args)
        if rc != 0:
            etm_lib.check(rc, self._entry_names[0 if actions_ptr is None else 1])
        self._done_event.record(stream)
        self._done_event.synchronize()

    def _results(self):
        """(rewards, dones, infos) of the last step from the pinned words (copies: the next launch rewrites the words)."""
        flags = self._flags_np
        dones = (flags & 1) != 0
        infos = [None] * self.num_envs
        for w in np.flatnonzero(dones):
            info = {"reward": float(self._returns_np[w]), "length": int(self._lengths_np[w]), "success": int(flags[w] >> 2 & 1)}
            if flags[w] & 2:
                info["truncated"] = True
            infos[w] = info
        return self._rewards_np.copy(), dones, infos

    def _frames_to(self, out):
        if out is None:
            return self._frames.cpu().numpy()
        if isinstance(out, np.ndarray) and out.flags.c_contiguous and out.dtype == np.uint8:
            torch.from_numpy(out).copy_(self._frames)
        else:
            out[...] = self._frames.cpu().numpy()
        return out

    # ---------------------------------------------------------------- the VecEnv protocol
    def reset(self, out=None):
        self._run(None, 0, self._frames.data_ptr(), torch.cuda.current_stream(self.device))
        return self._frames_to(out)

    def step(self, actions, out=None, on_rows=None):
        a = np.asarray(actions).reshape(self.num_envs, -1)[:, 0]
        top = self.num_actions - 1
        if a.min() < 0 or a.max() > top:
            raise ValueError(f"{self.TASK}: action {int(a[(a < 0) | (a > top)][0])} is outside Discrete({self.num_actions})")
        self._act_pin.numpy()[:] = a
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):
            self._act_dev.copy_(self._act_pin, non_blocking=True)
        self._run(self._act_dev.data_ptr(), 1, self._frames.data_ptr(), stream)
        self.protocol_steps += 1
        out = self._frames_to(out)
        if on_rows is not None:
            on_rows(0, self.num_envs)
        rewards, dones, infos = self._results()
        return out, rewards, dones, infos

    def action_masks(self, out=None):
        """The words of the frames last written (by ``reset``, ``step`` or ``step_device``)."""
        if out is None:
            return self._masks_np.view(np.uint64).copy()
        out.view(np.uint64)[...] = self._masks_np.view(np.uint64)
        return out

    # ---------------------------------------------------------------- the device-resident form
    def step_device(self, actions_dev, rows_dev, stream=None):
        """``actions_dev``: device int64 [W] or [W, 1] (a row stride is honoured), the rows the sampling kernel wrote; ``rows_dev``: a
        device uint8 tensor [W, 3, S, S] (contiguous) or the address of W contiguous frames -- rows [lo, hi) of a staging row;
        ``stream``: the torch stream the launch is enqueued on (None: the current one).  -> (rewards, dones, infos)."""
        if actions_dev.dtype != torch.int64 or actions_dev.shape[0] != self.num_envs:
            raise ValueError("step_device: actions_dev is the device int64 [W] / [W, 1] table of the sampling kernels")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rows = rows_dev.data_ptr() if hasattr(rows_dev, "data_ptr") else int(rows_dev)
        self._run(actions_dev.data_ptr(), actions_dev.stride(0), rows, stream)
        self.device_steps += 1
        return self._results()

    def close(self):
        return None


class CueRoomDeviceVecEnv(DeviceVecEnv):
    TASK, NUM_ACTIONS, ENTRY, SECTION = "CueRoom", 4, "etm_cue_room", staticmethod(cue_room_section)

    def __init__(self, num_envs, grid=7, cell=12, cue_steps=2, max_episode_steps=32, seed=0, first_worker_id=0, device=None):
        self._open(num_envs, first_worker_id, device, grid=grid, cell=cell, cue_steps=cue_steps, max_episode_steps=max_episode_steps,
                   seed=seed)

    def _rule_of(self, sec):
        self.cue_steps = sec["cue_steps"]
        return (sec["grid"], sec["cell"], sec["cue_steps"], sec["max_episode_steps"]), (sec["grid"], sec["cell"]), sec["max_episode_steps"]


class CommandRoomDeviceVecEnv(DeviceVecEnv):
    TASK, NUM_ACTIONS, ENTRY, SECTION = "CommandRoom", 5, "etm_command_room", staticmethod(command_room_section)

    def __init__(self, num_envs, grid=7, cell=12, command_count=8, show_steps=1, gap_steps=1, seed=0, first_worker_id=0, device=None):
        self._open(num_envs, first_worker_id, device, grid=grid, cell=cell, command_count=command_count, show_steps=show_steps,
                   gap_steps=gap_steps, seed=seed)

    def _rule_of(self, sec):
        self.command_count, self.show_steps, self.gap_steps = K, show, gap = sec["command_count"], sec["show_steps"], sec["gap_steps"]
        return (sec["grid"], sec["cell"], K, show, gap), (sec["grid"], sec["cell"], K), K * (show + gap) + K


class PathRoomDeviceVecEnv(DeviceVecEnv):
    TASK, NUM_ACTIONS, ENTRY, SECTION = "PathRoom", 4, "etm_path_room", staticmethod(path_room_section)

    def __init__(self, num_envs, grid=7, cell=12, path_moves=16, max_episode_steps=64, seed=0, first_worker_id=0, device=None):
        self._open(num_envs, first_worker_id, device, grid=grid, cell=cell, path_moves=path_moves, max_episode_steps=max_episode_steps,
                   seed=seed)

    def _rule_of(self, sec):
        self.path_moves = M = sec["path_moves"]
        return (sec["grid"], sec["cell"], M, sec["max_episode_steps"]), (sec["grid"], sec["cell"], M), sec["max_episode_steps"]


class SpotRoomDeviceVecEnv(DeviceVecEnv):
    TASK, NUM_ACTIONS, ENTRY, SECTION = "SpotRoom", 5, "etm_spot_room", staticmethod(spot_room_section)

    def __init__(self, num_envs, grid=7, cell=12, spotlights=2, light_steps=2, spot_period=2, health=5, max_episode_steps=64, seed=0,
                 first_worker_id=0, device=None):
        self._open(num_envs, first_worker_id, device, grid=grid, cell=cell, spotlights=spotlights, light_steps=light_steps,
                   spot_period=spot_period, health=health, max_episode_steps=max_episode_steps, seed=seed)

    def _rule_of(self, sec):
        self.spotlights, self.light_steps, self.spot_period, self.health = N, light, period, H = (
            sec["spotlights"], sec["light_steps"], sec["spot_period"], sec["health"])
        G, P, limit = sec["grid"], sec["cell"], sec["max_episode_steps"]
        return (G, P, N, light, period, H, limit), (G, P, N, H), limit
