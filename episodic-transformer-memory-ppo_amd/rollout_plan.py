"""Which form of the rollout step runs (``RolloutPlan``, decided once by ``plan_rollout``) and the state of one worker group
(``WorkerGroup``).  Nothing here touches the device at import; ``plan_rollout`` never does.

The 12 plans that exist are tabulated in DESIGN.md (section 4, Rollout); tests/test_host_logic.py enumerates them."""
from dataclasses import dataclass

import torch


@dataclass(frozen=True)
class RolloutPlan:
    """The host-side form of a rollout; every field False (``polite_wait`` aside) is the eager path."""
    graph: bool = False           # the step of a group is replayed from captured HIP graphs
    stream_obs: bool = False      # rows of observation t + 1 go into row t + 1 of the staging array while the environments still step
    host_flag: bool = False       # the sampling kernel writes the step counter into host memory (no event); the step is ONE graph
    own_stream: bool = False      # rows travel on the group's stream, the (step, slot) block is read in place from pinned memory
    direct_rows: bool = False     # the environments write the rows straight into the staging array in device memory (large BAR)
    direct_launch: bool = False   # hipGraphLaunch through the library instead of the framework's replay()
    native: bool = False          # the kernel library's driver runs the per-step loop (worker processes)
    polite_wait: bool = False     # the trainer thread sleeps through most of a flag wait (etm/hostcpu.py)


def plan_rollout(*, graph, stream_observations, host_flag_actions, direct_observation_rows, kv_cache, fused_encoder, heads_fusable,
                 several_groups, worker_processes, raw_graph_exec, large_bar, polite_wait) -> RolloutPlan:
    """The plan for the config keys ``hip_graph_rollout`` (``graph``), ``stream_observations``, ``host_flag_actions``,
    ``direct_observation_rows`` and what the model, the groups and the host offer.  ``several_groups``: every group has its own
    stream.  ``raw_graph_exec``: CUDAGraph.raw_cuda_graph_exec exists (torch >= 2.8).  ``large_bar``: a callable (it runs a device
    self-test), asked only when every other condition for direct rows holds."""
    if not graph:
        return RolloutPlan(polite_wait=polite_wait)
    fusable = kv_cache and heads_fusable
    if several_groups and not fusable:
        raise RuntimeError("rollout_groups > 1 needs the K/V cache (set rollout_groups: 1)")
    stream_obs = stream_observations and kv_cache and fused_encoder
    # host_flag_actions (default on): the sampling kernel stores the actions and then the step counter into pinned memory
    # and the host spins on the counter -- no event between the action hand-over and the rest of the step, so a step of a
    # group is ONE captured graph (one launch) instead of head + event + tail (measured: 287 -> 279 us per step)
    host_flag = host_flag_actions and fusable
    # With a stream per group (the pipelined default) the observation rows of a group go to the device on the GROUP's stream
    # -- stream order alone puts them before the step that reads them -- and the step's window kernel reads the
    # (episode step, slot) block straight from pinned host memory: no upload of that block, no event between an upload
    # stream and the step (each of those was a few us on the critical path of every step).
    own_stream = stream_obs and several_groups
    # one captured graph per step on the group's own stream, nothing to wait for: hipGraphLaunch through the library,
    # without the framework's stream switches around the replay (~6 us of every group's step on the host)
    direct_launch = host_flag and several_groups and raw_graph_exec
    # native rollout driver (worker processes): needs the flag hand-over, streamed observations on the groups' own streams and
    # the (step, slot) block read in place -- ONE predicate for "go words in the segment", "workers held spinning", "sequence
    # restarted" and "etm_rollout_drive called"
    native = worker_processes and own_stream and direct_launch
    # direct observation rows (in-process environments): the front-end writes the rows of step t + 1 straight into
    # their row of the staging array in DEVICE memory (large BAR: the hipMalloc pointer is a host address) -- no pinned
    # intermediate, no copy-engine transfer (677 KB per group and step at 3x84x84: ~20 us of the step's critical path) and no
    # runtime call; etm_host_store_fence (sfence + the device's HDP flush register) sits between the rows and the launch.
    # `direct_observation_rows: false`, a device without large BAR or a failed self-test: uploads.
    direct_rows = bool(own_stream and host_flag and not worker_processes and direct_observation_rows and large_bar())
    return RolloutPlan(True, stream_obs, host_flag, own_stream, direct_rows, direct_launch, native, polite_wait)


class WorkerGroup:
    """Device / pinned state of the workers [lo, hi) for one rollout step (see ``rollout_groups``).  The full-width group (eager
    path, single-group graph path) aliases the trainer's buffers; the pipelined groups own what cannot be a contiguous slice of them."""

    def __init__(self, tr, lo, hi, env, full, upload):
        dev, Wg, B = tr.device, hi - lo, tr._action_width
        self.lo, self.hi, self.W, self.env, self.full = lo, hi, Wg, env, full
        self.obs_pin, self.act_pin = tr._obs_pin[lo:hi], tr._act_pin[lo:hi]
        self.obs_np = tr.obs[lo:hi]
        acts = self.act_pin.numpy()
        self.acts_host = acts[:, 0] if B == 1 and tr.box is None else acts    # [Wg] for one branch, [Wg, B] multi-discrete, [Wg, A] Box
        self.obs_dev, self.mask_t, self.win_t, self.act_dev = tr._obs_dev[lo:hi], tr._mask_t[lo:hi], tr._win_t[lo:hi], tr._act_dev[lo:hi]
        self.kv = tr._kv_cache[lo:hi]
        # (episode step, episode slot) of the workers: the full-width group's block IS the trainer's, the host truth
        self.ss_pin = tr._ss_pin if full else torch.zeros((2, Wg), dtype=torch.int64).pin_memory()
        self.ss_dev = tr._ss_dev if full else torch.zeros((2, Wg), dtype=torch.int64, device=dev)
        # action_masks: the group's words of the trainer's pinned block, which the sampling kernels read in place, and of its device
        # twin (measurement only: PPOTrainer._mask_in_place); contiguous slices; None without the key
        self.am_pin = None if tr._am_pin is None else tr._am_pin[lo:hi]
        self.am_dev = None if tr._am_dev is None else tr._am_dev[lo:hi]
        # previous_step_input: the group's entries of the trainer's pinned block of last rewards (read in place by the rows kernel in
        # front of the step; a contiguous slice); None without the key or its reward
        self.rw_pin = None if tr._rw_pin is None else tr._rw_pin[lo:hi]
        self.item = torch.zeros((tr.num_blocks, Wg, tr.embed_dim), dtype=torch.float32, device=dev)      # the step's new memory items, block-major
        self.t_dev = torch.zeros((), dtype=torch.int64, device=dev)      # step counter, incremented by the sampling kernel
        self.t_row = torch.zeros((), dtype=torch.int64, device=dev)      # staging row of the step, for its tail
        self.ids = torch.arange(Wg, dtype=torch.int64, device=dev)
        self.act_ready, self.up_done = torch.cuda.Event(), torch.cuda.Event()
        # the pipelined groups replay on a stream each; the full-width group on the caller's
        self.stream = None if full else torch.cuda.Stream(device=dev)
        self.use_flag(torch.zeros((1,), dtype=torch.int64).pin_memory().numpy())
        self.ss_np = self.ss_pin.numpy()
        self._ss_all = tr._ss_pin.numpy()[:, lo:hi]       # this group's columns of the trainer's (step, slot) block: the host truth
        self.slot_dev = self.ss_dev[1]
        # (episode step, slot) as LATCHED by the head of a step for its tail: the host uploads the next step's block on the
        # upload stream while the tail (bank / cache writes under env.step) may still be running, and only the group's own
        # stream orders tail t before head t + 1 -- so the tail must not read the uploaded block itself
        self.ss_latch = torch.zeros((2, Wg), dtype=torch.int64, device=dev)
        self.step_l, self.slot_l = self.ss_latch[0], self.ss_latch[1]
        # observation rows: pinned source of the group's rows, its rows of staging row 0, bytes per row / per staging row
        self._upload, self.row_bytes = upload, tr._obs_pin[0].numel() * tr._obs_pin.element_size()      # (float32 or uint8 rows)
        self.rows_src = tr._obs_pin.data_ptr() + lo * self.row_bytes
        self.stage0 = tr._stage["obs"].data_ptr() + lo * self.row_bytes
        self._stage_pitch = tr.num_workers * self.row_bytes
        self.obs_stream = None        # raw handle of the stream the rows travel on (the group's own or the shared upload stream)
        # what the capture of the group's step leaves behind
        self.graphs = None            # (head, tail or None)
        self.graph_exec = None        # raw handle of the one-graph step (plan.direct_launch)
        self.h_part = None            # lin_hidden's K-slice partial sums (fixed address)
        self.rf_scratch = None        # the step kernel's scratch (launch counter, tags, slots, error word) ...
        self.rf_scratch_kind = None   # ... laid out for the group form (True) or the per-worker form (False)
        self.group_kernel = False     # the step runs the group form of the step kernel
        self.tail_in_kernel = False   # the step kernel writes the bank and cache rows itself

    def take_state(self):
        """(episode step, slot) of the group's workers, after the host bookkeeping of a step -> the group's pinned block."""
        if not self.full:
            self.ss_np[:] = self._ss_all

    def use_flag(self, word):
        """``word`` (numpy, one int64 in host memory the device can write) receives the step counter from the sampling kernel."""
        # the group's private pinned word, or -- native driver -- the shared segment's go word the workers spin on; its address is captured
        self.flag_pin = torch.from_numpy(word)
        self.flag_np = self.flag_pin.numpy()

    def restart(self):
        self.t_dev.zero_()
        self.flag_np[0] = 0

    def upload_rows(self, t, a, b):
        """Pinned rows [a, b) of the group -> row ``t`` of the staging array, on the group's observation stream."""
        rb = self.row_bytes
        self._upload(self.stage0 + t * self._stage_pitch + a * rb, self.rows_src + a * rb, (b - a) * rb, self.obs_stream)
