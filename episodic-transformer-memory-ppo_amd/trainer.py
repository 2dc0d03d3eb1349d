"""PPO trainer with TransformerXL episodic memory on one MI355X per process.

Keeps upstream's ``PPOTrainer`` surface (trainer.py:17 ctor, :101 run_training, :145 _sample_training_data,
:227 get_last_value, :239 _train_epochs, :258 _train_mini_batch, :364 close) and its bookkeeping semantics --
mask / window-index tables (bit-exact, :78, :88-90), per-step window rule (:165-166), the different window of
``get_last_value`` (:230-236, quirk Q5), episode hand-over on ``done`` (:195-213) -- while the data path is redesigned
for the GPU:

* rollout state (episode bank, tables, buffer) is HBM-resident; per step the observation rows are streamed from pinned
  memory into the staging array while the environments still step and the actions are stored into pinned memory by the
  sampling kernel (upstream: one ``.cpu()`` per worker, :190); the step itself is two captured HIP graphs;
* memory windows are never gathered: the attention kernel reads the bank through (slot, row) indices;
* GAE and the PPO loss (+ its backward) are single fused kernels; loss statistics stay on the device and are
  fetched once per update (upstream: 6 host syncs per minibatch, :318-323); the whole minibatch step (gather, forward,
  loss, backward, clip, AdamW) is one captured HIP graph with device-resident schedules;
* data parallelism (absent upstream): ``dp`` all-reduces (sums) one flat gradient bucket with RCCL between ``backward()``
  and gradient clipping (:310-311) -- the division by the world size rides in the clip coefficient -- and merges advantage
  statistics so normalisation is over the global minibatch.

* time-limit truncations (absent upstream; ``bootstrap_truncated: true``): an episode the environment reports as only cut is
  bootstrapped from the value of its final observation -- records in ``_hand_over_episodes``, one batched pass after the rollout
  (``_bootstrap_pass``), the select form of the GAE kernel.

There is no CPU path: constructing the trainer without a HIP device raises.
"""
import os
import sys
import time
from collections import deque
from functools import partial

import numpy as np
import torch

# Four worker groups want four pairs of streams (upload + step graph) running CONCURRENTLY; the HIP runtime maps streams onto its
# hardware queues, four by default.  With 4 queues four groups serialise (rollout 0.161 s per update instead of 0.087 s; two
# groups: 0.094 s), so "auto" forms two groups; four remain available as an explicit ``rollout_groups: 4``.
def default_rollout_groups(num_workers: int, min_group: int) -> int:
    """``rollout_groups: auto``: 2 when the groups keep ``min_group`` workers, else 1."""
    if num_workers % 2 == 0 and num_workers // 2 >= min_group:
        return 2
    return 1


from buffer import Buffer
from environments import action_space_kind, branch_bit_masks, empty_mask_branches, valid_action_share
from environments.vec_env import make_vec_env
from etm import lib as etm_lib
from etm import ops
from etm.ops import WindowSpec
from etm.optim import AdaptiveLr, FlatAdamW, KlGate
from model import ActorCriticModel, IndexedObservations, PreviousStep
from utils import kl_penalty_step, obs_reconstruction_coef, polynomial_decay, process_episode_info, target_kl_rows, attention_statistics_summary
from rollout_plan import RolloutPlan, WorkerGroup, plan_rollout
from checkpoint import segment_first_worker_id
# the optional keys: their checks, the order in which they refuse and what they come to live in run_settings.py; the names stay
# importable from here (tests, tools)
from run_settings import (RunSettings, world_of, check_kernel_shapes, check_box_policy, check_byte_observation_transport,      # noqa: F401
                          check_truncation_transport, check_action_mask_config, check_evaluation_config, check_normalization_config,
                          check_target_kl_config, check_adaptive_lr_config, check_kl_estimator_config, check_exact_kl_config,
                          check_kl_penalty_config, check_attention_statistics_config)
from trainer_parts import _CheckpointResume, _DataParallelStep, _NativeRolloutDrive, _RunOutputs


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def _make_writer(run_id):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except Exception:
        return _NullWriter()
    os.makedirs("./summaries", exist_ok=True)
    return SummaryWriter("./summaries/" + run_id + time.strftime("/%Y%m%d-%H%M%S/"))


def build_window_tables(memory_length: int, max_episode_length: int):
    """Attention-mask table [L, L] and sliding-window index table [T, L] (upstream trainer.py:78, :88-90).

    Integer/0-1 valued, built on the host: row s of the index table is the window used at episode step s
    ([0..L-1] while s < L-1, then [s-L+1..s]); mask row r has its first r entries set.
    """
    L, T = int(memory_length), int(max_episode_length)
    if T < L:
        raise ValueError(f"max_episode_steps ({T}) must be >= memory_length ({L})")
    mask = torch.tril(torch.ones((L, L), dtype=torch.float32), diagonal=-1)
    first = torch.clamp(torch.arange(T, dtype=torch.int64) - (L - 1), min=0)
    indices = first.unsqueeze(1) + torch.arange(L, dtype=torch.int64).unsqueeze(0)
    return mask, indices


def time_major(table, src):
    """The host table ``src`` [W, S(, B)] in the layout and type of the fixed-address device table ``table`` [S, W(, B)]."""
    x = torch.as_tensor(np.asarray(src), dtype=table.dtype)
    return x.reshape((table.shape[1], table.shape[0]) + tuple(table.shape[2:])).transpose(0, 1)


class PPOTrainer(_DataParallelStep, _NativeRolloutDrive, _RunOutputs, _CheckpointResume):
    def __init__(self, config: dict, run_id: str = "run", device: torch.device = None, env=None, dp=None,
                 first_worker_id: int = 0, tensorboard: bool = True, resume: str = None) -> None:
        """``resume``: the path of a training checkpoint (``save_checkpoint``) to continue from: the file is read and verified first,
        the environments are built with the worker ids of the next training segment, and the state is loaded in place once everything
        exists (``load_checkpoint`` without a second restart) -- also with ``worker_processes: true``.

        Seven stages; within and across them every statement that allocates device or pinned memory, draws from a generator, creates a
        stream or an event or touches the environment keeps its place in the order (keyed runs stay bit-equal, the allocator sees the
        same requests)."""
        resumed, first_worker_id = self._init_settings(config, run_id, device, env, dp, first_worker_id, tensorboard, resume)
        self._init_environment(env, first_worker_id)
        self._init_learner()
        self._init_pinned_staging(resumed, first_worker_id)
        self._init_step_operands()
        self._init_kv_cache_and_replays()
        self._init_worker_groups_and_tables()
        if resumed is not None:
            self._load_state(resumed, str(resume), restart=False)

    def _init_settings(self, config, run_id, device, env, dp, first_worker_id, tensorboard, resume):
        """Stage 1: the device, the library, the optional keys (``self.settings``: run_settings.RunSettings, stage one -- every refusal
        the config alone gives, in the order stated there) and the state a checkpoint carries over.  -> (the verified checkpoint or
        None, the first worker id of this training segment)."""
        if device is None:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("PPOTrainer needs an MI355X (HIP) device: this build has no CPU training path "
                               "(the CPU restatement under oracle/ is test infrastructure only)")
        self._etm = etm_lib.load()  # fail loudly if the kernels are not built
        # (placement of the step kernel's workgroups: a worker's whole team on one XCD, the library's default; the member-per-XCD map
        # measured equal -- 111.9 vs 112.2 us per step graph -- and is a kernel-level test only since round 6)
        etm_lib.check(self._etm.etm_rollout_trxl_set_placement(0), "etm_rollout_trxl_set_placement")
        self.config = config
        self.device = device
        self._dev_index = device.index if device.index is not None else torch.cuda.current_device()
        self.run_id = run_id
        self.dp = dp
        self.num_workers = config["n_workers"]
        self.lr_schedule = config["learning_rate_schedule"]
        self.beta_schedule = config["beta_schedule"]
        self.cr_schedule = config["clip_range_schedule"]
        t = config["transformer"]
        self.memory_length, self.num_blocks, self.embed_dim = t["memory_length"], t["num_blocks"], t["embed_dim"]
        self._world = world_of(dp)
        self.settings = RunSettings.before_environment(config, self._world, env, resume is not None)
        # training state that a checkpoint carries over (trainer_parts._CheckpointResume): completed updates, the training segment (the
        # number of resumes so far; its environments' worker ids start at segment_first_worker_id), the last episodes' infos
        self.update_index, self.segment, self._episode_infos = 0, 0, deque(maxlen=100)
        self._base_worker_id, self._env_supplied = int(first_worker_id), env is not None
        resumed = None
        if resume is not None:
            resumed = self._read_verified(resume)       # (before anything is built: a damaged file costs nothing)
            self.segment = int(resumed["segment"]) + 1
            first_worker_id = segment_first_worker_id(first_worker_id, self.segment)
        self.writer = _make_writer(run_id) if tensorboard else _NullWriter()
        return resumed, first_worker_id

    def _init_environment(self, env, first_worker_id):
        """Stage 2: the worker groups' number, the host CPU plan, the environments (``env``: a supplied front-end or None) and, with what
        they say about observations and actions, stage two of the settings -- the refusals that need the environment."""
        config = self.config
        # environments (batched front-end over the upstream per-worker protocol)
        # rollout_groups (default "auto": 2): the workers are stepped as that many groups in a software
        # pipeline -- while the host steps one group's environments the device runs the other groups' forward passes (small step
        # graphs overlap almost perfectly on the GPU: 117 us per round of two, 122 us per round of four vs 112 us each,
        # tools/rollout_profile.py; config 3: rollout 0.094 s per update with two groups, 0.087 s with four).  Needs an environment front-end made
        # of parts (make_vec_env(groups=...)); an externally supplied environment is stepped as one group.
        # Groups of fewer than 8 workers are not formed: they do not pay off, and one intermittent mismatch was seen with
        # groups of 2 workers while both groups' graphs had been captured on torch's shared capture stream, i.e. with ONE
        # BLAS scratch buffer between them (split-K solutions at a handful of rows per GEMM); the graphs are captured per
        # group stream now (_capture_step_graph), the threshold stays until that has been re-measured.
        min_group = int(config.get("rollout_min_group_size", 8))
        n_groups = config.get("rollout_groups", "auto")
        n_groups = default_rollout_groups(self.num_workers, min_group) if n_groups == "auto" else int(n_groups)
        if n_groups < 1 or self.num_workers % n_groups != 0 or self.num_workers // n_groups < min_group:
            n_groups = 1
        if config.get("rollout_groups", "auto") == "auto" and os.environ.get("ETM_QUIET") != "1":
            print(f"[etm] rollout worker groups: {n_groups} (rollout_groups: auto)", file=sys.stderr, flush=True)
        # round 5: the rank's host CPU share (affinity mask, cgroup CPU quota, ranks per node) against the threads a rollout keeps
        # busy -- trainer thread on the action flag, observation-copier helpers, worker processes (etm/hostcpu.py).  With room to
        # spare nothing changes; without it the helpers sleep between jobs, the copier / the worker processes shrink to what fits and
        # the trainer thread sleeps through most of the expected device time before it spins.  `host_cpu_plan: false` keeps the
        # configured values whatever the host looks like.
        from etm import hostcpu
        env_cfg = dict(config["environment"])
        # the threads that write a step's observation rows: the copier's (frame ring) or the generator pool's (pool: 0, fresh draws)
        row_threads = ("gen_threads" if int(env_cfg.get("pool", 64)) == 0 else "copy_threads") if env_cfg.get("type") == "Synthetic" else None
        self._host_plan = hostcpu.plan_host_threads(copy_threads=int(env_cfg.get(row_threads, 1)) if row_threads else 1,
                                                    worker_processes=self.settings.worker_processes,
                                                    num_envs=self.num_workers, envs_per_process=int(config.get("envs_per_process", 1)),
                                                    groups=n_groups, quiet=not config.get("host_cpu_plan", True))
        if not config.get("host_cpu_plan", True):
            self._host_plan.update(copy_threads=int(env_cfg.get(row_threads, 1)) if row_threads else 1, copier_spin=True, polite_wait=False,
                                   envs_per_process=int(config.get("envs_per_process", 1)), worker_spin=True, reason="host_cpu_plan: false")
        if row_threads and row_threads in env_cfg:
            env_cfg[row_threads] = self._host_plan["copy_threads"]
        if not self._host_plan["copier_spin"]:
            from environments import synthetic as _syn
            _syn.set_copier_spin(False)
        if self._host_plan["polite_wait"]:
            hostcpu.set_timer_slack_ns(1000)
        self._flag_wait_ema = 0.0
        ops.set_ln_grad_kernel(config.get("fused_ln_grad", True))      # (true / "outputs": from the window passes' outputs; "rows": round 5's pass over the window rows; false: the generic dX kernel -- tested options)
        # worker_processes (round 4; upstream trainer.py:62-66, worker.py): the environments live in worker PROCESSES over one shared,
        # HIP-registered segment (environments/shm_env.py): they take their actions straight from the device and step concurrently;
        # the per-step host loop is then the native driver of the kernel library (etm_rollout_drive) -- see _sample_training_data
        self._shm_env = None
        if self.settings.worker_processes:
            from environments.shm_env import ShmVecEnv
            self._shm_env = ShmVecEnv(env_cfg, self.num_workers, first_worker_id, groups=n_groups,
                                      envs_per_proc=self._host_plan["envs_per_process"], steps_per_rollout=config["worker_steps"],
                                      spin=self._host_plan["worker_spin"])
            env = self._shm_env
        self.env = env if env is not None else make_vec_env(env_cfg, self.num_workers, first_worker_id, groups=n_groups)
        self._env_cfg, self._env_groups = env_cfg, n_groups      # (the evaluator rebuilds its environments from these)
        self._evaluator = None            # evaluation.Evaluator, allocated by the first evaluate()
        self._draw_generator = None       # the rollout's draws come from torch's generator of the device (None) or from this one
        obs_shape = tuple(self.env.observation_space_shape)
        self.observation_space = type("Space", (), {"shape": obs_shape})()
        # uint8 image observations stay bytes from the environment's row to the first encoder layer's loads (byte k stands for
        # float32(k) / float32(255)): the environment says so (``observation_dtype``, or else ``observation_space.dtype``)
        from environments import observation_dtype as _observation_dtype
        self.observation_dtype = torch.uint8 if _observation_dtype(self.env) == np.uint8 else torch.float32
        # one branch per action dimension, from the environment (environments.action_space_shape: Discrete(n) -> (n,), MultiDiscrete
        # -> nvec); Discrete is upstream's single branch (trainer.py:47)
        self.action_space_shape = tuple(int(a) for a in getattr(self.env, "action_space_shape", None) or (self.env.num_actions,))
        # Box (continuous) spaces: a diagonal Gaussian policy over A = action_space_shape[0] dimensions (float action tables, the
        # environment receives the actions clipped to its bounds); None for Discrete / MultiDiscrete
        kind = getattr(self.env, "action_kind", None)
        if kind is None and hasattr(self.env, "action_space"):
            kind = action_space_kind(self.env.action_space)
        self.box = kind if kind is not None and kind.is_box else None
        self.max_episode_length = self.env.max_episode_steps
        # the environment's front-end, the observations, the width of the policy head and the kind of policy are known now
        s = self.settings = self.settings.with_environment(self.env, obs_shape, self.observation_dtype, self.action_space_shape, self.box)
        # action_masks
        self._masked = s.masked
        self.last_valid_action_share = None       # mean share of allowed actions in the last rollout's words (None without the key)
        # previous_step_input: {"action", "reward"} or None
        self._prev_cfg = s.prev
        # kl_estimator "analytic": the four Gaussian sampling sites stage the means, the buffer carries them and a snapshot of the
        # log-std, the Gaussian heads + loss kernel reduces the exact KL into stats[4].  exact_kl: a Box policy takes exactly that path; a
        # categorical one (masked or not) stages every column's log-prob at the four categorical sampling sites, the buffer carries the
        # rows, the categorical loss kernels reduce the exact KL into stats[4].  kl_penalty implies the exact KL's plumbing (the penalty is
        # coef times the very number that column 4 then holds).  (run_settings.kl_plumbing)
        self._kl_analytic, self._kl_exact_cat = s.kl_analytic, s.kl_exact_cat
        # obs_reconstruction: the schedule of the auxiliary loss's coefficient, or None
        self._recon = s.recon

    def _init_learner(self):
        """Stage 3: the per-feature device words, the buffer, the model, the optimiser and what hangs on them."""
        config, device, dp, s = self.config, self.device, self.dp, self.settings
        # kl_penalty: the coefficient lives in ONE device float32 at a fixed address: the loss kernels read it in place, in eager steps and
        # in captured graphs alike; the host writes it between updates only (_adapt_kl_penalty).  ``last_kl_penalty``: what the last
        # update used and decided (None without the key: nothing is allocated)
        self._kl_pen, self._kl_coef, self.last_kl_penalty = s.kl_penalty, None, None
        if self._kl_pen is not None:
            self._kl_coef = torch.full((1,), self._kl_pen["coef"], dtype=torch.float32, device=device)
        # obs_reconstruction: the coefficient lives in ONE device float32 at a fixed address that the fused last layer + loss kernel reads
        # in place, in eager steps and captured graphs alike; the host writes it once per update, outside every graph (_train_epochs).
        # Every step files its (unscaled) reconstruction loss in a device table of its own under a device counter; the eight statistics
        # columns are untouched.  ``last_obs_reconstruction``: {"loss", "coef"} of the last update (None without the key: nothing is
        # allocated)
        self._recon_coef = self._recon_tab = self._recon_row = self.last_obs_reconstruction = None
        if self._recon is not None:
            self._recon_coef_host = obs_reconstruction_coef(self._recon, 0)
            self._recon_coef = torch.full((1,), self._recon_coef_host, dtype=torch.float32, device=device)
            self._recon_tab = torch.zeros(max(1, int(config["epochs"]) * int(config["n_mini_batch"])), dtype=torch.float32, device=device)
            self._recon_row = torch.zeros(1, dtype=torch.long, device=device)

        if config.get("tunable_gemm", os.environ.get("ETM_TUNABLE_GEMM", "1") != "0"):
            # let PyTorch pick the fastest hipBLASLt / rocBLAS solution per GEMM shape (the small [N, D] x [D, D] products around
            # the kernels are far from the libraries' default heuristics: -5 % optimisation time, -14 us per rollout step);
            # every shape is met in the eager warm-up steps, i.e. before any graph capture.  fp32 in, fp32 out: only the
            # summation order can differ.
            try:
                import torch.cuda.tunable as tunable
                tunable.enable(True)
                tunable.tuning_enable(True)
                # results file (written by the library at exit) goes to the temp directory, not the working directory
                # one results file per rank: data-parallel ranks tune independently and must not write the same file
                rank_tag = "" if dp is None else f"_rank{dp.rank}"
                tunable.set_filename(os.path.join(os.environ.get("TMPDIR", "/tmp"), f"etm_tunableop_results{rank_tag}.csv"), True)
                tunable.set_max_tuning_duration(int(os.environ.get("ETM_TUNABLE_MS", 30)))
                tunable.set_max_tuning_iterations(int(os.environ.get("ETM_TUNABLE_ITERS", 20)))
            except Exception as exc:        # an older / newer torch without this API: run with the default heuristics
                print(f"[trainer] per-shape GEMM tuning not available ({exc})")
        box = self.box is not None
        # entries per worker of the action tables: one per branch, or the A dimensions of a Box
        self._action_width = self.action_space_shape[0] if box else len(self.action_space_shape)
        self.buffer = Buffer(config, self.observation_space, self.action_space_shape, self.max_episode_length, device, continuous=box,
                             observation_dtype=self.observation_dtype)
        self.model = ActorCriticModel(config, self.observation_space, self.action_space_shape, self.max_episode_length,
                                      continuous=box).to(device)
        self.model.train()
        self.model.graph_refresh = bool(config.get("hip_graph_rollout", True))      # (refresh_rollout_weights as a graph replay from its third call on)
        if self.dp is not None:
            self.dp.broadcast_parameters(self.model)
        self.params = [p for _, p in self.model.arena_parameters()]      # (a Box policy's policy_log_std last)
        if self._kl_analytic:
            self.buffer.log_std_source = self.model.policy_log_std       # (prepare_batch_dict snapshots it once per update)
        # The optimisation step of one minibatch (gather, forward, loss, backward, clipping, AdamW) is captured in a HIP graph
        # after two eager warm-up steps and replayed for every other minibatch of the run: the host then issues one launch
        # per minibatch instead of ~280.  lr / clip range / entropy coefficient live on the device so that their schedules
        # keep working under replay.  (Data-parallel runs replay two graphs around the eager RCCL all-reduce of the bucket.)
        self._use_train_graph = bool(config.get("hip_graph_train", True))
        self._train_graph = None
        self._train_warm = 0
        self._obs_train = None
        if self._use_train_graph:
            self._dyn = torch.zeros(2, dtype=torch.float64, device=device)      # (clip range, entropy coefficient)
            self._sched_host = [None, None, None]   # (lr, clip, beta) currently on the device
            self.profile_sample_every = 0     # bench.py: run every k-th minibatch eagerly so that per-kernel events exist
            self._mb_counter = 0
        # AdamW (torch defaults, like upstream's optim.AdamW(parameters, lr)) + global-norm clipping on flat arenas: parameters,
        # gradients and both moments share one layout, the step is two launches (etm/optim.py, csrc/optim.hip); lr and the step
        # counter live on the device.  The gradient arena is the one bucket the data-parallel all-reduce sums.
        self.optimizer = FlatAdamW(self.params, lr=self.lr_schedule["initial"])
        self.flat_grads = self.optimizer.flat_grads[: self.optimizer.total]
        self._grad_views = self.optimizer.grad_views
        if self.dp is not None:
            self.dp.flat = self.flat_grads
        self._build_grad_groups()
        # attention_statistics: the table every grad-enabled forward_window of the update adds to (ops.AttentionStatistics: fixed
        # addresses, so the captured step holds them), zeroed at the start of every update and read once behind its read-back; the
        # workspace takes any batch up to the whole buffer.  Not trainer state, not in the checkpoint.  ``last_attention_statistics``:
        # utils.attention_statistics_summary of the last update's table -- its ``rows`` say how many rows were counted: every pass that
        # was launched counts, also those of an update ``target_kl`` stopped (None without the key: nothing is allocated)
        self._attn_stats, self.last_attention_statistics = None, None
        if s.attention_statistics:
            t_ = config["transformer"]
            self._attn_stats = ops.AttentionStatistics(t_["num_blocks"], t_["num_heads"], self.buffer.batch_size, t_["memory_length"], device)
            self.model.transformer.attn_stats = self._attn_stats
        # target_kl: the gate of the KL early stop (etm/optim.py: KlGate), reset at the start of every update; not trainer state, not in
        # the checkpoint.  ``last_kl_stop``: what the last update's gate said (None without the key: nothing is allocated)
        kl_cfg = s.target_kl
        self._kl_cfg, self._kl_gate, self.last_kl_stop = kl_cfg, None, None
        if kl_cfg is not None:
            self._kl_gate = KlGate(kl_cfg["limit"], device, host_word=kl_cfg["host_check"] == "epoch")
            self._kl_event = torch.cuda.Event() if kl_cfg["host_check"] == "epoch" else None
        # adaptive_lr: the rule of the KL-adaptive learning rate (etm/optim.py: AdaptiveLr).  From here on the device owns lr_dev --
        # learning_rate_schedule.initial was its start value, ``_set_lr`` does nothing, the rate persists across updates and travels in
        # the optimiser's state; the two counters are per update.  ``last_adaptive_lr``: the rate and the counters after the last update
        # (None without the key: nothing is allocated)
        self._adapt, self.last_adaptive_lr = None, None
        if s.adaptive_lr is not None:
            self._adapt = AdaptiveLr(s.adaptive_lr, device)
            self.optimizer.attach_adaptive(self._adapt)

    def _init_pinned_staging(self, resumed, first_worker_id):
        """Stage 4: the pinned blocks the host and the device hand observations, actions, (step, slot), mask words and rewards over in,
        and the environments' first observations in them."""
        device, W, obs_shape, box = self.device, self.num_workers, self.observation_space.shape, self.box is not None
        # host <-> device staging (pinned)
        if self._shm_env is not None:
            # observation rows and action words live in the workers' shared segment, registered with the HIP runtime: the copy
            # engine reads the rows there, the sampling kernel writes the actions (and the step's sequence number) there
            seg = np.frombuffer(self._shm_env.shm.buf, dtype=np.uint8)
            etm_lib.check(etm_lib.load().etm_host_register(seg.ctypes.data, seg.nbytes), "etm_host_register")
            self._shm_registered = seg.ctypes.data
            self._obs_pin = torch.from_numpy(self._shm_env.v["obs"])
            self._act_pin = torch.from_numpy(self._shm_env.v["act"])
        else:
            self._obs_pin = torch.zeros((W,) + obs_shape, dtype=self.observation_dtype).pin_memory()
            self._act_pin = torch.zeros((W, self._action_width), dtype=torch.float32 if box else torch.int64).pin_memory()
        self.obs = self._obs_pin.numpy()
        # (episode step, episode slot) of every worker: one pinned [2, W] block, uploaded with ONE copy per rollout step
        self._ss_pin = torch.zeros((2, W), dtype=torch.int64).pin_memory()
        self._step_pin, self._slot_pin = self._ss_pin[0], self._ss_pin[1]
        self.worker_current_episode_step = self._step_pin.numpy()   # host truth, mirrored on device each step
        self.worker_episode_slot = self._slot_pin.numpy()
        self.worker_episode_slot[:] = np.arange(W)
        self._ss_dev = torch.zeros((2, W), dtype=torch.int64, device=device)
        self._ss_dev[1] = torch.arange(W, dtype=torch.int64, device=device)
        self._step_dev, self._slot_dev = self._ss_dev[0], self._ss_dev[1]
        # action_masks: the workers' words for the observation they are about to act on -- one pinned int64 [W] block (a group's
        # words are a contiguous slice, rollout_plan.WorkerGroup) that every sampling kernel reads IN PLACE at its start, in every plan:
        # the host rewrites a group's words only after it has that step's actions, i.e. after the read.  The device twin, handed over as
        # the (step, slot) block's twin is (an upload / a copy node per step where the plan does not read that block in place), was
        # measured against it and lost (``_mask_in_place = False`` selects it: tools/action_masks_measure.py, profiles/r15).  Nothing
        # is allocated without the key.
        self._mask_in_place = True
        self._am_pin = self._am_dev = self._am_np = None
        if self._masked:
            self._am_pin = torch.zeros(W, dtype=torch.int64).pin_memory()
            self._am_np = self._am_pin.numpy()
            self._branch_bits = branch_bit_masks(self.action_space_shape)
            self._am_dev = torch.zeros(W, dtype=torch.int64, device=device)
        # previous_step_input with the reward: the workers' last raw rewards, one pinned float32 [W] block that the rows kernel in front
        # of a step reads IN PLACE -- the discipline of the mask words: the host writes a group's entries where it writes
        # buffer.rewards[w, t], after env.step and before the next launch, i.e. after that step's actions are back.  Nothing is
        # allocated without the key.
        self._rw_pin = self._rw_np = None
        if self._prev_cfg is not None and self._prev_cfg["reward"]:
            self._rw_pin = torch.zeros(W, dtype=torch.float32).pin_memory()
            self._rw_np = self._rw_pin.numpy()
        if resumed is not None and self._env_supplied and hasattr(self.env, "restart"):
            self.env.restart(first_worker_id)              # (a supplied environment moves to the segment's worker ids itself)
        self.env.reset(out=self.obs)
        if self._masked:
            self._take_action_masks(self.env, 0, W, "reset")

    def _init_step_operands(self):
        """Stage 5: the fixed-address operands of the rollout step, the time-major staging of its outputs, the draw tables and the
        upload stream."""
        config, device, W, obs_shape, box = self.config, self.device, self.num_workers, self.observation_space.shape, self.box is not None
        # fixed-address operands of the rollout step (HIP-graph friendly) and time-major staging of the step outputs
        S, L, B = config["worker_steps"], self.memory_length, self._action_width
        self._obs_dev = torch.zeros((W,) + obs_shape, dtype=self.observation_dtype, device=device)
        self._stage = {
            "obs": torch.zeros((S, W) + obs_shape, dtype=self.observation_dtype, device=device),
            "memory_mask": torch.zeros((S, W, L), dtype=torch.bool, device=device),
            "memory_indices": torch.zeros((S, W, L), dtype=torch.int64, device=device),
            "actions": torch.zeros((S, W, B), dtype=torch.float32 if box else torch.int64, device=device),
            "log_probs": torch.zeros((S, W, 1 if box else B), dtype=torch.float32, device=device),      # (Box: one joint log-prob)
            "values": torch.zeros((S, W), dtype=torch.float32, device=device),
        }
        if self._kl_analytic:       # (the means next to the actions; _finish_rollout moves every staging table into the buffer's field)
            self._stage["means"] = torch.zeros((S, W, B), dtype=torch.float32, device=device)
        if self._kl_exact_cat:      # (every column's log-prob of every branch next to the actions; into the buffer's old_logps likewise)
            self._stage["logps"] = torch.zeros((S, W, sum(self.action_space_shape)), dtype=torch.float32, device=device)
        self._mask_t = torch.zeros((W, L), dtype=torch.bool, device=device)
        self._win_t = torch.zeros((W, L), dtype=torch.int64, device=device)
        self._act_dev = torch.zeros((W, B), dtype=torch.float32 if box else torch.int64, device=device)
        # one uniform per (step, worker, branch); a single branch keeps the [S, W] draw (the same bits as ever)
        self._uniforms = torch.zeros((S, W) if B == 1 else (S, W, B), dtype=torch.float32, device=device)
        # teacher forcing (parity tests): a non-negative entry replaces the sampled action of that (step, worker, branch); the table
        # has a fixed address, so the captured step graphs read it too -- every rollout path can be driven with recorded actions
        self._forced_tab = torch.full((S, W) if B == 1 else (S, W, B), -1, dtype=torch.int64, device=device)
        if box:
            # Box: one N(0, 1) draw per (step, worker, dimension), fixed address like the uniforms; forced actions are floats, NaN =
            # "sample" (the [S, W] uniforms stay allocated but are not drawn)
            self._normals = torch.zeros((S, W, B), dtype=torch.float32, device=device)
            self._forced_tab = torch.full((S, W, B), float("nan"), dtype=torch.float32, device=device)
        # observation streaming (graph rollout with the fused encoder): rows of the next observation go from pinned memory
        # straight into their row of the time-major staging array on a second stream while the environments still step
        self._up_stream = torch.cuda.Stream(device=device)
        self._step_graph = None      # (head, tail or None) of the first group, once captured
        self._chain_log = None       # tools/rollout_profile.py: per-step host timestamps of the first group
        self._plan = None            # the form of the captured step (rollout_plan.RolloutPlan), decided when it is captured
        self._stage_host = None      # host view of the staging array (direct observation rows)
        self._stage_read = torch.cuda.Event()      # (direct rows) the update's copy out of the staging array has run

    def _init_kv_cache_and_replays(self):
        """Stage 6: the rollout's K|V cache and the replays (cache refresh, last value, bootstrap pass) with their operands."""
        config, device, W, L, B = self.config, self.device, self.num_workers, self.memory_length, self._action_width
        # rollout K/V cache (weights are frozen while sampling): per worker [T, blocks, 2D] projections of its episode
        self._use_kv_cache = bool(config.get("kv_cache_rollout", True))
        T, nb, D = self.max_episode_length, self.num_blocks, self.embed_dim
        self._kv_cache = torch.zeros((W, T, nb, 2 * D), dtype=torch.float32, device=device)
        self._kv_init = torch.zeros((T, nb, 2 * D), dtype=torch.float32, device=device)
        self._kv_weights = self._kv_w_blocked = None
        # (both replays: ``enabled`` is set before every call -- hip_graph_rollout, and the bank has its final address)
        self._kv_refresh_replay = ops.ReplayAfterWarmup(self._refresh_kv_cache_now, device, what="_refresh_kv_cache")
        # get_last_value's forward pass as a replay (``_lv.graph`` once captured), carrying its fixed-address operands
        self._lv = lv = ops.ReplayAfterWarmup(self._last_value_now, device, what="get_last_value")
        lv.rows, lv.obs = torch.empty((W, L), dtype=torch.int64, device=device), torch.empty_like(self._obs_dev)
        lv.out = torch.empty(W, dtype=torch.float32, device=device)
        # bootstrap_truncated: the value of the observation after every time-limit cut of the rollout (_bootstrap_pass), W records per
        # replay on fixed-address operands of get_last_value's shape; nothing is allocated without the key
        self._bootstrap = bool(config.get("bootstrap_truncated", False))
        self._truncations = []            # (w, t, slot, s, final observation) of the running rollout
        self.last_truncations = []        # (w, t, slot, s) of the last rollout
        if self._bootstrap:
            self._bs = bs = ops.ReplayAfterWarmup(self._bootstrap_chunk_now, device, what="bootstrap pass")
            bs.obs, bs.rows, bs.pidx = torch.empty_like(self._obs_dev), torch.empty_like(lv.rows), torch.empty_like(lv.rows)
            bs.slot, bs.s = torch.zeros(W, dtype=torch.int64, device=device), torch.zeros(W, dtype=torch.int64, device=device)
            bs.out = torch.empty(W, dtype=torch.float32, device=device)
            if self._prev_cfg is not None:
                bs.pa, bs.pr = torch.zeros((W, B), dtype=torch.int64, device=device), torch.zeros(W, dtype=torch.float32, device=device)

    def _init_worker_groups_and_tables(self):
        """Stage 7: the worker groups over everything above, and the window tables."""
        device, W = self.device, self.num_workers
        # worker groups: the full-width group (eager path, single-group graph path) aliases the buffers above; the pipelined
        # groups own what cannot be a contiguous slice of them.  WorkerGroup reads from this object, so all of these exist by now:
        # device, box, _action_width, num_blocks, embed_dim, num_workers, obs / _obs_pin / _act_pin, _ss_pin / _ss_dev, _obs_dev,
        # _mask_t, _win_t, _act_dev, _kv_cache, _stage["obs"]
        self._group_all = WorkerGroup(self, 0, W, self.env, True, self._etm.etm_upload)
        parts = getattr(self.env, "parts", None)
        self._groups = [self._group_all]
        if parts is not None and len(parts) > 1:
            self._groups = [WorkerGroup(self, lo, hi, part, False, self._etm.etm_upload) for part, (lo, hi) in zip(parts, self.env.bounds)]

        mask, indices = build_window_tables(self.memory_length, self.max_episode_length)
        self.memory_mask, self.memory_indices = mask, indices                       # host copies (upstream names)
        self._mask_table = mask.bool().contiguous().to(device)
        self._index_table = indices.contiguous().to(device)
        self.last_update_timing = {}

    def _take_action_masks(self, env, lo, hi, step):
        """``action_masks: true``: the words of the observations ``env`` (workers [lo, hi)) returned last -> the pinned block the next
        step launch reads.  A word with an empty branch is an environment bug and raises here, before that launch (``step``: the
        rollout step whose observation it belongs to, or "reset")."""
        words = self._am_np[lo:hi]
        env.action_masks(out=words)
        empty = empty_mask_branches(words, self.action_space_shape, self._branch_bits)
        if empty.any():
            wl, b = (int(x) for x in np.argwhere(empty)[0])
            raise ValueError(f"action_masks: worker {lo + wl}, step {step}, branch {b} has no valid action (word {int(words[wl]):#x}, branches "
                             f"{self.action_space_shape}): an environment must leave at least one action of every branch allowed")

    # ------------------------------------------------------------------ properties mirroring upstream members
    @property
    def memory(self):
        """[W, T, blocks, D] live episodic memory of every worker (upstream ``self.memory``); a gathered copy."""
        return self.buffer.bank.index_select(0, self._slot_dev)

    @property
    def obs_norm(self):
        """``normalize_observations``: a read-only view {"clip", "epsilon", "stats" [3, F] float64 (count, mean, M2), "mean" [F],
        "rstd" [F]} of the model's running triple and frozen table (the tensors are the model's buffers); None without the key."""
        m = self.model
        if m.obs_norm is None:
            return None
        return dict(m.obs_norm, stats=m.obs_norm_stats, mean=m.obs_norm_mean, rstd=m.obs_norm_rstd)

    @property
    def return_norm(self):
        """``normalize_rewards``: a read-only view {"clip", "epsilon", "stats" [3] float64 (count, mean, M2 of the discounted returns),
        "carry" [W] float64, "scale" [1] float32 (of the last rollout), "scaled" [W, S] (the rewards GAE read)}; None without the key.
        Trainer state: the model file (.nn) does not hold it; the training checkpoint (``save_checkpoint``) stores ``stats``, and a
        resumed run continues the triple with ``carry`` zero (its episodes start afresh)."""
        b = self.buffer
        if b.return_norm is None:
            return None
        return dict(b.return_norm, stats=b.ret_stats, carry=b.ret_carry, scale=b.return_scale, scaled=b.rewards_scaled)

    def _training_observations(self):
        """What the captured step reads its observations from, when not from the gathered minibatch fields: the NHWC copy of visual
        observations, or -- ``normalize_observations`` -- the buffer's raw vector rows (the normalising launch gathers them)."""
        nhwc = self._observations_channels_last()
        if nhwc is None and self.model.obs_norm is not None:
            return self.buffer.samples_flat["obs"]
        return nhwc

    def _update_obs_norm(self):
        """After the last minibatch of an update: merge the update's W * S raw observations into the running triple and refresh the
        frozen table, in place (the captured graphs hold the addresses) -- the next rollout and optimisation run on the new table."""
        m = self.model
        with torch.no_grad():
            ops.obs_stats_update(self.buffer.samples_flat["obs"], m.obs_norm_stats, m.obs_norm_mean, m.obs_norm_rstd, m.obs_norm["epsilon"])

    # ------------------------------------------------------------------ training loop
    def run_training(self) -> None:
        print("Step 6: Starting training using " + str(self.device))
        episode_infos = self._episode_infos
        ckpt_every, ev_cfg = self.settings.checkpoint_interval, self.settings.evaluation
        ev_every = ev_cfg["interval"] if ev_cfg is not None else 0
        for update in range(self.update_index, self.config["updates"]):       # (a resumed run starts at the stored index)
            lr, beta, clip = self.schedules(update)
            t0 = time.perf_counter()
            sampled_episode_info = self._sample_training_data()
            self.buffer.prepare_batch_dict()
            training_stats, grad_info = self._train_epochs(lr, clip, beta)
            torch.cuda.synchronize(self.device)
            dt = time.perf_counter() - t0
            training_stats = np.mean(training_stats, axis=0)
            episode_infos.extend(sampled_episode_info)
            episode_result = process_episode_info(episode_infos)
            steps_per_s = self.num_workers * self.config["worker_steps"] / dt
            vmean, amean = torch.mean(self.buffer.values).item(), torch.mean(self.buffer.advantages).item()
            if episode_result:
                head = "{:4} reward={:.2f} std={:.2f} length={:.1f} std={:.2f}".format(
                    update, episode_result["reward_mean"], episode_result["reward_std"], episode_result["length_mean"],
                    episode_result["length_std"])
            else:
                head = "{:4} (no finished episode yet)".format(update)
            if "success_percent" in episode_result:
                head += " success={:.2f}".format(episode_result["success_percent"])
            if self._is_main:
                print(head + " pi_loss={:3f} v_loss={:3f} entropy={:.3f} loss={:3f} value={:.3f} advantage={:.3f} steps/s={:.0f}".format(
                    training_stats[0], training_stats[1], training_stats[3], training_stats[2], vmean, amean, steps_per_s))
            self._write_gradient_summary(update, grad_info)
            self._write_training_summary(update, training_stats, episode_result, vmean, amean, steps_per_s)
            if ev_every and ((update + 1) % ev_every == 0 or update + 1 == self.config["updates"]):
                self._write_evaluation_summary(update, self.evaluate(ev_cfg["episodes_per_worker"], ev_cfg["n_workers"], ev_cfg["deterministic"]))
            self.update_index = update + 1
            if ckpt_every and ((update + 1) % ckpt_every == 0 or update + 1 == self.config["updates"]):
                self.save_checkpoint()         # (model file + training checkpoint; refused in data-parallel runs, so one rank)
        if self._is_main and not ckpt_every:   # replicas are identical: one rank writes the model file
            self._save_model()
        if self.dp is not None:
            self.dp.barrier()

    @property
    def _is_main(self):
        return self.dp is None or self.dp.rank == 0

    def schedules(self, update: int):
        s = lambda c: polynomial_decay(c["initial"], c["final"], c["max_decay_steps"], c["power"], update)
        return s(self.lr_schedule), s(self.beta_schedule), s(self.cr_schedule)

    # ------------------------------------------------------------------ rollout
    # the form of the CAPTURED rollout step, read-only views of its plan (no plan -- before the first capture, after the step kernel's
    # time-out recovery -- reads False; an eager rollout runs on the all-false plan without replacing a captured one)
    _stream_obs = property(lambda self: self._plan is not None and self._plan.stream_obs)
    _host_flag = property(lambda self: self._plan is not None and self._plan.host_flag)
    _native_rollout = property(lambda self: self._plan is not None and self._plan.native)
    _direct_rows = property(lambda self: self._plan is not None and self._plan.direct_rows)

    def _sample_training_data(self, forced_actions=None, uniforms=None, normals=None, deterministic=False) -> list:
        """Runs all workers for ``worker_steps`` steps; fills the buffer; returns finished-episode infos.

        The device work of one step (window lookup, model forward, action sampling, staging of the step's buffer rows,
        action hand-over; then memory write and K/V projection of the new items) is captured ONCE in two HIP graphs -- head
        and tail -- per worker group and replayed per step (``hip_graph_rollout: false`` in the config selects the eager
        path).  With ``rollout_groups`` = 2 the groups form a software pipeline: the host steps one group's environments
        while the device runs the other group's head graph.  With the fused encoder the observation rows of step t+1 are
        streamed from pinned memory into row t+1 of the staging array on a second stream while the environments still step
        (``stream_observations``), together with the workers' (episode step, slot) vector; the actions arrive in pinned host
        memory straight from the sampling kernel.  Which of these forms apply is the rollout's plan (rollout_plan.py).
        ``forced_actions`` [W, S] or [W, S, B] (optional) replays recorded actions instead of sampling (teacher forcing for parity
        tests -- CPU and GPU RNG streams differ) on whichever path the config selects: the sampling
        kernels read them from a fixed-address table, so the captured graphs, the observation streaming and the worker-group
        pipeline run exactly as they do when sampling.
        ``uniforms`` [W, S] or [W, S, B] (optional, tests) replaces the rollout's uniform draws: every sampling kernel inverts its CDF at
        exactly these values (branch b of a MultiDiscrete policy at its own draw).
        Box policies: ``forced_actions`` [W, S, A] floats (NaN = sample), ``normals`` [W, S, A] (optional, tests) replaces the
        rollout's N(0, 1) draws.
        ``deterministic``: every action is the MODE of the policy on whichever path the config selects -- a categorical policy's
        uniform table is filled with the greedy sentinel -1 (etm_sample_branch: the first maximum of each branch's logits), a Box
        policy's normals table with zeros (the mean).  ``forced_actions`` keep their meaning; ``uniforms`` / ``normals`` together
        with it is a ValueError (a ``uniforms`` table may itself hold negative entries: greedy per entry)."""
        if deterministic and (uniforms is not None or normals is not None):
            raise ValueError("deterministic=True fills the draw tables itself: do not pass uniforms= / normals= with it")
        main = torch.cuda.current_stream(self.device)
        plan, groups = self._begin_rollout(main, forced_actions, uniforms, normals, deterministic)
        # the device work of a step of a group goes in flight in ONE of three forms
        launch = self._launch_graph_exec if plan.direct_launch else self._launch_replay if plan.graph else self._launch_eager
        for g in groups:
            launch(g, plan)
        episode_infos = []
        if plan.native:
            try:
                timing = self._drive_rollout_native(groups, episode_infos)
            finally:
                self._shm_env.park()          # whatever happened: no worker keeps spinning through the optimisation phase
        else:
            timing = self._drive_rollout_host(plan, groups, launch, episode_infos)
        for g in groups:
            if g.stream is not None:
                main.wait_stream(g.stream)
        self._check_step_kernels(groups)
        self._finish_rollout(plan, main, forced_actions is not None, timing)
        return episode_infos

    def _begin_rollout(self, main, forced_actions, uniforms, normals, deterministic=False):
        """Everything before step 0: episode slots, K/V cache and weight copies, the draw tables, the captured graphs (first rollout)
        and with them the plan, the streams, the rows of observation 0.  -> (plan, the groups that run)."""
        self.buffer.begin_rollout(self._slot_dev)
        self._truncations = []
        self.worker_episode_slot[:] = np.arange(self.num_workers)
        self._slot_dev.copy_(self._slot_pin, non_blocking=True)
        if self._use_kv_cache:
            self._refresh_kv_cache()
        self.model.refresh_rollout_weights()       # encoder weight copies for the fused rollout convolutions
        if forced_actions is not None:
            self._forced_tab.copy_(time_major(self._forced_tab, forced_actions).to(self.device))
        if self._masked:
            self.buffer.action_masks_host[:, 0] = self._am_np      # (the words of observation 0: taken after the last step / the reset)
        if self.config.get("hip_graph_rollout", True):
            groups = self._groups
            if groups[0].graphs is None:
                self._capture_step_graph(groups)
            plan = self._plan
        else:
            groups, plan = [self._group_all], RolloutPlan(polite_wait=bool(self._host_plan["polite_wait"]))
        if deterministic:
            # the mode at every entry: the greedy sentinel in the uniforms, zeros in the normals (x = mu + sigma * 0)
            if self.box is None:
                self._uniforms.fill_(-1.0)
            else:
                self._normals.zero_()
        elif self.box is None and uniforms is not None:
            self._uniforms.copy_(time_major(self._uniforms, uniforms))
        elif self.box is None:
            self._uniforms.uniform_(generator=self._draw_generator)      # one draw per (step, worker, branch) for the whole rollout
        elif normals is not None:
            self._normals.copy_(time_major(self._normals, normals))
        else:
            self._normals.normal_(generator=self._draw_generator)        # one N(0, 1) draw per (step, worker, dimension) for the whole rollout
        for g in groups:
            g.restart()
            if g.stream is not None:
                g.stream.wait_stream(main)         # buffers prepared above on the main stream
        if plan.stream_obs:
            self._up_stream.wait_stream(main)      # the staging array may still be read by the previous update
        if plan.direct_rows:
            # (the pinned buffer still receives the observation AFTER the last step: the bootstrap value and the next rollout's
            # observation 0 read it)
            self._stage_read.synchronize()         # the previous update's copy out of the staging array has run
        if plan.native:
            # the device's step counter restarts at 1: go = 0 on every group, acknowledged by every worker, BEFORE step 0 is launched;
            # the workers then spin (no self-parking) until the rollout is over
            self._shm_env.activate(hold=True)
            self._shm_env.restart_sequence()
        if plan.stream_obs:
            for g in groups:                       # observation 0 -> staging row 0
                g.upload_rows(0, 0, g.W)
        return plan, groups

    def _launch_graph_exec(self, g, plan):
        """One captured graph per step on the group's own stream, nothing to wait for: hipGraphLaunch through the library."""
        g.take_state()
        rc = self._etm.etm_graph_launch(g.graph_exec, g.stream.cuda_stream)
        if rc != 0:
            etm_lib.check(rc, "etm_graph_launch")

    def _launch_replay(self, g, plan):
        """Head graph, (event for the host,) tail graph through the framework's replay() on the group's stream."""
        g.take_state()
        with torch.cuda.stream(g.stream):        # (no stream of its own: the caller's)
            cur = g.stream if g.stream is not None else torch.cuda.current_stream(self.device)
            if plan.stream_obs and not plan.own_stream:
                # the (step, slot) block follows the observation rows on the shared upload stream; the step waits for both
                self._etm.etm_upload(g.ss_dev.data_ptr(), g.ss_pin.data_ptr(), g.ss_pin.numel() * 8, self._up_stream.cuda_stream)
                if g.am_pin is not None and not self._mask_in_place:         # (the words' device twin travels with the block)
                    self._etm.etm_upload(g.am_dev.data_ptr(), g.am_pin.data_ptr(), g.am_pin.numel() * 8, self._up_stream.cuda_stream)
                g.up_done.record(self._up_stream)
                cur.wait_event(g.up_done)
            g.graphs[0].replay()
            if not plan.host_flag:
                g.act_ready.record(cur)          # actions are in pinned memory once this event completes
            if g.graphs[1] is not None:
                g.graphs[1].replay()             # tail runs while the host steps the environments

    def _launch_eager(self, g, plan):
        with torch.no_grad():
            carry = self._rollout_step_head(g)
            g.act_ready.record(torch.cuda.current_stream(self.device))
            self._rollout_step_tail(g, carry)

    def _drive_rollout_host(self, plan, groups, launch, episode_infos):
        """Steps 0 .. S - 1 from this thread, step 0 of every group being in flight: per step and group wait for the actions, step
        the environments, do the episode bookkeeping, launch the next step.  -> seconds in (env.step, waiting, upload + launch)."""
        # this loop is the rollout's critical path: what the plan fixes is bound to locals here, once
        buf, S, clock = self.buffer, self.config["worker_steps"], time.perf_counter
        direct, stream_obs, host_flag, polite = plan.direct_rows, plan.stream_obs, plan.host_flag, plan.polite_wait
        masked, rw = self._masked, self._rw_np
        fence = self._etm.etm_host_store_fence
        t_env = t_wait = t_launch = 0.0
        # a device-resident front-end (environments/device_env.py) in a plan that streams observations: its kernel reads the actions in
        # g.act_dev and writes the frames of step t + 1 into the group's rows of staging row t + 1, on the group's stream -- behind the
        # step's sampling, in front of the next step's encoder; nothing is uploaded.  Every other front-end takes the branches of ever.
        resident = [stream_obs and bool(getattr(g.env, "device_resident", False)) for g in groups]
        main = torch.cuda.current_stream(self.device)
        for t in range(S):
            for g, on_device in zip(groups, resident):
                lo, hi = g.lo, g.hi
                tw = clock()
                if host_flag:
                    self._await_flag(g.flag_np, t + 1, polite)
                else:
                    g.act_ready.synchronize()
                te = clock()
                t_wait += te - tw
                if polite:
                    self._flag_wait_ema += 0.1 * ((te - tw) - self._flag_wait_ema)
                # the rows of observation t + 1 go straight into their staging row in device memory (the fence sits between them and
                # the next launch), or into pinned memory and from there, as the environment emits them, into their staging row, or
                # (unstreamed, and after the last step) into pinned memory alone
                if on_device and t + 1 < S:
                    rewards, dones, infos = g.env.step_device(g.act_dev, g.stage0 + (t + 1) * g._stage_pitch, g.stream if g.stream is not None else main)
                elif direct and t + 1 < S:
                    _, rewards, dones, infos = g.env.step(g.acts_host, out=self._stage_host[t + 1, lo:hi])
                    fence(self._dev_index)
                elif stream_obs and t + 1 < S:
                    _, rewards, dones, infos = g.env.step(g.acts_host, out=g.obs_np, on_rows=partial(g.upload_rows, t + 1))
                else:
                    _, rewards, dones, infos = g.env.step(g.acts_host, out=g.obs_np)
                t_env += clock() - te
                self.worker_current_episode_step[lo:hi] += 1
                if dones.any():
                    self._hand_over_episodes(g, t, dones, infos, episode_infos)
                if masked:
                    # the words of observation t + 1 (after an auto-reset: the new episode's) into the pinned block, before the launch
                    self._take_action_masks(g.env, lo, hi, t + 1)
                    if t + 1 < S:
                        buf.action_masks_host[lo:hi, t + 1] = self._am_np[lo:hi]
                if rw is not None:
                    rw[lo:hi] = rewards              # (previous_step_input: the raw rewards the next step's rows kernel reads in place)
                if t + 1 < S:
                    tl = clock()
                    launch(g, plan)                  # bookkeeping of this step is final: (step, slot) follow the observation rows
                    t_launch += clock() - tl
                    if self._chain_log is not None and g is groups[0]:
                        self._chain_log.append((tw, te, tl, clock()))
                buf.rewards[lo:hi, t] = rewards    # (after the launch: nothing on the device waits for these)
                buf.dones[lo:hi, t] = dones
        return t_env, t_wait, t_launch

    def _await_flag(self, flag, target, polite):
        """The sampling kernel stored the actions and then the step's number into the host word ``flag``: spin on it."""
        spins, t_wait0 = 0, time.perf_counter()
        if polite and flag[0] != target and self._flag_wait_ema > 80e-6:
            # not enough CPUs for a spinning trainer thread (etm/hostcpu.py): sleep through most of the wait this flag
            # usually takes (an average of the earlier waits), spin for the rest
            time.sleep(0.7 * self._flag_wait_ema)
        while flag[0] != target:
            spins += 1
            if spins % 4096 == 0 and time.perf_counter() - t_wait0 > 30.0:
                raise RuntimeError("rollout step did not complete within 30 s (device hang?)")

    def _hand_over_episodes(self, g, t, dones, infos, episode_infos):
        """Workers of group g whose episode ended at step t start the next one in a fresh slot (upstream :195-213)."""
        buf, S = self.buffer, self.config["worker_steps"]
        for wl in np.flatnonzero(dones):
            w = g.lo + int(wl)
            info = infos[wl]
            if info is not None and ("truncated" in info or "final_observation" in info):
                # a time-limit cut (environments/vec_env.py): with bootstrap_truncated remember where it happened -- the episode's
                # slot and length, before either is replaced -- and the observation after it; key on or off, the episode infos never carry the two keys
                if self._bootstrap and info.get("truncated"):
                    if info.get("final_observation") is None:
                        raise RuntimeError("bootstrap_truncated: a truncated episode's info carries no final_observation "
                                           "(environments/vec_env.py: the vectorised front-end stores it before it resets)")
                    self._truncations.append((w, int(t), int(self.worker_episode_slot[w]), int(self.worker_current_episode_step[w]),
                                              info["final_observation"]))
                    buf.truncated[w, t] = True
                info = {k: v for k, v in info.items() if k not in ("truncated", "final_observation")}
            self.worker_current_episode_step[w] = 0
            episode_infos.append(info)
            slot = buf.open_episode()                  # fresh zero memory for the next episode (upstream :208-213)
            self.worker_episode_slot[w] = slot
            if t < S - 1:
                buf.memory_index_host[w, t + 1:] = slot

    def _check_step_kernels(self, groups):
        """Raises if a step kernel set its error word during this rollout, after making the trainer fit to continue."""
        # a team member gave up waiting for its partners (not all workgroups were resident): this rollout's data are
        # unusable.  Leave the trainer in a state that can continue: clear the error words, switch to the multi-launch
        # step for the rest of the run and drop the captured graphs and their plan so that the next rollout re-decides and re-captures.
        every = groups + [self._group_all]
        if not any(g.rf_scratch is not None and int(ops.rollout_trxl_error(g.rf_scratch).item()) != 0 for g in every):
            return
        for g in every:
            if g.rf_scratch is not None:
                ops.rollout_trxl_clear_error(g.rf_scratch)
            g.graphs = g.graph_exec = None
        self.model.fused_rollout_block = False
        self.model._rf = self.model._rfg = None
        self._step_graph = self._plan = None
        raise RuntimeError("fused rollout step: a team member timed out waiting for its partners; this rollout is void. The "
                           "trainer has switched to the multi-launch step (fused_rollout_block: false) for the following rollouts")

    def _finish_rollout(self, plan, main, forced, timing):
        """Time-major staging -> the buffer's [W, S, ...] fields (one strided copy per field), bootstrap value, advantages."""
        buf = self.buffer
        forced_wsb = None
        if forced and self._masked:          # (which entries were forced, [W, S, B], before the table is cleared)
            W, S = self.num_workers, self.config["worker_steps"]
            forced_wsb = self._forced_tab.reshape(S, W, -1).transpose(0, 1).cpu().numpy()
        if forced:
            self._forced_tab.fill_(float("nan") if self.box is not None else -1)
        if self._masked:
            self.last_valid_action_share = valid_action_share(buf.action_masks_host, sum(self.action_space_shape))
        self._step_dev.copy_(self._step_pin, non_blocking=True)
        self._slot_dev.copy_(self._slot_pin, non_blocking=True)
        for name, stage in self._stage.items():      # (the buffer's field has the table's name; the log-prob rows are its old_logps)
            getattr(buf, "old_logps" if name == "logps" else name).copy_(stage.transpose(0, 1))
        if plan.direct_rows:
            self._stage_read.record(main)          # the next rollout's host writes into the staging array wait for this
        if forced_wsb is not None:
            self._check_forced_against_masks(forced_wsb)
        if self._bootstrap:                        # (after the staging copies: buf.memory_indices is final)
            self._bootstrap_pass()
        buf.calc_advantages(self.get_last_value(), self.config["gamma"], self.config["lamda"])
        if self._prev_cfg is not None:       # (after the uploads of the raw rewards and the done flags)
            buf.build_previous_step()
        self.last_update_timing.update(env_s=timing[0], wait_s=timing[1], launch_s=timing[2])

    def _check_forced_against_masks(self, forced):
        """After a rollout that was given ``forced_actions`` (``forced`` [W, S, B], negative = sampled): a forced action overrides
        sampling, so it must have been allowed by the word of its step -- raises ValueError naming the first one that was not.  Only
        the forced entries are looked at: a sampled action is allowed by construction."""
        words = self.buffer.action_masks_host.view(np.uint64)
        off = 0
        for b, a in enumerate(self.action_space_shape):
            fb = forced[:, :, b]
            bit = np.where(fb >= 0, fb, 0).astype(np.uint64) + np.uint64(off)
            bad = (fb >= 0) & (((words >> bit) & np.uint64(1)) == 0)
            if bad.any():
                w, t = (int(x) for x in np.argwhere(bad)[0])
                raise ValueError(f"forced_actions: worker {w}, step {t}, branch {b}: the forced action {int(fb[w, t])} is masked out "
                                 f"(word {int(words[w, t]):#x})")
            off += int(a)

    def _rollout_step_device(self, g, stream_obs=False, host_flag=False):
        """Device side of one rollout step of group ``g`` (upstream trainer.py:161-186) = head + tail."""
        carry = self._rollout_step_head(g, stream_obs, host_flag)
        self._rollout_step_tail(g, carry, stream_obs)

    def _choose_step_form(self, g, streamed):
        """Which kernels make up the step of group ``g``: sets ``g.group_kernel`` / ``g.tail_in_kernel`` (and the step kernel's scratch)
        before anything is launched.  -> (fused_step, the step kernel's weight table, the form of its hidden-layer input)."""
        # hidden-layer input: "conv3" / "partial" (lin_hidden as K-slice partial sums, with / without the last encoder layer in the same
        # launch) or "full" (the model's encoder)
        m, lib = self.model, self._etm
        rf = getattr(m, "_rf", None) if self._use_kv_cache else None
        # (every team of the step kernel must be resident at once, and the groups' step kernels run concurrently: the workgroups
        # of ALL groups together must fit the 256 CUs -- one 512-thread workgroup per CU --, else the multi-launch path)
        n_conc = len(self._groups) if not g.full else 1
        # GRU-gated layouts in groups of <= 8 workers take the GROUP form of the step kernel (weights once per group and
        # step, 32 workgroups per launch; csrc/rollout_group.hip)
        rfg = getattr(m, "_rfg", None) if rf is not None else None
        g.group_kernel = bool(rfg is not None and self.config.get("rollout_group_kernel", True)
                              and ops.rollout_trxl_group_ok(rfg, g.W, self.memory_length, m.hidden_size, m._rollout_actions(),
                                                            gaussian=self.box is not None)
                              and n_conc * lib.etm_rollout_trxl_group_grid() <= 256)
        fused_step = (rf is not None and m.rollout_heads_fusable()
                      and (g.group_kernel or n_conc * lib.etm_rollout_trxl_grid(g.W, rf["H"]) <= 256))
        g.tail_in_kernel = bool(fused_step and self.config.get("fused_rollout_tail", True) and self._kv_w_blocked is not None)
        if not fused_step:
            return False, None, None
        rf = rfg if g.group_kernel else rf
        if g.rf_scratch is None or g.rf_scratch_kind != g.group_kernel:
            # (the two forms of the kernel lay their scratch out differently: launch counter, tags and slots belong to one form)
            t_ = m.transformer
            g.rf_scratch = ops.rollout_trxl_scratch(g.W, t_.embed_dim, t_.num_heads, t_.num_blocks, self.device, group=g.group_kernel)
            g.rf_scratch_kind = g.group_kernel
        hidden = "full"
        if streamed and "hid_t" in rf:
            conv3 = self.config.get("fused_conv3_hidden", True) and ops.rollout_conv3_hidden_supported(m.conv3, *m.conv2_output_hw(), rf["hid_t"].shape[1])
            if conv3 and self._prev_cfg is not None:
                # previous_step_input adds one slice: one per output pixel + 1 must fit the step kernel's 64 slices, else `partial`
                h2, w2 = m.conv2_output_hw()
                conv3 = (h2 - 2) * (w2 - 2) + 1 <= 64
            hidden = "conv3" if conv3 else "partial"
        return True, rf, hidden

    def _hidden_input(self, g, hidden, rf, obs, obs_index, rows, ss_src=None):
        """The step kernel's hidden-layer input in the chosen form -> (h_in, the bias the kernel still has to add or None)."""
        m = self.model
        prev = self._rollout_prev(g, ss_src)
        if hidden == "full":
            if prev is None:
                return m._encode(obs, obs_index, rows), None
            # previous_step_input: a TWO-SLICE input -- x W^T into slice 0, the term into slice 1, lin_hidden's bias as the kernel's
            # bias: the step kernel's slices + bias + ReLU path.  (Where only the model's encoder builds the features -- library
            # convolutions -- its own road: the rows kernel with the bias, then relu(x W^T + that).)
            feats = m.rollout_features(obs, obs_index, rows)
            if feats is None:
                return m._encode(obs, obs_index, rows, prev=prev), None
            if g.h_part is None:
                g.h_part = torch.empty((2, feats.shape[0], m.lin_hidden.out_features), dtype=torch.float32, device=feats.device)
            torch.mm(feats, m.lin_hidden.weight.t(), out=g.h_part[0])
            sizes = self.action_space_shape if self._prev_cfg["action"] else ()
            ops.prev_input_rows(m.prev_input.weight, prev.actions, sizes, prev.rewards, ep_step=prev.ep_step, out=g.h_part[1])
            return g.h_part, m.lin_hidden.bias
        # lin_hidden as K-slice partial sums on 12 x 16 workgroups; the step kernel adds slices + bias + ReLU
        if hidden == "conv3":
            # the last encoder layer and lin_hidden's partial sums as ONE launch, one workgroup per output pixel
            # (csrc/conv3_hidden.hip): the step graph is conv1, conv2, this, the step kernel
            x, partial_sums = m._encode_fused(obs, obs_index, rows, features_only="conv2"), ops.rollout_conv3_hidden
            args = (m._w3k, m.conv3.bias, rf["hid_t"])
        else:
            x, partial_sums = m._encode_fused(obs, obs_index, rows, features_only=True), ops.rollout_hidden_partial
            args = (rf["hid_t"],)
        if prev is not None:
            # previous_step_input rides in as ONE MORE SLICE: the producer writes the first `splits` slices of the fixed-address block,
            # the rows kernel the last one, the step kernel adds the slices in slice order, then the bias, then the ReLU
            if g.h_part is None:
                first = partial_sums(x, *args)
                g.h_part = torch.empty((first.shape[0] + 1,) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
            splits = g.h_part.shape[0] - 1
            partial_sums(x, *args, out=g.h_part[:splits])
            sizes = self.action_space_shape if self._prev_cfg["action"] else ()
            ops.prev_input_rows(m.prev_input.weight, prev.actions, sizes, prev.rewards, ep_step=prev.ep_step, out=g.h_part[splits])
            return g.h_part, m.lin_hidden.bias
        if g.h_part is None:          # (the first call allocates the fixed-address result)
            g.h_part = partial_sums(x, *args)
        return partial_sums(x, *args, out=g.h_part), m.lin_hidden.bias

    def _rollout_prev(self, g, ss_src):
        """previous_step_input: the previous step of group ``g``'s workers in the rollout's form, or None without the key -- the
        group's ``act_dev`` (the actions of step t - 1, which the sampling of step t has not yet overwritten), its entries of the pinned
        block of last rewards, and row 0 of the (episode step, slot) block the step reads (0 = no previous step)."""
        if self._prev_cfg is None:
            return None
        return PreviousStep(g.act_dev, g.rw_pin, ss_src[0])

    def _rollout_step_head(self, g, stream_obs=False, host_flag=False):
        """Everything the ACTIONS of group ``g`` depend on: (observation / step / slot upload,) window lookup, model forward,
        sampling, staging of the step's rows, action hand-over.  Every operand has a fixed address (HIP-graph capturable).
        Returns what the tail needs (the new memory items, block-major)."""
        buf, st, m = self.buffer, self._stage, self.model
        rows = None if g.full else (g.lo, g.hi)
        if stream_obs:      # the observation of this step is already in row t of the staging array (see _sample_training_data)
            obs, obs_index = st["obs"], g.t_dev
        else:
            g.obs_dev.copy_(g.obs_pin, non_blocking=True)
            obs, obs_index, rows = g.obs_dev, None, None
            g.ss_dev.copy_(g.ss_pin, non_blocking=True)      # (streamed mode: uploaded with the observation rows)
            if g.am_pin is not None and not self._mask_in_place:
                g.am_dev.copy_(g.am_pin, non_blocking=True)  # (the words' device twin: likewise)
        policy_head = m.rollout_policy_head()
        mask_t, win_t = g.mask_t, g.win_t
        # streamed + pipelined mode: the (step, slot) block is read from pinned host memory (see rollout_plan.plan_rollout)
        ss_src = g.ss_pin if stream_obs and g.stream is not None else g.ss_dev
        # action_masks: the words are read in place from pinned memory (or take the block's road); None without the key: the entries without masks
        am_src = None if g.am_pin is None else (g.am_pin if self._mask_in_place or (stream_obs and g.stream is not None) else g.am_dev)
        fused_step, rf, hidden = self._choose_step_form(g, obs_index is not None)
        # The draw's operands, once per call, for whichever op the step's form selects.  The policy part: a Box policy's (log_std, low,
        # high) -- the Gaussian forms of the sampling kernels: normals in place of the uniforms, float forced / action tables -- and, with
        # kl_estimator: analytic, the means' table; or the branches (one entry: Discrete; the kernels then take their single-branch
        # entries), the mask words and, with exact_kl, the log-probs' table.  Without those keys exactly the calls of ever.
        box = None if self.box is None else (m.policy_log_std, self.box.low, self.box.high)
        if box is not None:
            policy = {"st_means": st["means"]} if self._kl_analytic else {}
        else:
            policy = dict(branches=self.action_space_shape, action_mask=am_src, **({"st_logps": st["logps"]} if self._kl_exact_cat else {}))
        # the staging part: the pre-drawn table, the forced actions, the step counter, the actions and the step's rows of the buffer
        staging = (self._uniforms if box is None else self._normals, self._forced_tab, g.t_dev, g.act_dev, st["actions"], st["log_probs"],
                   st["values"])
        hand_over = dict(host_actions=g.act_pin, host_flag=g.flag_pin if host_flag else None, w_off=g.lo)
        if fused_step:
            # post-LN blocks without gates: the transformer, the heads and the sampling are ONE launch -- one workgroup per
            # worker walks the whole chain as matrix-vector products over the L2-resident weights (csrc/rollout_fused.hip);
            # the step is then encoder (4 launches) + window lookup + this kernel instead of 26 dependent launches
            # (the kernel does the window lookup and the cache reset of new episodes itself by now: one launch fewer in the chain)
            h_in, h_bias = self._hidden_input(g, hidden, rf, obs, obs_index, rows, ss_src)
            # ... and, after the action hand-over, the memory-bank write and the K | V projection of the new items (the tail;
            # pre-LN: the kernel applies norm_kv)
            tail = (self._kv_w_blocked, m.transformer._pos(), g.step_l, g.slot_l, buf.bank) if g.tail_in_kernel else None
            ops.rollout_trxl(h_in, rf, g.kv, win_t, mask_t, g.item, policy_head, m.value, *staging, g.rf_scratch, tail=tail, h_bias=h_bias,
                             box=box, window=(ss_src, self._mask_table, self._index_table, st["memory_mask"], st["memory_indices"],
                                              g.ss_latch, g.t_row, self._kv_init), **hand_over, **policy)
            return g.item
        # window lookup + staging; the same launch records the staging row of this step for the tail (t_dev is incremented by
        # the sampling kernel) and resets the K/V cache of workers at episode step 0 (they start from the projection of an
        # empty memory)
        ops.rollout_window(ss_src[0], self._mask_table, self._index_table, g.t_dev, mask_t, win_t,
                           st["memory_mask"], st["memory_indices"], t_row=g.t_row,
                           reset=(g.kv, self._kv_init) if self._use_kv_cache else None, w_off=g.lo,
                           latch=(ss_src, g.ss_latch))
        kv_spec = WindowSpec.from_bank(g.kv, None, win_t, None, mask_t) if self._use_kv_cache else None
        # previous_step_input on the unfused roads: the encoder takes the previous step (nothing is passed without the key)
        pk = {} if self._prev_cfg is None else {"prev": self._rollout_prev(g, ss_src)}
        if kv_spec is not None and m.rollout_heads_fusable():
            # hidden heads -> ONE launch for output heads, sampling, staging, t += 1; the kernel stores the actions straight
            # into the pinned host buffer (no copy launch): they are visible to the host when the step's event (or, with
            # host_flag_actions, the flag) says the launch is done
            h2, item = m.forward_hidden_cached(obs, kv_spec, items_out=g.item, obs_index=obs_index, raw=True, obs_rows=rows, **pk)
            if box is not None:
                ops.rollout_policy_gaussian(h2, policy_head, m.value, box[0], *staging, low=box[1], high=box[2], h_bias=m._b_heads,
                                            **hand_over, **policy)
            else:
                ops.rollout_policy(h2, policy_head, m.value, *staging, h_bias=m._b_heads, **hand_over, **policy)
        else:
            if kv_spec is not None:
                logits, value, item = m.forward_logits_cached(obs, kv_spec, items_out=g.item, obs_index=obs_index, obs_rows=rows, **pk)
            else:
                spec = WindowSpec.from_bank(buf.bank, g.slot_dev, win_t, win_t, mask_t)
                logits, value, item = m.forward_logits(obs, spec, **pk)
                item = item.transpose(0, 1)
            if not g.full:
                raise RuntimeError("worker groups need the fused policy path (K/V cache)")
            # log-softmax + categorical sample (inverse CDF on pre-drawn uniforms) + log-prob + staging + t += 1, per action branch:
            # one launch (several branches: their logits side by side)
            lg = logits[0] if len(logits) == 1 else torch.cat(logits, dim=1)
            if box is not None:       # (the means; host actions clipped to the bounds)
                ops.rollout_sample_gaussian(lg, value, box[0], *staging, low=box[1], high=box[2], **policy)
            else:
                ops.rollout_sample(lg, value, *staging, **policy)
            g.act_pin.copy_(g.act_dev, non_blocking=True)
        if item.data_ptr() != g.item.data_ptr():
            g.item.copy_(item)
        return g.item

    def _rollout_step_tail(self, g, item, stream_obs=False):
        """What the host does NOT have to wait for before stepping the environments: memory-bank write (upstream :174),
        K/V projection of the new item into the cache, observation staging.  Runs under the host's env.step()."""
        buf, st = self.buffer, self._stage
        if not g.tail_in_kernel:                         # (else etm_rollout_trxl has written the bank and cache rows itself)
            item = item.transpose(0, 1)                  # block-major staging -> [Wg, blocks, D]
            buf.bank[g.slot_l, g.step_l] = item           # (step, slot) as latched by this step's head, see WorkerGroup
            if self._use_kv_cache:
                tr = self.model.transformer
                pos = tr._pos()
                pos_rows = pos.index_select(0, g.step_l) if pos is not None else None
                g.kv[g.ids, g.step_l] = tr.project_memory(item, pos_rows, self._kv_weights)
        if not stream_obs:
            st["obs"][:, g.lo:g.hi].index_copy_(0, g.t_row.view(1), g.obs_dev.unsqueeze(0))

    def _refresh_kv_cache(self):
        """Start of a rollout: re-project every live episode's memory with the CURRENT weights (they changed in the
        last optimisation phase) into the per-worker K/V cache [W, T, blocks, 2D]; rows that are not written yet hold the
        projection of a zero item, which is also the initial state of every episode that starts during the rollout.
        (A graph replay from its third call on, ops.ReplayAfterWarmup -- with ``hip_graph_rollout``.)"""
        r = self._kv_refresh_replay
        r.enabled = bool(self.config.get("hip_graph_rollout", True)) and self.buffer.address_captured      # (the bank keeps its address from the first captured step on)
        r()

    def _refresh_kv_cache_now(self):
        W, T = self.num_workers, self.max_episode_length
        tr = self.model.transformer
        with torch.no_grad():
            fresh = tr.kv_projection_weights()
            if self._kv_weights is None:      # fixed-address buffers: the captured step graph reads them every replay
                self._kv_weights = tuple(t.clone() if torch.is_tensor(t) else t for t in fresh)
            else:
                for dst, src in zip(self._kv_weights, fresh):
                    if torch.is_tensor(dst):
                        dst.copy_(src)
            # the step kernel's tail reads the projection weights member-blocked: [blocks, P, D, 2D / P] (fixed address)
            team = etm_lib.load().etm_rollout_trxl_team(tr.num_heads)
            w = self._kv_weights[0]                                    # [blocks, D, 2D] = [Wk^T | Wv^T]
            if w.shape[2] % (2 * team) == 0:
                # member m's block = [its D / P columns of K | its D / P columns of V]: exactly the cache columns it reads in the
                # attention phases, so the cache rows a member reads are only ever written by that member
                nb_, d_, d2_ = w.shape
                wb = w.reshape(nb_, d_, 2, team, d2_ // (2 * team)).permute(0, 3, 1, 2, 4).reshape(nb_, team, d_, d2_ // team)
                if self._kv_w_blocked is None:
                    self._kv_w_blocked = wb.contiguous()
                else:
                    self._kv_w_blocked.copy_(wb)
            pos = tr._pos()
            live = self.buffer.bank[:W].reshape(W * T, self.num_blocks, self.embed_dim)
            pos_all = pos.repeat(W, 1) if pos is not None else None
            self._kv_cache.copy_(tr.project_memory(live, pos_all, self._kv_weights).reshape(self._kv_cache.shape))
            zeros = torch.zeros((T, self.num_blocks, self.embed_dim), dtype=torch.float32, device=self.device)
            self._kv_init.copy_(tr.project_memory(zeros, pos, self._kv_weights))

    def _capture_step_graph(self, groups):
        """Decide the rollout's plan, warm the step of every worker group up on a side stream (library handles, MIOpen find, GEMM
        tuning, allocator), then capture it as TWO graphs per group: the head (ends with the action hand-over) and the tail (bank /
        cache / staging writes) -- or, with the flag hand-over, as one."""
        cfg = self.config
        with torch.no_grad():       # (both predicates of the model say no while autograd is on)
            plan = self._plan = plan_rollout(
                graph=True, stream_observations=bool(cfg.get("stream_observations", True)),
                host_flag_actions=bool(cfg.get("host_flag_actions", True)), direct_observation_rows=bool(cfg.get("direct_observation_rows", True)),
                kv_cache=self._use_kv_cache, fused_encoder=self.model._fused_encoder_ok(self._obs_dev),
                heads_fusable=self.model.rollout_heads_fusable(), several_groups=all(g.stream is not None for g in groups),
                worker_processes=self._shm_env is not None, raw_graph_exec=hasattr(torch.cuda.CUDAGraph, "raw_cuda_graph_exec"),
                large_bar=lambda: ops.host_direct_write_ok(self.device), polite_wait=bool(self._host_plan["polite_wait"]))
        so, hf = plan.stream_obs, plan.host_flag
        self._stage_host = ops.host_view(self._stage["obs"]) if plan.direct_rows else None
        for gi, g in enumerate(groups):
            g.obs_stream = g.stream.cuda_stream if plan.own_stream else self._up_stream.cuda_stream
            if plan.native:
                # the sampling kernels write the step's sequence number into the SEGMENT's go words (the workers spin on them) instead
                # of a private pinned word (decided here: the address is captured below)
                g.use_flag(self._shm_env.v["go"][gi, 0:1])
        # the warm-up executions below write the CURRENT step's memory item (and its K/V projection) into the bank / cache rows
        # (slot, step) of every worker.  A worker at episode step 0 attends over a fully masked window -- uniform weights over
        # ALL L rows, row 0 included (upstream quirk, transformer.py:66-68 with an all-zero mask row) -- so a row 0 left behind by
        # the warm-up would leak into the real step 0.  Keep the rows as they were.
        with torch.no_grad():
            ss = torch.from_numpy(self._ss_pin.numpy().copy()).to(self.device)
            all_ids = torch.arange(self.num_workers, device=self.device)
            saved_bank = self.buffer.bank[ss[1], ss[0]].clone()
            saved_kv = self._kv_cache[all_ids, ss[0]].clone()
            # (previous_step_input reads the last actions from act_dev, which the warm-up steps overwrite: kept likewise)
            saved_act = self._act_dev.clone() if self._prev_cfg is not None else None
        for g in groups:
            g.t_dev.zero_()
            # warm-up and capture run on the stream the group's graphs are replayed on: the BLAS workspace of the library
            # GEMMs is keyed by (handle, stream), so two groups whose graphs replay concurrently must not have been captured on
            # one shared capture stream (torch's default) -- split-K solutions would accumulate in the same scratch
            side = g.stream if g.stream is not None else torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side), torch.no_grad():
                for i in range(3):
                    self._rollout_step_device(g, so, hf)
                    side.synchronize()
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            pool = torch.cuda.graph_pool_handle()
            head, tail = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            # thread_local: only this thread's calls are checked during capture (RCCL's watchdog thread may query events)
            with torch.no_grad(), torch.cuda.graph(head, pool=pool, stream=g.stream, capture_error_mode="thread_local"):
                item = self._rollout_step_head(g, so, hf)
                if hf:
                    # the host learns about the actions from the flag the sampling kernel writes, not from an event between head and
                    # tail: the whole step is ONE graph (one launch per group and step on the host instead of two)
                    self._rollout_step_tail(g, item, so)
            if hf or (g.tail_in_kernel and so):
                tail = None                       # nothing left to launch after the hand-over
            else:
                with torch.no_grad(), torch.cuda.graph(tail, pool=pool, stream=g.stream, capture_error_mode="thread_local"):
                    self._rollout_step_tail(g, g.item, so)
            g.graphs = (head, tail)
            g.graph_exec = head.raw_cuda_graph_exec() if plan.direct_launch else None
            g.t_dev.zero_()
        with torch.no_grad():
            torch.cuda.synchronize(self.device)
            self.buffer.bank[ss[1], ss[0]] = saved_bank
            self._kv_cache[all_ids, ss[0]] = saved_kv
            if saved_act is not None:
                self._act_dev.copy_(saved_act)
        self.buffer.address_captured = True
        ops.freeze_workspaces(self.device)
        self._step_graph = groups[0].graphs

    def get_last_value(self):
        """Value of the observation after the last step (bootstrap for GAE), with upstream's window rule:
        rows [clip(step - L, 0), clip(step, L)) and positional indices of the last stored step (trainer.py:230-236)."""
        L, lv = self.memory_length, self._lv
        step = torch.from_numpy(self.worker_current_episode_step.copy())
        start = torch.clamp(step - L, min=0)
        lv.rows.copy_(start.unsqueeze(1) + torch.arange(L, dtype=torch.int64).unsqueeze(0), non_blocking=False)
        lv.obs.copy_(self._obs_pin, non_blocking=True)
        # ~100 small launches on 32 samples: 1.4 ms eager, once per update; as a graph replay it is the kernels' own time.  The first
        # two calls run eagerly (library handles, GEMM tuning), any capture failure keeps the eager path for good.
        lv.enabled = bool(self.config.get("hip_graph_rollout", True)) and self.buffer.address_captured
        lv()
        return lv.out

    def _last_value_now(self):
        """The forward pass of ``get_last_value`` on its fixed-address operands ``_lv.rows`` / ``.obs`` -> ``.out``."""
        lv, L = self._lv, self.memory_length
        with torch.no_grad():
            mask = self._mask_table[torch.clamp(self._step_dev, 0, L - 1)]
            spec = WindowSpec.from_bank(self.buffer.bank, self._slot_dev, lv.rows, self.buffer.memory_indices[:, -1], mask)
            # previous_step_input: every worker's last action and raw reward (act_dev, the pinned block), none where its episode just ended
            pk = {} if self._prev_cfg is None else {"prev": PreviousStep(self._act_dev, self._rw_pin, self._step_dev)}
            _, last_value, _ = self.model.forward_logits(lv.obs, spec, want_items=False, **pk)
            lv.out.copy_(last_value)

    def _bootstrap_pass(self):
        """bootstrap_truncated: the value of the final observation of every episode the rollout saw cut at a time limit -> its
        element of ``buffer.bootstrap_values``, with get_last_value's window rule applied where the cut happened: rows
        [clip(s - L, 0), +L) of the episode's slot, mask row clip(s, 0, L - 1), positional indices of the episode's last stored step
        (s = the episode's length) -- what get_last_value would have returned had the rollout ended there.  No record: no launch."""
        recs, self._truncations = self._truncations, []
        self.last_truncations = [r[:4] for r in recs]
        if not recs:
            return
        # W records per execution -- get_last_value's shape: the same kernels and GEMM solutions every update, however many records
        # there are (one call over all of them meets new GEMM shapes at every new count), and get_last_value's bits
        W, bs = self.num_workers, self._bs
        n, w, t, operands = self._bootstrap_operands(recs, W)
        bs.enabled = bool(self.config.get("hip_graph_rollout", True)) and self.buffer.address_captured
        with torch.no_grad():
            values = torch.empty(w.numel(), dtype=torch.float32, device=self.device)
            for lo in range(0, w.numel(), W):
                for dst, src in zip((bs.obs, bs.slot, bs.rows, bs.pidx, bs.s) + ((bs.pa, bs.pr) if self._prev_cfg is not None else ()), operands):
                    dst.copy_(src[lo: lo + W])
                bs()
                values[lo: lo + W] = bs.out
            self.buffer.bootstrap_values[w[:n], t[:n]] = values[:n]

    def _bootstrap_operands(self, recs, chunk):
        """The records as device operands of ``_bootstrap_forward``, filled up to a multiple of ``chunk`` by repeating the last chunk's
        first record -> (number of records, w, t, (obs, slot, rows, pidx, s))."""
        L, dev, n = self.memory_length, self.device, len(recs)
        idx = list(range(n)) + [n - (n % chunk)] * (-n % chunk)
        meta = torch.tensor([recs[i][:4] for i in idx], dtype=torch.int64).to(dev)      # (w, t, slot, s)
        obs = torch.from_numpy(np.stack([np.asarray(recs[i][4]) for i in idx])).to(dev)
        if obs.dtype != self.observation_dtype:
            obs = obs.to(self.observation_dtype)
        w, t, slot, s = meta.unbind(1)
        rows = torch.clamp(s - L, min=0).unsqueeze(1) + torch.arange(L, dtype=torch.int64, device=dev).unsqueeze(0)
        operands = (obs, slot, rows, self.buffer.memory_indices[w, t], s)
        if self._prev_cfg is not None:      # previous_step_input: the action and the raw reward of the recorded (worker, step)
            wt = meta[:, :2].cpu().numpy()
            operands += (self.buffer.actions[w, t], torch.from_numpy(self.buffer.rewards[wt[:, 0], wt[:, 1]].astype(np.float32)).to(dev))
        return n, w, t, operands

    def _bootstrap_forward(self, obs, slot, rows, pidx, s, prev=None):
        mask = self._mask_table[torch.clamp(s, 0, self.memory_length - 1)]
        spec = WindowSpec.from_bank(self.buffer.bank, slot, rows, pidx, mask)
        if prev is None:
            return self.model.forward_logits(obs, spec, want_items=False)[1]
        return self.model.forward_logits(obs, spec, want_items=False, prev=prev)[1]

    def _bootstrap_chunk_now(self):
        """One chunk of the bootstrap pass on its fixed-address operands ``_bs.obs / .slot / .rows / .pidx / .s`` -> ``.out``."""
        bs = self._bs
        with torch.no_grad():
            # (previous_step_input: the episode's length s >= 1 is the step word -- the final observation always has a previous step)
            prev = None if self._prev_cfg is None else PreviousStep(bs.pa, bs.pr if self._prev_cfg["reward"] else None, bs.s)
            bs.out.copy_(self._bootstrap_forward(bs.obs, bs.slot, bs.rows, bs.pidx, bs.s, prev))

    # ------------------------------------------------------------------ optimisation
    def _train_epochs(self, learning_rate: float, clip_range: float, beta: float, perms=None):
        """``epochs`` passes over shuffled minibatches.  Returns (list of 6-stat rows, {grad key: [norms]}).  ``target_kl``: the
        optimiser steps decide on the device whether they apply (``_step_gate``); a stopped update returns rows 0 ... steps applied
        (utils.target_kl_rows), and with ``host_check: epoch`` the host looks at the gate's pinned word after every epoch but the last and
        launches no further epoch once it is set -- they would be no-ops, the results are the same bits."""
        stats, norms = [], []
        monitor = self.config.get("monitor_gradients", True)
        # sinusoidal positions: add them to the (read-only) episode bank once per update instead of once per window row,
        # block, minibatch and epoch inside the kernels (bit-identical sums; halves the kernels' window-row loads)
        with torch.no_grad():
            self._bank_pos = self._bank_with_positions()
            self._obs_train = self._training_observations()
        mbs = self.buffer.batch_size // self.buffer.n_mini_batches
        # sort_minibatch (default on): the samples of a minibatch in ascending flat (worker, step) order.  The minibatch is the
        # same SET (every loss term is a mean over it; only summation order changes), but neighbouring samples then share most of
        # their window rows, which the window pass -- every XCD handles a contiguous chunk of the samples -- turns into L2 hits
        # (measured at config 3: 37.9 -> 29.9 us per pass).  One sort per epoch covers all of its minibatches.
        sort_mb = bool(self.config.get("sort_minibatch", True))
        # step_ends_fused (default on; False: the wiring before it, kept for the bit-for-bit test): the captured step takes its
        # minibatch from a device-resident table of the epoch's index vectors and files its results in device-resident tables, under a
        # device-resident step counter -- no copy between two replays (DESIGN section 4 "The ends of the step")
        n_mb = self.buffer.n_mini_batches
        tables = bool(self._use_train_graph and self.config.get("step_ends_fused", True) and mbs * n_mb == self.buffer.batch_size
                      and (perms is None or all(len(p) == self.buffer.batch_size for p in perms)))
        row = 0
        if tables:
            self._step_tables(mbs)
            self._tg_counter.zero_()
        if self._recon is not None:
            self._begin_reconstruction()
        gate, launched = self._kl_gate, 0
        if gate is not None:
            gate.reset()
        if self._adapt is not None:
            self._adapt.reset()
        if self._attn_stats is not None:
            self._attn_stats.reset()
        host_stop = False
        for epoch in range(self.config["epochs"]):
            if gate is not None and gate.host_word is not None and epoch > 0 and not host_stop:
                self._kl_event.record(torch.cuda.current_stream(self.device))
                self._kl_event.synchronize()
                host_stop = int(gate.host_word[0]) != 0
            if perms is None:
                perm = torch.randperm(self.buffer.batch_size, device=self.device)
            else:
                perm = torch.as_tensor(perms[epoch], device=self.device, dtype=torch.long)
            if host_stop:       # the update has stopped: its remaining steps would be no-ops (the generator still moves as ever)
                continue
            if sort_mb and perm.numel() % mbs == 0:
                perm = perm.view(-1, mbs).sort(dim=1).values.reshape(-1)
            self._epoch_stats3 = None
            if tables:
                self._tg_idx_table.copy_(perm.view(n_mb, mbs))       # the index vectors of the whole epoch: one copy
            if self.dp is not None and self.dp.active and perm.numel() % mbs == 0:
                # data parallel: the global-minibatch advantage statistics of ALL minibatches of the epoch from one all-gather
                # (they depend only on the advantages and the permutation, not on the weights)
                adv = self.buffer.samples_flat["advantages"].index_select(0, perm).view(-1, mbs)
                local = torch.stack([ops.adv_stats(adv[i]) for i in range(adv.shape[0])])
                self._epoch_stats3 = self.dp.merge_adv_stats(local)
            for start in range(0, self.buffer.batch_size, mbs):
                idx = perm[start: start + mbs]
                launched += 1
                self._mb_stats3 = self._epoch_stats3[start // mbs] if self._epoch_stats3 is not None else None
                if tables:
                    self._train_step_graph(idx, learning_rate, clip_range, beta, monitor, row=row)
                    row += 1
                    continue
                if self._use_train_graph and idx.numel() == mbs:
                    st_row, norm_row = self._train_step_graph(idx, learning_rate, clip_range, beta, monitor)
                    stats.append(st_row)
                    if monitor:
                        norms.append(norm_row)
                    continue
                mini_batch = self.buffer.gather(idx)
                stats.append(self._train_mini_batch(mini_batch, learning_rate, clip_range, beta))
                if monitor:
                    norms.append(self._grad_group_norms())
        if self.model.obs_norm is not None:
            self._update_obs_norm()
        # the only host sync of the optimisation phase (target_kl with host_check: epoch waits for an event between epochs as well)
        rows = launched
        if gate is not None:
            stopped, applied, kl = gate.read()
            rows = target_kl_rows(stopped, applied, launched)
            self.last_kl_stop = {"stopped": stopped, "steps_applied": applied, "steps_launched": launched, "kl": kl, "limit": gate.limit}
        if self._adapt is not None:
            (raised, lowered), ad = self._adapt.read(), self._adapt
            self.last_adaptive_lr = {"lr": float(self.optimizer.lr_dev.item()), "raised": raised, "lowered": lowered,
                                     "kl_low": ad.kl_low, "kl_high": ad.kl_high}
        train_info = (self._tg_stats_tab[:rows] if tables else torch.stack(stats[:rows])).cpu().numpy()
        if self._kl_pen is not None:
            self._adapt_kl_penalty(train_info)
        if self._recon is not None:
            # (behind the phase's read-back: the table is complete, the copy waits for nothing) the float32 of the float64 mean
            losses = self._recon_tab[:min(rows, self._recon_tab.numel())].cpu().numpy()
            self.last_obs_reconstruction = {"loss": float(np.float32(losses.astype(np.float64).mean())), "coef": float(self._recon_coef_host)}
        if self._attn_stats is not None:       # (behind the read-back too)
            self.last_attention_statistics = attention_statistics_summary(self._attn_stats.read(), self.memory_length)
        self._bank_pos = self._row_stats = None
        self._mb_stats3 = self._epoch_stats3 = None
        grad_info = {}
        if norms or (tables and monitor):
            allnorms = (self._tg_norm_tab[:rows] if tables else torch.stack(norms[:rows])).cpu().numpy()
            grad_info = {k: allnorms[:, i].tolist() for i, k in enumerate(self._grad_keys)}
        return [row for row in train_info], grad_info

    def _adapt_kl_penalty(self, train_info):
        """kl_penalty, once per update, behind the optimisation phase's one read-back and outside every graph: kl = float32(the mean of
        column 4 over the returned rows, accumulated in double and rounded once); with ``target`` the next update's coefficient is
        utils.kl_penalty_step's, written into the device word the loss kernels read in place."""
        coef = np.float32(self._kl_coef.item())
        kl = np.float32(np.asarray(train_info)[:, 4].astype(np.float64).mean())
        nxt, moved = (coef, 0)
        if self._kl_pen["adaptive"]:
            nxt, moved = kl_penalty_step(coef, kl, self._kl_pen)
            if np.float32(nxt) != coef:
                self._kl_coef.fill_(float(nxt))
        self.last_kl_penalty = {"coef": float(coef), "next_coef": float(np.float32(nxt)), "kl": float(kl), "moved": int(moved)}

    def _begin_reconstruction(self):
        """obs_reconstruction, once per update and outside every graph: the update's coefficient into the device word (written only
        when it moved) and the steps' loss table back to row 0."""
        coef = obs_reconstruction_coef(self._recon, self.update_index)
        if coef != self._recon_coef_host:
            self._recon_coef.fill_(coef)
            self._recon_coef_host = coef
        self._recon_row.zero_()

    def _add_reconstruction(self, loss, h, obs):
        """``loss`` + coef * (the reconstruction loss of the minibatch), one loss for ``_backward_into_arena``: the decoder on ``h``
        [N, D] up to its last layer's input, then the fused last layer + sigmoid cross-entropy against ``obs`` (the minibatch's
        observations: an ``IndexedObservations`` over the NHWC copy, or the gathered NCHW rows of the eager step).  The step's unscaled
        loss goes into row ``_recon_row`` of the table of its own and the counter moves on (round the table: a step asked for from
        outside an update never leaves it)."""
        target = obs if isinstance(obs, IndexedObservations) else obs.permute(0, 2, 3, 1)
        term, out = ops.obs_reconstruction_loss(self.model.reconstruct(h), self.model.dec_conv1, target, self._recon_coef, unit_grad=True,
                                                with_out=True)
        with torch.no_grad():
            self._recon_tab.index_copy_(0, self._recon_row, out[0:1])
            self._recon_row.add_(1).remainder_(self._recon_tab.numel())
        return loss + term

    def _train_mini_batch(self, samples: dict, learning_rate: float, clip_range: float, beta: float):
        """One optimiser step on one minibatch.  Returns a device tensor [policy, value, loss, entropy, kl, clip_frac]."""
        ep = samples.get("memory_index")  # None: upstream layout, ``memories`` already gathered per sample
        bank_pos = getattr(self, "_bank_pos", None)
        if bank_pos is not None and ep is not None and samples["memories"].data_ptr() == self.buffer.bank.data_ptr():
            spec = WindowSpec.from_bank(bank_pos, ep, samples["memory_indices"], None, samples["memory_mask"])
            spec.pos_included = True
            spec.row_stats = getattr(self, "_row_stats", None)
        else:
            spec = WindowSpec.from_bank(samples["memories"], ep, samples["memory_indices"], samples["memory_indices"],
                                        samples["memory_mask"])
            if ep is not None and self.model.transformer.pos_kind == "" and samples["memories"].data_ptr() == self.buffer.bank.data_ptr():
                spec.row_stats = getattr(self, "_row_stats", None)       # (as the captured bodies do: same work on both paths)
        stats3 = getattr(self, "_mb_stats3", None)
        if stats3 is None:
            stats3 = ops.adv_stats(samples["advantages"])
            if self.dp is not None:
                stats3 = self.dp.merge_adv_stats(stats3)
        loss, stats = self._loss_from(samples["obs"], spec, samples, clip_range, beta, stats3, dyn=None)
        self._set_lr(learning_rate)
        self._backward_into_arena(loss)
        if self.dp is not None:
            self.dp.all_reduce_grads(average=False)       # the sum; the 1 / world rides in the clip coefficient below
        # global-norm clipping (the rule of torch.nn.utils.clip_grad_norm_, upstream :311) + AdamW on the flat arenas: 2 launches
        self.optimizer.step(self.config["max_grad_norm"], grad_scale=self._grad_scale(), **self._step_gate(stats))
        return stats

    def _loss_from(self, obs, spec, mb, clip_range, beta, stats3, dyn="device"):
        """Model forward + PPO loss of one minibatch (trainer.py:268-304): -> (loss, stats[6]).  Policies whose hidden size and actions
        fit (every branch of a MultiDiscrete policy together) take the fused hidden-heads + loss kernel (``fused_heads_loss``, default
        on); others the separate heads and the per-branch loss."""
        m = self.model
        # what every route takes behind its own operands, the old policy of the exact KL rules among it: a Box policy's means and log-std
        # snapshot (kl_estimator: analytic), a categorical policy's log-prob rows (exact_kl), masks or not; stats[4] is then the exact KL.
        # kl_penalty: the coefficient's device word on top, read in place
        if self.box is not None:
            kw = dict(old_mean=mb["means"], old_log_std=self.buffer.old_log_std) if self._kl_analytic else {}
        else:
            kw = dict(action_mask=mb.get("action_masks"), **(dict(old_logps=mb["old_logps"]) if self._kl_exact_cat else {}))
        if self._kl_coef is not None:
            kw["kl_coef"] = self._kl_coef
        rest = (mb["actions"], mb["log_probs"], mb["advantages"], mb["values"], clip_range, self.config["value_loss_coefficient"], beta, stats3)
        kw["dyn"] = getattr(self, "_dyn", None) if dyn == "device" else dyn
        # previous_step_input: the minibatch's rows of the buffer's fields (a negative action = no previous step); {} without the key
        pk = {} if self._prev_cfg is None else {"prev": PreviousStep(mb.get("prev_actions"), mb.get("prev_rewards"))}
        if self.box is not None:
            # Box: the fused Gaussian heads + loss kernel is the only path (check_box_policy made sure it takes the shape)
            h, _ = m.forward_state(obs, spec, **pk)
            if not ops.heads_loss_supported_gaussian(h, m.lin_policy, m.policy_branches[0]):
                raise RuntimeError("Box policy: the minibatch is outside the fused Gaussian heads + loss kernel")
            loss, stats = ops.heads_ppo_loss_gaussian(h, m.lin_policy, m.lin_value, m.policy_branches[0], m.policy_log_std, m.value, *rest, unit_grad=True, **kw)
            return (loss, stats) if self._recon is None else (self._add_reconstruction(loss, h, obs), stats)
        if self.config.get("fused_heads_loss", True) or self._recon is not None:      # (obs_reconstruction reads h on every route)
            h, _ = m.forward_state(obs, spec, **pk)
            branch = m.policy_branches[0] if len(m.policy_branches) == 1 else list(m.policy_branches)
            if self.config.get("fused_heads_loss", True) and ops.heads_loss_supported(h, m.lin_policy, branch):      # (both callers run loss.backward() on this loss)
                loss, stats = ops.heads_ppo_loss(h, m.lin_policy, m.lin_value, branch, m.value, *rest, unit_grad=True, **kw)
                return (loss, stats) if self._recon is None else (self._add_reconstruction(loss, h, obs), stats)
            h_policy = ops.linear_relu(m.lin_policy, h)
            h_value = ops.linear_relu(m.lin_value, h)
            logits, value = [br(h_policy) for br in m.policy_branches], m.value(h_value).reshape(-1)
        else:
            h = None
            logits, value, _ = m.forward_logits(obs, spec, want_items=False, **pk)
        loss, stats = ops.ppo_loss(logits, value, *rest, **kw)
        return (loss, stats) if self._recon is None else (self._add_reconstruction(loss, h, obs), stats)

    def _dw_destinations(self):
        """{parameter data_ptr: its gradient view in the flat arena}: the [out, in] views of the 2-D parameters for the grouped weight-
        gradient launch (``grouped_dw_train: false`` in the config: none, every layer multiplies its own weight gradient) and the
        1-D views (LayerNorm weights / biases, linear / convolution biases) and the convolution weights' views for the grouped
        column-sum / slice reductions (``grouped_colsum_train``)."""
        if getattr(self, "_dw_dest", None) is None:
            dw, cs = self.config.get("grouped_dw_train", True), self.config.get("grouped_colsum_train", True)
            self._dw_dest = {p.data_ptr(): v for p, v in zip(self.params, self._grad_views)
                             if (p.dim() == 2 and dw) or (p.dim() == 1 and cs) or (p.dim() == 4 and cs)}
        return self._dw_dest

    def _unit_gradient(self, loss):
        """d loss / d loss = 1 from a cached tensor (autograd would fill a fresh one every step: one launch)."""
        one = getattr(self, "_one", None)
        if one is None or one.device != loss.device or one.shape != loss.shape:
            one = self._one = torch.ones_like(loss)
        return one

    def _grad_scale(self):
        return self.dp.grad_scale if self.dp is not None else 1.0

    def _set_lr(self, learning_rate: float):
        if self._adapt is not None:         # adaptive_lr: the device owns the learning rate (the schedule gave its start value only)
            return
        self.optimizer.set_lr(learning_rate)

    def _bank_with_positions(self):
        """Episode bank with the sinusoidal positional rows pre-added, in a buffer that keeps its address (the captured
        training step reads it); None when the positional encoding is not the fixed sinusoid."""
        tr = self.model.transformer
        self._row_stats = None
        if tr.pos_kind not in ("relative", ""):
            return None
        mem = self.buffer.memories
        if tr.pos_kind == "relative":
            if getattr(self, "_bank_pos_buf", None) is None or self._bank_pos_buf.shape != self.buffer.bank.shape:
                self._bank_pos_buf = torch.empty_like(self.buffer.bank)
            out = self._bank_pos_buf[: mem.shape[0]]
            torch.add(mem, tr._pos_table[None, : mem.shape[1], None, :], out=out)
        self._row_stats = self._bank_row_stats(self._bank_pos_buf if tr.pos_kind == "relative" else self.buffer.bank, mem.shape[0])
        return self._bank_pos_buf if tr.pos_kind == "relative" else None

    def _bank_row_stats(self, bank, used):
        """Pre-LN models (norm_kv, transformer.py:128-131): LayerNorm statistics of every used row of the (position-augmented) bank,
        once per update, in a buffer [blocks, slots, T, 2] that keeps its address -- the window passes gather their per-window
        statistics from it instead of re-reading every window row (ops.WindowSpec.row_stats).  None: not applicable."""
        blk = self.model.transformer.transformer_blocks[0]
        # bank_row_stats (default on; False: every window pass computes the statistics of its own rows).  Measured at config 5:
        # optimisation phase 0.107 -> 0.102 s per update.  (It was opt-in for part of round 5: one teacher-forced flow diverged with it.
        # The cause was elsewhere -- torch's column sum in the norm_kv gradient pass's fallback inside the captured step,
        # profiles/r05/graph_reduce_hazard.txt; this option merely changed the graph enough to expose it.)
        if blk.layer_norm != "pre" or not self.buffer.block_major or not self.config.get("bank_row_stats", True):
            return None
        E, T, nb, D = bank.shape
        if D % 128 != 0 or D > 1024:
            return None
        if getattr(self, "_row_stats_buf", None) is None or self._row_stats_buf.shape != (nb, E, T, 2):
            self._row_stats_buf = torch.zeros((nb, E, T, 2), dtype=torch.float32, device=self.device)
        lib = etm_lib.load()
        st = torch.cuda.current_stream(self.device).cuda_stream
        for b in range(nb):           # the used slots of block b are one contiguous run of rows in a block-major bank
            rows = bank[:used, :, b, :]
            etm_lib.check(lib.etm_ln_row_stats(rows.data_ptr(), float(blk.norm_kv.eps), self._row_stats_buf[b].data_ptr(), used * T, D, st),
                          "etm_ln_row_stats")
        return self._row_stats_buf

    def _observations_channels_last(self):
        """Visual observations of the whole buffer in NHWC memory order, converted ONCE per update into a fixed-address buffer
        (the library convolutions of the optimisation phase run on channels_last activations; converting every gathered
        minibatch costs a 173 MB copy per minibatch at config 3).  Returns the flat [W*S, H, W, C] buffer or None."""
        obs = self.buffer.samples_flat["obs"]
        if obs.dim() != 4 or not getattr(self.model, "channels_last", False):
            return None
        n, c, h, w = obs.shape
        if getattr(self, "_obs_nhwc_buf", None) is None or self._obs_nhwc_buf.shape != (n, h, w, c):
            self._obs_nhwc_buf = torch.empty((n, h, w, c), dtype=obs.dtype, device=self.device)
        self._obs_nhwc_buf.copy_(obs.permute(0, 2, 3, 1))
        return self._obs_nhwc_buf

    def _step_tables(self, mbs):
        """Device-resident state of the table-driven step (allocated with ``_tg_idx``, whose address the captured graph holds too):
        the step counter, the epoch's index vectors [n_mini_batch, mbs], the statistics and gradient-norm rows of a whole update."""
        if getattr(self, "_tg_idx", None) is None or self._tg_idx.numel() != mbs:
            self._tg_idx = torch.empty(mbs, dtype=torch.long, device=self.device)
            self._tg_stats3 = torch.zeros(3, dtype=torch.float32, device=self.device) if self.dp is not None else None
            self._tg_idx_table, self._train_graph = None, None        # (a graph captured at another size holds the old addresses)
        if getattr(self, "_tg_idx_table", None) is None:
            n_mb, steps = self.buffer.n_mini_batches, self.config["epochs"] * self.buffer.n_mini_batches
            self._tg_counter = torch.zeros(1, dtype=torch.long, device=self.device)
            self._tg_idx_table = torch.zeros((n_mb, mbs), dtype=torch.long, device=self.device)
            self._tg_stats_tab = torch.zeros((steps, 6), dtype=torch.float32, device=self.device)
            self._tg_norm_tab = torch.zeros((steps, len(self._grad_keys)), dtype=torch.float32, device=self.device)

    def _gather_minibatch(self, keys, idx, stats3, head):
        """The per-sample fields ``keys`` of the minibatch as a dict, and the advantage statistics.  ``head``: ``idx`` is the step's
        fixed-address index vector, and ONE launch (etm_step_head) fills it from row ``counter`` of the epoch's index table, gathers
        the fields through that row and, when ``stats3`` is None, computes the statistics.  Else: ``gather_rows`` on ``idx``."""
        buf = self.buffer
        fields = [buf.samples_flat[k] for k in keys]
        if not head:
            return dict(zip(keys, ops.gather_rows(fields, idx))), stats3
        adv = buf.samples_flat["advantages"]
        own = stats3 is None and etm_lib.load().etm_adv_stats_workspace_bytes(idx.numel()) == 0      # (larger: adv_stats' split form)
        outs, st3 = ops.step_head(fields, self._tg_idx_table, self._tg_counter, idx_out=idx, adv_src=adv if own else None)
        return dict(zip(keys, outs)), (st3 if own else stats3)

    def _train_body_a(self, idx, clip_range, beta, stats3=None, head=False):
        """First half of one optimiser step on the minibatch ``idx`` (device int64 [mbs], fixed address): gather, forward,
        loss, backward, gradients packed into the flat bucket.  ``stats3``: (count, mean, M2) of the GLOBAL minibatch's
        advantages (data-parallel runs merge them over ranks before this graph); None: computed here.  ``head``: see
        ``_gather_minibatch``.  Returns stats[6]."""
        buf = self.buffer
        skip = ("obs",) if self._obs_train is not None else ()
        keys = [k for k in buf.samples_flat if k not in skip]
        mb, stats3 = self._gather_minibatch(keys, idx, stats3, head)    # one launch for the small fields
        if self._bank_pos is not None:
            spec = WindowSpec.from_bank(self._bank_pos_buf, mb["memory_index"], mb["memory_indices"], None, mb["memory_mask"])
            spec.pos_included = True
            spec.row_stats = getattr(self, "_row_stats", None)
        else:
            spec = WindowSpec.from_bank(buf.bank, mb["memory_index"], mb["memory_indices"], mb["memory_indices"], mb["memory_mask"])
            if self.model.transformer.pos_kind == "":
                spec.row_stats = getattr(self, "_row_stats", None)
        obs = mb.get("obs")
        if self._obs_train is not None:     # NHWC rows of the minibatch: gathered by the first encoder layer itself
            obs = IndexedObservations(self._obs_train, idx)
        if stats3 is None:
            stats3 = ops.adv_stats(mb["advantages"])
        loss, stats = self._loss_from(obs, spec, mb, clip_range, beta, stats3)
        self._backward_into_arena(loss)
        return stats

    def _backward_into_arena(self, loss):
        """``loss.backward()`` with every gradient ending up in its view of the flat gradient arena."""
        # backward() hands every parameter its gradient tensor (no accumulate launch while .grad is None); ONE multi-tensor copy
        # packs them into the flat bucket that the all-reduce, clipping and the fused AdamW read -- ~50 launches fewer per step
        # than accumulating into the zeroed bucket (the python-side re-aliasing below costs nothing under graph replay)
        for p in self.params:
            p.grad = None
        # the weight gradients of the dense layers (dW = dy^T x, a contraction over the minibatch with a small output) are collected
        # during backward and computed by ONE grouped launch straight into their arena views (csrc/grouped_dw.hip)
        with ops.DeferredDw(self._dw_destinations(), tail=bool(self.config.get("step_ends_fused", True))) as dw:
            loss.backward(self._unit_gradient(loss))
        dw.pack(self.params, self._grad_views, [p.grad for p in self.params])
        for p, v in zip(self.params, self._grad_views):
            p.grad = v

    def minibatch_gradients(self, idx, clip_range: float, beta: float) -> dict:
        """Un-clipped gradient of the PPO loss (trainer.py:276-310) on the minibatch ``idx`` (flat sample indices of the prepared
        buffer) under the current weights: {parameter name: tensor}.  No optimiser step, no schedule side effects -- for parity
        tests and diagnostics (the gradient is what `loss.backward()` leaves in `.grad` before upstream's clip_grad_norm_)."""
        idx = torch.as_tensor(np.asarray(idx.cpu() if torch.is_tensor(idx) else idx), device=self.device, dtype=torch.long)
        if self.config.get("sort_minibatch", True):
            idx = idx.sort().values
        with torch.no_grad():
            self._bank_pos = self._bank_with_positions()
            self._obs_train = self._training_observations()
        if self._recon is not None:
            self._begin_reconstruction()
        if self._use_train_graph:
            self._dyn.copy_(torch.tensor([clip_range, beta], dtype=torch.float64))
            self._sched_host[1:] = [clip_range, beta]
        stats3 = None
        if self.dp is not None:
            stats3 = self.dp.merge_adv_stats(ops.adv_stats(self.buffer.samples_flat["advantages"].index_select(0, idx)))
        self._train_body_a(idx, clip_range, beta, stats3)
        grads = {n: p.grad.detach().clone() for n, p in self.model.named_parameters() if p.requires_grad}
        self._bank_pos = self._row_stats = None
        return grads

    def _step_gate(self, stats):
        """What the optimiser's step takes besides the clipping: ``gate`` (``target_kl``: the update's gate) and ``adapt``
        (``adaptive_lr``: the learning-rate rule), each with its ``kl`` pointed at element 4 of the step's own statistics (the k3 estimate
        of the loss on the weights before the step), each None without its key."""
        gate, adapt = self._kl_gate, self._adapt
        if gate is not None or adapt is not None:
            if stats is None or stats.dtype != torch.float32 or stats.dim() != 1 or stats.numel() < 5 or not stats.is_contiguous():
                raise RuntimeError("target_kl / adaptive_lr: the step's statistics must be a contiguous float32 vector with the kl at index 4")
            kl = stats[4:5]
            if gate is not None:
                gate.kl = kl
            if adapt is not None:
                adapt.kl = kl
        return {"gate": gate, "adapt": adapt}

    def _train_body_b(self, monitor, stats=None, kl_stats=None):
        """Second half: global-norm clipping (same rule as torch.nn.utils.clip_grad_norm_, upstream :311) on the flat bucket,
        fused AdamW, monitored gradient norms.  ``stats`` (the table-driven step): the step's statistics; they and the norms are
        filed under row ``counter`` of the result tables and the counter moves on, inside the norm monitor's two launches.
        ``kl_stats`` (``target_kl`` / ``adaptive_lr``): the step's statistics in every form of the step, for the optimiser's gate and
        learning-rate rule."""
        self.optimizer.step(self.config["max_grad_norm"], grad_scale=self._grad_scale(),
                            **(self._step_gate(kl_stats) if self._kl_gate is not None or self._adapt is not None else {}))
        if stats is None:
            return self._grad_group_norms() if monitor else None
        if stats.numel() != self._tg_stats_tab.shape[1] or stats.dtype != torch.float32 or not stats.is_contiguous():
            raise RuntimeError("the step's statistics do not fit the rows of the statistics table")
        if monitor:
            return self._grad_group_norms(step=(stats, self._tg_stats_tab, self._tg_norm_tab, self._tg_counter))
        etm_lib.check(etm_lib.load().etm_step_end(stats.data_ptr(), stats.numel(), self._tg_stats_tab.data_ptr(), self._tg_stats_tab.shape[0],
                                                  self._tg_counter.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "etm_step_end")
        return None

    def _train_step_graph(self, idx, learning_rate, clip_range, beta, monitor, row=None):
        """Minibatch step through captured graphs (two eager warm-up steps first).  Single GPU: one graph.  Data parallel: the
        merged advantage statistics are computed eagerly first (one all-gather per epoch), then ONE graph that holds the packed
        gradients' RCCL all-reduce between the backward pass and clip + AdamW (round 6; upstream insertion point trainer.py:310-311)
        when the library collective's captured form passed its self-test on every rank (etm/dist.py: graph_collective_ok) --
        otherwise graph A, the all-reduce as a host call, graph B.  Returns (stats[6], norms or None).
        ``row`` (``_train_epochs``, table-driven step): ``idx`` is row ``row % n_mini_batch`` of the index table already and the
        device counter stands at ``row``; the results stay in row ``row`` of the result tables and nothing is returned."""
        dp = self.dp
        tables = bool(self.config.get("step_ends_fused", True))
        if getattr(self, "_tg_idx", None) is None:
            if tables:
                self._step_tables(idx.numel())
            else:
                self._tg_idx = torch.empty_like(idx)
                self._tg_stats3 = torch.zeros(3, dtype=torch.float32, device=self.device) if dp is not None else None
                self._tg_idx_table = None
        tables = self._tg_tables = tables and self._tg_idx_table is not None
        if not tables:
            self._tg_idx.copy_(idx)
        elif row is None:                   # a single step asked for from outside _train_epochs: an "update" of one step
            self._tg_counter.zero_()
            if self._kl_gate is not None:
                self._kl_gate.reset()
            if self._adapt is not None:
                self._adapt.reset()
            self._tg_idx_table[0].copy_(idx)
        self._set_lr(learning_rate)
        if self._sched_host[1] != clip_range or self._sched_host[2] != beta:
            self._dyn.copy_(torch.tensor([clip_range, beta], dtype=torch.float64))
            self._sched_host[1:] = [clip_range, beta]
        if dp is not None:
            if getattr(self, "_mb_stats3", None) is not None:
                self._tg_stats3.copy_(self._mb_stats3)
            else:
                adv = self.buffer.samples_flat["advantages"].index_select(0, idx if tables else self._tg_idx)
                self._tg_stats3.copy_(dp.merge_adv_stats(ops.adv_stats(adv)))
        self._mb_counter += 1
        sample_eager = self.profile_sample_every and self._mb_counter % self.profile_sample_every == 0
        key = (monitor, self._bank_pos is not None)
        overlap = self._dp_overlap_ready()
        one_graph = bool(dp is not None and self.config.get("dp_graph_collective", True) and dp.graph_collective_ok()
                         and not getattr(self, "_dp_one_graph_failed", False))
        if (self._train_graph is None and self._train_warm < 2) or sample_eager:
            self._train_warm += 1
            if overlap:
                st, dfe = self._train_body_a1(self._tg_idx, clip_range, beta, self._tg_stats3, head=tables)
                self._allreduce_rest_async()
                self._train_body_a2(dfe)
                self._allreduce_conv_and_join()
            else:
                st = self._train_body_a(self._tg_idx, clip_range, beta, self._tg_stats3, head=tables)
                if dp is not None:
                    dp.all_reduce_grads(average=False)
            nm = self._train_body_b(monitor, st if tables else None, kl_stats=st)
            if tables:
                return self._step_rows(row, monitor)
            return st.clone(), (nm.clone() if nm is not None else None)
        if self._train_graph is None or self._tg_key != key:
            torch.cuda.synchronize(self.device)
            ga, gb, ga2 = self._capture_one_graph_dp_step(clip_range, beta, monitor, overlap) if one_graph else None, None, None
            one_graph = ga is not None
            if dp is not None and dp.world > 1 and self.config.get("dp_graph_collective", True) and dp.graph_collective_ok():
                # every rank must replay the same form: a rank whose capture failed takes everybody to the three-call step
                if not dp.agree(one_graph):
                    ga, one_graph, self._dp_one_graph_failed = None, False, True
            if ga is None:
                ga = torch.cuda.CUDAGraph()
                # (one memory pool for the pieces of the overlapped step: part 2 reads tensors part 1 allocated)
                pool = torch.cuda.graph_pool_handle() if overlap else None
                with torch.cuda.graph(ga, pool=pool, capture_error_mode="thread_local"):
                    if overlap:
                        self._tg_stats, self._tg_dfeats = self._train_body_a1(self._tg_idx, clip_range, beta, self._tg_stats3, head=tables)
                    else:
                        self._tg_stats = self._train_body_a(self._tg_idx, clip_range, beta, self._tg_stats3, head=tables)
                    if dp is None:
                        self._tg_norms = self._train_body_b(monitor, self._tg_stats if tables else None, kl_stats=self._tg_stats)
                if overlap:
                    ga2 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(ga2, pool=pool, capture_error_mode="thread_local"):
                        self._train_body_a2(self._tg_dfeats)
                if dp is not None:
                    gb = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gb, pool=pool, capture_error_mode="thread_local"):
                        self._tg_norms = self._train_body_b(monitor, self._tg_stats if tables else None)
            self._train_graph, self._tg_key, self._train_graph_a2 = (ga, gb), key, ga2
            self._dp_one_graph = one_graph
            self.buffer.address_captured = True
            ops.freeze_workspaces(self.device)
        ga, gb = self._train_graph
        ga.replay()
        if gb is not None:
            if getattr(self, "_train_graph_a2", None) is not None:
                self._allreduce_rest_async()                # heads + transformer + lin_hidden slice on the side stream ...
                self._train_graph_a2.replay()               # ... under the encoder's backward pass
                self._allreduce_conv_and_join()
            else:
                dp.all_reduce_grads(average=False)
            gb.replay()
        if tables:
            return self._step_rows(row, monitor)
        return self._tg_stats.clone(), (self._tg_norms.clone() if monitor else None)

    def _step_rows(self, row, monitor):
        """What a table-driven step hands back: nothing inside ``_train_epochs`` (the rows are read once, after the last step); row 0
        of the result tables for a single step asked for from outside."""
        if row is not None:
            return None, None
        return self._tg_stats_tab[0].clone(), (self._tg_norm_tab[0].clone() if monitor else None)

    def evaluate(self, episodes_per_worker=1, n_workers=None, deterministic=True, seed=None, worker_steps=None) -> dict:
        """Plays ``episodes_per_worker`` whole episodes in each of ``n_workers`` (None: the config's) held-out environments with the
        current weights, through the same step kernels and captured step graphs as a training rollout -> {"episodes", "result",
        "steps", "seconds"} (evaluation.Evaluator).  ``deterministic``: the mode of the policy at every step, else sampled from the
        evaluator's own generator.  ``seed`` (None: ``evaluation.seed``, or else 100000): the first worker id of the evaluation's
        environments and the seed of sampled draws.  The evaluator owns its environments and rollout state: training with
        evaluations interleaved computes the same bits as training without."""
        from evaluation import Evaluator, evaluation_defaults
        ev = evaluation_defaults(self.config)
        if self._evaluator is None:
            self._evaluator = Evaluator(self.config, self.device, self.run_id, parameters=lambda: self.optimizer.flat_params,
                                        buffers=lambda: dict(self.model.named_buffers()))
        return self._evaluator.run(episodes_per_worker=int(episodes_per_worker), n_workers=n_workers, deterministic=bool(deterministic),
                                   seed=ev["seed"] if seed is None else int(seed),
                                   worker_steps=ev["worker_steps"] if worker_steps is None else int(worker_steps))

    def close(self, exit_process: bool = False) -> None:
        """Releases environments and the summary writer (upstream also ``exit(0)``s; opt in with exit_process)."""
        if getattr(self, "_evaluator", None) is not None:
            self._evaluator.close()
            self._evaluator = None
        if getattr(self, "_shm_registered", None):
            try:
                torch.cuda.synchronize(self.device)
                etm_lib.load().etm_host_unregister(self._shm_registered)
            except Exception:
                pass
            self._shm_registered = None
        for closer in (self.env.close, self.writer.close):
            try:
                closer()
            except Exception:
                pass
        if exit_process:
            time.sleep(1.0)
            raise SystemExit(0)
