"""Rollout buffer + whole-episode memory bank, resident in HBM.

API of upstream buffer.py (constructor, fields, prepare_batch_dict / mini_batch_generator / calc_advantages), with
the storage redesigned for the MI355X path:

* every sample tensor lives on the device; ``rewards`` / ``dones`` / ``memory_index`` are produced by the host-side
  environment loop, so they are pinned host arrays that are uploaded once per update;
* ``memories`` is not a python list of per-episode tensors (upstream buffer.py:40, trainer.py:154,205-213) but the
  first ``num_episodes`` slots of one preallocated bank [capacity, T, blocks, D]: a live episode writes its items
  straight into its slot, finishing an episode just opens a new (zero) slot -- no clone, no ``torch.stack``;
* minibatches carry *indices* (``memory_index`` [N] into the bank + ``memory_indices`` [N, L]); the attention kernel
  gathers the window rows in place, so upstream's 906 MB ``memories[memory_index[idx]]`` copy (buffer.py:90) and the
  [N, L, blocks, D] gather (trainer.py:271) do not exist.  ``materialize=True`` reproduces upstream's minibatch
  layout for API users that want it.
* GAE (buffer.py:95-113) is the ``etm_gae`` kernel, bit-identical to the upstream loop.
* ``bootstrap_truncated: true`` (absent upstream): ``truncated`` [W, S] marks the steps whose episode was only cut at a time limit,
  ``bootstrap_values`` [W, S] holds the value of the observation after the cut; GAE (``etm_gae_truncated``) takes the next value of
  such a step from there instead of 0.  Neither is allocated without the key.
* ``normalize_rewards`` (absent upstream): ``calc_advantages`` scales the uploaded rewards by the running spread of the discounted
  return (``etm_return_scale``) into ``rewards_scaled`` [W, S], which GAE reads; ``rewards`` keeps the raw values.  The running triple
  ``ret_stats`` and the per-worker returns ``ret_carry`` are float64 device arrays that live as long as the buffer (trainer state: not
  in the model file; the training checkpoint of ``PPOTrainer.save_checkpoint`` stores the triple).  Nothing is allocated without the key.
* ``action_masks: true`` (absent upstream): ``action_masks_host`` [W, S] is the pinned array the environment loop writes each step's
  invalid-action word into (bit j = column j of the concatenated policy head is allowed), ``action_masks`` [W, S] int64 its device
  copy (uploaded by ``prepare_batch_dict``) and a member of ``samples_flat``, so every minibatch carries its samples' words.  Without
  the key neither exists and ``samples_flat`` has its usual keys.
* ``kl_estimator: analytic`` (absent upstream; Box policies): ``means`` [W, S, A], the rollout's Gaussian means, a member of
  ``samples_flat``, and ``old_log_std`` [A], the log-std that drew them, copied once per update by ``prepare_batch_dict``.  They live
  for one rollout (nothing of them is in a checkpoint).  Without the key neither exists.
* ``exact_kl: true`` (absent upstream): on a Box policy exactly the two fields above; on a Discrete / MultiDiscrete policy (masked or
  not) ``old_logps`` [W, S, sum A_b], the rollout's log-probs of every column of every branch (-inf where a column was masked out), a
  member of ``samples_flat``.  The rows live for one rollout (nothing of them is in a checkpoint).  Without the key it does not exist.
* ``kl_penalty`` (absent upstream) implies ``exact_kl: true``: the same fields, for either policy kind (the penalty is a term in that KL).
* ``previous_step_input`` (absent upstream): ``prev_actions`` [W, S, B] int64 (-1 at an episode's first step) and, with the reward,
  ``prev_rewards`` [W, S] float32 (the raw reward, 0 there), members of ``samples_flat``; built on the device after the rollout by
  ``build_previous_step`` (utils.previous_step_fields is the rule) with a per-worker carry across rollouts that a restart clears
  (nothing of them is in a checkpoint).  Without the key neither exists.
"""
import numpy as np
import torch

from etm import ops
from run_settings import kl_plumbing
from utils import normalization_section, previous_step_input_section


class Buffer:
    def __init__(self, config: dict, observation_space, action_space_shape: tuple, max_episode_length: int,
                 device: torch.device, continuous: bool = False, observation_dtype: torch.dtype = torch.float32) -> None:
        """``observation_dtype``: ``torch.uint8`` keeps image observations as the bytes the environment emits (byte k stands for
        float32(k) / float32(255); the encoder's first layer reads them) -- ``obs`` is then a quarter of its float32 size."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Buffer is HBM-resident: it needs the MI355X (HIP) device; there is no CPU path in this build")
        self.n_workers = config["n_workers"]
        self.worker_steps = config["worker_steps"]
        self.n_mini_batches = config["n_mini_batch"]
        self.batch_size = self.n_workers * self.worker_steps
        self.mini_batch_size = self.batch_size // self.n_mini_batches
        self.max_episode_length = max_episode_length
        t = config["transformer"]
        self.memory_length, self.num_blocks, self.embed_dim = t["memory_length"], t["num_blocks"], t["embed_dim"]
        W, S, L, dev = self.n_workers, self.worker_steps, self.memory_length, self.device
        B = action_space_shape[0] if continuous else len(action_space_shape)      # (Box: the A dimensions of one action)

        pin = lambda shape, dtype: torch.zeros(shape, dtype=dtype).pin_memory()
        self._rewards_host = pin((W, S), torch.float32)
        self._dones_host = pin((W, S), torch.bool)
        self._memory_index_host = pin((W, S), torch.int64)
        self.rewards = self._rewards_host.numpy()            # written by the env loop
        self.dones = self._dones_host.numpy()
        self.memory_index_host = self._memory_index_host.numpy()
        self.rewards_dev = torch.zeros((W, S), dtype=torch.float32, device=dev)
        self.dones_dev = torch.zeros((W, S), dtype=torch.bool, device=dev)
        # time-limit truncations (bootstrap_truncated: true): flags from the env loop like ``dones``, values from the trainer's
        # bootstrap pass; None without the key
        self.truncated = self.truncated_dev = self.bootstrap_values = None
        if config.get("bootstrap_truncated", False):
            self._truncated_host = pin((W, S), torch.bool)
            self.truncated = self._truncated_host.numpy()
            self.truncated_dev = torch.zeros((W, S), dtype=torch.bool, device=dev)
            self.bootstrap_values = torch.zeros((W, S), dtype=torch.float32, device=dev)

        # invalid-action words (action_masks: true): written by the env loop like ``memory_index_host``; None without the key
        self.action_masks = self.action_masks_host = None
        if config.get("action_masks", False):
            self._action_masks_host = pin((W, S), torch.int64)
            self.action_masks_host = self._action_masks_host.numpy()
            self.action_masks = torch.zeros((W, S), dtype=torch.int64, device=dev)

        # the exact Gaussian KL (kl_estimator: analytic, Box policies): the rollout's means [W, S, A] next to ``actions`` (a member of
        # ``samples_flat``, so every minibatch carries its samples' old means) and a snapshot of the log-std that drew them -- the
        # parameter moves during the update --, taken by ``prepare_batch_dict`` from ``log_std_source`` (the trainer sets it: the
        # model's policy_log_std); None without the key
        self.means = self.old_log_std = self.log_std_source = None
        kl_analytic, kl_exact_cat = kl_plumbing(config, continuous)      # (the rule the trainer stages by)
        if kl_analytic:
            if not continuous:
                raise ValueError("kl_estimator: analytic needs a Box (continuous) policy; remove the key")
            self.means = torch.zeros((W, S, B), dtype=torch.float32, device=dev)
            self.old_log_std = torch.zeros(B, dtype=torch.float32, device=dev)
        # the exact categorical KL (exact_kl: true, Discrete / MultiDiscrete policies, masked or not): the rollout's log-probs of every
        # column of every branch [W, S, sum A_b] next to ``actions``, a member of ``samples_flat``; None without the key
        self.old_logps = None
        if kl_exact_cat:
            self.old_logps = torch.zeros((W, S, sum(int(a) for a in action_space_shape)), dtype=torch.float32, device=dev)

        # previous_step_input (absent upstream): what the model is fed of step t - 1 at every sample -- ``prev_actions`` [W, S, B] int64
        # (-1 in every branch at an episode's first step) and, with the reward, ``prev_rewards`` [W, S] float32 (the RAW reward, 0 there);
        # members of ``samples_flat``.  Built on the device after the rollout (``build_previous_step``; utils.previous_step_fields is the
        # rule) from ``actions``, the raw rewards, the done flags and the carry of the rollout before: the last step's action and reward
        # per worker and whether its episode goes on (``prev_live``; all False at the start and after a restart).  None without the key
        self.prev_actions = self.prev_rewards = self.prev_live = None
        prev_cfg = None if continuous else previous_step_input_section(config)
        if prev_cfg is not None:
            self.prev_actions = torch.full((W, S, B), -1, dtype=torch.int64, device=dev)
            self.prev_rewards = torch.zeros((W, S), dtype=torch.float32, device=dev) if prev_cfg["reward"] else None
            self._prev_carry_a = torch.full((W, B), -1, dtype=torch.int64, device=dev)
            self._prev_carry_r = torch.zeros(W, dtype=torch.float32, device=dev)
            self.prev_live = torch.zeros(W, dtype=torch.bool, device=dev)

        # return-based reward scaling (normalize_rewards): None without the key
        self.return_norm = normalization_section(config, "normalize_rewards")
        self.rewards_scaled = self.ret_carry = self.ret_stats = self.return_scale = None
        if self.return_norm is not None:
            self.rewards_scaled = torch.zeros((W, S), dtype=torch.float32, device=dev)
            self.ret_carry = torch.zeros(W, dtype=torch.float64, device=dev)
            self.ret_stats = torch.zeros(3, dtype=torch.float64, device=dev)
            self._ret_ws = ops.return_scale_workspace(W, dev)
            self.return_scale = self._ret_ws[:4].view(torch.float32)       # (the scale of the last call; 0 before the first)

        # (Box: the raw float actions [W, S, A] and one joint log-prob per sample)
        self.actions = torch.zeros((W, S, B), dtype=torch.float32 if continuous else torch.long, device=dev)
        if observation_dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"observations are float32 or uint8, got {observation_dtype}")
        self.obs = torch.zeros((W, S) + tuple(observation_space.shape), dtype=observation_dtype, device=dev)
        self.log_probs = torch.zeros((W, S, 1 if continuous else B), dtype=torch.float32, device=dev)
        self.values = torch.zeros((W, S), dtype=torch.float32, device=dev)
        self.advantages = torch.zeros((W, S), dtype=torch.float32, device=dev)
        self.memory_mask = torch.zeros((W, S, L), dtype=torch.bool, device=dev)
        self.memory_index = torch.zeros((W, S), dtype=torch.long, device=dev)
        self.memory_indices = torch.zeros((W, S, L), dtype=torch.long, device=dev)

        # whole-episode memory bank: slot e holds one episode's [T, blocks, D] items
        # default capacity = worst case (every step ends an episode): the bank then never reallocates, which keeps its
        # address stable for the captured rollout graph; 288 GB of HBM make this affordable (7.3 GB at BASELINE config 3)
        cap = config.get("episode_bank_capacity", W + self.batch_size)
        # BLOCK-MAJOR in memory (round 4): [blocks][slots][T][D] -- the L window rows of a (sample, block) are one
        # contiguous run of L * D floats (upstream's [slots, T, blocks, D] order interleaves the blocks: a row every blocks * D floats).
        # ``bank`` keeps upstream's logical shape [slots, T, blocks, D] as a VIEW; every kernel addresses it through its strides
        # (etm/ops.py:WindowSpec.from_bank, the tail of etm_rollout_trxl).  (Round 3's interleaved order was an option until round 6:
        # window passes 8 % slower at config 3)
        self.block_major = True
        self.bank = self._new_bank(cap)
        self.num_episodes = W
        self.address_captured = False      # set by the trainer once a captured graph reads / writes the bank
        self.samples_flat = None

    def _new_bank(self, slots: int) -> torch.Tensor:
        shape = (slots, self.max_episode_length, self.num_blocks, self.embed_dim)
        store = torch.zeros((self.num_blocks, slots, self.max_episode_length, self.embed_dim), dtype=torch.float32, device=self.device)
        return store.permute(1, 2, 0, 3)

    # ------------------------------------------------------------------ episode bank
    @property
    def memories(self):
        """[E, T, blocks, D] -- the episodes referenced by ``memory_index`` (upstream: stacked list, buffer.py:65)."""
        return self.bank[: self.num_episodes]

    def begin_rollout(self, live_slots: torch.Tensor):
        """Start of an update: live episodes move to slots 0..W-1, every other used slot is cleared."""
        # the pinned bookkeeping arrays (memory_index, rewards, done flags) are the sources of ASYNCHRONOUS uploads of the previous
        # update (prepare_batch_dict, calc_advantages): the host must not rewrite them before those copies have run.  With an
        # optimisation phase in between they long have; a caller that samples again at once (tests, tools) runs ahead of the device
        # since round 6 (get_last_value is one graph launch instead of ~100 eager ones) and would hand the copy the NEW contents.
        ev = getattr(self, "_host_arrays_uploaded", None)
        if ev is not None:
            ev.synchronize()
        W = self.n_workers
        live = self.bank.index_select(0, live_slots)
        self.bank[:W].copy_(live)
        if self.num_episodes > W:
            self.bank[W: self.num_episodes].zero_()
        self.num_episodes = W
        self.memory_index_host[:] = np.arange(W, dtype=np.int64)[:, None]
        if self.truncated is not None:
            self.truncated[:] = False
            self.bootstrap_values.zero_()

    def _mark_host_arrays_uploaded(self):
        if self.device.type == "cuda":
            if getattr(self, "_host_arrays_uploaded", None) is None:
                self._host_arrays_uploaded = torch.cuda.Event()
            self._host_arrays_uploaded.record(torch.cuda.current_stream(self.device))

    def open_episode(self) -> int:
        """Reserve the next (zero-filled) slot and return its index; grows the bank if it is full."""
        if self.num_episodes == self.bank.shape[0]:
            if self.address_captured:
                raise RuntimeError(f"episode bank is full ({self.bank.shape[0]} slots) and captured HIP graphs hold its address: raise "
                                   "episode_bank_capacity (default n_workers * (worker_steps + 1) never fills) or disable "
                                   "hip_graph_rollout / hip_graph_train")
            grown = self._new_bank(2 * self.bank.shape[0])
            grown[: self.bank.shape[0]].copy_(self.bank)
            self.bank = grown
        slot = self.num_episodes
        self.num_episodes += 1
        return slot

    # ------------------------------------------------------------------ upstream API
    def prepare_batch_dict(self) -> None:
        """Upload the host-side bookkeeping and expose the samples flattened to [W*S, ...] (W-major, views)."""
        self.memory_index.copy_(self._memory_index_host, non_blocking=True)
        if self.action_masks is not None:
            self.action_masks.copy_(self._action_masks_host, non_blocking=True)
        if self.old_log_std is not None:
            if self.log_std_source is None:
                raise RuntimeError("kl_estimator: analytic: the buffer has no log_std_source to take the update's snapshot from")
            self.old_log_std.copy_(self.log_std_source.detach().reshape(-1))       # one device-to-device copy per update
        self._mark_host_arrays_uploaded()
        samples = {
            "actions": self.actions, "values": self.values, "log_probs": self.log_probs, "advantages": self.advantages,
            "obs": self.obs, "memory_mask": self.memory_mask, "memory_index": self.memory_index,
            "memory_indices": self.memory_indices,
        }
        if self.action_masks is not None:
            samples["action_masks"] = self.action_masks
        if self.means is not None:
            samples["means"] = self.means
        if self.old_logps is not None:
            samples["old_logps"] = self.old_logps
        if self.prev_actions is not None:
            samples["prev_actions"] = self.prev_actions
        if self.prev_rewards is not None:
            samples["prev_rewards"] = self.prev_rewards
        self.samples_flat = {k: v.reshape(v.shape[0] * v.shape[1], *v.shape[2:]) for k, v in samples.items()}

    def mini_batch_generator(self, indices: torch.Tensor = None, materialize: bool = False):
        """Yield shuffled minibatches.  ``indices``: optional explicit permutation (tests / teacher forcing).

        Each dict has the upstream keys ``actions, values, log_probs, advantages, obs, memory_mask, memory_indices``
        plus ``memory_index`` [N] and ``memories`` = the episode bank [E, T, blocks, D] (indexed by ``memory_index``).
        With ``materialize=True`` ``memories`` is upstream's gathered [N, T, blocks, D] tensor instead.
        """
        if indices is None:
            indices = torch.randperm(self.batch_size, device=self.device)
        else:
            indices = torch.as_tensor(indices, device=self.device, dtype=torch.long)
        mbs = self.batch_size // self.n_mini_batches
        for start in range(0, self.batch_size, mbs):
            idx = indices[start: start + mbs]
            mini_batch = {k: v.index_select(0, idx) for k, v in self.samples_flat.items()}
            if materialize:
                mini_batch["memories"] = self.memories[mini_batch.pop("memory_index")]
            else:
                mini_batch["memories"] = self.memories
            yield mini_batch

    def gather(self, idx: torch.Tensor, materialize: bool = False) -> dict:
        """One minibatch dict (see ``mini_batch_generator``) for the flat sample indices ``idx``."""
        mini_batch = {k: v.index_select(0, idx) for k, v in self.samples_flat.items()}
        mini_batch["memories"] = self.memories[mini_batch.pop("memory_index")] if materialize else self.memories
        return mini_batch

    def build_previous_step(self) -> None:
        """previous_step_input: ``prev_actions`` / ``prev_rewards`` of the rollout just staged, on the device, and the carry for the next
        one (utils.previous_step_fields).  After ``calc_advantages``: ``rewards_dev`` (raw) and ``dones_dev`` are this rollout's."""
        a, r, d = self.actions, self.rewards_dev, self.dones_dev
        live = self.prev_live
        self.prev_actions[:, 0] = torch.where(live.unsqueeze(1), self._prev_carry_a, torch.full_like(self._prev_carry_a, -1))
        self.prev_actions[:, 1:] = torch.where(d[:, :-1].unsqueeze(2), torch.full_like(a[:, :-1], -1), a[:, :-1])
        if self.prev_rewards is not None:
            self.prev_rewards[:, 0] = torch.where(live, self._prev_carry_r, torch.zeros_like(self._prev_carry_r))
            self.prev_rewards[:, 1:] = torch.where(d[:, :-1], torch.zeros_like(r[:, :-1]), r[:, :-1])
        self._prev_carry_a.copy_(a[:, -1])
        self._prev_carry_r.copy_(r[:, -1])
        self.prev_live.copy_(~d[:, -1])

    def calc_advantages(self, last_value: torch.Tensor, gamma: float, lamda: float) -> None:
        """GAE over the [W, S] buffer on device (upstream buffer.py:95-113)."""
        self.rewards_dev.copy_(self._rewards_host, non_blocking=True)
        self.dones_dev.copy_(self._dones_host, non_blocking=True)
        if self.truncated is not None:
            self.truncated_dev.copy_(self._truncated_host, non_blocking=True)
        self._mark_host_arrays_uploaded()
        rewards = self.rewards_dev
        if self.return_norm is not None:
            # the rollout's returns continue from ret_carry and join the running triple; the rewards GAE reads are scaled with the
            # triple that already includes this rollout
            rewards, _ = ops.return_scale(self.rewards_dev, self.dones_dev, self.ret_carry, self.ret_stats, gamma, self.return_norm["epsilon"],
                                          self.return_norm["clip"], out=self.rewards_scaled, ws=self._ret_ws)
        if self.truncated is not None:
            ops.gae(rewards, self.dones_dev, self.values, last_value.detach(), gamma, lamda, out=self.advantages,
                    truncated=self.truncated_dev, boot=self.bootstrap_values)
            return
        ops.gae(rewards, self.dones_dev, self.values, last_value.detach(), gamma, lamda, out=self.advantages)
