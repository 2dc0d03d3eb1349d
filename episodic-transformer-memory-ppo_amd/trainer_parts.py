"""Parts of ``PPOTrainer`` (trainer.py) that are not the sampler / optimiser core, as mix-ins (round 6: trainer.py was 1,591 lines):

* ``_DataParallelStep``   the overlapped / one-graph forms of the data-parallel minibatch step (insertion point upstream trainer.py:310-311);
* ``_NativeRolloutDrive`` the rollout loop through the kernel library's driver (worker processes; upstream trainer.py:159-218);
* ``_RunOutputs``         TensorBoard summaries, the monitored gradient norms and the checkpoint (upstream trainer.py:325-362, model.py:128-151);
* ``_CheckpointResume``   the training checkpoint next to upstream's model file, loading it in place, restarting the episodes.

Every method runs on the trainer's own attributes; nothing here is importable on its own."""
import os
import pickle
import sys

import numpy as np
import torch

from etm import lib as etm_lib
from etm import ops
from etm.ops import WindowSpec
from model import IndexedObservations


class _DataParallelStep:
    # ---- data-parallel overlap (dp_overlap, SURVEY 8e / upstream insertion point trainer.py:310-311): the backward pass is cut at the
    # encoder output.  Part 1 (heads, transformer, lin_hidden: 98 % of the gradient arena) is summed over the ranks on a side stream
    # while part 2 (the encoder's backward, ~0.5 ms at config 3) runs; the small convolution slice follows on the main stream.
    def _train_body_a1(self, idx, clip_range, beta, stats3=None, head=False):
        """Gather, forward, loss, backward DOWN TO the encoder features; every gradient except the convolutions' is in its arena
        view afterwards.  Returns (stats[6], d loss / d features) -- the features themselves stay in ``self.model._encoder_features``."""
        buf = self.buffer
        skip = ("obs",) if self._obs_train is not None else ()
        keys = [k for k in buf.samples_flat if k not in skip]
        mb, stats3 = self._gather_minibatch(keys, idx, stats3, head)
        if self._bank_pos is not None:
            spec = WindowSpec.from_bank(self._bank_pos_buf, mb["memory_index"], mb["memory_indices"], None, mb["memory_mask"])
            spec.pos_included = True
            spec.row_stats = getattr(self, "_row_stats", None)
        else:
            spec = WindowSpec.from_bank(buf.bank, mb["memory_index"], mb["memory_indices"], mb["memory_indices"], mb["memory_mask"])
            if self.model.transformer.pos_kind == "":
                spec.row_stats = getattr(self, "_row_stats", None)
        obs = IndexedObservations(self._obs_train, idx)
        if stats3 is None:
            stats3 = ops.adv_stats(mb["advantages"])
        self.model._encoder_features, self.model._keep_encoder_features = None, True
        try:
            loss, stats = self._loss_from(obs, spec, mb, clip_range, beta, stats3)
        finally:
            self.model._keep_encoder_features = False
        feats = self.model._encoder_features
        if feats is None or feats.grad_fn is None:
            raise RuntimeError("dp_overlap needs the hand-written training encoder (visual observations, fused_train_encoder)")
        n_conv = self._n_conv_params
        rest = self.params[n_conv:]
        for p in self.params:
            p.grad = None
        with ops.DeferredDw(self._dw_destinations(), tail=bool(self.config.get("step_ends_fused", True))) as dw:
            got = torch.autograd.grad(loss, [feats] + rest, grad_outputs=self._unit_gradient(loss), allow_unused=True)
        dw.pack(rest, self._grad_views[n_conv:], got[1:])
        return stats, got[0]

    def _train_body_a2(self, dfeats):
        """The encoder's backward pass from d loss / d features; the convolutions' gradients end up in their arena views."""
        feats = self.model._encoder_features
        n_conv = self._n_conv_params
        convs = self.params[:n_conv]
        with ops.DeferredDw(self._dw_destinations(), tail=bool(self.config.get("step_ends_fused", True))) as dw:
            got = torch.autograd.grad(feats, convs, grad_outputs=dfeats, allow_unused=True)
        dw.pack(convs, self._grad_views[:n_conv], got)
        for p, v in zip(self.params, self._grad_views):
            p.grad = v
        self.model._encoder_features = None

    def _dp_overlap_ready(self):
        """dp_overlap applies when the run is data parallel, the optimisation phase runs the hand-written encoder on indexed
        observations, and the convolution parameters are the FIRST parameters of the arena (model.py: conv1..3 are created first)."""
        if self.dp is None or not self.config.get("dp_overlap", False) or self._obs_train is None:
            return False
        if getattr(self, "_n_conv_params", None) is None:
            names = [n for n, _ in self.model.arena_parameters()]
            k = 0
            while k < len(names) and names[k].startswith("conv"):
                k += 1
            self._n_conv_params = k if (k > 0 and not any(n.startswith("conv") for n in names[k:])) else 0
            self._conv_floats = sum(p.numel() for p in self.params[: self._n_conv_params])
            v0, vk = self._grad_views[0], self._grad_views[self._n_conv_params]
            if self._n_conv_params and (vk.data_ptr() - v0.data_ptr()) // 4 != self._conv_floats:
                self._conv_floats = (vk.data_ptr() - v0.data_ptr()) // 4        # (arena views are padded: the slice boundary in floats)
            self._ar_side = torch.cuda.Stream(device=self.device)
            self._ar_fork, self._ar_fork2, self._ar_join = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        return self._n_conv_params > 0

    def _capture_one_graph_dp_step(self, clip_range, beta, monitor, overlap):
        """Data-parallel minibatch step as ONE graph (round 6): gather, forward, loss, backward, the library's RCCL all-reduce of
        the flat gradient arena (etm_allreduce_f32 enqueues on the capturing stream like every other entry; with dp_overlap the
        two slices on the side stream, which joins the capture through the fork event and leaves it through the join event), clip +
        AdamW.  Returns the captured graph or None (capture failed: the caller captures graph A / graph B around the host-side
        collective instead)."""
        ga = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(ga, capture_error_mode="thread_local"):
                if overlap:
                    self._tg_stats, dfe = self._train_body_a1(self._tg_idx, clip_range, beta, self._tg_stats3, head=self._tg_tables)
                    self._allreduce_rest_async()
                    self._train_body_a2(dfe)
                    self._allreduce_conv_and_join()
                else:
                    self._tg_stats = self._train_body_a(self._tg_idx, clip_range, beta, self._tg_stats3, head=self._tg_tables)
                    self.dp.all_reduce_grads(average=False)
                self._tg_norms = self._train_body_b(monitor, self._tg_stats if self._tg_tables else None)
            return ga
        except Exception as exc:       # noqa: BLE001
            print(f"[etm] one-graph data-parallel step not captured ({exc!r}); using graph A -> all-reduce -> graph B", file=sys.stderr, flush=True)
            torch.cuda.synchronize(self.device)
            self._dp_one_graph_failed = True
            return None

    def _allreduce_rest_async(self):
        main = torch.cuda.current_stream(self.device)
        self._ar_fork.record(main)
        self._ar_side.wait_event(self._ar_fork)
        self.dp.all_reduce_slice(self._conv_floats, self.flat_grads.numel(), self._ar_side)

    def _allreduce_conv_and_join(self):
        """The convolutions' slice follows on the SAME side stream (one communicator: its collectives stay on one stream, in one
        order on every rank), after the encoder's backward pass; the main stream then waits for both."""
        main = torch.cuda.current_stream(self.device)
        self._ar_fork2.record(main)
        self._ar_side.wait_event(self._ar_fork2)
        self.dp.all_reduce_slice(0, self._conv_floats, self._ar_side)
        self._ar_join.record(self._ar_side)
        if getattr(self, "_ar_probe", None) is not None:       # bench.py: how long the main stream really waits for the side stream
            self._ar_probe[0].record(main)
        main.wait_event(self._ar_join)
        if getattr(self, "_ar_probe", None) is not None:
            self._ar_probe[1].record(main)


class _NativeRolloutDrive:
    def _drive_rollout_native(self, groups, episode_infos):
        """Steps 0 .. S - 1 of a rollout through the kernel library's driver (csrc/rollout_driver.hip): step 0 of every group is
        already enqueued; the workers (processes, environments/shm_env.py) take their actions from the device and publish their
        results in the shared segment; this call blocks until the bookkeeping of the last step is done.  Afterwards: rewards /
        done flags / episode results / memory_index rows are taken over from the segment and the driver's event list."""
        import ctypes
        buf, W, S = self.buffer, self.num_workers, self.config["worker_steps"]
        env, lib = self._shm_env, etm_lib.load()
        G = len(groups)
        arr = (etm_lib.RolloutGroup * G)()
        row_bytes = groups[0].row_bytes
        for gi, g in enumerate(groups):
            a = arr[gi]
            a.graph_exec = g.graph_exec
            a.stream = g.stream.cuda_stream
            first = gi * env.procs_per_group
            a.ready = env.v["ready"][first:].ctypes.data
            a.n_procs, a.ready_stride = env.procs_per_group, env.v["ready"].shape[1]
            a.lo, a.hi = g.lo, g.hi
            a.obs_src, a.stage_dst = g.rows_src, g.stage0      # the group's pinned rows and its rows of staging row 0
            a.ss_dst = g.ss_pin.data_ptr()
        if getattr(self, "_drive_events", None) is None:
            self._drive_events = np.zeros((W * S, 3), dtype=np.int64)
            self._drive_counters = np.zeros(2, dtype=np.int64)          # [next slot, number of events]
            self._drive_timing = np.zeros(2, dtype=np.float64)
        ctr = self._drive_counters
        ctr[0], ctr[1] = buf.num_episodes, 0
        chain = None
        if self._chain_log is not None:
            chain = np.zeros((S, 4), dtype=np.float64)
        abort = env.v["err"]          # the workers' error words (one cache line apart) ...
        # (groups are served ready-first: as soon as a group's worker processes have published the step; slot numbers stay in
        # (step, group) order -- csrc/rollout_driver.hip)
        rc = lib.etm_rollout_drive(ctypes.cast(arr, ctypes.c_void_p), G, 0, S, W, row_bytes, W * row_bytes,
                                   env.v["dones"].ctypes.data, self._ss_pin[0].data_ptr(), self._ss_pin[1].data_ptr(),
                                   ctr.ctypes.data, int(buf.bank.shape[0]), self._drive_events.ctypes.data, self._drive_events.shape[0],
                                   ctr[1:].ctypes.data, abort.ctypes.data, abort.shape[0], abort.shape[1],
                                   float(self.config.get("rollout_step_timeout_s", 30.0)), self._drive_timing.ctypes.data,
                                   chain.ctypes.data if chain is not None else None)
        env.park()
        if rc != 0:
            env._check()
            etm_lib.check(rc, "etm_rollout_drive")
        buf.num_episodes = int(ctr[0])
        buf.rewards[:, :] = env.v["rewards"].T
        buf.dones[:, :] = env.v["dones"].T.astype(bool)
        for t, w, slot in self._drive_events[: int(ctr[1])]:
            episode_infos.append(env.info_at(int(t), int(w)))
            if t < S - 1:
                buf.memory_index_host[w, t + 1:] = slot
        if chain is not None:
            self._chain_log.extend(tuple(r) for r in chain[: S - 1])
        return 0.0, float(self._drive_timing[0]), float(self._drive_timing[1])      # seconds in (env.step, waiting, upload + launch)


class _RunOutputs:
    def _write_training_summary(self, update, training_stats, episode_result, value_mean, advantage_mean, steps_per_s) -> None:
        if episode_result:
            for key in episode_result:
                if "std" not in key:
                    self.writer.add_scalar("episode/" + key, episode_result[key], update)
        self.writer.add_scalar("losses/loss", training_stats[2], update)
        self.writer.add_scalar("losses/policy_loss", training_stats[0], update)
        self.writer.add_scalar("losses/value_loss", training_stats[1], update)
        self.writer.add_scalar("losses/entropy", training_stats[3], update)
        self.writer.add_scalar("training/value_mean", value_mean, update)
        self.writer.add_scalar("training/advantage_mean", advantage_mean, update)
        # upstream swaps these two tags (trainer.py:343-344 vs :322-323); written correctly here
        self.writer.add_scalar("other/kl", training_stats[4], update)
        self.writer.add_scalar("other/clip_fraction", training_stats[5], update)
        self.writer.add_scalar("other/env_steps_per_second", steps_per_s, update)
        if self.last_kl_stop is not None:                # (target_kl: did the update stop, and how many optimiser steps it applied)
            self.writer.add_scalar("other/kl_stopped", float(self.last_kl_stop["stopped"]), update)
            self.writer.add_scalar("other/optimizer_steps", self.last_kl_stop["steps_applied"], update)
        if self.last_adaptive_lr is not None:            # (adaptive_lr: the rate the update ended with, and how often it moved)
            self.writer.add_scalar("other/learning_rate", self.last_adaptive_lr["lr"], update)
            self.writer.add_scalar("other/lr_raised", self.last_adaptive_lr["raised"], update)
            self.writer.add_scalar("other/lr_lowered", self.last_adaptive_lr["lowered"], update)
        if self.last_kl_penalty is not None:             # (kl_penalty: the coefficient the update's steps used)
            self.writer.add_scalar("other/kl_coef", self.last_kl_penalty["coef"], update)
        if self.last_obs_reconstruction is not None:     # (obs_reconstruction: the mean of the steps' loss, and the coefficient they used)
            self.writer.add_scalar("losses/obs_reconstruction", self.last_obs_reconstruction["loss"], update)
            self.writer.add_scalar("other/obs_reconstruction_coef", self.last_obs_reconstruction["coef"], update)
        if self.last_valid_action_share is not None:     # (action_masks: mean share of allowed actions in the rollout's words)
            self.writer.add_scalar("other/valid_action_share", self.last_valid_action_share, update)
        if self.last_attention_statistics is not None:   # (attention_statistics: per block and head, where the update's attention landed)
            st = self.last_attention_statistics
            for b, h in np.ndindex(st["rows"].shape):
                for key in ("normalised_entropy", "mean_age", "max_prob"):
                    self.writer.add_scalar(f"attention/b{b}h{h}_{key}", float(st[key][b, h]), update)
        if self.buffer.return_norm is not None:          # (the scale the last rollout's rewards were multiplied with)
            self.writer.add_scalar("training/return_scale", float(self.buffer.return_scale.item()), update)
        if self.model.obs_norm is not None:              # (the spread of the frozen table the next rollout runs on)
            lo, hi = torch.aminmax(self.model.obs_norm_rstd)
            self.writer.add_scalar("training/obs_norm_rstd_min", float(lo.item()), update)
            self.writer.add_scalar("training/obs_norm_rstd_max", float(hi.item()), update)

    def _write_evaluation_summary(self, update, evaluation) -> None:
        """``evaluation/<key>`` scalars of one periodic evaluation (PPOTrainer.evaluate's dict) and one printed line."""
        result = evaluation["result"]
        for key in result:
            if "std" not in key:
                self.writer.add_scalar("evaluation/" + key, result[key], update)
        self.writer.add_scalar("evaluation/env_steps_per_second", evaluation["steps"] / max(evaluation["seconds"], 1e-9), update)
        if self._is_main:
            line = "{:4} evaluation episodes={}".format(update, len(evaluation["episodes"]))
            if "reward_mean" in result and "length_mean" in result:
                line += " reward={:.2f} std={:.2f} length={:.1f}".format(result["reward_mean"], result["reward_std"], result["length_mean"])
            if "success_percent" in result:
                line += " success={:.2f}".format(result["success_percent"])
            print(line + " steps={} seconds={:.3f}".format(evaluation["steps"], evaluation["seconds"]))

    def _write_gradient_summary(self, update, grad_info):
        for key, value in grad_info.items():
            self.writer.add_scalar("gradients/" + key, np.mean(value), update)

    def _save_model(self) -> None:
        """``pickle((state_dict, config))`` to ./models/<run_id>.nn -- upstream's checkpoint format (trainer.py:356-362)."""
        os.makedirs("./models", exist_ok=True)
        state = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        path = "./models/" + self.run_id + ".nn"
        with open(path + ".tmp", "wb") as f:
            pickle.dump((state, self.config), f)
        os.replace(path + ".tmp", path)                # never a torn file at the final path
        print("Model saved to " + "./models/" + self.run_id + ".nn")

    def _build_grad_groups(self):
        """Group-membership matrix so all monitored gradient norms come from one pass over per-parameter norms."""
        groups = self.model._grad_groups()
        index = {id(p): i for i, p in enumerate(self.params)}
        self._grad_keys = list(groups.keys())
        member = torch.zeros((len(groups), len(self.params)), dtype=torch.float32)
        for g, modules in enumerate(groups.values()):
            for m in modules:
                for p in m.parameters():
                    member[g, index[id(p)]] += 1.0   # upstream concatenates, so a parameter listed twice counts twice
        self._grad_member = member.to(self.device)
        # segments of the flat gradient arena (<= 4096 floats, inside one tensor) for etm_group_norms
        base = self.flat_grads.data_ptr()
        starts, lens, owner = [], [], []
        for i, p in enumerate(self.params):
            off = (self._grad_views[i].data_ptr() - base) // 4
            for s in range(0, p.numel(), 4096):
                starts.append(off + s)
                lens.append(min(4096, p.numel() - s))
                owner.append(i)
        self._seg_start = torch.tensor(starts, dtype=torch.int64, device=self.device)
        self._seg_len = torch.tensor(lens, dtype=torch.int32, device=self.device)
        self._seg_member = member[:, owner].contiguous().to(self.device)
        self._seg_partial = torch.empty(len(starts), dtype=torch.float32, device=self.device)

    def _grad_group_norms(self, step=None):
        """The monitored norms.  ``step`` = (statistics, statistics table, norm table, counter) of the table-driven step: the same two
        launches also file the statistics and the norms under row ``counter`` of the tables and advance the counter."""
        arena = self.flat_grads.is_cuda and all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(self.params[:2], self._grad_views[:2]))
        if step is not None:
            if not arena:
                raise RuntimeError("the table-driven step needs the gradients in the flat arena")
            stats, stats_tab, norm_tab, counter = step
            out = torch.empty(len(self._grad_keys), dtype=torch.float32, device=self.device)
            etm_lib.check(etm_lib.load().etm_group_norms_step(self.flat_grads.data_ptr(), self._seg_start.data_ptr(), self._seg_len.data_ptr(),
                                                              self._seg_start.numel(), self._seg_member.data_ptr(), len(self._grad_keys),
                                                              self._seg_partial.data_ptr(), out.data_ptr(), norm_tab.data_ptr(), stats.data_ptr(),
                                                              stats.numel(), stats_tab.data_ptr(), stats_tab.shape[0], counter.data_ptr(),
                                                              torch.cuda.current_stream(self.device).cuda_stream), "etm_group_norms_step")
            return out
        if arena:
            out = torch.empty(len(self._grad_keys), dtype=torch.float32, device=self.device)
            etm_lib.check(etm_lib.load().etm_group_norms(self.flat_grads.data_ptr(), self._seg_start.data_ptr(), self._seg_len.data_ptr(),
                                                         self._seg_start.numel(), self._seg_member.data_ptr(), len(self._grad_keys),
                                                         self._seg_partial.data_ptr(), out.data_ptr(),
                                                         torch.cuda.current_stream(self.device).cuda_stream), "etm_group_norms")
            return out
        sq = torch.stack(torch._foreach_norm([p.grad for p in self.params])) ** 2
        return torch.sqrt(self._grad_member @ sq)

    # ------------------------------------------------------------------ logging / checkpoint


class _CheckpointResume:
    """Checkpoint and resume of training (absent upstream): ``save_checkpoint`` / ``state_digest`` / ``load_checkpoint`` /
    ``restart_episodes`` and the pieces ``PPOTrainer(..., resume=path)`` runs.  The file format and the host-side checks live in
    checkpoint.py; nothing here allocates or launches until one of these methods is called."""

    ARENAS = ("params", "exp_avg", "exp_avg_sq")

    def _arenas(self):
        opt = self.optimizer
        return {"params": opt.flat_params, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}

    def _arena_digests(self):
        """{arena: the four words of etm_arena_digest as python ints}: three pairs of launches and one copy of 3 x 32 bytes."""
        if getattr(self, "_digest_out", None) is None:
            self._digest_out = torch.zeros((3, 4), dtype=torch.int64, device=self.device)
            self._digest_partial = ops.arena_digest_workspace(self.device)
        arenas = self._arenas()
        for i, name in enumerate(self.ARENAS):
            ops.arena_digest(arenas[name], out=self._digest_out[i], partial=self._digest_partial)
        words = self._digest_out.cpu().numpy().view(np.uint64)
        return {name: tuple(int(w) for w in words[i]) for i, name in enumerate(self.ARENAS)}

    def state_digest(self) -> dict:
        """{"params", "exp_avg", "exp_avg_sq": (fingerprint, number of Inf / NaN words, largest finite |x|), "step": the optimiser's
        step count} -- the public way to compare the training state of two runs: equal fingerprints = the same bits at the same
        places (etm_arena_digest; 32 bytes per arena travel to the host)."""
        out = {name: (w[0], w[1], float(np.array([w[2]], dtype=np.uint32).view(np.float32)[0])) for name, w in self._arena_digests().items()}
        out["step"] = int(self.optimizer.step_dev.item())
        return out

    def _arena_layout(self):
        return [(name, [int(d) for d in p.shape]) for name, p in self.model.arena_parameters()]

    def _state_buffers(self):
        """The model's persistent buffers by name (the ``obs_norm_*`` triple and table, when present): state outside the arena."""
        params = {n for n, _ in self.model.named_parameters()}
        keep = set(self.model.state_dict().keys()) - params
        return {n: b for n, b in self.model.named_buffers() if n in keep}

    def _fixed_addresses(self) -> dict:
        """data_ptr() of everything a load writes into and a captured graph may hold."""
        opt, buf = self.optimizer, self.buffer
        out = {"flat_params": opt.flat_params.data_ptr(), "flat_grads": opt.flat_grads.data_ptr(), "exp_avg": opt.exp_avg.data_ptr(),
               "exp_avg_sq": opt.exp_avg_sq.data_ptr(), "step_dev": opt.step_dev.data_ptr(), "lr_dev": opt.lr_dev.data_ptr()}
        if self._kl_coef is not None:
            out["kl_coef"] = self._kl_coef.data_ptr()
        if self._recon_coef is not None:
            out["obs_reconstruction_coef"] = self._recon_coef.data_ptr()
        out.update({"param:" + n: p.data_ptr() for n, p in self.model.named_parameters()})
        out.update({"buffer:" + n: b.data_ptr() for n, b in self.model.named_buffers()})
        if buf.ret_stats is not None:
            out.update(ret_stats=buf.ret_stats.data_ptr(), ret_carry=buf.ret_carry.data_ptr())
        return out

    def save_checkpoint(self, path=None) -> str:
        """Writes ./models/<run_id>.nn (the model file of ``_save_model``, unchanged: evaluate.py, enjoy.py and upstream's loader read
        it) and the training checkpoint ``path`` (default ./models/<run_id>.ckpt; -> the path), which holds what continues the run:
        completed updates and ``segment``; the config; the arena layout [(parameter name, shape)]; the flat parameter arena; the
        optimiser state (FlatAdamW.state_dict: both moments, step, lr, hyper-parameters); the model's buffers outside the arena (the
        ``obs_norm_*`` triple and table); ``buffer.ret_stats``; torch's CPU and device generator states; the last <= 100 episode
        infos; the digests of the three arenas; with ``kl_penalty`` one more entry, ``kl_coef``, the float32 coefficient of the next
        update (absent without the key).
        Before anything is written etm_arena_digest runs over the three arenas: a non-finite value in any of them raises
        FloatingPointError (arena, count, update) and leaves both files of the previous save as they are.
        Episodes in flight are NOT saved (environment state in general cannot be): a resumed run starts every worker on a fresh
        episode; statistics keep the steps already merged."""
        digests = self._arena_digests()
        for name in self.ARENAS:
            if digests[name][1] > 0:
                raise FloatingPointError(f"save_checkpoint: {digests[name][1]} non-finite value(s) in the {name} arena after update "
                                         f"{self.update_index}: nothing written, the previous checkpoint files stay as they are")
        import checkpoint as ck
        self._save_model()
        path = "./models/" + self.run_id + ".ckpt" if path is None else str(path)
        buf = self.buffer
        torch.cuda.synchronize(self.device)
        state = {
            "update": int(self.update_index), "segment": int(self.segment), "config": self.config, "layout": self._arena_layout(),
            "params": self.optimizer.flat_params.cpu().numpy(), "optimizer": self.optimizer.state_dict(),
            "buffers": {n: b.detach().cpu().numpy() for n, b in self._state_buffers().items()},
            "ret_stats": buf.ret_stats.cpu().numpy() if buf.ret_stats is not None else None,
            "rng_cpu": torch.get_rng_state().numpy().copy(), "rng_device": torch.cuda.get_rng_state(self.device).numpy().copy(),
            "episode_infos": list(self._episode_infos), "digests": {n: [int(w) for w in digests[n]] for n in self.ARENAS},
        }
        if self._kl_coef is not None:       # (kl_penalty: the coefficient is trainer state; no entry without the key)
            state["kl_coef"] = np.float32(self._kl_coef.item())
        ck.write_checkpoint(path, state)
        print("Checkpoint saved to " + path)
        return path

    @staticmethod
    def _read_verified(path) -> dict:
        """The checkpoint at ``path`` with every arena checked against its stored digest on the host (checkpoint.digest_numpy)."""
        import checkpoint as ck
        state = ck.read_checkpoint(path)
        arenas = {"params": state["params"], "exp_avg": state["optimizer"]["exp_avg"], "exp_avg_sq": state["optimizer"]["exp_avg_sq"]}
        for name, a in arenas.items():
            got, want = ck.digest_numpy(a), tuple(int(w) for w in state["digests"][name])
            if got != want:
                raise ValueError(f"{path}: the {name} arena does not match its stored digest (file {got}, stored {want}): the file is damaged")
        return state

    def load_checkpoint(self, path) -> None:
        """Continues from the training checkpoint ``path`` IN PLACE, on this live trainer: the file is read and every arena verified
        against its digest on the host before a byte of the trainer is touched; a different arena layout, or a difference in whether
        ``normalize_observations`` / ``normalize_rewards`` are set, is refused (any other differing config key is printed on one line;
        the current config wins); everything is copied into place at fixed addresses (asserted), the device digest must equal the
        stored one; then the update index and the generator states are set and ``restart_episodes(segment + 1)`` runs.
        Nothing derived from the weights survives stale, because nothing is rebound and every derived copy is rebuilt from the
        fixed-address arena before it is read: the rollout weight repackings (``model.refresh_rollout_weights``) and the K | V cache
        (``_refresh_kv_cache``) at the start of every rollout -- eagerly or as ``ReplayAfterWarmup`` graphs, whose frozen pointer
        tables stay valid exactly because no parameter moves --, the evaluator's parameter and table copies before every evaluation,
        the bank-with-positions and the training observations at the start of every optimisation phase.
        ``worker_processes: true``: refused (live worker processes cannot be restarted on fresh environments): build a new trainer
        with ``resume=path``."""
        if self._shm_env is not None:
            raise ValueError("load_checkpoint on a live trainer with worker_processes: true: the worker processes' environments cannot "
                             "be restarted in place; build the trainer with PPOTrainer(..., resume=path) (train.py --resume PATH)")
        import checkpoint as ck
        ck.check_checkpoint_config(self.config, self._world, resume=True)
        self._load_state(self._read_verified(path), str(path), restart=True)

    def _load_state(self, state, what, restart):
        import checkpoint as ck
        from utils import normalization_section
        if [(e[0], tuple(e[1])) for e in state["layout"]] != [(n, tuple(s)) for n, s in self._arena_layout()]:
            saved, mine = {e[0]: list(e[1]) for e in state["layout"]}, dict(self._arena_layout())
            diff = sorted(set(saved) ^ set(mine)) + [n for n in saved if n in mine and saved[n] != mine[n]]
            raise ValueError(f"{what}: the parameter arena of the checkpoint is laid out differently (parameters that differ: "
                             f"{diff[:8] or 'their order'})")
        for key in ("normalize_observations", "normalize_rewards"):
            if (normalization_section(state["config"], key) is None) != (normalization_section(self.config, key) is None):
                raise ValueError(f"{what}: {key} is {'set' if normalization_section(state['config'], key) is not None else 'not set'} in the "
                                 "checkpoint and the opposite in this run: the running statistics cannot be continued")
        buffers, buf, opt = self._state_buffers(), self.buffer, self.optimizer
        if set(buffers) != set(state["buffers"]) or (buf.ret_stats is None) != (state["ret_stats"] is None):
            raise ValueError(f"{what}: the state outside the arena differs (checkpoint {sorted(state['buffers'])}, this run {sorted(buffers)})")
        diff = ck.config_differences(state["config"], self.config)
        if diff:
            print(f"[etm] resume: config keys that differ from the checkpoint (the current config wins): {', '.join(diff)}", flush=True)
        before = self._fixed_addresses()
        with torch.no_grad():
            opt.flat_params.copy_(torch.from_numpy(np.ascontiguousarray(state["params"])))
            opt.load_state_dict(state["optimizer"])
            for name, b in buffers.items():
                b.copy_(torch.from_numpy(np.ascontiguousarray(state["buffers"][name])))
            if buf.ret_stats is not None:
                buf.ret_stats.copy_(torch.from_numpy(np.ascontiguousarray(state["ret_stats"])))
            if self._kl_coef is not None:
                # kl_penalty: the current config wins (as for adaptive_lr) -- a fixed coefficient is the config's, an adaptive one
                # continues from the checkpoint's; a checkpoint without the entry starts at the config's coef
                start = self._kl_pen["coef"]
                if self._kl_pen["adaptive"] and state.get("kl_coef") is not None:
                    start = float(np.float32(state["kl_coef"]))
                self._kl_coef.fill_(start)
                self.last_kl_penalty = None
        after = self._fixed_addresses()
        assert after == before, "a load moved " + ", ".join(k for k in before if before[k] != after.get(k))
        digests = self._arena_digests()
        for name in self.ARENAS:
            if digests[name] != tuple(int(w) for w in state["digests"][name]):
                raise RuntimeError(f"{what}: the {name} arena on the device does not match the checkpoint's digest after the upload "
                                   f"(device {digests[name]}, stored {tuple(state['digests'][name])})")
        self.update_index = int(state["update"])
        self._episode_infos.clear()
        self._episode_infos.extend(state["episode_infos"])
        torch.set_rng_state(torch.from_numpy(np.ascontiguousarray(state["rng_cpu"])))
        torch.cuda.set_rng_state(torch.from_numpy(np.ascontiguousarray(state["rng_device"])), self.device)
        if restart:
            self.restart_episodes(int(state["segment"]) + 1)

    def restart_episodes(self, segment: int) -> None:
        """Every worker at step 0 of an empty episode on fresh environments of training segment ``segment``: worker ids from
        ``checkpoint.segment_first_worker_id`` on, the running return of every worker (``ret_carry``) zero, pending truncation records
        dropped.  An environment supplied through ``env=`` gets ``env.restart(first_worker_id)`` if it has that method, else only
        ``env.reset``.  Episodes in flight are dropped -- a documented deviation of resumed runs."""
        import checkpoint as ck
        if self._shm_env is not None:
            raise ValueError("restart_episodes with worker_processes: true: live worker processes cannot be restarted on fresh "
                             "environments; build the trainer with PPOTrainer(..., resume=path)")
        self._restart_workers(ck.segment_first_worker_id(self._base_worker_id, segment))
        self.segment = int(segment)

    def _restart_workers(self, first_worker_id: int) -> None:
        """Fresh environments from ``first_worker_id`` on, every worker at step 0 of an empty episode in slot w."""
        from environments.vec_env import make_vec_env
        W, buf = self.num_workers, self.buffer
        torch.cuda.synchronize(self.device)
        if self._env_supplied:
            if hasattr(self.env, "restart"):
                self.env.restart(int(first_worker_id))
        else:
            self.env.close()
            self.env = make_vec_env(self._env_cfg, W, int(first_worker_id), groups=self._env_groups)
            parts = getattr(self.env, "parts", None)
            self._group_all.env = self.env
            if parts is not None and len(parts) == len(self._groups) > 1:
                for g, part in zip(self._groups, parts):
                    g.env = part
        ev = getattr(buf, "_host_arrays_uploaded", None)
        if ev is not None:
            ev.synchronize()
        buf.bank[: buf.num_episodes].zero_()
        buf.num_episodes = W
        if buf.ret_carry is not None:
            buf.ret_carry.zero_()
        if buf.prev_actions is not None:      # previous_step_input: every worker starts an episode, nothing is carried over
            buf.prev_live.zero_()
        self._truncations = []
        self.worker_current_episode_step[:] = 0
        self.worker_episode_slot[:] = range(W)
        self._ss_dev.copy_(self._ss_pin)
        self.env.reset(out=self.obs)
        if self._masked:
            self._take_action_masks(self.env, 0, W, "reset")
