"""The trainer on CommandRoom: the device-resident front-end (``device: true``) against the host twin (``device: false``, serial), bit
for bit -- the rollout's buffer, the episode infos, the rows after the last step, the parameters after two updates, and an
evaluation -- in the captured plan that streams observations (where the fast path must really be taken), on the protocol path, with
two worker groups, with action masks and with the previous step as input."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, S, EPOCHS, N_MB = 4, 8, 2, 2
FORMS = {
    "captured": {},
    "protocol": {"hip_graph_rollout": False},
    "two groups": {"rollout_groups": 2, "rollout_min_group_size": 2},
    "action masks": {"action_masks": True},
    "previous step": {"previous_step_input": True},
}


def _config(device, **over):
    env = dict(type="CommandRoom", grid=3, cell=12, command_count=2, show_steps=1, gap_steps=0, seed=5, device=bool(device),
               vectorize="serial")
    sched = dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10)
    cfg = dict(environment=env, gamma=0.99, lamda=0.95, updates=2, epochs=EPOCHS, n_workers=W, worker_steps=S, n_mini_batch=N_MB,
               value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False, rollout_groups=1,
               transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(sched), beta_schedule=dict(sched, initial=1e-3, final=1e-3),
               clip_range_schedule=dict(sched, initial=0.1, final=0.1))
    cfg.update(over)
    return cfg


def _trainer(cfg):
    from trainer import PPOTrainer
    torch.manual_seed(11)
    return PPOTrainer(cfg, run_id="command_room", device=torch.device("cuda", 0), tensorboard=False)


def _release(*trainers):
    for tr in trainers:
        tr.close()
    del trainers
    gc.collect()
    torch.cuda.synchronize()


def _front_ends(tr):
    return list(getattr(tr.env, "parts", None) or [tr.env])


def _eq(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


FIELDS = ("obs", "actions", "log_probs", "values", "rewards", "dones", "memory_index", "advantages")


def _field(buf, name):
    # (the host array is what the rollout writes; the device field is uploaded from it when the batch is prepared)
    return buf.memory_index_host if name == "memory_index" else getattr(buf, name)


@pytest.mark.parametrize("form", list(FORMS))
def test_device_front_end_trains_bit_for_bit_like_the_host_twin(form):
    from environments.device_env import CommandRoomDeviceVecEnv
    from environments.vec_env import SerialVecEnv
    dev, host = _trainer(_config(True, **FORMS[form])), _trainer(_config(False, **FORMS[form]))
    try:
        assert all(isinstance(e, CommandRoomDeviceVecEnv) for e in _front_ends(dev))
        assert all(isinstance(e, SerialVecEnv) for e in _front_ends(host))
        assert len(_front_ends(dev)) == len(_front_ends(host)) == (2 if form == "two groups" else 1)
        assert dev.observation_dtype == torch.uint8 and _eq(dev.obs, host.obs)
        rng = np.random.default_rng(3)
        for update in range(2):
            uniforms = rng.random((W, S), dtype=np.float32)
            perms = [np.random.default_rng(40 + 10 * update + e).permutation(W * S) for e in range(EPOCHS)]
            infos = []
            for tr in (dev, host):
                lr, beta, clip = tr.schedules(update)
                infos.append(tr._sample_training_data(uniforms=uniforms))
                torch.cuda.synchronize()
            for name in FIELDS:
                assert _eq(_field(dev.buffer, name), _field(host.buffer, name)), f"update {update}: buffer.{name} differs"
            assert infos[0] == infos[1], f"update {update}: the finished episodes' infos differ"
            assert _eq(dev.obs, host.obs), "the rows after the last step (the bootstrap observation) differ"
            if form == "action masks":
                assert _eq(dev.buffer.action_masks_host, host.buffer.action_masks_host)
                assert dev.last_valid_action_share == host.last_valid_action_share < 1.0
            # which path stepped the environments: in a plan that streams observations every step but the rollout's last one is
            # the kernel writing into the staging row; else the protocol path alone
            fast = sum(e.device_steps for e in _front_ends(dev))
            slow = sum(e.protocol_steps for e in _front_ends(dev))
            n = len(_front_ends(dev))
            if form == "protocol":
                assert dev._plan is None and (fast, slow) == (0, (update + 1) * S)
            else:
                assert dev._plan is not None and dev._plan.stream_obs and host._plan == dev._plan
                assert (fast, slow) == ((update + 1) * (S - 1) * n, (update + 1) * n), "the fast path was not taken"
            for tr in (dev, host):
                tr.buffer.prepare_batch_dict()
                tr._train_epochs(lr, clip, beta, perms=perms)
                tr.update_index += 1
            torch.cuda.synchronize()
            assert _eq(dev.optimizer.flat_params, host.optimizer.flat_params), f"update {update}: the parameter arenas differ"
        assert len(infos[0]) >= W and all(set(i) == {"reward", "length", "success"} for i in infos[0])
    finally:
        _release(dev, host)


def test_evaluation_on_the_device_config_returns_the_host_twins_result():
    dev, host = _trainer(_config(True)), _trainer(_config(False))
    try:
        a = dev.evaluate(episodes_per_worker=2, n_workers=4, deterministic=True, seed=700, worker_steps=8)
        b = host.evaluate(episodes_per_worker=2, n_workers=4, deterministic=True, seed=700, worker_steps=8)
        assert a["episodes"] == b["episodes"] and a["result"] == b["result"] and a["steps"] == b["steps"]
        assert len(a["episodes"]) == 8
        a = dev.evaluate(episodes_per_worker=1, n_workers=4, deterministic=False, seed=701, worker_steps=8)
        b = host.evaluate(episodes_per_worker=1, n_workers=4, deterministic=False, seed=701, worker_steps=8)
        assert a["episodes"] == b["episodes"] and a["result"] == b["result"]
    finally:
        _release(dev, host)


@pytest.mark.parametrize("over, match", [
    (dict(worker_processes=True), "worker_processes: false"),
    (dict(bootstrap_truncated=True), "bootstrap_truncated"),
    (dict(transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=5, positional_encoding="relative", layer_norm="post",
                           gtrxl=False, gtrxl_bias=0.0)), "memory_length"),
])
def test_refused_at_construction(over, match):
    with pytest.raises(ValueError, match=match):
        _trainer(_config(True, **over))


def test_worker_processes_are_refused_for_the_host_twin_too():
    # the shared segment's rows are float32 and the type has no float form: the refusal CueRoom gets
    with pytest.raises(ValueError, match="uint8"):
        _trainer(_config(False, worker_processes=True))


def test_refused_in_a_data_parallel_run():
    class _Dp:
        world, rank = 2, 0
    from trainer import PPOTrainer
    with pytest.raises(ValueError, match="data-parallel"):
        PPOTrainer(_config(True), run_id="command_room_dp", device=torch.device("cuda", 0), tensorboard=False, dp=_Dp())
