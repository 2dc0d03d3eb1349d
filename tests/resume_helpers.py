"""Shared by tests/test_resume_gpu.py: the tiny trainer of tests/test_normalization_gpu.py (W = 4, S = 16, memory length 4, one block,
D = 64, a synthetic environment with a vector observation and ``pool: 4``) with both normalisation keys on and a DECAYING learning
rate, one training update driven the way ``run_training`` drives it, and a recording of everything a resumed run must reproduce."""
import gc

import numpy as np
import torch

W_T, S_T, F_OBS = 4, 16, 5


def dev():
    return torch.device("cuda", 0)


def config(**over):
    cfg = dict(environment=dict(type="Synthetic", obs_shape=[F_OBS], num_actions=3, max_episode_steps=16, seed=2, p_done=0.1, pool=4),
               gamma=0.99, lamda=0.95, updates=4, epochs=2, n_workers=W_T, worker_steps=S_T, n_mini_batch=2,
               value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False,
               normalize_observations={"clip": 5.0}, normalize_rewards=True,
               transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=1e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-4, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.05, power=1.0, max_decay_steps=10))
    cfg.update(over)
    return cfg


def modes(graph):
    return dict(hip_graph_rollout=bool(graph), hip_graph_train=bool(graph))


def trainer(cfg, seed=11, run_id="resume", **kw):
    from trainer import PPOTrainer
    torch.manual_seed(seed)
    return PPOTrainer(cfg, run_id=run_id, device=dev(), tensorboard=False, **kw)


def release(*trainers):
    for tr in trainers:
        if tr is not None:
            tr.close()
    del trainers
    gc.collect()
    torch.cuda.synchronize()


def update(tr, **kw):
    """Update number ``tr.update_index`` as ``run_training`` runs it (the trainer's own draws and permutations unless ``kw`` says
    otherwise: uniforms=, perms=) -> ``record(tr)``."""
    lr, beta, clip = tr.schedules(tr.update_index)
    tr._sample_training_data(uniforms=kw.get("uniforms"))
    tr.buffer.prepare_batch_dict()
    tr._train_epochs(lr, clip, beta, perms=kw.get("perms"))
    tr.update_index += 1
    torch.cuda.synchronize()
    return record(tr)


def state(tr):
    """Everything a checkpoint carries that lives on the device, as host arrays."""
    opt, buf = tr.optimizer, tr.buffer
    out = {"param:" + n: p.detach().cpu().numpy().copy() for n, p in tr.model.named_parameters()}
    out.update(arena=opt.flat_params.cpu().numpy(), exp_avg=opt.exp_avg.cpu().numpy(), exp_avg_sq=opt.exp_avg_sq.cpu().numpy(),
               step=np.asarray(opt.step_dev.item()), lr=opt.lr_dev.cpu().numpy())
    for name in ("obs_norm_stats", "obs_norm_mean", "obs_norm_rstd"):
        if hasattr(tr.model, name):
            out[name] = getattr(tr.model, name).cpu().numpy()
    if buf.ret_stats is not None:
        out["ret_stats"] = buf.ret_stats.cpu().numpy()
    return out


def record(tr):
    buf = tr.buffer
    out = state(tr)
    out.update(values=buf.values.cpu().numpy(), log_probs=buf.log_probs.cpu().numpy(), actions=buf.actions.cpu().numpy(),
               advantages=buf.advantages.cpu().numpy(), obs=buf.obs.cpu().numpy())
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def differing(a, b):
    """The keys at which two recordings differ in a bit (or in dtype / shape)."""
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    return [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or not np.array_equal(bits(a[k]), bits(b[k]))]


def largest_relative_parameter_difference(a, b):
    """max over parameter tensors of max|a - b| / max|a| (two recordings)."""
    worst = 0.0
    for k in a:
        if k.startswith("param:"):
            worst = max(worst, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max() / max(np.abs(a[k]).max(), 1e-30)))
    return worst
