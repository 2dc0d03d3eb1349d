"""uint8 image observations on the device: every result computed from bytes is BIT-IDENTICAL to what the float path of the same build
computes from ``k.astype(np.float32) / np.float32(255)`` (the arithmetic of an image wrapper that divides on the host).

Covered: the expand kernel (``ops.bytes_to_unit``), the rollout encoder's first layer on bytes (``ops.conv_relu``,
``model._encode_fused``), the training encoder on the bf16 matrix pipe (``ops.encoder_train``: features, ReLU pattern words, the six
gradients; plain, indexed, through ``DeferredDw``), the fallback (expand + float kernels) for everything that has no byte kernel, two
trainers that differ in the observation dtype alone, and a checkpoint of a byte run played by enjoy.py.

The inputs of every kernel case hold all 256 byte values, one all-0 and one all-255 image.  Comparisons are ``torch.equal``.
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TABLE = np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda", 0)


def _unit(t):
    """The float twin of a byte tensor, formed on the HOST with numpy's division (the reference arithmetic)."""
    return torch.from_numpy(TABLE[t.cpu().numpy()]).to(t.device)


def _byte_images(n, shape, seed):
    """n >= 1 images of ``shape`` (any layout): random bytes; all 256 values occur; with n >= 3 image 1 is all 0 and image 2 all 255."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n,) + tuple(shape), generator=g, dtype=torch.int64).to(torch.uint8)
    if n >= 3:
        x[1] = 0
        x[2] = 255
    flat = x[0].reshape(-1)
    assert flat.numel() >= 256
    flat[:256] = torch.arange(256, dtype=torch.int64).to(torch.uint8)[torch.randperm(256, generator=g)]
    assert len(torch.unique(x)) == 256
    return x


def _extreme_batches(n, shape):
    """Batches of n < 3 images (too few for ``_byte_images`` to hold them) that bring the all-0 and the all-255 image to a small-N case:
    one batch of [all-0, all-255] for n = 2, one batch each for n = 1."""
    zero, full = torch.zeros((1,) + tuple(shape), dtype=torch.uint8), torch.full((1,) + tuple(shape), 255, dtype=torch.uint8)
    return [zero, full] if n == 1 else [torch.cat((zero, full))]


class _Calls:
    """Counts the calls of the library's byte entry points (patched on the loaded library object; restored on exit)."""
    NAMES = ("etm_bytes_to_unit", "etm_conv_relu_u8", "etm_conv_b3_fwd_u8", "etm_conv_b3_wgrad_u8")

    def __enter__(self):
        from etm import lib
        self.lib = lib.load()
        self.orig = {n: getattr(self.lib, n) for n in self.NAMES}
        self.count = {n: 0 for n in self.NAMES}
        for n in self.NAMES:
            setattr(self.lib, n, self._wrap(n))
        return self

    def _wrap(self, name):
        def call(*a):
            self.count[name] += 1
            return self.orig[name](*a)
        return call

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.lib, n, self.orig[n])


# ------------------------------------------------------------------ the expand kernel
@pytest.mark.parametrize("row_bytes", (1, 15, 16, 17, 4099))
@pytest.mark.parametrize("offset", (0, 1, 3))
def test_bytes_to_unit_exact(row_bytes, offset):
    from etm import ops
    dev = _dev()
    rows = max(7, -(-600 // row_bytes))                     # at least 600 bytes: all 256 values, several blocks at 4,099
    g = torch.Generator().manual_seed(row_bytes * 7 + offset)
    flat = torch.randint(0, 256, (rows * row_bytes,), generator=g, dtype=torch.int64).to(torch.uint8)
    flat[:256] = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    flat.view(rows, row_bytes)[-2] = 0                      # an all-0 and an all-255 row (behind the 256 values: rows * row_bytes >= 600)
    flat.view(rows, row_bytes)[-1] = 255
    alloc = torch.zeros(rows * row_bytes + 8, dtype=torch.uint8, device=dev)
    src = alloc[offset:offset + rows * row_bytes].view(rows, row_bytes)      # a view that starts `offset` bytes off its allocation
    src.copy_(flat.view(rows, row_bytes))
    assert src.data_ptr() % 4 == offset % 4
    want = torch.from_numpy(TABLE[flat.view(rows, row_bytes).numpy()])
    got = ops.bytes_to_unit(src)
    assert got.dtype == torch.float32 and got.shape == (rows, row_bytes)
    assert torch.equal(got.cpu(), want)
    index = torch.cat((torch.arange(rows - 1, -1, -1), torch.tensor([0, 0, rows - 1, 2, 2])))      # reversed, then repeats
    got = ops.bytes_to_unit(src, index=index.to(dev))
    assert torch.equal(got.cpu(), want[index])


def test_device_unit_is_not_a_multiply():
    """The device values are the quotients, which k * fp32(1 / 255) misses for 126 of the 256 bytes."""
    from etm import ops
    got = ops.bytes_to_unit(torch.arange(256, dtype=torch.int64).to(torch.uint8).to(_dev()).view(1, 256)).cpu().numpy()[0]
    assert np.array_equal(got.view(np.uint32), TABLE.view(np.uint32))
    prod = np.arange(256, dtype=np.float32) * np.float32(1 / 255)
    assert int((prod != got).sum()) == 126


# ------------------------------------------------------------------ rollout layer 1
def _rollout_model(shape, seed=0):
    from model import ActorCriticModel
    cfg = dict(hidden_layer_size=128, transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=8,
                                                       positional_encoding="", layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    torch.manual_seed(seed)
    m = ActorCriticModel(cfg, SimpleNamespace(shape=shape), (3,), 8).to(_dev())
    with torch.no_grad():
        for conv in (m.conv1, m.conv2, m.conv3):
            conv.bias.uniform_(-0.1, 0.1)
    m.refresh_rollout_weights()
    return m


@pytest.mark.parametrize("shape,n", (((3, 84, 84), 1), ((3, 84, 84), 8), ((3, 84, 84), 33), ((3, 36, 36), 8), ((1, 84, 84), 8)),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rollout_layer1_bytes_equal_floats(shape, n):
    from etm import ops
    m = _rollout_model(shape)
    c, h, w = shape
    xb = _byte_images(n, shape, seed=n + h).to(_dev())
    xf = _unit(xb)
    with torch.no_grad(), _Calls() as calls:
        got = ops.conv_relu(xb, m._w1p, m.conv1.bias, c, h, w, 8, 8, 4, False, False)
        assert calls.count["etm_conv_relu_u8"] == 1 and calls.count["etm_bytes_to_unit"] == 0
        want = ops.conv_relu(xf, m._w1p, m.conv1.bias, c, h, w, 8, 8, 4, False, False)
        assert torch.equal(got, want)
        assert m._fused_encoder_ok(xb)
        assert torch.equal(m._encode_fused(xb), m._encode_fused(xf))
        assert torch.equal(m._encode(xb), m._encode(xf))
        for xe in (_extreme_batches(n, shape) if n < 3 else ()):      # (n >= 3: images 1 and 2 of xb are the all-0 and the all-255 image)
            xe = xe.to(_dev())
            assert torch.equal(ops.conv_relu(xe, m._w1p, m.conv1.bias, c, h, w, 8, 8, 4, False, False),
                               ops.conv_relu(_unit(xe), m._w1p, m.conv1.bias, c, h, w, 8, 8, 4, False, False))
            assert torch.equal(m._encode_fused(xe), m._encode_fused(_unit(xe)))


def test_rollout_layer1_bytes_stacked_index_and_rows():
    from etm import ops
    m = _rollout_model((3, 84, 84))
    n, lo, hi = 11, 2, 9
    xb = _byte_images(3 * n, (3, 84, 84), seed=5).view(3, n, 3, 84, 84).to(_dev())
    xf = _unit(xb)
    with torch.no_grad():
        for i in (0, 1, 2):
            index = torch.tensor(i, dtype=torch.int64, device=_dev())
            for rows in (None, (lo, hi)):
                got = ops.conv_relu(xb, m._w1p, m.conv1.bias, 3, 84, 84, 8, 8, 4, False, False, index=index, rows=rows)
                want = ops.conv_relu(xf, m._w1p, m.conv1.bias, 3, 84, 84, 8, 8, 4, False, False, index=index, rows=rows)
                plain = ops.conv_relu(xf[i] if rows is None else xf[i, lo:hi].contiguous(), m._w1p, m.conv1.bias, 3, 84, 84, 8, 8, 4, False, False)
                assert got.shape[0] == (n if rows is None else hi - lo)
                assert torch.equal(got, want) and torch.equal(got, plain), (i, rows)
                assert torch.equal(m._encode(xb, index, rows), m._encode(xf, index, rows)), (i, rows)


def test_rollout_layer1_misaligned_bytes_take_the_fallback():
    """A byte input that does not start on a 4-byte boundary has no byte kernel: expanded, then the float kernel; equal all the same."""
    from etm import ops
    m = _rollout_model((3, 84, 84))
    n, lo, hi = 6, 1, 5
    data = _byte_images(2 * n, (3, 84, 84), seed=8)
    alloc = torch.zeros(data.numel() + 8, dtype=torch.uint8, device=_dev())
    xb = alloc[1:1 + data.numel()].view(2, n, 3, 84, 84)
    xb.copy_(data.view(2, n, 3, 84, 84))
    assert xb.data_ptr() % 4 == 1
    xf = _unit(xb)
    index = torch.tensor(1, dtype=torch.int64, device=_dev())
    with torch.no_grad(), _Calls() as calls:
        for kw in (dict(), dict(index=index), dict(index=index, rows=(lo, hi))):
            src_b, src_f = (xb, xf) if kw else (xb[0], xf[0])
            got = ops.conv_relu(src_b, m._w1p, m.conv1.bias, 3, 84, 84, 8, 8, 4, False, False, **kw)
            want = ops.conv_relu(src_f, m._w1p, m.conv1.bias, 3, 84, 84, 8, 8, 4, False, False, **kw)
            assert torch.equal(got, want), kw
    assert calls.count["etm_bytes_to_unit"] == 3 and calls.count["etm_conv_relu_u8"] == 0


# ------------------------------------------------------------------ training encoder
def _convs(c, seed):
    torch.manual_seed(seed)
    convs = [torch.nn.Conv2d(c, 32, 8, 4), torch.nn.Conv2d(32, 64, 4, 2), torch.nn.Conv2d(64, 64, 3, 1)]
    return [cv.to(_dev()) for cv in convs]


def _patterns(feats):
    """The ReLU pattern tensors the forward pass saved for backward (int32 words; bf16x3 products only)."""
    return [t for t in feats.grad_fn.saved_tensors if t is not None and t.dtype == torch.int32]


def _train_twins(shape, n, products, indexed, deferred):
    """encoder_train on bytes and on their float twin: features, ReLU patterns, the six gradients -> equal.  Every case sees the all-0
    and the all-255 image: in its batch where N allows, else in further calls of the same N (``_extreme_batches``; indexed: further
    index vectors that select images 1 and 2 of the bank).  -> (pattern tensors per call, calls made on bytes)."""
    from etm import ops
    c, h, w = shape
    dev = _dev()
    convs = _convs(c, seed=n)
    params = [t for cv in convs for t in (cv.weight, cv.bias)]
    extra = []
    if indexed:
        bank = _byte_images(300, (h, w, c), seed=n + 1).to(dev)
        g = torch.Generator().manual_seed(n)
        idx = torch.randint(0, 300, (n,), generator=g)
        idx = torch.sort(idx, descending=True).values
        if n >= 2:
            idx[1] = idx[0]                                  # a repeated entry
        if n >= 7:
            idx[3:6] = torch.tensor([1, 2, 2])               # the all-0 and the all-255 image, the latter twice
        else:
            for pick in ((1,), (2,)) if n == 1 else ((2, 1),):
                e = idx.clone()
                e[: len(pick)] = torch.tensor(pick)
                extra.append((bank, e.to(dev)))
        index = idx.to(dev)
        xb = bank
    else:
        xb, index = _byte_images(n, (h, w, c), seed=n + 1).to(dev), None
        if n < 3:
            extra = [(xe.to(dev), None) for xe in _extreme_batches(n, (h, w, c))]
    patterns = 0
    for xb, index in [(xb, index)] + extra:
        patterns = _train_pair(ops, convs, params, xb, index, products, deferred)
    return patterns, 1 + len(extra)


def _train_pair(ops, convs, params, xb, index, products, deferred):
    dev = _dev()
    xf = _unit(xb)
    f0 = ops.encoder_train(xf, *convs, index=index, products=products)
    gout = torch.randn(f0.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    out = {}
    for name, x in (("float", xf), ("byte", xb)):
        feats = ops.encoder_train(x, *convs, index=index, products=products)
        pats = [p.clone() for p in _patterns(feats)]
        if deferred:
            views = [torch.full_like(t, float("nan")) for t in params]
            with ops.DeferredDw({t.data_ptr(): v for t, v in zip(params, views)}) as col:
                (feats * gout).sum().backward()
            assert col.written == {t.data_ptr() for t in params} and all(t.grad is None for t in params)
            grads = views
        else:
            grads = torch.autograd.grad(feats, params, gout)
        out[name] = (feats.detach(), pats, grads)
    (ff, pf, gf), (fb, pb, gb) = out["float"], out["byte"]
    assert torch.equal(fb, ff), "features"
    assert len(pb) == len(pf) and all(torch.equal(a, b) for a, b in zip(pb, pf)), "ReLU patterns"
    assert all(torch.isfinite(g).all() for g in gb)
    assert all(torch.equal(a, b) for a, b in zip(gb, gf)), "gradients"
    return len(pb)


@pytest.mark.parametrize("deferred", (False, True), ids=("autograd", "deferred_dw"))
@pytest.mark.parametrize("indexed", (False, True), ids=("plain", "indexed"))
@pytest.mark.parametrize("n", (1, 2, 7, 129))
def test_training_encoder_bytes_equal_floats(n, indexed, deferred):
    with _Calls() as calls:
        patterns, runs = _train_twins((3, 84, 84), n, "bf16x3", indexed, deferred)
    assert patterns == 3
    assert calls.count["etm_conv_b3_fwd_u8"] == runs and calls.count["etm_conv_b3_wgrad_u8"] == runs
    assert calls.count["etm_bytes_to_unit"] == 0


@pytest.mark.parametrize("shape,n,products", (((3, 84, 84), 7, "fp32"), ((3, 44, 60), 5, None), ((4, 84, 84), 3, None)),
                         ids=("3x84x84_fp32", "3x44x60", "4x84x84"))
@pytest.mark.parametrize("indexed", (False, True), ids=("plain", "indexed"))
def test_fallback_expands_then_runs_the_float_kernels(shape, n, products, indexed):
    with _Calls() as calls:
        _, runs = _train_twins(shape, n, products, indexed, False)
    assert calls.count["etm_bytes_to_unit"] == 2 * runs      # every byte run's forward and its backward
    assert calls.count["etm_conv_b3_fwd_u8"] == 0 and calls.count["etm_conv_b3_wgrad_u8"] == 0 and calls.count["etm_conv_relu_u8"] == 0


def test_model_paths_take_bytes():
    """forward_banked on bytes (training encoder, library convolutions, indexed minibatch) equals the float twin; a byte vector is
    refused.  The library-convolution branch holds the ONE comparison of this file that is not bitwise: the library picks its
    algorithm per call, so two calls on identical floats need not agree in the last bits.  What is asserted bitwise there is what the
    byte path is answerable for -- the tensor handed to conv1 (values, dtype, strides), caught by a forward pre-hook; the outputs are
    then only held to a tolerance."""
    from model import ActorCriticModel, IndexedObservations
    from etm.ops import WindowSpec
    dev = _dev()
    cfg = dict(hidden_layer_size=64, transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=4,
                                                      positional_encoding="", layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    torch.manual_seed(1)
    m = ActorCriticModel(cfg, SimpleNamespace(shape=(3, 84, 84)), (3,), 8).to(dev)
    n = 5
    xb = _byte_images(n, (84, 84, 3), seed=9).to(dev)         # NHWC memory, as the trainer keeps it
    xf = _unit(xb)
    idx = torch.tensor([4, 1, 1, 2, 0], device=dev)
    mem = torch.randn((n, 4, 1, 64), device=dev)
    mask = torch.ones((n, 4), dtype=torch.bool, device=dev)
    midx = torch.arange(4, device=dev).repeat(n, 1)
    seen = []
    hook = m.conv1.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    for train_encoder in (True, False):
        m.train_encoder = train_encoder
        for make in (lambda x: x.permute(0, 3, 1, 2), lambda x: IndexedObservations(x, idx)):
            outs = []
            del seen[:]
            for x in (xf, xb):
                pi, v, items = m.forward_banked(make(x), WindowSpec.from_windows(mem, midx, mask))
                outs.append((pi[0].logits, v, items))
            if train_encoder:
                assert not seen and all(torch.equal(a, b) for a, b in zip(*outs))
            else:
                # the library convolutions choose their algorithm per call, so two calls on the same floats need not agree bit for
                # bit; what the byte path owes them is the same input: the same values in the same memory order
                assert len(seen) == 2 and seen[1].dtype == torch.float32 and torch.equal(seen[0], seen[1])
                assert seen[0].stride() == seen[1].stride()
                assert all(torch.allclose(a, b, rtol=1e-4, atol=1e-5) for a, b in zip(*outs))
    hook.remove()
    mv = ActorCriticModel(cfg, SimpleNamespace(shape=(6,)), (3,), 8).to(dev)
    with pytest.raises(ValueError):
        mv._encode(torch.zeros((2, 6), dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------ two trainers that differ in the observation dtype alone
def _release(tr):
    import gc
    tr.close()
    del tr
    gc.collect()
    torch.cuda.synchronize()


def _trainer_config(byte, graph, direct, pool, groups, gated):
    """The smallest model shape tests/test_rollout_step_vs_float64.py drives through the fused step kernel (team1_h1: D 128, one head,
    L 32, two blocks; gated: g4_64, the group kernel's smallest shape) on 3 x 84 x 84 observations, 16 workers."""
    L = 32
    env = dict(type="Synthetic", obs_shape=[3, 84, 84], num_actions=4, max_episode_steps=L + 5, seed=3, p_done=0.5 / L, pool=pool,
               gen_threads=2, copy_threads=2, observation_levels=256)
    if byte:
        env["observation_dtype"] = "uint8"
    return dict(environment=env, gamma=0.99, lamda=0.95, updates=2, epochs=1, n_workers=16, worker_steps=L + 12, n_mini_batch=2,
                value_loss_coefficient=0.5, hidden_layer_size=128, max_grad_norm=0.5, rollout_groups=groups, rollout_min_group_size=2,
                hip_graph_rollout=graph, hip_graph_train=graph, direct_observation_rows=direct, tunable_gemm=False,
                transformer=dict(num_blocks=2, embed_dim=128, num_heads=1, memory_length=L, positional_encoding="" if gated else "relative",
                                 layer_norm="pre" if gated else "post", gtrxl=gated, gtrxl_bias=0.0),
                learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
                beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
                clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))


def _run_trainer(cfg, updates=2):
    """-> (per update: the buffer's tensors, the used bank slots, every parameter), the observation dtype, the plan's text."""
    from trainer import PPOTrainer
    torch.manual_seed(11)
    tr = PPOTrainer(cfg, run_id="bytes_twin", device=_dev(), tensorboard=False)
    snaps = []
    try:
        for _ in range(updates):
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            stats, _ = tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            assert np.isfinite(np.asarray(stats)).all()
            b = tr.buffer
            snap = {k: getattr(b, k).clone() for k in ("actions", "log_probs", "values", "advantages", "memory_mask", "memory_indices", "obs")}
            snap["bank"] = b.bank[: b.num_episodes].clone()
            snap["params"] = [p.detach().clone() for p in tr.params]
            snaps.append(snap)
        dtypes = dict(buffer=tr.buffer.obs.dtype, pin=tr._obs_pin.dtype, dev=tr._obs_dev.dtype, stage=tr._stage["obs"].dtype, lv=tr._lv.obs.dtype,
                      nhwc=None if tr._obs_train is None else tr._obs_train.dtype, groups=[g.obs_dev.dtype for g in tr._groups],
                      row_bytes=tr._groups[0].row_bytes, group_kernel=[g.group_kernel for g in tr._groups])
        return snaps, dtypes, repr(tr._plan)
    finally:
        _release(tr)


# (id, graphs, direct_observation_rows, pool, rollout_groups, gated): graphs x direct rows x pool x groups, and the gated pre-LN layout
TWIN_CASES = tuple((f"{'graph' if gr else 'eager'}_{'direct' if di else 'upload'}_{'ring' if pool else 'fresh'}_{groups}group", gr, di, pool, groups, False)
                   for gr in (True, False) for di in (True, False) for pool in (4, 0) for groups in (2, 1))
TWIN_CASES += (("graph_direct_ring_2group_gated_preln", True, True, 4, 2, True),)


@pytest.mark.parametrize("case", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_trainer_on_bytes_equals_its_float_twin(case):
    _, graph, direct, pool, groups, gated = case
    with _Calls() as calls:
        byte, bt, bplan = _run_trainer(_trainer_config(True, graph, direct, pool, groups, gated))
    # the byte run's rollout and update reached the byte kernels, never the expansion (captured steps count once, at their capture)
    assert calls.count["etm_conv_relu_u8"] > 0 and calls.count["etm_conv_b3_fwd_u8"] > 0 and calls.count["etm_conv_b3_wgrad_u8"] > 0, calls.count
    assert calls.count["etm_bytes_to_unit"] == 0, calls.count
    with _Calls() as calls:
        flt, ft, fplan = _run_trainer(_trainer_config(False, graph, direct, pool, groups, gated))
    assert not any(calls.count.values()), calls.count
    print(f"[{case[0]}] byte run: {bplan}; float run: {fplan}; group kernel: {bt['group_kernel']}")
    assert bplan == fplan
    assert all(bt[k] == torch.uint8 for k in ("buffer", "pin", "dev", "stage", "lv", "nhwc")) and all(d == torch.uint8 for d in bt["groups"])
    assert all(ft[k] == torch.float32 for k in ("buffer", "pin", "dev", "stage", "lv", "nhwc"))
    assert bt["row_bytes"] == 3 * 84 * 84 and ft["row_bytes"] == 4 * 3 * 84 * 84
    assert len(bt["groups"]) == groups
    if gated:
        assert all(bt["group_kernel"]), "the gated layout did not run the group form of the step kernel"
    for u, (a, b) in enumerate(zip(byte, flt)):
        assert a["obs"].dtype == torch.uint8 and torch.equal(_unit(a["obs"]), b["obs"]), (u, "observations")
        for k in ("actions", "log_probs", "values", "advantages", "memory_mask", "memory_indices", "bank"):
            assert torch.equal(a[k], b[k]), (u, k)
        assert all(torch.equal(p, q) for p, q in zip(a["params"], b["params"])), (u, "parameters")
    assert not torch.equal(byte[0]["params"][0], byte[1]["params"][0])      # (the updates moved the first convolution)


def test_byte_checkpoint_runs_one_episode(tmp_path):
    """A checkpoint written by a byte-observation run is loaded as enjoy.py loads it and plays one episode on byte frames."""
    import pickle
    import enjoy
    from environments import action_space_kind
    from model import ActorCriticModel
    from trainer import PPOTrainer
    from utils import create_env
    dev = _dev()
    cfg = _trainer_config(True, False, False, 4, 1, False)
    cfg.update(n_workers=4, worker_steps=8, updates=1)
    torch.manual_seed(2)
    tr = PPOTrainer(cfg, run_id="bytes_ckpt", device=dev, tensorboard=False)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        tr._train_epochs(3e-4, 0.1, 1e-3)
        tr._save_model()
        keys = list(tr.model.state_dict().keys())
    finally:
        os.chdir(cwd)
        _release(tr)
    with open(tmp_path / "models" / "bytes_ckpt.nn", "rb") as f:
        state_dict, config = pickle.load(f)
    assert list(state_dict.keys()) == keys and all(v.dtype != torch.uint8 for v in state_dict.values())
    env = create_env(config["environment"])
    assert env.observation_space.dtype == np.uint8
    kind = action_space_kind(env.action_space)
    model = ActorCriticModel(config, env.observation_space, kind.shape, env.max_episode_steps)
    model.load_state_dict(state_dict)
    model.to(dev).eval()
    frames = []
    reset0, step0 = env.reset, env.step
    env.reset = lambda **kw: (frames.append(reset0(**kw)), frames[-1])[1]

    def spy(a):
        out = step0(a)
        frames.append(out[0])
        return out

    env.step = spy
    with torch.no_grad():
        rewards, info = enjoy.run_episode(model, env, config, dev)
    assert 0 < len(rewards) <= env.max_episode_steps and info is not None
    assert all(f.dtype == np.uint8 for f in frames)
    env.close()
