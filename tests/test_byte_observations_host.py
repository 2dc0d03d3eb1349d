"""uint8 image observations, host side (no device): the value a byte stands for, the synthetic byte / float twins, the refusals, and
the model's CPU path.

A byte k stands for ``np.float32(k) / np.float32(255)`` -- what an image wrapper that divides on the host computes.  The anchor is that
one line of numpy; everything else here is compared against it bit for bit.
"""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

QUOTIENT = np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the value of a byte
def test_value_table_is_the_float32_quotient_and_not_a_product():
    from environments.synthetic import BYTE_UNIT
    from etm import ops
    for table in (ops.byte_unit_table(), BYTE_UNIT):
        assert table.dtype == np.float32 and table.shape == (256,)
        assert np.array_equal(_bits(table), _bits(QUOTIENT))
    assert np.array_equal(_bits(np.float32(np.arange(256, dtype=np.float64) / 255)), _bits(QUOTIENT))
    product = np.arange(256, dtype=np.float32) * np.float32(1 / 255)
    assert not np.array_equal(_bits(product), _bits(QUOTIENT))           # a later "optimisation" to a multiply trips this
    assert int((product != QUOTIENT).sum()) == 126


def _rn32(x):
    """Fraction -> the nearest float32 (ties to even), exactly."""
    if x == 0:
        return Fraction(0)
    e = 0
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    while Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    n = x / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl * ulp


def test_kernel_arithmetic_gives_the_quotient_for_every_byte():
    """A proof of the derivation, not a test of the code: the arithmetic etm_byte_unit (csrc/etm_common.h) is written to perform --
    q = k y, r = fma(-255, q, k), result = fma(r, y, q) with y = float32(1 / 255) -- restated here in exact rational arithmetic with one
    rounding per operation gives the quotient for all 256 bytes.  It does not touch the C++ helper and would not notice a change to
    it; what guards the helper are the device tests (tests/test_byte_observations_gpu.py: test_bytes_to_unit_exact,
    test_device_unit_is_not_a_multiply)."""
    y = Fraction(float(np.float32(1) / np.float32(255)))
    for k in range(256):
        q = _rn32(k * y)
        r = k - 255 * q
        assert r == 0 or (r > 0 and _rn32(r) == r) or (r < 0 and _rn32(-r) == -r), k      # the residual is exact in float32
        got = _rn32(q + r * y)
        assert got == Fraction(float(QUOTIENT[k])), k


# ------------------------------------------------------------------ synthetic twins
SHAPE = (3, 12, 12)
BASE = dict(obs_shape=SHAPE, num_actions=3, max_episode_steps=4, seed=5, p_done=0.2)


def _vec_run(pool, steps=10, **keys):
    from environments.synthetic import SyntheticVecEnv
    env = SyntheticVecEnv(3, pool=pool, gen_threads=2, copy_threads=2, **BASE, **keys)
    obs = [env.reset().copy()]
    rest = []
    for _ in range(steps):
        o, r, d, info = env.step(np.zeros(3, dtype=np.int64))
        obs.append(o.copy())
        rest.append((r.copy(), d.copy(), list(info)))
    env.close()
    return env, np.stack(obs), rest


def _single_run(pool, worker, steps=10, **keys):
    from environments.synthetic import SyntheticEnv
    env = SyntheticEnv(pool=pool, worker_id=worker, **BASE, **keys)
    obs, rest = [np.array(env.reset())], []
    for _ in range(steps):
        o, r, d, info = env.step(0)
        rest.append((r, d, info))
        obs.append(np.array(env.reset()) if d else np.array(o))
    return env, np.stack(obs), rest


@pytest.mark.parametrize("pool", (4, 0), ids=("ring", "fresh"))
def test_synthetic_byte_and_float_forms_are_twins(pool):
    plain_env, plain, plain_rest = _vec_run(pool)
    lev_env, lev, lev_rest = _vec_run(pool, observation_levels=256)
    byte_env, byt, byte_rest = _vec_run(pool, observation_levels=256, observation_dtype="uint8")
    assert byt.dtype == np.uint8 and lev.dtype == np.float32 and plain.dtype == np.float32
    assert byte_env.observation_dtype == np.uint8 and lev_env.observation_dtype == np.float32 and plain_env.observation_dtype == np.float32
    assert np.array_equal(_bits(QUOTIENT[byt]), _bits(lev))                            # the twins
    assert np.array_equal(byt, np.floor(plain.astype(np.float64) * 256).astype(np.uint8))      # both derive from the plain draws
    assert any(d.any() for _, d, _ in plain_rest), "no episode ended inside the run"
    for a, b, c in zip(plain_rest, lev_rest, byte_rest):                                # reward / done / info streams untouched
        for other in (b, c):
            assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2] == other[2]
    # the plain config's observations are what they were: the generator's own float32 draws
    for w in range(3):
        rng = np.random.default_rng(BASE["seed"] + w)
        if pool:
            ring = rng.random((pool,) + SHAPE, dtype=np.float32)
            want = np.stack([ring[t % pool] for t in range(plain.shape[0])])
        else:
            want = np.stack([rng.random(SHAPE, dtype=np.float32) for _ in range(plain.shape[0])])
        assert np.array_equal(_bits(plain[:, w]), _bits(want)), w
    # the single-environment form (reference env API) emits the same rows
    for w in range(3):
        e, o, rest = _single_run(pool, w, observation_levels=256, observation_dtype="uint8")
        assert e.observation_space.dtype == np.uint8 and o.dtype == np.uint8
        assert np.array_equal(o, byt[:, w]), w
        assert [bool(d) for _, d, _ in rest] == [bool(x[1][w]) for x in byte_rest]
        e, o, _ = _single_run(pool, w, observation_levels=256)
        assert e.observation_space.dtype == np.float32 and np.array_equal(_bits(o), _bits(lev[:, w])), w


def test_front_end_options_do_not_change_the_bytes():
    from environments.synthetic import SyntheticVecEnv
    from environments.vec_env import make_vec_env
    for pool in (4, 0):
        runs = []
        for threads in (1, 3):
            env = SyntheticVecEnv(4, pool=pool, gen_threads=threads, copy_threads=threads, observation_levels=256, observation_dtype="uint8", **BASE)
            out = np.zeros((4,) + SHAPE, dtype=np.uint8)
            rows = []
            env.reset(out=out)
            frames = [out.copy()]
            for _ in range(3):
                env.step(np.zeros(4, dtype=np.int64), out=out, on_rows=lambda a, b: rows.append((a, b)))
                frames.append(out.copy())
            runs.append(np.stack(frames))
            assert rows and rows[-1][1] == 4
            env.close()
        assert np.array_equal(runs[0], runs[1])
        cfg = dict(type="Synthetic", pool=pool, observation_levels=256, observation_dtype="uint8", **BASE)
        comp = make_vec_env(cfg, 4, groups=2)
        assert comp.observation_dtype == np.uint8
        got = comp.reset()
        assert got.dtype == np.uint8 and np.array_equal(got, runs[0][0])
        comp.close()


# ------------------------------------------------------------------ refusals
def test_validation_of_the_two_keys():
    from environments.synthetic import SyntheticEnv, SyntheticVecEnv
    for make in (lambda **kw: SyntheticEnv(pool=2, **BASE, **kw), lambda **kw: SyntheticVecEnv(2, pool=2, **BASE, **kw)):
        with pytest.raises(ValueError):
            make(observation_dtype="uint8")                                    # bytes without the levels
        for bad in (128, 255, 0, "256", True):
            with pytest.raises(ValueError):
                make(observation_levels=bad)
        for bad in ("int8", "uint16", "float64", "bytes", 8):
            with pytest.raises(ValueError):
                make(observation_levels=256, observation_dtype=bad)
        make(observation_levels=256, observation_dtype="uint8").close()


def test_uint8_vector_observations_are_refused():
    from model import ActorCriticModel
    cfg = dict(hidden_layer_size=64, transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=4, positional_encoding="",
                                                      layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    m = ActorCriticModel(cfg, SimpleNamespace(shape=(6,)), (3,), 8)
    with pytest.raises(ValueError):
        m._encode(torch.zeros((2, 6), dtype=torch.uint8))


def test_worker_processes_with_bytes_is_refused_before_anything_is_built(monkeypatch):
    import trainer
    from environments import shm_env, synthetic
    built = []

    def recording(name, real):
        def factory(*a, **kw):
            built.append(name)
            return real(*a, **kw)
        return factory

    monkeypatch.setattr(shm_env, "ShmVecEnv", recording("ShmVecEnv", shm_env.ShmVecEnv))
    monkeypatch.setattr(shm_env, "_probe_env", recording("_probe_env", shm_env._probe_env))
    monkeypatch.setattr(trainer, "make_vec_env", recording("make_vec_env", trainer.make_vec_env))
    monkeypatch.setattr(synthetic, "SyntheticEnv", recording("SyntheticEnv", synthetic.SyntheticEnv))
    monkeypatch.setattr(synthetic, "SyntheticVecEnv", recording("SyntheticVecEnv", synthetic.SyntheticVecEnv))
    cfg = dict(environment=dict(type="Synthetic", pool=2, observation_levels=256, observation_dtype="uint8", **BASE),
               worker_processes=True, n_workers=4, worker_steps=8, n_mini_batch=2, epochs=1, updates=1, gamma=0.99, lamda=0.95,
               value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5,
               transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=4, positional_encoding="", layer_norm="post",
                                gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    with pytest.raises(ValueError, match="worker_processes"):
        trainer.PPOTrainer(cfg, run_id="refused", device=torch.device("cuda", 0), tensorboard=False)
    assert built == []
    # the float twin of the same config is not refused by this check
    trainer.check_byte_observation_transport(dict(cfg, environment=dict(cfg["environment"], observation_dtype="float32")))
    trainer.check_byte_observation_transport(dict(cfg, worker_processes=False))


# ------------------------------------------------------------------ the model on the CPU
def test_cpu_model_on_bytes_equals_its_float_twin():
    from model import ActorCriticModel
    cfg = dict(hidden_layer_size=64, transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=4, positional_encoding="",
                                                      layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    torch.manual_seed(0)
    m = ActorCriticModel(cfg, SimpleNamespace(shape=(3, 84, 84)), (3,), 8)
    g = torch.Generator().manual_seed(1)
    xb = torch.randint(0, 256, (4, 3, 84, 84), generator=g, dtype=torch.int64).to(torch.uint8)
    xb[0].view(-1)[:256] = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    xb[1], xb[2] = 0, 255
    xf = torch.from_numpy(QUOTIENT[xb.numpy()])
    assert torch.equal(xb.to(torch.float32) / 255, xf)                     # torch's CPU division is the quotient too
    hb, hf = m._encode(xb), m._encode(xf)          # (the encoder: the part of the model that has a CPU path in this build)
    assert hb.dtype == torch.float32 and torch.equal(hb, hf)
    (hb.sum()).backward()                          # gradients reach the convolutions through the byte input's conversion
    assert m.conv1.weight.grad is not None and torch.isfinite(m.conv1.weight.grad).all()
