"""Observation reconstruction (``obs_reconstruction``) on the host: the rule's gradient against central differences of its loss, the
plain-numpy last layer against torch's transposed convolution, both tails of the logit, the byte targets, the key's parser and every
refusal, the decoder's place in the state dict, the CPU expression of the op against the rule, the config and the ABI.  No GPU.

The central differences: f = the mean loss over M elements is evaluated in float64 at z_k +- h, h = 1e-4.  The error of
(f(z + h) - f(z - h)) / 2h against f'(z) is at most  h^2 / 6 * max |f'''|  +  (rounding of one f) / h.
  f'' = s (1 - s) / M and f''' = s (1 - s)(1 - 2 s) / M with s = sigma(z_k): |f'''| <= 1 / (6 sqrt 3) / M for every s in [0, 1].
  One f is the sum of M terms l_j = max(z, 0) - z t + log1p(exp(-|z|)), each a handful of operations on parts of size max(z, 0), |z| t
  and log1p(.) (<= 16 eps of their sum S_j), added pairwise by numpy (<= (ceil(log2 M) + 1) eps of sum_j S_j) and divided once:
  rounding <= (16 + ceil(log2 M) + 2) eps sum_j S_j / M.
Both are computed from the inputs alone; nothing is tuned to the result."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "episodic-transformer-memory-ppo_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from utils import (obs_reconstruction_coef, obs_reconstruction_loss, obs_reconstruction_maps_back, obs_reconstruction_section,  # noqa: E402
                   obs_reconstruction_sizes, obs_reconstruction_target, transposed_conv_last)

H = 1.0e-4
EPS64 = float(np.finfo(np.float64).eps)
M3 = 1.0 / (6.0 * math.sqrt(3.0))


def _case(seed=0, shape=(2, 8, 8, 3)):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=shape) * 2.0
    t = rng.random(shape)
    t.reshape(-1)[:4] = (0.0, 1.0, 0.0, 1.0)          # the ends of the target range, at logits of either sign
    z.reshape(-1)[:4] = (3.0, 3.0, -3.0, -3.0)
    return z, t


def test_gradient_against_central_differences():
    z, t = _case()
    M = z.size
    loss, grad = obs_reconstruction_loss(z, t, np.float64)
    assert grad.shape == z.shape and grad.dtype == np.float64 and isinstance(loss, np.float64)
    S = (np.maximum(z, 0) + np.abs(z) * t + np.log1p(np.exp(-np.abs(z)))).sum()
    rounding = (16 + math.ceil(math.log2(M)) + 2) * EPS64 * S / M
    bound = M3 / M * H * H / 6.0 + rounding / H
    flat, worst = z.reshape(-1), 0.0
    for k in range(M):
        keep = flat[k]
        flat[k] = keep + H
        up = obs_reconstruction_loss(z, t, np.float64)[0]
        flat[k] = keep - H
        dn = obs_reconstruction_loss(z, t, np.float64)[0]
        flat[k] = keep
        err = abs((up - dn) / (2 * H) - grad.reshape(-1)[k])
        worst = max(worst, err)
        assert err <= bound, (k, err, bound)
    print(f"[central differences] M {M}, h {H:g}, bound {bound:.3e}, worst error {worst:.3e}, largest |gradient| {np.abs(grad).max():.3e}")


@pytest.mark.parametrize("shape", [(1, 1, 1, 32, 1), (2, 2, 2, 32, 3), (1, 3, 2, 32, 3), (1, 2, 3, 5, 4)], ids=str)
def test_transposed_conv_last_equals_torch_in_float64(shape):
    import torch
    n, hi, wi, cin, c = shape
    rng = np.random.default_rng(sum(shape))
    a, w, b = rng.normal(size=(n, hi, wi, cin)), rng.normal(size=(cin, c, 8, 8)), rng.normal(size=c)
    got = transposed_conv_last(a, w, b, np.float64)
    assert got.shape == (n, 4 * hi + 4, 4 * wi + 4, c) and got.dtype == np.float64
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(a).permute(0, 3, 1, 2), torch.from_numpy(w), torch.from_numpy(b), stride=4)
    want = want.permute(0, 2, 3, 1).numpy()
    # rounding only: each output is a sum of at most 4 cin products and the bias, in whatever order
    bound = (4 * cin + 2) * EPS64 * transposed_conv_last(np.abs(a), np.abs(w), np.abs(b), np.float64)
    assert np.all(np.abs(got - want) <= bound), float(np.abs(got - want).max())
    # the corner pixel has one input pixel, the centre of a 2 x 2 (and larger) input has four
    assert np.isclose(got[0, 0, 0, 0], a[0, 0, 0] @ w[:, 0, 0, 0] + b[0], rtol=0, atol=float(bound[0, 0, 0, 0]))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_both_tails_are_finite(dt):
    z = np.array([200.0, -200.0, 200.0, -200.0, 0.0, 88.8, -88.8, 1.0e4, -1.0e4], dtype=dt)
    t = np.array([0.0, 0.0, 1.0, 1.0, 0.5, 0.25, 0.75, 1.0, 0.0], dtype=dt)
    with np.errstate(all="raise", under="ignore"):
        loss, grad = obs_reconstruction_loss(z, t, dt)
    assert np.isfinite(loss) and np.all(np.isfinite(grad)) and grad.dtype == dt
    M = z.size
    # sigma(200) = 1, sigma(-200) = 0 to every digit: the gradient is (1 - t) / M and (0 - t) / M, the loss z (1 - t) and -z t
    assert np.allclose(grad[:4] * M, [1.0, 0.0, 0.0, -1.0], rtol=0, atol=1e-30)
    want = (200.0 + 0.0 + 0.0 + 200.0 + math.log(2.0) + 88.8 * 0.75 + 88.8 * 0.75 + 0.0 + 0.0) / M
    assert abs(float(loss) - want) <= 64 * float(np.finfo(dt).eps) * want


def test_byte_targets_are_the_correctly_rounded_quotient():
    got = obs_reconstruction_target(np.arange(256, dtype=np.uint8), np.float32)
    assert got.dtype == np.float32 and got.shape == (256,)
    for k in range(256):
        c, exact = np.float32(got[k]), Fraction(k, 255)
        err = abs(Fraction(float(c)) - exact)
        for other in (np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-1))):
            assert err <= abs(Fraction(float(other)) - exact), k
    # a byte array and its float twin give the same loss and gradient, in float64 and in float32
    rng = np.random.default_rng(3)
    z, byt = rng.normal(size=(2, 8, 8, 3)), rng.integers(0, 256, size=(2, 8, 8, 3), dtype=np.uint8)
    for dt in (np.float64, np.float32):
        a, b = obs_reconstruction_loss(z, byt, dt), obs_reconstruction_loss(z, byt.astype(np.float32) / np.float32(255), dt)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_section_values_and_schedule():
    assert obs_reconstruction_section({}) is None
    sec = obs_reconstruction_section({"obs_reconstruction": 0.1})
    assert sec == dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=0.0)
    assert obs_reconstruction_coef(sec, 0) == obs_reconstruction_coef(sec, 10 ** 6) == float(np.float32(0.1))
    sec = obs_reconstruction_section({"obs_reconstruction": {"initial": 0.1, "final": 0.0, "power": 1.0, "max_decay_steps": 1000}})
    assert sec == dict(initial=0.1, final=0.0, power=1.0, max_decay_steps=1000.0)
    assert obs_reconstruction_coef(sec, 0) == float(np.float32(0.1)) and obs_reconstruction_coef(sec, 500) == float(np.float32(0.05))
    assert obs_reconstruction_coef(sec, 1000) == 0.0 and obs_reconstruction_coef(sec, 1001) == 0.0
    # schedules that are exactly 0 after update 0 (the frozen-decoder test's); a decay of 0 steps is `initial` at update 0, then `final`
    for steps in (1, 0):
        sec = obs_reconstruction_section({"obs_reconstruction": {"initial": 0.5, "final": 0.0, "power": 1.0, "max_decay_steps": steps}})
        assert [obs_reconstruction_coef(sec, u) for u in (0, 1, 2)] == [0.5, 0.0, 0.0]
    assert obs_reconstruction_section({"obs_reconstruction": 0.1}, (3, 84, 84)) is not None
    assert obs_reconstruction_section({"obs_reconstruction": 0.1}, (1, 36, 84)) is not None
    assert obs_reconstruction_maps_back(84) and obs_reconstruction_maps_back(36) and not obs_reconstruction_maps_back(40)
    assert not obs_reconstruction_maps_back(7) and 84 in obs_reconstruction_sizes() and obs_reconstruction_sizes()[0] == 36


FULL = {"initial": 0.1, "final": 0.0, "power": 1.0, "max_decay_steps": 10}


@pytest.mark.parametrize("value,message", [
    (0, r"must be a number > 0 .*or a schedule.*remove the key"),
    (-0.1, r"must be a number > 0"),
    (True, r"must be a number > 0"),
    ("0.1", r"must be a number > 0"),
    (float("nan"), r"must be a number > 0"),
    (float("inf"), r"must be a number > 0"),
    ([0.1], r"must be a number > 0"),
    ({k: v for k, v in FULL.items() if k != "power"}, r"exactly the keys.*missing: \['power'\].*write all four, or a single number"),
    (dict(FULL, coef=1.0), r"exactly the keys.*unknown: \['coef'\]"),
    (dict(FULL, initial=0.0), r"initial must be > 0.*remove the key"),
    (dict(FULL, final=-0.1), r"obs_reconstruction.final must be a finite number >= 0"),
    (dict(FULL, power=float("nan")), r"obs_reconstruction.power must be a finite number >= 0"),
    (dict(FULL, max_decay_steps="10"), r"obs_reconstruction.max_decay_steps must be a finite number >= 0"),
    (dict(FULL, initial=True), r"obs_reconstruction.initial must be a finite number >= 0"),
])
def test_value_refusals(value, message):
    with pytest.raises(ValueError, match=message):
        obs_reconstruction_section({"obs_reconstruction": value})


def test_shape_and_world_refusals():
    with pytest.raises(ValueError, match=r"is for image observations.*observation shape \(4,\).*remove the key"):
        obs_reconstruction_section({"obs_reconstruction": 0.1}, (4,))
    with pytest.raises(ValueError, match=r"does not map a side of 40 pixels back onto itself.*sides that work: \[36, 44, 52.*84.*resize the observation, or remove the key"):
        obs_reconstruction_section({"obs_reconstruction": 0.1}, (3, 84, 40))
    with pytest.raises(ValueError, match=r"at most 4 image channels, got 5"):
        obs_reconstruction_section({"obs_reconstruction": 0.1}, (5, 84, 84))
    with pytest.raises(ValueError, match=r"obs_reconstruction in a data-parallel run.*remove the key, or train on one device"):
        obs_reconstruction_section({"obs_reconstruction": 0.1}, (3, 84, 84), world=2)
    assert obs_reconstruction_section({}, (4,), world=2) is None        # (absent: nothing is looked at)


def _model(key, shape=(3, 36, 36)):
    import torch
    from model import ActorCriticModel
    cfg = dict(hidden_layer_size=32, transformer=dict(num_blocks=1, embed_dim=32, num_heads=2, memory_length=4, positional_encoding="relative",
                                                      layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    if key is not None:
        cfg["obs_reconstruction"] = key
    torch.manual_seed(0)
    return ActorCriticModel(cfg, type("Space", (), {"shape": shape})(), (3,), 8)


NEW_KEYS = [f"{m}.{p}" for m in ("dec_hidden", "dec_conv3", "dec_conv2", "dec_conv1") for p in ("weight", "bias")]


def test_the_decoder_is_the_last_four_modules_of_the_state_dict():
    plain, keyed = _model(None), _model(0.1)
    base, keys = list(plain.state_dict().keys()), list(keyed.state_dict().keys())
    assert not any("dec_" in k for k in base) and plain.recon_cfg is None and "decoder" not in plain._grad_groups()
    assert base[:6] == ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias"] and base[-2:] == ["value.weight", "value.bias"]
    assert keys == base + NEW_KEYS
    assert [n for n, _ in keyed.arena_parameters()] == [n for n, _ in plain.arena_parameters()] + NEW_KEYS
    # every other parameter is the key-absent model's, bit for bit (the decoder draws from the generator after them)
    for k in base:
        assert keyed.state_dict()[k].equal(plain.state_dict()[k]), k
    sd = keyed.state_dict()
    assert tuple(sd["dec_hidden.weight"].shape) == (64, 32) and tuple(sd["dec_conv3.weight"].shape) == (64, 64, 3, 3)
    assert tuple(sd["dec_conv2.weight"].shape) == (64, 32, 4, 4) and tuple(sd["dec_conv1.weight"].shape) == (32, 3, 8, 8)
    assert list(keyed._grad_groups())[-2:] == ["decoder", "model"]
    with pytest.raises(ValueError, match="built without obs_reconstruction"):
        plain.reconstruct(None)
    with pytest.raises(ValueError, match="is for image observations"):
        _model(0.1, shape=(4,))
    with pytest.raises(ValueError, match="does not map a side of 40"):
        _model(0.1, shape=(3, 40, 40))


@pytest.mark.parametrize("byte", [False, True], ids=["float", "uint8"])
def test_the_cpu_expression_of_the_op_is_the_rule(byte):
    import torch
    from etm import ops
    m = _model(0.1).double()
    rng = np.random.default_rng(5)
    h = torch.from_numpy(rng.normal(size=(3, 32)))
    a2 = m.reconstruct(h)
    assert tuple(a2.shape) == (3, 8, 8, 32) and a2.is_contiguous()
    obs = rng.integers(0, 256, size=(5, 36, 36, 3), dtype=np.uint8) if byte else rng.random((5, 36, 36, 3)).astype(np.float32)
    index = np.array([4, 0, 4])
    coef = torch.tensor([0.25], dtype=torch.float64)
    bank = type("Bank", (), {"bank": torch.from_numpy(obs), "index": torch.from_numpy(index)})()
    term, out = ops.obs_reconstruction_loss(a2, m.dec_conv1, bank, coef, with_out=True)
    z = transposed_conv_last(a2.detach().numpy(), m.dec_conv1.weight.detach().numpy(), m.dec_conv1.bias.detach().numpy())
    loss, dz = obs_reconstruction_loss(z, obs[index])
    assert abs(float(out[0]) - loss) <= 64 * EPS64 * loss and abs(float(term.detach()) - 0.25 * loss) <= 64 * EPS64 * loss
    (g,) = torch.autograd.grad(term, m.dec_conv1.bias)
    assert np.allclose(g.numpy(), 0.25 * dz.sum(axis=(0, 1, 2)), rtol=1e-10, atol=1e-14)


def test_the_new_config_is_its_base_plus_the_key():
    from yaml_parser import YamlParser
    cfgs = os.path.join(PKG, "configs")
    b = YamlParser(os.path.join(cfgs, "synthetic_minigrid_u8.yaml")).get_config()
    n = YamlParser(os.path.join(cfgs, "synthetic_minigrid_recon.yaml")).get_config()
    assert obs_reconstruction_section(n, n["environment"]["obs_shape"]) is not None
    assert n.pop("obs_reconstruction") == 0.1
    assert n == b


def test_the_abi_grows_additively_at_version_61():
    from etm import lib
    assert lib.ABI_VERSION == 61
    names = ("etm_obs_recon_supported", "etm_obs_recon_workspace_bytes", "etm_obs_recon_fwd_loss", "etm_obs_recon_dgrad")
    header = open(os.path.join(REPO, "include", "etm_hip.h")).read()
    for name in names:
        assert name in lib.SIGNATURES and f" {name}(" in header, name
    assert "etm_conv_train_wgrad(x := dz" in header, "the weight gradient's identity is stated next to the new entries"
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.etm_abi_version() == 61
        assert handle.etm_obs_recon_supported(3, 20, 20) == 1 and handle.etm_obs_recon_supported(5, 20, 20) == 0
        assert handle.etm_obs_recon_supported(0, 20, 20) == 0 and handle.etm_obs_recon_supported(3, 0, 20) == 0
        assert handle.etm_obs_recon_workspace_bytes(0, 3, 20, 20) == 0 and handle.etm_obs_recon_workspace_bytes(2, 3, 20, 20) == (4 * 8 + 32 * 3 * 64) * 8
