"""CPU-side checks of the running normalisations (``normalize_observations`` / ``normalize_rewards``): the config surface and its
refusals, the state-dict keys, the CPU encoder path bit for bit, the float64 restatement of both rules (the GPU tests compare the
kernels against the same helper, tests/normalization_reference.py), a pickled checkpoint reproducing the table."""
import copy
import os
import pickle
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import normalization_reference as nr

HERE = os.path.dirname(os.path.abspath(__file__))
CFG_DIR = os.path.join(HERE, "..", "episodic-transformer-memory-ppo_amd", "configs")


def _model_cfg(**over):
    cfg = dict(hidden_layer_size=64,
               transformer=dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative",
                                layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    cfg.update(over)
    return cfg


def _model(F=5, **over):
    from model import ActorCriticModel
    return ActorCriticModel(_model_cfg(**over), SimpleNamespace(shape=(F,)), (3,), 16)


# ------------------------------------------------------------------ config surface
def test_sections_parse_with_defaults():
    from trainer import check_normalization_config
    assert check_normalization_config({}) == {"observations": None, "rewards": None}
    assert check_normalization_config({"normalize_observations": False, "normalize_rewards": None}) == {"observations": None, "rewards": None}
    out = check_normalization_config({"normalize_observations": True, "normalize_rewards": {"clip": 5, "epsilon": 1e-4}})
    assert out == {"observations": {"clip": 10.0, "epsilon": 1e-8}, "rewards": {"clip": 5.0, "epsilon": 1e-4}}
    out = check_normalization_config({"normalize_observations": {"clip": 3.0}}, observation_shape=(7,), observation_dtype=torch.float32)
    assert out["observations"] == {"clip": 3.0, "epsilon": 1e-8} and out["rewards"] is None


def test_config_file_sets_both_keys():
    from trainer import check_box_policy, check_normalization_config
    from yaml_parser import YamlParser
    cfg = YamlParser(os.path.join(CFG_DIR, "synthetic_continuous_normalized.yaml")).get_config()
    base = YamlParser(os.path.join(CFG_DIR, "synthetic_cartpole.yaml")).get_config()
    assert cfg["environment"]["obs_shape"] == base["environment"]["obs_shape"] == [4]
    assert cfg["transformer"] == base["transformer"] and cfg["environment"]["continuous_actions"] == 2
    assert check_box_policy(cfg) == 2
    sec = {"clip": 10.0, "epsilon": 1e-8}
    assert check_normalization_config(cfg, observation_shape=(4,), observation_dtype=torch.float32) == {"observations": sec, "rewards": sec}


@pytest.mark.parametrize("key", ("normalize_observations", "normalize_rewards"))
def test_refusals(key):
    from trainer import check_normalization_config
    with pytest.raises(ValueError, match="unknown keys.*remove"):
        check_normalization_config({key: {"clip": 10.0, "momentum": 0.9}})
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"clip must be a positive number.*default"):
            check_normalization_config({key: {"clip": bad}})
        with pytest.raises(ValueError, match=r"epsilon must be a positive number.*default"):
            check_normalization_config({key: {"epsilon": bad}})
    with pytest.raises(ValueError, match="expected true or a section"):
        check_normalization_config({key: 3})
    with pytest.raises(ValueError, match="data-parallel.*one device"):
        check_normalization_config({key: True}, world=2)
    assert check_normalization_config({key: True}, world=1)


def test_observation_key_refuses_images_bytes_and_wide_rows():
    from model import ActorCriticModel
    from trainer import check_normalization_config
    cfg = {"normalize_observations": True}
    with pytest.raises(ValueError, match=r"image / uint8.*already.*remove the key"):
        check_normalization_config(cfg, observation_shape=(3, 84, 84), observation_dtype=torch.float32)
    with pytest.raises(ValueError, match=r"image / uint8.*remove the key"):
        check_normalization_config(cfg, observation_shape=(3, 84, 84), observation_dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"1025 features.*1 to 1024"):
        check_normalization_config(cfg, observation_shape=(1025,), observation_dtype=torch.float32)
    check_normalization_config(cfg, observation_shape=(1024,), observation_dtype=torch.float32)
    # rewards: any environment
    check_normalization_config({"normalize_rewards": True}, observation_shape=(3, 84, 84), observation_dtype=torch.uint8)
    with pytest.raises(ValueError, match="vector observations"):
        ActorCriticModel(_model_cfg(normalize_observations=True), SimpleNamespace(shape=(3, 84, 84)), (3,), 16)


# ------------------------------------------------------------------ state dict
def test_state_dict_keys():
    plain, normed = _model(), _model(normalize_observations=True)
    extra = ["obs_norm_stats", "obs_norm_mean", "obs_norm_rstd"]
    assert not [k for k in plain.state_dict() if "obs_norm" in k] and plain.obs_norm is None
    assert not [n for n, _ in plain.named_buffers() if "obs_norm" in n]
    assert set(normed.state_dict()) == set(plain.state_dict()) | set(extra)
    assert len(normed.state_dict()) == len(plain.state_dict()) + 3
    assert [n for n, _ in normed.named_parameters()] == [n for n, _ in plain.named_parameters()]
    sd = normed.state_dict()
    assert sd["obs_norm_stats"].dtype == torch.float64 and tuple(sd["obs_norm_stats"].shape) == (3, 5)
    assert sd["obs_norm_mean"].dtype == sd["obs_norm_rstd"].dtype == torch.float32
    # an empty triple is the identity table
    assert not sd["obs_norm_stats"].any() and not sd["obs_norm_mean"].any() and (sd["obs_norm_rstd"] == 1).all()
    # normalize_rewards adds nothing to the model
    assert set(_model(normalize_rewards=True).state_dict()) == set(plain.state_dict())


# ------------------------------------------------------------------ the CPU encoder path
def _table(F, seed):
    rng = np.random.default_rng(seed)
    mean = (rng.normal(size=F) * 50).astype(np.float32)
    rstd = (1.0 / (0.01 + rng.random(F) * 30)).astype(np.float32)
    return mean, rstd


@pytest.mark.parametrize("F", (1, 5, 33))
def test_cpu_encode_equals_the_fp32_numpy_expression_bit_for_bit(F):
    from model import IndexedObservations
    torch.manual_seed(3)
    m = _model(F=F, normalize_observations={"clip": 2.5})
    mean, rstd = _table(F, F)
    with torch.no_grad():
        m.obs_norm_mean.copy_(torch.from_numpy(mean))
        m.obs_norm_rstd.copy_(torch.from_numpy(rstd))
    rng = np.random.default_rng(7)
    x = (mean + rng.normal(size=(64, F)) / rstd).astype(np.float32)
    x[0] = mean + np.float32(2.5) / rstd            # on the clip (up to rounding) ...
    x[1] = mean - np.float32(2.5) / rstd
    x[2] = mean + np.float32(4.0) / rstd            # ... and beyond it
    x[3] = mean - np.float32(4.0) / rstd
    ref = nr.obs_normalize_f32(x, mean, rstd, 2.5)
    assert (np.abs(ref) == 2.5).any() and (np.abs(ref) < 2.5).any()
    got = m.normalize_observations(torch.from_numpy(x)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    idx = torch.tensor([5, 0, 5, 63, 2, 2])
    got_i = m.normalize_observations(IndexedObservations(torch.from_numpy(x), idx)).numpy()
    assert np.array_equal(got_i.view(np.uint32), ref[idx.numpy()].view(np.uint32))
    # _encode: the normalised rows go through lin_hidden + ReLU and nothing else
    h = m._encode(torch.from_numpy(x)).detach()
    want = torch.relu(torch.nn.functional.linear(torch.from_numpy(ref), m.lin_hidden.weight, m.lin_hidden.bias)).detach()
    assert torch.equal(h, want)
    plain = _model(F=F)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if "obs_norm" not in k})
    assert torch.equal(plain._encode(torch.from_numpy(ref)).detach(), h), "the key absent on normalised rows = the key set on raw rows"


# ------------------------------------------------------------------ the float64 restatement of both rules
def test_observation_rule_restated():
    """Rollout 0 runs on the identity table; the table of update k is the exact statistics of updates 0 .. k - 1; the chained float64
    merge of Chan et al. agrees with the exact triple of the concatenated data inside the bound the kernels are held to."""
    from model import obs_norm_table
    rng = np.random.default_rng(11)
    F, eps, clip = 6, 1e-8, 10.0
    off, sc = rng.normal(size=F) * 100, 10.0 ** rng.uniform(-3, 3, size=F)
    batches = [(off + sc * rng.normal(size=(n, F))).astype(np.float32) for n in (64, 1, 300)]
    for b in batches:
        b[:, 2] = np.float32(7.25)                 # a constant feature: variance 0
    steps, trip = nr.obs_rule_float64(batches, eps, clip)
    mean0, rstd0, y0 = steps[0]
    assert not mean0.any() and (rstd0 == 1).all() and np.array_equal(y0, np.clip(batches[0], -10, 10))
    for k in (1, 2, 3):
        exact = nr.exact_triples_per_feature(np.concatenate(batches[:k]))
        got = nr.obs_rule_float64(batches[:k], eps, clip)[1]
        for f in range(F):
            n, mean, m2 = exact[f]
            scale = float(np.abs(batches[0][:, f]).max())
            assert got[f][0] == n
            assert nr.triple_error(got[f][1], mean, scale) <= nr.TRIPLE_REL and nr.triple_error(got[f][2], m2, scale * scale) <= nr.TRIPLE_REL
        if k < 3:
            mean_k, rstd_k, y_k = steps[k]
            want_mean = np.array([nr.round_to_f32(e[1]) for e in exact], dtype=np.float32)
            want_rstd = np.array([nr.exact_rstd_f32(e[0], e[2], eps) for e in exact], dtype=np.float32)
            assert nr.ulps32(mean_k, want_mean).max() <= 1 and nr.ulps32(rstd_k, want_rstd).max() <= 1
            assert np.abs(y_k).max() <= clip and y_k[:, 2].max() == 0.0 == y_k[:, 2].min()
            # the product's host derivation of the table from a triple
            tm, tr = obs_norm_table(torch.tensor([[t[0] for t in got], [t[1] for t in got], [t[2] for t in got]], dtype=torch.float64), eps)
            assert nr.ulps32(tm.numpy(), want_mean).max() <= 1 and nr.ulps32(tr.numpy(), want_rstd).max() <= 1
    assert exact[2][2] == 0 and want_rstd[2] == np.float32(1.0 / np.sqrt(eps))
    tm, tr = obs_norm_table(torch.zeros((3, F), dtype=torch.float64), eps)
    assert not tm.any() and (tr == 1).all()


def test_reward_rule_restated():
    """The return recurrence resets AFTER a done step and carries over rollouts; two halves = the whole; the statistics include the
    current rollout; the scaled rewards are clamp(r * scale) in float32."""
    rng = np.random.default_rng(5)
    W, S, gamma, eps, clip = 3, 10, 0.9, 1e-8, 0.5
    r = rng.normal(size=(W, S)).astype(np.float32)
    d = np.zeros((W, S), dtype=bool)
    d[0, 3] = d[1, S - 1] = d[2, 0] = True
    R, carry = nr.return_recurrence(r, d, np.zeros(W), gamma)
    assert R[0, 3] == gamma * R[0, 2] + r[0, 3] and R[0, 4] == r[0, 4], "the done step still continues the return; the next starts at 0"
    assert carry[1] == 0.0 and carry[0] == R[0, -1] and R[2, 1] == r[2, 1]
    Ra, ca = nr.return_recurrence(r[:, :4], d[:, :4], np.zeros(W), gamma)
    Rb, cb = nr.return_recurrence(r[:, 4:], d[:, 4:], ca, gamma)
    assert np.array_equal(np.concatenate([Ra, Rb], axis=1), R) and np.array_equal(cb, carry)
    one = nr.return_rule_exact(r, d, np.zeros(W), np.zeros(0), gamma, eps, clip)
    assert one["count"] == W * S
    var = float(one["m2"] / one["count"])
    assert abs(float(one["scale"]) - 1.0 / np.sqrt(var + eps)) <= 1e-6 * float(one["scale"])
    assert np.array_equal(one["scaled"], np.clip(r * one["scale"], np.float32(-clip), np.float32(clip)))
    assert (np.abs(one["scaled"]) == np.float32(clip)).any() and np.abs(one["scaled"]).max() <= clip
    # a second rollout joins the statistics of the first
    r2 = (3 * rng.normal(size=(W, S))).astype(np.float32)
    two = nr.return_rule_exact(r2, d, one["carry"], one["R"], gamma, eps, clip)
    assert two["count"] == 2 * W * S and two["scale"] < one["scale"]
    n, mean, m2 = nr.exact_triple(np.concatenate([one["R"].reshape(-1), two["R"].reshape(-1)]))
    assert (n, mean, m2) == (two["count"], two["mean"], two["m2"])
    chained = nr.merge_float64((float(W * S), float(one["R"].mean()), float(((one["R"] - one["R"].mean()) ** 2).sum())),
                               (float(W * S), float(two["R"].mean()), float(((two["R"] - two["R"].mean()) ** 2).sum())))
    assert nr.triple_error(chained[1], mean, 1.0) <= nr.TRIPLE_REL and nr.triple_error(chained[2], m2, 1.0) <= nr.TRIPLE_REL


def test_exact_triple_helper():
    x = np.array([1.5, -2.25, 1e-3, 3e7], dtype=np.float32)
    n, mean, m2 = nr.exact_triple(x)
    fr = [Fraction(float(v)) for v in x]
    assert n == 4 and mean == sum(fr) / 4 and m2 == sum((f - mean) ** 2 for f in fr)
    assert nr.exact_triple(x.astype(np.float64)) == (n, mean, m2)
    assert nr.ulps32(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).tolist() == [1, 0]


# ------------------------------------------------------------------ checkpoint
def test_pickled_checkpoint_reproduces_the_table(tmp_path):
    torch.manual_seed(1)
    cfg = _model_cfg(normalize_observations={"clip": 4.0, "epsilon": 1e-6})
    m = _model(F=5, normalize_observations=cfg["normalize_observations"])
    rng = np.random.default_rng(2)
    x = (rng.normal(size=(40, 5)) * [1, 10, 100, 1e-3, 5] + [0, 50, -7, 1, 1e3]).astype(np.float32)
    trip = nr.exact_triples_per_feature(x)
    with torch.no_grad():
        m.obs_norm_stats.copy_(torch.tensor([[float(t[0]) for t in trip], [float(t[1]) for t in trip], [float(t[2]) for t in trip]],
                                            dtype=torch.float64))
    m.refresh_obs_norm_table()
    want_rstd = np.array([nr.exact_rstd_f32(t[0], t[2], 1e-6) for t in trip], dtype=np.float32)
    assert nr.ulps32(m.obs_norm_rstd.numpy(), want_rstd).max() <= 1
    path = tmp_path / "run.nn"
    with open(path, "wb") as f:
        pickle.dump(({k: v.detach().cpu() for k, v in m.state_dict().items()}, cfg), f)
    with open(path, "rb") as f:
        state_dict, config = pickle.load(f)
    from model import ActorCriticModel
    fresh = ActorCriticModel(config, SimpleNamespace(shape=(5,)), (3,), 16)
    assert (fresh.obs_norm_rstd == 1).all()
    before = [b.data_ptr() for _, b in fresh.named_buffers()]
    fresh.load_state_dict(state_dict)
    assert before == [b.data_ptr() for _, b in fresh.named_buffers()], "loaded in place: the buffers keep their addresses"
    for name in ("obs_norm_stats", "obs_norm_mean", "obs_norm_rstd"):
        assert torch.equal(getattr(fresh, name), getattr(m, name)) and getattr(fresh, name).dtype == getattr(m, name).dtype
    xt = torch.from_numpy(x)
    assert torch.equal(fresh._encode(xt).detach(), m._encode(xt).detach())
    # a checkpoint without the key does not load into a model with it (the table would silently be the identity), and vice versa
    plain = _model(F=5)
    with pytest.raises(RuntimeError, match="obs_norm"):
        fresh.load_state_dict(plain.state_dict())
    with pytest.raises(RuntimeError, match="obs_norm"):
        plain.load_state_dict(copy.deepcopy(state_dict))
