"""Without a GPU: run_settings.py -- the refusal order of stage one called directly (the two walks of
tests/test_constructor_refusals_gpu.py), ``kl_plumbing`` against the rule written out, that the buffer's and the trainer's call sites
of it agree, the re-exports of trainer.py, and that the record is frozen."""
import copy
import dataclasses
import itertools

import pytest

import run_settings as rs
from test_constructor_refusals_gpu import DATA_PARALLEL_WALK, SINGLE_DEVICE_WALK, data_parallel_config, single_device_config

CHECKS = ("check_kernel_shapes", "check_box_policy", "check_byte_observation_transport", "check_truncation_transport",
          "check_action_mask_config", "check_evaluation_config", "check_normalization_config", "check_target_kl_config",
          "check_adaptive_lr_config", "check_kl_estimator_config", "check_exact_kl_config", "check_kl_penalty_config",
          "check_attention_statistics_config")


def _refused(cfg, world, message):
    with pytest.raises(ValueError) as exc:
        rs.RunSettings.before_environment(copy.deepcopy(cfg), world)
    assert str(exc.value).startswith(message), str(exc.value)


def test_data_parallel_walk():
    cfg = data_parallel_config()
    for removed, message in DATA_PARALLEL_WALK:
        for key in removed:
            del cfg[key]
        _refused(cfg, 2, message)
    del cfg["attention_statistics"]
    s = rs.RunSettings.before_environment(cfg, 2)
    assert (s.world, s.worker_processes, s.target_kl, s.adaptive_lr, s.kl_penalty, s.attention_statistics, s.evaluation,
            s.checkpoint_interval) == (2, False, None, None, None, False, None, None)
    assert (s.masked, s.prev, s.kl_analytic, s.kl_exact_cat, s.recon, s.normalization) == (None,) * 6       # (stage two fills them)


def test_single_device_walk():
    cfg = single_device_config()
    for message, fix in SINGLE_DEVICE_WALK:
        _refused(cfg, 1, message)
        fix(cfg)
    assert rs.RunSettings.before_environment(cfg, 1).worker_processes is False


def test_stage_one_keeps_what_the_keys_come_to():
    cfg = data_parallel_config()
    s = rs.RunSettings.before_environment(cfg, 1, resume=False)
    assert s.target_kl == rs.check_target_kl_config(cfg) and s.target_kl["value"] == 0.02
    assert s.adaptive_lr == rs.check_adaptive_lr_config(cfg) and s.kl_penalty == rs.check_kl_penalty_config(cfg)
    assert s.attention_statistics is True and s.checkpoint_interval == 1
    assert s.evaluation == rs.check_evaluation_config(cfg) and s.evaluation["interval"] == 2
    # a supplied environment: never worker processes, and the device-environment check is its builder's
    assert rs.RunSettings.before_environment(dict(cfg, worker_processes=True), 1, env=object()).worker_processes is False


def _kl_cells():
    """Every (config keys, continuous) of the cross product that the checks accept."""
    for est, exact, pen, box in itertools.product((None, "k3", "analytic"), (None, False, True), (None, 0.5), (False, True)):
        keys = {k: v for k, v in (("kl_estimator", est), ("exact_kl", exact), ("kl_penalty", pen)) if v is not None}
        try:
            rs.check_kl_estimator_config(keys, box)
            rs.check_exact_kl_config(keys, box)
            rs.check_kl_penalty_config(keys)
        except ValueError:
            continue
        yield keys, box


def test_kl_plumbing_is_the_rule():
    cells = list(_kl_cells())
    # refused: analytic on a categorical policy (6 cells); of the 30 others, next to k3, exact_kl: true (4) or kl_penalty without it
    # (4); kl_penalty next to exact_kl: false where k3 has not refused it already (2 without kl_estimator, 1 analytic on a Box)
    assert len(cells) == 36 - 6 - 8 - 3
    for keys, box in cells:
        exact_kl, kl_penalty, kl_estimator = bool(keys.get("exact_kl", False)), "kl_penalty" in keys, keys.get("kl_estimator", "k3")
        exact = exact_kl or kl_penalty
        analytic = kl_estimator == "analytic" or (exact and box)
        exact_cat = exact and not box
        assert rs.kl_plumbing(keys, box) == (analytic, exact_cat), (keys, box)
        assert not (analytic and exact_cat)


def test_buffer_and_trainer_agree():
    """``Buffer(config, ..., continuous=box)`` and ``RunSettings.with_environment(..., box)`` hand the one function the same two
    arguments: the config they were given and whether the policy is a Box."""
    import inspect

    import buffer
    kind = type("Kind", (), {"shape": (2,)})()
    for keys, box in _kl_cells():
        cfg = dict(keys, hidden_layer_size=64)
        stage_two = rs.RunSettings(config=cfg, world=1, worker_processes=False).with_environment(None, (4,), None, (2,) if box else (3,),
                                                                                               kind if box else None)
        assert (stage_two.kl_analytic, stage_two.kl_exact_cat) == rs.kl_plumbing(cfg, box), (keys, box)
    source = inspect.getsource(buffer.Buffer.__init__)
    assert buffer.kl_plumbing is rs.kl_plumbing and "kl_plumbing(config, continuous)" in source
    assert not any(name in source for name in ("exact_kl_section", "kl_penalty_section", "kl_estimator_section"))


def test_trainer_re_exports_every_check():
    import evaluation
    import trainer
    for name in CHECKS:
        assert getattr(trainer, name) is getattr(rs, name), name
    assert trainer.world_of is rs.world_of and evaluation.check_evaluation_config is rs.check_evaluation_config


def test_world_of():
    import types
    assert rs.world_of(None) == 1 and rs.world_of(types.SimpleNamespace(world=4, rank=1)) == 4 and rs.world_of(object()) == 1


def test_the_record_is_frozen():
    s = rs.RunSettings.before_environment(single_device_fixed(), 1)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.masked = True
    with pytest.raises(dataclasses.FrozenInstanceError):
        del s.world


def single_device_fixed():
    cfg = single_device_config()
    for _, fix in SINGLE_DEVICE_WALK:
        fix(cfg)
    return cfg
