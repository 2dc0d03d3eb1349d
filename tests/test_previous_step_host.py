"""previous_step_input on the host (no GPU): the parser's truth table and every refusal, utils.previous_step_fields on hand-built
rollouts, and the rows / gradient rules in float64 against a one-hot matrix product."""
import numpy as np
import pytest

from utils import (PREVIOUS_STEP_MAX_ROWS, previous_step_coefficients, previous_step_fields, previous_step_input_section, previous_step_rows,
                   previous_step_table_grad, previous_step_table_rows)


def test_parser_truth_table():
    assert previous_step_input_section({}) is None
    assert previous_step_input_section({"previous_step_input": None}) is None
    assert previous_step_input_section({"previous_step_input": False}) is None
    assert previous_step_input_section({"previous_step_input": True}) == dict(action=True, reward=True)
    for a in (False, True):
        for r in (False, True):
            cfg = {"previous_step_input": {"action": a, "reward": r}}
            if not a and not r:
                with pytest.raises(ValueError, match="at least one"):
                    previous_step_input_section(cfg)
            else:
                assert previous_step_input_section(cfg) == dict(action=a, reward=r)
    assert previous_step_input_section({"previous_step_input": {"reward": True}}) == dict(action=False, reward=True)
    assert previous_step_input_section({"previous_step_input": {"action": True}}) == dict(action=True, reward=False)


@pytest.mark.parametrize("value,match", [(1, "must be true or"), ("yes", "must be true or"), ([True], "must be true or"), (0.5, "must be true or"),
                                         ({"action": 1, "reward": True}, "action must be true or false"),
                                         ({"action": True, "reward": "no"}, "reward must be true or false"),
                                         ({"action": True, "rewards": True}, "unknown keys"), ({}, "at least one"),
                                         ({"action": False, "reward": False}, "at least one")])
def test_parser_refuses_malformed_values(value, match):
    with pytest.raises(ValueError, match=match):
        previous_step_input_section({"previous_step_input": value})


def test_parser_refuses_what_the_feature_does_not_carry():
    on = {"previous_step_input": True}
    with pytest.raises(ValueError, match="Box policy"):
        previous_step_input_section(on, action_space_shape=(2,), box=True)
    with pytest.raises(ValueError, match="worker_processes: false"):
        previous_step_input_section(on, action_space_shape=(2,), worker_processes=True)
    assert PREVIOUS_STEP_MAX_ROWS == 64
    assert previous_step_input_section(on, action_space_shape=(63,)) == dict(action=True, reward=True)
    with pytest.raises(ValueError, match="65 rows"):
        previous_step_input_section(on, action_space_shape=(64,))
    no_reward = {"previous_step_input": {"action": True}}
    assert previous_step_input_section(no_reward, action_space_shape=(32, 32)) == dict(action=True, reward=False)
    with pytest.raises(ValueError, match="65 rows"):
        previous_step_input_section(no_reward, action_space_shape=(32, 33))
    # the key absent: nothing is looked at
    assert previous_step_input_section({}, action_space_shape=(500,), box=True, worker_processes=True) is None


def test_table_rows():
    assert previous_step_table_rows((2,), True) == 3 and previous_step_table_rows((2,), False) == 2
    assert previous_step_table_rows((2, 1, 5), True) == 9 and previous_step_table_rows((63,), True) == 64
    with pytest.raises(ValueError):
        previous_step_table_rows((2, 0), True)


def test_fields_done_at_the_last_step_and_live_carry():
    # worker 0: an episode ends at step 1 and at the LAST step; worker 1: no done at all
    actions = np.array([[[1], [0], [2], [1]], [[2], [2], [0], [1]]])
    rewards = np.array([[0.5, -1.0, 2.0, 3.0], [1.0, 0.0, 0.25, -4.0]], dtype=np.float32)
    dones = np.array([[0, 1, 0, 1], [0, 0, 0, 0]], dtype=bool)
    pa, pr, carry = previous_step_fields(actions, rewards, dones)
    assert pa.dtype == np.int64 and pr.dtype == np.float32 and pa.shape == (2, 4, 1) and pr.shape == (2, 4)
    # no carry: both workers start an episode at step 0
    assert pa[:, :, 0].tolist() == [[-1, 1, -1, 2], [-1, 2, 2, 0]]
    assert pr.tolist() == [[0.0, 0.5, 0.0, 2.0], [0.0, 1.0, 0.0, 0.25]]
    ca, cr, live = carry
    assert ca.tolist() == [[1], [1]] and cr.tolist() == [3.0, -4.0] and live.tolist() == [False, True]
    # the next rollout: worker 0's step 0 has no previous step (the done at the last step), worker 1's is the carry
    actions2 = np.array([[[0], [1]], [[1], [0]]])
    rewards2 = np.array([[7.0, 8.0], [9.0, 10.0]], dtype=np.float32)
    pa2, pr2, carry2 = previous_step_fields(actions2, rewards2, np.zeros((2, 2), dtype=bool), *carry)
    assert pa2[:, :, 0].tolist() == [[-1, 0], [1, 1]]
    assert pr2.tolist() == [[0.0, 7.0], [-4.0, 9.0]]
    assert carry2[2].tolist() == [True, True] and carry2[0].tolist() == [[1], [0]] and carry2[1].tolist() == [8.0, 10.0]
    # a zero at an episode's first step is +0
    assert not np.signbit(pr[pr == 0]).any() and not np.signbit(pr2[pr2 == 0]).any()


def test_fields_multidiscrete_and_2d_actions():
    actions = np.array([[[1, 0, 4], [0, 0, 3], [1, 0, 0]]])
    rewards = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    dones = np.array([[0, 1, 0]], dtype=bool)
    pa, pr, carry = previous_step_fields(actions, rewards, dones, carry_actions=[[0, 0, 2]], carry_rewards=[-1.5], carry_live=[True])
    assert pa[0].tolist() == [[0, 0, 2], [1, 0, 4], [-1, -1, -1]]
    assert pr[0].tolist() == [-1.5, 1.0, 0.0]
    assert carry[0].tolist() == [[1, 0, 0]] and carry[2].tolist() == [True]
    # a Discrete rollout handed over as [W, S]
    pa1, _, _ = previous_step_fields(actions[:, :, 0], rewards, dones)
    assert pa1.shape == (1, 3, 1) and pa1[0, :, 0].tolist() == [-1, 1, -1]
    with pytest.raises(ValueError):
        previous_step_fields(actions, rewards[:, :2], dones)


@pytest.mark.parametrize("sizes", [(2,), (3, 3), (2, 1, 5), (63,)])
@pytest.mark.parametrize("reward", (False, True))
def test_rules_against_a_one_hot_product(sizes, reward):
    rng = np.random.default_rng(sum(sizes) + reward)
    N, D = 41, 12
    R = previous_step_table_rows(sizes, reward)
    T = rng.standard_normal((R, D))
    a = np.stack([rng.integers(0, s, size=N) for s in sizes], axis=1)
    a[rng.random(N) < 0.3] = -1
    r = rng.standard_normal(N) if reward else None
    c = previous_step_coefficients(a, r, sizes, R)
    # the coefficients: one 1 per branch inside the branch's rows, the reward in the last row, nothing for a sample without a previous step
    has = a[:, 0] >= 0
    assert (c[~has] == 0).all()
    off = 0
    for b, s in enumerate(sizes):
        assert (c[has, off:off + s].sum(axis=1) == 1).all() and (c[has, off + a[has, b]] == 1).all()
        off += s
    if reward:
        assert np.array_equal(c[has, -1], r[has])
    e = previous_step_rows(T, a, r, sizes)
    assert e.dtype == np.float64 and np.allclose(e, c @ T, rtol=0, atol=1e-14)
    assert (e[~has] == 0).all() and not np.signbit(e[~has]).any()
    bias = rng.standard_normal(D)
    assert np.allclose(previous_step_rows(T, a, r, sizes, bias=bias), c @ T + bias, rtol=0, atol=1e-14)
    gm = rng.standard_normal((N, D))
    dT = previous_step_table_grad(gm, a, r, sizes, R)
    assert dT.dtype == np.float64 and np.allclose(dT, c.T @ gm, rtol=0, atol=1e-13)
    untouched = np.abs(c).sum(axis=0) == 0
    assert untouched.any() or sizes != (63,)
    assert (dT[untouched] == 0).all() and not np.signbit(dT[untouched]).any()
    # float32: the rule's own dtype, every operation rounded on its own
    e32 = previous_step_rows(T.astype(np.float32), a, None if r is None else r.astype(np.float32), sizes, dtype=np.float32)
    assert e32.dtype == np.float32 and np.allclose(e32, e, rtol=1e-5, atol=1e-6)


def test_rows_rule_order_and_signed_zero():
    # two branches and the reward: ((+0 + T[a0]) + T[off1 + a1]) + r * T[-1] in float32, one rounding per operation
    T = np.array([[1.0], [2.0 ** -24], [3.0], [-(2.0 ** -24)], [2.0 ** -25]], dtype=np.float32)          # branches (2, 2) + the reward row
    a = np.array([[0, 1], [1, 0], [-1, 0]])
    r = np.array([3.0, 1.0, 5.0], dtype=np.float32)
    e = previous_step_rows(T, a, r, (2, 2), dtype=np.float32)
    f = np.float32
    want0 = f(f(f(0) + T[0, 0]) + T[3, 0]) + f(r[0] * T[4, 0])
    assert e[0, 0] == f(want0) and e[1, 0] == f(f(T[1, 0] + T[2, 0]) + f(r[1] * T[4, 0]))
    assert e[2, 0] == 0 and not np.signbit(e[2, 0])
    # a table of negative zeros still gives +0 (the sum starts at +0)
    z = previous_step_rows(np.full((3, 2), -0.0, dtype=np.float32), np.array([[1]]), np.array([2.0], dtype=np.float32), (2,), dtype=np.float32)
    assert (z == 0).all() and not np.signbit(z).any()
    # the action rows are not fed back: sizes () and no actions
    only_r = previous_step_rows(T, None, r, (), dtype=np.float32)
    assert np.array_equal(only_r[:, 0], r * T[4, 0])
    with pytest.raises(ValueError, match="outside its branch"):
        previous_step_rows(T, np.array([[2, 0]]), r[:1], (2, 2))
    with pytest.raises(ValueError):
        previous_step_rows(T, a, r, (2, 3))                                                          # 5 + 1 rows needed
