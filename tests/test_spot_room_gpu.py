"""SpotRoom on the device against the host rule, byte for byte: the kernel through the C ABI (csrc/device_env.hip) and the
device-resident front-end (environments/device_env.py) against a SerialVecEnv of host twins.  The bodies that hold for every task
are in device_env_harness.py; here are SpotRoom's cases."""
import numpy as np
import pytest

import device_env_harness as harness
import spot_room_reference as ref

pytestmark = pytest.mark.gpu

GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
WIDTHS = [1, 3, 33]
CASES = [(0, 1, 1, 1, 6, 41), (1, 2, 1, 2, 9, 41), (2, 1, 2, 3, 20, 41), (4, 3, 3, 15, 40, 70)]      # (N, light, period, health, max_steps, steps)
# and the only geometry where lane bit 4 and phase bit 5 of a spotlight are live
LARGEST = [(31, 4, W, 4, 3, 3, 15, 40, 70) for W in (1, 3)]
ALL = [(G, P, W, *case) for G, P in GEOMETRIES for W in WIDTHS for case in CASES] + LARGEST


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()


def _call(lib, G, P, W, N, light, period, health, limit, **kw):
    return harness.Call(lib, "etm_spot_room", W, (G, P, N, light, period, health, limit), **kw)


@pytest.mark.parametrize("G, P, W, N, light, period, health, limit, S", ALL)
def test_kernel_equals_the_rule_byte_for_byte(lib, G, P, W, N, light, period, health, limit, S):
    # (frames go into a slice with a pitch above the frame size, the actions have a row stride of 3, every sentinel is checked and
    # two runs are compared: harness.Call and assert_kernel_equals_the_rule)
    want = ref.kernel_case(G, P, W, N, light, period, health, limit, S)
    raw = want["raw"]                                                   # the kernel is given the raw values, -1 .. 6
    assert -1 <= raw.min() and raw.max() <= 6 and (W < 33 or (raw.min(), raw.max()) == (-1, 6))
    assert lib.etm_spot_room_supported(G, P, N, health) == 1 and lib.etm_spot_room_state_bytes(W) == 32 * W
    harness.assert_kernel_equals_the_rule(lambda **kw: _call(lib, G, P, W, N, light, period, health, limit, **kw), raw, want, S, W, G * P)


def test_step_advances_the_state_exactly_once(lib):
    G, P, W, N, light, period, health, limit, S = 5, 8, 3, 1, 2, 1, 2, 9, 41
    want = ref.kernel_case(G, P, W, N, light, period, health, limit, S)
    harness.assert_step_advances_the_state_exactly_once(_call(lib, G, P, W, N, light, period, health, limit), want["raw"], want)


def test_einval_leaves_every_sentinel_in_place(lib):
    G, P, W, N, light, period, health, limit = 5, 8, 3, 1, 2, 1, 2, 9
    good = (W, G, P, N, light, period, health, limit, 0)
    # every rule word below its range, and above it where it has an upper end
    own = [good[:k] + (v,) + good[k + 1:] for k, values in ((3, (-1, 5)), (4, (0, -2)), (5, (0, -1)), (6, (0, 16, -3)), (7, (0, -4)))
           for v in values]
    assert len(own) == 11
    harness.assert_einval_leaves_every_sentinel_in_place(_call(lib, G, P, W, N, light, period, health, limit), own)
    assert lib.etm_spot_room_state_bytes(0) == 0 and lib.etm_spot_room_state_bytes(-2) == 0
    assert lib.etm_spot_room_state_bytes(1) == 32 and lib.etm_spot_room_state_bytes(1 << 20) == 32 << 20
    assert lib.etm_spot_room_supported(7, 12, 0, 1) == 1 and lib.etm_spot_room_supported(31, 64, 4, 15) == 1
    assert lib.etm_spot_room_supported(3, 4, 4, 15) == 1
    assert lib.etm_spot_room_supported(7, 12, 5, 5) == 0 and lib.etm_spot_room_supported(7, 12, -1, 5) == 0
    assert lib.etm_spot_room_supported(7, 12, 2, 0) == 0 and lib.etm_spot_room_supported(7, 12, 2, 16) == 0
    assert lib.etm_spot_room_supported(6, 12, 2, 5) == 0 and lib.etm_spot_room_supported(7, 10, 2, 5) == 0
    assert lib.etm_spot_room_supported(33, 12, 2, 5) == 0 and lib.etm_spot_room_supported(7, 68, 2, 5) == 0


# ---------------------------------------------------------------------------------------------------------------- the front-end
@pytest.mark.parametrize("groups", [1, "parts"])
def test_front_end_equals_a_serial_vec_env_of_host_twins(groups):
    from environments.device_env import SpotRoomDeviceVecEnv
    cfg = dict(type="SpotRoom", grid=3, cell=12, spotlights=1, light_steps=1, spot_period=1, health=2, max_episode_steps=6, seed=21,
               device=True)
    W = 5
    # (test_spot_room_host.py runs this chooser on the host twins alone: it ends episodes with and without success)
    zeros = np.zeros(W, dtype=np.int64)
    ended, succeeded = harness.front_end_against_host_twins(groups, cfg, SpotRoomDeviceVecEnv, 5, 6, ref.front_end_chooser(W),
                                                            (zeros, zeros + 4))
    assert 0 < succeeded < ended


def test_step_device_writes_the_rows_it_is_given():
    from environments.device_env import SpotRoomDeviceVecEnv
    cfg = dict(type="SpotRoom", grid=3, cell=12, spotlights=1, light_steps=1, spot_period=1, health=2, max_episode_steps=6, seed=1)
    harness.step_device_writes_the_rows_it_is_given(cfg, SpotRoomDeviceVecEnv, 5)
