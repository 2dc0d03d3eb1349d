"""PathRoom on the device against the host rule, byte for byte: the kernel through the C ABI (csrc/device_env.hip) and the
device-resident front-end (environments/device_env.py) against a SerialVecEnv of host twins.  The bodies that hold for every task
are in device_env_harness.py; here are PathRoom's cases."""
import numpy as np
import pytest

import device_env_harness as harness
import path_room_reference as ref

pytestmark = pytest.mark.gpu

GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
WIDTHS = [1, 3, 33]
CASES = [(1, 4, 41), (5, 9, 41), (12, 20, 41), (32, 40, 70)]        # (M, max_steps, steps)
# and the only geometry where bit 63 of the path word is live: move 31 exists only at G = 31, M = 32
LARGEST = [(31, 4, W, 32, 40, 70) for W in (1, 3)]
ALL = [(G, P, W, M, limit, S) for G, P in GEOMETRIES for W in WIDTHS for M, limit, S in CASES] + LARGEST


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()


def _call(lib, G, P, W, M, limit, **kw):
    return harness.Call(lib, "etm_path_room", W, (G, P, M, limit), **kw)


@pytest.mark.parametrize("G, P, W, M, limit, S", ALL)
def test_kernel_equals_the_rule_byte_for_byte(lib, G, P, W, M, limit, S):
    # (frames go into a slice with a pitch above the frame size, the actions have a row stride of 3, every sentinel is checked and
    # two runs are compared: harness.Call and assert_kernel_equals_the_rule)
    want = ref.kernel_case(G, P, W, M, limit, S)
    raw = want["raw"]                                                   # the kernel is given the raw values, -1 .. 5
    assert -1 <= raw.min() and raw.max() <= 5 and (W < 33 or (raw.min(), raw.max()) == (-1, 5))
    assert lib.etm_path_room_supported(G, P, M) == 1 and lib.etm_path_room_state_bytes(W) == 32 * W
    harness.assert_kernel_equals_the_rule(lambda **kw: _call(lib, G, P, W, M, limit, **kw), raw, want, S, W, G * P)


def test_step_advances_the_state_exactly_once(lib):
    G, P, W, M, limit, S = 5, 8, 3, 5, 9, 41
    want = ref.kernel_case(G, P, W, M, limit, S)
    harness.assert_step_advances_the_state_exactly_once(_call(lib, G, P, W, M, limit), want["raw"], want)


def test_einval_leaves_every_sentinel_in_place(lib):
    G, P, W, M, limit = 5, 8, 3, 5, 9
    own = [(W, G, P, 0, limit, 0), (W, G, P, 33, limit, 0), (W, G, P, -1, limit, 0), (W, G, P, M, 0, 0), (W, G, P, M, -4, 0)]
    harness.assert_einval_leaves_every_sentinel_in_place(_call(lib, G, P, W, M, limit), own)
    assert lib.etm_path_room_state_bytes(0) == 0 and lib.etm_path_room_state_bytes(-2) == 0
    assert lib.etm_path_room_supported(7, 12, 32) == 1 and lib.etm_path_room_supported(31, 64, 1) == 1
    assert lib.etm_path_room_supported(7, 12, 33) == 0 and lib.etm_path_room_supported(7, 12, 0) == 0
    assert lib.etm_path_room_supported(6, 12, 8) == 0 and lib.etm_path_room_supported(7, 10, 8) == 0


# ---------------------------------------------------------------------------------------------------------------- the front-end
@pytest.mark.parametrize("groups", [1, "parts"])
def test_front_end_equals_a_serial_vec_env_of_host_twins(groups):
    from environments.device_env import PathRoomDeviceVecEnv
    cfg = dict(type="PathRoom", grid=3, cell=12, path_moves=3, max_episode_steps=6, seed=21, device=True)
    W = 5
    rng = np.random.default_rng(8)

    def choose(t, host):
        # the path's next move three times in four, so that episodes end both ways
        acts = rng.integers(0, 4, size=W).astype(np.int64)
        for w, e in enumerate(host.envs):
            if rng.integers(0, 4) != 0:
                acts[w] = e.moves[e.cells.index((e.row, e.col))]
        return acts
    zeros = np.zeros(W, dtype=np.int64)
    ended, succeeded = harness.front_end_against_host_twins(groups, cfg, PathRoomDeviceVecEnv, 4, 6, choose, (zeros, zeros + 3))
    assert 0 < succeeded < ended


def test_step_device_writes_the_rows_it_is_given():
    from environments.device_env import PathRoomDeviceVecEnv
    cfg = dict(type="PathRoom", grid=3, cell=12, path_moves=3, max_episode_steps=6, seed=1)
    harness.step_device_writes_the_rows_it_is_given(cfg, PathRoomDeviceVecEnv, 4)
