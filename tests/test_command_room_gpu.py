"""CommandRoom on the device against the host rule, byte for byte: the kernel through the C ABI (csrc/device_env.hip) and the
device-resident front-end (environments/device_env.py) against a SerialVecEnv of host twins.  The bodies that hold for every task
are in device_env_harness.py; here are CommandRoom's cases."""
import numpy as np
import pytest

import command_room_reference as ref
import device_env_harness as harness

pytestmark = pytest.mark.gpu

GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
WIDTHS = [1, 3, 33]
CASES = [(1, 1, 0, 41), (3, 2, 1, 41), (5, 1, 2, 41), (16, 1, 0, 70)]        # (K, show_steps, gap_steps, steps)


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()


def _call(lib, G, P, W, K, show, gap, **kw):
    return harness.Call(lib, "etm_command_room", W, (G, P, K, show, gap), **kw)


@pytest.mark.parametrize("G, P", GEOMETRIES)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("K, show, gap, S", CASES)
def test_kernel_equals_the_rule_byte_for_byte(lib, G, P, W, K, show, gap, S):
    want = ref.kernel_case(G, P, W, K, show, gap, S)
    raw = want["raw"]                                                   # the kernel is given the raw values, -1 .. 6
    if W == 33:
        ref.assert_covered(want["cover"])
    assert lib.etm_command_room_supported(G, P, K) == 1 and lib.etm_command_room_state_bytes(W) == 32 * W
    harness.assert_kernel_equals_the_rule(lambda **kw: _call(lib, G, P, W, K, show, gap, **kw), raw, want, S, W, G * P)


def test_step_advances_the_state_exactly_once(lib):
    G, P, W, K, show, gap, S = 5, 8, 3, 1, 1, 0, 41
    want = ref.kernel_case(G, P, W, K, show, gap, S)
    harness.assert_step_advances_the_state_exactly_once(_call(lib, G, P, W, K, show, gap), want["raw"], want)


def test_einval_leaves_every_sentinel_in_place(lib):
    G, P, W, K = 5, 8, 3, 3
    own = [(W, G, P, 0, 2, 1, 0), (W, G, P, 17, 2, 1, 0), (W, G, P, -1, 2, 1, 0), (W, G, P, K, 0, 1, 0), (W, G, P, K, 2, -1, 0),
           (W, G, P, K, 2 ** 30, 2 ** 30, 0)]
    harness.assert_einval_leaves_every_sentinel_in_place(_call(lib, G, P, W, K, 2, 1), own)
    assert lib.etm_command_room_state_bytes(0) == 0 and lib.etm_command_room_supported(7, 12, 16) == 1
    assert lib.etm_command_room_supported(7, 12, 17) == 0 and lib.etm_command_room_supported(6, 12, 8) == 0


# ---------------------------------------------------------------------------------------------------------------- the front-end
@pytest.mark.parametrize("groups", [1, "parts"])
def test_front_end_equals_a_serial_vec_env_of_host_twins(groups):
    from environments.device_env import CommandRoomDeviceVecEnv
    cfg = dict(type="CommandRoom", grid=3, cell=12, command_count=2, show_steps=1, gap_steps=1, seed=21, device=True)
    W = 5
    rng = np.random.default_rng(8)

    def choose(t, host):
        # the correct command three times in four where one is due, so that episodes end both ways
        acts = rng.integers(0, 5, size=W).astype(np.int64)
        for w, e in enumerate(host.envs):
            if e.t >= e.show_length and rng.integers(0, 4) != 0:
                acts[w] = e.commands[e.t - e.show_length]
        return acts
    zeros = np.zeros(W, dtype=np.int64)
    ended, succeeded = harness.front_end_against_host_twins(groups, cfg, CommandRoomDeviceVecEnv, 5, 6, choose, (zeros, zeros + 4))
    assert 0 < succeeded < ended


def test_step_device_writes_the_rows_it_is_given():
    from environments.device_env import CommandRoomDeviceVecEnv
    cfg = dict(type="CommandRoom", grid=3, cell=12, command_count=1, show_steps=1, gap_steps=0, seed=1)
    harness.step_device_writes_the_rows_it_is_given(cfg, CommandRoomDeviceVecEnv, 5)
