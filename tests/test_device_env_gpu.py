"""CueRoom on the device against the host rule, byte for byte: the kernel through the C ABI (csrc/device_env.hip) and the
device-resident front-end (environments/device_env.py) against a SerialVecEnv of host twins.  The bodies that hold for every task
are in device_env_harness.py; here are CueRoom's cases."""
import itertools

import numpy as np
import pytest

import cue_room_reference as ref
import device_env_harness as harness

pytestmark = pytest.mark.gpu

GEOMETRIES = [(3, 12), (9, 4), (5, 8), (7, 12)]
WIDTHS = [1, 3, 33]
CUES = [1, 3]
LIMITS = [4, 9]


@pytest.fixture(scope="module")
def lib():
    from etm import lib as etm_lib
    return etm_lib.load()


def _call(lib, G, P, W, cue_steps, max_steps, **kw):
    return harness.Call(lib, "etm_cue_room", W, (G, P, cue_steps, max_steps), **kw)


@pytest.mark.parametrize("G, P", GEOMETRIES)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("cue_steps", CUES)
@pytest.mark.parametrize("max_steps", LIMITS)
def test_kernel_equals_the_rule_byte_for_byte(lib, G, P, W, cue_steps, max_steps):
    S = 40
    raw, want = ref.kernel_case(G, P, W, cue_steps, max_steps)          # 41 steps: the last one checks the carried state
    assert raw.min() < 0 and raw.max() > 3 or W == 1                    # (out-of-range actions for the clamp)
    assert lib.etm_cue_room_supported(G, P) == 1 and lib.etm_cue_room_state_bytes(W) == 32 * W
    harness.assert_kernel_equals_the_rule(lambda **kw: _call(lib, G, P, W, cue_steps, max_steps, **kw), raw, want, S + 1, W, G * P)


def test_the_action_sequences_cover_every_event():
    # from the rule alone: over the cases above, target hits, wrong corners, time-limit cuts and off-grid moves each occurred --
    # in every geometry, and clamped actions were among the moves
    for G, P in GEOMETRIES:
        total = dict(hit=0, wrong=0, cut=0, off_grid=0)
        for W, cue_steps, max_steps in itertools.product(WIDTHS, CUES, LIMITS):
            raw, want = ref.kernel_case(G, P, W, cue_steps, max_steps)
            for k, v in want["cover"].items():
                total[k] += v
        ref.assert_covered(total)


def test_step_advances_the_state_exactly_once(lib):
    G, P, W = 5, 8, 3
    raw, want = ref.kernel_case(G, P, W, 1, 9)
    harness.assert_step_advances_the_state_exactly_once(_call(lib, G, P, W, 1, 9), raw, want)


def test_einval_leaves_every_sentinel_in_place(lib):
    G, P, W = 5, 8, 3
    harness.assert_einval_leaves_every_sentinel_in_place(_call(lib, G, P, W, 2, 9), [(W, G, P, 0, 9, 0), (W, G, P, 2, 0, 0)])
    assert lib.etm_cue_room_state_bytes(0) == 0 and lib.etm_cue_room_supported(7, 12) == 1


# ---------------------------------------------------------------------------------------------------------------- the front-end
@pytest.mark.parametrize("groups", [1, "parts"])
def test_front_end_equals_a_serial_vec_env_of_host_twins(groups):
    from environments.device_env import CueRoomDeviceVecEnv
    cfg = dict(type="CueRoom", grid=3, cell=12, cue_steps=2, max_episode_steps=6, seed=21, device=True)
    acts = np.random.default_rng(8).integers(0, 4, size=(30, 5)).astype(np.int64)
    harness.front_end_against_host_twins(groups, cfg, CueRoomDeviceVecEnv, 4, 6, lambda t, host: acts[t], (acts[0], acts[1]))


def test_step_device_writes_the_rows_it_is_given():
    from environments.device_env import CueRoomDeviceVecEnv
    cfg = dict(type="CueRoom", grid=3, cell=12, cue_steps=1, max_episode_steps=6, seed=1)
    harness.step_device_writes_the_rows_it_is_given(cfg, CueRoomDeviceVecEnv, 4)
