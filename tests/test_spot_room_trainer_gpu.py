"""The trainer on SpotRoom: the device-resident front-end (``device: true``) against the host twin (``device: false``, serial), bit
for bit -- the rollout's buffer, the episode infos, the rows after the last step, the parameters after two updates, and an
evaluation -- in the captured plan that streams observations (where the fast path must really be taken), on the protocol path, with
two worker groups, with action masks and with the previous step as input.  The bodies are device_env_harness.py's; here is
SpotRoom's configuration."""
import pytest

import device_env_harness as harness

pytestmark = pytest.mark.gpu

ENV = dict(type="SpotRoom", grid=3, cell=12, spotlights=1, light_steps=1, spot_period=1, health=2, max_episode_steps=6, seed=5)
RUN = "spot_room"


@pytest.mark.parametrize("form", list(harness.FORMS))
def test_device_front_end_trains_bit_for_bit_like_the_host_twin(form):
    from environments.device_env import SpotRoomDeviceVecEnv
    harness.trains_bit_for_bit_like_the_host_twin(form, ENV, RUN, SpotRoomDeviceVecEnv)


def test_evaluation_on_the_device_config_returns_the_host_twins_result():
    harness.evaluation_returns_the_host_twins_result(ENV, RUN)


@pytest.mark.parametrize("over, match", harness.REFUSED + [
    (dict(transformer=dict(harness.TRANSFORMER, memory_length=7)), "memory_length"),      # above max_episode_steps = 6
])
def test_refused_at_construction(over, match):
    harness.refused_at_construction(ENV, RUN, over, match)


def test_worker_processes_are_refused_for_the_host_twin_too():
    harness.worker_processes_are_refused_for_the_host_twin_too(ENV, RUN)


def test_refused_in_a_data_parallel_run():
    harness.refused_in_a_data_parallel_run(ENV, RUN)
