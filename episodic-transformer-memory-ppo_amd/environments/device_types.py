"""The environment types that have a device-resident front-end, as ONE table: what ``utils.create_env``, ``vec_env.make_vec_env``,
``check_device_env_config`` (below) and ``trainer.check_byte_observation_transport`` ask about a ``type`` is looked up here, so
no type is spelled in their code.  All of these types emit uint8 frames only (no float form) and take ``device: true``.

An entry names the rule's module (under ``environments``), its section reader, its host class and its front-end class (in
``environments/device_env.py``); everything is imported on use, so reading the table needs neither torch nor the native library.
The host class and the front-end take the section's keys (without ``device``) as keyword arguments.
"""
import importlib
from collections import namedtuple

DeviceEnvType = namedtuple("DeviceEnvType", "module section host_class front_end")

DEVICE_ENV_TYPES = {
    "CueRoom": DeviceEnvType("environments.cue_room_env", "cue_room_section", "CueRoomEnv", "CueRoomDeviceVecEnv"),
    "CommandRoom": DeviceEnvType("environments.command_room_env", "command_room_section", "CommandRoomEnv", "CommandRoomDeviceVecEnv"),
    "PathRoom": DeviceEnvType("environments.path_room_env", "path_room_section", "PathRoomEnv", "PathRoomDeviceVecEnv"),
    "SpotRoom": DeviceEnvType("environments.spot_room_env", "spot_room_section", "SpotRoomEnv", "SpotRoomDeviceVecEnv"),
}


def is_byte_only(kind) -> bool:
    """Whether environments of this ``type`` emit uint8 observations whatever ``observation_dtype`` says (they have no float form)."""
    return kind in DEVICE_ENV_TYPES


def device_env_section(env_config: dict):
    """The checked section of a config whose type is in the table (the type's own reader: defaults filled, refusals raised) -> dict
    with ``device`` among its keys; None for every other type."""
    entry = DEVICE_ENV_TYPES.get(env_config.get("type"))
    if entry is None:
        return None
    return getattr(importlib.import_module(entry.module), entry.section)(env_config)


def check_device_env_config(config: dict, world: int = 1) -> bool:
    """``environment.device: true`` against the rest of the config, before anything is built -> whether the key is on.  Refused:
    ``worker_processes: true`` (the environments live on the device, no process steps them), ``bootstrap_truncated: true`` (the
    front-end keeps no final observation) and a data-parallel run (``world`` > 1: not built, not measured).  Every type of the table
    is covered alike."""
    sec = device_env_section(config.get("environment", {}))
    if sec is None or not sec["device"]:
        return False
    if config.get("worker_processes", False):
        raise ValueError("environment.device: true keeps the environments on the device, worker_processes: true in host processes: set "
                         "worker_processes: false, or device: false to step the host twin in the worker processes")
    if config.get("bootstrap_truncated", False):
        raise ValueError("environment.device: true does not carry bootstrap_truncated: true (the device front-end keeps no final "
                         "observation): set device: false (the host twin hands it over in its info), or leave bootstrap_truncated off")
    if int(world) > 1:
        raise ValueError("environment.device: true is not built for data-parallel runs (every rank would need its own worker streams and "
                         "nothing here has run more than one rank): run one rank, or set device: false")
    return True


def _arguments(sec: dict) -> dict:
    return {k: v for k, v in sec.items() if k != "device"}


def make_host_env(env_config: dict, worker_id: int = 0):
    """The host twin (one environment) of a type in the table; ``device`` means nothing to a single environment."""
    entry = DEVICE_ENV_TYPES[env_config["type"]]
    sec = device_env_section(env_config)
    return getattr(importlib.import_module(entry.module), entry.host_class)(worker_id=worker_id, **_arguments(sec))


def make_device_vec_env(env_config: dict, num_envs: int, first_worker_id: int = 0):
    """The device-resident front-end of a type in the table (``device: true`` was asked for)."""
    entry = DEVICE_ENV_TYPES[env_config["type"]]
    sec = device_env_section(env_config)
    cls = getattr(importlib.import_module("environments.device_env"), entry.front_end)
    return cls(num_envs, first_worker_id=first_worker_id, **_arguments(sec))
