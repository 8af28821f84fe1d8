"""ctypes binding of libmegaverse_hip.so exposing the reference's ``MegaverseGym`` method table.

Reference: class MegaverseGym, src/libs/bindings/megaverse.cpp:34-292 (pybind11 module
``megaverse.extension.megaverse``).  Method names, arity and argument meaning are the same so that
``MegaverseEnv`` (megaverse_env.py here, megaverse/megaverse_env.py there) reads the same.  There is
no CPU fallback: if the shared library or a HIP device is missing, construction raises.
"""
import collections
import ctypes as C
import os
import warnings

import numpy as np

from . import build as _build

_LIB = None


class _Config(C.Structure):
    _fields_ = [
        ("scenario", C.c_char_p), ("obs_width", C.c_int32), ("obs_height", C.c_int32), ("num_envs", C.c_int32),
        ("num_agents_per_env", C.c_int32), ("num_simulation_threads", C.c_int32), ("use_vulkan", C.c_int32),
        ("device", C.c_int32), ("param_keys", C.POINTER(C.c_char_p)), ("param_vals", C.POINTER(C.c_float)),
        ("num_params", C.c_int32), ("env_offset", C.c_int32), ("total_envs", C.c_int32), ("env_stride", C.c_int32),
    ]


# every symbol include/megaverse_hip.h declares: (name, restype, argtypes)
_P, _I, _U, _F = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
SYMBOLS = [
    ("mv_last_error", C.c_char_p, []), ("mv_device_count", C.c_int, []), ("mv_abi_version", C.c_int, []),
    ("mv_create", C.c_int, [C.POINTER(_Config), C.POINTER(_P)]),
    ("mv_close", C.c_int, [_P]), ("mv_destroy", C.c_int, [_P]),
    ("mv_num_agents", C.c_int, [_P]), ("mv_action_space_sizes", C.c_int, [_P]),
    ("mv_seed", C.c_int, [_P, _I]), ("mv_reset", C.c_int, [_P]),
    ("mv_set_actions", C.c_int, [_P, _I, _I, _P, _I]),
    ("mv_set_actions_batched", C.c_int, [_P, _P]), ("mv_set_actions_device", C.c_int, [_P, _P]),
    ("mv_sample_random_actions", C.c_int, [_P, _U, _U]),
    ("mv_step_many", C.c_int, [_P, _I, _I, _I, _U, _U]),
    ("mv_group_create", C.c_int, [_P, _I, C.POINTER(_P)]), ("mv_group_step", C.c_int, [_P, _I, _I, _I, _U, _U]), ("mv_group_destroy", C.c_int, [_P]),
    ("mv_step", C.c_int, [_P]), ("mv_step_no_render", C.c_int, [_P]), ("mv_render", C.c_int, [_P]),
    ("mv_step_n", C.c_int, [_P, _I, _I, _U, _U]), ("mv_step_n_render", C.c_int, [_P, _I, _I, _U, _U, _I]), ("mv_set_sample_policy", C.c_int, [_P, _I]),
    ("mv_set_action_ring", C.c_int, [_P, _I, _P]), ("mv_debug_launch_counts", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("mv_fork_envs", C.c_int, [_P, _P]), ("mv_fork_envs_host", C.c_int, [_P, _P]), ("mv_debug_fork_plan_host", C.c_int, [_P, _I, _P, _P]),
    ("mv_debug_episodes_consumed", C.c_int, [_P, _P]), ("mv_fork_bytes_per_env", C.c_int64, [_P]),
    ("mv_resample_envs", C.c_int, [_P, _P]), ("mv_resample_envs_host", C.c_int, [_P, _P]), ("mv_resample_staging_bytes", C.c_int64, [_P]),
    ("mv_debug_resample_plan_host", C.c_int, [_P, _I, _P, _P, _P]), ("mv_debug_resample_apply_host", C.c_int, [_P, _I, _I, _P, _I]),
    ("mv_env_record_bytes", C.c_int64, [_P]), ("mv_env_record_layout", C.c_uint64, [_P]),
    ("mv_save_envs", C.c_int, [_P, _P, _P, _I]), ("mv_save_envs_host", C.c_int, [_P, _P, _P, _I]),
    ("mv_load_envs", C.c_int, [_P, _P, _P, _I]), ("mv_load_envs_host", C.c_int, [_P, _P, _P, _I]),
    ("mv_debug_env_store_plan_host", C.c_int, [_P, _I, _I, _I, _P, _P]), ("mv_debug_env_record_layout_host", C.c_int64, [_P, _I, _I, _P]),
    ("mv_debug_env_record_pack_host", C.c_int, [_P, _I, _I, C.c_uint64, _I, _P, _P]),
    ("mv_debug_env_record_unpack_host", C.c_int, [_P, _I, _I, C.c_uint64, _I, _P, _P]),
    ("mv_reset_envs", C.c_int, [_P, _P, _I]), ("mv_reset_envs_host", C.c_int, [_P, _P, _I]), ("mv_debug_episode_log_cut_host", C.c_int, [_P, _I, _I, _P, _P]),
    ("mv_seed_envs", C.c_int, [_P, _P]), ("mv_seed_envs_host", C.c_int, [_P, _P]),
    ("mv_debug_feeder_reseed_script", C.c_int, [C.c_char_p, _I, _I, _I, _P, _P, _I, _P, C.c_int64, _P]),
    ("mv_set_output_ring", C.c_int, [_P, _I, _P, _P, _P]),
    ("mv_set_pass_overlap", C.c_int, [_P, _I]),
    ("mv_recommended_ticks_per_call", C.c_int, [_P]), ("mv_recommended_pass_overlap", C.c_int, [_P]), ("mv_arena_bytes", C.c_int64, [_P]),
    ("mv_host_generator_threads", C.c_int, [_P]), ("mv_device_generator", C.c_int, [_P]),
    ("mv_is_done", C.c_int, [_P, _I]), ("mv_get_dones", C.c_int, [_P, _P]),
    ("mv_get_last_rewards", C.c_int, [_P, _P]),
    ("mv_true_objective", C.c_int, [_P, _I, _I, C.POINTER(_F)]), ("mv_get_true_objectives", C.c_int, [_P, _P]),
    ("mv_get_observation", C.c_int, [_P, _I, _I, _P]),
    ("mv_obs_device_ptr", _P, [_P]), ("mv_rewards_device_ptr", _P, [_P]), ("mv_dones_device_ptr", _P, [_P]),
    ("mv_true_objectives_device_ptr", _P, [_P]),
    ("mv_set_obs_buffer", C.c_int, [_P, _P]), ("mv_set_stream", C.c_int, [_P, _P]),
    ("mv_set_pixel_mode", C.c_int, [_P, _I]), ("mv_get_pixel_mode", C.c_int, [_P]),
    ("mv_set_obs_layout", C.c_int, [_P, _I]), ("mv_get_obs_layout", C.c_int, [_P]),
    ("mv_set_render_resolution", C.c_int, [_P, _I, _I]), ("mv_draw_hires", C.c_int, [_P]),
    ("mv_get_hires_observation", C.c_int, [_P, _I, _I, _P]), ("mv_draw_overview", C.c_int, [_P]),
    ("mv_num_reward_shaping_keys", C.c_int, [_P]), ("mv_reward_shaping_key", C.c_char_p, [_P, _I]),
    ("mv_get_reward_shaping", C.c_int, [_P, _I, _I, C.c_char_p, C.POINTER(_F)]),
    ("mv_set_reward_shaping", C.c_int, [_P, _I, _I, C.c_char_p, _F]),
    ("mv_synchronize", C.c_int, [_P]),
    ("mv_profile_begin", C.c_int, [_P, _I]), ("mv_profile_end", C.c_int, [_P, _P, _P]),
    ("mv_set_pipelining", C.c_int, [_P, _I]), ("mv_get_pipelining", C.c_int, [_P]),
    ("mv_debug_set_agent_pos", C.c_int, [_P, _I, _I, _F, _F, _F]),
    ("mv_debug_set_agent_pitch", C.c_int, [_P, _I, _I, _F]), ("mv_debug_set_objects", C.c_int, [_P, _I, _P, _I]),
    ("mv_debug_set_agent_yaw", C.c_int, [_P, _I, _I, _F, _F]), ("mv_debug_set_agent_velocity", C.c_int, [_P, _I, _I, _F, _F, _F]),
    ("mv_debug_snapshot_size", C.c_int, [_P]), ("mv_debug_snapshot", C.c_int, [_P, _I, _P]),
    ("mv_debug_boxagone_state", C.c_int, [_P, _I, _P]),
    ("mv_debug_football_state", C.c_int, [_P, _I, _P]), ("mv_debug_set_football_state", C.c_int, [_P, _I, _P]),
    ("mv_debug_rng", C.c_int, [_I, _U, _I, _P, _P, _I, _P]),
    ("mv_debug_math", C.c_int, [_I, _I, _P, _P, _I, _P]),
    ("mv_debug_sweep", C.c_int, [_I, _I, _P, _I, _P, _I, _P]), ("mv_debug_recover", C.c_int, [_I, _I, _P, _I, _P, _I, _P]),
    ("mv_debug_player_step", C.c_int, [_I, _I, _P, _I, _P, _I, _P]),
    ("mv_debug_generate_episode", C.c_int, [C.c_char_p, _I, _I, _I, _F, _P, _I]),
    ("mv_debug_feeder_selftest", C.c_int, [C.c_char_p, _I, _I, _I, _I]),
    ("mv_debug_generate_sokoban", C.c_int, [_I, _I, _I, _F, _P, _I]),
    ("mv_debug_generate_football", C.c_int, [_I, _I, _I, _F, _P, _I]),
    ("mv_debug_collect_draw_host", C.c_int, [_I, _I, _I, _F, _P, _I]),
    ("mv_debug_collect_draw_device", C.c_int, [_I, _I, _P, _I, _I, _F, _P, C.c_int64, _P]),
    ("mv_debug_obstacles_draw_host", C.c_int, [C.c_char_p, _I, _I, _I, _F, _P, _I]),
    ("mv_debug_obstacles_draw_stats_host", C.c_int, [C.c_char_p, _I, _I, _I, _F, _P]),
    ("mv_debug_obstacles_draw_device", C.c_int, [_I, C.c_char_p, _I, _P, _I, _I, _F, _P, C.c_int64, _P]),
    ("mv_set_episode_log", C.c_int, [_P, _I]), ("mv_get_episode_log_capacity", C.c_int, [_P]), ("mv_flush_episode_log", C.c_int, [_P]),
    ("mv_episode_log_count", C.c_int, [_P, C.POINTER(_U), C.POINTER(_U)]), ("mv_drain_episode_log", C.c_int, [_P, _P, _I, C.POINTER(_U)]),
    ("mv_episode_log_records_device_ptr", _P, [_P]), ("mv_episode_log_count_device_ptr", _P, [_P]),
    ("mv_episode_returns_device_ptr", _P, [_P]), ("mv_episode_lengths_device_ptr", _P, [_P]), ("mv_ticks_since_reset", C.c_int64, [_P]),
    ("mv_debug_episode_log_host", C.c_int, [_P, _P, _P, _I, _I, _I, _I, _U, _P, _P, _P, C.POINTER(_U), C.POINTER(_U)]),
    ("mv_set_step_mask", C.c_int, [_P, _P]), ("mv_set_step_mask_host", C.c_int, [_P, _P]), ("mv_get_step_mask", C.c_int, [_P]),
    ("mv_debug_episode_log_masked_host", C.c_int, [_P, _P, _P, _I, _I, _I, _I, _U, _P, _P, _P, C.POINTER(_U), C.POINTER(_U), _P]),
    ("mv_set_episode_budget", C.c_int, [_P, _P]), ("mv_set_episode_budget_host", C.c_int, [_P, _P]), ("mv_get_episode_budget", C.c_int, [_P]),
    ("mv_episode_budget_device_ptr", _P, [_P]), ("mv_halted_count_device_ptr", _P, [_P]), ("mv_halted_count", C.c_int, [_P, C.POINTER(_I)]),
    ("mv_debug_episode_log_budget_host", C.c_int, [_P, _P, _P, _I, _I, _I, _I, _U, _P, _P, _P, C.POINTER(_U), C.POINTER(_U), _P, _P]),
    ("mv_debug_episode_budget_host", C.c_int, [_P, _P, _P, _I, _I, _P, _P]),
    ("mv_debug_raster_consts_host", C.c_int, [_I, _I, _P, _P, _P, _P]), ("mv_debug_raster_div_host", C.c_int, [_U, _U, _P, _P]),
    ("mv_set_draw_mask", C.c_int, [_P, _P]), ("mv_set_draw_mask_host", C.c_int, [_P, _P]), ("mv_get_draw_mask", C.c_int, [_P]),
    ("mv_set_state_obs", C.c_int, [_P, _P]), ("mv_get_state_obs", C.c_int, [_P]), ("mv_get_state_observation", C.c_int, [_P, _I, _I, _P]),
    ("mv_debug_state_obs_host", C.c_int, [_P, _P, _P]), ("mv_get_output_ring", C.c_int, [_P]),
    ("mv_set_scene_obs", C.c_int, [_P, _P]), ("mv_get_scene_obs", C.c_int, [_P]), ("mv_get_scene_observation", C.c_int, [_P, _I, _P]),
    ("mv_debug_scene_obs_host", C.c_int, [_I, _P, _P, _P, _I, _P, _P]),
    ("mv_entity_obs_rows", C.c_int, [_P]), ("mv_entity_obs_layout", C.c_int, [_P, _P]), ("mv_set_entity_obs", C.c_int, [_P, _P]),
    ("mv_get_entity_obs", C.c_int, [_P]), ("mv_get_entity_observation", C.c_int, [_P, _I, _P]),
    ("mv_debug_entity_obs_host", C.c_int, [_I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    ("mv_macro_step", C.c_int, [_P, _I, _P, _P, _I]), ("mv_macro_step_host", C.c_int, [_P, _I, _P, _P, _I]),
    ("mv_debug_episode_log_macro_host", C.c_int, [_P, _P, _P, _I, _I, _I, _I, _U, _P, _P, _P, C.POINTER(_U), C.POINTER(_U), _P, _P, _P]),
    ("mv_debug_macro_rule_host", C.c_int, [_P, _P, _P, _P, _I, _I, _P, _P, _P]), ("mv_debug_macro_fold_host", C.c_int, [_P, _I, _I, _P]),
    ("mv_set_still_frames", C.c_int, [_P, _I]), ("mv_get_still_frames", C.c_int, [_P]),
    ("mv_debug_still_rule_host", C.c_int, [_P, _P, _P, _P, _I, _I, _P, _P]), ("mv_debug_still_carry_host", C.c_int, [_P, _P, _I, _I, _I, _I, _P, _P]),
    ("mv_set_depth_obs", C.c_int, [_P, _P, _I]), ("mv_get_depth_obs", C.c_int, [_P]), ("mv_get_depth_format", C.c_int, [_P]),
    ("mv_get_depth_observation", C.c_int, [_P, _I, _I, _P]), ("mv_debug_depth_pack_host", C.c_int, [_P, _P, _I, _I, _P]),
    ("mv_set_normal_obs", C.c_int, [_P, _P, _I]), ("mv_get_normal_obs", C.c_int, [_P]), ("mv_get_normal_format", C.c_int, [_P]),
    ("mv_get_normal_observation", C.c_int, [_P, _I, _I, _P]), ("mv_debug_normal_pack_host", C.c_int, [_P, _P, _I, _I, _P]),
    ("mv_set_seg_obs", C.c_int, [_P, _P, _I]), ("mv_get_seg_obs", C.c_int, [_P]), ("mv_get_seg_format", C.c_int, [_P]),
    ("mv_get_seg_observation", C.c_int, [_P, _I, _I, _P]), ("mv_seg_class_name", C.c_char_p, [_I]),
    ("mv_debug_seg_bounds_host", C.c_int, [_I, _I, _I, _I, _I, _I, _I, _I, _P]), ("mv_debug_seg_rule_host", C.c_int, [_I, _I, _P, _I, _I, _P]),
    ("mv_debug_seg_pack_host", C.c_int, [_P, _P, _I, _I, _P]),
    ("mv_set_overview", C.c_int, [_P, _I, _I, _P]), ("mv_set_overview_cameras", C.c_int, [_P, _P]), ("mv_set_overview_cameras_host", C.c_int, [_P, _P]),
    ("mv_get_overview_observation", C.c_int, [_P, _I, _P]), ("mv_overview_device_ptr", _P, [_P]), ("mv_overview_dropped", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("mv_overview_capacity", C.c_int, [_P]), ("mv_overview_default_camera", C.c_int, [_P]), ("mv_debug_overview_camera_host", C.c_int, [_P, _P, _P]),
]

# include/megaverse_hip.h: mv_camera, one overview camera (mv_set_overview; megaverse_amd/csrc/mv_overview.h has the rule)
MV_CAMERA_FIRST_PERSON = 1
CAMERA_DTYPE = np.dtype({"names": ["eye", "agent", "c", "flags", "pad"], "formats": [("<f4", 3), "<i4", ("<f4", 9), "<i4", ("<i4", 2)],
                         "offsets": [0, 12, 16, 52, 56], "itemsize": 64})


def overview_default_camera():
    """-> the reference's overview pose as one CAMERA_DTYPE record (render_utils.cpp:34-55; mv_overview_default_camera): eye about (-0.1414, 20, 0), looking
    along about (0.5417, -0.6428, 0.5417)"""
    out = np.zeros((), CAMERA_DTYPE)
    if load_library().mv_overview_default_camera(out.ctypes.data) != 0:
        raise RuntimeError(load_library().mv_last_error().decode())
    return out


def look_at(eye, target, up=(0, 1, 0)):
    """-> a FREE camera record at eye looking at target.  In float32, every operation rounded once: back = (eye - target) / |eye - target|,
    right = cross(up, back) / |cross(up, back)|, up' = cross(back, right); |v| = sqrt((x x + y y) + z z); cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
    a.x b.y - a.y b.x).  c's columns are right / up' / back.  ValueError where eye == target or up is parallel to the view direction."""
    f = np.float32
    e, t, u = (np.asarray(v, f).reshape(3) for v in (eye, target, up))

    def norm(v):
        n = np.sqrt(f(f(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        if not n > 0:
            raise ValueError("look_at: eye == target, or up is parallel to the view direction")
        return (v / n).astype(f)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f)

    back = norm((e - t).astype(f))
    right = norm(cross(u, back))
    up2 = cross(back, right)
    out = np.zeros((), CAMERA_DTYPE)
    out["eye"] = e
    out["agent"] = -1
    out["c"] = np.stack([right, up2, back], axis=1).reshape(9)
    return out


def follow(agent, back=0.0, up=0.0, first_person=False):
    """-> an AGENT camera record: agent's own camera, moved `back` along its back axis and `up` along its up axis (both 0: the agent's very eye, no
    arithmetic).  first_person: the agent's capsule and eyes box are not drawn -- the rule of its own observation"""
    out = np.zeros((), CAMERA_DTYPE)
    out["eye"] = (0.0, float(up), float(back))
    out["agent"] = int(agent)
    out["flags"] = MV_CAMERA_FIRST_PERSON if first_person else 0
    return out


def debug_overview_camera_host(cam, agent_state=None):
    """mv_debug_overview_camera_host: the camera the device would build from one CAMERA_DTYPE record and (AGENT mode) the 128-byte state record of its
    agent -> (eye float32 [3], c float32 [3, 3])"""
    rec = np.ascontiguousarray(np.asarray(cam, CAMERA_DTYPE).reshape(()))
    st = None if agent_state is None else np.ascontiguousarray(agent_state)
    if st is not None and st.nbytes != 128:
        raise ValueError("debug_overview_camera_host: an agent's state record is 128 bytes")
    out = np.empty(12, np.float32)
    lib = load_library()
    if lib.mv_debug_overview_camera_host(rec.ctypes.data, None if st is None else st.ctypes.data, out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out[:3].copy(), out[3:].reshape(3, 3).copy()


def check_overview_cameras(cams, num_envs, num_agents, who="set_overview_cameras"):
    """-> [num_envs] CAMERA_DTYPE, contiguous: one record (given to every env) or num_envs of them; ValueError for an agent outside -1 .. num_agents - 1
    or non-zero pad words"""
    arr = np.asarray(cams, CAMERA_DTYPE) if not (isinstance(cams, np.ndarray) and cams.dtype == CAMERA_DTYPE) else cams
    arr = arr.reshape(-1)
    if arr.size == 1:
        arr = np.repeat(arr, num_envs)
    if arr.size != num_envs:
        raise ValueError(f"{who}: {arr.size} records for {num_envs} envs")
    if ((arr["agent"] < -1) | (arr["agent"] >= num_agents)).any():
        raise ValueError(f"{who}: agent outside -1 .. {num_agents - 1}")
    if arr["pad"].any():
        raise ValueError(f"{who}: the pad words must be 0")
    return np.ascontiguousarray(arr)

# include/megaverse_hip.h: the formats of a label plane (mv_set_seg_obs), and the classes (megaverse_amd/csrc/mv_seg_obs.h has the table), name -> value
MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16 = 0, 1
SEG_FORMATS = {"class": MV_SEG_CLASS_U8, "instance": MV_SEG_INSTANCE_U16}
SEG_INSTANCE_BITS = 12
SEG_CLASSES = {name: i for i, name in enumerate((
    "NONE", "FLOOR", "STRUCTURE", "EXIT", "LAVA", "BUILDING_ZONE", "FURNITURE", "TARGET", "MOVABLE", "CARRIED", "COLLECTABLE", "HAZARD", "BALL", "AGENT", "HUD"))}


def seg_format_of(fmt):
    """'class' / 'instance' (or MV_SEG_CLASS_U8 / MV_SEG_INSTANCE_U16 themselves) -> MV_SEG_* (ValueError otherwise)"""
    if isinstance(fmt, str) and fmt in SEG_FORMATS:
        return SEG_FORMATS[fmt]
    if not isinstance(fmt, (str, bool)) and fmt in (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16):
        return int(fmt)
    raise ValueError(f"set_seg_obs: fmt must be 'class' or 'instance', got {fmt!r}")


def seg_split(words):
    """the words of an 'instance' label plane (torch tensor or numpy array, any shape) -> (cls, instance): class = word >> 12 as uint8, instance = word & 4095
    as int16 (torch has no uint16 arithmetic: an int16 tensor's bits are read as the unsigned word)"""
    if isinstance(words, np.ndarray):
        w = words.astype(np.uint16, copy=False) if words.dtype != np.int16 else words.view(np.uint16)
        return (w >> SEG_INSTANCE_BITS).astype(np.uint8), (w & 4095).astype(np.int16)
    import torch
    w = words.to(torch.int32) & 0xffff
    return (w >> SEG_INSTANCE_BITS).to(torch.uint8), (w & 4095).to(torch.int16)


def seg_class_name(cls):
    """mv_seg_class_name: the name of a class value, None outside the table (no device)"""
    name = load_library().mv_seg_class_name(int(cls))
    return name.decode() if name is not None else None


def debug_seg_bounds_host(scenario, L, W, num_boxes, num_terrain, num_objects, num_rewards, num_agents):
    """mv_debug_seg_bounds_host: an env's group boundaries (terrain, objects, rewards, agents, end) from its header's counts, on the CPU"""
    out = np.zeros(5, np.int32)
    lib = load_library()
    if lib.mv_debug_seg_bounds_host(int(scenario), int(L), int(W), int(num_boxes), int(num_terrain), int(num_objects), int(num_rewards), int(num_agents),
                                    out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return tuple(int(x) for x in out)


def debug_seg_rule_host(scenario, slot, bounds, subtype, fmt):
    """mv_debug_seg_rule_host: the label rule on the CPU (no device): one slot of an env with the group boundaries `bounds` (5 ints), subtype = the value of
    the slot's record that tells its group's sub-types apart -> the byte ('class') or the word ('instance') as an int"""
    lib = load_library()
    fmt = seg_format_of(fmt)
    b = np.ascontiguousarray(bounds, np.int32)
    if b.size != 5:
        raise ValueError("debug_seg_rule_host: bounds must hold 5 ints")
    out = np.zeros(1, np.uint16 if fmt == MV_SEG_INSTANCE_U16 else np.uint8)
    if lib.mv_debug_seg_rule_host(int(scenario), int(slot), b.ctypes.data, int(subtype), fmt, out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return int(out[0])


def debug_seg_pack_host(cls, instance, fmt):
    """mv_debug_seg_pack_host: (class, instance) pairs -> numpy uint8 [n] ('class') or uint16 [n] ('instance'), as the kernels store them (no device)"""
    lib = load_library()
    fmt = seg_format_of(fmt)
    cls = np.ascontiguousarray(cls, np.int32).ravel()
    instance = np.ascontiguousarray(instance, np.int32).ravel()
    if cls.size != instance.size:
        raise ValueError("debug_seg_pack_host: cls and instance differ in length")
    out = np.empty(cls.size, np.uint16 if fmt == MV_SEG_INSTANCE_U16 else np.uint8)
    if lib.mv_debug_seg_pack_host(cls.ctypes.data, instance.ctypes.data, int(cls.size), fmt, out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


def check_seg_obs(buf, entries, num_frames, h, w, fmt, device):
    """the argument check of MegaverseGym.set_seg_obs for a tensor: contiguous torch.uint8 ('class') or torch.int16 / torch.uint16 ('instance') of shape
    (entries, num_frames, h, w) on CUDA device `device`; entries None: any number of entries"""
    return _check_obs_tensor(buf, entries, (int(num_frames), int(h), int(w)), OBS_STREAMS['seg'].dtypes(fmt), device, 'set_seg_obs')

# include/megaverse_hip.h: the formats of a depth plane (mv_set_depth_obs), torch dtype name -> MV_DEPTH_*
MV_DEPTH_F32, MV_DEPTH_F16 = 0, 1
DEPTH_FORMATS = {"float32": MV_DEPTH_F32, "float16": MV_DEPTH_F16}


def depth_format_of(dtype):
    """a torch dtype, a numpy dtype or its name ('float32', 'float16', 'torch.float16', np.float16 ...) -> MV_DEPTH_F32 / MV_DEPTH_F16 (ValueError otherwise)"""
    name = getattr(dtype, "__name__", None) if isinstance(dtype, type) else None
    name = (name or str(dtype)).replace("torch.", "").replace("half", "float16")
    if name not in DEPTH_FORMATS:
        raise ValueError(f"set_depth_obs: dtype must be float32 or float16, got {dtype!r}")
    return DEPTH_FORMATS[name]


def debug_depth_pack_host(t, hit, fmt):
    """mv_debug_depth_pack_host: the pack rule of a depth plane on the CPU (no device): float32 t [n], hit [n] (non-zero: the ray hit) -> numpy float32 [n]
    (MV_DEPTH_F32) or float16 [n] (MV_DEPTH_F16), 0 where nothing was hit"""
    lib = load_library()
    t = np.ascontiguousarray(t, np.float32).ravel()
    hit = np.ascontiguousarray(hit, np.uint8).ravel()
    if t.size != hit.size:
        raise ValueError("debug_depth_pack_host: t and hit differ in length")
    out = np.empty(t.size, np.float16 if int(fmt) == MV_DEPTH_F16 else np.float32)
    if lib.mv_debug_depth_pack_host(t.ctypes.data, hit.ctypes.data, int(t.size), int(fmt), out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


def check_depth_obs(buf, entries, num_frames, h, w, fmt, device):
    """the argument check of MegaverseGym.set_depth_obs for a tensor: contiguous torch.float32 / torch.float16 (as fmt says) of shape (entries, num_frames, h,
    w) on CUDA device `device`; entries None: any number of entries (the check made before the gym is asked for its ring count)"""
    return _check_obs_tensor(buf, entries, (int(num_frames), int(h), int(w)), OBS_STREAMS['depth'].dtypes(fmt), device, 'set_depth_obs')

# include/megaverse_hip.h: the formats of a normal plane (mv_set_normal_obs), torch dtype name -> MV_NORMAL_*
MV_NORMAL_F16, MV_NORMAL_SNORM8 = 0, 1
NORMAL_FORMATS = {"float16": MV_NORMAL_F16, "int8": MV_NORMAL_SNORM8}


def normal_format_of(dtype):
    """a torch dtype, a numpy dtype or its name ('float16', 'int8', 'torch.int8', np.int8 ...) -> MV_NORMAL_F16 / MV_NORMAL_SNORM8 (ValueError otherwise)"""
    name = getattr(dtype, "__name__", None) if isinstance(dtype, type) else None
    name = (name or str(dtype)).replace("torch.", "").replace("half", "float16")
    if name not in NORMAL_FORMATS:
        raise ValueError(f"set_normal_obs: dtype must be float16 or int8, got {dtype!r}")
    return NORMAL_FORMATS[name]


def debug_normal_pack_host(xyz, hit, fmt):
    """mv_debug_normal_pack_host: the pack rule of a normal plane on the CPU (no device): float32 xyz [n, 3], hit [n] (non-zero: the ray hit) -> numpy
    float16 [n, 4] (MV_NORMAL_F16: x, y, z, 1) or int8 [n, 4] (MV_NORMAL_SNORM8: q(x), q(y), q(z), 127), four zeros where nothing was hit"""
    lib = load_library()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    hit = np.ascontiguousarray(hit, np.uint8).ravel()
    if xyz.shape[0] != hit.size:
        raise ValueError("debug_normal_pack_host: xyz and hit differ in length")
    out = np.empty((hit.size, 4), np.int8 if int(fmt) == MV_NORMAL_SNORM8 else np.float16)
    if lib.mv_debug_normal_pack_host(xyz.ctypes.data, hit.ctypes.data, int(hit.size), int(fmt), out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


def check_normal_obs(buf, entries, num_frames, h, w, fmt, device):
    """the argument check of MegaverseGym.set_normal_obs for a tensor: contiguous torch.float16 / torch.int8 (as fmt says) of shape (entries, num_frames, h,
    w, 4) on CUDA device `device`; entries None: any number of entries (the check made before the gym is asked for its ring count)"""
    return _check_obs_tensor(buf, entries, (int(num_frames), int(h), int(w), 4), OBS_STREAMS['normal'].dtypes(fmt), device, 'set_normal_obs')


def normals_to_float(planes):
    """a normal plane of either format -- a torch tensor or numpy array [..., 4] of float16 (MV_NORMAL_F16) or int8 (MV_NORMAL_SNORM8) -> (xyz, valid): the
    normals as float32 [..., 3] (halves widened exactly, bytes as b / 127) and a bool mask [...], True where the pixel shows a surface (w != 0)"""
    name = str(planes.dtype).replace("torch.", "")
    if name not in NORMAL_FORMATS or tuple(planes.shape)[-1:] != (4,):
        raise ValueError(f"normals_to_float: a float16 or int8 array whose last extent is 4, got {planes.dtype} {tuple(planes.shape)}")
    if isinstance(planes, np.ndarray):
        f = planes.astype(np.float32)
    else:
        import torch
        f = planes.to(torch.float32)
    if name == "int8":
        f = f / 127.0
    return f[..., :3], planes[..., 3] != 0


# include/megaverse_hip.h: MV_STATE_OBS_FLOATS and the columns of a state-observation row (mv_set_state_obs), name -> index
MV_STATE_OBS_FLOATS = 16
STATE_OBS_FIELDS = {name: i for i, name in enumerate((
    "pos_x", "pos_y", "pos_z", "m00", "m02", "m20", "m22", "pitch", "hvx", "hvz", "vvel", "carrying", "episode_sec", "episode_len", "total_reward",
    "reserved"))}


def debug_state_obs_host(agent_state, env_header):
    """mv_debug_state_obs_host: the state-observation record on the CPU (no device): the 128 bytes of one AgentState and the 128 bytes of one EnvHeader
    (megaverse_amd/csrc/mv_types.h) -> the agent's row, float32 [16]"""
    lib = load_library()
    a = np.ascontiguousarray(np.frombuffer(bytes(agent_state), np.uint8))
    h = np.ascontiguousarray(np.frombuffer(bytes(env_header), np.uint8))
    if a.size != 128 or h.size != 128:
        raise ValueError("debug_state_obs_host: an AgentState and an EnvHeader are 128 bytes each")
    out = np.empty(MV_STATE_OBS_FLOATS, np.float32)
    if lib.mv_debug_state_obs_host(a.ctypes.data, h.ctypes.data, out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


# include/megaverse_hip.h: MV_SCENE_OBS_FLOATS and the columns of a scene-observation row (mv_set_scene_obs).  SCENE_OBS_FIELDS: columns 0..15, the same for every
# scenario, name -> index; SCENE_OBS_SCENARIO_FIELDS: scenario name -> {column name: index} for columns 16..31 ({}: the scenario has none, its block is +0.0f).
# Voxel coordinates (room_*, bz_*, exit_*) are world coordinates at voxel size 1: comparable with pos_x / pos_y / pos_z of STATE_OBS_FIELDS as they are.
MV_SCENE_OBS_FLOATS = 32
SCENE_OBS_FIELDS = {name: i for i, name in enumerate((
    "scenario", "room_l", "room_h", "room_w", "num_frames", "episode_sec", "episode_len", "episodes_consumed", "solved", "highest_tower", "bz_reward",
    "num_objects", "num_rewards", "num_platforms", "num_terrain", "reserved"))}
_SCENE_TOWER = {"bz_min_x": 16, "bz_max_x": 17, "bz_min_z": 18, "bz_max_z": 19}
_SCENE_OBSTACLES = {"num_exits": 16, "exit_min_x": 17, "exit_min_y": 18, "exit_min_z": 19, "exit_max_x": 20, "exit_max_y": 21, "exit_max_z": 22,
                    "diamonds_left": 23}
_SCENE_HEX_EXPLORE = {"target_x": 16, "target_z": 17}
_SCENE_FOOTBALL = {"ball_x": 16, "ball_y": 17, "ball_z": 18, "ball_radius": 19, "ball_vx": 20, "ball_vy": 21, "ball_vz": 22, "kicks": 23,
                   "ball_wx": 24, "ball_wy": 25, "ball_wz": 26, "contacts": 27, "ball_fx": 28, "ball_fy": 29, "ball_fz": 30}
SCENE_OBS_SCENARIO_FIELDS = {
    "TowerBuilding": _SCENE_TOWER, "ObstaclesEasy": _SCENE_OBSTACLES, "ObstaclesMedium": _SCENE_OBSTACLES, "ObstaclesHard": _SCENE_OBSTACLES,
    "ObstaclesWalls": _SCENE_OBSTACLES, "ObstaclesSteps": _SCENE_OBSTACLES, "ObstaclesLava": _SCENE_OBSTACLES, "HexExplore": _SCENE_HEX_EXPLORE,
    "Football": _SCENE_FOOTBALL, "Collect": {}, "Sokoban": {}, "HexMemory": {}, "Rearrange": {}, "Empty": {}, "BoxAGone": {}}


def debug_scene_obs_host(scenario, env_header, terrain=None, rewards=None, football_state=None):
    """mv_debug_scene_obs_host: the scene-observation record on the CPU (no device): the SCN_* family id, the 128 bytes of one EnvHeader, the 512 bytes of 16
    TerrainBox, 4 bytes per MovableObject of the reward list (at most 96) and the 64 bytes of one FootballState (megaverse_amd/csrc/mv_types.h; what the
    scenario does not read may be None) -> the env's row, float32 [32]"""
    lib = load_library()
    def raw(x, size, what):
        if x is None:
            return None
        b = np.ascontiguousarray(np.frombuffer(bytes(x), np.uint8))
        if size is not None and b.size != size:
            raise ValueError(f"debug_scene_obs_host: {what} is {size} bytes")
        return b
    h, t, f = raw(env_header, 128, "an EnvHeader"), raw(terrain, 512, "a terrain list"), raw(football_state, 64, "a FootballState")
    r = raw(rewards, None, "a reward list")
    if h is None or (r is not None and r.size % 4):
        raise ValueError("debug_scene_obs_host: an EnvHeader is required, and a reward list is 4 bytes per object")
    ptr = lambda b: None if b is None or b.size == 0 else b.ctypes.data   # noqa: E731
    out = np.empty(MV_SCENE_OBS_FLOATS, np.float32)
    if lib.mv_debug_scene_obs_host(int(scenario), ptr(h), ptr(t), ptr(r), 0 if r is None else r.size // 4, ptr(f), out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


# include/megaverse_hip.h: MV_ENTITY_OBS_FLOATS and the columns of an entity-observation row (mv_set_entity_obs; megaverse_amd/csrc/mv_entity_obs.h has the table
# of every scenario's rows).  seg_word: the row's segmentation word class << 12 | instance as a float, 0 for an empty row; centre and half extents in world units.
MV_ENTITY_OBS_FLOATS = 8
ENTITY_OBS_FIELDS = {name: i for i, name in enumerate(("seg_word", "x", "y", "z", "half_x", "half_y", "half_z", "state"))}
ENTITY_GROUPS = ("terrain", "objects", "rewards", "agents")   # mv_entity_obs_layout's order: the label rule's groups
# What libmegaverse_hip.so can construct (mv_create; mv_scenarios.h has the library's row per family): every scenario of the reference's multi-task sets,
# Empty, BoxAGone and Football -- display name -> SCN_* family id (mv_types.h).  megaverse_env.SUPPORTED_SCENARIOS is this table's names, in this order.
SCENARIOS = {"TowerBuilding": 0, "ObstaclesEasy": 1, "ObstaclesMedium": 1, "ObstaclesHard": 1, "ObstaclesWalls": 1, "ObstaclesSteps": 1, "ObstaclesLava": 1,
             "Collect": 2, "Sokoban": 4, "HexMemory": 6, "HexExplore": 7, "Rearrange": 3, "Empty": 5, "BoxAGone": 8, "Football": 9}
_SCN = {name.casefold(): fam for name, fam in SCENARIOS.items()}
# the reference's eight-scenario multi-task set (megaverse_env.py:17): defined here, once, for megaverse_env, multitask and rl
MEGAVERSE8 = ["TowerBuilding", "ObstaclesEasy", "ObstaclesHard", "Collect", "Sokoban", "HexMemory", "HexExplore", "Rearrange"]
# the capacities the entity rows come from (mv_types.h)
_ENTITY_TERRAIN = {0: (1, "BUILDING_ZONE"), 1: (16, "EXIT"), 3: (8, "TARGET"), 4: (80, "EXIT")}      # family -> (rows, class of the first kind)
_ENTITY_REWARDS = {1: (16, "COLLECTABLE"), 2: (96, "COLLECTABLE"), 6: (128, "COLLECTABLE"), 7: (128, "COLLECTABLE"), 9: (1, "BALL")}
_ENTITY_OBJECTS = (0, 1, 2, 3, 4)                                                                      # the families with movable objects (80 rows)


def scenario_family(scenario):
    """a scenario name (any case) or an SCN_* family id -> the family id (ValueError: unknown)"""
    if isinstance(scenario, (int, np.integer)) and not isinstance(scenario, (bool, np.bool_)) and 0 <= int(scenario) <= max(SCENARIOS.values()):
        return int(scenario)
    fam = _SCN.get(str(scenario).casefold())
    if fam is None:
        raise ValueError(f"unknown scenario {scenario!r}")
    return fam


def _entity_groups(scenario, num_agents):
    """-> [(name, base row, rows, class value of the group's first kind or 0)] in ENTITY_GROUPS' order"""
    fam, A = scenario_family(scenario), int(num_agents)
    if not 1 <= A <= 8:
        raise ValueError(f"entity_layout: 1 <= num_agents <= 8 required, got {num_agents!r}")
    sizes = [_ENTITY_TERRAIN.get(fam, (0, "NONE")), (80, "MOVABLE") if fam in _ENTITY_OBJECTS else (0, "NONE"), _ENTITY_REWARDS.get(fam, (0, "NONE")), (A, "AGENT")]
    out, at = [], 0
    for name, (rows, cls) in zip(ENTITY_GROUPS, sizes):
        out.append((name, at, rows, SEG_CLASSES[cls]))
        at += rows
    return out


def entity_layout(scenario, num_agents):
    """the rows of an entity-observation tensor (MegaverseGym.set_entity_obs): group name ('terrain', 'objects', 'rewards', 'agents') -> slice of row indices,
    fixed for a scenario and an agent count; an empty slice: the scenario has no such group.  sum of the lengths = MegaverseGym.entity_rows()"""
    return {name: slice(base, base + rows) for name, base, rows, _ in _entity_groups(scenario, num_agents)}


def entity_rows(scenario, num_agents):
    """E: the rows per env of an entity-observation tensor"""
    return sum(rows for _, _, rows, _ in _entity_groups(scenario, num_agents))


def entity_row_of(words, scenario, num_agents):
    """the words of an 'instance' label plane (int16 / int32 torch tensor, or numpy array, any shape) -> the row index of each word's entity in the env's
    [E, 8] entity rows, same shape, int32 (numpy) / int64 (torch): rows are slot-addressed, so this is arithmetic -- group base + instance.  -1: the word's
    class has no rows (NONE, FLOOR, STRUCTURE, FURNITURE, HUD, a class of another scenario), its instance lies beyond the group -- and Sokoban's EXIT, the one
    compacted group: find its row by comparing the word with column 0 of the group's rows."""
    groups = {name: (base, rows) for name, base, rows, _ in _entity_groups(scenario, num_agents)}
    fam = scenario_family(scenario)
    by_class = {}   # class value -> (base, rows)
    if fam != 4:
        for cls in {0: ("BUILDING_ZONE",), 1: ("EXIT", "LAVA"), 3: ("TARGET",)}.get(fam, ()):
            by_class[SEG_CLASSES[cls]] = groups["terrain"]
    for cls in ("MOVABLE", "CARRIED"):
        by_class[SEG_CLASSES[cls]] = groups["objects"]
    for cls in {1: ("COLLECTABLE",), 2: ("COLLECTABLE", "HAZARD"), 6: ("COLLECTABLE",), 7: ("COLLECTABLE",), 9: ("BALL",)}.get(fam, ()):
        by_class[SEG_CLASSES[cls]] = groups["rewards"]
    by_class[SEG_CLASSES["AGENT"]] = groups["agents"]
    is_np = isinstance(words, np.ndarray)
    if is_np:
        w = (words.view(np.uint16) if words.dtype == np.int16 else words).astype(np.int32) & 0xffff
        out = np.full(w.shape, -1, np.int32)
    else:
        import torch
        w = words.to(torch.int64) & 0xffff
        out = torch.full_like(w, -1)
    cls, inst = w >> SEG_INSTANCE_BITS, w & 4095
    for c, (base, rows) in by_class.items():
        hit = (cls == c) & (inst < rows)
        out[hit] = (base + inst[hit]).to(out.dtype) if not is_np else (base + inst[hit]).astype(out.dtype)
    return out


def debug_entity_obs_host(scenario, num_agents, env_header, agents, terrain=None, items=None, soko=None, objects=None, rewards=None, hex_objs=None,
                          football_state=None):
    """mv_debug_entity_obs_host: the entity-observation record on the CPU (no device): the SCN_* family id, the agent count, the 128 bytes of one EnvHeader,
    128 bytes per AgentState, and -- what the scenario does not read may be None -- the 512 bytes of 16 TerrainBox, the 256 of 8 ArrangementItem, the 1024
    Sokoban cell bytes, the 320 of 80 MovableObject, 4 bytes per MovableObject of the reward list, the 4096 of 128 HexRec, the 64 of one FootballState
    (megaverse_amd/csrc/mv_types.h) -> the env's rows, float32 [E, 8]"""
    lib = load_library()
    def raw(x, size, what):
        if x is None:
            return None
        b = np.ascontiguousarray(np.frombuffer(bytes(x), np.uint8))
        if size is not None and b.size != size:
            raise ValueError(f"debug_entity_obs_host: {what} is {size} bytes")
        return b
    A = int(num_agents)
    E = entity_rows(scenario, A)
    h, a = raw(env_header, 128, "an EnvHeader"), raw(agents, 128 * A, "num_agents AgentStates")
    t, it, sk = raw(terrain, 512, "a terrain list"), raw(items, 256, "an item list"), raw(soko, 1024, "Sokoban's cells")
    o, hx, f = raw(objects, 320, "an object list"), raw(hex_objs, 4096, "a HexRec list"), raw(football_state, 64, "a FootballState")
    r = raw(rewards, None, "a reward list")
    if h is None or a is None or (r is not None and r.size % 4):
        raise ValueError("debug_entity_obs_host: an EnvHeader and the AgentStates are required, and a reward list is 4 bytes per object")
    ptr = lambda b: None if b is None or b.size == 0 else b.ctypes.data   # noqa: E731
    out = np.empty((E, MV_ENTITY_OBS_FLOATS), np.float32)
    if lib.mv_debug_entity_obs_host(scenario_family(scenario), A, ptr(h), ptr(t), ptr(it), ptr(sk), ptr(o), ptr(r), 0 if r is None else r.size // 4, ptr(hx),
                                    ptr(f), ptr(a), out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


# mv_episode_record (include/megaverse_hip.h): one finished episode of one agent, 24 bytes
EPISODE_RECORD_DTYPE = np.dtype({"names": ["agent", "length", "end_tick", "true_objective", "ret"],
                                 "formats": ["<i4", "<i4", "<u4", "<f4", "<f8"], "offsets": [0, 4, 8, 12, 16], "itemsize": 24})


class _DeviceArray:
    """a device pointer as something torch.as_tensor takes (the CUDA array interface): no copy, the gym keeps the memory"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def debug_episode_log_host(rewards, dones, true_objectives, agents_per_env, capacity, first_tick=0, state=None):
    """mv_debug_episode_log_host: the episode log's per-tick body on the CPU (no device).  rewards / true_objectives [k][N*A] float32, dones [k][N] uint8.
    state: what an earlier call returned (carried on), or None for a log just switched on.  -> state = {'ret', 'len', 'records', 'count', 'dropped'};
    state['records'][:state['count']] is the log."""
    return _episode_log_host(False, None, rewards, dones, true_objectives, agents_per_env, capacity, first_tick, state)


def debug_episode_log_masked_host(step_mask, rewards, dones, true_objectives, agents_per_env, capacity, first_tick=0, state=None):
    """mv_debug_episode_log_masked_host: debug_episode_log_host with a step mask (mv_set_step_mask) -- step_mask: [N] raw bytes, the envs whose byte is 0
    skip all k ticks; None: the hook's NULL mask, every env steps."""
    return _episode_log_host(True, step_mask, rewards, dones, true_objectives, agents_per_env, capacity, first_tick, state)


def debug_episode_log_budget_host(step_mask, left, rewards, dones, true_objectives, agents_per_env, capacity, first_tick=0, state=None):
    """mv_debug_episode_log_budget_host: debug_episode_log_masked_host with an episode budget (mv_set_episode_budget) -- left: int32 [N], the log's mirror of
    the budgets, advanced IN PLACE tick by tick (it must be a contiguous int32 numpy array); None: the hook's NULL, no budget."""
    if left is not None and not (isinstance(left, np.ndarray) and left.dtype == np.int32 and left.flags.c_contiguous and left.ndim == 1):
        raise ValueError("debug_episode_log_budget_host: left is a contiguous int32 numpy array [N], advanced in place")
    return _episode_log_host(True, step_mask, rewards, dones, true_objectives, agents_per_env, capacity, first_tick, state, budget=(left,))


def debug_episode_log_macro_host(step_mask, left, tl, rewards, dones, true_objectives, agents_per_env, capacity, first_tick=0, state=None):
    """mv_debug_episode_log_macro_host: debug_episode_log_budget_host for the k ticks of one macro step (mv_macro_step) -- tl: int32 [N], the log's mirror of
    the envs' ticks left, set by the caller to the call's clamped ticks and advanced IN PLACE tick by tick (a contiguous int32 numpy array); None: the
    hook's NULL, no macro step"""
    for name, v in (("left", left), ("tl", tl)):
        if v is not None and not (isinstance(v, np.ndarray) and v.dtype == np.int32 and v.flags.c_contiguous and v.ndim == 1):
            raise ValueError(f"debug_episode_log_macro_host: {name} is a contiguous int32 numpy array [N], advanced in place")
    return _episode_log_host(True, step_mask, rewards, dones, true_objectives, agents_per_env, capacity, first_tick, state, budget=(left, tl))


def debug_episode_budget_host(dones, mask, left):
    """mv_debug_episode_budget_host: the rule of episode budgets on the CPU (no device).  dones [k][N]: what tick t stages for env e if it steps; mask [N]
    bytes or None; left int32 [N] -> (steps uint8 [k][N]: 1 where the env steps in the tick, left int32 [N] behind the last tick)"""
    lib = load_library()
    dones = np.ascontiguousarray(dones, np.uint8)
    k, N = dones.shape
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    if left.size != N or (m is not None and m.size != N):
        raise ValueError("debug_episode_budget_host: dones is [k][N], mask and left are [N]")
    steps, out = np.full((k, N), 9, np.uint8), np.full(N, -9, np.int32)
    if lib.mv_debug_episode_budget_host(dones.ctypes.data, None if m is None else m.ctypes.data, left.ctypes.data, k, N, steps.ctypes.data, out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return steps, out


def debug_macro_rule_host(dones, mask, left, ticks):
    """mv_debug_macro_rule_host: the rule of macro steps on the CPU (no device), one call of k ticks.  dones [k][N]: what tick t stages for env e if it steps;
    mask [N] bytes or None; left int32 [N] or None (no budget: -1 for every env); ticks int32 [N] or None (every env: k) -> (steps uint8 [k][N]: 1 where
    the env steps in the tick, left int32 [N] and ticks left int32 [N] behind the last tick)"""
    lib = load_library()
    dones = np.ascontiguousarray(dones, np.uint8)
    k, N = dones.shape
    left = np.full(N, -1, np.int32) if left is None else np.ascontiguousarray(left, np.int32).reshape(-1)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    t = None if ticks is None else np.ascontiguousarray(ticks, np.int32).reshape(-1)
    if left.size != N or (m is not None and m.size != N) or (t is not None and t.size != N):
        raise ValueError("debug_macro_rule_host: dones is [k][N], mask, left and ticks are [N]")
    steps, left_out, ticks_out = np.full((k, N), 9, np.uint8), np.full(N, -9, np.int32), np.full(N, -9, np.int32)
    if lib.mv_debug_macro_rule_host(dones.ctypes.data, None if m is None else m.ctypes.data, left.ctypes.data, None if t is None else t.ctypes.data, k, N,
                                    steps.ctypes.data, left_out.ctypes.data, ticks_out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return steps, left_out, ticks_out


def debug_macro_fold_host(values):
    """mv_debug_macro_fold_host: the fold of a macro step's rewards on the CPU (no device): values float32 [k][n] -> float32 [n], s = v_0; s = s + v_t in
    tick order"""
    lib = load_library()
    v = np.ascontiguousarray(values, np.float32)
    if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError("debug_macro_fold_host: values is [k][n], k >= 1, n >= 1")
    out = np.empty(v.shape[1], np.float32)
    if lib.mv_debug_macro_fold_host(v.ctypes.data, v.shape[0], v.shape[1], out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


def debug_still_rule_host(steps, has_pass, draw_mask, stale):
    """mv_debug_still_rule_host: the rule of still frames on the CPU (no device).  steps [k][N]: 1 where the env steps in the tick; has_pass [k]: 1 where the
    tick has an observation pass; draw_mask [N] or None; stale [N].  -> (verdict int32 [k][N]: 0 no pass, 1 drawn, -1 user-undrawn, -2 still; stale uint8 [N]
    behind the last tick)"""
    lib = load_library()
    steps = np.ascontiguousarray(steps, dtype=np.uint8)
    has_pass = np.ascontiguousarray(has_pass, dtype=np.uint8)
    stale = np.ascontiguousarray(stale, dtype=np.uint8)
    m = None if draw_mask is None else np.ascontiguousarray(draw_mask, dtype=np.uint8)
    if steps.ndim != 2 or has_pass.shape != (steps.shape[0],) or stale.shape != (steps.shape[1],) or (m is not None and m.shape != stale.shape):
        raise ValueError("debug_still_rule_host: steps is [k][N], has_pass [k], draw_mask and stale are [N]")
    k, N = steps.shape
    verdict, out = np.zeros((k, N), np.int32), np.zeros(N, np.uint8)
    if lib.mv_debug_still_rule_host(steps.ctypes.data, has_pass.ctypes.data, None if m is None else m.ctypes.data, stale.ctypes.data, k, N,
                                    verdict.ctypes.data, out.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return verdict, out


def debug_still_carry_host(verdict, entries, ring, home):
    """mv_debug_still_carry_host: the carry of still frames on the CPU (no device), one call.  verdict int32 [k][frames]: what the passes read (>= 0 drawn,
    -1 user-undrawn, -2 still); entries [k]: each rendered tick's ring entry; ring: contiguous uint8 [R][frames][frame_bytes], copied IN PLACE; home:
    contiguous int32 [frames], advanced IN PLACE."""
    lib = load_library()
    verdict = np.ascontiguousarray(verdict, dtype=np.int32)
    entries = np.ascontiguousarray(entries, dtype=np.int32)
    for name, a, dt in (("ring", ring, np.uint8), ("home", home, np.int32)):
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous:
            raise ValueError(f"debug_still_carry_host: {name} is a contiguous {np.dtype(dt).name} numpy array, changed in place")
    if verdict.ndim != 2 or ring.ndim != 3 or entries.shape != (verdict.shape[0],) or ring.shape[1] != verdict.shape[1] or home.shape != (verdict.shape[1],):
        raise ValueError("debug_still_carry_host: verdict is [k][frames], entries [k], ring [R][frames][frame_bytes], home [frames]")
    if lib.mv_debug_still_carry_host(verdict.ctypes.data, entries.ctypes.data, verdict.shape[0], verdict.shape[1], ring.shape[0], ring.shape[2],
                                     ring.ctypes.data, home.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())


def check_macro_step_args(actions, ticks, num_envs, num_agents):
    """the argument check of MegaverseGym.macro_step: actions [num_envs * num_agents, 6] and ticks [num_envs] or None, both int32 -- either contiguous CUDA
    tensors (-> 'device': read in place) or host arrays (-> contiguous int32 numpy arrays); the two must be of the same kind"""
    na, n = int(num_envs) * int(num_agents), int(num_envs)

    def one(x, shape, what):
        if hasattr(x, 'data_ptr'):
            contiguous = getattr(x, 'is_contiguous', None)
            if tuple(getattr(x, 'shape', ())) != shape or str(getattr(x, 'dtype', None)) != 'torch.int32' \
                    or not getattr(x, 'is_cuda', False) or not (callable(contiguous) and contiguous()):
                raise ValueError(f'macro_step: a tensor of {what} must be a contiguous int32 CUDA tensor of shape {shape}, '
                                 f"got {getattr(x, 'dtype', None)} {tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', 'an unknown device')}")
            return 'device'
        b = np.asarray(x)
        if b.shape != shape or b.dtype.kind not in 'iu' or (b.size and (b.min() < -2 ** 31 or b.max() >= 2 ** 31)):
            raise ValueError(f'macro_step: {what} must be int32 values of shape {shape}, got {b.dtype} {b.shape}')
        return np.ascontiguousarray(b, dtype=np.int32)

    if actions is None:
        raise ValueError('macro_step: actions are required')
    a = one(actions, (na, 6), 'actions')
    t = None if ticks is None else one(ticks, (n,), 'ticks')
    if t is not None and isinstance(a, str) != isinstance(t, str):
        raise ValueError('macro_step: actions and ticks must both be CUDA tensors or both be host arrays')
    return a, t


def _episode_log_host(masked, step_mask, rewards, dones, true_objectives, agents_per_env, capacity, first_tick, state, budget=None):
    lib = load_library()
    rewards = np.ascontiguousarray(rewards, np.float32)
    dones = np.ascontiguousarray(dones, np.uint8)
    true_objectives = np.ascontiguousarray(true_objectives, np.float32)
    k, N = dones.shape
    A = int(agents_per_env)
    if rewards.shape != (k, N * A) or true_objectives.shape != (k, N * A):
        raise ValueError("debug_episode_log_host: rewards and true_objectives are [k][N*A], dones [k][N]")
    if state is None:
        state = {"ret": np.zeros(N * A, np.float64), "len": np.zeros(N, np.int32), "records": np.zeros(max(int(capacity), 0), EPISODE_RECORD_DTYPE),
                 "count": 0, "dropped": 0}
    count, dropped = _U(state["count"]), _U(state["dropped"])
    args = (rewards.ctypes.data, dones.ctypes.data, true_objectives.ctypes.data, k, N, A, int(capacity), int(first_tick) & 0xFFFFFFFF,
            state["ret"].ctypes.data, state["len"].ctypes.data, state["records"].ctypes.data, C.byref(count), C.byref(dropped))
    if not masked:
        rc = lib.mv_debug_episode_log_host(*args)
    else:
        m = None if step_mask is None else np.ascontiguousarray(step_mask, np.uint8).reshape(-1)   # (the raw bytes: any non-zero byte steps)
        if m is not None and m.size != N:
            raise ValueError("debug_episode_log_masked_host: step_mask is [N] bytes")
        if budget is None:
            rc = lib.mv_debug_episode_log_masked_host(*args, None if m is None else m.ctypes.data)
        else:
            left = budget[0]
            if left is not None and left.size != N:
                raise ValueError("debug_episode_log_budget_host: left is [N]")
            if len(budget) > 1:   # (debug_episode_log_macro_host)
                tl = budget[1]
                if tl is not None and tl.size != N:
                    raise ValueError("debug_episode_log_macro_host: tl is [N]")
                rc = lib.mv_debug_episode_log_macro_host(*args, None if m is None else m.ctypes.data, None if left is None else left.ctypes.data,
                                                         None if tl is None else tl.ctypes.data)
            else:
                rc = lib.mv_debug_episode_log_budget_host(*args, None if m is None else m.ctypes.data, None if left is None else left.ctypes.data)
    if rc != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    state["count"], state["dropped"] = int(count.value), int(dropped.value)
    return state


def debug_fork_plan_host(src_of):
    """mv_debug_fork_plan_host: the rule of a fork map on the CPU (no device) -> (resolved int32 [N]: the source of entry d, or -1; invalid uint8-like [N])"""
    lib = load_library()
    m = np.ascontiguousarray(src_of, np.int32).reshape(-1)
    resolved, invalid = np.full(m.size, -9, np.int32), np.full(m.size, -9, np.int32)
    if m.size and lib.mv_debug_fork_plan_host(m.ctypes.data, m.size, resolved.ctypes.data, invalid.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return resolved, invalid


def debug_resample_plan_host(src_of):
    """mv_debug_resample_plan_host: the rule of a resampling map on the CPU (no device) -> (resolved int32 [N]: the source of entry d, or -1; staged [N]: 1
    where env d's new state goes through the staging arena; invalid [N]: 1 where the index is out of range)"""
    lib = load_library()
    m = np.ascontiguousarray(src_of, np.int32).reshape(-1)
    resolved, staged, invalid = (np.full(m.size, -9, np.int32) for _ in range(3))
    if m.size and lib.mv_debug_resample_plan_host(m.ctypes.data, m.size, resolved.ctypes.data, staged.ctypes.data, invalid.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return resolved, staged, invalid


def debug_resample_apply_host(src_of, state, order=0):
    """mv_debug_resample_apply_host: the two phases of mv_resample_envs on the CPU (no device) over state, a uint8 array [N][bytes per env] -> the state
    after the call (a copy).  order: 0 / 1 / 2 = the envs of each phase ascending / descending / in a fixed pseudo-random order."""
    lib = load_library()
    m = np.ascontiguousarray(src_of, np.int32).reshape(-1)
    state = np.asarray(state)
    if state.dtype != np.uint8 or state.ndim != 2 or state.shape[0] != m.size:
        raise ValueError("debug_resample_apply_host: state is a uint8 array [N][bytes per env], N the length of the map")
    out = np.array(state, order="C", copy=True)   # (never None for ctypes, even where it is empty)
    if m.size and lib.mv_debug_resample_apply_host(m.ctypes.data, m.size, out.shape[1], out.ctypes.data, int(order)) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return out


def check_fork_map(src_of, num_envs, who='fork_envs', meaning='src_of[d] = the env that env d continues from, -1 or d: left alone'):
    """the argument check of MegaverseGym.fork_envs (and, with their own who / meaning, of save_envs / load_envs): a CUDA int32 tensor of shape (num_envs,)
    -> 'device'; anything else -> a contiguous int32 numpy array"""
    if hasattr(src_of, 'data_ptr'):
        if tuple(src_of.shape) != (int(num_envs),) or str(src_of.dtype) != 'torch.int32' or not src_of.is_cuda or not src_of.is_contiguous():
            raise ValueError(f'{who}: a tensor map must be a contiguous int32 CUDA tensor of shape ({int(num_envs)},), '
                             f'got {src_of.dtype} {tuple(src_of.shape)} on {src_of.device}')
        return 'device'
    m = np.asarray(src_of)
    if m.shape != (int(num_envs),) or m.dtype.kind not in 'iu':
        raise ValueError(f'{who}: the map must be {int(num_envs)} integers ({meaning}), '
                         f'got {m.dtype} {m.shape}')
    return np.ascontiguousarray(m, dtype=np.int32)


def check_env_store(store, record_bytes, who='save_envs'):
    """the argument check of MegaverseGym.save_envs / load_envs for the store: a contiguous CUDA uint8 tensor [slots, record_bytes] -> slots"""
    if not hasattr(store, 'data_ptr') or str(store.dtype) != 'torch.uint8' or not store.is_cuda:
        raise ValueError(f'{who}: the store must be a torch.uint8 CUDA tensor of shape (slots, {int(record_bytes)}) (new_env_store makes one)')
    if store.dim() != 2 or int(store.shape[1]) != int(record_bytes) or int(store.shape[0]) < 1:
        raise ValueError(f'{who}: the store must have shape (slots, {int(record_bytes)}) -- one record of env_record_bytes() bytes per slot -- '
                         f'got {tuple(store.shape)}')
    if not store.is_contiguous():
        raise ValueError(f'{who}: the store must be contiguous (its records are read and written in place)')
    return int(store.shape[0])


def debug_env_store_plan_host(slot_of, slots, is_save):
    """mv_debug_env_store_plan_host: the rule of a save_envs / load_envs map on the CPU (no device) -> (resolved int32 [N]: the slot of entry e, or -1;
    invalid [N])"""
    lib = load_library()
    m = np.ascontiguousarray(slot_of, np.int32).reshape(-1)
    resolved, invalid = np.full(m.size, -9, np.int32), np.full(m.size, -9, np.int32)
    if m.size and lib.mv_debug_env_store_plan_host(m.ctypes.data, m.size, int(slots), int(bool(is_save)), resolved.ctypes.data, invalid.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return resolved, invalid


def debug_env_record_layout_host(array_bytes, agents_per_env):
    """mv_debug_env_record_layout_host -> (record bytes, offsets uint32 [count + 3]: the EnvHeader, each array, ret, len)"""
    lib = load_library()
    b = np.ascontiguousarray(array_bytes, np.uint32).reshape(-1)
    off = np.zeros(b.size + 3, np.uint32)
    n = lib.mv_debug_env_record_layout_host(b.ctypes.data if b.size else off.ctypes.data, b.size, int(agents_per_env), off.ctypes.data)
    if n < 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return int(n), off


def debug_env_record_pack_host(array_bytes, agents_per_env, layout_word, log_on, env_state):
    """mv_debug_env_record_pack_host: env_state (uint8: the 128-byte EnvHeader, the arrays, double ret[A], int32 len, without gaps) -> the record (uint8)"""
    lib = load_library()
    b = np.ascontiguousarray(array_bytes, np.uint32).reshape(-1)
    env = np.ascontiguousarray(env_state, np.uint8).reshape(-1)
    if env.size != 128 + int(b.sum()) + 8 * int(agents_per_env) + 4:
        raise ValueError("debug_env_record_pack_host: env_state is the EnvHeader, the arrays, ret[A] and len, one behind the other")
    record = np.full(debug_env_record_layout_host(b, agents_per_env)[0], 0xEE, np.uint8)
    if lib.mv_debug_env_record_pack_host(b.ctypes.data if b.size else record.ctypes.data, b.size, int(agents_per_env), int(layout_word), int(bool(log_on)),
                                         env.ctypes.data, record.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return record


def debug_env_record_unpack_host(array_bytes, agents_per_env, layout_word, log_on, record, env_state):
    """mv_debug_env_record_unpack_host: the record into a copy of env_state -> (refused: bool, the env afterwards)"""
    lib = load_library()
    b = np.ascontiguousarray(array_bytes, np.uint32).reshape(-1)
    env = np.array(env_state, dtype=np.uint8, order="C", copy=True).reshape(-1)
    rec = np.ascontiguousarray(record, np.uint8).reshape(-1)
    if env.size != 128 + int(b.sum()) + 8 * int(agents_per_env) + 4 or rec.size != debug_env_record_layout_host(b, agents_per_env)[0]:
        raise ValueError("debug_env_record_unpack_host: wrong size of env_state or record")
    rc = lib.mv_debug_env_record_unpack_host(b.ctypes.data if b.size else rec.ctypes.data, b.size, int(agents_per_env), int(layout_word), int(bool(log_on)),
                                             rec.ctypes.data, env.ctypes.data)
    if rc < 0:
        raise RuntimeError(lib.mv_last_error().decode())
    return rc == 1, env


def debug_episode_log_cut_host(mask, agents_per_env, ret, length):
    """mv_debug_episode_log_cut_host: the episode log's masked clear on the CPU (no device).  mask [N] (non-zero: cut), ret float64 [N*A] and length
    int32 [N] are changed in place: a flagged env's running returns and running length go to zero."""
    lib = load_library()
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    A = int(agents_per_env)
    if ret.dtype != np.float64 or length.dtype != np.int32 or ret.shape != (m.size * A,) or length.shape != (m.size,) \
            or not ret.flags.c_contiguous or not length.flags.c_contiguous:
        raise ValueError("debug_episode_log_cut_host: ret is a contiguous float64 [N*A], length a contiguous int32 [N]")
    if lib.mv_debug_episode_log_cut_host(m.ctypes.data, m.size, A, ret.ctypes.data, length.ctypes.data) != 0:
        raise RuntimeError(lib.mv_last_error().decode())


def _check_env_mask(mask, num_envs, who, non_zero):
    """one byte per env, for `who`: a CUDA bool / uint8 tensor (or anything with data_ptr()) of shape (num_envs,) -> 'device'; anything else -> a contiguous
    uint8 numpy array; non_zero: what a set byte means, for the error text"""
    n = int(num_envs)
    if hasattr(mask, 'data_ptr'):
        contiguous = getattr(mask, 'is_contiguous', None)
        if tuple(getattr(mask, 'shape', ())) != (n,) or str(getattr(mask, 'dtype', None)) not in ('torch.bool', 'torch.uint8') \
                or not getattr(mask, 'is_cuda', False) or not (callable(contiguous) and contiguous()):
            raise ValueError(f'{who}: a tensor mask must be a contiguous bool or uint8 CUDA tensor of shape ({n},), '
                             f"got {getattr(mask, 'dtype', None)} {tuple(getattr(mask, 'shape', ()))} on {getattr(mask, 'device', 'an unknown device')}")
        return 'device'
    m = np.asarray(mask)
    if m.shape != (n,) or m.dtype.kind not in 'bu' or (m.dtype.kind == 'u' and m.dtype.itemsize != 1):
        raise ValueError(f'{who}: the mask must be {n} bools (or uint8: non-zero = {non_zero}), got {m.dtype} {m.shape}')
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def check_reset_mask(mask, num_envs):
    """the argument check of MegaverseGym.reset_envs: a CUDA bool / uint8 tensor (or anything with data_ptr()) of shape (num_envs,) -> 'device'; anything else
    -> a contiguous uint8 numpy array, one byte per env"""
    return _check_env_mask(mask, num_envs, 'reset_envs', 'reset this env')


def check_step_mask(mask, num_envs):
    """the argument check of MegaverseGym.set_step_mask: None (detach) -> None; otherwise check_reset_mask's rules -- a contiguous bool / uint8 CUDA tensor of
    shape (num_envs,) -> 'device'; anything else -> a contiguous uint8 numpy array, one byte per env (non-zero: the env steps, 0: it is frozen)"""
    return None if mask is None else _check_env_mask(mask, num_envs, 'set_step_mask', 'the env steps')


def check_draw_mask(mask, num_envs):
    """the argument check of MegaverseGym.set_draw_mask: check_step_mask's rules (non-zero: the env's frames are drawn, 0: they are neither set up nor drawn)"""
    return None if mask is None else _check_env_mask(mask, num_envs, 'set_draw_mask', 'the env is drawn')


def check_state_obs(buf, entries, num_rows, device):
    """the argument check of MegaverseGym.set_state_obs for a tensor: contiguous torch.float32 of shape (entries, num_rows, 16) on CUDA device `device`;
    entries None: any number of entries (the check made before the gym is asked for its ring count)"""
    return _check_obs_tensor(buf, entries, (int(num_rows), MV_STATE_OBS_FLOATS), OBS_STREAMS['state'].dtypes(None), device, 'set_state_obs')


def check_scene_obs(buf, entries, num_envs, device):
    """the argument check of MegaverseGym.set_scene_obs for a tensor: contiguous torch.float32 of shape (entries, num_envs, 32) on CUDA device `device`;
    entries None: any number of entries (the check made before the gym is asked for its ring count)"""
    return _check_obs_tensor(buf, entries, (int(num_envs), MV_SCENE_OBS_FLOATS), OBS_STREAMS['scene'].dtypes(None), device, 'set_scene_obs')


def check_entity_obs(buf, entries, num_envs, rows, device):
    """the argument check of MegaverseGym.set_entity_obs for a tensor: contiguous torch.float32 of shape (entries, num_envs, rows, 8) on CUDA device `device`,
    16-byte aligned; entries None: any number of entries (the check made before the gym is asked for its ring count)"""
    return _check_obs_tensor(buf, entries, (int(num_envs), int(rows), MV_ENTITY_OBS_FLOATS), OBS_STREAMS['entity'].dtypes(None), device, 'set_entity_obs')


def _check_obs_tensor(buf, entries, tail, dtypes, device, who):
    """the one tensor check of the observation streams, for the setter `who`: contiguous, one of `dtypes` (torch dtype names), of shape (entries,) + tail on
    CUDA device `device`; entries None: any number of entries (the check made before the gym is asked for its ring count) -> buf"""
    got = tuple(getattr(buf, 'shape', ()))
    shape = ((got[0] if len(got) == len(tail) + 1 else 1) if entries is None else int(entries),) + tuple(tail)
    contiguous = getattr(buf, 'is_contiguous', None)
    dev = getattr(buf, 'device', None)
    index = getattr(dev, 'index', None)
    if not hasattr(buf, 'data_ptr') or got != shape or str(getattr(buf, 'dtype', None)) not in dtypes \
            or not getattr(buf, 'is_cuda', False) or not (callable(contiguous) and contiguous()) or (index is not None and int(index) != int(device)):
        raise ValueError(f"{who}: the buffer must be a contiguous {' / '.join(x[6:] for x in dtypes)} CUDA tensor of shape {shape} on device {int(device)}, "
                         f"got {getattr(buf, 'dtype', type(buf).__name__)} {tuple(getattr(buf, 'shape', ()))} on {dev if dev is not None else 'no device'}")
    return buf


# The six per-tick observation streams of a MegaverseGym, stated once: the library's setter and single-row reader, the shape behind `entries` as a function
# of the gym (a read-back's row is that shape without its first extent), format -> the torch dtype names a tensor may have (the first: what True allocates),
# the arguments behind the null pointer of a detach, the numpy dtype a read-back hands out.  A new stream is one row here.
_ObsStream = collections.namedtuple('_ObsStream', 'setter reader tail dtypes detach read')
_FLOAT32 = ('torch.float32',)
OBS_STREAMS = {
    'state': _ObsStream('mv_set_state_obs', 'mv_get_state_observation', lambda g: (g.num_envs * g.num_agents_per_env, MV_STATE_OBS_FLOATS),
                        lambda fmt: _FLOAT32, (), np.float32),
    'scene': _ObsStream('mv_set_scene_obs', 'mv_get_scene_observation', lambda g: (g.num_envs, MV_SCENE_OBS_FLOATS), lambda fmt: _FLOAT32, (), np.float32),
    'entity': _ObsStream('mv_set_entity_obs', 'mv_get_entity_observation',
                         lambda g: (g.num_envs, entity_rows(g.scenario, g.num_agents_per_env), MV_ENTITY_OBS_FLOATS), lambda fmt: _FLOAT32, (), np.float32),
    'depth': _ObsStream('mv_set_depth_obs', 'mv_get_depth_observation', lambda g: (g.num_envs * g.num_agents_per_env, g.h, g.w),
                        lambda fmt: ('torch.float16',) if int(fmt) == MV_DEPTH_F16 else _FLOAT32, (MV_DEPTH_F32,), np.float32),
    'seg': _ObsStream('mv_set_seg_obs', 'mv_get_seg_observation', lambda g: (g.num_envs * g.num_agents_per_env, g.h, g.w),
                      lambda fmt: ('torch.int16', 'torch.uint16') if int(fmt) == MV_SEG_INSTANCE_U16 else ('torch.uint8',), (MV_SEG_CLASS_U8,), np.uint16),
    'normal': _ObsStream('mv_set_normal_obs', 'mv_get_normal_observation', lambda g: (g.num_envs * g.num_agents_per_env, g.h, g.w, 4),
                         lambda fmt: ('torch.int8',) if int(fmt) == MV_NORMAL_SNORM8 else ('torch.float16',), (MV_NORMAL_F16,), np.float32),
}


def check_episode_budget(budget, num_envs):
    """the argument check of MegaverseGym.set_episode_budget: None (detach) -> None; an int -> that value for every env; a contiguous torch.int32 CUDA tensor
    of shape (num_envs,) (or anything with data_ptr()) -> 'device'; anything else -> a contiguous int32 numpy array, one value per env"""
    n = int(num_envs)
    if budget is None:
        return None
    if isinstance(budget, (int, np.integer)) and not isinstance(budget, (bool, np.bool_)):
        if not -2 ** 31 <= int(budget) < 2 ** 31:
            raise ValueError(f'set_episode_budget: {budget} is not an int32')
        return np.full(n, int(budget), np.int32)
    if hasattr(budget, 'data_ptr'):
        contiguous = getattr(budget, 'is_contiguous', None)
        if tuple(getattr(budget, 'shape', ())) != (n,) or str(getattr(budget, 'dtype', None)) != 'torch.int32' \
                or not getattr(budget, 'is_cuda', False) or not (callable(contiguous) and contiguous()):
            raise ValueError(f'set_episode_budget: a tensor budget must be a contiguous int32 CUDA tensor of shape ({n},), '
                             f"got {getattr(budget, 'dtype', None)} {tuple(getattr(budget, 'shape', ()))} on {getattr(budget, 'device', 'an unknown device')}")
        return 'device'
    b = np.asarray(budget)
    if b.shape != (n,) or b.dtype.kind not in 'iu' or (b.size and (b.min() < -2 ** 31 or b.max() >= 2 ** 31)):
        raise ValueError(f'set_episode_budget: the budget must be {n} int32 values (< 0: unlimited, 0: halted), got {b.dtype} {b.shape}')
    return np.ascontiguousarray(b, dtype=np.int32)


def check_env_seeds(seeds, num_envs):
    """the argument check of MegaverseGym.seed_envs (include/megaverse_hip.h: mv_seed_envs).  A contiguous torch.int32 CUDA tensor of shape (num_envs,) (or
    anything with data_ptr()) -> 'device'.  Anything else -> a contiguous int32 numpy array, one word per env, negative = "leave this env alone": a dict
    {env: seed}; a sequence or array of num_envs ints in which None, like a negative entry, leaves the env alone."""
    n = int(num_envs)
    if hasattr(seeds, 'data_ptr'):
        contiguous = getattr(seeds, 'is_contiguous', None)
        if tuple(getattr(seeds, 'shape', ())) != (n,) or str(getattr(seeds, 'dtype', None)) != 'torch.int32' \
                or not getattr(seeds, 'is_cuda', False) or not (callable(contiguous) and contiguous()):
            raise ValueError(f'seed_envs: a tensor of seeds must be a contiguous int32 CUDA tensor of shape ({n},), '
                             f"got {getattr(seeds, 'dtype', None)} {tuple(getattr(seeds, 'shape', ()))} on {getattr(seeds, 'device', 'an unknown device')}")
        return 'device'

    def word(v, what):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'seed_envs: {what} must be an int, got {v!r}')
        if not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f'seed_envs: {what} = {v} is not an int32')
        return int(v)

    out = np.full(n, -1, np.int32)
    if isinstance(seeds, dict):
        for e, v in seeds.items():
            e = word(e, 'an env index')
            if not 0 <= e < n:
                raise ValueError(f'seed_envs: env {e} is not within 0 .. {n - 1}')
            if v is not None:
                out[e] = word(v, f'the seed of env {e}')
        return out
    if isinstance(seeds, np.ndarray):
        if seeds.shape != (n,) or (seeds.dtype.kind not in 'iu' and seeds.dtype != object):
            raise ValueError(f'seed_envs: the seeds must be {n} ints (negative or None: leave the env alone), got {seeds.dtype} {seeds.shape}')
        if seeds.dtype != object:
            if seeds.size and (seeds.min() < -2 ** 31 or seeds.max() >= 2 ** 31):
                raise ValueError('seed_envs: a seed is not an int32')
            return np.ascontiguousarray(seeds, dtype=np.int32)
    try:
        items = list(seeds)
    except TypeError:
        raise ValueError(f'seed_envs: {n} ints, a dict {{env: seed}} or an int32 CUDA tensor, got {type(seeds).__name__}') from None
    if len(items) != n:
        raise ValueError(f'seed_envs: the seeds must be {n} ints (negative or None: leave the env alone), got {len(items)}')
    for e, v in enumerate(items):
        if v is not None:
            out[e] = word(v, f'the seed of env {e}')
    return out


def debug_feeder_reseed_script(scenario, num_agents, threads, env_seeds, script):
    """mv_debug_feeder_reseed_script: the episode feeder driven without a device.  env_seeds: the envs' initial seeds; script: a list of ('take', env),
    ('seed', env, value) and ('commit',) -- a commit is ONE reseed_envs call with the seeds listed since the last.  Every delivered episode is compared
    inside with straight sequential generation (RuntimeError on a difference).  -> [(env, the record's bytes, the bytes the feeder reports as used)] per take"""
    lib = load_library()
    seeds = np.ascontiguousarray(env_seeds, np.int32).reshape(-1)
    ops = np.zeros((len(script), 3), np.int32)
    for k, op in enumerate(script):
        ops[k] = {'take': (0, op[1] if len(op) > 1 else 0, 0), 'seed': (1, op[1] if len(op) > 1 else 0, op[2] if len(op) > 2 else 0), 'commit': (2, 0, 0)}[op[0]]
    takes = int((ops[:, 0] == 0).sum())
    size = lib.mv_debug_feeder_reseed_script(scenario.encode(), 1, 1, 1, None, None, 0, None, 0, None)
    if size < 0:
        raise RuntimeError(lib.mv_last_error().decode())
    out = np.zeros((max(1, takes), size), np.uint8)
    used = np.zeros(max(1, takes), np.int32)
    rc = lib.mv_debug_feeder_reseed_script(scenario.encode(), seeds.size, int(num_agents), int(threads), seeds.ctypes.data, ops.ctypes.data, len(script),
                                           out.ctypes.data, out.nbytes, used.ctypes.data)
    if rc < 0:
        raise RuntimeError(lib.mv_last_error().decode())
    envs = ops[ops[:, 0] == 0, 1]
    return [(int(envs[i]), out[i].tobytes(), int(used[i])) for i in range(rc)]


# include/megaverse_hip.h: MV_RENDER_EVERY / MV_RENDER_LAST / MV_RENDER_NONE, by the names step_n(render=...) takes
RENDER_MODES = {"every": 0, "last": 1, "none": 2}


def render_mode_of(render):
    """the argument check of MegaverseGym.step_n's render: 'every' | 'last' | 'none' -> MV_RENDER_*"""
    try:
        return RENDER_MODES[render]
    except (KeyError, TypeError):
        raise ValueError(f"step_n: render must be one of {sorted(RENDER_MODES)}, got {render!r}") from None


def library_path():
    return _build.LIB


def load_library():
    """dlopen libmegaverse_hip.so (building it first if a source is newer) and type every symbol."""
    global _LIB
    if _LIB is None:
        path = _build.LIB
        if _build.is_stale() and os.path.exists("/opt/rocm/bin/hipcc"):
            _build.build()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        # PyTorch wheels bundle their own HIP/HSA runtime under the system runtime's SONAME.  If torch is
        # imported AFTER this library, the process ends up with two runtimes and the second one to
        # initialise reports "no ROCm-capable device".  Importing torch first makes both share one.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(path)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)   # AttributeError here == the C ABI lost a symbol
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


class GymGroup:
    """mv_group: up to eight gyms of one job stepped with union launches (one step launch, at most two observation launches per tick).
    The gyms must share device, observation size, agents per env and stream (set_stream first)."""

    def __init__(self, gyms):
        self._lib = load_library()
        self.gyms = list(gyms)
        handles = (_P * len(self.gyms))(*[g._g for g in self.gyms])
        h = _P()
        if self._lib.mv_group_create(handles, len(self.gyms), C.byref(h)) != 0:
            raise RuntimeError("mv_group_create: " + self._lib.mv_last_error().decode())
        self._h = h

    def step(self, k=1, render=True, policy="none", seed=0, first_step_index=0):
        rc = self._lib.mv_group_step(self._h, int(k), 1 if render else 0, int(MegaverseGym.POLICIES.get(policy, policy)), int(seed) & 0xFFFFFFFF,
                                     int(first_step_index) & 0xFFFFFFFF)
        if rc < 0:
            raise RuntimeError(self._lib.mv_last_error().decode())
        if rc > 0:
            warnings.warn(self._lib.mv_last_error().decode(), RuntimeWarning, stacklevel=2)

    def close(self):
        if self._h is not None:
            self._lib.mv_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_log_level = 2


def set_megaverse_log_level(level):
    """reference: setMegaverseLogLevel, megaverse.cpp:29-32.  The HIP library does not log."""
    global _log_level
    _log_level = int(level)


class MegaverseGym:
    """Same constructor and methods as the reference's pybind class (megaverse.cpp:267-292)."""

    def __init__(self, scenario, w, h, num_envs, num_agents_per_env, num_simulation_threads, use_vulkan, float_params,
                 device=0, env_offset=0, total_envs=0, env_stride=1):
        self._lib = load_library()
        fp = dict(float_params or {})
        keys = (C.c_char_p * max(1, len(fp)))(*[k.encode() for k in fp])
        vals = (C.c_float * max(1, len(fp)))(*[float(v) for v in fp.values()])
        self._keep = (keys, vals)
        cfg = _Config(scenario.encode(), int(w), int(h), int(num_envs), int(num_agents_per_env), int(num_simulation_threads),
                      int(bool(use_vulkan)), int(device), keys, vals, len(fp), int(env_offset), int(total_envs), int(env_stride))
        handle = _P()
        self._g = None
        if self._lib.mv_create(C.byref(cfg), C.byref(handle)) != 0:
            raise RuntimeError("mv_create: " + self._lib.mv_last_error().decode())
        self._g = handle
        self.w, self.h, self.num_envs, self.num_agents_per_env, self.device = int(w), int(h), int(num_envs), int(num_agents_per_env), int(device)
        self.scenario = str(scenario)
        self.render_w, self.render_h = 768, 432
        self._fork_held = None   # fork_envs: the caller's device map, kept until the next step has been enqueued
        self._reset_held = None  # reset_envs: the caller's device mask, likewise
        self._seed_held = []     # seed_envs: the caller's device seeds, likewise (calls may follow each other without a step: every tensor is kept)
        self._step_mask_held = None  # set_step_mask: the caller's device mask, kept until it is replaced or detached
        self._draw_mask_held = None  # set_draw_mask: the caller's device mask, kept until it is replaced or detached
        self._obs = {}               # set_*_obs: stream name (OBS_STREAMS) -> the attached tensor
        self._ring_ticks = 0         # ticks stepped through this object since set_output_ring (the library's own count: which entry the last tick went to)
        self._macro_held = None      # macro_step: the caller's device tensors of the last call, read in stream order: kept until the next macro step
        self._budget_held = None     # set_episode_budget: the caller's device tensor, read in stream order: kept until the next step has been enqueued
        self._store_held = []    # save_envs / load_envs: the caller's stores and device maps, kept until the next step has been enqueued
        self._overview = None    # set_overview: the attached tensor (the caller's, or a view of the gym's own frames)
        self._overview_cams_held = None  # set_overview_cameras: the caller's device records, copied in stream order: kept until they are replaced

    def _ck(self, rc):
        if rc < 0:
            raise RuntimeError(self._lib.mv_last_error().decode())
        return rc

    def _ckw(self, rc):
        """stepping calls: 1 = done, with a warning (a capacity limit was hit and is reported once; include/megaverse_hip.h)"""
        if rc < 0:
            raise RuntimeError(self._lib.mv_last_error().decode())
        if rc > 0:
            warnings.warn(self._lib.mv_last_error().decode(), RuntimeWarning, stacklevel=3)
        return rc

    # ---- the reference's method table ----
    def num_agents(self):
        return self.num_agents_per_env

    def action_space_sizes(self):
        out = (C.c_int32 * 6)()
        self._lib.mv_action_space_sizes(out)
        return list(out)

    def seed(self, seed):
        self._ck(self._lib.mv_seed(self._g, int(seed)))

    def reset(self):
        self._ckw(self._lib.mv_reset(self._g))

    def set_actions(self, env_idx, agent_idx, actions):
        arr = (C.c_int32 * len(actions))(*[int(a) for a in actions])
        self._ck(self._lib.mv_set_actions(self._g, int(env_idx), int(agent_idx), arr, len(actions)))

    def step(self):
        self._ckw(self._lib.mv_step(self._g))
        self._ring_ticks += 1
        self._fork_held = self._reset_held = self._budget_held = None
        self._store_held = []
        self._seed_held = []

    def is_done(self, env_idx):
        return bool(self._ck(self._lib.mv_is_done(self._g, int(env_idx))))

    def get_observation(self, env_idx, agent_idx):
        out = np.empty((self.h, self.w, 4), np.uint8)
        self._ck(self._lib.mv_get_observation(self._g, int(env_idx), int(agent_idx), out.ctypes.data))
        return out

    def get_last_rewards(self):
        out = np.empty(self.num_envs * self.num_agents_per_env, np.float32)
        self._ck(self._lib.mv_get_last_rewards(self._g, out.ctypes.data))
        return out.tolist()

    def true_objective(self, env_idx, agent_idx):
        v = _F()
        self._ck(self._lib.mv_true_objective(self._g, int(env_idx), int(agent_idx), C.byref(v)))
        return float(v.value)

    def set_render_resolution(self, w, h):
        self._ck(self._lib.mv_set_render_resolution(self._g, int(w), int(h)))
        self.render_w, self.render_h = int(w), int(h)

    def draw_hires(self):
        self._ck(self._lib.mv_draw_hires(self._g))

    def draw_overview(self):
        """With an overview attached (set_overview): every env drawn from its overview camera into overview_obs(), in the order of the gym's stream, no host
        wait.  With none: nothing, as the reference's build without a window."""
        self._ck(self._lib.mv_draw_overview(self._g))

    def set_overview(self, w, h, buf=True):
        """Overview cameras (include/megaverse_hip.h: mv_set_overview): one camera per env, free in the world or attached to an agent, drawn by
        draw_overview() with the exact pass's arithmetic into a CUDA uint8 tensor [num_envs, h, w, 4] (RGBA, row 0 the bottom row) -- the caller's (checked,
        ValueError), or with True / None the gym's own.  1 <= w, h <= 1024; w = h = 0 detaches.  Every env starts at the reference's pose
        (overview_default_camera).  Nothing a stepping call launches or writes changes.  -> overview_obs()"""
        w, h = int(w), int(h)
        if w == 0 and h == 0:
            self._ck(self._lib.mv_set_overview(self._g, 0, 0, None))
            self._overview = None
            return None
        if buf is None or buf is True:
            self._ck(self._lib.mv_set_overview(self._g, w, h, None))
            import torch
            ptr = int(self._lib.mv_overview_device_ptr(self._g))
            self._overview = torch.as_tensor(_DeviceArray(ptr, (self.num_envs, h, w, 4), "|u1"), device=f'cuda:{self.device}')
            return self._overview
        import torch
        if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()
                and tuple(buf.shape) == (self.num_envs, h, w, 4) and (buf.device.index or 0) == self.device):
            raise ValueError(f"set_overview: the buffer must be a contiguous CUDA uint8 tensor [{self.num_envs}, {h}, {w}, 4] on device {self.device}")
        self._ck(self._lib.mv_set_overview(self._g, w, h, _P(int(buf.data_ptr()))))
        self._overview = buf
        return buf

    def overview_obs(self):
        """-> torch.uint8 [num_envs, h, w, 4]: the frames draw_overview writes, valid in the order of the gym's stream; None with no overview attached"""
        return self._overview

    def set_overview_cameras(self, cams):
        """One camera per env (CAMERA_DTYPE; look_at, follow, overview_default_camera build records): a record or a sequence / array of num_envs records --
        checked (ValueError) and copied in stream order, the host free again on return --; a CUDA tensor of num_envs * 16 int32 / float32 words holding the
        same records -- copied on the gym's stream, an agent outside -1 .. A - 1 taken as FREE and counted (overview_dropped) --; None: back to the default pose."""
        if cams is None:
            self._ck(self._lib.mv_set_overview_cameras_host(self._g, None))
            self._overview_cams_held = None
            return
        if hasattr(cams, 'data_ptr'):
            import torch
            if not (cams.is_cuda and cams.dtype in (torch.int32, torch.float32) and cams.is_contiguous() and cams.numel() == self.num_envs * 16
                    and (cams.device.index or 0) == self.device):
                raise ValueError(f"set_overview_cameras: a device form is a contiguous CUDA int32 / float32 tensor of {self.num_envs} x 16 words on device {self.device}")
            self._ck(self._lib.mv_set_overview_cameras(self._g, _P(int(cams.data_ptr()))))
            self._overview_cams_held = cams
            return
        arr = check_overview_cameras(cams, self.num_envs, self.num_agents_per_env)
        self._ck(self._lib.mv_set_overview_cameras_host(self._g, arr.ctypes.data))
        self._overview_cams_held = None

    def get_overview_observation(self, env_idx):
        """-> numpy uint8 [h, w, 4]: one env's overview frame as last drawn (waits for the gym's stream)"""
        if self._overview is None:
            raise RuntimeError("get_overview_observation: no overview attached (set_overview)")
        out = np.empty(tuple(self._overview.shape[1:]), np.uint8)
        self._ck(self._lib.mv_get_overview_observation(self._g, int(env_idx), out.ctypes.data))
        return out

    def overview_dropped(self):
        """-> (primitives that did not fit an env's list, clamped agent indices of device records) since the first attach (waits for the gym's stream)"""
        v = C.c_int64(0)
        self._ck(self._lib.mv_overview_dropped(self._g, C.byref(v)))
        return int(v.value) & 0xffffffff, (int(v.value) >> 32) & 0xffffffff

    def overview_capacity(self):
        """-> the list capacity per env of this gym's overview: 256, 1024 or 2048, by the scenario's slot count"""
        return self._ck(self._lib.mv_overview_capacity(self._g))

    def get_hires_observation(self, env_idx, agent_idx):
        out = np.empty((self.render_h, self.render_w, 4), np.uint8)
        self._ck(self._lib.mv_get_hires_observation(self._g, int(env_idx), int(agent_idx), out.ctypes.data))
        return out

    def get_reward_shaping(self, env_idx, agent_idx):
        out = {}
        for i in range(self._lib.mv_num_reward_shaping_keys(self._g)):
            key = self._lib.mv_reward_shaping_key(self._g, i)
            v = _F()
            self._ck(self._lib.mv_get_reward_shaping(self._g, int(env_idx), int(agent_idx), key, C.byref(v)))
            out[key.decode()] = float(v.value)
        return out

    def set_reward_shaping(self, env_idx, agent_idx, reward_shaping):
        # reference semantics: the map is REPLACED (scenario.hpp:215); keys this scenario does not
        # know are an error here instead of a later std::out_of_range
        for k, v in reward_shaping.items():
            self._ck(self._lib.mv_set_reward_shaping(self._g, int(env_idx), int(agent_idx), k.encode(), float(v)))

    def close(self):
        if self._g is not None:
            self._lib.mv_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- batched extensions (no per-agent Python loop; SURVEY.md 3.2 hot loop iii) ----
    def set_actions_batched(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(self.num_envs * self.num_agents_per_env, 6)
        self._ck(self._lib.mv_set_actions_batched(self._g, a.ctypes.data))

    def set_actions_device(self, device_ptr):
        """int32 [num_agents, 6] multi-discrete actions in device memory.  Nothing is launched here: the NEXT step kernel reads the buffer (in the
        order of the gym's stream), so the caller keeps it alive and unchanged until that step() call has returned; mv_reset and the host-side
        action setters read a pending buffer at once instead (last writer wins)."""
        self._ck(self._lib.mv_set_actions_device(self._g, _P(int(device_ptr))))

    def sample_random_actions(self, seed, step_index):
        self._ck(self._lib.mv_sample_random_actions(self._g, int(seed) & 0xFFFFFFFF, int(step_index) & 0xFFFFFFFF))

    def step_no_render(self):
        self._ckw(self._lib.mv_step_no_render(self._g))
        self._ring_ticks += 1
        self._fork_held = self._reset_held = self._budget_held = None
        self._store_held = []
        self._seed_held = []

    POLICIES = {"none": 0, "multidiscrete": 1, "single-bit": 2, "sequence": 3}

    def step_n(self, k, policy="multidiscrete", seed=0, first_step_index=0, render="every"):
        """k open-loop ticks (each stepped and rendered) with one call; tick j draws its actions from (policy, seed, first_step_index + j) --
        policy 'sequence': it acts on entry (first_step_index + j) % count of the action ring (set_action_ring), seed is ignored.
        render (include/megaverse_hip.h: mv_step_n_render): 'every' (default: mv_step_n itself); 'none': the ticks run, rewards and dones go where they
        always go, nothing is drawn and no byte of the observation slab or ring is written; 'last': as 'none', and the call's last tick is drawn into its
        own place."""
        mode = render_mode_of(render)
        args = (self._g, int(k), int(self.POLICIES.get(policy, policy)), int(seed) & 0xFFFFFFFF, int(first_step_index) & 0xFFFFFFFF)
        self._ckw(self._lib.mv_step_n(*args) if mode == 0 else self._lib.mv_step_n_render(*args, mode))
        self._ring_ticks += int(k)
        self._fork_held = self._reset_held = self._budget_held = None
        self._store_held = []
        self._seed_held = []

    def macro_step(self, k, actions, ticks=None, render="last"):
        """A macro step (include/megaverse_hip.h: mv_macro_step): the actions -- int32 [num_agents, 6], multi-discrete -- are held for up to k ticks, every
        env stops at its own first done (it then stands on the first frame of its next episode), and the call leaves ONE set of outputs: the rewards summed
        in tick order (fp32, left to right), the dones OR-ed, and with render='last' the frame behind the call's last tick ('none': nothing is drawn).  With
        an output ring the call fills one entry.  ticks: None (every env: k) or int32 [num_envs], clamped to [0, k] -- env e holds its action for ticks[e]
        ticks; 0: it does not step.  Contiguous int32 CUDA tensors are read in place, in the order of the gym's stream, without a host synchronisation (the
        gym holds a reference until the next stepping call has been enqueued; leave them unchanged until the stream has passed the call); numpy arrays or
        lists are copied through a staging buffer.  render='every' is refused: a decision has one frame."""
        mode = render_mode_of(render)
        a, t = check_macro_step_args(actions, ticks, self.num_envs, self.num_agents_per_env)
        if isinstance(a, str):
            rc = self._lib.mv_macro_step(self._g, int(k), _P(int(actions.data_ptr())), None if t is None else _P(int(ticks.data_ptr())), mode)
        else:
            rc = self._lib.mv_macro_step_host(self._g, int(k), a.ctypes.data, None if t is None else t.ctypes.data, mode)
        self._ckw(rc)
        self._ring_ticks += 1
        self._fork_held = self._reset_held = self._budget_held = None
        self._store_held = []
        self._seed_held = []
        self._macro_held = (actions, ticks) if isinstance(a, str) else None   # (read in the order of the gym's stream, which need not be torch's current one)

    def fork_envs(self, src_of):
        """Env forks (include/megaverse_hip.h: mv_fork_envs): src_of[d] = s makes env d leave its running episode and continue env s's from s's current
        state; -1 or d leaves env d alone.  Env d keeps its own seed chain and resident next episodes.  A contiguous int32 CUDA tensor of shape (num_envs,) is
        read in place, in the order of the gym's stream, without a host synchronisation (it is held until the next step; an invalid entry is skipped and
        reported by the next stepping call as a warning); a numpy array or a sequence is validated on the host first (RuntimeError, nothing forked).  A
        source may serve many destinations but may not be a destination in the same call."""
        m = check_fork_map(src_of, self.num_envs)
        if isinstance(m, str):
            self._ck(self._lib.mv_fork_envs(self._g, _P(int(src_of.data_ptr()))))
            self._fork_held = src_of
        else:
            self._ck(self._lib.mv_fork_envs_host(self._g, m.ctypes.data))

    def resample_envs(self, src_of):
        """Resampling (include/megaverse_hip.h: mv_resample_envs): env d's new state is the state env src_of[d] had before the call, for any map -- chains,
        swaps, cycles, a source that is overwritten itself; -1 or d leaves env d alone.  Every env keeps its own seed chain and resident next episodes.  The
        argument is fork_envs': a contiguous int32 CUDA tensor of shape (num_envs,) is read in place, in the order of the gym's stream, without a host
        synchronisation (it is held until the next step; an index out of range is skipped and reported by the next stepping call as a warning); a numpy
        array or a sequence is validated on the host first (RuntimeError, nothing copied)."""
        m = check_fork_map(src_of, self.num_envs)
        if isinstance(m, str):
            self._ck(self._lib.mv_resample_envs(self._g, _P(int(src_of.data_ptr()))))
            held = self._fork_held if isinstance(self._fork_held, list) else [self._fork_held]
            held.append(src_of)   # (calls may follow each other without a step: every map is kept)
            self._fork_held = held
        else:
            self._ck(self._lib.mv_resample_envs_host(self._g, m.ctypes.data))

    # ---- env stores (include/megaverse_hip.h: mv_save_envs / mv_load_envs) ----
    def env_record_bytes(self):
        """bytes of one record of an env store: a multiple of 16"""
        return int(self._ck(self._lib.mv_env_record_bytes(self._g)))

    def env_record_layout(self):
        """the layout word of this gym's records: two gyms with the same word can exchange records"""
        return int(self._lib.mv_env_record_layout(self._g))

    def new_env_store(self, slots):
        """a zeroed store of `slots` records on the gym's device: a torch.uint8 tensor [slots, env_record_bytes()].  The caller owns it."""
        import torch
        if int(slots) < 1:
            raise ValueError(f'new_env_store: slots must be positive, got {slots}')
        return torch.zeros((int(slots), self.env_record_bytes()), dtype=torch.uint8, device=f'cuda:{self.device}')

    def _env_store_call(self, who, meaning, device_form, host_form, slot_of, store):
        slots = check_env_store(store, self.env_record_bytes(), who)
        m = check_fork_map(slot_of, self.num_envs, who, meaning)
        if isinstance(m, str):
            self._ck(device_form(self._g, _P(int(slot_of.data_ptr())), _P(int(store.data_ptr())), slots))
            self._store_held.append(slot_of)
        else:
            self._ck(host_form(self._g, m.ctypes.data, _P(int(store.data_ptr())), slots))
        self._store_held.append(store)

    def save_envs(self, slot_of, store):
        """Env stores (include/megaverse_hip.h: mv_save_envs): slot_of[e] = m writes env e's current episode state into record m of store, a contiguous
        torch.uint8 CUDA tensor [slots, env_record_bytes()] (new_env_store); -1: env e is not saved.  Nothing in the gym changes.  The map takes
        fork_envs' rule: a contiguous int32 CUDA tensor of shape (num_envs,) is read in place, in the order of the gym's stream, without a host
        synchronisation (an invalid entry -- out of range, or a slot that two envs name -- is skipped and reported by the next stepping call as a warning);
        a numpy array or a sequence is validated on the host first (RuntimeError, nothing copied).  Map and store are held until the next step."""
        self._env_store_call('save_envs', 'slot_of[e] = the record env e is saved into, -1: not saved', self._lib.mv_save_envs, self._lib.mv_save_envs_host,
                             slot_of, store)

    def load_envs(self, slot_of, store):
        """Env stores (include/megaverse_hip.h: mv_load_envs): slot_of[d] = m makes env d leave its running episode and continue record m's; -1 leaves env d
        alone; many envs may load one record.  Env d keeps its own seed chain and resident next episodes, as a fork destination does.  A record that this
        gym's configuration did not write -- a zeroed slot, another scenario or parameter set -- is skipped, the env stays as it was, and the next stepping
        call reports it as a warning (in both forms: record headers are visible on the device only).  The arguments are save_envs'."""
        self._env_store_call('load_envs', 'slot_of[d] = the record env d continues from, -1: left alone', self._lib.mv_load_envs, self._lib.mv_load_envs_host,
                             slot_of, store)

    def resample_staging_bytes(self):
        """bytes of resample_envs' staging arena: 0 before the first call"""
        return int(self._lib.mv_resample_staging_bytes(self._g))

    def reset_envs(self, mask, render=True):
        """Masked resets (include/megaverse_hip.h: mv_reset_envs): every env whose mask entry is set abandons its running episode and takes the next episode
        of its own sequence; the others are untouched.  A contiguous torch.bool / uint8 CUDA tensor of shape (num_envs,) is read in place, in the order of
        the gym's stream, without a host synchronisation (it is held until the next step); a numpy array or a sequence of bools goes through the host form,
        which makes sure every flagged env has an episode resident.  render: draw the observations behind the reset, where step() leaves them."""
        m = check_reset_mask(mask, self.num_envs)
        if isinstance(m, str):
            self._ckw(self._lib.mv_reset_envs(self._g, _P(int(mask.data_ptr())), int(bool(render))))
            self._reset_held = mask
        else:
            self._ckw(self._lib.mv_reset_envs_host(self._g, m.ctypes.data, int(bool(render))))

    def episodes_drawn_on_device(self):
        """True for TowerBuilding, whose episode generators live on the device (the gyms that take seed_envs' device form); every other scenario's live
        in the host's episode feeder"""
        return self.scenario.casefold() == "towerbuilding"

    def seed_envs(self, seeds):
        """Level seeds (include/megaverse_hip.h: mv_seed_envs): env e restarts its episode stream from seeds[e] -- Env::seed, the value seed() hands an env
        from its master stream (megaverse_amd.distributed.env_seeds lists them).  Its running episode goes on; its NEXT reset -- an auto-reset, reset(),
        reset_envs -- plays the first episode of the new stream.  seeds: num_envs ints (negative or None: the env is left alone), a dict {env: seed}, or
        a contiguous int32 CUDA tensor of shape (num_envs,), which is read in place in the order of the gym's stream without a host synchronisation
        (TowerBuilding only: every other scenario's generators live on the host and take the host forms, which wait for the device)."""
        m = check_env_seeds(seeds, self.num_envs)
        if isinstance(m, str):
            self._ck(self._lib.mv_seed_envs(self._g, _P(int(seeds.data_ptr()))))
            self._seed_held.append(seeds)
        else:
            self._ckw(self._lib.mv_seed_envs_host(self._g, m.ctypes.data))

    STEP_MASK_FORMS = ("none", "device", "host")

    def _set_env_mask(self, check, set_fn, set_host_fn, held_attr, mask):
        """set_step_mask / set_draw_mask: None detaches, a CUDA tensor is attached in place and held, anything else goes through the host form.  set_fn,
        set_host_fn: the library calls' names (the library is not touched before the mask has passed its check)"""
        m = check(mask, self.num_envs)
        if isinstance(m, str):
            self._ck(getattr(self._lib, set_fn)(self._g, _P(int(mask.data_ptr()))))
        elif m is None:
            self._ck(getattr(self._lib, set_fn)(self._g, None))
        else:
            self._ck(getattr(self._lib, set_host_fn)(self._g, m.ctypes.data))
        setattr(self, held_attr, mask if isinstance(m, str) else None)

    def set_step_mask(self, mask):
        """Step masks (include/megaverse_hip.h: mv_set_step_mask): mask[e] non-zero: env e steps; 0: env e is frozen -- every tick of every later stepping
        call leaves its state alone, reports reward 0 and done 0 for it and discards its actions -- until the mask is replaced or detached (None).  A
        contiguous torch.bool / uint8 CUDA tensor of shape (num_envs,) is read in place by the step kernels (the gym holds a reference; after rewriting it,
        call this again); a numpy array or a sequence of bools is copied to a buffer of the gym's.  Neither form waits on the host."""
        self._set_env_mask(check_step_mask, 'mv_set_step_mask', 'mv_set_step_mask_host', '_step_mask_held', mask)

    def step_mask(self):
        """-> 'none' | 'device' | 'host': the form of the step mask attached (set_step_mask)"""
        return self.STEP_MASK_FORMS[self._ck(self._lib.mv_get_step_mask(self._g))]

    def set_draw_mask(self, mask):
        """Draw masks (include/megaverse_hip.h: mv_set_draw_mask): mask[e] non-zero: env e is drawn as always; 0: none of env e's frames is set up or drawn
        by any later observation pass -- step, step_n in every render mode, the frame behind reset and reset_envs(render=True), render -- and no byte of
        their rows in the observation slab or ring is written: the rows keep what they held.  Physics, rewards, dones and the episode log are those of a
        drawn env.  Until the mask is replaced or detached (None).  A contiguous torch.bool / uint8 CUDA tensor of shape (num_envs,) is read in place (the gym
        holds a reference; after rewriting it, call this again); a numpy array or a sequence of bools is copied to a buffer of the gym's.  Neither form
        waits on the host.  draw_hires ignores the mask."""
        self._set_env_mask(check_draw_mask, 'mv_set_draw_mask', 'mv_set_draw_mask_host', '_draw_mask_held', mask)

    def draw_mask(self):
        """-> 'none' | 'device' | 'host': the form of the draw mask attached (set_draw_mask)"""
        return self.STEP_MASK_FORMS[self._ck(self._lib.mv_get_draw_mask(self._g))]

    def set_still_frames(self, on=True):
        """Still frames (include/megaverse_hip.h: mv_set_still_frames): while on, every later observation pass of step, step_n (every render mode) and
        macro_step sets up and draws an env's frames only where the env's state may have changed since they were drawn last -- an env frozen by a step mask,
        halted by its budget or stopped inside a macro step is not ray-cast again.  Its rows show the frame drawn last: in the observation slab they are left
        alone, in an output ring they are copied on the device from the entry that holds it.  Every observation byte, reward, done and log record equals
        those of a gym with the option off.  reset, reset_envs, fork_envs, resample_envs, load_envs, seed, render and the setters that change what or where
        the gym draws make every env due again.  Never waits on the host; draw_hires ignores it; groups refuse a gym that has it on."""
        self._ck(self._lib.mv_set_still_frames(self._g, 1 if on else 0))

    def still_frames(self):
        """-> bool: whether still frames are switched on (set_still_frames)"""
        return self._ck(self._lib.mv_get_still_frames(self._g)) != 0

    def set_state_obs(self, buf=True):
        """State observations (include/megaverse_hip.h: mv_set_state_obs): every tick of every later stepping call -- in every render mode, 'none' included --
        leaves one row of 16 float32 per agent (STATE_OBS_FIELDS: pose, velocities, carrying, episode time, total reward; the state AFTER the tick, bit for
        bit) in entry t % entries of a float32 CUDA tensor [entries, num_envs * num_agents, 16], entries = the output ring's count, or 1 without a ring: the
        entry the tick's rewards go to.  True allocates the tensor on the gym's device and returns it; a tensor is checked (ValueError) and attached; None
        detaches.  Nothing waits on the host; the rows are visible on the gym's stream when the call's rewards are.  While attached, set_output_ring is
        refused."""
        return self._attach_obs('state', buf)

    def _attach_obs(self, name, buf, fmt=None):
        """set_*_obs: attach (True: allocate) or detach (None) the tensor [entries, *tail] of one stream of OBS_STREAMS; fmt: the library's format word of a
        plane stream -> the tensor, or None"""
        s = OBS_STREAMS[name]
        if buf is None:
            self._ck(getattr(self._lib, s.setter)(self._g, None, *s.detach))
            self._obs.pop(name, None)
            return None
        tail, dtypes, who = s.tail(self), s.dtypes(fmt), s.setter[3:]
        if buf is not True:
            _check_obs_tensor(buf, None, tail, dtypes, self.device, who)   # (what needs no gym first: the library stays untouched by a tensor that is wrong anyway)
        entries = max(1, self._ck(self._lib.mv_get_output_ring(self._g)))   # (the library's own count: the depth it will write)
        if buf is True:
            import torch
            buf = torch.zeros((entries,) + tail, dtype=getattr(torch, dtypes[0][6:]), device=f'cuda:{self.device}')
        else:
            _check_obs_tensor(buf, entries, tail, dtypes, self.device, who)
        self._ck(getattr(self._lib, s.setter)(self._g, _P(int(buf.data_ptr())), *(() if fmt is None else (fmt,))))
        self._obs[name] = buf
        return buf

    def _obs_last(self, name):
        """*_obs: the last tick's entry of one stream's attached tensor, or None (ticks stepped by calling the library directly, past this object, are not
        counted)"""
        buf = self._obs.get(name)
        return None if buf is None else buf[(max(1, self._ring_ticks) - 1) % int(buf.shape[0])]

    def _read_obs(self, name, *index):
        """get_*_observation: one row or plane of the last tick's entry through the library's reader -> numpy"""
        s = OBS_STREAMS[name]
        out = np.empty(s.tail(self)[1:], s.read)
        self._ck(getattr(self._lib, s.reader)(self._g, *(int(i) for i in index), out.ctypes.data))
        return out

    def state_obs(self):
        """-> the tensor set_state_obs attached, or None"""
        return self._obs.get('state')

    def set_scene_obs(self, buf=True):
        """Scene observations (include/megaverse_hip.h: mv_set_scene_obs), the per-env counterpart of set_state_obs: every tick of every later stepping call
        leaves one row of 32 float32 per ENV (SCENE_OBS_FIELDS: room, episode time and counter, solved, tower, counts; SCENE_OBS_SCENARIO_FIELDS: the
        building zone, the exit pad and the diamonds left, the hex target, the ball; the state AFTER the tick) in entry t % entries of a float32 CUDA tensor
        [entries, num_envs, 32], entries = the output ring's count, or 1 without a ring.  True allocates the tensor on the gym's device and returns it; a
        tensor is checked (ValueError) and attached; None detaches.  Nothing waits on the host.  While attached, set_output_ring is refused."""
        return self._attach_obs('scene', buf)

    def scene_obs_ring(self):
        """-> the tensor set_scene_obs attached, [entries, num_envs, 32] (entry t % entries: what tick t left), or None"""
        return self._obs.get('scene')

    def scene_obs(self):
        """-> the entry of the last tick, (num_envs, 32): a view of the attached tensor, valid in the order of the gym's stream; None with nothing attached.
        With an output ring: the entry the last tick stepped through this object went to (scene_obs_ring has them all)"""
        return self._obs_last('scene')

    def get_scene_observation(self, env_idx):
        """-> numpy float32 [32]: the last tick's row of one env (waits for the gym's stream)"""
        return self._read_obs('scene', env_idx)

    def entity_rows(self):
        """-> E: the rows per env of the entity observations (mv_entity_obs_rows), fixed for the gym's scenario and agent count"""
        return self._ck(self._lib.mv_entity_obs_rows(self._g))

    def entity_layout(self):
        """-> {group name: slice of rows} as the library states it (mv_entity_obs_layout; megaverse_amd.entity_layout gives the same without a gym)"""
        out = np.zeros((4, 3), np.int32)
        self._ck(self._lib.mv_entity_obs_layout(self._g, out.ctypes.data))
        return {name: slice(int(b), int(b + n)) for name, (b, n, _) in zip(ENTITY_GROUPS, out)}

    def set_entity_obs(self, buf=True):
        """Entity observations (include/megaverse_hip.h: mv_set_entity_obs): the objects themselves.  Every tick of every later stepping call leaves
        entity_rows() rows of 8 float32 per ENV (ENTITY_OBS_FIELDS: the entity's segmentation word, centre, half extents, state; entity_layout: which rows are
        terrain, movable objects, collectables, agents; the state AFTER the tick) in entry t % entries of a float32 CUDA tensor [entries, num_envs, E, 8],
        entries = the output ring's count, or 1 without a ring.  Rows are slot-addressed: a record keeps its row, one that does not exist is all zero, and
        entity_row_of maps the words of an 'instance' label plane (set_seg_obs) to rows.  True allocates the tensor on the gym's device and returns it; a
        tensor is checked (ValueError) and attached; None detaches.  Nothing waits on the host.  While attached, set_output_ring is refused."""
        return self._attach_obs('entity', buf)

    def entity_obs_ring(self):
        """-> the tensor set_entity_obs attached, [entries, num_envs, E, 8] (entry t % entries: what tick t left), or None"""
        return self._obs.get('entity')

    def entity_obs(self):
        """-> the entry of the last tick, (num_envs, E, 8): a view of the attached tensor, valid in the order of the gym's stream; None with nothing attached.
        With an output ring: the entry the last tick stepped through this object went to (entity_obs_ring has them all)"""
        return self._obs_last('entity')

    def get_entity_observation(self, env_idx):
        """-> numpy float32 [E, 8]: the last tick's rows of one env (waits for the gym's stream)"""
        return self._read_obs('entity', env_idx)

    def set_depth_obs(self, buf=True, dtype=None):
        """Depth observations (include/megaverse_hip.h: mv_set_depth_obs): every frame a later observation pass draws -- step, every tick of step_n, the last
        tick of render='last' and of macro_step(render='last'), the frame behind reset and reset_envs(render=True), render -- leaves its per-pixel camera
        depth (planar, world units, 0: no surface; row 0 is the bottom row) in entry t % entries of a CUDA tensor [entries, num_envs * num_agents, H, W] of
        float32 or float16, entries = the output ring's count, or 1 without a ring: the entry the frame goes to.  True allocates the tensor on the gym's
        device and returns it, in dtype (torch.float32, the default, or torch.float16; their names are accepted too); a tensor is checked (ValueError) and
        attached -- its own dtype decides the format; None detaches.  Nothing waits on the host.
        While attached, set_output_ring, set_render_resolution and set_still_frames(True) are refused."""
        if buf is None:
            return self._attach_obs('depth', None)
        if dtype is None:   # (the default: torch.float32, named without importing torch where nothing is allocated)
            dtype = "float32"
        return self._attach_obs('depth', buf, depth_format_of(dtype if buf is True else getattr(buf, 'dtype', dtype)))

    def depth_obs_ring(self):
        """-> the tensor set_depth_obs attached, [entries, num_envs * num_agents, H, W] (entry t % entries: the planes of tick t's frames), or None"""
        return self._obs.get('depth')

    def depth_obs(self):
        """-> the entry of the last tick, (num_envs * num_agents, H, W): a view of the attached tensor, valid in the order of the gym's stream; None with
        nothing attached.  A tick that drew no frame wrote nothing there.  With an output ring: the entry the last tick stepped through this object went to"""
        return self._obs_last('depth')

    def get_depth_observation(self, env_idx, agent_idx):
        """-> numpy float32 [H, W]: the depth plane of one agent in the last tick's entry, float16 widened (waits for the gym's stream)"""
        return self._read_obs('depth', env_idx, agent_idx)

    def set_seg_obs(self, buf=True, fmt="class"):
        """Segmentation observations (include/megaverse_hip.h: mv_set_seg_obs): every frame a later observation pass draws -- the passes set_depth_obs names --
        leaves a per-pixel label of the drawable it shows (0: no surface, exactly where the depth is 0; row 0 is the bottom row) in entry t % entries of a
        CUDA tensor [entries, num_envs * num_agents, H, W], entries = the output ring's count, or 1 without a ring.  fmt 'class': torch.uint8, a value of
        SEG_CLASSES; fmt 'instance': torch.int16 holding the 16-bit word class << 12 | instance (seg_split takes it apart), instance = the index of the
        drawable's record within its class's array.  True allocates the tensor on the gym's device and returns it; a tensor is checked (ValueError) and
        attached -- fmt must name its format; None detaches.  Nothing waits on the host.  Depth and labels attach independently: with both, a fast-mode
        tick still costs ONE launch behind its passes.
        While attached, set_output_ring, set_render_resolution and set_still_frames(True) are refused."""
        return self._attach_obs('seg', buf, None if buf is None else seg_format_of(fmt))

    def seg_obs_ring(self):
        """-> the tensor set_seg_obs attached, [entries, num_envs * num_agents, H, W] (entry t % entries: the planes of tick t's frames), or None"""
        return self._obs.get('seg')

    def seg_obs(self):
        """-> the entry of the last tick, (num_envs * num_agents, H, W): a view of the attached tensor, valid in the order of the gym's stream; None with
        nothing attached.  A tick that drew no frame wrote nothing there.  With an output ring: the entry the last tick stepped through this object went to"""
        return self._obs_last('seg')

    def get_seg_observation(self, env_idx, agent_idx):
        """-> numpy uint16 [H, W]: the label plane of one agent in the last tick's entry, a 'class' plane widened (waits for the gym's stream)"""
        return self._read_obs('seg', env_idx, agent_idx)

    def set_normal_obs(self, buf=True, dtype=None):
        """Normal observations (include/megaverse_hip.h: mv_set_normal_obs): every frame a later observation pass draws -- the passes set_depth_obs names --
        leaves the per-pixel unit surface normal in the viewer's camera frame (x right, y up, z back; (x, y, z, 1) where there is a surface, four zeros
        where the depth is 0; row 0 is the bottom row) in entry t % entries of a CUDA tensor [entries, num_envs * num_agents, H, W, 4] of float16 or int8
        (signed normalised: b / 127; normals_to_float widens either), entries = the output ring's count, or 1 without a ring.  True allocates the tensor on
        the gym's device and returns it, in dtype (torch.float16, the default, or torch.int8; their names are accepted too); a tensor is checked
        (ValueError) and attached -- its own dtype decides the format; None detaches.  Nothing waits on the host.  Depth, labels and normals attach
        independently: with any of them, a fast-mode tick costs ONE launch behind its passes.  Unlike the labels, the normals of a batched call's earlier
        frames do not change when their env begins a new episode inside the call.
        While attached, set_output_ring, set_render_resolution and set_still_frames(True) are refused."""
        if buf is None:
            return self._attach_obs('normal', None)
        if dtype is None:
            dtype = "float16"
        return self._attach_obs('normal', buf, normal_format_of(dtype if buf is True else getattr(buf, 'dtype', dtype)))

    def normal_obs_ring(self):
        """-> the tensor set_normal_obs attached, [entries, num_envs * num_agents, H, W, 4] (entry t % entries: the planes of tick t's frames), or None"""
        return self._obs.get('normal')

    def normal_obs(self):
        """-> the entry of the last tick, (num_envs * num_agents, H, W, 4): a view of the attached tensor, valid in the order of the gym's stream; None with
        nothing attached.  A tick that drew no frame wrote nothing there.  With an output ring: the entry the last tick stepped through this object went to"""
        return self._obs_last('normal')

    def get_normal_observation(self, env_idx, agent_idx):
        """-> numpy float32 [H, W, 4]: the normal plane of one agent in the last tick's entry, widened (waits for the gym's stream)"""
        return self._read_obs('normal', env_idx, agent_idx)

    def get_state_observation(self, env_idx, agent_idx):
        """-> numpy float32 [16]: the last tick's row of one agent (waits for the gym's stream)"""
        return self._read_obs('state', env_idx, agent_idx)

    def set_episode_budget(self, budget):
        """Episode budgets (include/megaverse_hip.h: mv_set_episode_budget): env e may finish budget[e] more episodes (< 0: unlimited) and then HALTS on the
        device -- in the middle of a batched call too -- frozen on the first frame of its next episode: reward 0, done 0, its state untouched.  An int gives
        every env that value; a contiguous torch.int32 CUDA tensor of shape (num_envs,) is read once, in the order of the gym's stream (the gym holds a
        reference until the next stepping call has been enqueued; leave it unchanged until the stream has passed the attach); a numpy array or a
        list is copied through a staging buffer; None detaches.  Attaching again replaces every value.  Neither form waits on the host."""
        b = check_episode_budget(budget, self.num_envs)
        if b is None:
            self._ck(self._lib.mv_set_episode_budget(self._g, None))
        elif isinstance(b, str):
            self._ck(self._lib.mv_set_episode_budget(self._g, _P(int(budget.data_ptr()))))
            self._budget_held = budget   # (the attach kernel reads it in the order of the gym's stream, which need not be torch's current one)
        else:
            self._ck(self._lib.mv_set_episode_budget_host(self._g, b.ctypes.data))

    def has_episode_budget(self):
        return self._ck(self._lib.mv_get_episode_budget(self._g)) == 1

    def episode_budget(self):
        """int32 CUDA tensor [num_envs]: what every env may still finish (0: halted), a view of the gym's memory, valid in the order of the gym's stream
        after any stepping call"""
        import torch
        ptr = int(self._lib.mv_episode_budget_device_ptr(self._g) or 0)
        if not ptr:
            raise RuntimeError("no episode budget attached (set_episode_budget)")
        return torch.as_tensor(_DeviceArray(ptr, (self.num_envs,), "<i4"), device=f"cuda:{self.device}")

    def halted_count_tensor(self):
        """uint32 as an int32 CUDA tensor [1]: the number of halted envs (a view, like episode_budget)"""
        import torch
        ptr = int(self._lib.mv_halted_count_device_ptr(self._g) or 0)
        if not ptr:
            raise RuntimeError("no episode budget attached (set_episode_budget)")
        return torch.as_tensor(_DeviceArray(ptr, (1,), "<i4"), device=f"cuda:{self.device}")

    def halted_count(self):
        """-> the number of halted envs; synchronises the gym's stream"""
        out = _I()
        self._ck(self._lib.mv_halted_count(self._g, C.byref(out)))
        return int(out.value)

    def set_action_ring(self, count, device_ptr=0):
        """int32 [count, num_agents, 6] multi-discrete actions in device memory for step_n(..., 'sequence') (include/megaverse_hip.h: mv_set_action_ring);
        count = 0 detaches.  Nothing is launched or copied: the step kernels read the caller's buffer, which the caller keeps alive.  The call orders what
        the gym's stream holds so far -- the kernel that filled the ring -- before the next step; after rewriting entries, call it again."""
        self._ck(self._lib.mv_set_action_ring(self._g, int(count), _P(int(device_ptr) or None)))

    def debug_launch_counts(self):
        """-> (step launches, observation launches) the stepping calls have enqueued for this gym -- in a group: for the group -- so far (a test hook)"""
        out = (C.c_int64 * 2)()
        self._ck(self._lib.mv_debug_launch_counts(self._g, out))
        return int(out[0]), int(out[1])

    def set_sample_policy(self, policy):
        """'multidiscrete' (action_space.sample()) or 'single-bit' (the reference's megaverse_test_app policy) for sample_random_actions"""
        self._ck(self._lib.mv_set_sample_policy(self._g, int(self.POLICIES.get(policy, policy))))

    def set_output_ring(self, count, obs_ptr=0, rewards_ptr=0, dones_ptr=0):
        """tick t leaves its outputs in entry t % count of the given device rings (0 = keep that output in its single array)"""
        self._ck(self._lib.mv_set_output_ring(self._g, int(count), _P(int(obs_ptr) or None), _P(int(rewards_ptr) or None), _P(int(dones_ptr) or None)))
        self._ring_ticks = 0

    def set_pass_overlap(self, on=True):
        """with a ring at least two calls deep, the observation passes of consecutive step_n calls overlap (include/megaverse_hip.h: mv_set_pass_overlap);
        an entry must then be consumed before the next stepping call after the one that produced it"""
        self._ck(self._lib.mv_set_pass_overlap(self._g, int(bool(on))))

    def recommended_ticks_per_call(self):
        """the k to ask step_n for (the measured rules of include/megaverse_hip.h: 16 for 1024..2047 frames per tick, else 8; 1 for few-tick episodes)"""
        return int(self._lib.mv_recommended_ticks_per_call(self._g))

    def recommended_pass_overlap(self):
        return bool(self._lib.mv_recommended_pass_overlap(self._g))

    def host_generator_threads(self):
        """threads of the host-side episode feeder; 0 = the episodes are drawn on the device (TowerBuilding; Collect with the device generator)"""
        return int(self._lib.mv_host_generator_threads(self._g))

    def device_generator(self):
        """are the episodes drawn on the device?  True: TowerBuilding; Collect with the device generator; the Obstacles family and Empty with
        MV_OBSTACLES_DEVICE_GEN=1 in the environment when the gym was made.  host_generator_threads() is 0 exactly then."""
        return int(self._lib.mv_device_generator(self._g)) == 1

    def arena_bytes(self):
        return int(self._lib.mv_arena_bytes(self._g))

    # ---- episode log (include/megaverse_hip.h: mv_set_episode_log; no reference counterpart) ----
    def set_episode_log(self, capacity):
        """capacity > 0: per-agent returns and per-env lengths are summed on the device and every finished env appends one record per agent to a device
        buffer of `capacity` records, in (end_tick, agent) order; 0: off"""
        self._ck(self._lib.mv_set_episode_log(self._g, int(capacity)))

    def episode_log_capacity(self):
        return int(self._lib.mv_get_episode_log_capacity(self._g))

    def flush_episode_log(self):
        self._ck(self._lib.mv_flush_episode_log(self._g))

    def episode_log_count(self):
        """-> (records in the buffer, records dropped since the log was switched on); synchronises the gym's stream"""
        count, dropped = _U(), _U()
        self._ck(self._lib.mv_episode_log_count(self._g, C.byref(count), C.byref(dropped)))
        return int(count.value), int(dropped.value)

    def drain_episode_log(self, max_records=None):
        """the oldest max_records (default: all) records as a numpy array of EPISODE_RECORD_DTYPE, removed from the device buffer; synchronises the gym's
        stream.  self.episode_log_dropped: the records lost to a full buffer since the log was switched on."""
        if max_records is None:
            max_records = self.episode_log_capacity()
        out = np.zeros(max(int(max_records), 0), EPISODE_RECORD_DTYPE)
        dropped = _U()
        n = self._ck(self._lib.mv_drain_episode_log(self._g, out.ctypes.data if out.size else None, out.size, C.byref(dropped)))
        self.episode_log_dropped = int(dropped.value)
        return out[:n]

    def ticks_since_reset(self):
        return int(self._lib.mv_ticks_since_reset(self._g))

    def episode_returns_device_ptr(self):
        return int(self._lib.mv_episode_returns_device_ptr(self._g) or 0)

    def episode_lengths_device_ptr(self):
        return int(self._lib.mv_episode_lengths_device_ptr(self._g) or 0)

    def episode_log_records_device_ptr(self):
        return int(self._lib.mv_episode_log_records_device_ptr(self._g) or 0)

    def episode_log_count_device_ptr(self):
        return int(self._lib.mv_episode_log_count_device_ptr(self._g) or 0)

    def episode_returns_tensor(self):
        """float64 CUDA tensor [num_envs * num_agents_per_env]: the running returns, a view of the gym's memory (valid in the order of the gym's stream,
        until set_episode_log / close)"""
        import torch
        if not self.episode_returns_device_ptr():
            raise RuntimeError("the episode log is off (set_episode_log)")
        return torch.as_tensor(_DeviceArray(self.episode_returns_device_ptr(), (self.num_envs * self.num_agents_per_env,), "<f8"), device=f"cuda:{self.device}")

    def episode_lengths_tensor(self):
        """int32 CUDA tensor [num_envs]: the running episode lengths in ticks (a view, like episode_returns_tensor)"""
        import torch
        if not self.episode_lengths_device_ptr():
            raise RuntimeError("the episode log is off (set_episode_log)")
        return torch.as_tensor(_DeviceArray(self.episode_lengths_device_ptr(), (self.num_envs,), "<i4"), device=f"cuda:{self.device}")

    def render(self):
        self._ck(self._lib.mv_render(self._g))

    def synchronize(self):
        self._ck(self._lib.mv_synchronize(self._g))

    def get_dones(self):
        out = np.empty(self.num_envs, np.uint8)
        self._ck(self._lib.mv_get_dones(self._g, out.ctypes.data))
        return out

    def get_rewards_array(self):
        out = np.empty(self.num_envs * self.num_agents_per_env, np.float32)
        self._ck(self._lib.mv_get_last_rewards(self._g, out.ctypes.data))
        return out

    def get_true_objectives(self):
        out = np.empty(self.num_envs * self.num_agents_per_env, np.float32)
        self._ck(self._lib.mv_get_true_objectives(self._g, out.ctypes.data))
        return out

    def obs_device_ptr(self):
        return int(self._lib.mv_obs_device_ptr(self._g) or 0)

    def rewards_device_ptr(self):
        return int(self._lib.mv_rewards_device_ptr(self._g) or 0)

    def dones_device_ptr(self):
        return int(self._lib.mv_dones_device_ptr(self._g) or 0)

    def true_objectives_device_ptr(self):
        return int(self._lib.mv_true_objectives_device_ptr(self._g) or 0)

    def set_obs_buffer(self, device_ptr):
        self._ck(self._lib.mv_set_obs_buffer(self._g, _P(int(device_ptr))))

    def set_pixel_mode(self, mode):
        """'fast' (default: hardware rcp/rsqrt, pixels within DESIGN.md's tolerance) or 'exact' (bit-identical to the oracle)"""
        m = {"exact": 0, "fast": 1}.get(mode, mode)
        self._ck(self._lib.mv_set_pixel_mode(self._g, int(m)))

    def pixel_mode(self):
        return "fast" if self._lib.mv_get_pixel_mode(self._g) == 1 else "exact"

    def set_obs_layout(self, layout):
        """the observation slab's layout (include/megaverse_hip.h: mv_set_obs_layout): 'rgba' ([N*A][h][w][4], the default) or 'chw' ([N*A][3][h][w]
        uint8, planes R, G, B, written so by the observation pass); before the gym's first reset / render / set_obs_buffer / set_output_ring"""
        if isinstance(layout, str):
            if layout not in ("rgba", "chw"):
                raise ValueError(f"set_obs_layout: {layout!r}: the layouts are 'rgba' and 'chw'")
            layout = 0 if layout == "rgba" else 1
        self._ck(self._lib.mv_set_obs_layout(self._g, int(layout)))

    def obs_layout(self):
        return "chw" if self._lib.mv_get_obs_layout(self._g) == 1 else "rgba"

    def set_pipelining(self, on):
        """one-step-ahead pipelining of the step kernels against the observation pass (include/megaverse_hip.h); on by default"""
        self._ck(self._lib.mv_set_pipelining(self._g, 1 if on else 0))

    def pipelining(self):
        return self._lib.mv_get_pipelining(self._g) == 1

    def set_stream(self, hip_stream):
        self._ck(self._lib.mv_set_stream(self._g, _P(int(hip_stream))))

    def profile_begin(self, max_steps):
        self._ck(self._lib.mv_profile_begin(self._g, int(max_steps)))

    def profile_end(self):
        """-> {'step': (avg_ms, n), 'reset': (...), 'setup': (...), 'raster': (...)} measured with HIP events on the gym's stream"""
        ms = (C.c_float * 4)()
        cnt = (C.c_int32 * 4)()
        self._ck(self._lib.mv_profile_end(self._g, ms, cnt))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(("step", "reset", "setup", "raster"))}

    def debug_set_agent_pos(self, env_idx, agent_idx, x, y, z):
        self._ck(self._lib.mv_debug_set_agent_pos(self._g, int(env_idx), int(agent_idx), float(x), float(y), float(z)))

    def debug_set_agent_yaw(self, env_idx, agent_idx, c, s):
        self._ck(self._lib.mv_debug_set_agent_yaw(self._g, int(env_idx), int(agent_idx), float(c), float(s)))

    def debug_set_agent_velocity(self, env_idx, agent_idx, hvx, hvz, vvel):
        self._ck(self._lib.mv_debug_set_agent_velocity(self._g, int(env_idx), int(agent_idx), float(hvx), float(hvz), float(vvel)))

    def debug_set_agent_pitch(self, env_idx, agent_idx, pitch):
        self._ck(self._lib.mv_debug_set_agent_pitch(self._g, int(env_idx), int(agent_idx), float(pitch)))

    def debug_set_objects(self, env_idx, objects):
        """TowerBuilding: env env_idx's movable boxes, int8 [n, 4] rows (x, y, z, state: 0 placed, 1 + k carried by agent k), n <= 80 -- records, count,
        the chunk's object bits, every agent's `carrying` and bz_reward follow (include/megaverse_hip.h: mv_debug_set_objects)"""
        o = np.ascontiguousarray(objects, dtype=np.int8).reshape(-1, 4)
        self._ck(self._lib.mv_debug_set_objects(self._g, int(env_idx), o.ctypes.data, len(o)))

    def debug_boxagone_state(self, env_idx):
        """BoxAGone: env env_idx's BoxAGoneState (mv_types.h) as raw bytes -- platform table, temporary ring, timers, cell map."""
        n = self._lib.mv_debug_boxagone_state(self._g, int(env_idx), None)
        self._ck(n)
        buf = np.zeros(n, np.uint8)
        self._ck(self._lib.mv_debug_boxagone_state(self._g, int(env_idx), buf.ctypes.data))
        return buf

    def debug_football_state(self, env_idx):
        """Football: env env_idx's ball as a dict of numpy values (FootballState, mv_types.h): pos, radius (drawn), vel, kicks, ang, contacts, force."""
        n = self._lib.mv_debug_football_state(self._g, int(env_idx), None)
        self._ck(n)
        buf = np.zeros(n, np.uint8)
        self._ck(self._lib.mv_debug_football_state(self._g, int(env_idx), buf.ctypes.data))
        f, i = buf.view(np.float32), buf.view(np.int32)
        return {"pos": f[0:3].copy(), "radius": f[3], "vel": f[4:7].copy(), "kicks": int(i[7]), "ang": f[8:11].copy(), "contacts": int(i[11]),
                "force": f[12:15].copy()}

    def debug_set_football_state(self, env_idx, pos, vel=(0.0, 0.0, 0.0), ang=(0.0, 0.0, 0.0), force=(0.0, 0.0, 0.0), radius=1.0):
        """Football: place env env_idx's ball -- centre, velocity, angular velocity, the force pending for the next tick, drawn radius."""
        buf = np.zeros(16, np.float32)
        buf[0:3], buf[3], buf[4:7], buf[8:11], buf[12:15] = pos, radius, vel, ang, force
        self._ck(self._lib.mv_debug_set_football_state(self._g, int(env_idx), buf.ctypes.data))

    def fork_bytes_per_env(self):
        """bytes a fork copies per destination env: the size of an env's episode state"""
        return int(self._lib.mv_fork_bytes_per_env(self._g))

    def debug_episodes_consumed(self):
        """int32 [num_envs]: the episodes of its own sequence every env has taken so far (a test hook; synchronises)"""
        out = np.zeros(self.num_envs, np.int32)
        self._ck(self._lib.mv_debug_episodes_consumed(self._g, out.ctypes.data))
        return out

    def debug_snapshot_bytes(self, env_idx):
        n = self._lib.mv_debug_snapshot_size(self._g)
        buf = np.zeros(n, np.uint8)
        self._ck(self._lib.mv_debug_snapshot(self._g, int(env_idx), buf.ctypes.data))
        return buf
