"""State observations, restated for the tests: the two structs of megaverse_amd/csrc/mv_types.h the record reads, as numpy dtypes, and the record's table
(include/megaverse_hip.h: mv_set_state_obs) applied to a debug snapshot -- the oracle's or the gym's, they share a layout (oracle_lib.SNAP)."""
import numpy as np

F = {name: i for i, name in enumerate(("pos_x", "pos_y", "pos_z", "m00", "m02", "m20", "m22", "pitch", "hvx", "hvz", "vvel", "carrying", "episode_sec",
                                       "episode_len", "total_reward", "reserved"))}

# struct AgentState, 128 bytes
AGENT_STATE = np.dtype([
    ("pos", "<f4", 3), ("m00", "<f4"), ("m02", "<f4"), ("m20", "<f4"), ("m22", "<f4"), ("pitch", "<f4"), ("hvx", "<f4"), ("hvz", "<f4"), ("vvel", "<f4"),
    ("voffset", "<f4"), ("step_offset", "<f4"), ("jump_speed", "<f4"), ("was_jumping", "<i4"), ("carrying", "<i4"), ("picked_up", "<i4"),
    ("visited_zone", "<i4"), ("spawn", "<i4", 3), ("last_reward", "<f4"), ("total_reward", "<f4"), ("shaping", "<f4", 8), ("pad", "<i4", 1),
])
# struct EnvHeader, 128 bytes
ENV_HEADER = np.dtype([
    ("L", "<i4"), ("H", "<i4"), ("W", "<i4"), ("bz", "<i4", 4), ("layout_color", "<i4"), ("wall_color", "<i4"), ("draw_walls", "<i4"),
    ("num_objects", "<i4"), ("num_boxes", "<i4"), ("num_frames", "<i4"), ("done", "<i4"), ("highest_tower", "<i4"), ("episode_sec", "<f4"),
    ("episode_len", "<f4"), ("bz_reward", "<f4"), ("bar_half_width", "<f4"), ("next_seed", "<u4"), ("seed_is_env_seed", "<i4"),
    ("p_episode_len_sec", "<f4"), ("p_vertical_look_limit", "<f4"), ("scenario", "<i4"), ("num_terrain", "<i4"), ("num_rewards", "<i4"),
    ("num_platforms", "<i4"), ("solved", "<i4"), ("episodes_consumed", "<i4"), ("starved", "<i4"), ("hex_target", "<f4", 2),
])
assert AGENT_STATE.itemsize == 128 and ENV_HEADER.itemsize == 128


def struct_images(snap, a):
    """-> (AgentState, EnvHeader) records holding what a snapshot says about agent a and its env (what it does not say stays zero)"""
    sa = snap["agents"][a]
    agent, header = np.zeros(1, AGENT_STATE), np.zeros(1, ENV_HEADER)
    agent["pos"] = sa["pos"]
    for k, name in enumerate(("m00", "m02", "m20", "m22")):
        agent[name] = sa["basis"][k]
    agent["hvx"], agent["hvz"] = sa["hv"][0], sa["hv"][1]
    for name in ("pitch", "vvel", "voffset", "step_offset", "jump_speed", "was_jumping", "carrying", "picked_up", "visited_zone", "spawn", "last_reward",
                 "total_reward", "shaping"):
        agent[name] = sa[name]
    for name in ("L", "H", "W", "bz", "layout_color", "wall_color", "draw_walls", "num_objects", "num_boxes", "num_frames", "done", "highest_tower",
                 "episode_sec", "episode_len", "bz_reward", "bar_half_width", "scenario", "num_terrain", "num_rewards", "num_platforms", "solved"):
        header[name] = snap[name]
    return agent, header


def rows_of_snapshot(snap, A):
    """the table applied to one env's snapshot -> uint32 [A, 16]: every copied column is the snapshot field's own 32 bits"""
    out = np.zeros((A, 16), np.uint32)
    bits = lambda x: np.asarray(x, "<f4").reshape(-1).view(np.uint32)   # noqa: E731
    for a in range(A):
        sa = snap["agents"][a]
        out[a, 0:3] = bits(sa["pos"])
        out[a, 3:7] = bits(sa["basis"])
        out[a, 7] = bits(sa["pitch"])[0]
        out[a, 8:10] = bits(sa["hv"])
        out[a, 10] = bits(sa["vvel"])[0]
        out[a, 11] = 0x3f800000 if int(sa["carrying"]) >= 0 else 0
        out[a, 12] = bits(snap["episode_sec"])[0]
        out[a, 13] = bits(snap["episode_len"])[0]
        out[a, 14] = bits(sa["total_reward"])[0]
        out[a, 15] = 0
    return out


def rows_of_gym_snapshots(snapshot_of, N, A):
    """-> uint32 [N * A, 16] from snapshot_of(env) for every env"""
    return np.concatenate([rows_of_snapshot(snapshot_of(e), A) for e in range(N)], axis=0)
