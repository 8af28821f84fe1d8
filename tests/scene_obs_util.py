"""Scene observations, restated for the tests: the record's table (include/megaverse_hip.h: mv_set_scene_obs; megaverse_amd/csrc/mv_scene_obs.h) in numpy,
applied to a debug snapshot -- the oracle's or the gym's, they share a layout (oracle_lib.SNAP) -- and, for Football, to the football_model.STATE record both
sides expose.  Column 0 comes from the name -> SCN_* table below (restated from mv_types.h), column 7 from mv_debug_episodes_consumed."""
import numpy as np

import football_model
from state_obs_util import ENV_HEADER

FLOATS = 32
# mv_types.h: SCN_*
SCN = {"TowerBuilding": 0, "ObstaclesEasy": 1, "ObstaclesMedium": 1, "ObstaclesHard": 1, "ObstaclesWalls": 1, "ObstaclesSteps": 1, "ObstaclesLava": 1,
       "Collect": 2, "Rearrange": 3, "Sokoban": 4, "Empty": 5, "HexMemory": 6, "HexExplore": 7, "BoxAGone": 8, "Football": 9}
SCN_TOWER, SCN_OBSTACLES, SCN_HEX_EXPLORE, SCN_FOOTBALL = 0, 1, 7, 9
TERRAIN_EXIT, TERRAIN_LAVA = 1, 2
TERRAIN_BOX = np.dtype([("min", "<i4", 3), ("type", "<i4"), ("max", "<i4", 3), ("pad", "<i4")])
MOVABLE = np.dtype([("x", "i1"), ("y", "i1"), ("z", "i1"), ("state", "i1")])
assert TERRAIN_BOX.itemsize == 32 and MOVABLE.itemsize == 4

F = {name: i for i, name in enumerate(("scenario", "room_l", "room_h", "room_w", "num_frames", "episode_sec", "episode_len", "episodes_consumed", "solved",
                                       "highest_tower", "bz_reward", "num_objects", "num_rewards", "num_platforms", "num_terrain", "reserved"))}
NUM_EXITS, EXIT_MIN, EXIT_MAX, DIAMONDS = 16, 17, 20, 23
BALL_POS, BALL_RADIUS, KICKS, CONTACTS = 16, 19, 23, 27


def copied(x):
    """the 32 bits of float32 values"""
    return np.asarray(x, "<f4").reshape(-1).view(np.uint32)


def of_int(x):
    """int32 values converted with (float): the bits of the float32"""
    return np.asarray(x, np.int64).astype(np.float32).reshape(-1).view(np.uint32)


def row(scenario, hdr, consumed, terrain=None, rewards=None, hex_target=None, ball=None):
    """the table -> uint32 [32].  scenario: SCN_*; hdr: anything indexable by the header's field names (a snapshot, an ENV_HEADER record); consumed: column
    7's int; terrain int32 [16, 8] in TerrainBox's order; rewards int8 [n, 4]; hex_target: (x, z) float32; ball: a football_model.STATE record"""
    out = np.zeros(FLOATS, np.uint32)
    out[0] = of_int(scenario)[0]
    out[1:4] = of_int([hdr["L"], hdr["H"], hdr["W"]])
    out[4] = of_int(hdr["num_frames"])[0]
    out[5], out[6] = copied(hdr["episode_sec"])[0], copied(hdr["episode_len"])[0]
    out[7] = of_int(consumed)[0]
    out[8], out[9] = of_int(hdr["solved"])[0], of_int(hdr["highest_tower"])[0]
    out[10] = copied(hdr["bz_reward"])[0]
    out[11:15] = of_int([hdr["num_objects"], hdr["num_rewards"], hdr["num_platforms"], hdr["num_terrain"]])
    if scenario == SCN_TOWER:
        out[16:20] = of_int(hdr["bz"])
    elif scenario == SCN_OBSTACLES:
        t = np.asarray(terrain, np.int32).reshape(-1, 8)[:int(hdr["num_terrain"])]
        exits = [i for i in range(len(t)) if t[i, 3] & TERRAIN_EXIT]
        out[NUM_EXITS] = of_int(len(exits))[0]
        if exits:
            out[17:20], out[20:23] = of_int(t[exits[0], 0:3]), of_int(t[exits[0], 4:7])
        r = np.asarray(rewards, np.int8).reshape(-1, 4)[:int(hdr["num_rewards"])]
        out[DIAMONDS] = of_int(int((r[:, 3] != 0).sum()))[0]
    elif scenario == SCN_HEX_EXPLORE:
        out[16:18] = copied(hex_target)
    elif scenario == SCN_FOOTBALL:
        out[16:19], out[19], out[20:23] = copied(ball["pos"]), copied(ball["radius"])[0], copied(ball["vel"])
        out[23] = of_int(ball["kicks"])[0]
        out[24:27] = copied(ball["ang"])
        out[27] = of_int(ball["contacts"])[0]
        out[28:31] = copied(ball["force"])
    return out


def terrain_boxes(snap):
    """a snapshot's terrain rows (min[3], max[3], type, 0) in TerrainBox's order (min[3], type, max[3], pad) -> int32 [16, 8]"""
    t = np.asarray(snap["terrain"], np.int32)
    return np.concatenate([t[:, 0:3], t[:, 6:7], t[:, 3:6], t[:, 7:8]], axis=1)


HEX_LISTS = ("HexMemory", "HexExplore", "BoxAGone", "Football")   # the scenarios whose boxes and collectables are HexRec lists (GymView::hex_boxes, hex_objs)


def header_of_snapshot(name, snap):
    """the header fields the record reads, as EnvHeader holds them.  A snapshot reports three of them under other names (mv_api_debug.hip): with HexRec lists
    the header's num_rewards counts the collectables (hex_num_objs) and its num_terrain the colliding boxes, which come first in the list (meta bit 4);
    Rearrange keeps its item count in num_terrain (num_items)"""
    h = {k: snap[k] for k in ("L", "H", "W", "bz", "num_frames", "episode_sec", "episode_len", "solved", "highest_tower", "bz_reward", "num_objects",
                              "num_rewards", "num_platforms", "num_terrain")}
    if name in HEX_LISTS:
        h["num_rewards"] = snap["hex_num_objs"]
        h["num_terrain"] = int(((np.asarray(snap["hex_boxes"]["meta"][:int(snap["hex_num_boxes"])]) >> 4) & 1).sum())
    if name == "Rearrange":
        h["num_terrain"] = snap["num_items"]
    return h


def row_of_snapshot(name, snap, consumed, ball=None):
    """the table applied to one env's debug snapshot (SNAP.hex_target is x, y, z: the record's two words are x and z)"""
    return row(SCN[name], header_of_snapshot(name, snap), consumed, terrain=terrain_boxes(snap), rewards=snap["rewards"],
               hex_target=np.asarray(snap["hex_target"])[[0, 2]], ball=ball)


def rows_of(name, snapshot_of, consumed, n, ball_of=None):
    """-> uint32 [n, 32] from snapshot_of(env), consumed[env] and, Football, ball_of(env)"""
    return np.stack([row_of_snapshot(name, snapshot_of(e), consumed[e], ball_of(e) if name == "Football" else None) for e in range(n)])


def header_record(**fields):
    """an ENV_HEADER record (128 bytes) with the given fields"""
    h = np.zeros(1, ENV_HEADER)
    for k, v in fields.items():
        h[k] = v
    return h[0]


assert football_model.STATE.itemsize == 64
