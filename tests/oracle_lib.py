"""ctypes binding of the CPU oracle (oracle/libmv_oracle.so).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")

MAX_BOXES, MAX_OBJECTS, MAX_AGENTS, CHUNK = 1024, 80, 8, 32 * 16 * 32
MAX_TERRAIN, MAX_REWARDS, MAX_SHAPING, HM_DIM = 16, 96, 8, 42
EXPLAIN_MAX = 64   # MVO_EXPLAIN_MAX: candidate colours kept per pixel by mvo_explain_f64

SNAP_AGENT = np.dtype([
    ("pos", "<f4", 3), ("basis", "<f4", 4), ("pitch", "<f4"), ("hv", "<f4", 2), ("vvel", "<f4"), ("voffset", "<f4"),
    ("step_offset", "<f4"), ("jump_speed", "<f4"), ("was_jumping", "<i4"), ("carrying", "<i4"), ("picked_up", "<i4"),
    ("visited_zone", "<i4"), ("spawn", "<i4", 3), ("last_reward", "<f4"), ("total_reward", "<f4"), ("shaping", "<f4", MAX_SHAPING),
])
HEX_MAX_BOXES, HEX_MAX_OBJS = 2048, 128
HEX_REC = np.dtype([("a", "<f4", 3), ("meta", "<i4"), ("b", "<f4", 3), ("color", "<i4")])
SNAP = np.dtype([
    ("scenario", "<i4"), ("L", "<i4"), ("H", "<i4"), ("W", "<i4"), ("bz", "<i4", 4), ("layout_color", "<i4"), ("wall_color", "<i4"),
    ("draw_walls", "<i4"), ("num_objects", "<i4"), ("num_boxes", "<i4"), ("num_frames", "<i4"), ("done", "<i4"),
    ("highest_tower", "<i4"), ("num_agents", "<i4"), ("num_terrain", "<i4"), ("num_rewards", "<i4"), ("num_platforms", "<i4"),
    ("solved", "<i4"), ("episode_sec", "<f4"), ("episode_len", "<f4"), ("bz_reward", "<f4"),
    ("bar_half_width", "<f4"), ("boxes", "<i4", (MAX_BOXES, 8)), ("terrain", "<i4", (MAX_TERRAIN, 8)),
    ("objects", "i1", (MAX_OBJECTS, 4)), ("rewards", "i1", (MAX_REWARDS, 4)),
    ("agents", SNAP_AGENT, MAX_AGENTS), ("chunk", "u1", CHUNK), ("heightmap", "i1", HM_DIM * HM_DIM),
    ("num_items", "<i4"), ("items", "<i4", (8, 5)), ("soko", "u1", 32 * 32),
    ("hex_num_boxes", "<i4"), ("hex_num_objs", "<i4"), ("hex_target", "<f4", 3),
    ("hex_boxes", HEX_REC, HEX_MAX_BOXES), ("hex_objs", HEX_REC, HEX_MAX_OBJS),
])


def build_oracle():
    so = os.path.join(ORACLE_DIR, "libmv_oracle.so")
    src = os.path.join(ORACLE_DIR, "mv_oracle.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build_oracle())
        L.mvo_create.restype = C.c_void_p
        L.mvo_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p),
                                 C.POINTER(C.c_float), C.c_int]
        for name in ("mvo_close", "mvo_reset", "mvo_step", "mvo_step_norender", "mvo_render"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        L.mvo_seed.argtypes = [C.c_void_p, C.c_int]
        L.mvo_set_actions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.mvo_set_action_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mvo_is_done.argtypes = [C.c_void_p, C.c_int]
        L.mvo_get_dones.argtypes = [C.c_void_p, C.c_void_p]
        L.mvo_render_env.argtypes = [C.c_void_p, C.c_int]
        L.mvo_set_raster.argtypes = [C.c_void_p, C.c_int]
        L.mvo_render_f64.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.mvo_render_f64.restype = None
        L.mvo_explain_f64.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.mvo_explain_f64.restype = None
        L.mvo_prim_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mvo_get_last_rewards.argtypes = [C.c_void_p, C.c_void_p]
        L.mvo_true_objective.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mvo_true_objective.restype = C.c_float
        L.mvo_get_observation.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mvo_get_observation.restype = C.c_void_p
        L.mvo_get_reward_shaping.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
        L.mvo_get_reward_shaping.restype = C.c_float
        L.mvo_set_reward_shaping.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_float]
        L.mvo_debug_set_agent_pos.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
        L.mvo_debug_set_agent_yaw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
        L.mvo_debug_set_agent_velocity.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
        L.mvo_debug_set_agent_pitch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
        L.mvo_debug_set_objects.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.mvo_set_action_masks.argtypes = [C.c_void_p, C.c_void_p]
        L.mvo_snapshot_size.argtypes = [C.c_void_p]
        L.mvo_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_debug_boxagone_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_debug_football_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_debug_set_football_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_mt19937_nth.argtypes = [C.c_uint32, C.c_int]
        L.mvo_mt19937_nth.restype = C.c_uint32
        L.mvo_rand_range_seq.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_frand_seq.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        L.mvo_shuffle_iota.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        L.mvo_action_mask.argtypes = [C.POINTER(C.c_int), C.c_int]
        L.mvo_get_coords.argtypes = [C.c_void_p, C.c_void_p]
        L.mvo_building_reward_coeff.argtypes = [C.c_float]
        L.mvo_building_reward_coeff.restype = C.c_float
        L.mvo_sincos.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.mvo_perlin_octave2_01.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mvo_debug_sweep.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_debug_recover.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mvo_debug_player_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


# ---- the controller's physics on caller-given colliders (mv_oracle.h: mvo_debug_sweep ...; records: tests/physics_reference.py)

def _oracle_cols(cols):
    """COL records with the device's kinds -> the oracle's: a hex box 3 + f becomes 3 | f << 8, the ball (7) becomes 4"""
    import physics_reference as R
    out = np.ascontiguousarray(cols, R.COL).copy()
    k = out["kind"].copy()
    hexf = (k >= 3) & (k <= 5)
    out["kind"] = np.where(hexf, 3 | ((k - 3) << 8), np.where(k == R.KIND_BALL, 4, k))
    assert np.isin(k, (0, 1, 2, 3, 4, 5, R.KIND_BALL)).all()
    return out


def debug_sweep(cols, queries):
    """the oracle's sweep() for every QUERY against the colliders -> SWEEP_OUT [n]"""
    import physics_reference as R
    oc, q = _oracle_cols(cols), np.ascontiguousarray(queries, R.QUERY)
    out = np.zeros(len(q), R.SWEEP_OUT)
    assert lib().mvo_debug_sweep(oc.ctypes.data, len(oc), q.ctypes.data, len(q), out.ctypes.data) == 0
    return out


def debug_recover(cols, positions):
    """the oracle's push-out loop from every position [n, 3] -> RECOVER_OUT [n]"""
    import physics_reference as R
    oc, p = _oracle_cols(cols), np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    out = np.zeros(len(p), R.RECOVER_OUT)
    assert lib().mvo_debug_recover(oc.ctypes.data, len(oc), p.ctypes.data, len(p), out.ctypes.data) == 0
    return out


def debug_player_step(cols, agents):
    """the oracle's player_step for every AGENT record -> (AGENT [n] after the step, [n] sweeps its plain forward loop ran)"""
    import physics_reference as R
    oc, a = _oracle_cols(cols), np.ascontiguousarray(agents, R.AGENT)
    out, sweeps = np.zeros(len(a), R.AGENT), np.zeros(len(a), np.int32)
    assert lib().mvo_debug_player_step(oc.ctypes.data, len(oc), a.ctypes.data, len(a), out.ctypes.data, sweeps.ctypes.data) == 0
    return out, sweeps


def ref_lib():
    """oracle/_ref/libmv_ref_util.so: the reference's own util.hpp compiled in place (or None)."""
    p = os.path.join(ORACLE_DIR, "_ref", "libmv_ref_util.so")
    if not os.path.exists(p):
        return None
    L = C.CDLL(p)
    L.mvref_rand_range_seq.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.mvref_frand_seq.argtypes = [C.c_uint, C.c_int, C.c_void_p]
    L.mvref_random_bool_seq.argtypes = [C.c_uint, C.c_int, C.c_void_p]
    L.mvref_env_seeds.argtypes = [C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "mvref_perlin_octave2_01"):
        L.mvref_perlin_octave2_01.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


class OracleGym:
    """Same method table as MegaverseGym (bindings/megaverse.cpp:267-292), backed by the oracle."""

    def __init__(self, scenario, w, h, num_envs, num_agents_per_env, num_simulation_threads=1, use_vulkan=False,
                 float_params=None):
        self.L = lib()
        fp = float_params or {}
        keys = (C.c_char_p * max(1, len(fp)))(*[k.encode() for k in fp])
        vals = (C.c_float * max(1, len(fp)))(*[float(v) for v in fp.values()])
        self.w, self.h, self.num_envs, self.num_agents_per_env = w, h, num_envs, num_agents_per_env
        self.g = self.L.mvo_create(scenario.encode(), w, h, num_envs, num_agents_per_env, num_simulation_threads, keys,
                                   vals, len(fp))
        if not self.g:
            raise RuntimeError("mvo_create failed")

    def num_agents(self): return self.num_agents_per_env
    def action_space_sizes(self): return [3, 3, 3, 2, 2, 3]
    def seed(self, s): self.L.mvo_seed(self.g, int(s))
    def reset(self): self.L.mvo_reset(self.g)

    def set_actions(self, env_idx, agent_idx, actions):
        arr = (C.c_int * len(actions))(*[int(a) for a in actions])
        self.L.mvo_set_actions(self.g, env_idx, agent_idx, arr, len(actions))

    def set_action_mask(self, env_idx, agent_idx, mask): self.L.mvo_set_action_mask(self.g, env_idx, agent_idx, int(mask))

    def set_action_masks(self, masks):
        m = np.ascontiguousarray(masks, dtype=np.int32).reshape(self.num_envs * self.num_agents_per_env)
        self.L.mvo_set_action_masks(self.g, m.ctypes.data)

    def step(self): self.L.mvo_step(self.g)
    def step_norender(self): self.L.mvo_step_norender(self.g)
    def render(self): self.L.mvo_render(self.g)
    def is_done(self, env_idx): return bool(self.L.mvo_is_done(self.g, env_idx))

    def get_dones(self):
        out = np.empty(self.num_envs, np.uint8)
        self.L.mvo_get_dones(self.g, out.ctypes.data)
        return out

    def render_env(self, env_idx): self.L.mvo_render_env(self.g, int(env_idx))
    def set_raster(self, tiled): self.L.mvo_set_raster(self.g, 1 if tiled else 0)

    def render_f64(self, env_idx, agent_idx):
        """the float64 reference's frame -> (rgba [h, w, 4] uint8, prim [h, w] int32: the winning primitive's index in the draw list, -1 for a miss)"""
        rgba = np.zeros((self.h, self.w, 4), np.uint8)
        prim = np.full((self.h, self.w), -2, np.int32)
        self.L.mvo_render_f64(self.g, int(env_idx), int(agent_idx), rgba.ctypes.data, prim.ctypes.data)
        return rgba, prim

    def explain_f64(self, env_idx, agent_idx, xy, delta_px, eps_t):
        """xy [n, 2] = (column, row) -> (colours [n, EXPLAIN_MAX, 4] uint8, counts [n]): every colour the float64 reference allows at these pixels for an
        evaluation off by at most delta_px in the ray's screen position and eps_t (relative) in depth; colours[i, :counts[i]] are valid"""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        assert ((xy >= 0) & (xy < [self.w, self.h])).all(), "pixel outside the frame"
        colors = np.zeros((len(xy), EXPLAIN_MAX, 4), np.uint8)
        counts = np.zeros(len(xy), np.int32)
        self.L.mvo_explain_f64(self.g, int(env_idx), int(agent_idx), len(xy), xy.ctypes.data, float(delta_px), float(eps_t), colors.ctypes.data, counts.ctypes.data)
        return colors, counts

    def prim_table(self, env_idx, agent_idx):
        """the frame's draw list as [n, 2] = (kind, frame) rows, indexed by render_f64's prim"""
        n = self.L.mvo_prim_table(self.g, int(env_idx), int(agent_idx), 0, None)
        out = np.zeros((n, 2), np.int32)
        assert self.L.mvo_prim_table(self.g, int(env_idx), int(agent_idx), n, out.ctypes.data) == n
        return out

    def get_last_rewards(self):
        out = np.zeros(self.num_envs * self.num_agents_per_env, np.float32)
        self.L.mvo_get_last_rewards(self.g, out.ctypes.data)
        return out

    def true_objective(self, env_idx, agent_idx): return float(self.L.mvo_true_objective(self.g, env_idx, agent_idx))

    def get_observation(self, env_idx, agent_idx):
        p = self.L.mvo_get_observation(self.g, env_idx, agent_idx)
        buf = (C.c_uint8 * (self.h * self.w * 4)).from_address(p)
        return np.frombuffer(buf, np.uint8).reshape(self.h, self.w, 4)

    def get_reward_shaping(self, env_idx, agent_idx):
        out = {}
        for k in ("teamSpirit", "towerPickedUpObject", "towerVisitedBuildingZoneWithObject", "towerBuildingReward",
                  "obstaclesAgentAtExit", "obstaclesAllAgentsAtExit", "obstaclesExtraReward", "obstaclesAgentCarriedObjectToExit",
                  "memoryCollectGood", "memoryCollectBad", "exploreSolved",
                  "collectSingleGood", "collectSingleBad", "collectAll", "collectAbyss",
                  "rearrangeOneMoreObjectCorrectPosition", "rearrangeAllObjectsCorrectPosition",
                  "sokobanBoxOnTarget", "sokobanBoxLeavesTarget", "sokobanAllBoxesOnTarget",
                  "boxagoneTouchedFloor", "boxagonePerStepReward"):
            f = C.c_int(0)
            v = self.L.mvo_get_reward_shaping(self.g, env_idx, agent_idx, k.encode(), C.byref(f))
            if f.value:
                out[k] = float(v)
        return out

    def set_reward_shaping(self, env_idx, agent_idx, rs):
        for k, v in rs.items():
            self.L.mvo_set_reward_shaping(self.g, env_idx, agent_idx, k.encode(), float(v))

    def debug_set_agent_pos(self, env_idx, agent_idx, x, y, z): self.L.mvo_debug_set_agent_pos(self.g, env_idx, agent_idx, x, y, z)
    def debug_set_agent_yaw(self, env_idx, agent_idx, c, s): self.L.mvo_debug_set_agent_yaw(self.g, env_idx, agent_idx, c, s)
    def debug_set_agent_velocity(self, env_idx, agent_idx, hvx, hvz, vvel): self.L.mvo_debug_set_agent_velocity(self.g, env_idx, agent_idx, hvx, hvz, vvel)

    def debug_set_agent_pitch(self, env_idx, agent_idx, pitch):
        if self.L.mvo_debug_set_agent_pitch(self.g, env_idx, agent_idx, pitch) != 0:
            raise RuntimeError("mvo_debug_set_agent_pitch: index out of range")

    def debug_set_objects(self, env_idx, objects):
        """TowerBuilding: the env's movable boxes, int8 [n, 4] rows (x, y, z, state) -- same arguments and refusals as MegaverseGym.debug_set_objects"""
        o = np.ascontiguousarray(objects, dtype=np.int8).reshape(-1, 4)
        if self.L.mvo_debug_set_objects(self.g, env_idx, o.ctypes.data, len(o)) != 0:
            raise RuntimeError("mvo_debug_set_objects: refused")

    def snapshot(self, env_idx):
        assert self.L.mvo_snapshot_size(self.g) == SNAP.itemsize, (self.L.mvo_snapshot_size(self.g), SNAP.itemsize)
        buf = np.zeros(1, SNAP)
        self.L.mvo_snapshot(self.g, env_idx, buf.ctypes.data)
        return buf[0]

    def boxagone_state(self, env_idx):
        """BoxAGone: the device's BoxAGoneState record (tests/boxagone_model.STATE) as the oracle's containers describe it"""
        import boxagone_model
        assert self.L.mvo_debug_boxagone_state(self.g, env_idx, None) == boxagone_model.STATE.itemsize
        buf = np.zeros(1, boxagone_model.STATE)
        assert self.L.mvo_debug_boxagone_state(self.g, env_idx, buf.ctypes.data) == boxagone_model.STATE.itemsize
        return buf[0]

    def football_state(self, env_idx):
        """Football: the device's FootballState record (tests/football_model.STATE) of the oracle's ball"""
        import football_model
        assert self.L.mvo_debug_football_state(self.g, env_idx, None) == football_model.STATE.itemsize
        buf = np.zeros(1, football_model.STATE)
        assert self.L.mvo_debug_football_state(self.g, env_idx, buf.ctypes.data) == football_model.STATE.itemsize
        return buf[0]

    def set_football_state(self, env_idx, pos, vel=(0.0, 0.0, 0.0), ang=(0.0, 0.0, 0.0), force=(0.0, 0.0, 0.0), radius=1.0):
        """Football: place the ball (same arguments as MegaverseGym.debug_set_football_state); its drawn record follows"""
        import football_model
        s = np.zeros(1, football_model.STATE)
        s["pos"], s["vel"], s["ang"], s["force"], s["radius"] = pos, vel, ang, force, radius
        assert self.L.mvo_debug_set_football_state(self.g, env_idx, s.ctypes.data) == 0

    def close(self):
        if self.g:
            self.L.mvo_close(self.g)
            self.g = None
