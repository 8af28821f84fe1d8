"""Scene observations on the GPU (include/megaverse_hip.h: mv_set_scene_obs): one row of 32 float32 per ENV for every tick of every stepping call, in the
ring entry of its tick.

Every comparison is equality of uint32 views, bit for bit.  What a row must hold comes from outside the feature: the record's table restated in numpy
(scene_obs_util) applied to the CPU oracle's snapshot, or to the debug snapshot of a twin gym WITHOUT a buffer that is stepped tick by tick with mv_step on the
same actions; column 7 comes from mv_debug_episodes_consumed.  Every case runs at 32 x 32 pixels with 3 or 9 envs: with 9 the 288 words of a tick straddle two
256-thread blocks of the gather and publish kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_log_util as U
import football_cases as FC
import football_model
import oracle_lib
import scene_obs_util as S
import state_obs_util as SO
from hip_util import hip_snapshot
from megaverse_amd.extension import SCENE_OBS_FIELDS, SCENE_OBS_SCENARIO_FIELDS, MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = pytest.mark.gpu

ENV_SEED, POLICY_SEED = 42, 1234
W = H = 32
DEV = "cuda:0"
SENT = 0xA5A5A5A5 - (1 << 32)   # (as an int32: the sentinel's bits in every word the gym must not write)


def acts_of(tick, rows):
    return sample_actions(POLICY_SEED, tick, rows)


class Rig:
    """one gym; optionally output rings of `ring` entries, a scene buffer (and a state buffer) with one entry more than the gym is given: the extra one must
    keep the sentinel"""

    def __init__(self, scenario, A=1, n=3, ring=0, scene=True, state=False, mode="fast", params=None, log=0, pipelining=True, overlap=False,
                 attach_before_reset=False):
        import torch
        U.boxoban_env()
        self.scenario, self.A, self.n, self.R, self.rows = scenario, A, n, ring, n * A
        self.g = g = MegaverseGym(scenario, W, H, n, A, 1, False, dict(params or {}))
        g.set_pixel_mode(mode)
        if not pipelining:
            g.set_pipelining(False)
        g.seed(ENV_SEED)
        if log:
            g.set_episode_log(log)
        self.entries = max(1, ring)
        self.slab = torch.zeros((self.rows, H, W, 4), dtype=torch.uint8, device=DEV)
        self.obs = torch.zeros((ring, self.rows, H, W, 4), dtype=torch.uint8, device=DEV) if ring else None
        self.rew = torch.full((ring, self.rows), -7.0, dtype=torch.float32, device=DEV) if ring else None
        self.done = torch.full((ring, n), 9, dtype=torch.uint8, device=DEV) if ring else None
        self.buf = torch.full((self.entries + 1, n, 32), SENT, dtype=torch.int32, device=DEV).view(torch.float32) if scene else None
        self.sbuf = torch.full((self.entries + 1, self.rows, 16), SENT, dtype=torch.int32, device=DEV).view(torch.float32) if state else None
        torch.cuda.synchronize()
        g.set_obs_buffer(self.slab.data_ptr())
        if attach_before_reset:   # (valid before the first mv_reset; without a ring: one entry)
            assert ring == 0
            self.attach()
        g.reset()
        if ring:   # (attached behind the reset: tick t of the calls that follow goes to entry t % ring)
            g.set_output_ring(ring, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        if not attach_before_reset:
            self.attach()
        if overlap:
            g.set_pass_overlap(True)
        self.ticks = 0

    def attach(self, scene=True, state=True):
        if self.buf is not None and scene:
            got = self.g.set_scene_obs(self.buf[:self.entries])
            assert got.data_ptr() == self.buf.data_ptr() and self.g.scene_obs_ring() is got
            assert self.g._lib.mv_get_scene_obs(self.g._g) == self.entries
        if self.sbuf is not None and state:
            self.g.set_state_obs(self.sbuf[:self.entries])

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def scene(self):
        """-> uint32 [entries, n, 32], after checking that the entry past the last one still holds the sentinel"""
        self.sync()
        x = self.buf.cpu().numpy().view(np.uint32)
        assert (x[self.entries] == 0xA5A5A5A5).all(), "the gym wrote past the last entry of the scene buffer"
        return x[:self.entries]

    def state(self):
        self.sync()
        x = self.sbuf.cpu().numpy().view(np.uint32)
        assert (x[self.entries] == 0xA5A5A5A5).all(), "the gym wrote past the last entry of the state buffer"
        return x[:self.entries]

    def ball(self, e):
        return FC.record(self.g.debug_football_state(e))

    def truth(self):
        """the table applied to mv_debug_snapshot (and the debug hooks for column 7 and the ball) of every env -> uint32 [n, 32]"""
        self.sync()
        return S.rows_of(self.scenario, lambda e: hip_snapshot(self.g, e), self.g.debug_episodes_consumed(), self.n, self.ball)

    def state_truth(self):
        return SO.rows_of_gym_snapshots(lambda e: hip_snapshot(self.g, e), self.n, self.A)

    def step(self, acts=None, render=True):
        self.g.set_actions_batched(acts_of(self.ticks, self.rows) if acts is None else acts)
        rc = (self.g._lib.mv_step if render else self.g._lib.mv_step_no_render)(self.g._g)
        assert rc >= 0, self.g._lib.mv_last_error()
        self.ticks += 1

    def set_action_ring(self, ticks):
        import torch
        self.actions = torch.as_tensor(np.stack([acts_of(t, self.rows) for t in range(ticks)])).to(DEV).contiguous()
        torch.cuda.synchronize()
        self.g.set_action_ring(ticks, self.actions.data_ptr())

    def step_n(self, k, render="every", policy="sequence"):
        self.g.step_n(k, policy, POLICY_SEED, self.ticks, render=render)
        self.ticks += k

    def plant(self):
        """every word of the scene buffer back to the sentinel"""
        self.sync()
        self.buf.view(__import__("torch").int32).fill_(SENT)
        self.sync()

    def close(self):
        self.sync()
        self.g.close()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x}"


def f32(words):
    return np.asarray(words, np.uint32).view(np.float32)


def set_masks(og, acts, n, A):
    masks = action_masks(acts)
    for e in range(n):
        for a in range(A):
            og.set_action_mask(e, a, int(masks[e * A + a]))


def first_exit(snap):
    """(centre x, y just inside, centre z) of the first exit box of a snapshot (SNAP.terrain rows: min[3], max[3], type, 0), or None"""
    for t in snap["terrain"][:int(snap["num_terrain"])]:
        if t[6] & S.TERRAIN_EXIT:
            return 0.5 * (t[0] + t[3]), t[1] + 0.5, 0.5 * (t[2] + t[5])
    return None


# ---- 1. against the oracle, tick by tick ------------------------------------------------------------------------------------------------------------------
# episodeLengthSec: TowerBuilding adds 4 s per object and Collect 2 s per diamond to it, so a negative value makes every episode end on its first tick (a new
# level on every tick); HexExplore and Football take it as it is (1.5 s: dones on ticks 22 and 45).  The Obstacles family never goes below 35 s per platform
# whatever the parameter says: its envs end their episodes at the exit pad, where every agent is put at ticks 4 and 30 (the hook both sides have).
CASES = {"tower_a1": ("TowerBuilding", 1, -300.0), "tower_a4": ("TowerBuilding", 4, -300.0), "obstacles_easy": ("ObstaclesEasy", 1, None),
         "obstacles_hard": ("ObstaclesHard", 1, None), "hex_explore": ("HexExplore", 1, 1.5), "football_a1": ("Football", 1, 1.5),
         "football_a2": ("Football", 2, 1.5), "collect": ("Collect", 1, -200.0)}
ORACLE_TICKS, EXIT_TICKS = 56, (4, 30)


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_the_oracle_tick_by_tick(hip, case):
    """1. 3 envs, 56 ticks of mv_step under the in-kernel random policy: the row behind mv_reset and every env's row behind every tick is the table applied
    to the oracle's snapshot; every env auto-resets at least twice; column 7 goes up by exactly 1 on the ticks that report done, and on no other"""
    scenario, A, sec = CASES[case]
    n = 3
    params = {} if sec is None else {"episodeLengthSec": sec}
    U.boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, n, A, 1, False, params or None)
    og.seed(ENV_SEED)
    og.reset()
    r = Rig(scenario, A, n, params=params, attach_before_reset=True, mode="exact")
    ball_of = og.football_state
    consumed = r.g.debug_episodes_consumed()
    same(r.scene()[0], S.rows_of(scenario, og.snapshot, consumed, n, ball_of), f"{case}: behind mv_reset")
    resets = np.zeros(n, int)
    distinct = set()
    for t in range(ORACLE_TICKS):
        if sec is None and t in EXIT_TICKS:
            for e in range(n):
                spot = first_exit(og.snapshot(e))
                assert spot is not None, "a level without an exit pad"
                for a in range(A):
                    og.debug_set_agent_pos(e, a, *[float(v) for v in spot])
                    r.g.debug_set_agent_pos(e, a, *[float(v) for v in spot])
        set_masks(og, acts_of(t, n * A), n, A)
        og.step_norender()
        r.g.sample_random_actions(POLICY_SEED, t)
        r.g.step()
        before, consumed = consumed, r.g.debug_episodes_consumed()
        dones = np.asarray(og.get_dones(), np.uint8)
        assert r.g.get_dones().tolist() == dones.tolist(), f"{case}: dones of tick {t}"
        got = r.scene()[0]
        same(got, S.rows_of(scenario, og.snapshot, consumed, n, ball_of), f"{case}: tick {t}")
        assert (consumed - before).tolist() == dones.astype(int).tolist(), f"{case}, tick {t}: the episode counter moved {consumed - before}, dones {dones}"
        same(got[:, S.F["episodes_consumed"]], S.of_int(consumed), f"{case}: column 7 of tick {t}")
        resets += dones
        distinct.add(got.tobytes())
    same(r.g.get_scene_observation(n - 1).view(np.uint32), got[n - 1], f"{case}: mv_get_scene_observation")
    assert (resets >= 2).all(), f"{case}: auto-resets per env {resets}"
    assert len(distinct) == ORACLE_TICKS, "the rows did not change on every tick: the comparison would prove less than it says"
    if sec is None:
        assert (got[:, S.NUM_EXITS] != 0).all()
    og.close(); r.close()


# ---- 2. Obstacles events ------------------------------------------------------------------------------------------------------------------------------------
def test_obstacles_events(hip):
    """2. ObstaclesHard, two agents per env, the teleport hooks on both sides: an agent on a diamond's cell -- column 23 drops by one; an agent on a lava box
    -- it is back at its spawn cell; every agent on the exit pad -- column 8 becomes 1.  Expectations are the oracle's; the gym's rows equal the oracle's on
    every tick"""
    scenario, n, A = "ObstaclesHard", 3, 2
    U.boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, n, A, 1, False, None)
    og.seed(ENV_SEED); og.reset()
    r = Rig(scenario, A, n)
    seen = {"diamond": 0, "lava": 0, "exit": 0}
    idle = np.zeros((n * A, 6), np.int32)

    def both(fn, *args):
        getattr(og, fn)(*args); getattr(r.g, fn)(*args)

    def tick(what):
        set_masks(og, idle, n, A)
        og.step_norender()
        r.step(idle)
        want = S.rows_of(scenario, og.snapshot, r.g.debug_episodes_consumed(), n)
        same(r.scene()[0], want, what)
        return want

    rows = tick("an idle tick")
    for e in range(n):   # a diamond
        s = og.snapshot(e)
        there = [i for i in range(int(s["num_rewards"])) if s["rewards"][i][3] != 0]
        if there:
            x, y, z = [int(v) for v in s["rewards"][there[0]][:3]]
            both("debug_set_agent_pos", e, 0, x + 0.5, y + 0.5, z + 0.5)
            both("debug_set_agent_velocity", e, 0, 0.0, 0.0, 0.0)
    after = tick("agents on diamonds")
    for e in range(n):
        if f32(after[e, S.DIAMONDS]) == f32(rows[e, S.DIAMONDS]) - 1:
            seen["diamond"] += 1
    rows = after
    placed = {}
    for e in range(n):   # lava, where the level has some
        s = og.snapshot(e)
        for t in s["terrain"][:int(s["num_terrain"])]:
            if t[6] & S.TERRAIN_LAVA:
                both("debug_set_agent_pos", e, 1, 0.5 * (t[0] + t[3]), t[1] + 0.5, 0.5 * (t[2] + t[5]))
                both("debug_set_agent_velocity", e, 1, 0.0, 0.0, 0.0)
                placed[e] = s["agents"][1]["spawn"].copy()
                break
    tick("agents on lava")
    for e, spawn in placed.items():
        p = og.snapshot(e)["agents"][1]["pos"]
        if int(np.floor(p[0])) == spawn[0] and int(np.floor(p[2])) == spawn[2]:
            seen["lava"] += 1
    for e in range(n):   # the exit pad
        spot = first_exit(og.snapshot(e))
        for a in range(A):
            both("debug_set_agent_pos", e, a, *[float(v) for v in spot])
    after = tick("every agent on the exit pad")
    seen["exit"] = int((f32(after[:, S.F["solved"]]) == 1.0).sum())
    assert (f32(rows[:, S.F["solved"]]) == 0.0).all()
    assert seen["exit"] == n and seen["diamond"] > 0, seen
    assert any(seen.values()), seen
    for k in range(8):   # ... and the episode ends 0.3 s later: the rows show the next level
        after = tick(f"behind the exit, tick {k}")
    assert (f32(after[:, S.F["solved"]]) == 0.0).all() and (f32(after[:, S.F["episodes_consumed"]]) > f32(rows[:, S.F["episodes_consumed"]])).all()
    og.close(); r.close()


# ---- 3. Football --------------------------------------------------------------------------------------------------------------------------------------------
def test_football(hip):
    """3. the ball placed in flight, resting and against a wall on both sides, the agents beside it, a chase-and-kick script for 30 ticks: columns 16..30 (and
    every other) on every tick; the drawn radius is 0.5 on the frame after a reset and 1.0 after the first tick; a kick is seen"""
    n, A = 3, 1
    U.boxoban_env()
    og = oracle_lib.OracleGym("Football", W, H, n, A, 1, False, None)
    og.seed(ENV_SEED); og.reset()
    r = Rig("Football", A, n, attach_before_reset=True)
    row0 = r.scene()[0]
    same(row0, S.rows_of("Football", og.snapshot, r.g.debug_episodes_consumed(), n, og.football_state), "behind mv_reset")
    assert (f32(row0[:, S.BALL_RADIUS]) == 0.5).all()
    balls = [dict(pos=(6.0, 3.5, 6.0), vel=(2.0, 3.0, -1.0)), dict(pos=(6.0, 2.0, 6.0)), dict(pos=(2.0, 2.0, 6.0), vel=(-3.0, 0.0, 0.0))]
    for e, b in enumerate(balls):
        og.set_football_state(e, radius=0.5, **b)
        r.g.debug_set_football_state(e, radius=0.5, **b)
        p = (b["pos"][0] + 1.8, FC.REST_Y, b["pos"][2])
        for g in (og, r.g):
            g.debug_set_agent_pos(e, 0, *p)
            g.debug_set_agent_yaw(e, 0, *FC.facing(p, b["pos"]))
    same(r.scene()[0], row0, "the debug setters touched a row")
    kicks = walls = 0
    for t in range(30):
        acts = np.concatenate([FC.chaser(og.snapshot(e), og.football_state(e)["pos"], A) for e in range(n)])
        set_masks(og, acts, n, A)
        og.step_norender()
        r.step(acts)
        want = S.rows_of("Football", og.snapshot, r.g.debug_episodes_consumed(), n, og.football_state)
        got = r.scene()[0]
        same(got[:, 16:31], want[:, 16:31], f"tick {t}: the ball's columns")
        same(got, want, f"tick {t}")
        assert (f32(got[:, S.BALL_RADIUS]) == 1.0).all()
        kicks += int((f32(want[:, S.KICKS]) > 0).sum())
        walls += int(sum(bool(int(x) & (0xF << 9)) for x in f32(want[:, S.CONTACTS])))
    assert kicks > 0, "no kick in 30 ticks of chasing"
    assert walls > 0, "the ball never touched a wall"
    og.close(); r.close()


# ---- 4. launch shapes -----------------------------------------------------------------------------------------------------------------------------------------
TWIN_TICKS = 51
SHAPE_GYMS = {"tower_a4": ("TowerBuilding", 4), "obstacles_a2": ("ObstaclesHard", 2)}


@functools.lru_cache(maxsize=None)
def twin_rows(gym, policy):
    """a gym WITHOUT a buffer, 3 envs, stepped by mv_step tick by tick -- `sequence`: on acts_of(t); `multidiscrete`: on the in-kernel random policy's
    actions of (POLICY_SEED, t) -> (rows uint32 [51, 3, 32] from its debug snapshots, rewards uint32 [51, 3 A], dones uint8 [51, 3])"""
    scenario, A = SHAPE_GYMS[gym]
    t = Rig(scenario, A, scene=False)
    rows, rew, done = [], [], []
    for k in range(TWIN_TICKS):
        if policy == "sequence":
            t.step()
        else:
            t.g.sample_random_actions(POLICY_SEED, k)
            t.g.step()
        rows.append(t.truth())
        rew.append(t.g.get_rewards_array().view(np.uint32).copy())
        done.append(t.g.get_dones().copy())
    t.close()
    out = np.stack(rows), np.stack(rew), np.stack(done)
    for x in out:
        x.setflags(write=False)
    return out


def run_shape(gym, k, calls, render, policy, ring, pipelining=True, overlap=False):
    scenario, A = SHAPE_GYMS[gym]
    rows, rew, done = twin_rows(gym, policy)
    r = Rig(scenario, A, ring=ring, pipelining=pipelining, overlap=overlap)
    if policy == "sequence":
        r.set_action_ring(TWIN_TICKS)
    what = f"{gym}, k {k}, {render}, {policy}, ring {ring}, pipelining {pipelining}, overlap {overlap}"

    def check(ticks):
        sc = r.scene()
        for t in ticks:
            same(sc[t % r.entries], rows[t], f"{what}: tick {t}, entry {t % r.entries}")
            if ring:
                same(r.rew.cpu().numpy().view(np.uint32)[t % ring], rew[t], f"{what}: tick {t}, reward ring")
                same(r.done.cpu().numpy()[t % ring], done[t], f"{what}: tick {t}, done ring")

    for c in range(calls):
        r.step_n(k, render, policy)
        if not overlap:   # (the entries that still hold a tick of this call: all of them with a ring of k or more, the last `entries` otherwise)
            check(range(max(r.ticks - k, r.ticks - r.entries), r.ticks))
    if overlap:   # (the calls back to back, no host wait between them)
        check(range(r.ticks - ring, r.ticks))
    r.close()


@pytest.mark.parametrize("render", ["every", "none", "last"])
@pytest.mark.parametrize("gym", sorted(SHAPE_GYMS))
def test_launch_shapes(hip, gym, render):
    """4. step_n with k in {1, 8, 9, 16, 17}, two calls each, into rings of k entries (k = 1: no ring), policies `sequence` and `multidiscrete` in turn: every
    tick's entry equals the twin's row of that tick, and the reward and done rings what the twin reported.  TowerBuilding with four agents: the multi-wave
    workgroup, whose first wave stores behind the barrier; ObstaclesHard with two: the tick-by-tick multi-agent path, and the wave's reductions"""
    for i, k in enumerate((1, 8, 9, 16, 17)):
        run_shape(gym, k, 2, render, ("sequence", "multidiscrete")[i % 2], 0 if k == 1 else k)
    run_shape(gym, 16, 2, render, "multidiscrete", 16)
    run_shape(gym, 9, 2, render, "sequence", 9)


@pytest.mark.parametrize("gym", sorted(SHAPE_GYMS))
def test_launch_shapes_rings_and_streams(hip, gym):
    """4. no ring (the one entry holds the call's last tick), a ring of 4 with k = 6 (the entries wrap inside the call), pipelining off, pass overlap on"""
    run_shape(gym, 9, 3, "every", "sequence", 0)
    run_shape(gym, 6, 3, "every", "multidiscrete", 4)
    run_shape(gym, 6, 3, "none", "sequence", 4)
    run_shape(gym, 16, 2, "every", "sequence", 16, pipelining=False)
    run_shape(gym, 16, 2, "last", "multidiscrete", 16, pipelining=False)
    run_shape(gym, 16, 3, "every", "sequence", 32, overlap=True)


def test_step_no_render_and_one_agent_kernels(hip):
    """4. one agent per env (the one-wave resident kernels and the software-pipelined one), 9 envs: mv_step_no_render tick by tick, then calls of 16 in every
    render mode -- every entry is the table applied to the same gym's snapshot where a snapshot can be taken (behind the call: its last tick)"""
    for scenario in ("ObstaclesHard", "Empty", "HexExplore", "Football", "TowerBuilding"):
        r = Rig(scenario, n=9, ring=16)
        r.set_action_ring(64)
        for t in range(3):
            r.step(render=False)
            same(r.scene()[(r.ticks - 1) % 16], r.truth(), f"{scenario}: mv_step_no_render, tick {t}")
        for render in ("every", "none", "last"):
            r.step_n(16, render)
            sc = r.scene()
            same(sc[(r.ticks - 1) % 16], r.truth(), f"{scenario}: step_n(16, {render})")
            col = S.F["num_frames"]   # (every entry is a different tick of the call: the frame counter, or the episode counter, moved)
            assert len({(sc[j, e, col], sc[j, e, S.F["episodes_consumed"]]) for j in range(16) for e in range(1)}) == 16
        r.close()


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------------------------------------
SHORT = (("episodeLengthSec", 5.0),)   # 75 ticks where the scenario adds no time of its own


def test_step_mask_and_both_records(hip):
    """5. the odd envs frozen for a 16-tick call, state observations attached too: frozen envs repeat their row in every entry, both buffers' last entries
    equal the run's snapshots, and the call with both attached took ONE publication launch: the count with either alone"""
    n = 9
    r = Rig("TowerBuilding", 2, n, ring=16, state=True)
    r.set_action_ring(64)
    r.step_n(16)
    held = r.scene()[15].copy()
    same(held, r.truth(), "before the mask")
    same(r.state()[15], r.state_truth(), "before the mask: state rows")
    odd = np.arange(n) % 2 == 1
    r.g.set_step_mask(~odd)
    c0 = r.g.debug_launch_counts()
    r.step_n(16)
    both = np.array(r.g.debug_launch_counts()) - np.array(c0)
    sc = r.scene()
    for j in range(16):
        same(sc[j][odd], held[odd], f"entry {j}: frozen envs")
        assert not (sc[j][~odd] == held[~odd]).all(axis=1).any(), f"entry {j}: a stepping env's row did not move"
    same(sc[15], r.truth(), "behind the masked call")
    same(r.state()[15], r.state_truth(), "behind the masked call: state rows")
    counts = {}
    for name, scene, state in (("scene", True, False), ("state", False, True), ("neither", False, False)):
        r.g.set_scene_obs(None); r.g.set_state_obs(None)
        r.attach(scene, state)
        c0 = r.g.debug_launch_counts()
        r.step_n(16)
        counts[name] = np.array(r.g.debug_launch_counts()) - np.array(c0)
    assert both.tolist() == counts["scene"].tolist() == counts["state"].tolist(), (both, counts)
    assert counts["neither"][0] == both[0] and counts["neither"][1] == both[1] - 1, (both, counts)
    r.close()


def test_episode_budget_halts_inside_a_resident_launch(hip):
    """5. Empty, episodes of 75 ticks, budget 1, calls of 16: an env that halts inside a launch repeats the row of its finishing tick -- the first state of
    its next episode -- in every later entry; the last entry equals the snapshot behind every call"""
    n = 9
    r = Rig("Empty", n=n, ring=16, params=dict(SHORT))
    r.g.set_episode_budget(1)
    r.set_action_ring(96)
    halted_at, row_at = np.full(n, -1), {}
    for c in range(6):
        r.step_n(16)
        sc, done = r.scene(), r.done.cpu().numpy()
        same(sc[15], r.truth(), f"call {c}")
        for t in range(16 * c, 16 * c + 16):
            for e in range(n):
                if halted_at[e] >= 0:
                    same(sc[t % 16][e], row_at[e], f"tick {t}, env {e}: halted at tick {halted_at[e]}")
                elif done[t % 16][e]:
                    halted_at[e], row_at[e] = t, sc[t % 16][e].copy()
    assert (halted_at >= 64).all() and (halted_at % 16 != 15).any() and r.g.halted_count() == n
    r.close()


def test_draw_mask_still_frames_and_macro_steps(hip):
    """5. a draw mask and still frames on top of a step mask: the rows are the snapshots', drawn or not; macro steps with per-env ticks publish the rows behind
    their last tick only, into the call's one entry"""
    n = 9
    r = Rig("ObstaclesHard", 1, n, ring=4, state=True)
    r.g.set_draw_mask(np.arange(n) % 3 != 0)
    r.g.set_still_frames(True)
    r.g.set_step_mask(np.arange(n) % 2 == 0)
    r.set_action_ring(64)
    r.step_n(6)
    same(r.scene()[5 % 4], r.truth(), "draw mask, still frames, step mask: step_n(6)")
    r.step()
    same(r.scene()[6 % 4], r.truth(), "... mv_step")
    r.g.set_step_mask(None)
    r.plant()
    ticks = (np.arange(n) % 5).astype(np.int32)   # (0: the env does not step at all)
    before = r.truth()
    r.g.macro_step(4, acts_of(99, n), ticks, render="last")
    sc = r.scene()
    entry = 7 % 4
    same(sc[entry], r.truth(), "behind the macro step")
    same(r.state()[entry], r.state_truth(), "behind the macro step: state rows")
    same(sc[entry][ticks == 0], before[ticks == 0], "macro step: envs with 0 ticks")
    frames = S.F["num_frames"]
    assert (f32(sc[entry][:, frames]) - f32(before[:, frames])).tolist() == ticks.astype(np.float32).tolist(), "every env stepped its own number of ticks"
    for j in range(4):
        if j != entry:
            assert (sc[j] == 0xA5A5A5A5).all(), f"the macro step wrote entry {j}"
    r.g.macro_step(3, acts_of(100, n), None, render="none")
    same(r.scene()[8 % 4], r.truth(), "behind the second macro step")
    r.close()


# ---- 6. refresh and non-refresh -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_refresh_and_moves(hip, scenario):
    """6. mv_reset and mv_render refresh every row; reset_envs(mask, render=1) the flagged rows only, the others keep planted bytes; forks, resampling, loads,
    seeds and the debug setters change no byte until the next tick or mv_render"""
    n = 9
    r = Rig(scenario, 1, n)
    for _ in range(5):
        r.step()
    same(r.scene()[0], r.truth(), "behind 5 ticks")
    r.plant()
    r.g.render()
    same(r.scene()[0], r.truth(), "mv_render refreshes every row")
    r.plant()
    flagged = np.zeros(n, bool); flagged[[0, 3, 8]] = True
    r.g.reset_envs(flagged, render=True)
    sc, want = r.scene()[0], r.truth()
    same(sc[flagged], want[flagged], "reset_envs: the flagged rows")
    assert (sc[~flagged] == 0xA5A5A5A5).all(), "reset_envs wrote an unflagged env's row"
    import torch
    dev_mask = torch.as_tensor(~flagged).to(DEV)
    torch.cuda.synchronize()
    r.g.reset_envs(dev_mask, render=True)   # (the device form: the other six, across the gather's block boundary)
    same(r.scene()[0], r.truth(), "reset_envs, device mask: every row has been refreshed now")
    r.plant()
    r.g.reset_envs(flagged, render=False)
    assert (r.scene()[0] == 0xA5A5A5A5).all(), "reset_envs(render=0) wrote a row"
    r.g.reset()
    same(r.scene()[0], r.truth(), "mv_reset refreshes every row")
    for _ in range(3):
        r.step()
    r.plant()
    fork = np.full(n, -1, np.int32); fork[1] = 0
    r.g.fork_envs(fork)
    swap = np.full(n, -1, np.int32); swap[2], swap[3] = 3, 2
    r.g.resample_envs(swap)
    store = r.g.new_env_store(1)
    slot = np.full(n, -1, np.int32); slot[4] = 0
    r.g.save_envs(slot, store)
    slot = np.full(n, -1, np.int32); slot[5] = 0
    r.g.load_envs(slot, store)
    r.g.seed_envs({6: 7})
    r.g.debug_set_agent_pos(7, 0, 3.5, 3.5, 3.5)
    r.g.debug_set_agent_velocity(7, 0, 0.0, 0.0, 0.0)
    assert (r.scene()[0] == 0xA5A5A5A5).all(), "a fork, a resample, a load, a seed or a debug setter wrote a row"
    r.g.render()
    same(r.scene()[0], r.truth(), "mv_render shows the moved state")
    r.step()
    same(r.scene()[0], r.truth(), "the next tick")
    r.close()
    del store


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 2), ("ObstaclesHard", 1)])
def test_nothing_else_moves(hip, scenario, A):
    """7. a gym with the buffer attached and an unattached twin, 32 ticks (16 of mv_step, one call of 16), exact pixels, the episode log on: observations,
    rewards, dones, true objectives, snapshots and the drained log are identical; the same holds after detaching"""
    kw = dict(mode="exact", log=4096, A=A, n=3, ring=16)
    a, b = Rig(scenario, **kw), Rig(scenario, scene=False, **kw)
    for r in (a, b):
        r.set_action_ring(64)

    def compare(what):
        a.sync(); b.sync()
        for name in ("get_rewards_array", "get_dones", "get_true_objectives", "debug_episodes_consumed"):
            assert getattr(a.g, name)().tobytes() == getattr(b.g, name)().tobytes(), f"{what}: {name}"
        for x, y, nm in ((a.slab, b.slab, "slab"), (a.obs, b.obs, "observation ring"), (a.rew, b.rew, "reward ring"), (a.done, b.done, "done ring")):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"{what}: {nm}"
        bad = [e for e in range(a.n) if a.g.debug_snapshot_bytes(e).tobytes() != b.g.debug_snapshot_bytes(e).tobytes()]
        assert not bad, f"{what}: state of envs {bad}"

    def run(what):
        for t in range(16):
            a.step(); b.step()
            compare(f"{what}: tick {t}")
        a.step_n(16); b.step_n(16)
        compare(f"{what}: step_n(16)")

    run("attached")
    a.scene()
    a.g.set_scene_obs(None)
    held = a.scene().copy()
    a.ticks = b.ticks = 0
    run("detached")
    same(a.scene(), held, "rows written after the detach")
    la, lb = a.g.drain_episode_log(), b.g.drain_episode_log()
    assert la.tobytes() == lb.tobytes() and a.g.episode_log_dropped == b.g.episode_log_dropped
    a.close(); b.close()


# ---- 8. refusals and surface ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """8. a member of a group; mv_group_create / mv_step_many with an attached gym (nothing stepped), valid again after detach; mv_set_output_ring while
    attached; a wrong shape / dtype / device; an index out of range; a closed gym"""
    import torch
    n = 3
    ra, rb = Rig("TowerBuilding", n=n), Rig("ObstaclesEasy", n=n, scene=False)
    a, b = ra.g, rb.g
    lib = a._lib
    snaps = lambda g: [g.debug_snapshot_bytes(e).tobytes() for e in range(n)]   # noqa: E731
    handles = (C.c_void_p * 2)(a._g, b._g)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == -1 and b"mv_set_scene_obs" in lib.mv_last_error()
    before = snaps(a), snaps(b)
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) == -1 and b"mv_set_scene_obs" in lib.mv_last_error()
    assert (snaps(a), snaps(b)) == before, "mv_step_many stepped a gym before it refused"
    ring = torch.zeros((4, n), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="detach the scene observations first"):
        a.set_output_ring(4, 0, ring.data_ptr(), 0)
    for bad in (torch.zeros((1, n, 31), dtype=torch.float32, device=DEV), torch.zeros((2, n, 32), dtype=torch.float32, device=DEV),
                torch.zeros((1, n, 32), dtype=torch.float64, device=DEV), torch.zeros((1, n, 32), dtype=torch.float32),
                torch.zeros((1, n, 64), dtype=torch.float32, device=DEV)[:, :, ::2], np.zeros((1, n, 32), np.float32)):
        with pytest.raises(ValueError, match="set_scene_obs"):
            a.set_scene_obs(bad)
    assert a.scene_obs_ring() is not None and lib.mv_get_scene_obs(a._g) == 1
    with pytest.raises(RuntimeError, match="index out of range"):
        a.get_scene_observation(n)
    with pytest.raises(RuntimeError, match="index out of range"):
        a.get_scene_observation(-1)
    arena = a.arena_bytes()
    assert a.set_scene_obs(None) is None and a.scene_obs() is None and lib.mv_get_scene_obs(a._g) == 0
    with pytest.raises(RuntimeError, match="no scene observations attached"):
        a.get_scene_observation(0)
    assert a.arena_bytes() == arena and arena - rb.g.arena_bytes() != 0   # (the staging rows stay counted until mv_close)
    a.set_output_ring(4, 0, ring.data_ptr(), 0)   # (allowed again)
    a.set_output_ring(0)
    ra.sync(); rb.sync()
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) >= 0, lib.mv_last_error()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    for g in (a, b):
        assert lib.mv_set_scene_obs(g._g, C.c_void_p(ra.buf.data_ptr())) == -1 and b"mv_group" in lib.mv_last_error()
        assert lib.mv_get_scene_obs(g._g) == 0
        with pytest.raises(RuntimeError, match="mv_group"):
            g.set_scene_obs(True)
    assert lib.mv_group_destroy(grp) == 0
    ra.attach()   # (valid again once the group is gone)
    ra.step()
    same(ra.scene()[0], ra.truth(), "attached again")
    same(a.scene_obs().cpu().numpy().view(np.uint32), ra.scene()[0], "MegaverseGym.scene_obs()")
    ra.sync()
    handle = a._g
    lib.mv_close(handle)
    out = np.zeros(32, np.float32)
    assert lib.mv_set_scene_obs(handle, C.c_void_p(ra.buf.data_ptr())) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_scene_obs(handle) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_scene_observation(handle, 0, out.ctypes.data) == -1 and b"closed" in lib.mv_last_error()
    a.close(); rb.close()


def test_env_scene_obs(hip):
    """MegaverseEnv(..., scene_obs=True): scene_obs() is the last tick's [num_envs, 32] device view through reset, step_device and step_sequence (whose rings
    the env swaps under the buffer), with columns looked up through the tables; MegaverseGym.scene_obs() follows a ring"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("ObstaclesEasy", 3, 2, img_w=W, img_h=H, scene_obs=True, state_obs=True)
    env.seed(ENV_SEED)
    env.reset()
    assert env.SCENE_OBS_FIELDS is SCENE_OBS_FIELDS and env.SCENE_OBS_SCENARIO_FIELDS is SCENE_OBS_SCENARIO_FIELDS

    def check(what):
        rows = env.scene_obs()
        assert rows.shape == (3, 32) and rows.is_cuda and rows.dtype == torch.float32
        env.env.synchronize(); torch.cuda.synchronize()
        want = S.rows_of("ObstaclesEasy", lambda e: hip_snapshot(env.env, e), env.env.debug_episodes_consumed(), 3)
        same(rows.cpu().numpy().view(np.uint32), want, what)
        same(env.env.scene_obs().cpu().numpy().view(np.uint32), want, what + ": MegaverseGym.scene_obs()")
        assert env.state_obs().shape == (6, 16)
        return rows

    check("behind reset")
    env.step_device(acts_of(0, 6))
    check("behind step_device")
    env.step_sequence(np.stack([acts_of(t, 6) for t in range(1, 6)]))
    rows = check("behind step_sequence")
    assert env.env.scene_obs_ring().shape == (5, 3, 32)
    env.step_device(acts_of(6, 6))
    rows = check("behind step_device again")
    t = SCENE_OBS_SCENARIO_FIELDS["ObstaclesEasy"]
    assert (rows[:, SCENE_OBS_FIELDS["scenario"]] == 1.0).all() and (rows[:, t["num_exits"]] >= 1.0).all()
    assert (rows[:, t["exit_max_x"]] > rows[:, t["exit_min_x"]]).all() and (rows[:, SCENE_OBS_FIELDS["room_l"]] >= rows[:, t["exit_max_x"]]).all()
    env.close()
