"""State observations on the GPU (include/megaverse_hip.h: mv_set_state_obs): one row of 16 float32 per agent for every tick of every stepping call, in the
ring entry of its tick.

Every comparison is equality of uint32 views, bit for bit.  What a row must hold comes from outside the feature: the record's table restated in numpy
(state_obs_util.rows_of_snapshot) applied to the CPU oracle's snapshot, or to the debug snapshot of a twin gym WITHOUT a state buffer that is stepped tick by
tick with mv_step on the same actions.  Every case runs at 32 x 32 pixels."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_log_util as U
import oracle_lib
import state_obs_util as S
from hip_util import hip_snapshot
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = pytest.mark.gpu

ENV_SEED, POLICY_SEED = 42, 1234
W = H = 32
DEV = "cuda:0"
SENT = 0xA5A5A5A5 - (1 << 32)   # (as an int32: the sentinel's bits in every word the gym must not write)


def acts_of(tick, rows):
    return sample_actions(POLICY_SEED, tick, rows)


class Rig:
    """one gym; optionally output rings of `ring` entries and a state buffer with one entry more than the gym is given: the extra one must keep the sentinel"""

    def __init__(self, scenario, A=1, n=8, ring=0, state=True, mode="fast", params=None, log=0, pipelining=True, overlap=False, attach_before_reset=False):
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
        self.buf = torch.full((self.entries + 1, self.rows, 16), SENT, dtype=torch.int32, device=DEV).view(torch.float32) if state else None
        torch.cuda.synchronize()
        g.set_obs_buffer(self.slab.data_ptr())
        if state and attach_before_reset:   # (valid before the first mv_reset; without a ring: one entry)
            assert ring == 0
            self.attach()
        g.reset()
        if ring:   # (attached behind the reset: tick t of the calls that follow goes to entry t % ring)
            g.set_output_ring(ring, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        if state and not attach_before_reset:
            self.attach()
        if overlap:
            g.set_pass_overlap(True)
        self.ticks = 0

    def attach(self):
        got = self.g.set_state_obs(self.buf[:self.entries])
        assert got.data_ptr() == self.buf.data_ptr() and self.g.state_obs() is got
        assert self.g._lib.mv_get_state_obs(self.g._g) == self.entries

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def state(self):
        """-> uint32 [entries, rows, 16], after checking that the entry past the last one still holds the sentinel"""
        self.sync()
        x = self.buf.cpu().numpy().view(np.uint32)
        assert (x[self.entries] == 0xA5A5A5A5).all(), "the gym wrote past the last entry of the state buffer"
        return x[:self.entries]

    def snapshot_rows(self):
        """the table applied to mv_debug_snapshot of every env -> uint32 [rows, 16]"""
        return S.rows_of_gym_snapshots(lambda e: hip_snapshot(self.g, e), self.n, self.A)

    def step(self, acts=None, render=True):
        self.g.set_actions_batched(acts_of(self.ticks, self.rows) if acts is None else acts)
        rc = (self.g._lib.mv_step if render else self.g._lib.mv_step_no_render)(self.g._g)
        assert rc >= 0, self.g._lib.mv_last_error()
        self.ticks += 1

    def set_action_ring(self, ticks):
        """the actions of ticks 0 .. ticks - 1 as the gym's action ring: step_n(k, 'sequence', 0, t) then acts on what step() acts on at tick t"""
        import torch
        self.actions = torch.as_tensor(np.stack([acts_of(t, self.rows) for t in range(ticks)])).to(DEV).contiguous()
        torch.cuda.synchronize()
        self.g.set_action_ring(ticks, self.actions.data_ptr())

    def step_n(self, k, render="every"):
        self.g.step_n(k, "sequence", 0, self.ticks, render=render)
        self.ticks += k

    def close(self):
        self.sync()
        self.g.close()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x}"


# ---- the references, computed once ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(scenario, A, n, ticks, params_items=()):
    """the oracle stepped on acts_of(t): -> (rows uint32 [ticks + 1, n * A, 16]: index 0 behind reset, index t + 1 behind tick t; dones uint8 [ticks, n])"""
    U.boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, n, A, 1, False, dict(params_items) or None)
    og.seed(ENV_SEED)
    og.reset()
    rows = [S.rows_of_gym_snapshots(og.snapshot, n, A)]
    dones = []
    for t in range(ticks):
        masks = action_masks(acts_of(t, n * A))
        for e in range(n):
            for a in range(A):
                og.set_action_mask(e, a, int(masks[e * A + a]))
        og.step_norender()
        rows.append(S.rows_of_gym_snapshots(og.snapshot, n, A))
        dones.append(np.asarray(og.get_dones(), np.uint8).copy())
    og.close()
    out = np.stack(rows), np.stack(dones)
    for x in out:
        x.setflags(write=False)
    return out


TWIN_TICKS = 48


@functools.lru_cache(maxsize=None)
def twin_rows(scenario, A=1):
    """a gym WITHOUT a state buffer, 8 envs, stepped by mv_step on acts_of(t): -> (rows uint32 [48, 8 A, 16] from its debug snapshots, rewards
    uint32 [48, 8 A], dones uint8 [48, 8])"""
    t = Rig(scenario, A, state=False)
    rows, rew, done = [], [], []
    for _ in range(TWIN_TICKS):
        t.step()
        rows.append(t.snapshot_rows())
        rew.append(t.g.get_rewards_array().view(np.uint32).copy())
        done.append(t.g.get_dones().copy())
    t.close()
    out = np.stack(rows), np.stack(rew), np.stack(done)
    for x in out:
        x.setflags(write=False)
    return out


# ---- 1. against the oracle, tick by tick ------------------------------------------------------------------------------------------------------------------
FAMILIES = {"tower_a1": ("TowerBuilding", 1), "tower_a4": ("TowerBuilding", 4), "obstacles_hard": ("ObstaclesHard", 1), "collect": ("Collect", 1),
            "rearrange": ("Rearrange", 1), "sokoban": ("Sokoban", 1), "hex_memory": ("HexMemory", 1), "boxagone": ("BoxAGone", 1), "football": ("Football", 1),
            "empty": ("Empty", 1)}


@pytest.mark.parametrize("case", sorted(FAMILIES))
def test_against_the_oracle_tick_by_tick(hip, case):
    """1. 8 envs, 48 ticks of mv_step on the oracle's actions: the row behind mv_reset and every row behind every tick is the table applied to the oracle's
    snapshot; mv_get_state_observation reads the same row"""
    scenario, A = FAMILIES[case]
    ref, _ = oracle_rows(scenario, A, 8, 48)
    r = Rig(scenario, A, attach_before_reset=True, mode="exact")
    same(r.state()[0], ref[0], f"{case}: behind mv_reset")
    for t in range(48):
        r.step()
        same(r.state()[0], ref[t + 1], f"{case}: tick {t}")
    same(r.g.get_state_observation(7, A - 1).view(np.uint32), ref[48][7 * A + A - 1], f"{case}: mv_get_state_observation")
    assert len({ref[t].tobytes() for t in range(49)}) == 49, "the oracle's rows never changed: the comparison would prove nothing"
    r.close()


# ---- 2. launch shapes -------------------------------------------------------------------------------------------------------------------------------------
SHAPES = {
    # name: (ring, ticks per call, calls, render, pipelining, overlap)
    "two_resident_launches": (16, 16, 2, "every", True, False), "k3": (6, 3, 4, "every", True, False), "render_none": (16, 16, 2, "none", True, False),
    "render_last": (16, 16, 2, "last", True, False), "not_pipelined": (16, 16, 2, "every", False, False), "overlap": (32, 16, 3, "every", True, True),
}


@pytest.mark.parametrize("scenario", ["TowerBuilding", "HexMemory"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_launch_shapes(hip, scenario, shape):
    """2. batched calls replaying the twin's actions: behind every call, the state ring's entry of each of its ticks is the twin's row of that tick, and
    the reward and done rings hold what the twin (no state buffer) reported"""
    ring, k, calls, render, pipelining, overlap = SHAPES[shape]
    rows, rew, done = twin_rows(scenario)
    r = Rig(scenario, ring=ring, pipelining=pipelining, overlap=overlap)
    r.set_action_ring(TWIN_TICKS)
    def check(ticks, what):
        st = r.state()
        got_rew, got_done = r.rew.cpu().numpy().view(np.uint32), r.done.cpu().numpy()
        for t in ticks:
            same(st[t % ring], rows[t], f"{scenario}, {shape}: {what}, tick {t}, state ring entry {t % ring}")
            same(got_rew[t % ring], rew[t], f"{scenario}, {shape}: {what}, tick {t}, reward ring")
            same(got_done[t % ring], done[t], f"{scenario}, {shape}: {what}, tick {t}, done ring")

    for c in range(calls):
        r.step_n(k, render)
        if not overlap:
            check(range(r.ticks - k, r.ticks), f"call {c}")
    if overlap:   # (the calls back to back, no host wait between them: the ring holds the last 32 ticks)
        check(range(r.ticks - ring, r.ticks), "behind the last call")
    r.close()


@pytest.mark.parametrize("render", ["every", "none", "last"])
def test_launch_shapes_several_agents(hip, render):
    """2, TowerBuilding with two agents per env (every wave of the workgroup ticks; without frame setups nothing but a barrier separates a tick's rows from
    the other waves' next tick): 3 calls of 16 into rings of 16, every tick's rows and rewards are the twin's"""
    rows, rew, _ = twin_rows("TowerBuilding", 2)
    r = Rig("TowerBuilding", 2, ring=16)
    r.set_action_ring(TWIN_TICKS)
    for c in range(3):
        r.step_n(16, render)
        st, got_rew = r.state(), r.rew.cpu().numpy().view(np.uint32)
        for t in range(16 * c, 16 * c + 16):
            same(st[t % 16], rows[t], f"{render}: call {c}, tick {t}")
            same(got_rew[t % 16], rew[t], f"{render}: call {c}, tick {t}, reward ring")
    r.close()


@pytest.mark.parametrize("scenario", ["TowerBuilding", "HexMemory"])
def test_step_no_render(hip, scenario):
    """2. mv_step_no_render, tick by tick, no ring: the one entry holds the twin's row of every tick, the rewards are the twin's"""
    rows, rew, _ = twin_rows(scenario)
    r = Rig(scenario)
    for t in range(12):
        r.step(render=False)
        same(r.state()[0], rows[t], f"{scenario}: tick {t}")
        same(r.g.get_rewards_array().view(np.uint32), rew[t], f"{scenario}: rewards of tick {t}")
    r.close()


# ---- 3. an episode ends inside a resident launch ------------------------------------------------------------------------------------------------------------
SHORT = (("episodeLengthSec", 5.0),)   # 75 ticks where the scenario adds no time of its own: above the 64 ticks below which a gym is stepped tick by tick


@pytest.mark.parametrize("scenario", ["Empty", "Rearrange"])
def test_episode_ends_inside_a_resident_launch(hip, scenario):
    """3. episodes of 75 ticks (scenarios whose episodes are as long as episodeLengthSec says; Empty: the software-pipelined kernel, Rearrange: the one-wave
    one), 6 calls of 16: every row equals the oracle's; the rows of the tick that finishes an episode show the next episode's first state (episode_sec back
    at its start value)"""
    ref, dones = oracle_rows(scenario, 1, 8, 96, SHORT)
    assert dones[:64].sum() == 0 and dones[64:80].any(axis=0).all(), "the oracle's episodes do not end where this test looks"
    r = Rig(scenario, ring=16, params=dict(SHORT))
    assert r.g.recommended_ticks_per_call() > 1   # (batched calls: not the tick-by-tick rule)
    r.set_action_ring(96)
    sec = S.F["episode_sec"]
    for c in range(6):
        r.step_n(16)
        st = r.state()
        for t in range(16 * c, 16 * c + 16):
            same(st[t % 16], ref[t + 1], f"call {c}, tick {t}")
            for e in np.nonzero(dones[t])[0]:
                assert st[t % 16][e][sec] == ref[0][e][sec] and st[t % 16][e].tobytes() != st[(t - 1) % 16][e].tobytes(), f"tick {t}, env {e}: not a spawn state"
    r.close()


# ---- 4. masks and budgets ---------------------------------------------------------------------------------------------------------------------------------
def test_step_mask(hip):
    """4. the odd envs frozen for a 16-tick call: their rows repeat, bit for bit, what they held before it; the even envs' rows follow the twin, whose envs
    step on the same actions (envs are independent of each other)"""
    rows, _, _ = twin_rows("TowerBuilding")
    r = Rig("TowerBuilding", ring=16)
    r.set_action_ring(TWIN_TICKS)
    r.step_n(16)
    same(r.state()[15], rows[15], "before the mask")
    odd = np.arange(8) % 2 == 1
    r.g.set_step_mask(~odd)
    r.step_n(16)
    st = r.state()
    for t in range(16, 32):
        same(st[t % 16][~odd], rows[t][~odd], f"tick {t}: stepping envs")
        same(st[t % 16][odd], rows[15][odd], f"tick {t}: frozen envs")
    r.close()


def test_episode_budget(hip):
    """4. budget 1, episodes of 75 ticks: up to its done an env's rows are the oracle's; from the finishing tick on a halted env's rows stay at its next
    episode's first state -- the oracle's row of the finishing tick"""
    ref, dones = oracle_rows("Empty", 1, 8, 96, SHORT)
    r = Rig("Empty", ring=16, params=dict(SHORT))
    r.g.set_episode_budget(1)
    r.set_action_ring(96)
    ended = np.full(8, -1)
    for c in range(6):
        r.step_n(16)
        st = r.state()
        for t in range(16 * c, 16 * c + 16):
            for e in range(8):
                if ended[e] < 0 and dones[t][e]:
                    ended[e] = t
                want = ref[t + 1][e] if ended[e] < 0 else ref[ended[e] + 1][e]
                same(st[t % 16][e], want, f"tick {t}, env {e} (finished at tick {ended[e]})")
    assert (ended >= 0).all() and r.g.halted_count() == 8
    r.close()


def test_draw_mask(hip):
    """4. half of the envs undrawn: the state rows are the twin's, drawn or not"""
    rows, _, _ = twin_rows("TowerBuilding")
    r = Rig("TowerBuilding", ring=16)
    r.set_action_ring(TWIN_TICKS)
    r.g.set_draw_mask(np.arange(8) % 2 == 0)
    r.step_n(16)
    st = r.state()
    for t in range(16):
        same(st[t], rows[t], f"tick {t}")
    r.step()   # (mv_step: the one-tick kernels)
    same(r.state()[16 % 16], rows[16], "tick 16, mv_step")
    r.close()


# ---- 5. moves ---------------------------------------------------------------------------------------------------------------------------------------------
def test_moves_touch_no_row_until_render(hip):
    """5. fork, resample, load: the rows stay what the last tick left until mv_render (or the next tick) shows the moved state"""
    n = 8
    r = Rig("TowerBuilding")
    for _ in range(6):
        r.step()
    before = r.state()[0].copy()
    same(before, r.snapshot_rows(), "behind 6 ticks")
    assert len({before[e].tobytes() for e in range(n)}) == n, "the envs did not diverge: the moves would prove nothing"
    fork = np.zeros(n, np.int32); fork[0] = -1
    r.g.fork_envs(fork)
    same(r.state()[0], before, "behind the fork, before mv_render")
    r.g.render()
    st = r.state()[0].copy()
    for e in range(n):
        same(st[e], before[0], f"behind the fork and mv_render: env {e}")
    for _ in range(4):   # (different actions per env: the copies diverge again)
        r.step()
    before = r.state()[0].copy()
    assert before[0].tobytes() != before[1].tobytes()
    swap = np.full(n, -1, np.int32); swap[0], swap[1] = 1, 0
    r.g.resample_envs(swap)
    same(r.state()[0], before, "behind the swap, before mv_render")
    r.g.render()
    want = before.copy(); want[0], want[1] = before[1], before[0]
    same(r.state()[0], want, "behind the swap and mv_render")
    same(want, r.snapshot_rows(), "the swapped state itself")
    store = r.g.new_env_store(1)
    save = np.full(n, -1, np.int32); save[2] = 0
    r.g.save_envs(save, store)
    for _ in range(3):
        r.step()
    before = r.state()[0].copy()
    load = np.full(n, -1, np.int32); load[5] = 0
    r.g.load_envs(load, store)
    same(r.state()[0], before, "behind the load, before the next tick")
    r.g.render()
    after = before.copy(); after[5] = want[2]
    same(r.state()[0], after, "behind the load and mv_render")
    r.step()   # (the next stepping call shows moved state too)
    same(r.state()[0], r.snapshot_rows(), "the tick behind the load")
    r.close()
    del store


def test_reset_envs_refreshes_the_flagged_rows_only(hip):
    """5. reset_envs(render=True) of a subset, 6 ticks in: a flagged env's row is the row of an oracle that was reset there, an unflagged env's row is
    untouched -- also where its state has moved since (a fork destination keeps its stale row, as every output does)"""
    n, T0 = 8, 6
    ref, _ = oracle_rows("TowerBuilding", 1, n, 48)
    og = oracle_lib.OracleGym("TowerBuilding", W, H, n, 1, 1, False, None)
    og.seed(ENV_SEED)
    og.reset()
    for t in range(T0):
        masks = action_masks(acts_of(t, n))
        for e in range(n):
            og.set_action_mask(e, 0, int(masks[e]))
        og.step_norender()
    og.reset()
    fresh = S.rows_of_gym_snapshots(og.snapshot, n, 1)
    og.close()
    r = Rig("TowerBuilding")
    for _ in range(T0):
        r.step()
    same(r.state()[0], ref[T0], "before the reset")
    fork = np.full(n, -1, np.int32); fork[7] = 6   # (env 7's state moves; its row must not)
    r.g.fork_envs(fork)
    flagged = np.zeros(n, bool); flagged[[0, 3, 4]] = True
    r.g.reset_envs(flagged, render=True)
    st = r.state()[0]
    same(st[flagged], fresh[flagged], "flagged envs")
    same(st[~flagged], ref[T0][~flagged], "unflagged envs")
    assert fresh[flagged].tobytes() != ref[T0][flagged].tobytes()
    r.close()


# ---- 6. ragged sizes --------------------------------------------------------------------------------------------------------------------------------------
def test_ragged_sizes(hip):
    """6. 130 envs x 2 agents, 8 ticks with one call: 260 rows, 4160 words -- the publish launch's blocks end in a ragged tail; every row is the table applied
    to mv_debug_snapshot of its env behind the call"""
    r = Rig("TowerBuilding", A=2, n=130)
    r.g.step_n(8, "multidiscrete", POLICY_SEED, 0)
    st = r.state()[0]
    same(st, r.snapshot_rows(), "behind step_n(8)")
    assert len({st[i].tobytes() for i in range(260)}) > 200
    r.close()


# ---- 7. identity ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mv_step_short_episodes", "batched"])
def test_identity(hip, case):
    """7. a gym with the buffer attached and a twin without, 64 ticks each, exact pixels, the episode log on: rewards, dones, true objectives, pixels, status
    words and the drained log are identical; the sentinel past the buffer's last row is intact (Rig.state)"""
    kw = dict(mode="exact", log=4096, A=2)
    if case == "mv_step_short_episodes":   # (Empty: its episodes are as long as episodeLengthSec says, 30 ticks)
        scenario = "Empty"
        kw.update(params={"episodeLengthSec": 2.0})
    else:
        scenario = "TowerBuilding"
        kw.update(ring=16)
    a, b = Rig(scenario, **kw), Rig(scenario, state=False, **kw)

    def compare(what):
        a.state(); b.sync()
        # (status words: the per-env consumed counts, the project's stand-in -- the word with the ST_* flag bits has no read hook; a raised flag would
        # surface as a warning of the stepping calls above, which Rig.step asserts on and step_n turns into a RuntimeWarning)
        for name in ("get_rewards_array", "get_dones", "get_true_objectives", "debug_episodes_consumed"):
            assert getattr(a.g, name)().tobytes() == getattr(b.g, name)().tobytes(), f"{what}: {name}"
        for x, y, n in ((a.slab, b.slab, "slab"), (a.obs, b.obs, "observation ring"), (a.rew, b.rew, "reward ring"), (a.done, b.done, "done ring")):
            assert (x is None and y is None) or x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"{what}: {n}"
        bad = [e for e in range(a.n) if a.g.debug_snapshot_bytes(e).tobytes() != b.g.debug_snapshot_bytes(e).tobytes()]
        assert not bad, f"{what}: state of envs {bad}"

    if case == "mv_step_short_episodes":
        for t in range(64):
            a.step(); b.step()
            compare(f"tick {t}")
    else:
        for c in range(4):
            for r in (a, b):
                r.g.step_n(16, "multidiscrete", POLICY_SEED, 16 * c)
            compare(f"call {c}")
    la, lb = a.g.drain_episode_log(), b.g.drain_episode_log()
    assert la.tobytes() == lb.tobytes() and a.g.episode_log_dropped == b.g.episode_log_dropped
    if case == "mv_step_short_episodes":
        assert la.size > 0, "no episode ended: the log comparison would prove nothing"
    a.close(); b.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """8. a member of a group; mv_group_create / mv_step_many with an attached gym (nothing stepped), valid again after detach; mv_set_output_ring while
    attached; a wrong shape / dtype / device; detach restores the unmasked kernels' launches; a closed gym"""
    import torch
    n = 8
    ra, rb, fresh = Rig("TowerBuilding"), Rig("ObstaclesEasy", state=False), Rig("TowerBuilding", state=False)
    a, b = ra.g, rb.g
    lib = a._lib
    snaps = lambda g: [g.debug_snapshot_bytes(e).tobytes() for e in range(n)]   # noqa: E731
    handles = (C.c_void_p * 2)(a._g, b._g)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == -1 and b"state observations" in lib.mv_last_error()
    before = snaps(a), snaps(b)
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) == -1 and b"state observations" in lib.mv_last_error()
    assert (snaps(a), snaps(b)) == before, "mv_step_many stepped a gym before it refused"
    ring = torch.zeros((4, n), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="detach the state observations first"):
        a.set_output_ring(4, 0, ring.data_ptr(), 0)
    for bad in (torch.zeros((1, n, 15), dtype=torch.float32, device=DEV), torch.zeros((2, n, 16), dtype=torch.float32, device=DEV),
                torch.zeros((1, n, 16), dtype=torch.float64, device=DEV), torch.zeros((1, n, 16), dtype=torch.float32),
                torch.zeros((1, n, 32), dtype=torch.float32, device=DEV)[:, :, ::2], np.zeros((1, n, 16), np.float32)):
        with pytest.raises(ValueError, match="set_state_obs"):
            a.set_state_obs(bad)
    assert a.state_obs() is not None and lib.mv_get_state_obs(a._g) == 1
    # detached: the launches of a gym that never had a buffer, call for call, and no row written any more
    assert a.set_state_obs(None) is None and a.state_obs() is None and lib.mv_get_state_obs(a._g) == 0
    held = ra.state().copy()
    for r in (ra, fresh):
        c0 = r.g.debug_launch_counts()
        r.step()
        r.g.step_n(8, "multidiscrete", POLICY_SEED, 1)
        r.g.step_n(8, "multidiscrete", POLICY_SEED, 9, render="none")
        c1 = r.g.debug_launch_counts()
        r.counts = (c1[0] - c0[0], c1[1] - c0[1])
    assert ra.counts == fresh.counts
    same(ra.state(), held, "rows written after the detach")
    with pytest.raises(RuntimeError, match="no state observations attached"):
        a.get_state_observation(0, 0)
    a.set_output_ring(4, 0, ring.data_ptr(), 0)   # (allowed again)
    a.set_output_ring(0)
    ra.sync(); rb.sync()
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) >= 0, lib.mv_last_error()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    for g in (a, b):
        assert lib.mv_set_state_obs(g._g, C.c_void_p(ra.buf.data_ptr())) == -1 and b"mv_group" in lib.mv_last_error()
        assert lib.mv_get_state_obs(g._g) == 0
        with pytest.raises(RuntimeError, match="mv_group"):
            g.set_state_obs(True)
    assert lib.mv_group_destroy(grp) == 0
    ra.attach()   # (valid again once the group is gone)
    ra.step()
    same(ra.state()[0], ra.snapshot_rows(), "attached again")
    with pytest.raises(RuntimeError, match="index out of range"):
        a.get_state_observation(n, 0)
    ra.sync()
    handle = a._g
    lib.mv_close(handle)
    out = np.zeros(16, np.float32)
    assert lib.mv_set_state_obs(handle, C.c_void_p(ra.buf.data_ptr())) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_state_obs(handle) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_state_observation(handle, 0, 0, out.ctypes.data) == -1 and b"closed" in lib.mv_last_error()
    a.close(); rb.close(); fresh.close()


# ---- the MegaverseEnv surface -----------------------------------------------------------------------------------------------------------------------------
def test_env_state_obs(hip):
    """MegaverseEnv(..., state_obs=True): state_obs() is the last tick's [num_agents, 16] device view through reset, step_device and step_sequence (whose
    rings the env swaps under the buffer), equal to the table applied to the gym's debug snapshots"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("TowerBuilding", 4, 2, img_w=W, img_h=H, state_obs=True)
    env.seed(ENV_SEED)
    env.reset()

    def check(what):
        rows = env.state_obs()
        assert rows.shape == (8, 16) and rows.is_cuda and rows.dtype == torch.float32
        env.env.synchronize(); torch.cuda.synchronize()
        same(rows.cpu().numpy().view(np.uint32), S.rows_of_gym_snapshots(lambda e: hip_snapshot(env.env, e), 4, 2), what)

    check("behind reset")
    env.step_device(acts_of(0, 8))
    check("behind step_device")
    acts = np.stack([acts_of(t, 8) for t in range(1, 6)])
    env.step_sequence(acts)
    check("behind step_sequence")
    assert env.env.state_obs().shape == (5, 8, 16)
    env.step_device(acts_of(6, 8))
    check("behind step_device again")
    assert env.state_obs()[:, env.STATE_OBS_FIELDS["pos_y"]].min().item() > 0.0
    env.close()
