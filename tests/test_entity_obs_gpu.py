"""Entity observations on the GPU (include/megaverse_hip.h: mv_set_entity_obs): E rows of 8 float32 per ENV for every tick of every stepping call, in the ring
entry of its tick.

Every comparison is equality of uint32 views, bit for bit.  What a row must hold comes from outside the feature: the record's table restated in numpy
(entity_obs_util) applied to the CPU oracle's snapshot, which is stepped on the same scripted actions -- or, where no oracle runs beside the gym, to the gym's
own debug snapshot.  Shapes are the smallest that reach every path: 3 envs, 32 x 32 pixels, 1, 2 and 4 agents (the one-wave, two-wave and several-agent step
kernels), calls of 9 ticks (two resident step launches)."""
import ctypes as C
import functools

import numpy as np
import pytest

import entity_obs_util as EU
import episode_log_util as U
import football_cases as FC
import oracle_lib
from hip_util import hip_snapshot
from megaverse_amd import entity_layout, entity_row_of, entity_rows
from megaverse_amd.extension import ENTITY_OBS_FIELDS, MegaverseGym, seg_split
from megaverse_amd.rollout import action_masks

pytestmark = pytest.mark.gpu

ENV_SEED, POLICY_SEED = 42, 7
W = H = 32
N, K = 3, 9
DEV = "cuda:0"
SENT = 0xA5A5A5A5 - (1 << 32)   # (as an int32: the sentinel's bits in every word the gym must not write)
SINGLE, RING_CALLS = 6, ("every", "last", "none")
TICKS = SINGLE + K * len(RING_CALLS)
# HexExplore, Football, Empty: episodes of 1.5 s = 22 ticks, so the second call of 9 (ticks 15..23) holds a natural reset at its tick 7
PARAMS = {"HexExplore": {"episodeLengthSec": 1.5}, "Football": {"episodeLengthSec": 1.5}, "Empty": {"episodeLengthSec": 1.5}}


def acts_of(tick, rows):
    return EU.scripted_actions(POLICY_SEED, tick, rows)


class Rig:
    """one gym; optionally output rings of `ring` entries and an entity buffer with one entry more than the gym is given: the extra one must keep the sentinel"""

    def __init__(self, scenario, A=1, n=N, ring=0, entity=True, scene=False, state=False, mode="fast", params=None, attach_before_reset=False):
        import torch
        U.boxoban_env()
        self.scenario, self.A, self.n, self.rows = scenario, A, n, n * A
        self.g = g = MegaverseGym(scenario, W, H, n, A, 1, False, dict(PARAMS.get(scenario, {}) if params is None else params))
        g.set_pixel_mode(mode)
        g.seed(ENV_SEED)
        self.E = entity_rows(scenario, A)
        assert g.entity_rows() == self.E and g.entity_layout() == entity_layout(scenario, A)
        table = np.zeros((4, 3), np.int32)   # (mv_entity_obs_layout against the model's table: base row, rows, class of the group's first kind)
        assert g._lib.mv_entity_obs_layout(g._g, table.ctypes.data) == 0 and table.tolist() == [list(v) for v in EU.layout(scenario, A)[0].values()]
        self.slab = torch.zeros((self.rows, H, W, 4), dtype=torch.uint8, device=DEV)
        self.want_entity, self.want_scene, self.want_state = entity, scene, state
        self.buf = self.obs = self.rew = self.done = None
        torch.cuda.synchronize()
        g.set_obs_buffer(self.slab.data_ptr())
        self.ring = 0
        if attach_before_reset:
            self.attach()
        g.reset()
        if ring:
            self.set_ring(ring)
        elif not attach_before_reset:
            self.attach()
        self.ticks = 0

    def set_ring(self, ring):
        """output rings of `ring` entries (0: none); the row records are detached around the change and attached again at the new depth"""
        import torch
        self.sync()
        for setter in (self.g.set_entity_obs, self.g.set_scene_obs, self.g.set_state_obs):
            setter(None)
        self.ring = ring
        self.obs = torch.zeros((ring, self.rows, H, W, 4), dtype=torch.uint8, device=DEV) if ring else None
        self.rew = torch.full((ring, self.rows), -7.0, dtype=torch.float32, device=DEV) if ring else None
        self.done = torch.full((ring, self.n), 9, dtype=torch.uint8, device=DEV) if ring else None
        torch.cuda.synchronize()
        if ring:
            self.g.set_output_ring(ring, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        else:
            self.g.set_output_ring(0)
        self.attach()

    def attach(self):
        import torch
        self.entries = max(1, self.ring)
        if self.want_entity:
            self.buf = torch.full((self.entries + 1, self.n, self.E, 8), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
            torch.cuda.synchronize()
            got = self.g.set_entity_obs(self.buf[:self.entries])
            assert got.data_ptr() == self.buf.data_ptr() and self.g.entity_obs_ring() is got
            assert self.g._lib.mv_get_entity_obs(self.g._g) == self.entries
        if self.want_scene:
            self.g.set_scene_obs(True)
        if self.want_state:
            self.g.set_state_obs(True)

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def entity(self):
        """-> uint32 [entries, n, E, 8], after checking that the entry past the last one still holds the sentinel"""
        self.sync()
        x = self.buf.cpu().numpy().view(np.uint32)
        assert (x[self.entries] == 0xA5A5A5A5).all(), "the gym wrote past the last entry of the entity buffer"
        return x[:self.entries]

    def truth(self):
        """the model applied to mv_debug_snapshot (and the ball's debug hook) of every env -> uint32 [n, E, 8]"""
        self.sync()
        ball = (lambda e: FC.record(self.g.debug_football_state(e))) if self.scenario == "Football" else None
        return EU.rows_of(self.scenario, self.A, lambda e: hip_snapshot(self.g, e), self.n, ball)

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

    def step_n(self, k=K, render="every"):
        self.g.step_n(k, "sequence", POLICY_SEED, self.ticks, render=render)
        self.ticks += k

    def plant(self):
        """every word of the entity buffer back to the sentinel"""
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


def set_masks(og, acts, n, A):
    masks = action_masks(acts)
    for e in range(n):
        for a in range(A):
            og.set_action_mask(e, a, int(masks[e * A + a]))


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(scenario, A, ticks=TICKS, hold=False):
    """the oracle, 3 envs, stepped `ticks` times on acts_of(t) (hold: on acts_of(0) every tick -- a macro step's held actions) -> (rows uint32
    [ticks + 1, 3, E, 8]: [0] behind the reset, [t + 1] behind tick t; dones uint8 [ticks, 3]).  Computed once per case and shared, read-only"""
    U.boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, PARAMS.get(scenario))
    og.seed(ENV_SEED)
    og.reset()
    rows, dones = [EU.rows_of(scenario, A, og.snapshot, N, og.football_state)], []
    for t in range(ticks):
        set_masks(og, acts_of(0 if hold else t, N * A), N, A)
        og.step_norender()
        rows.append(EU.rows_of(scenario, A, og.snapshot, N, og.football_state))
        dones.append(np.asarray(og.get_dones(), np.uint8).copy())
    og.close()
    out = np.stack(rows), np.stack(dones)
    for x in out:
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("A", [1, 2, 4])
@pytest.mark.parametrize("scenario", EU.SCENARIOS)
def test_against_the_oracle(hip, scenario, A):
    """1. the rows behind mv_reset, behind 3 ticks of mv_step and 3 of mv_step_no_render, and EVERY ring entry of three calls of 9 ticks (policy `sequence`,
    the action ring scripted as the oracle's masks) in render modes every, last and none: the model applied to the oracle's snapshot of the same tick"""
    want, dones = oracle_rows(scenario, A)
    r = Rig(scenario, A, attach_before_reset=True)
    what = f"{scenario}, {A} agents"
    same(r.entity()[0], want[0], f"{what}: behind mv_reset")
    for t in range(SINGLE):
        r.step(render=t < SINGLE // 2)
        same(r.entity()[0], want[t + 1], f"{what}: tick {t}, {'mv_step' if t < SINGLE // 2 else 'mv_step_no_render'}")
        assert r.g.get_dones().tolist() == dones[t].tolist()
    same(r.g.get_entity_observation(N - 1).view(np.uint32), want[SINGLE][N - 1], f"{what}: mv_get_entity_observation")
    r.set_ring(K)
    r.set_action_ring(TICKS)
    for c, render in enumerate(RING_CALLS):
        r.step_n(K, render)
        got = r.entity()
        for j in range(K):
            t = SINGLE + c * K + j
            same(got[j], want[t + 1], f"{what}: step_n(9, {render}), tick {t}, entry {j}")
        assert r.done.cpu().numpy().tolist() == dones[SINGLE + c * K:SINGLE + (c + 1) * K].tolist()
    assert len({want[t].tobytes() for t in range(TICKS + 1)}) > TICKS // 2, "the rows barely changed: the comparison would prove less than it says"
    r.close()


@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 1), ("ObstaclesHard", 2), ("Collect", 1), ("Sokoban", 2), ("HexMemory", 4), ("Football", 1)])
def test_macro_step_against_the_oracle(hip, scenario, A):
    """1. mv_macro_step of 5 ticks, the actions held: its single entry holds the rows behind its last tick; no env finishes inside it (asserted on the oracle)"""
    want, dones = oracle_rows(scenario, A, 5, True)
    assert not dones.any()
    for render in ("last", "none"):
        r = Rig(scenario, A)
        r.plant()
        r.g.macro_step(5, acts_of(0, N * A), None, render=render)
        same(r.entity()[0], want[5], f"{scenario}, {A} agents: macro_step(5, {render})")
        r.close()


@pytest.mark.parametrize("scenario,A", [("Football", 2), ("Empty", 1), ("HexExplore", 4)])
def test_reset_inside_a_call(hip, scenario, A):
    """2. episodes of 22 ticks and calls of 9 from tick 0: every env resets at tick j = 4 of the third call.  Entries before j show the old episode, entry j and
    those after it the new one -- the rows are written by the tick itself"""
    want, dones = oracle_rows(scenario, A)
    r = Rig(scenario, A, ring=K)
    r.set_action_ring(TICKS)
    for c in range(3):
        r.step_n(K, "none" if c % 2 else "every")
        got = r.entity()
        for j in range(K):
            same(got[j], want[c * K + j + 1], f"{scenario}: call {c}, entry {j}")
    j = np.flatnonzero(dones[2 * K:3 * K].all(axis=1))
    assert j.tolist() == [4], f"the reset is not where the test expects it: {dones[:3 * K].tolist()}"
    agents = entity_layout(scenario, A)["agents"]
    assert (got[3, :, agents] != got[4, :, agents]).any() and r.done.cpu().numpy()[4].all()
    r.close()


# ---- 3. step masks and budgets ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 2), ("Collect", 1)])
def test_step_mask(hip, scenario, A):
    """3. env 1 frozen for a call of 9: each of its entries equals its rows of the tick before; the stepping envs' entries equal an unmasked twin's"""
    a, b = Rig(scenario, A, ring=K), Rig(scenario, A, ring=K)
    for r in (a, b):
        r.set_action_ring(2 * K)
        r.step_n(K)
    held = a.entity()[K - 1].copy()
    same(held, b.entity()[K - 1], "before the mask")
    same(held, a.truth(), "before the mask: the snapshot")
    steps = np.array([True, False, True])
    a.g.set_step_mask(steps)
    a.step_n(K); b.step_n(K)
    ga, gb = a.entity(), b.entity()
    for j in range(K):
        same(ga[j][1], held[1], f"entry {j}: the frozen env")
        same(ga[j][steps], gb[j][steps], f"entry {j}: the stepping envs against the twin")
    assert (gb[K - 1][1] != held[1]).any(), "the twin's env 1 did not move: freezing it shows nothing"
    a.close(); b.close()


def test_episode_budget(hip):
    """3. Empty, episodes of 22 ticks, budget 1 for env 2, calls of 9: env 2 halts inside the third call and repeats the rows of its finishing tick -- the
    first state of its next episode -- in every later entry; the other envs equal an unbudgeted twin's"""
    a, b = Rig("Empty", 2, ring=K), Rig("Empty", 2, ring=K)
    a.g.set_episode_budget(np.array([-1, -1, 1], np.int32))
    halted_at, row = -1, None
    for r in (a, b):
        r.set_action_ring(5 * K)
    for c in range(5):
        a.step_n(K); b.step_n(K)
        ga, gb, done = a.entity(), b.entity(), a.done.cpu().numpy()
        for j in range(K):
            same(ga[j][:2], gb[j][:2], f"call {c}, entry {j}: the envs without a budget against the twin")
            if halted_at >= 0:
                same(ga[j][2], row, f"call {c}, entry {j}: halted at tick {halted_at}")
            else:
                same(ga[j][2], gb[j][2], f"call {c}, entry {j}: env 2 before it halts")
                if done[j][2]:
                    halted_at, row = c * K + j, ga[j][2].copy()
    assert halted_at == 22 and a.g.halted_count() == 1
    a.close(); b.close()


# ---- 4. refresh and non-refresh --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesHard"])
def test_refresh_and_moves(hip, scenario):
    """4. mv_reset and mv_render refresh every row; reset_envs(mask, render=1) the flagged envs' rows only, the others keep planted bytes; forks, resampling
    and loads change no byte until the next tick"""
    r = Rig(scenario, 2)
    for _ in range(4):
        r.step()
    same(r.entity()[0], r.truth(), "behind 4 ticks")
    r.plant()
    r.g.render()
    same(r.entity()[0], r.truth(), "mv_render refreshes every row")
    r.plant()
    flagged = np.array([False, True, False])
    r.g.reset_envs(flagged, render=True)
    got, want = r.entity()[0], r.truth()
    same(got[flagged], want[flagged], "reset_envs: the flagged rows")
    assert (got[~flagged] == 0xA5A5A5A5).all(), "reset_envs wrote an unflagged env's row"
    r.plant()
    r.g.reset_envs(flagged, render=False)
    assert (r.entity()[0] == 0xA5A5A5A5).all(), "reset_envs(render=0) wrote a row"
    r.g.reset()
    same(r.entity()[0], r.truth(), "mv_reset refreshes every row")
    for _ in range(3):
        r.step()
    r.plant()
    fork = np.full(N, -1, np.int32); fork[1] = 0
    r.g.fork_envs(fork)
    swap = np.full(N, -1, np.int32); swap[0], swap[2] = 2, 0
    r.g.resample_envs(swap)
    store = r.g.new_env_store(1)
    slot = np.full(N, -1, np.int32); slot[2] = 0
    r.g.save_envs(slot, store)
    slot = np.full(N, -1, np.int32); slot[1] = 0
    r.g.load_envs(slot, store)
    assert (r.entity()[0] == 0xA5A5A5A5).all(), "a fork, a resample or a load wrote a row"
    r.step()
    same(r.entity()[0], r.truth(), "the next tick shows the moved state")
    r.close()
    del store


# ---- 5. launches -------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_publication_launch_and_nothing_else_moves(hip):
    """5. state + scene + entity attached: mv_debug_launch_counts out[1] grows per call by what it grows with scene alone (ONE publication launch); with
    nothing attached the counts equal a never-attached twin's, and so do its rewards, dones and pixels"""
    kw = dict(A=2, ring=K, mode="exact")
    a, b = Rig("ObstaclesHard", scene=True, state=True, **kw), Rig("ObstaclesHard", entity=False, **kw)
    for r in (a, b):
        r.set_action_ring(4 * K)

    def call(r):
        c0 = np.array(r.g.debug_launch_counts())
        r.step_n(K)
        r.sync()
        return np.array(r.g.debug_launch_counts()) - c0

    both, none = call(a), call(b)
    same(a.entity()[K - 1], a.truth(), "all three attached")
    a.g.set_entity_obs(None); a.g.set_state_obs(None)
    scene = call(a); call(b)
    assert both.tolist() == scene.tolist() and both[1] == none[1] + 1 and both[0] == none[0], (both, scene, none)
    a.g.set_scene_obs(None)
    detached, twin = call(a), call(b)
    assert detached.tolist() == twin.tolist() == none.tolist(), (detached, twin, none)
    for x, y, nm in ((a.slab, b.slab, "slab"), (a.obs, b.obs, "observation ring"), (a.rew, b.rew, "reward ring"), (a.done, b.done, "done ring")):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"detached against never attached: {nm}"
    assert [a.g.debug_snapshot_bytes(e).tobytes() for e in range(N)] == [b.g.debug_snapshot_bytes(e).tobytes() for e in range(N)]
    a.close(); b.close()


# ---- 6. the labels ---------------------------------------------------------------------------------------------------------------------------------------------
LABEL_TICKS = 12
NO_ENTITY_CLASSES = ("BoxAGone", "Empty")   # (their rows are the agents': nothing else to see)


@pytest.mark.parametrize("scenario", EU.SCENARIOS)
def test_labels_index_the_rows(hip, scenario):
    """6. exact pixels, instance planes attached, 12 ticks of mv_step, two agents: for every pixel whose class has rows, entity_row_of(word) names a row of
    the pixel's env whose column 0 equals the word; Sokoban's EXIT is found by searching the goal rows.  The frames show such pixels, of a non-agent class
    where the scenario has one"""
    A = 2
    r = Rig(scenario, A, mode="exact")
    seg = r.g.set_seg_obs(True, "instance")
    K_ = EU.K
    seen = {}
    terrain = entity_layout(scenario, A)["terrain"]
    for t in range(LABEL_TICKS):
        r.step()
        rows = r.entity()[0]
        r.sync()
        planes = seg[0].cpu().numpy().view(np.uint16).reshape(N, A * H * W)
        for e in range(N):
            words = np.unique(planes[e])
            where = entity_row_of(words.view(np.int16), scenario, A)
            cls, _ = seg_split(words)
            for w, row, c in zip(words.tolist(), where.tolist(), cls.tolist()):
                if scenario == "Sokoban" and c == K_["EXIT"]:
                    assert row == -1
                    hit = np.flatnonzero(rows[e, terrain, 0] == EU.of_int(w)[0])
                    assert hit.size == 1, f"tick {t}, env {e}: goal pad {w:#x} is in {hit.size} rows"
                    row = terrain.start + int(hit[0])
                if row >= 0:
                    assert rows[e, row, 0] == EU.of_int(w)[0], f"tick {t}, env {e}: word {w:#x} names row {row}, which holds {rows[e, row].tolist()}"
                    seen[c] = seen.get(c, 0) + 1
                else:
                    assert c in (K_["NONE"], K_["FLOOR"], K_["STRUCTURE"], K_["FURNITURE"], K_["HUD"]), f"tick {t}, env {e}: word {w:#x} has no row"
    assert seen, "no pixel of a class with rows"
    if scenario not in NO_ENTITY_CLASSES:
        assert set(seen) - {K_["AGENT"]}, f"only agents were seen: {seen}"
    r.close()


# ---- 7. refusals and surface -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """7. mv_group_create / mv_step_many with an attached gym (nothing stepped); a member of a group; mv_set_output_ring while attached; a NULL gym; a
    misaligned buffer; a wrong shape; an index out of range: -1 with text, and nothing changed"""
    import torch
    ra, rb = Rig("TowerBuilding", entity=False), Rig("ObstaclesEasy", entity=False)
    a, b = ra.g, rb.g
    lib = a._lib
    arena0 = a.arena_bytes()
    ra.want_entity = True
    ra.attach()
    snaps = lambda g: [g.debug_snapshot_bytes(e).tobytes() for e in range(N)]   # noqa: E731
    handles = (C.c_void_p * 2)(a._g, b._g)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == -1 and b"mv_set_entity_obs" in lib.mv_last_error()
    before = snaps(a), snaps(b)
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) == -1 and b"mv_set_entity_obs" in lib.mv_last_error()
    assert (snaps(a), snaps(b)) == before, "mv_step_many stepped a gym before it refused"
    ring = torch.zeros((4, N), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="detach the entity observations first"):
        a.set_output_ring(4, 0, ring.data_ptr(), 0)
    assert lib.mv_set_entity_obs(None, C.c_void_p(ra.buf.data_ptr())) == -1 and b"null gym" in lib.mv_last_error()
    ra.step()
    held = ra.entity().copy()
    assert lib.mv_set_entity_obs(a._g, C.c_void_p(ra.buf.data_ptr() + 4)) == -1 and b"16-byte aligned" in lib.mv_last_error()
    assert lib.mv_get_entity_obs(a._g) == 1 and a.entity_obs_ring() is not None
    E = ra.E
    for bad in (torch.zeros((1, N, E, 7), dtype=torch.float32, device=DEV), torch.zeros((2, N, E, 8), dtype=torch.float32, device=DEV),
                torch.zeros((1, N, E + 1, 8), dtype=torch.float32, device=DEV), torch.zeros((1, N, E, 8), dtype=torch.float64, device=DEV),
                torch.zeros((1, N, E, 8), dtype=torch.float32), np.zeros((1, N, E, 8), np.float32)):
        with pytest.raises(ValueError, match="set_entity_obs"):
            a.set_entity_obs(bad)
    for env in (N, -1):
        with pytest.raises(RuntimeError, match="index out of range"):
            a.get_entity_observation(env)
    ra.step()   # (the refused calls left the buffer attached: the next tick writes it)
    assert (ra.entity() != held).any()
    same(ra.entity()[0], ra.truth(), "behind the refusals")
    arena = a.arena_bytes()
    assert a.set_entity_obs(None) is None and a.entity_obs() is None and lib.mv_get_entity_obs(a._g) == 0
    with pytest.raises(RuntimeError, match="no entity observations attached"):
        a.get_entity_observation(0)
    staged = arena - arena0
    assert a.arena_bytes() == arena and staged > 0 and staged % (N * E * 32) == 0   # (the staging rows, slots x N x E x 32 bytes, stay counted until mv_close)
    ra.sync(); rb.sync()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    for g in (a, b):
        assert lib.mv_set_entity_obs(g._g, C.c_void_p(ra.buf.data_ptr())) == -1 and b"mv_group" in lib.mv_last_error()
        assert lib.mv_get_entity_obs(g._g) == 0
    assert lib.mv_group_destroy(grp) == 0
    ra.close(); rb.close()


def test_env_entity_obs(hip):
    """MegaverseEnv(..., entity_obs=True): entity_obs() is the last tick's [num_envs, E, 8] device view through reset, step_device and step_sequence (whose
    rings the env swaps under the buffer), with columns looked up through ENTITY_OBS_FIELDS and rows through entity_layout"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("ObstaclesEasy", N, 2, img_w=W, img_h=H, entity_obs=True, scene_obs=True)
    env.seed(ENV_SEED)
    env.reset()
    assert env.ENTITY_OBS_FIELDS is ENTITY_OBS_FIELDS
    E = entity_rows("ObstaclesEasy", 2)

    def check(what):
        rows = env.entity_obs()
        assert rows.shape == (N, E, 8) and rows.is_cuda and rows.dtype == torch.float32
        env.env.synchronize(); torch.cuda.synchronize()
        want = EU.rows_of("ObstaclesEasy", 2, lambda e: hip_snapshot(env.env, e), N)
        same(rows.cpu().numpy().view(np.uint32), want, what)
        same(env.env.entity_obs().cpu().numpy().view(np.uint32), want, what + ": MegaverseGym.entity_obs()")
        return rows

    check("behind reset")
    env.step_device(acts_of(0, 2 * N))
    check("behind step_device")
    env.step_sequence(np.stack([acts_of(t, 2 * N) for t in range(1, 6)]))
    rows = check("behind step_sequence")
    assert env.env.entity_obs_ring().shape == (5, N, E, 8)
    lay = entity_layout("ObstaclesEasy", 2)
    assert (rows[:, lay["agents"], ENTITY_OBS_FIELDS["seg_word"]] == torch.tensor([13 << 12, (13 << 12) + 1], device=DEV)).all()
    assert (rows[:, lay["terrain"], ENTITY_OBS_FIELDS["seg_word"]] != 0).any()
    env.close()
