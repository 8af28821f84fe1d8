"""Still frames on the GPU (include/megaverse_hip.h: mv_set_still_frames): envs that did not change are not drawn again, and every byte stays what it is
without the option.

Every test runs two gyms with the same seed through the same calls: one with still frames on, its twin with the option off.  Behind every call every
observation byte (the slab AND every ring entry), the reward and done rings, rewards, dones, true objectives and the debug snapshot of every env must equal
the twin's.  That frames were skipped and not redrawn is shown separately: in the slab a sentinel planted before the call survives in a still env's rows; in a
ring a pattern planted in the still env's home row appears in its rows of the call's entries.  Comparisons are equality of bytes."""
import numpy as np
import pytest

import episode_log_util as U
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import sample_actions

pytestmark = pytest.mark.gpu

ENV_SEED, POLICY_SEED = 42, 1234
SENT = 0xA5
DEV = "cuda:0"
N = 12


class Rig:
    """one gym and the torch buffers its observations (slab, ring), rewards and dones go to"""

    def __init__(self, scenario="TowerBuilding", A=1, n=N, w=64, h=64, mode="fast", ring=0, layout="rgba", params=None, still=False, overlap=False,
                 gym=None, log=0):
        import torch
        U.boxoban_env()
        self.A, self.R, self.ticks, self.still = A, ring, 0, still
        if gym is None:
            self.g = g = MegaverseGym(scenario, w, h, n, A, 1, False, dict(params or {}))
            g.set_pixel_mode(mode)
            if layout == "chw":
                g.set_obs_layout("chw")
            g.seed(ENV_SEED)
            if log:
                g.set_episode_log(log)
        else:   # (a gym another test's helper made and reset)
            self.g = g = gym
            n = g.num_envs
        self.n = n
        fs = (3, h, w) if layout == "chw" else (h, w, 4)
        self.slab = torch.full((n * A,) + fs, SENT, dtype=torch.uint8, device=DEV)
        self.obs = torch.full((ring, n * A) + fs, SENT, dtype=torch.uint8, device=DEV) if ring else None
        self.rew = torch.full((ring, n * A), -7.0, dtype=torch.float32, device=DEV) if ring else None
        self.done = torch.full((ring, n), 9, dtype=torch.uint8, device=DEV) if ring else None
        torch.cuda.synchronize()
        g.set_obs_buffer(self.slab.data_ptr())
        if gym is None:
            g.reset()
        if ring:   # (attached behind the reset: tick t of the calls that follow goes to entry t % R)
            g.set_output_ring(ring, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        if overlap:
            g.set_pass_overlap(True)
        if still:
            assert g.still_frames() is False
            g.set_still_frames(True)
            assert g.still_frames() is True

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def step(self, act=None):
        if act is None:
            self.g.sample_random_actions(POLICY_SEED, self.ticks)
        else:
            self.g.set_actions_batched(act)
        assert self.g._lib.mv_step(self.g._g) >= 0, self.g._lib.mv_last_error()
        self.ticks += 1
        return [(self.ticks - 1) % self.R] if self.R else []

    def step_n(self, k, render="every"):
        """-> the ring entries of the call's ticks"""
        self.g.step_n(k, "multidiscrete", POLICY_SEED, self.ticks, render=render)
        entries = [(self.ticks + j) % self.R for j in range(k)] if self.R else []
        self.ticks += k
        return entries

    def macro(self, k, c, ticks=None, render="last"):
        """-> the ring entry of the call"""
        acts = np.ascontiguousarray(sample_actions(POLICY_SEED, 50000 + c, self.n * self.A), np.int32).reshape(self.n * self.A, 6)
        self.g.macro_step(k, acts, ticks=None if ticks is None else np.asarray(ticks, np.int32), render=render)
        self.ticks += 1
        return [(self.ticks - 1) % self.R] if self.R else []

    def launches(self):
        return np.array(self.g.debug_launch_counts(), np.int64)

    def close(self):
        self.sync()
        self.g.close()


def pair(*args, **kw):
    """(the gym with still frames on, its twin)"""
    return Rig(*args, still=True, **kw), Rig(*args, still=False, **kw)


def rows_of(envs, A):
    return np.repeat(np.asarray(envs, bool), A)


def same(m, t, what, skip_envs=None):
    """every observation byte of the slab and of every ring entry (skip_envs: but the rows of envs a test planted bytes in), the reward and done rings,
    rewards, dones, true objectives and the snapshot of every env: the twin's"""
    m.sync(); t.sync()
    keep = ~rows_of(skip_envs if skip_envs is not None else np.zeros(m.n, bool), m.A)
    a, b = m.slab.cpu().numpy(), t.slab.cpu().numpy()
    bad = [int(r) for r in np.nonzero(keep)[0] if a[r].tobytes() != b[r].tobytes()]
    assert not bad, f"{what}: slab rows {bad} differ from the twin's"
    if m.R:
        a, b = m.obs.cpu().numpy(), t.obs.cpu().numpy()
        bad = [(j, int(r)) for j in range(m.R) for r in np.nonzero(keep)[0] if a[j, r].tobytes() != b[j, r].tobytes()]
        assert not bad, f"{what}: ring (entry, row) {bad} differ from the twin's"
        assert m.rew.cpu().numpy().tobytes() == t.rew.cpu().numpy().tobytes(), f"{what}: reward ring"
        assert m.done.cpu().numpy().tobytes() == t.done.cpu().numpy().tobytes(), f"{what}: done ring"
    for name in ("get_rewards_array", "get_dones", "get_true_objectives"):
        assert getattr(m.g, name)().tobytes() == getattr(t.g, name)().tobytes(), f"{what}: {name}"
    bad = [e for e in range(m.n) if m.g.debug_snapshot_bytes(e).tobytes() != t.g.debug_snapshot_bytes(e).tobytes()]
    assert not bad, f"{what}: state of envs {bad}"


def slab_skipped(m, t, still_envs, call, what):
    """the slab proof: the sentinel into every byte of m's slab on the gym's stream, the call on both gyms; behind it the rows of the still envs hold the
    sentinel in every byte -- nothing drew them -- and every other row the twin's bytes.  Then mv_render on both puts the frames back."""
    m.sync()
    m.slab.fill_(SENT)
    m.sync()
    call(m); call(t)
    m.sync(); t.sync()
    a, b = m.slab.cpu().numpy(), t.slab.cpu().numpy()
    st = rows_of(still_envs, m.A)
    bad = [int(r) for r in np.nonzero(st)[0] if not (a[r] == SENT).all()]
    assert not bad, f"{what}: rows {bad} of still envs were drawn"
    bad = [int(r) for r in np.nonzero(~st)[0] if a[r].tobytes() != b[r].tobytes()]
    assert not bad, f"{what}: rows {bad} of changed envs differ from the twin's"
    assert all((b[r] != SENT).any() for r in range(b.shape[0])), f"{what}: the twin drew nothing"
    same(m, t, what, skip_envs=still_envs)
    m.g.render(); t.g.render()
    same(m, t, what + ", rendered again")


def ring_carried(m, t, still_envs, call, what):
    """the ring proof: a pattern over the rows of the still envs in the entry of the last tick (their home), the call on both gyms; behind it the pattern is
    in those rows of every entry the call rendered -- copied, not drawn -- and every other row is the twin's.  -> the planted envs (their rows stay
    patterned until the envs are drawn again)"""
    import torch
    m.sync()
    home = (m.ticks - 1) % m.R
    st = torch.from_numpy(rows_of(still_envs, m.A)).to(DEV)
    pattern = torch.arange(m.obs[home, 0].numel(), dtype=torch.int64, device=DEV).mul(37).add(11).remainder(251).to(torch.uint8).reshape(m.obs[home, 0].shape)
    m.obs[home, st] = pattern
    m.sync()
    em, et = call(m), call(t)
    assert em == et and em
    m.sync()
    a, p = m.obs.cpu().numpy(), pattern.cpu().numpy()
    for j in set(em) | {home}:
        bad = [int(r) for r in np.nonzero(st.cpu().numpy())[0] if a[j, r].tobytes() != p.tobytes()]
        assert not bad, f"{what}: entry {j}, rows {bad} of still envs do not hold the bytes of their home row"
    same(m, t, what, skip_envs=still_envs)


HALF = (np.arange(N) % 2 == 0)   # the envs that step; the odd ones are frozen


def freeze_half(m, t, stepping=HALF):
    for r in (m, t):
        r.g.set_step_mask(np.asarray(stepping, bool))


# ---- step masks ---------------------------------------------------------------------------------------------------------------------------------------------
def test_half_frozen_single_ticks_into_the_slab(hip):
    m, t = pair()
    freeze_half(m, t)
    m.step(); t.step()   # (every env is stale behind switching on: this pass draws them all)
    same(m, t, "first tick")
    for tick in range(3):
        slab_skipped(m, t, ~HALF, lambda r: r.step(), f"mv_step {tick}")
        m.step(); t.step()   # (mv_render made every env stale again)
        same(m, t, f"after render {tick}")
    # thaw: the next tick shows the thawed envs
    for r in (m, t):
        r.g.set_step_mask(None)
    for tick in range(2):
        m.step(); t.step()
        same(m, t, f"thawed {tick}")
    m.close(); t.close()


def test_half_frozen_step_n_16_into_the_slab_and_launch_counts(hip):
    """step_n(16) is two launches of 8: the choice crosses the chunk; without a ring no launch is added"""
    m, t = pair()
    freeze_half(m, t)
    m.step_n(16); t.step_n(16)
    same(m, t, "first call")
    l0, l1 = m.launches(), t.launches()
    slab_skipped(m, t, ~HALF, lambda r: r.step_n(16), "step_n(16)")
    m.step_n(16); t.step_n(16)
    same(m, t, "third call")
    assert ((m.launches() - l0) == (t.launches() - l1)).all(), "launches without a ring"
    m.close(); t.close()


@pytest.mark.parametrize("ring", [16, 32])
def test_half_frozen_ring(hip, ring):
    """count == k and count == 2k, a wrap over several calls, one more observation launch per call, thaw after many still calls"""
    m, t = pair(ring=ring)
    freeze_half(m, t)
    for c in range(3):
        l0, l1 = m.launches(), t.launches()
        m.step_n(16); t.step_n(16)
        same(m, t, f"ring {ring}, call {c}")
        dm, dt = m.launches() - l0, t.launches() - l1
        assert dm[0] == dt[0] and dm[1] == dt[1] + 1, f"ring {ring}, call {c}: launches {dm} against the twin's {dt}"
    for c in range(2):
        m.step_n(8); t.step_n(8)     # (k = 8 into the same rings: the entries run on from where they stand)
        same(m, t, f"ring {ring}, short call {c}")
    m.step(); t.step()
    same(m, t, f"ring {ring}, mv_step")
    ring_carried(m, t, ~HALF, lambda r: r.step_n(16), f"ring {ring}, planted")
    for r in (m, t):
        r.g.set_step_mask(None)
    for c in range(2):   # thaw: every env steps and is drawn into every entry of the two calls -- the pattern is gone from a ring of 16, and from 32 after both
        m.step_n(16); t.step_n(16)
    same(m, t, f"ring {ring}, thawed")
    m.close(); t.close()


@pytest.mark.parametrize("ring", [0, 16])
def test_render_last_and_none_then_a_rendered_call(hip, ring):
    """ticks without a pass make a stepping env stale and leave a frozen one alone"""
    m, t = pair(ring=ring)
    freeze_half(m, t)
    m.step_n(8); t.step_n(8)
    same(m, t, "first call")
    for c, (k, render) in enumerate([(16, "none"), (8, "last"), (16, "last"), (8, "none"), (8, "every"), (16, "last"), (1, "every")]):
        m.step_n(k, render); t.step_n(k, render)
        same(m, t, f"call {c}: {k} ticks, render={render}")
    if ring:
        ring_carried(m, t, ~HALF, lambda r: r.step_n(16, "last")[-1:], "render=last, planted")
    else:
        slab_skipped(m, t, ~HALF, lambda r: r.step_n(16, "last"), "render=last")
    m.close(); t.close()


# ---- budgets --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [0, 16])
def test_budget_one_halts_inside_a_resident_launch(hip, ring):
    """the clocks staggered as tests/test_episode_budget_gpu.py staggers them: with budget 1 the envs halt on different ticks of a 16-tick call -- on ticks 7
    and 8, the boundary between its two launches, and inside a launch -- and are still from the tick behind; then further calls on the halted batch"""
    from test_episode_budget_gpu import make, stagger
    rigs = []
    for still in (True, False):
        g = make("tower_long", 1, "fast")
        stagger(g, "tower_long", 1)
        g.set_episode_budget(1)
        rigs.append(Rig(gym=g, n=g.num_envs, w=32, h=32, ring=ring, still=still))
    m, t = rigs
    for c in range(3):
        m.step_n(16); t.step_n(16)
        same(m, t, f"budget 1, call {c}")
    halted = m.g.episode_budget().cpu().numpy() == 0
    assert halted.sum() >= 3, halted
    if ring:
        ring_carried(m, t, halted, lambda r: r.step_n(16), "halted, planted")
    else:
        slab_skipped(m, t, halted, lambda r: r.step_n(16), "halted")
    m.close(); t.close()


def test_budget_with_ordinary_episode_lengths_across_calls(hip):
    """budgets of one and two episodes, the episode log on, the clocks staggered: some envs halt in the first call and stay still for the calls behind,
    the others run on"""
    from test_episode_budget_gpu import make, stagger
    rigs = []
    for still in (True, False):
        g = make("tower_long", 1, "fast", log=256)
        stagger(g, "tower_long", 1)
        g.set_episode_budget(np.array([1, 2] * (g.num_envs // 2), np.int32))
        rigs.append(Rig(gym=g, w=32, h=32, ring=16, still=still))
    m, t = rigs
    for c in range(6):
        m.step_n(16); t.step_n(16)
        same(m, t, f"budgets, call {c}")
    left = m.g.episode_budget().cpu().numpy()
    assert (left == 0).any() and (left != 0).any(), left
    a, b = m.g.drain_episode_log(), t.g.drain_episode_log()
    assert len(a) > 0 and a.tobytes() == b.tobytes(), "episode log"
    m.close(); t.close()


# ---- macro steps -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [0, 4])
def test_macro_step_with_per_env_ticks(hip, ring):
    """envs whose macro step is over early are still at the call's one pass only if they did not step at all; ticks[e] = 0 freezes an env for the call"""
    m, t = pair(ring=ring)
    ticks = np.array([0, 3, 8, 0, 1, 8, 0, 5, 2, 0, 8, 4], np.int32)
    for c in range(3):
        m.macro(8, c, ticks); t.macro(8, c, ticks)
        same(m, t, f"macro step {c}")
    if ring:
        ring_carried(m, t, ticks == 0, lambda r: r.macro(8, 7, ticks), "macro step, planted")
    else:
        slab_skipped(m, t, ticks == 0, lambda r: r.macro(8, 7, ticks), "macro step")
    for c in range(4):   # no ticks given: every env steps and is drawn -- into every entry of the ring of 4
        m.macro(11, 20 + c); t.macro(11, 20 + c)
    m.macro(4, 30, render="none"); t.macro(4, 30, render="none")
    m.step(); t.step()
    same(m, t, "macro steps, all envs")
    m.close(); t.close()


# ---- draw masks, state observations, the episode log ---------------------------------------------------------------------------------------------------------------
def test_draw_mask_on_top(hip):
    """user-undrawn rows keep the sentinel and the env stays stale: when the mask lets it through it is drawn although it is frozen"""
    import torch
    m, t = pair(log=64)
    so_m, so_t = m.g.set_state_obs(True), t.g.set_state_obs(True)
    freeze_half(m, t)
    undrawn = np.zeros(N, bool); undrawn[[1, 2]] = True   # a frozen and a stepping env
    for r in (m, t):
        r.g.set_draw_mask(~undrawn)
    for r in (m, t):
        r.sync(); r.slab.fill_(SENT); r.sync()
    for tick in range(3):
        m.step(); t.step()
        same(m, t, f"draw mask, tick {tick}")
        m.sync()
        assert (m.slab.cpu().numpy()[rows_of(undrawn, 1)] == SENT).all() and not (m.slab.cpu().numpy()[rows_of(~undrawn, 1)] == SENT).all()
        assert torch.equal(so_m, so_t)
    for r in (m, t):
        r.g.set_draw_mask(None)
    m.step(); t.step()   # env 1 is frozen, was never drawn with the option on: stale, so this pass draws it
    same(m, t, "draw mask lifted")
    assert not (m.slab.cpu().numpy() == SENT).all(axis=(1, 2, 3)).any()
    m.close(); t.close()


# ---- calls that change state: the next tick shows the new view ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [0, 16])
def test_fork_reset_load_into_frozen_envs(hip, ring):
    m, t = pair(ring=ring)
    freeze_half(m, t)
    stores = [r.g.new_env_store(2) for r in (m, t)]
    for r, s in zip((m, t), stores):
        r.step_n(8)
        r.g.save_envs(np.array([0] + [-1] * (N - 1), np.int32), s)
        r.step_n(8)
    same(m, t, "before")
    fork = np.full(N, -1, np.int32); fork[1] = 4          # the stepping env 4 continues in the frozen env 1
    load = np.full(N, -1, np.int32); load[5] = 0          # the saved env 0 continues in the frozen env 5
    reset = np.zeros(N, bool); reset[3] = True            # the frozen env 3 starts its next episode
    ops = [lambda r, s: r.g.fork_envs(fork), lambda r, s: r.g.reset_envs(reset, render=False), lambda r, s: r.g.load_envs(load, s),
           lambda r, s: r.g.reset_envs(reset, render=True), lambda r, s: r.g.debug_set_agent_pos(7, 0, 3.5, 1.0, 3.5)]
    for i, op in enumerate(ops):
        for r, s in zip((m, t), stores):
            op(r, s)
            r.step()
        same(m, t, f"op {i}, the tick behind it")
        m.step_n(8); t.step_n(8)
        same(m, t, f"op {i}, a call later")
    m.close(); t.close()


# ---- pixel modes, layouts, scenarios ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_pixels_against_the_oracle(hip):
    """exact mode: the rows equal the twin's, and the rows of envs frozen since the reset equal the CPU oracle's render of the reset state"""
    import oracle_lib
    n, A = 8, 2
    m, t = pair("TowerBuilding", A, n, mode="exact")
    og = oracle_lib.OracleGym("TowerBuilding", 64, 64, n, A, 1, False, {})
    og.seed(ENV_SEED)
    og.reset()
    stepping = np.arange(n) % 2 == 1
    freeze_half(m, t, stepping)
    for tick in range(4):
        act = sample_actions(POLICY_SEED, tick, n * A)
        m.step(act); t.step(act)
        same(m, t, f"exact, tick {tick}")
        got = m.slab.cpu().numpy()
        for e in np.nonzero(~stepping)[0]:
            for a in range(A):
                assert np.array_equal(got[e * A + a], og.get_observation(int(e), a)), f"exact, tick {tick}: frozen env {e} agent {a} against the oracle"
    slab_skipped(m, t, ~stepping, lambda r: r.step(sample_actions(POLICY_SEED, 9, n * A)), "exact")
    og.close()
    m.close(); t.close()
    m, t = pair(mode="exact", ring=8)
    freeze_half(m, t)
    for c in range(3):
        m.step_n(8); t.step_n(8)
        same(m, t, f"exact, step_n(8), call {c}")
    m.close(); t.close()


CASES = {
    "chw": dict(layout="chw"), "chw_48x20": dict(layout="chw", w=48, h=20), "tower_a2": dict(A=2), "hex_memory": dict(scenario="HexMemory"),
    "obstacles_easy": dict(scenario="ObstaclesEasy"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_layouts_agents_scenarios(hip, case):
    """the CHW layout (also with rows that are no multiple of 16 bytes times an odd count), TowerBuilding with 2 agents (par_agents), a long-list scenario
    and a host-fed short-list scenario: single ticks into the slab, then batched calls into a ring, then the ring proof"""
    kw = dict(CASES[case])
    m, t = pair(**kw)
    freeze_half(m, t)
    m.step(); t.step()
    slab_skipped(m, t, ~HALF, lambda r: r.step(), f"{case}, mv_step")
    m.close(); t.close()
    m, t = pair(ring=16, **kw)
    freeze_half(m, t)
    for c in range(2):
        m.step_n(16); t.step_n(16)
        same(m, t, f"{case}, call {c}")
    m.step_n(8, "last"); t.step_n(8, "last")
    same(m, t, f"{case}, render=last")
    ring_carried(m, t, ~HALF, lambda r: r.step_n(16), f"{case}, planted")
    m.close(); t.close()


# ---- overlap, switching off, refusals, memory ------------------------------------------------------------------------------------------------------------------------
def test_pass_overlap_with_a_ring_runs_in_order(hip):
    m, t = pair(n=16, ring=32, overlap=True)
    half = np.arange(16) % 2 == 0
    freeze_half(m, t, half)
    for c in range(4):
        m.step_n(16); t.step_n(16)
        same(m, t, f"overlap, call {c}")
    m.close(); t.close()


def test_switching_off_mid_run(hip):
    m, t = pair(ring=16)
    freeze_half(m, t)
    for c in range(2):
        m.step_n(16); t.step_n(16)
    same(m, t, "on")
    m.g.set_still_frames(False)
    assert m.g.still_frames() is False
    l0, l1 = m.launches(), t.launches()
    m.step_n(16); t.step_n(16)
    same(m, t, "off")
    assert ((m.launches() - l0) == (t.launches() - l1)).all(), "switched off: the twin's launches"
    # off: every env is drawn again -- a sentinel over the whole ring is gone behind one call
    m.sync(); m.obs.fill_(SENT); m.sync()
    m.step_n(16); t.step_n(16)
    same(m, t, "off, drawn whole")
    m.g.set_still_frames(True)   # on again: every env stale
    m.sync(); m.obs.fill_(SENT); m.sync()
    m.step_n(16); t.step_n(16)
    same(m, t, "on again")
    m.close(); t.close()


def test_refusals_and_arena_bytes(hip):
    import ctypes as C
    U.boxoban_env()
    g = MegaverseGym("TowerBuilding", 64, 64, N, 1, 1, False, {})
    h = MegaverseGym("TowerBuilding", 64, 64, N, 1, 1, False, {})
    b0 = g.arena_bytes()
    g.set_still_frames(True)     # (valid before the first reset)
    b1 = g.arena_bytes()
    assert b1 == b0 + N * 4 + N
    g.set_still_frames(False); g.set_still_frames(True)
    assert g.arena_bytes() == b1, "arena_bytes grows on first use only"
    g.reset(); h.reset()
    lib = g._lib
    arr = (C.c_void_p * 2)(g._g, h._g)
    grp = C.c_void_p()
    assert lib.mv_group_create(arr, 2, C.byref(grp)) == -1
    msg = lib.mv_last_error().decode()
    assert "mv_group_create" in msg and "mv_set_still_frames" in msg, msg
    assert lib.mv_step_many(arr, 2, 1, 1, 1, 0) == -1
    msg = lib.mv_last_error().decode()
    assert "mv_step_many: gym 0" in msg and "mv_set_still_frames" in msg, msg
    g.set_still_frames(False)
    assert lib.mv_group_create(arr, 2, C.byref(grp)) == 0, lib.mv_last_error()
    assert lib.mv_set_still_frames(g._g, 1) == -1 and "mv_group" in lib.mv_last_error().decode()
    assert lib.mv_group_destroy(grp) == 0
    g.close(); h.close()
