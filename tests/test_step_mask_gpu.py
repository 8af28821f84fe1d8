"""Step masks on the GPU (include/megaverse_hip.h: mv_set_step_mask): the envs a mask freezes skip ticks and stay as they are, on the device.

Every test uses 8 envs and 32 x 32 frames (tests/step_mask_util.py) and the masks "{env 0, env 3, env 7} step" and its complement unless it says otherwise.
Envs are independent, so expected values come from the CPU oracle as it is: oracle P steps every tick, oracle Q skips the ticks of the frozen window and then
acts on the actions of the GYM's tick index; a stepping env is P's env, a frozen or once-frozen env Q's, and on a frozen tick the expected rewards and dones
are zeros.  Where a test compares two paths of the library instead, one of them is the tick-by-tick path the oracle tests pin.  Every comparison is equality
of bytes; no env, tick or byte is left out."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_log_util as U
import oracle_lib
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions
from step_mask_util import COMPLEMENT, H, MASK, N, STEPPING, W, MaskedModel, mask_of
from test_reset_envs_gpu import ENV_SEED, ORACLE_CASES, POLICY_SEED, act, all_raw, capture, check_env, device_mask, make_gym, raw, slab

pytestmark = pytest.mark.gpu

T0, TF, T1 = 7, 5, 12   # ticks before the mask, with it, behind it


def step_ok(g):
    """mv_step that returned 0: no error and no warning"""
    assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()


# ---- 1. against the oracle, every scenario family ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_pq(scenario, A, params_items=(), t0=T0, tf=TF, t1=T1):
    """oracle P steps t0 + tf + t1 ticks; oracle Q the first t0 and the last t1 of them, with the actions of those tick indices -> (P's capture behind every
    tick, {tick: Q's capture} for the ticks behind the window), computed once per scenario and shared by the masks"""
    U.boxoban_env()
    pq = []
    for _ in range(2):
        og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, dict(params_items))
        og.seed(ENV_SEED)
        og.reset()
        pq.append(og)
    P, Q = pq
    caps_p, caps_q = [], {}
    for t in range(t0 + tf + t1):
        m = action_masks(sample_actions(POLICY_SEED, t, N * A))
        P.set_action_masks(m)
        P.step()
        caps_p.append(capture(P, scenario, A))
        if t < t0:
            Q.set_action_masks(m)
            Q.step_norender()
        elif t >= t0 + tf:
            Q.set_action_masks(m)
            Q.step()
            caps_q[t] = capture(Q, scenario, A)
    P.close(); Q.close()
    return caps_p, caps_q


def expected(ref, steps, e, t, t0, tf):
    """what env e is behind tick t: (capture, whether t is a frozen tick of e)"""
    caps_p, caps_q = ref
    if steps[e] or t < t0:
        return caps_p[t], False
    if t < t0 + tf:
        c = caps_p[t0 - 1]
        return dict(c, rewards=np.zeros_like(c["rewards"]), dones=np.zeros_like(c["dones"])), True
    return caps_q[t], False


def run_schedule(hg, scenario, A, steps, ref, what, t0=T0, tf=TF, t1=T1, attach=None):
    """t0 ticks, the mask on for tf ticks, the mask off, t1 more ticks of mv_step (each returns 0: no warning); every env is checked behind every tick"""
    attach = attach or (lambda g, m: g.set_step_mask(m))
    consumed = None
    for t in range(t0 + tf + t1):
        if t == t0:
            attach(hg, steps)
            consumed = hg.debug_episodes_consumed().tolist()
        if t == t0 + tf:
            hg.set_step_mask(None)
            assert hg.step_mask() == "none"
        act(hg, A, t)
        step_ok(hg)
        now = hg.debug_episodes_consumed().tolist()
        for e in range(N):
            ref_e, frozen = expected(ref, steps, e, t, t0, tf)
            check_env(hg, ref_e, scenario, A, e, f"{what}, tick {t}{' (frozen)' if frozen else ''}")
            if frozen:
                assert now[e] == consumed[e], f"{what}, tick {t}: frozen env {e} took an episode"
    assert hg.ticks_since_reset() == t0 + tf + t1


@pytest.mark.parametrize("mask_name", sorted(STEPPING))
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_frozen_envs_against_the_oracle(hip, case, mask_name):
    """1. 7 ticks, the mask (host form) on for 5 ticks, off, 12 more ticks: snapshot, scenario state, reward bits, dones, true objectives and exact-mode
    frames of every env behind every tick"""
    scenario, A = ORACLE_CASES[case]
    steps = STEPPING[mask_name]
    ref = oracle_pq(scenario, A)
    assert ref[0][T0 + TF]["snap"][0].tobytes() != ref[1][T0 + TF]["snap"][0].tobytes(), "P and Q agree behind the window: the test would prove nothing"
    hg = make_gym(scenario, A, "exact")

    def attach(g, m):
        g.set_step_mask(m)
        assert g.step_mask() == "host"

    run_schedule(hg, scenario, A, steps, ref, f"{case}, {mask_name}", attach=attach)
    hg.close()


# ---- 2. the device form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_device_form_equals_host_form(hip, scenario):
    """2. output rings 16 deep, step_n(8) twice.  Device form: the mask is written by a torch kernel on the gym's stream, attached, the call enqueued, the
    mask REWRITTEN (its complement) by another kernel and attached again, the second call enqueued -- nothing synchronises in between.  Host form: the same
    two masks with a synchronisation on every side.  Rings, snapshots, consumed counts: the same bytes."""
    import torch
    A, K = 1, 8
    out = []
    for form in ("device", "host"):
        g = make_gym(scenario, A, "fast")
        rings = (torch.zeros((2 * K, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0"), torch.full((2 * K, N * A), -7.0, dtype=torch.float32, device="cuda:0"),
                 torch.full((2 * K, N), 9, dtype=torch.uint8, device="cuda:0"))
        src = [torch.as_tensor(MASK).to("cuda:0"), torch.as_tensor(COMPLEMENT).to("cuda:0")]
        m = torch.ones(N, dtype=torch.bool, device="cuda:0")   # (would freeze nobody, were it read before the kernels below have run)
        torch.cuda.synchronize()
        g.set_output_ring(2 * K, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
        for c in range(2):
            if form == "device":
                torch.logical_and(src[c], src[c], out=m)
                g.set_step_mask(m)
                assert g.step_mask() == "device"
            else:
                g.synchronize()
                g.set_step_mask([MASK, COMPLEMENT][c])
                assert g.step_mask() == "host"
                g.synchronize()
            c0 = g.debug_launch_counts()
            g.step_n(K, "multidiscrete", POLICY_SEED, c * K)
            assert g.debug_launch_counts()[0] - c0[0] == 1, "a masked call is one step launch, as an unmasked one"
        g.synchronize()
        out.append(([r.cpu().numpy() for r in rings], all_raw(g), g.debug_episodes_consumed().tolist()))
        g.close()
        del m
    (ra, sa, ca), (rb, sb, cb) = out
    for x, y, name in zip(ra, rb, ("observations", "rewards", "dones")):
        assert x.tobytes() == y.tobytes(), f"{name} rings differ between the forms"
    assert sa == sb and ca == cb
    rew, done = ra[1].reshape(2, K, N, A), ra[2].reshape(2, K, N)
    assert not rew[0][:, ~MASK].any() and not rew[1][:, ~COMPLEMENT].any() and not done[0][:, ~MASK].any() and not done[1][:, ~COMPLEMENT].any()
    assert rew.view(np.uint32)[0][:, ~MASK].max() == 0 and rew.view(np.uint32)[1][:, ~COMPLEMENT].max() == 0   # (+0.0f, not -0.0f)
    for e in range(N):   # a frozen env's frame is the frame it had: call 0 leaves the frozen envs at their reset view in all 8 entries
        if not MASK[e]:
            assert all(ra[0][j][e].tobytes() == ra[0][0][e].tobytes() for j in range(K))


# ---- 3. every stepping entry and policy against a tick-by-tick masked twin; 4. several agents ------------------------------------------------------------
TICKS = 16
ENTRIES = ("step", "step_no_render", "step_n_8", "step_n_16", "render_none", "render_last")
SENTINEL = 0xAB


def ring_actions(A):
    return np.stack([sample_actions(POLICY_SEED + 1, t, N * A) for t in range(TICKS)]).astype(np.int32)


def run_entry(g, entry, policy, A):
    """16 ticks of gym g through one entry with one policy -> every tick's rewards and dones, the frames the entry draws, the slab, the final state, the
    launches it took"""
    import torch
    NA = N * A
    rew, done, frames = np.zeros((TICKS, NA), np.float32), np.zeros((TICKS, N), np.uint8), {}
    keep = []
    if policy == "single-bit":
        g.set_sample_policy("single-bit")
    if policy == "none":   # (the first tick acts on what was set, the following ones on cleared actions)
        g.set_actions_batched(sample_actions(POLICY_SEED + 2, 0, NA))
    if policy == "sequence":
        ring = torch.as_tensor(ring_actions(A)).to("cuda:0")
        torch.cuda.synchronize()
        keep.append(ring)
        g.set_action_ring(TICKS, ring.data_ptr())
    slab_t = torch.zeros((NA, H, W, 4), dtype=torch.uint8, device="cuda:0")
    g.set_obs_buffer(slab_t.data_ptr())
    g.synchronize()
    slab_t.fill_(SENTINEL)
    torch.cuda.synchronize()
    c0 = g.debug_launch_counts()
    if entry in ("step", "step_no_render"):
        for t in range(TICKS):
            if policy in ("multidiscrete", "single-bit"):
                g.sample_random_actions(POLICY_SEED, t)
            elif policy == "sequence":
                g.set_actions_device(ring[t].data_ptr())
            rc = g._lib.mv_step(g._g) if entry == "step" else g._lib.mv_step_no_render(g._g)
            assert rc == 0, g._lib.mv_last_error()
            rew[t], done[t] = g.get_rewards_array(), g.get_dones()
            if entry == "step":
                g.synchronize()
                frames[t] = slab_t.cpu().numpy()
    else:
        k = 8 if entry == "step_n_8" else TICKS
        mode = {"render_none": "none", "render_last": "last"}.get(entry, "every")
        rings = [torch.full((TICKS, NA), -7.0, dtype=torch.float32, device="cuda:0"), torch.full((TICKS, N), 9, dtype=torch.uint8, device="cuda:0")]
        obs = torch.zeros((TICKS, NA, H, W, 4), dtype=torch.uint8, device="cuda:0") if mode == "every" else None
        torch.cuda.synchronize()
        g.set_output_ring(TICKS, obs.data_ptr() if obs is not None else 0, rings[0].data_ptr(), rings[1].data_ptr())
        for first in range(0, TICKS, k):
            g.step_n(k, policy, POLICY_SEED, first, render=mode)
        g.synchronize()
        rew[:], done[:] = rings[0].cpu().numpy(), rings[1].cpu().numpy()
        if obs is not None:
            frames = {t: f for t, f in enumerate(obs.cpu().numpy())}
        if mode == "last":
            frames[TICKS - 1] = slab_t.cpu().numpy()
        g.set_output_ring(0)
    c1 = g.debug_launch_counts()
    g.synchronize()
    out = {"rew": rew, "done": done, "frames": frames, "slab": slab_t.cpu().numpy(), "snaps": all_raw(g), "tobj": g.get_true_objectives(),
           "consumed": g.debug_episodes_consumed().tolist(), "launches": (c1[0] - c0[0], c1[1] - c0[1])}
    del keep
    return out


@functools.lru_cache(maxsize=None)
def twin_reference(scenario, A, policy, mask_name):
    """the masked twin, tick by tick through mv_step (the entry test 1 pins to the oracle), not pipelined: sequence = the ring's entry handed over as
    this tick's actions"""
    g = make_gym(scenario, A, "fast")
    g.set_pipelining(False)
    g.set_step_mask(STEPPING[mask_name])
    out = run_entry(g, "step", policy, A)
    g.close()
    return out


def check_entry(hip, monkeypatch, scenario, A, entry, policy, variants, mask_name="step_0_3_last"):
    steps = STEPPING[mask_name]
    ref = twin_reference(scenario, A, policy, mask_name)
    per = np.repeat(steps, A)
    assert not ref["rew"][:, ~per].any() and not ref["done"][:, ~steps].any()
    for variant in variants:
        what = f"{scenario} x {A}, {entry}, {policy}, {variant}"
        monkeypatch.delenv("MV_STEP_PIPE", raising=False)
        if variant in ("pipe0", "pipe1"):
            monkeypatch.setenv("MV_STEP_PIPE", variant[-1])
        outs = []
        for masked in (True, False):
            g = make_gym(scenario, A, "fast")
            if variant == "unpipelined":
                g.set_pipelining(False)
            if masked:
                g.set_step_mask(steps)
            outs.append(run_entry(g, entry, policy, A))
            g.close()
        got, plain = outs
        assert got["launches"] == plain["launches"], f"{what}: {got['launches']} launches with a mask, {plain['launches']} without"
        assert got["rew"].tobytes() == ref["rew"].tobytes(), f"{what}: rewards"
        assert got["done"].tobytes() == ref["done"].tobytes(), f"{what}: dones"
        assert got["snaps"] == ref["snaps"], f"{what}: final state of envs {[e for e in range(N) if got['snaps'][e] != ref['snaps'][e]]}"
        assert got["tobj"].tobytes() == ref["tobj"].tobytes() and got["consumed"] == ref["consumed"], what
        assert got["snaps"] != plain["snaps"], f"{what}: the mask changed nothing"
        drawn = {"step": range(TICKS), "step_n_8": range(TICKS), "step_n_16": range(TICKS), "render_last": [TICKS - 1]}.get(entry, [])
        assert sorted(got["frames"]) == list(drawn)
        for t in drawn:
            assert got["frames"][t].tobytes() == ref["frames"][t].tobytes(), f"{what}: frames of tick {t}"
        if entry in ("step_no_render", "render_none", "step_n_8", "step_n_16"):   # (the ring entries took the frames, or nothing was drawn)
            assert (got["slab"] == SENTINEL).all(), f"{what}: {int((got['slab'] != SENTINEL).sum())} bytes of the slab were written"


TOWER_MATRIX = [(e, p) for e in ENTRIES for p in ("multidiscrete", "single-bit", "sequence", "none")]


@pytest.mark.parametrize("entry,policy", TOWER_MATRIX, ids=[f"{e}-{p}" for e, p in TOWER_MATRIX])
def test_every_entry_and_policy(hip, monkeypatch, entry, policy):
    """3. TowerBuilding, fast pixels (what the one-launch paths need), 16 ticks with {0, 3, 7} stepping, through each entry and policy: rewards and dones
    of every tick, every drawn frame, final snapshots, true objectives and consumed counts equal the tick-by-tick twin's; the launches equal the same
    calls' without a mask; MV_RENDER_NONE, mv_step_no_render and calls into rings write not one byte of the slab.  Pipelined (the default), not pipelined,
    and with the software-pipelined kernel forced off and on."""
    variants = ("default", "unpipelined") if entry in ("step", "step_no_render") else ("default", "unpipelined", "pipe0", "pipe1")
    check_entry(hip, monkeypatch, "TowerBuilding", 1, entry, policy, variants)


FAMILIES = ["ObstaclesEasy", "Collect", "Rearrange", "Sokoban", "HexMemory", "BoxAGone", "Empty", "Football"]


@pytest.mark.parametrize("entry", ["step_n_8", "render_none", "render_last"])
@pytest.mark.parametrize("scenario", FAMILIES)
def test_batched_entries_every_family(hip, monkeypatch, scenario, entry):
    """3, the multi-tick kernels of every other scenario family (each has its own instantiations of the shared bodies), complement mask"""
    check_entry(hip, monkeypatch, scenario, 1, entry, "multidiscrete", ("default", "pipe0"), mask_name="step_complement")


@pytest.mark.parametrize("entry", ["step", "step_n_8", "step_n_16", "render_none", "render_last"])
def test_several_agents_tower(hip, monkeypatch, entry):
    """4. TowerBuilding with four agents per env: every wave of the workgroup takes part in the tick (par_agents), in the single-tick kernel and in the
    multi-tick ones"""
    check_entry(hip, monkeypatch, "TowerBuilding", 4, entry, "multidiscrete", ("default", "unpipelined"))


@pytest.mark.parametrize("entry", ["step_no_render", "step_n_8", "render_last"])
def test_several_agents_obstacles(hip, monkeypatch, entry):
    """4. ObstaclesEasy with two agents per env: the tick-by-tick multi-agent path"""
    check_entry(hip, monkeypatch, "ObstaclesEasy", 2, entry, "multidiscrete", ("default",))


@pytest.mark.parametrize("mask_name", sorted(STEPPING))
@pytest.mark.parametrize("scenario,A", [("TowerBuilding", 4), ("ObstaclesEasy", 2)])
def test_several_agents_against_the_oracle(hip, scenario, A, mask_name):
    """4. ... and both against the oracle, on the schedule of test 1"""
    hg = make_gym(scenario, A, "exact")
    run_schedule(hg, scenario, A, STEPPING[mask_name], oracle_pq(scenario, A), f"{scenario} x {A}, {mask_name}")
    hg.close()


# ---- 5. episodes ending beside frozen envs -------------------------------------------------------------------------------------------------------------
SHORT = {"rearrange": ("Rearrange", 1, {"episodeLengthSec": 0.19}), "tower": ("TowerBuilding", 2, {"episodeLengthSec": -220.0})}


@pytest.mark.parametrize("mask_name", sorted(STEPPING))
@pytest.mark.parametrize("case", sorted(SHORT))
def test_episodes_end_beside_frozen_envs(hip, case, mask_name):
    """5. episodes of a few ticks (host-fed Rearrange through the refill protocol, device-drawn TowerBuilding), 5 ticks, the mask on for 24, off, 12 more:
    the stepping envs auto-reset several times inside the window while the frozen ones keep their snapshot and their consumed count; no call returns a
    warning; behind the thaw the frozen envs take the episodes of their own sequence -- every env, every tick against P and Q"""
    scenario, A, params = SHORT[case]
    steps = STEPPING[mask_name]
    t0, tf, t1 = 5, 24, 12
    ref = oracle_pq(scenario, A, tuple(sorted(params.items())), t0, tf, t1)
    ends = np.stack([c["dones"] for c in ref[0][t0:t0 + tf]]).sum(axis=0)
    # (TowerBuilding's episode length follows the room: some envs' episodes outlast the window whatever the parameter)
    assert ends[steps].sum() >= 8 and (ends[steps] >= 2).sum() >= 2, f"stepping envs finished {ends[steps].tolist()} episodes inside the window: too few"
    assert sum(int(c["dones"][~steps].sum()) for c in ref[1].values()) >= 2, "no once-frozen env finishes an episode behind the thaw"
    hg = make_gym(scenario, A, "exact", params)
    run_schedule(hg, scenario, A, steps, ref, f"{case}, {mask_name}", t0, tf, t1)
    hg.close()


# ---- 6. the episode log on the device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_episode_log_every_entry(hip, entry):
    """6. Sokoban with episodes of 4.5 s (every episode ends at its 68th stepped tick), six legs of 16 ticks through one entry; the second leg runs with
    {0, 3, 7} stepping, the third with the complement, so every env stands still for 16 ticks inside its first episode.  The model (MaskedModel) is fed the
    gym's own per-tick outputs and the leg's mask: records, running returns and lengths byte for byte behind every leg; a record's length counts the ticks
    its env stepped (68), its end_tick the gym's ticks (83)."""
    import torch
    A, K, legs = 1, 16, [None, MASK, COMPLEMENT, None, None, None]
    g = make_gym("Sokoban", A, "fast", {"episodeLengthSec": 4.5}, log=4096)
    model = MaskedModel(N, A)
    batched = entry not in ("step", "step_no_render")
    if batched:
        k = 8 if entry == "step_n_8" else K
        mode = {"render_none": "none", "render_last": "last"}.get(entry, "every")
        rings = [torch.zeros((K, N * A), dtype=torch.float32, device="cuda:0"), torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")]
        obs = torch.zeros((K, N * A, H, W, 4), dtype=torch.uint8, device="cuda:0") if mode == "every" else None
        torch.cuda.synchronize()
        g.set_output_ring(K, obs.data_ptr() if obs is not None else 0, rings[0].data_ptr(), rings[1].data_ptr())
    for leg, mask in enumerate(legs):
        g.set_step_mask(mask)
        if batched:
            for first in range(0, K, k):
                g.step_n(k, "multidiscrete", POLICY_SEED, leg * K + first, render=mode)
            g.synchronize()
            rew, done = rings[0].cpu().numpy(), rings[1].cpu().numpy()
            assert (done.sum(axis=0) <= 1).all()
            model.feed(rew, done, np.repeat(g.get_true_objectives()[None], K, axis=0), mask)
        else:
            for t in range(K):
                g.sample_random_actions(POLICY_SEED, leg * K + t)
                rc = g._lib.mv_step(g._g) if entry == "step" else g._lib.mv_step_no_render(g._g)
                assert rc == 0, g._lib.mv_last_error()
                model.feed(g.get_rewards_array()[None], g.get_dones()[None], g.get_true_objectives()[None], mask)
        assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes(), f"running returns behind leg {leg}"
        assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes(), f"running lengths behind leg {leg}"
        if leg == 2:
            assert model.len.tolist() == [2 * K] * N, "every env has stepped 32 of the gym's 48 ticks"
    want = np.array(model.records, U.RECORD)
    assert sorted(want["agent"].tolist()) == list(range(N)), "every env finishes exactly one episode inside the run"
    assert want["length"].tolist() == [68] * N and want["end_tick"].tolist() == [67 + K] * N
    got = g.drain_episode_log()
    assert g.episode_log_dropped == 0
    assert got.tobytes() == want.tobytes()
    assert g.ticks_since_reset() == len(legs) * K == model.tick
    g.close()


def test_episode_log_several_agents_short_episodes(hip):
    """6. TowerBuilding, two agents per env, episodes that end every tick or every few ticks at first (stepped one tick per call): 4 ticks, {0, 3, 7}
    stepping for 8, the complement for 8, no mask for 8 -- records of the stepping envs in both masked legs, none of a frozen env while it is frozen"""
    A = 2
    g = make_gym("TowerBuilding", A, "fast", {"episodeLengthSec": -200.0}, log=4096)
    model = MaskedModel(N, A)
    tick = 0
    for mask, ticks in ((None, 4), (MASK, 8), (COMPLEMENT, 8), (None, 8)):
        g.set_step_mask(mask)
        before = len(model.records)
        for _ in range(ticks):
            assert g._lib.mv_step_n(g._g, 1, 1, POLICY_SEED, tick) == 0, g._lib.mv_last_error()
            model.feed(g.get_rewards_array()[None], g.get_dones()[None], g.get_true_objectives()[None], mask)
            tick += 1
        new = np.array(model.records[before:], U.RECORD)
        if mask is not None:
            assert len(new) > 0, "no episode ended inside a masked leg"
            assert set((new["agent"] // A).tolist()) <= set(np.flatnonzero(mask).tolist())
    got = g.drain_episode_log()
    assert got.tobytes() == np.array(model.records, U.RECORD).tobytes()
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == model.ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == model.len.tobytes()
    assert g.ticks_since_reset() == tick == model.tick
    g.close()


# ---- 7. a savepoint that keeps -------------------------------------------------------------------------------------------------------------------------
def test_savepoint(hip):
    """7. TowerBuilding, 7 ticks, env 0 frozen; three iterations of: fork envs 1..7 from env 0, step_n(8, 'sequence', render='none') on the next 8 entries
    of an action ring.  Env 0's snapshot is the same bytes throughout; behind each iteration env d is the env 0 of an oracle that stepped the 7 ticks and
    then 8 ticks on d's column of those entries.  reset_envs on the frozen env 0 gives it the next episode of its own sequence, which it then keeps."""
    import torch
    A, K, ITER = 1, 8, 3
    g = make_gym("TowerBuilding", A, "exact")
    script = [sample_actions(POLICY_SEED, t, N * A) for t in range(T0)]
    for t in range(T0):
        g.set_actions_batched(script[t])
        step_ok(g)
    plans = np.stack([sample_actions(POLICY_SEED + 5, t, N * A) for t in range(ITER * K)]).astype(np.int32)
    ring = torch.as_tensor(plans).to("cuda:0")
    torch.cuda.synchronize()
    g.set_action_ring(ITER * K, ring.data_ptr())
    g.set_step_mask(mask_of(range(1, N)))
    saved = raw(g, 0)

    def oracle_branch(it, d):
        og = oracle_lib.OracleGym("TowerBuilding", W, H, 1, A, 1, False, {})   # (env 0 of a one-env gym is env 0 of any gym with this seed)
        og.seed(ENV_SEED)
        og.reset()
        for t in range(T0):
            og.set_action_masks(action_masks(script[t][:A]))
            og.step_norender()
        if it < 0:
            og.reset()
        else:
            for j in range(K):
                og.set_action_masks(action_masks(plans[it * K + j][d * A:(d + 1) * A]))
                og.step_norender()
        out = og.snapshot(0), og.get_last_rewards().copy()
        og.close()
        return out

    for it in range(ITER):
        g.fork_envs([-1] + [0] * (N - 1))
        assert all(raw(g, d) == saved for d in range(1, N))
        g.step_n(K, "sequence", 0, it * K, render="none")
        assert raw(g, 0) == saved, f"iteration {it}: the savepoint moved"
        rew = g.get_rewards_array()
        assert rew.view(np.uint32)[0] == 0
        for d in range(1, N):
            snap, last = oracle_branch(it, d)
            assert diff_snapshots(snap, hip_snapshot(g, d), A) == [], f"iteration {it}: env {d}"
            assert rew[d * A:(d + 1) * A].tobytes() == last.tobytes(), f"iteration {it}: rewards of env {d}"
        assert len({raw(g, d) for d in range(1, N)}) > 1, "the branches did not diverge"
    assert g.debug_episodes_consumed().tolist() == [1] * N
    g.reset_envs(mask_of([0]))
    assert g.debug_episodes_consumed().tolist() == [2] + [1] * (N - 1)
    snap, _ = oracle_branch(-1, 0)
    assert diff_snapshots(snap, hip_snapshot(g, 0), A) == [], "the frozen env's next episode"
    fresh = raw(g, 0)
    assert fresh != saved
    g.sample_random_actions(POLICY_SEED, 99)
    step_ok(g)
    assert raw(g, 0) == fresh and g.step_mask() == "host"
    g.close()


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy"])
def test_all_zero_mask(hip, scenario):
    """8. nobody steps for 16 ticks (both forms, 8 ticks each): no snapshot and no consumed count changes, rewards and dones are zero bits, true objectives
    stay, every frame is the frame before; the ticks are counted.  The status word has no read hook of its own: its per-env part is the consumed count read
    here, and its flag bits are what a stepping call reports as a warning -- every call returns 0"""
    A = 1
    g = make_gym(scenario, A, "exact")
    for t in range(3):
        act(g, A, t)
        step_ok(g)
    before, frames, consumed, tobj = all_raw(g), slab(g, A).tobytes(), g.debug_episodes_consumed().tolist(), g.get_true_objectives().tobytes()
    zeros = device_mask(np.zeros(N, bool))
    for form in (zeros, np.zeros(N, bool)):
        g.set_step_mask(form)
        for t in range(8):
            act(g, A, 3 + t)
            step_ok(g)
            assert all_raw(g) == before and slab(g, A).tobytes() == frames
            assert g.get_rewards_array().tobytes() == bytes(4 * N * A) and g.get_dones().tobytes() == bytes(N)
            assert g.get_true_objectives().tobytes() == tobj and g.debug_episodes_consumed().tolist() == consumed
    assert g.ticks_since_reset() == 3 + 16
    g.close()
    del zeros


def test_all_ones_detach_and_reset(hip):
    """8. an all-ones mask and a mask attached and detached again are no mask, byte for byte; reset() with a mask attached resets every env and keeps the
    mask; a frozen env's pending actions are discarded, they do not wait for the thaw"""
    A = 1
    gU, gO, gD, gM = (make_gym("TowerBuilding", A, "exact") for _ in range(4))
    gO.set_step_mask(np.ones(N, bool))
    gD.set_step_mask(MASK)
    gD.set_step_mask(None)
    gM.set_step_mask(MASK)
    assert (gU.step_mask(), gO.step_mask(), gD.step_mask(), gM.step_mask()) == ("none", "host", "none", "host")
    for t in range(8):
        for g in (gU, gO, gD, gM):
            act(g, A, t)
            step_ok(g)
        for g in (gO, gD):
            assert all_raw(g) == all_raw(gU) and slab(g, A).tobytes() == slab(gU, A).tobytes()
            assert g.get_rewards_array().tobytes() == gU.get_rewards_array().tobytes() and g.get_dones().tobytes() == gU.get_dones().tobytes()
    assert [raw(gM, e) == raw(gU, e) for e in range(N)] == MASK.tolist()
    # reset(): every env of M takes its second episode, as every env of U does
    gM.reset()
    gU.reset()
    assert gM.step_mask() == "host"
    assert all_raw(gM) == all_raw(gU) and slab(gM, A).tobytes() == slab(gU, A).tobytes()
    assert gM.debug_episodes_consumed().tolist() == gU.debug_episodes_consumed().tolist() == [2] * N
    # ... and the mask still holds; the actions handed to the frozen envs for that tick are gone when they thaw
    fresh = all_raw(gM)
    act(gM, A, 50)
    step_ok(gM)
    assert [raw(gM, e) != fresh[e] for e in range(N)] == MASK.tolist()
    gM.set_step_mask(COMPLEMENT)   # (the envs that have not stepped yet step now, on NO action: nothing was set for this tick)
    step_ok(gM)
    step_ok(gU)                    # (U: one tick on no action from the same fresh episodes)
    assert [raw(gM, e) == raw(gU, e) for e in range(N)] == COMPLEMENT.tolist()
    for g in (gU, gO, gD, gM):
        g.close()


# ---- 9. the launch shape of the product ----------------------------------------------------------------------------------------------------------------
def test_launch_shape_1024_envs(hip):
    """9. TowerBuilding, 1024 envs x 32 x 32, exact pixels, rings 16 deep: step_n(16) with every odd env frozen, then step_n(16) with every even env frozen.
    Oracle E steps ticks 0..15, oracle O ticks 16..31, both from the reset: an even env is E's, an odd env O's.  Rewards and dones of every tick, every
    env's snapshot at the end, and the frames of eight sampled envs (the last ring entry)."""
    import torch
    n, A, K = 1024, 1, 16
    sampled = [0, 1, 2, 511, 512, 777, 1022, 1023]
    even = np.arange(n) % 2 == 0
    g = MegaverseGym("TowerBuilding", W, H, n, A, 1, False, {})
    g.set_pixel_mode("exact")
    g.seed(ENV_SEED)
    g.reset()
    rings = (torch.zeros((K, n * A, H, W, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((K, n * A), dtype=torch.float32, device="cuda:0"),
             torch.zeros((K, n), dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    g.set_output_ring(K, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
    oracles = []
    for first in (0, K):
        og = oracle_lib.OracleGym("TowerBuilding", W, H, n, A, 1, False, {})
        og.seed(ENV_SEED)
        og.reset()
        rew, done = np.zeros((K, n * A), np.float32), np.zeros((K, n), np.uint8)
        for j in range(K):
            og.set_action_masks(action_masks(sample_actions(POLICY_SEED, first + j, n * A)))
            og.step_norender()
            rew[j], done[j] = og.get_last_rewards(), og.get_dones()
        oracles.append((og, rew, done))
    for c, steps in enumerate((even, ~even)):
        g.set_step_mask(steps)
        c0 = g.debug_launch_counts()
        g.step_n(K, "multidiscrete", POLICY_SEED, c * K)
        assert g.debug_launch_counts()[0] - c0[0] == 2, "16 ticks are two step launches of 8"
        g.synchronize()
        _, rew, done = oracles[c]
        want_rew, want_done = np.where(steps[None], rew, np.float32(0.0)), np.where(steps[None], done, np.uint8(0))
        assert rings[1].cpu().numpy().tobytes() == want_rew.astype(np.float32).tobytes(), f"call {c}: rewards"
        assert rings[2].cpu().numpy().tobytes() == want_done.astype(np.uint8).tobytes(), f"call {c}: dones"
    last = rings[0][K - 1].cpu().numpy()
    for e in range(n):
        og = oracles[0 if even[e] else 1][0]
        assert diff_snapshots(og.snapshot(e), hip_snapshot(g, e), A) == [], f"env {e}"
    for e in sampled:
        og = oracles[0 if even[e] else 1][0]
        og.render_env(e)
        assert np.array_equal(last[e], og.get_observation(e, 0)), f"frame of env {e}"
    for og, _, _ in oracles:
        og.close()
    g.close()


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """10. a gym in a group; mv_group_create and mv_step_many with a masked member; a closed gym; a wrong-shaped tensor (ValueError)"""
    import torch
    a, b = make_gym("TowerBuilding", 1, "fast"), make_gym("ObstaclesEasy", 1, "fast")
    lib = a._lib
    data = np.ones(N, np.uint8)
    handles = (C.c_void_p * 2)(a._g, b._g)
    a.set_step_mask(MASK)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == -1 and b"step mask" in lib.mv_last_error()
    before = all_raw(a), all_raw(b)
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) == -1 and b"step mask" in lib.mv_last_error()
    assert (all_raw(a), all_raw(b)) == before, "mv_step_many stepped a gym before it refused"
    a.set_step_mask(None)
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    for g in (a, b):
        for fn in (lib.mv_set_step_mask_host, lib.mv_set_step_mask):
            assert fn(g._g, data.ctypes.data) == -1 and b"mv_group" in lib.mv_last_error()
        assert lib.mv_get_step_mask(g._g) == 0
        with pytest.raises(RuntimeError, match="mv_group"):
            g.set_step_mask(MASK)
    assert lib.mv_group_destroy(grp) == 0
    with pytest.raises(ValueError, match="set_step_mask"):
        a.set_step_mask(torch.zeros(N + 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError, match="set_step_mask"):
        a.set_step_mask(torch.zeros(N, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError, match="set_step_mask"):
        a.set_step_mask(torch.zeros(N, dtype=torch.bool))
    with pytest.raises(ValueError, match="set_step_mask"):
        a.set_step_mask(np.zeros(N - 1, bool))
    assert a.step_mask() == "none"
    a.set_step_mask(MASK)   # (valid again once the group is gone)
    handle = a._g
    lib.mv_close(handle)
    for fn in (lib.mv_set_step_mask_host, lib.mv_set_step_mask):
        assert fn(handle, data.ctypes.data) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_step_mask(handle) == -1 and b"closed" in lib.mv_last_error()
    a.close(); b.close()


def test_before_the_first_reset_and_arena_bytes(hip):
    """the mask may be attached before the first mv_reset; the host form's buffer is counted in mv_arena_bytes from its first use"""
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    bytes0 = g.arena_bytes()
    g.set_step_mask(MASK)
    assert g.arena_bytes() == bytes0 + N and g.step_mask() == "host"
    g.set_step_mask(COMPLEMENT)
    assert g.arena_bytes() == bytes0 + N
    g.seed(ENV_SEED)
    g.reset()
    fresh = all_raw(g)
    act(g, 1, 0)
    step_ok(g)
    assert [raw(g, e) != fresh[e] for e in range(N)] == COMPLEMENT.tolist()
    g.close()


def test_host_form_many_times_without_a_synchronisation(hip):
    """the host form six times in a row with steps in flight and nothing synchronising (its pinned staging buffers are reused as their copies complete,
    asked for, never waited for): the last mask holds, every stepping call returns 0"""
    A = 1
    g, tw = make_gym("TowerBuilding", A, "fast"), make_gym("TowerBuilding", A, "fast")
    tw.set_step_mask(COMPLEMENT)
    for i in range(6):
        g.set_step_mask([MASK, np.zeros(N, bool), np.ones(N, bool)][i % 3] if i < 5 else COMPLEMENT)
    for t in range(4):
        for x in (g, tw):
            x.sample_random_actions(POLICY_SEED, t)
            step_ok(x)
        g.set_step_mask(COMPLEMENT)   # (again, between steps in flight)
    assert all_raw(g) == all_raw(tw) and slab(g, A).tobytes() == slab(tw, A).tobytes()
    g.close(); tw.close()


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------------
def test_env_freeze_and_thaw(hip):
    """MegaverseEnv.freeze / thaw / set_step_mask through step_device and step_sequence: the frozen envs' observations, rewards and dones"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    env = MegaverseEnv("TowerBuilding", N, 1, 1, False, None, img_w=W, img_h=H)
    env.seed(3)
    env.reset()
    for t in range(3):
        obs, rew, done = env.step_device(sample_actions(POLICY_SEED, t, N))
    env.env.synchronize()
    before, states = obs.cpu().numpy().copy(), all_raw(env.env)
    env.freeze([1, 2])
    env.freeze([5])
    assert env.env.step_mask() == "host"
    obs, rew, done = env.step_device(sample_actions(POLICY_SEED, 3, N))
    env.env.synchronize()
    after, now = obs.cpu().numpy(), all_raw(env.env)
    frozen = mask_of([1, 2, 5])
    assert [now[e] == states[e] for e in range(N)] == frozen.tolist()
    assert all(np.array_equal(before[e], after[e]) for e in np.flatnonzero(frozen))
    assert not rew.cpu().numpy()[frozen].any() and not done.cpu().numpy()[frozen].any()
    o, r, d = env.step_sequence(np.stack([sample_actions(POLICY_SEED, 4 + j, N) for j in range(4)]), render="none")
    env.env.synchronize()
    assert o is None and not r.cpu().numpy()[:, frozen].any()
    assert [raw(env.env, e) == states[e] for e in range(N)] == frozen.tolist()
    env.thaw([1])
    assert env.env.step_mask() == "host"
    env.thaw()
    assert env.env.step_mask() == "none"
    keep = torch.as_tensor(~frozen).to("cuda:0")
    env.set_step_mask(keep)
    assert env.env.step_mask() == "device"
    env.step_device(sample_actions(POLICY_SEED, 8, N))
    env.set_step_mask(None)
    assert env.env.step_mask() == "none"
    with pytest.raises(ValueError, match="freeze"):
        env.freeze([N])
    env.close()
    del keep
