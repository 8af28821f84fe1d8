"""Action rings (include/megaverse_hip.h: mv_set_action_ring, MV_POLICY_SEQUENCE): batched calls that replay GIVEN actions.

The scripts are purposeful (tests/action_ring_util.py: make_script), so the one-launch step kernels and the batched observation launches are compared on
ticks that earn rewards and finish episodes -- against the CPU oracle, against the tick-by-tick path (mv_set_actions_device + mv_step) and against the
reference's own recorded rollout (tests/golden/py_surface_collect_a1)."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
import py_surface
from action_ring_util import CALLS, CASES, EPISODE_SEC, TICKS, WARMUP, make_script
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_ring_entry

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 36, 16
PARAMS = {"episodeLengthSec": EPISODE_SEC}
BOXOBAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban")
# cases the oracle cannot pin at this size or pins elsewhere: against single ticks only
EXTRA = {"sokoban": ("Sokoban", 6, 1), "boxagone": ("BoxAGone", 5, 1), "football": ("Football", 5, 1)}
BATCHED = [c for c in CASES if c != "obstacles_easy_a2"]   # every case with a multi-tick step kernel (several agents: TowerBuilding only)


def rings_of(torch, count, N, A, layout="rgba"):
    frame = (3, H, W) if layout == "chw" else (H, W, 4)
    t = (torch.zeros((count, N * A) + frame, dtype=torch.uint8, device="cuda:0"), torch.full((count, N * A), -7.0, dtype=torch.float32, device="cuda:0"),
         torch.full((count, N), 9, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    return t


def make_gym(scenario, N, A, mode, warmup=0, layout="rgba", params=PARAMS, w=W, h=H, seed=42):
    g = MegaverseGym(scenario, w, h, N, A, 1, False, params)
    if layout != "rgba":
        g.set_obs_layout(layout)
    g.set_pixel_mode(mode)
    g.seed(seed)
    g.reset()
    for _ in range(warmup):   # idle ticks up to the window the script plays in (tests/action_ring_util.py: WARMUP)
        g.step_no_render()
    return g


def attach(g, rings):
    g.set_output_ring(rings[0].shape[0], rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())


def host(rings):
    return [r.cpu().numpy() for r in rings]


def single_ticks(g, dev_script, entries):
    """the path callers had before: one mv_set_actions_device + mv_step per tick, fed the given ring entries"""
    for e in entries:
        g.set_actions_device(dev_script[e].data_ptr())
        g.step()


def assert_rings_equal(a, b, what):
    for x, y, name in zip(host(a), host(b), ("observations", "rewards", "dones")):
        assert x.tobytes() == y.tobytes(), f"{what}: {name} rings differ"


def assert_states_equal(a, b, N, what):
    for e in range(N):
        assert a.debug_snapshot_bytes(e).tobytes() == b.debug_snapshot_bytes(e).tobytes(), f"{what}: state of env {e}"


@functools.lru_cache(maxsize=None)
def oracle_rollout(case):
    """the oracle's side of a case, computed once: per tick (frames [N*A, H, W, 4], rewards, dones), and the final snapshots"""
    scenario, N, A = CASES[case]
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, PARAMS)
    og.seed(42)
    og.reset()
    for _ in range(WARMUP[case][0]):
        og.step_norender()
    script = make_script(WARMUP[case][1], TICKS, N * A)
    ticks = []
    for t in range(TICKS):
        for e in range(N):
            for a in range(A):
                og.set_actions(e, a, script[t, e * A + a].tolist())
        og.step()
        ticks.append((np.stack([og.get_observation(e, a) for e in range(N) for a in range(A)]).copy(), og.get_last_rewards().copy(), og.get_dones().copy()))
    snaps = [og.snapshot(e).copy() for e in range(N)]
    og.close()
    return script, ticks, snaps


def test_shortest_episodes_that_still_batch(hip):
    """EPISODE_SEC is the shortest episodeLengthSec (to 0.01 s) for which calls are still batched: an auto-reset falls inside a call"""
    for sec, want_batched in ((EPISODE_SEC, True), (EPISODE_SEC - 0.01, False)):
        g = MegaverseGym("Rearrange", W, H, 6, 1, 1, False, {"episodeLengthSec": sec})
        assert (g.recommended_ticks_per_call() >= 8) == want_batched, (sec, g.recommended_ticks_per_call())
        g.close()


@pytest.mark.parametrize("case", list(CASES))
def test_sequence_calls_equal_the_oracle(hip, case):
    """1. a 96-tick script out of a 96-entry ring in calls of 8, 16, 5, 16, 3, 16, 16, 16 into output rings 16 deep == the oracle fed the same actions tick by
    tick: rewards as bit patterns, dones and exact-mode frames of every ring entry before it is overwritten, every env's state at the end."""
    import torch
    scenario, N, A = CASES[case]
    script, ticks, snaps = oracle_rollout(case)
    # the oracle's side: the script is purposeful in this window
    assert any((r != 0).any() for _, r, _ in ticks), "the oracle earns no reward in the compared window"
    assert any(d.any() for _, _, d in ticks), "the oracle finishes no episode in the compared window"
    hg = make_gym(scenario, N, A, "exact", WARMUP[case][0])
    assert hg.recommended_ticks_per_call() >= 8
    dev_script = torch.as_tensor(script).to("cuda:0")
    rings = rings_of(torch, DEPTH, N, A)
    attach(hg, rings)
    hg.set_action_ring(TICKS, dev_script.data_ptr())
    first = 0
    for k in CALLS:
        hg.step_n(k, "sequence", 0, first)
        hg.synchronize()
        o, r, d = host(rings)
        for t in range(first, first + k):
            wo, wr, wd = ticks[t]
            j = t % DEPTH
            assert r[j].tobytes() == wr.tobytes(), f"rewards, tick {t}: {r[j]} vs {wr}"
            assert np.array_equal(d[j], wd), f"dones, tick {t}"
            assert np.array_equal(o[j], wo), f"frames, tick {t}: {np.argwhere((o[j] != wo).any(axis=(1, 2, 3))).ravel().tolist()}"
        first += k
    assert first == TICKS
    for e in range(N):
        assert diff_snapshots(snaps[e], hip_snapshot(hg, e), A) == [], f"state of env {e}"
    hg.close()


def run_against_single_ticks(scenario, N, A, warmup, seed, layout="rgba", overlap=False, depth=DEPTH):
    import torch
    script = make_script(seed, TICKS, N * A)
    dev_script = torch.as_tensor(script).to("cuda:0")
    seq, ref = make_gym(scenario, N, A, "fast", warmup, layout), make_gym(scenario, N, A, "fast", warmup, layout)
    rs, rr = rings_of(torch, depth, N, A, layout), rings_of(torch, depth, N, A, layout)
    attach(seq, rs)
    attach(ref, rr)
    if overlap:
        seq.set_pass_overlap(True)
    seq.set_action_ring(TICKS, dev_script.data_ptr())
    first = 0
    for k in CALLS:
        seq.step_n(k, "sequence", 0, first)
        single_ticks(ref, dev_script, range(first, first + k))
        seq.synchronize()
        ref.synchronize()
        assert_rings_equal(rs, rr, f"{scenario} after the call at tick {first}")
        first += k
    assert_states_equal(seq, ref, N, scenario)
    assert seq.get_true_objectives().tobytes() == ref.get_true_objectives().tobytes()
    seq.close()
    ref.close()


@pytest.mark.parametrize("case", list(CASES) + list(EXTRA))
def test_sequence_calls_equal_single_ticks(hip, case, monkeypatch):
    """2. the same calls in fast pixel mode == mv_set_actions_device + mv_step per tick: whole rings byte for byte after every call, state at the end"""
    monkeypatch.setenv("BOXOBAN_LEVELS", BOXOBAN)
    scenario, N, A = CASES.get(case) or EXTRA[case]
    warmup, seed = WARMUP.get(case, (0, 3))
    run_against_single_ticks(scenario, N, A, warmup, seed)


def test_sequence_calls_equal_single_ticks_chw(hip):
    """2. ... a gym that writes planar frames"""
    run_against_single_ticks("TowerBuilding", 7, 1, *WARMUP["tower"], layout="chw")


def test_sequence_calls_equal_single_ticks_overlapped_passes(hip):
    """2. ... overlapped passes (rings two calls deep: 32)"""
    run_against_single_ticks("Rearrange", 6, 1, *WARMUP["rearrange"], overlap=True, depth=32)


@pytest.mark.parametrize("case", list(CASES))
def test_launch_shape_is_the_batched_one(hip, case):
    """3. a sequence call takes the launches a random-policy call takes: the one-launch step kernels and the batched observation launch wherever they exist
    (every one-agent case, TowerBuilding with three agents), 16 launches of each where they do not (ObstaclesEasy with two agents)"""
    import torch
    scenario, N, A = CASES[case]
    script = torch.as_tensor(make_script(5, 16, N * A)).to("cuda:0")
    deltas = []
    for policy in ("sequence", "multidiscrete"):
        g = make_gym(scenario, N, A, "fast")
        rings = rings_of(torch, DEPTH, N, A)
        attach(g, rings)
        if policy == "sequence":
            g.set_action_ring(16, script.data_ptr())
        g.step_n(16, policy, 7, 0)   # (the first call after a reset: both twins in the same state)
        before = g.debug_launch_counts()
        g.step_n(16, policy, 7, 16)
        after = g.debug_launch_counts()
        g.synchronize()
        deltas.append((after[0] - before[0], after[1] - before[1]))
        g.close()
    assert deltas[0] == deltas[1], f"sequence {deltas[0]} vs multidiscrete {deltas[1]}"
    if case in BATCHED:
        assert deltas[0][0] < 16, deltas   # (not one step launch per tick)
    else:
        assert deltas[0] == (16, 16), deltas


def test_ring_indexing(hip):
    """4. tick j of a call acts on entry (first_step_index + j) % count in uint32: a ring of 5, calls of 8 from 3 and from 2^32 - 4 (the index wraps), count 1"""
    import torch
    scenario, N, A = "TowerBuilding", 7, 1
    script = make_script(9, 5, N * A)
    dev_script = torch.as_tensor(script).to("cuda:0")
    seq, ref = make_gym(scenario, N, A, "fast"), make_gym(scenario, N, A, "fast")
    rs, rr = rings_of(torch, DEPTH, N, A), rings_of(torch, DEPTH, N, A)
    attach(seq, rs)
    attach(ref, rr)
    seq.set_action_ring(5, dev_script.data_ptr())
    for first in (3, 2 ** 32 - 4):
        seq.step_n(8, "sequence", 0, first)
        entries = [action_ring_entry(first, j, 5) for j in range(8)]
        assert entries == [((first + j) % 2 ** 32) % 5 for j in range(8)]
        single_ticks(ref, dev_script, entries)
        seq.synchronize(); ref.synchronize()
        assert_rings_equal(rs, rr, f"first_step_index {first}")
    seq.set_action_ring(1, dev_script[2].data_ptr())   # action repeat
    seq.step_n(8, "sequence", 0, 77)
    single_ticks(ref, dev_script, [2] * 8)
    seq.synchronize(); ref.synchronize()
    assert_rings_equal(rs, rr, "count = 1")
    assert_states_equal(seq, ref, N, "indexing")
    seq.close(); ref.close()


def test_errors(hip):
    """no ring: an error with text; mv_set_sample_policy does not take the sequence policy; count = 0 detaches"""
    import torch
    g = make_gym("TowerBuilding", 3, 1, "fast")
    with pytest.raises(RuntimeError, match="no action ring"):
        g.step_n(4, "sequence", 0, 0)
    with pytest.raises(RuntimeError):
        g.set_sample_policy("sequence")
    with pytest.raises(RuntimeError):
        g.set_action_ring(4, 0)
    script = torch.as_tensor(make_script(1, 4, 3)).to("cuda:0")
    g.set_action_ring(4, script.data_ptr())
    g.step_n(4, "sequence", 0, 0)
    g.set_action_ring(0)
    with pytest.raises(RuntimeError, match="no action ring"):
        g.step_n(4, "sequence", 0, 0)
    g.synchronize()
    g.close()


def test_group_replays_every_members_ring(hip):
    """5. a group: Collect first (the long-lists-last reorder of the union launch moves it, and its ring with it), rings of 8, a 40-tick script in calls of 8 ==
    three gyms of their own stepped tick by tick on the same per-env actions; two launches per call; a member without a ring is named"""
    import torch
    from megaverse_amd.multitask import MultiTaskGym, split_action_ring
    names, NE, K, T = ["Collect", "TowerBuilding", "ObstaclesEasy"], 12, 8, 40
    S, n = len(names), NE // len(names)
    mt = MultiTaskGym(names, W, H, NE, 1, 1, PARAMS)
    mt.set_pixel_mode("fast")
    mt.seed(42)
    mt.reset()
    ring_obs, ring_rew, ring_done = mt.set_output_ring(K)
    script = make_script(4, T, NE)
    parts = mt.set_action_ring(torch.as_tensor(script).to("cuda:0"))
    for k, p in enumerate(parts):   # locate's rule: global env i is local env i // S of sub-gym i % S
        assert np.array_equal(p.cpu().numpy(), script[:, k::S]), k
        assert np.array_equal(p.cpu().numpy(), split_action_ring(script, S, 1)[k])
    refs, ref_rings = [], []
    for k, name in enumerate(names):
        g = MegaverseGym(name, W, H, n, 1, 1, False, PARAMS, env_offset=k, total_envs=NE, env_stride=S)
        g.set_pixel_mode("fast"); g.seed(42); g.reset()
        ref_rings.append(rings_of(torch, K, n, 1))
        attach(g, ref_rings[-1])
        refs.append(g)
    for first in range(0, T, K):
        before = mt.gyms[0].debug_launch_counts()
        mt.step_n(K, "sequence", 0, first)
        after = mt.gyms[0].debug_launch_counts()
        assert (after[0] - before[0], after[1] - before[1]) == (1, 1), (first, before, after)
        assert mt.gyms[2].debug_launch_counts() == after   # (a member reports the group's launches)
        for k, g in enumerate(refs):
            single_ticks(g, parts[k], range(first, first + K))
            g.synchronize()
        mt.synchronize()
        for k in range(S):
            assert_rings_equal((ring_obs[k], ring_rew[k], ring_done[k]), ref_rings[k], f"{names[k]}, call at tick {first}")
    for k, g in enumerate(refs):
        assert_states_equal(mt.gyms[k], g, n, names[k])
        assert mt.gyms[k].get_true_objectives().tobytes() == g.get_true_objectives().tobytes(), names[k]
    mt.gyms[1].set_action_ring(0)
    with pytest.raises(RuntimeError, match="gym 1 "):
        mt.step_n(K, "sequence", 0, T)
    mt.synchronize()
    for g in refs:
        g.close()
    mt.close()


def test_rewritten_ring_is_ordered_before_the_next_call(hip):
    """6. entries rewritten by a kernel on the gym's stream, mv_set_action_ring again, mv_step_n -- no host synchronisation in between: the call acts on the
    new entries (a twin gym that had them from the start)"""
    import torch
    scenario, N, A, K = "TowerBuilding", 7, 1, 8
    x, y = make_script(1, K, N * A), make_script(2, K, N * A)
    assert not np.array_equal(x, y)
    seq, twin = make_gym(scenario, N, A, "fast"), make_gym(scenario, N, A, "fast")
    rs, rt = rings_of(torch, DEPTH, N, A), rings_of(torch, DEPTH, N, A)
    attach(seq, rs)
    attach(twin, rt)
    ring, dev_x, dev_y = torch.as_tensor(x).to("cuda:0"), torch.as_tensor(x).to("cuda:0"), torch.as_tensor(y).to("cuda:0")
    torch.cuda.synchronize()
    seq.set_action_ring(K, ring.data_ptr())
    seq.step_n(K, "sequence", 0, 0)
    torch.add(dev_y, 0, out=ring)   # (the gym's stream is torch's current one: the null stream)
    seq.set_action_ring(K, ring.data_ptr())
    seq.step_n(K, "sequence", 0, 0)
    twin.set_action_ring(K, dev_x.data_ptr())
    twin.step_n(K, "sequence", 0, 0)
    twin.set_action_ring(K, dev_y.data_ptr())
    twin.step_n(K, "sequence", 0, 0)
    seq.synchronize(); twin.synchronize()
    assert_rings_equal(rs, rt, "after the rewrite")
    assert_states_equal(seq, twin, N, "after the rewrite")
    # ... and the rewrite mattered: the same gym without it ends elsewhere
    stale = make_gym(scenario, N, A, "fast")
    attach(stale, rt)
    stale.set_action_ring(K, dev_x.data_ptr())
    stale.step_n(K, "sequence", 0, 0)
    stale.step_n(K, "sequence", 0, 0)
    stale.synchronize()
    assert any(stale.debug_snapshot_bytes(e).tobytes() != seq.debug_snapshot_bytes(e).tobytes() for e in range(N))
    for g in (seq, twin, stale):
        g.close()


def test_an_attached_ring_changes_nothing_else(hip):
    """7. with a ring attached, mv_step, mv_sample_random_actions + mv_step and mv_step_n with a random policy give the bytes of a twin gym without one"""
    import torch
    scenario, N, A = "TowerBuilding", 7, 1
    script = torch.as_tensor(make_script(6, 8, N * A)).to("cuda:0")
    a, b = make_gym(scenario, N, A, "fast"), make_gym(scenario, N, A, "fast")
    ra, rb = rings_of(torch, DEPTH, N, A), rings_of(torch, DEPTH, N, A)
    attach(a, ra)
    attach(b, rb)
    a.set_action_ring(8, script.data_ptr())
    for g in (a, b):
        g.step()
        g.sample_random_actions(3, 0); g.step()
        g.set_actions_device(script[1].data_ptr()); g.step()
        g.step_n(8, "multidiscrete", 3, 1)
        g.step_n(4, "none", 0, 0)
        g.synchronize()
    assert_rings_equal(ra, rb, "ring attached / not attached")
    assert_states_equal(a, b, N, "ring attached / not attached")
    a.close(); b.close()


def test_reference_recorded_rollout_replayed(hip):
    """8. the reference's own recorded rollout (tests/golden/py_surface_collect_a1: the actions its purposeful controller chose) on a bare gym in exact pixels,
    once through mv_step_n(sequence) and once through single ticks: equal rings and state; the recorded frames of ticks 100 / 200 / 300 are the ring entries of
    those ticks after the fixture's CHW conversion (RGB of the RGBA frame, transposed: megaverse_env.py:121-130).  The fixture's rewards ARE the gym's raw
    rewards for this case -- py_surface.replay compares them with what MegaverseEnv.step returns, which is get_last_rewards() untouched, and the case has no
    shaping schedule and no team-spirit annealing -- so they are compared, as float32 bit patterns."""
    import torch
    rec, data = py_surface.load("collect_a1")
    spec, case = rec["spec"], py_surface.CASES["collect_a1"]
    assert all(spec[k] == case[k] for k in ("scenario", "num_envs", "agents", "seed", "steps", "params"))
    N, A, T = spec["num_envs"], spec["agents"], spec["steps"]
    w, h = rec["img"][0], rec["img"][1]
    actions = np.ascontiguousarray(data["actions"], dtype=np.int32)
    assert actions.shape == (T, N * A, 6)
    dev = torch.as_tensor(actions).to("cuda:0")
    shaping_at = case["shaping_at"]   # {step: (actor, {key: value})}, applied before that step
    assert {int(k): v for k, v in rec["shaping_at"].items()} == {k: list(v) for k, v in shaping_at.items()}
    cuts = sorted(set([0, T] + [s for s in shaping_at if 0 < s < T]))

    def make():
        g = make_gym(spec["scenario"], N, A, "exact", params=spec["params"], w=w, h=h, seed=spec["seed"])
        frame = (h, w, 4)
        rings = (torch.zeros((T, N * A) + frame, dtype=torch.uint8, device="cuda:0"), torch.zeros((T, N * A), dtype=torch.float32, device="cuda:0"),
                 torch.zeros((T, N), dtype=torch.uint8, device="cuda:0"))
        torch.cuda.synchronize()
        attach(g, rings)
        return g, rings

    def shape(g, st):
        if st in shaping_at:
            actor, upd = shaping_at[st]
            cur = g.get_reward_shaping(actor // A, actor % A)
            cur.update(upd)
            g.set_reward_shaping(actor // A, actor % A, cur)

    seq, rs = make()
    ref, rr = make()
    seq.set_action_ring(T, dev.data_ptr())
    for lo, hi in zip(cuts[:-1], cuts[1:]):   # calls split where the fixture changes the shaping
        for g in (seq, ref):
            shape(g, lo)
        seq.step_n(hi - lo, "sequence", 0, lo)
        single_ticks(ref, dev, range(lo, hi))
    seq.synchronize(); ref.synchronize()
    assert_rings_equal(rs, rr, "collect_a1")
    assert_states_equal(seq, ref, N, "collect_a1")
    o, r, d = host(rs)
    for st in (100, 200, 300):
        assert np.array_equal(o[st - 1][..., :3].transpose(0, 3, 1, 2), data[f"frames_{st}"]), f"frames after step {st}"
    assert r.tobytes() == data["rewards"].astype(np.float32).tobytes() and np.array_equal(data["rewards"].astype(np.float32).astype(np.float64), data["rewards"])
    assert np.array_equal(np.repeat(d.astype(bool), A, axis=1), data["dones"])
    assert (r != 0).sum() >= spec["min_nonzero_rewards"] and d.any()
    seq.close(); ref.close()


@pytest.mark.parametrize("layout", ["rgba", "chw"])
def test_env_step_sequence(hip, layout):
    """MegaverseEnv.step_sequence: k = 20 ticks (more than one call holds) from a numpy array and from a device tensor == step_device tick by tick"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    N, A, K = 6, 2, 20
    script = make_script(8, 2 * K, N * A)

    def make():
        e = MegaverseEnv("TowerBuilding", N, A, 1, False, PARAMS, img_w=W, img_h=H, obs_layout=layout)
        e.env.set_pixel_mode("fast")
        e.seed(3)
        e.reset()
        return e

    a, b = make(), make()
    want = []
    for t in range(2 * K):
        o, r, d = b.step_device(script[t])
        want.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy()))
    for part, acts in enumerate((script[:K], torch.as_tensor(script[K:]).to("cuda:0"))):
        o, r, d = a.step_sequence(acts)
        assert tuple(o.shape) == (K, N * A, 3, H, W) and tuple(r.shape) == (K, N * A) and tuple(d.shape) == (K, N)
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
        for j in range(K):
            wo, wr, wd = want[part * K + j]
            assert np.array_equal(o[j], wo) and r[j].tobytes() == wr.tobytes() and np.array_equal(d[j], wd), (part, j)
    # back on the single slab: the next ordinary step is the twin's
    oa, ra, da = a.step_device(script[0])
    ob, rb, db = b.step_device(script[0])
    assert np.array_equal(oa.cpu().numpy(), ob.cpu().numpy()) and ra.cpu().numpy().tobytes() == rb.cpu().numpy().tobytes()
    a.close(); b.close()
