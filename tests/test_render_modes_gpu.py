"""Render modes of batched calls (include/megaverse_hip.h: mv_step_n_render): k ticks simulated, none of them drawn (MV_RENDER_NONE) or the last only
(MV_RENDER_LAST) -- against the CPU oracle where frames and rewards are pinned to it (exact pixels), against a twin gym stepped with MV_RENDER_EVERY
everywhere else.  The scripts, windows and cases are the action-ring tests' (tests/action_ring_util.py); the oracle's rollout of a case is computed once
and shared with them (test_action_ring_gpu.oracle_rollout)."""
import numpy as np
import pytest

from action_ring_util import CALLS, CASES, EPISODE_SEC, TICKS, WARMUP, make_script
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import GymGroup, MegaverseGym
from test_action_ring_gpu import DEPTH, PARAMS, H, W, assert_states_equal, attach, host, make_gym, oracle_rollout

pytestmark = pytest.mark.gpu

SENT_OBS, SENT_REW, SENT_DONE = 0xA5, -7.0, 9
# the 96 ticks again, for MV_RENDER_LAST: a call of 16 is two step launches of 8, a call of 1 has nothing in front of its drawn tick
LAST_CALLS = [8, 16, 5, 16, 3, 16, 16, 15, 1]
assert sum(LAST_CALLS) == TICKS
MODES = ["none", "last", "every", "none", "every", "last"]


def sentinel_rings(torch, count, N, A, layout="rgba"):
    frame = (3, H, W) if layout == "chw" else (H, W, 4)
    t = (torch.full((count, N * A) + frame, SENT_OBS, dtype=torch.uint8, device="cuda:0"),
         torch.full((count, N * A), SENT_REW, dtype=torch.float32, device="cuda:0"), torch.full((count, N), SENT_DONE, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    return t


def oracle_side(case):
    script, ticks, snaps = oracle_rollout(case)
    assert any((r != 0).any() for _, r, _ in ticks), "the oracle earns no reward in the compared window"
    assert any(d.any() for _, _, d in ticks), "the oracle finishes no episode in the compared window"
    return script, ticks, snaps


@pytest.mark.parametrize("case", list(CASES))
def test_none_equals_the_oracle(hip, case):
    """1. the script in CALLS' sizes with render='none' into sentinel-filled rings 16 deep: per tick rewards (bit patterns) and dones are the oracle's, no
    byte of the observation ring is written, every env ends in the oracle's state"""
    import torch
    scenario, N, A = CASES[case]
    script, ticks, snaps = oracle_side(case)
    hg = make_gym(scenario, N, A, "exact", WARMUP[case][0])
    dev_script = torch.as_tensor(script).to("cuda:0")
    rings = sentinel_rings(torch, DEPTH, N, A)
    attach(hg, rings)
    hg.set_action_ring(TICKS, dev_script.data_ptr())
    first = 0
    for k in CALLS:
        hg.step_n(k, "sequence", 0, first, render="none")
        hg.synchronize()
        r, d = host(rings[1:])
        for t in range(first, first + k):
            _, wr, wd = ticks[t]
            assert r[t % DEPTH].tobytes() == wr.tobytes(), f"rewards, tick {t}: {r[t % DEPTH]} vs {wr}"
            assert np.array_equal(d[t % DEPTH], wd), f"dones, tick {t}"
        first += k
    assert first == TICKS
    assert bool((rings[0] == SENT_OBS).all()), "a render='none' call wrote into the observation ring"
    for e in range(N):
        assert diff_snapshots(snaps[e], hip_snapshot(hg, e), A) == [], f"state of env {e}"
    hg.close()


@pytest.mark.parametrize("case", list(CASES))
def test_last_equals_the_oracle(hip, case):
    """2. render='last': after each call the entry of its last tick holds the oracle's frames of that tick (exact pixels), rewards and dones of every tick are
    the oracle's, and the entries no last tick fell into are still sentinel; calls of 16 (two launches of 8) and of 1 included"""
    import torch
    scenario, N, A = CASES[case]
    script, ticks, snaps = oracle_side(case)
    hg = make_gym(scenario, N, A, "exact", WARMUP[case][0])
    dev_script = torch.as_tensor(script).to("cuda:0")
    rings = sentinel_rings(torch, DEPTH, N, A)
    attach(hg, rings)
    hg.set_action_ring(TICKS, dev_script.data_ptr())
    first, drawn = 0, set()
    for k in LAST_CALLS:
        hg.step_n(k, "sequence", 0, first, render="last")
        hg.synchronize()
        o, r, d = host(rings)
        for t in range(first, first + k):
            _, wr, wd = ticks[t]
            assert r[t % DEPTH].tobytes() == wr.tobytes(), f"rewards, tick {t}"
            assert np.array_equal(d[t % DEPTH], wd), f"dones, tick {t}"
        last = first + k - 1
        drawn.add(last % DEPTH)
        wo = ticks[last][0]
        assert np.array_equal(o[last % DEPTH], wo), f"frames, tick {last}: {np.argwhere((o[last % DEPTH] != wo).any(axis=(1, 2, 3))).ravel().tolist()}"
        for j in set(range(DEPTH)) - drawn:
            assert (o[j] == SENT_OBS).all(), f"entry {j} was written by the call that ended at tick {last}"
        first += k
    assert first == TICKS and 1 in LAST_CALLS and 16 in LAST_CALLS and len(drawn) < DEPTH
    for e in range(N):
        assert diff_snapshots(snaps[e], hip_snapshot(hg, e), A) == [], f"state of env {e}"
    hg.close()


def run_against_every(scenario, N, A, modes, calls=CALLS, warmup=0, seed=3, layout="rgba", policy="sequence", params=PARAMS, pipelined=True, rings=True,
                      log=0, pixels="fast"):
    """two gyms in one state; `a` takes calls[i] ticks in modes[i % len(modes)], its twin `b` the same ticks with render='every': rewards / dones rings (or,
    without rings, the public arrays) byte-equal after every call, observation entries wherever `a` drew, states and true objectives at the end.
    -> (a, b, the two gyms' rings) still open"""
    import torch
    script = torch.as_tensor(make_script(seed, TICKS, N * A)).to("cuda:0")
    a, b = (make_gym(scenario, N, A, pixels, warmup, layout, params) for _ in range(2))
    ra, rb = (sentinel_rings(torch, DEPTH, N, A, layout) if rings else None for _ in range(2))
    for g, r in ((a, ra), (b, rb)):
        if not pipelined:
            g.set_pipelining(False)
        if log:
            g.set_episode_log(log)
        if rings:
            attach(g, r)
        g.set_action_ring(TICKS, script.data_ptr())
    first = 0
    for i, k in enumerate(calls):
        mode = modes[i % len(modes)]
        a.step_n(k, policy, 11, first, render=mode)
        b.step_n(k, policy, 11, first)
        a.synchronize(); b.synchronize()
        what = f"{scenario}, {mode} call of {k} at tick {first}"
        if rings:
            assert ra[1].cpu().numpy().tobytes() == rb[1].cpu().numpy().tobytes(), f"{what}: rewards rings"
            assert ra[2].cpu().numpy().tobytes() == rb[2].cpu().numpy().tobytes(), f"{what}: dones rings"
            ticks = {"none": [], "last": [first + k - 1], "every": range(first, first + k)}[mode]
            for t in ticks:
                assert torch.equal(ra[0][t % DEPTH], rb[0][t % DEPTH]), f"{what}: frames of tick {t}"
        else:
            assert a.get_rewards_array().tobytes() == b.get_rewards_array().tobytes(), f"{what}: rewards"
            assert a.get_dones().tobytes() == b.get_dones().tobytes(), f"{what}: dones"
        assert a.get_true_objectives().tobytes() == b.get_true_objectives().tobytes(), f"{what}: true objectives"
        if log:
            assert torch.equal(a.episode_returns_tensor(), b.episode_returns_tensor()), f"{what}: running returns"
        first += k
    assert_states_equal(a, b, N, scenario)
    return a, b, ra, rb


@pytest.mark.parametrize("case,layout", [("tower", "rgba"), ("collect", "rgba"), ("tower_a3", "rgba"), ("tower", "chw")])
def test_modes_interleaved_equal_every(hip, case, layout):
    """3. calls cycling none, last, every, none, every, last on one gym == a twin stepped with 'every', default (fast) pixels; once more in the planar layout"""
    scenario, N, A = CASES[case]
    a, b, ra, _ = run_against_every(scenario, N, A, MODES, warmup=WARMUP[case][0], seed=WARMUP[case][1], layout=layout)
    assert bool((ra[1] != SENT_REW).all()) and bool((ra[2] != SENT_DONE).all())   # (every entry of the rewards / dones rings was published)
    a.close(); b.close()


@pytest.mark.parametrize("policy", ["sequence", "multidiscrete"])
def test_launch_shapes(hip, policy):
    """4. TowerBuilding 7 x 1 with rings: 'none' takes one step launch per 8 ticks and no observation launch; 'last' one observation launch and at most two
    step launches"""
    import torch
    N, A = 7, 1
    g = make_gym("TowerBuilding", N, A, "fast")
    rings = sentinel_rings(torch, DEPTH, N, A)
    attach(g, rings)
    script = torch.as_tensor(make_script(5, 16, N * A)).to("cuda:0")
    g.set_action_ring(16, script.data_ptr())

    def delta(k, mode, first):
        before = g.debug_launch_counts()
        g.step_n(k, policy, 7, first, render=mode)
        after = g.debug_launch_counts()
        return after[0] - before[0], after[1] - before[1]

    assert delta(8, "none", 0) == (1, 0)
    assert delta(16, "none", 8) == (2, 0)
    steps, passes = delta(8, "last", 24)
    assert passes == 1 and 1 <= steps <= 2, (steps, passes)
    steps, passes = delta(16, "last", 32)
    assert passes == 1 and steps == 2, (steps, passes)
    g.synchronize()
    assert bool((rings[0][[j for j in range(DEPTH) if j not in (31 % DEPTH, 47 % DEPTH)]] == SENT_OBS).all())
    g.close()


@pytest.mark.parametrize("case", ["rearrange", "obstacles_hard"])
@pytest.mark.parametrize("policy", ["multidiscrete", "single-bit"])
def test_in_kernel_policies(hip, case, policy):
    """5. 'none' with the policies drawn inside the step kernel == a twin running 'every' with the same (seed, first_step_index): states, rewards rings"""
    scenario, N, A = CASES[case]
    a, b, _, _ = run_against_every(scenario, N, A, ["none"], warmup=WARMUP[case][0], policy=policy)
    a.close(); b.close()


FALLBACKS = {
    "obstacles_easy_a2": dict(scenario="ObstaclesEasy", N=6, A=2, warmup=WARMUP["obstacles_easy_a2"][0]),   # no multi-tick step kernel
    "not_pipelined": dict(scenario="TowerBuilding", N=7, A=1, warmup=WARMUP["tower"][0], pipelined=False),   # the kernels write the public arrays themselves
    "no_rings": dict(scenario="Collect", N=5, A=1, warmup=WARMUP["collect"][0], rings=False),                # the public arrays hold the last tick's
    "tick_by_tick": dict(scenario="Rearrange", N=6, A=1, warmup=WARMUP["rearrange"][0], params={"episodeLengthSec": EPISODE_SEC - 0.01}),
    "boxagone": dict(scenario="BoxAGone", N=5, A=1), "football": dict(scenario="Football", N=5, A=1),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallback_paths(hip, name):
    """6. the shapes that take other launches, each against an 'every' twin in calls alternating none / last: states, rewards and dones equal"""
    kw = dict(FALLBACKS[name])
    scenario, N, A = kw.pop("scenario"), kw.pop("N"), kw.pop("A")
    a, b, _, _ = run_against_every(scenario, N, A, ["none", "last"], seed=WARMUP.get(name, (0, 3))[1], **kw)
    if name == "tick_by_tick":
        assert a.recommended_ticks_per_call() == 1
    if name == "obstacles_easy_a2":   # (one launch per tick)
        before = a.debug_launch_counts()
        a.step_n(8, "sequence", 0, 0, render="last")
        after = a.debug_launch_counts()
        a.synchronize()
        assert (after[0] - before[0], after[1] - before[1]) == (8, 1)
    a.close(); b.close()


def test_render_after_none_equals_the_oracle(hip):
    """7. mv_render behind a 'none' call draws the state the call left: the oracle's frames of the call's last tick (exact pixels), into the slab"""
    import torch
    case = "collect"
    scenario, N, A = CASES[case]
    script, ticks, _ = oracle_side(case)
    hg = make_gym(scenario, N, A, "exact", WARMUP[case][0])
    dev_script = torch.as_tensor(script).to("cuda:0")
    hg.set_action_ring(TICKS, dev_script.data_ptr())
    first = 0
    for k in (16, 5):
        hg.step_n(k, "sequence", 0, first, render="none")
        first += k
        hg.render()
        hg.synchronize()
        got = np.stack([hg.get_observation(e, a) for e in range(N) for a in range(A)])
        assert np.array_equal(got, ticks[first - 1][0]), f"mv_render after tick {first - 1}"
    assert hg.get_rewards_array().tobytes() == ticks[first - 1][1].tobytes()
    hg.close()


def test_episode_log(hip):
    """8. episode log on (256 records): the running returns are a twin's mid-run (every call), the records drained after 96 ticks of 'none' are its records"""
    case = "tower"
    scenario, N, A = CASES[case]
    a, b, _, _ = run_against_every(scenario, N, A, ["none"], warmup=WARMUP[case][0], seed=WARMUP[case][1], log=256)
    ra, rb = a.drain_episode_log(), b.drain_episode_log()
    assert len(ra) > 0, "no env finished in the compared window"
    assert ra.tobytes() == rb.tobytes()
    assert a.ticks_since_reset() == b.ticks_since_reset()
    a.close(); b.close()


def test_with_forks(hip):
    """9. fork_envs (env 0 into all), then 16 ticks of 'none' == the same on a twin with 'every'; then reset_envs of all destinations on both: still equal"""
    import torch
    case = "tower"
    scenario, N, A = CASES[case]
    script = torch.as_tensor(make_script(WARMUP[case][1], 16, N * A)).to("cuda:0")
    a, b = (make_gym(scenario, N, A, "fast", 40) for _ in range(2))
    fork = np.zeros(N, np.int32)
    fork[0] = -1
    mask = np.ones(N, bool)
    mask[0] = False
    for g, mode in ((a, "none"), (b, "every")):
        g.set_action_ring(16, script.data_ptr())
        g.step_n(8, "sequence", 0, 0, render=mode)
        g.fork_envs(fork)
        g.step_n(16, "sequence", 0, 0, render=mode)
        g.synchronize()
    assert_states_equal(a, b, N, "after the fork and 16 ticks")
    assert a.get_rewards_array().tobytes() == b.get_rewards_array().tobytes()
    for g in (a, b):
        g.reset_envs(mask, render=False)
        g.synchronize()
    assert_states_equal(a, b, N, "after the masked reset")
    for g, mode in ((a, "none"), (b, "every")):
        g.step_n(8, "sequence", 0, 0, render=mode)
        g.synchronize()
    assert_states_equal(a, b, N, "8 ticks after the masked reset")
    a.close(); b.close()


@pytest.mark.parametrize("layout", ["rgba", "chw"])
def test_env_step_sequence(hip, layout):
    """10. MegaverseEnv.step_sequence(actions, render=...): 'none' -> (None, rewards [k, ...], dones [k, ...]); 'last' -> observations [1, num_agents, 3, H, W],
    the last entry of what 'every' returns; rewards and dones equal across the three modes (k = 20: more than one step launch holds)"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    N, A, K = 6, 2, 20
    script = make_script(8, K, N * A)
    out = {}
    for mode in ("every", "last", "none"):
        e = MegaverseEnv("TowerBuilding", N, A, 1, False, PARAMS, img_w=W, img_h=H, obs_layout=layout)
        e.env.set_pixel_mode("fast")
        e.seed(3)
        e.reset()
        o, r, d = e.step_sequence(script, render=mode)
        e.env.synchronize()
        assert tuple(r.shape) == (K, N * A) and tuple(d.shape) == (K, N)
        out[mode] = (None if o is None else o.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy())
        if mode == "last":   # a second call reuses the rings; an ordinary step afterwards is back on the slab
            o2, r2, d2 = e.step_sequence(script, render="last")
            assert tuple(o2.shape) == (1, N * A, 3, H, W)
            e.step_device(script[0])
        e.close()
    assert out["none"][0] is None
    assert out["every"][0].shape == (K, N * A, 3, H, W) and out["last"][0].shape == (1, N * A, 3, H, W)
    assert np.array_equal(out["last"][0][0], out["every"][0][K - 1])
    for mode in ("last", "none"):
        assert out[mode][1].tobytes() == out["every"][1].tobytes(), f"rewards, {mode}"
        assert out[mode][2].tobytes() == out["every"][2].tobytes(), f"dones, {mode}"
    with pytest.raises(ValueError, match="render"):
        MegaverseEnv.step_sequence(None, script, render="first")


def test_refusals(hip):
    """11. an unknown mode, a gym in a group and a call before mv_reset: -1 with a text that names mv_step_n_render"""
    lib = hip.load_library()
    g = make_gym("TowerBuilding", 3, 1, "fast")
    assert lib.mv_step_n_render(g._g, 4, 1, 0, 0, 7) == -1
    assert "mv_step_n_render" in lib.mv_last_error().decode() and "mode" in lib.mv_last_error().decode()
    assert lib.mv_step_n_render(g._g, 4, 1, 0, 0, -1) == -1
    with pytest.raises(RuntimeError, match="mv_step_n_render.*action ring"):   # (what mv_step_n refuses)
        g.step_n(4, "sequence", 0, 0, render="none")
    with pytest.raises(RuntimeError, match="mv_step_n_render"):
        g.step_n(0, "multidiscrete", 0, 0, render="last")
    h = make_gym("TowerBuilding", 3, 1, "fast")
    grp = GymGroup([g, h])
    for mode in ("none", "last"):
        with pytest.raises(RuntimeError, match="mv_step_n_render.*group"):
            g.step_n(4, "multidiscrete", 0, 0, render=mode)
    grp.step(2, False, "multidiscrete", 1, 0)   # (the group's own render flag is what groups keep)
    g.synchronize()
    grp.close()
    fresh = MegaverseGym("TowerBuilding", W, H, 3, 1, 1, False, PARAMS)
    with pytest.raises(RuntimeError, match="mv_step_n_render.*mv_reset"):
        fresh.step_n(4, "multidiscrete", 0, 0, render="none")
    for x in (g, h, fresh):
        x.close()
