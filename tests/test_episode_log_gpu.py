"""GPU: the on-device episode log (include/megaverse_hip.h: mv_set_episode_log) against the log the CPU oracle's outputs imply.

Expected values never come from the library: the oracle (tests/oracle_lib.py) is stepped with the same seeds and the same actions (env seed 42, policy seed 7,
multidiscrete policy, tick index as step index) and the bookkeeping is done in numpy float64 (tests/episode_log_util.py: Model).  Comparison is tobytes()
equality of the drained records, of `dropped` and of the final ret / len.  Every rollout's floors are asserted on the EXPECTED log first."""
import ctypes as C
import os

import numpy as np
import pytest

import episode_log_util as U
import oracle_lib
from hip_util import hip_snapshot
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = pytest.mark.gpu

CAP = 1 << 16
# Host-generated scenarios (Collect, Sokoban) keep two episodes resident per env and refill them from a host feeder.  Sokoban's 64 envs all finish in the
# same tick, every 68 ticks: a feeder of one thread behind a host that enqueues hundreds of ticks ahead starves them, the envs repeat their done step (the
# library's documented warning) and the rollout is no longer the oracle's.  The gyms here get the feeder tests/test_refill_protocol_gpu.py uses (8
# threads), and the open-loop rollouts let the device catch up every fourth call.
FEEDER_THREADS = 8


def make_gym(hip, name, capacity=CAP, layout="rgba", pipelining=True, pixel_mode="fast", **shard):
    scenario, N, A, params, *_ = U.ALL_ROLLOUTS[name]
    U.boxoban_env()
    g = hip.MegaverseGym(scenario, U.W, U.H, shard.pop("num_envs", N), A, FEEDER_THREADS, False, params, **shard)
    g.set_pixel_mode(pixel_mode)   # (the batched one-launch paths are the fast pixel mode's)
    if layout != "rgba":
        g.set_obs_layout(layout)
    g.set_pipelining(pipelining)
    g.seed(U.ENV_SEED)
    if capacity:
        g.set_episode_log(capacity)
    g.reset()
    return g


def rings(g, count, layout="rgba"):
    import torch
    NA = g.num_envs * g.num_agents_per_env
    frame = (3, g.h, g.w) if layout == "chw" else (g.h, g.w, 4)
    t = (torch.zeros((count, NA) + frame, dtype=torch.uint8, device="cuda"), torch.zeros((count, NA), dtype=torch.float32, device="cuda"),
         torch.zeros((count, g.num_envs), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    g.set_output_ring(count, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    return t


def expected(name):
    want = U.expected_log(name)
    records = want.drain()
    U.assert_floors(name, records)
    return want, records


def check_final(g, want, records, got, dropped=0):
    assert got.dtype.itemsize == 24
    assert len(got) == len(records), (len(got), len(records))
    assert got.tobytes() == records.tobytes()
    assert g.episode_log_count() == (0, dropped)
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == want.ret.tobytes()
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == want.len.tobytes()
    assert g.ticks_since_reset() == want.tick


@pytest.mark.parametrize("drain_every", [50, 0])
@pytest.mark.parametrize("name", sorted(U.ROLLOUTS))
def test_mv_step_per_tick(hip, name, drain_every):
    ticks = U.ROLLOUTS[name][4]
    want, records = expected(name)
    g = make_gym(hip, name)
    parts = []
    for t in range(ticks):
        g.sample_random_actions(U.POLICY_SEED, t)
        g.step() if t % 3 else g.step_no_render()   # (mv_step and mv_step_no_render)
        if drain_every and (t + 1) % drain_every == 0:
            parts.append(g.drain_episode_log())
        elif t % 64 == 63:
            g.synchronize()   # (FEEDER_THREADS: the host does not run hundreds of ticks ahead of the episode feeder)
    parts.append(g.drain_episode_log())
    check_final(g, want, records, np.concatenate(parts))
    g.close()


SHAPES = {
    # call size, ring depth, pass overlap, pipelining, layout
    "n16_ring16": (16, 16, False, True, "rgba"),
    "n16_no_ring": (16, 0, False, True, "rgba"),
    "n16_ring32_overlap": (16, 32, True, True, "rgba"),
    "n40_split": (40, 0, False, True, "rgba"),
    "n40_split_ring80_overlap": (40, 80, True, True, "rgba"),
    "n16_ring16_not_pipelined": (16, 16, False, False, "rgba"),
    "n16_no_ring_not_pipelined": (16, 0, False, False, "rgba"),
    "n16_ring16_planar": (16, 16, False, True, "chw"),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(U.ROLLOUTS))
def test_mv_step_n(hip, name, shape):
    k, depth, overlap, pipelining, layout = SHAPES[shape]
    ticks = U.ROLLOUTS[name][4]
    assert ticks % k == 0
    want, records = expected(name)
    g = make_gym(hip, name, layout=layout, pipelining=pipelining)
    keep = rings(g, depth, layout) if depth else None
    if overlap:
        g.set_pass_overlap(True)
    for call, t0 in enumerate(range(0, ticks, k)):
        g.step_n(k, "multidiscrete", U.POLICY_SEED, t0)
        if call % 4 == 3:
            g.synchronize()
    check_final(g, want, records, g.drain_episode_log())
    g.close()
    del keep


@pytest.mark.parametrize("mode", ["mv_step", "n16_ring16", "n16_no_ring"])
@pytest.mark.parametrize("name", sorted(U.LARGE_ROLLOUTS))
def test_more_than_1024_agents(hip, name, mode):
    """The kernel's threads take several agents each: an env's agents in different waves and chunks (3 agents per env), the order across chunks (4 agents
    per env), more cells than threads in the scan (4160 agents x 16 ticks).  CAP is smaller than tower_1040x4's log: the test drains as it goes."""
    ticks = U.ALL_ROLLOUTS[name][4]
    want, records = expected(name)
    g = make_gym(hip, name)
    keep = rings(g, 16) if mode == "n16_ring16" else None
    parts = []
    for t in range(ticks):
        if mode == "mv_step":
            g.sample_random_actions(U.POLICY_SEED, t)
            g.step()
        elif t % 16 == 0:
            g.step_n(16, "multidiscrete", U.POLICY_SEED, t)
        if t % 16 == 15:
            parts.append(g.drain_episode_log())
    assert g.episode_log_dropped == 0
    check_final(g, want, records, np.concatenate(parts))
    g.close()
    del keep


@pytest.mark.parametrize("per_launch", [1, 5])
def test_a_call_split_over_several_launches(hip, monkeypatch, per_launch):
    """MV_EPISODE_LOG_TICKS caps the ticks of one launch: a call of 16 ticks takes several, as it does for gyms of more than 32768 agents"""
    name = "tower_short"
    want, records = expected(name)
    monkeypatch.setenv("MV_EPISODE_LOG_TICKS", str(per_launch))
    g = make_gym(hip, name)
    for t0 in range(0, U.ROLLOUTS[name][4], 16):
        g.step_n(16, "multidiscrete", U.POLICY_SEED, t0)
    check_final(g, want, records, g.drain_episode_log())
    g.close()


def test_device_pointers_and_partial_drain(hip):
    """the count and the records are readable on the device without a drain; a partial drain removes the oldest records and keeps the order"""
    import torch
    name = "tower_short"
    want, records = expected(name)
    g = make_gym(hip, name)
    for t in range(U.ROLLOUTS[name][4]):
        g.sample_random_actions(U.POLICY_SEED, t)
        g.step_no_render()
    g.flush_episode_log()
    g.synchronize()
    hdr = torch.as_tensor(hip._DeviceArray(g.episode_log_count_device_ptr(), (4,), "<u4"), device="cuda").cpu().numpy()
    assert int(hdr[0]) == len(records) and int(hdr[1]) == 0
    raw = torch.as_tensor(hip._DeviceArray(g.episode_log_records_device_ptr(), (len(records) * 24,), "|u1"), device="cuda").cpu().numpy()
    assert raw.tobytes() == records.tobytes()
    first = g.drain_episode_log(100)
    assert g.episode_log_count() == (len(records) - 100, 0)
    rest = g.drain_episode_log()
    assert first.tobytes() == records[:100].tobytes() and rest.tobytes() == records[100:].tobytes()
    assert g.arena_bytes() > CAP * 24
    g.close()


def group_members(hip, tower_len=4.5):
    """Collect + Sokoban + TowerBuilding, one agent per env, 480 ticks.  The oracle alone gives (checked on the CPU): Collect 128 envs 89 records, finishing
    at scattered ticks, Sokoban 64 envs 448, all in the same seven ticks; TowerBuilding 32 envs with episodeLengthSec 4.5 -- long episodes, which the group's batched path needs -- none
    (its running ret / len and its counter are what is compared), with -200 (the group then runs tick by tick) several hundred."""
    cfg = [("Collect", 128, {"episodeLengthSec": 4.5}, 70), ("Sokoban", 64, {"episodeLengthSec": 4.5}, 400),
           ("TowerBuilding", 32, {"episodeLengthSec": tower_len}, 0 if tower_len > 0 else 300)]
    U.boxoban_env()
    gyms, wants = [], []
    ticks = 480
    for scenario, N, params, floor in cfg:
        m = U.Model(N, 1)
        m.feed(*U.oracle_outputs(scenario, N, 1, tuple(sorted(params.items())), ticks))
        assert len(m.records) >= floor, (scenario, len(m.records))
        wants.append(m)
        g = hip.MegaverseGym(scenario, U.W, U.H, N, 1, FEEDER_THREADS, False, params)
        g.set_pixel_mode("fast")
        g.seed(U.ENV_SEED)
        g.set_episode_log(CAP)
        g.reset()
        gyms.append(g)
    return gyms, wants, ticks


@pytest.mark.parametrize("k", [8, 1])
def test_group_every_member_keeps_its_own_log(hip, k):
    """mv_group_step: the two-launch batched path (8 ticks per call, rings 8 deep) and the tick-by-tick one; each member against its own oracle"""
    gyms, wants, ticks = group_members(hip, tower_len=4.5 if k > 1 else -200.0)
    keep = [rings(g, 8) for g in gyms] if k > 1 else None
    grp = hip.GymGroup(gyms)
    for call, t0 in enumerate(range(0, ticks, k)):
        grp.step(k, True, "multidiscrete", U.POLICY_SEED, t0)
        if call % 4 == 3:
            gyms[0].synchronize()
    for g, want in zip(gyms, wants):
        records = want.drain()
        check_final(g, want, records, g.drain_episode_log())
    grp.close()
    for g in gyms:
        g.close()
    del keep


def test_group_log_switched_on_inside_a_group(hip):
    gyms, wants, ticks = group_members(hip)
    for g in gyms:
        g.set_episode_log(0)
    grp = hip.GymGroup(gyms)
    gyms[1].set_episode_log(CAP)   # Sokoban alone
    for t in range(ticks):
        grp.step(1, True, "multidiscrete", U.POLICY_SEED, t)
        if t % 4 == 3:
            gyms[0].synchronize()
    records = wants[1].drain()
    check_final(gyms[1], wants[1], records, gyms[1].drain_episode_log())
    grp.close()
    for g in gyms:
        g.close()


def test_mv_step_many_every_gym_keeps_its_own_log(hip):
    names, ticks = ["tower_short", "boxagone"], 320
    gyms = [make_gym(hip, n) for n in names]
    handles = (C.c_void_p * 2)(*[g._g for g in gyms])
    lib = gyms[0]._lib
    for t in range(ticks):
        assert lib.mv_step_many(handles, 2, 1, 1, U.POLICY_SEED, t) >= 0, lib.mv_last_error()
        if t % 64 == 63:
            gyms[0].synchronize()
    for n, g in zip(names, gyms):
        _, N, A, *_ = U.ROLLOUTS[n]
        expected(n)   # (the rollout's floors)
        m = U.Model(N, A)
        m.feed(*[x[:ticks] for x in U.rollout(n)])
        records = m.drain()
        assert len(records) >= 30
        check_final(g, m, records, g.drain_episode_log())
        g.close()


def test_pybind_module_drains_the_same_records(hip):
    """megaverse_amd/pybind: set_episode_log / episode_log_count / drain_episode_log beside the reference's table"""
    from megaverse_amd.pybind import megaverse as m
    name = "boxagone"
    scenario, N, A, params, ticks, *_ = U.ROLLOUTS[name]
    want, records = expected(name)
    g = m.MegaverseGym(scenario, U.W, U.H, N, A, 1, False, params)
    g.seed(U.ENV_SEED)
    g.set_episode_log(256)
    g.reset()
    for t in range(ticks):
        acts = sample_actions(U.POLICY_SEED, t, N * A)
        for e in range(N):
            for a in range(A):
                g.set_actions(e, a, acts[e * A + a].tolist())
        g.step()
    g.flush_episode_log()
    assert tuple(g.episode_log_count()) == (len(records), 0)
    got = g.drain_episode_log()
    assert got.dtype.itemsize == 24 and got.dtype.names == U.RECORD.names
    assert got.tobytes() == records.tobytes()
    assert tuple(g.episode_log_count()) == (0, 0) and g.episode_returns_device_ptr() != 0 and g.episode_lengths_device_ptr() != 0
    g.close()


def test_multitask_gym_drains_one_array_in_batch_numbering(hip):
    from megaverse_amd.multitask import MULTITASK_EPISODE_DTYPE, MultiTaskGym
    U.boxoban_env()
    scenarios, per, ticks, params = ["Collect", "Sokoban"], 16, 320, {"episodeLengthSec": 4.5}
    mt = MultiTaskGym(scenarios, U.W, U.H, per * 2, 1, FEEDER_THREADS, params)
    mt.set_pixel_mode("fast")
    mt.seed(U.ENV_SEED)
    mt.set_episode_log(4096)
    mt.reset()
    for t in range(ticks):
        mt.sample_random_actions(U.POLICY_SEED, t)
        mt.step()
        if t % 64 == 63:
            mt.synchronize()
    got = mt.drain_episode_log()
    # (Sokoban's episodes of 4.5 s are 68 ticks long: four whole ones per env in 320 ticks)
    assert got.dtype == MULTITASK_EPISODE_DTYPE and int((got["task"] == 1).sum()) >= 4 * per
    key = got["end_tick"].astype(np.int64) * (1 << 20) + got["agent"]
    assert (np.diff(key) > 0).all()
    for r in got:
        g, local = mt.locate(int(r["agent"]))
        assert g is mt.gyms[int(r["task"])] and 0 <= local < per
    assert (got["length"][got["task"] == 1] <= 68).all() and (got["length"] >= 1).all()
    # every env's lengths add up to the ticks between its records
    for agent in np.unique(got["agent"]):
        mine = got[got["agent"] == agent]
        assert (np.cumsum(mine["length"]) == mine["end_tick"].astype(np.int64) + 1).all()
    assert mt.episode_log_count() == (0, 0)
    mt.close()


@pytest.mark.parametrize("name", ["tower_short", "sokoban"])
def test_sharded_pair_equals_the_unsharded_log(hip, name):
    _, N, A, _, ticks, *_ = U.ROLLOUTS[name]
    want, records = expected(name)
    half = N // 2
    shards = [make_gym(hip, name, num_envs=half, env_offset=off, total_envs=N) for off in (0, half)]
    parts = []
    for off, g in zip((0, half), shards):
        for call, t0 in enumerate(range(0, ticks, 16)):
            g.step_n(16, "multidiscrete", U.POLICY_SEED, t0)
            if call % 4 == 3:
                g.synchronize()
        r = g.drain_episode_log()
        assert (r["agent"] < half * A).all()   # indices stay local
        r["agent"] += off * A
        parts.append(r)
        assert g.episode_returns_tensor().cpu().numpy().tobytes() == want.ret[off * A:(off + half) * A].tobytes()
        g.close()
    both = np.concatenate(parts)
    both = both[np.lexsort((both["agent"], both["end_tick"]))]
    assert both.tobytes() == records.tobytes()


def test_overflow_is_reported_once_and_stepping_goes_on(hip):
    name = "tower_short"
    ticks = U.ROLLOUTS[name][4]
    want, records = expected(name)
    g = make_gym(hip, name, capacity=64)
    lib = g._lib
    reports = 0
    for t in range(ticks):
        g.sample_random_actions(U.POLICY_SEED, t)
        rc = lib.mv_step(g._g)
        assert rc >= 0, lib.mv_last_error()
        if rc == 1 and b"episode log" in lib.mv_last_error():
            reports += 1
    assert reports == 1
    got = g.drain_episode_log()
    assert got.tobytes() == records[:64].tobytes()
    assert g.episode_log_dropped == len(records) - 64
    assert g.episode_log_count() == (0, len(records) - 64)
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == want.ret.tobytes()   # accumulators are reset all the same
    assert g.episode_lengths_tensor().cpu().numpy().tobytes() == want.len.tobytes()
    g.close()


def oracle_with_reset(name, reset_at):
    scenario, N, A, params, ticks, *_ = U.ROLLOUTS[name]
    og = oracle_lib.OracleGym(scenario, U.W, U.H, N, A, 1, False, params)
    og.seed(U.ENV_SEED)
    og.reset()
    m = U.Model(N, A)
    for t in range(ticks):
        if t == reset_at:
            og.reset()
            m.reset()
        og.set_action_masks(action_masks(sample_actions(U.POLICY_SEED, t, N * A)))
        og.step_norender()
        d = og.get_dones()
        o = np.zeros(N * A, np.float32)
        for e in np.flatnonzero(d).tolist():
            for a in range(A):
                o[e * A + a] = og.true_objective(e, a)
        m.feed(og.get_last_rewards()[None], d[None], o[None])
    og.close()
    return m


def test_reset_zeroes_accumulators_and_end_tick_and_keeps_the_records(hip):
    name, reset_at = "tower_short", 203
    ticks = U.ROLLOUTS[name][4]
    want = oracle_with_reset(name, reset_at)
    records = want.drain()
    before = int((np.diff(records["end_tick"].astype(np.int64)) < 0).argmax()) + 1   # where end_tick starts again
    assert before >= 700 and len(records) - before >= 700 and records["end_tick"][before] < 16
    g = make_gym(hip, name)
    for t in range(ticks):
        if t == reset_at:
            g.reset()
            assert g.ticks_since_reset() == 0
            assert not g.episode_returns_tensor().cpu().numpy().any() and not g.episode_lengths_tensor().cpu().numpy().any()
            assert g.episode_log_count()[0] == before   # the records stay
        g.sample_random_actions(U.POLICY_SEED, t)
        g.step()
    check_final(g, want, records, g.drain_episode_log())
    g.close()


def test_log_switched_off_and_on_again(hip):
    name = "collect_short"
    scenario, N, A, params, ticks, *_ = U.ROLLOUTS[name]
    rewards, dones, tobj = U.rollout(name)
    m = U.Model(N, A)
    g = make_gym(hip, name)

    def run(t0, t1):
        for t in range(t0, t1):
            g.sample_random_actions(U.POLICY_SEED, t)
            g.step()
        m.feed(rewards[t0:t1], dones[t0:t1], tobj[t0:t1])

    run(0, 150)
    first = m.drain()
    assert len(first) >= 250
    assert g.drain_episode_log().tobytes() == first.tobytes()
    g.set_episode_log(0)
    assert g.episode_log_capacity() == 0 and g.episode_returns_device_ptr() == 0
    with pytest.raises(RuntimeError, match="episode log is off"):
        g.drain_episode_log(4)
    run(150, 200)
    g.set_episode_log(CAP)   # episodes already running are counted from this tick; end_tick still counts from the reset
    m.restart()
    run(200, ticks)
    second = m.drain()
    assert len(second) >= 250 and second["end_tick"].min() >= 200   # (the oracle alone gives 290)
    check_final(g, m, second, g.drain_episode_log())
    g.close()


def test_argument_errors_on_a_gym(hip):
    g = make_gym(hip, "boxagone", capacity=0)
    with pytest.raises(RuntimeError, match="capacity >= 0"):
        g.set_episode_log(-1)
    with pytest.raises(RuntimeError, match="episode log is off"):
        g.episode_log_count()
    with pytest.raises(RuntimeError, match="episode log is off"):
        g.flush_episode_log()
    before = g.arena_bytes()
    g.set_episode_log(1000)
    assert g.arena_bytes() >= before + 1000 * 24 + g.num_envs * 12
    g.set_episode_log(0)
    assert g.arena_bytes() == before
    g.close()


def test_wrapper_step_device_reports_what_step_batched_reports(hip):
    """against the parent's own path: Wrapper.step_batched per tick (host bookkeeping) and Wrapper.step_device + drain_episode_stats on two equal gyms give
    the same z_* values as Python floats"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    from megaverse_amd.rl import Wrapper
    N, A, ticks, params = 8, 2, 400, {"episodeLengthSec": -200.0}
    envs = [MegaverseEnv("TowerBuilding", N, A, params=params, img_w=U.W, img_h=U.H, episode_log=cap) for cap in (0, 4096)]
    host, dev = Wrapper(envs[0]), Wrapper(envs[1])
    for w in (host, dev):
        w.seed(U.ENV_SEED)
        w.reset()
    from_host, from_device = [], []
    for t in range(ticks):
        acts = sample_actions(U.POLICY_SEED, t, N * A)
        _, _, dones, _, infos = host.step_batched(acts)
        for i in np.flatnonzero(dones).tolist():
            s = infos[i]["episode_extra_stats"]
            from_host.append((t, i, s["z_towerbuilding_reward"], s["z_towerbuilding_true_objective"], infos[i]["true_objective"]))
        obs, rew, term, trunc, _ = dev.step_device(torch.as_tensor(acts, device="cuda"))
        assert obs.is_cuda and rew.is_cuda and term.is_cuda and trunc.is_cuda and term.shape == (N * A,)
        if (t + 1) % 25 == 0:
            for d in dev.drain_episode_stats():
                assert set(d) == {"true_objective", "episode_extra_stats", "agent", "length", "end_tick"}
                s = d["episode_extra_stats"]
                assert set(s) == {"z_towerbuilding_true_objective", "z_towerbuilding_reward", "z_approx_total_training_steps"}
                from_device.append((d["end_tick"], d["agent"], s["z_towerbuilding_reward"], s["z_towerbuilding_true_objective"], d["true_objective"]))
    # (the oracle-checked TowerBuilding rollout of the same parameters logs 1860 records in 400 ticks of 128 agents: 230 for 16 agents; less than half would be odd)
    assert len(from_host) >= 100
    assert from_device == from_host
    assert all(type(v) is float for row in from_device for v in row[2:])
    host.close()
    dev.close()


@pytest.mark.parametrize("mode", ["pipelined", "not_pipelined", "device_actions", "step_n_ring"])
def test_nothing_else_changes_with_the_log_on(hip, mode):
    """state snapshots, rewards, dones, true objectives and exact-mode pixels of a 64-tick TowerBuilding rollout equal those of a gym with the log off"""
    import torch
    N, A, ticks = 8, 2, 64
    gyms = []
    for cap in (0, 4096):
        g = hip.MegaverseGym("TowerBuilding", 128, 72, N, A, 1, False, {"episodeLengthSec": -200.0})
        g.set_pixel_mode("exact")
        g.set_pipelining(mode != "not_pipelined")
        g.seed(U.ENV_SEED)
        if cap:
            g.set_episode_log(cap)
        g.reset()
        gyms.append(g)
    finished = 0

    def compare(t):
        nonlocal finished
        off, on = gyms
        assert off.get_rewards_array().tobytes() == on.get_rewards_array().tobytes(), t
        assert off.get_dones().tobytes() == on.get_dones().tobytes(), t
        assert off.get_true_objectives().tobytes() == on.get_true_objectives().tobytes(), t
        finished += int(off.get_dones().sum())
        for e in range(N):
            assert hip_snapshot(off, e).tobytes() == hip_snapshot(on, e).tobytes(), (t, e)
            for a in range(A):
                assert np.array_equal(off.get_observation(e, a), on.get_observation(e, a)), (t, e, a)

    if mode == "step_n_ring":
        keep = [rings(g, 8) for g in gyms]
        for t0 in range(0, ticks, 8):
            for g in gyms:
                g.step_n(8, "multidiscrete", U.POLICY_SEED, t0)
            for j in range(8):
                assert keep[0][1][j].cpu().numpy().tobytes() == keep[1][1][j].cpu().numpy().tobytes()
                assert keep[0][2][j].cpu().numpy().tobytes() == keep[1][2][j].cpu().numpy().tobytes()
                assert torch.equal(keep[0][0][j], keep[1][0][j])
            compare(t0 + 7)
    else:
        for t in range(ticks):
            acts = sample_actions(U.POLICY_SEED, t, N * A)
            held = torch.as_tensor(acts, device="cuda")
            for g in gyms:
                if mode == "device_actions":
                    g.set_actions_device(held.data_ptr())
                else:
                    g.set_actions_batched(acts)
                g.step()
            compare(t)
    assert finished >= 1   # (an episode did end inside the comparison)
    assert gyms[1].episode_log_count()[0] >= A
    for g in gyms:
        g.close()
