"""Level seeds on the GPU (include/megaverse_hip.h: mv_seed_envs): chosen envs restart their episode stream from a seed.

Every test uses 8 envs, 32 x 32 frames and exact pixels unless it says otherwise (tests/seed_envs_util.py).  Expected values come from twin gyms that reach
the same streams through mv_seed, and from the CPU oracle: an env given Env::seed(s) plays what env p of an oracle gym plays whose master seed hands env p
the value s (megaverse_amd.distributed.env_seeds).  No env, tick or byte is left out of a comparison.

Short episodes.  An auto-reset has to fall inside a rollout of a few dozen ticks, so the gyms get a small episodeLengthSec: 0.8 s (12 ticks) where the
scenario's episodes last exactly that; a negative one where the scenario adds its own time per object (TowerBuilding, Collect, HexMemory: every env then
finishes EVERY tick, an auto-reset per tick and a chain of two dozen episodes per env; no agent scores in a one-tick episode, so the true objectives stay
the zeros a fresh oracle has).  ObstaclesEasy cannot be short -- its episodes last at least 35 s per platform, 900 to 1155 ticks for these seeds.  Test 1
steps its three twin gyms through 1150 ticks, past the auto-reset of every env (a few seconds).  Test 2 would need the CPU oracle to step and draw as many
ticks (7 s and more on its own), so there ObstaclesEasy crosses a masked reset of every env (mv_reset_envs: "the next reset" in its other form) where the
other families cross auto-resets; its auto-resets into a new stream are test 1's to pin."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import episode_log_util as U
import oracle_lib
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.distributed import env_seeds
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions
from seed_envs_util import H, MASK, MASKS, N, PERM, S1, S2, W, mask_of, seed_words
from test_reset_envs_gpu import ORACLE_CASES, capture, check_env

pytestmark = pytest.mark.gpu

POLICY_SEED = 1234
T0 = 7
# case -> (params, ticks behind the call, the tick behind the call at which every gym resets every env with mv_reset_envs, or None)
SHORT = {"tower_a1": ({"episodeLengthSec": -330.0}, 14, None), "tower_a2": ({"episodeLengthSec": -330.0}, 14, None),
         "obstacles_easy": ({}, 14, 5), "collect": ({"episodeLengthSec": -250.0}, 14, None), "rearrange": ({"episodeLengthSec": 0.8}, 20, None),
         "sokoban": ({"episodeLengthSec": 0.8}, 20, None), "hex_memory": ({"episodeLengthSec": -200.0}, 14, None),
         "boxagone": ({"episodeLengthSec": 0.8}, 20, None), "empty": ({"episodeLengthSec": 0.8}, 20, None),
         "football": ({"episodeLengthSec": 0.8}, 20, None)}
# test 1: ObstaclesEasy runs until every env's first episode (S1's) has ended by itself -- the last one at tick 1140 (measured on the CPU oracle; asserted)
LONG = {"obstacles_easy": 1150}
ALL = np.ones(N, np.bool_)


def make_gym(scenario, A, params=None, seed=S1, mode="exact", log=0, n=N):
    U.boxoban_env()
    g = MegaverseGym(scenario, W, H, n, A, 1, False, params or {})
    g.set_pixel_mode(mode)
    g.seed(seed)
    if log:
        g.set_episode_log(log)
    g.reset()
    return g


def rows(t, A, n=N):
    return sample_actions(POLICY_SEED, t, n * A)


def act(g, A, t, perm=None, n=N):
    a = np.asarray(rows(t, A, n)).reshape(n, A, 6)
    g.set_actions_batched(a if perm is None else a[list(perm)])


def step(g):
    """one tick; a warning (return 1: a starved env, a capacity flag) fails the test"""
    assert g._lib.mv_step(g._g) == 0, g._lib.mv_last_error()


def raw(g, e):
    return g.debug_snapshot_bytes(e).tobytes()


def all_raw(g, n=N):
    return [raw(g, e) for e in range(n)]


def frames(g, A, e):
    return b"".join(g.get_observation(e, a).tobytes() for a in range(A))


def outputs(g, A, e):
    s = slice(e * A, (e + 1) * A)
    return g.get_rewards_array()[s].tobytes() + g.get_dones()[e:e + 1].tobytes() + g.get_true_objectives()[s].tobytes()


def everything(g, A, e):
    return raw(g, e), outputs(g, A, e), frames(g, A, e)


def device_seeds(words):
    """the seed words as a torch.int32 CUDA tensor, written by a kernel on the gym's stream (torch's current one: the null stream)"""
    import torch
    src = torch.as_tensor(np.asarray(words, np.int32)).to("cuda:0")
    out = torch.full((len(words),), -1, dtype=torch.int32, device="cuda:0")   # (would seed nobody, were it read before the kernel below has run)
    torch.cuda.synchronize()
    torch.add(src, 0, out=out)
    return out


# ---- 1. against mv_seed, every scenario family ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_name", sorted(MASKS))
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_against_mv_seed(hip, case, mask_name):
    """1. three gyms share seed S1 and an action script.  At tick 7 G calls seed_envs (host form) with env_seeds(S2, 8)[e] for the flagged envs, twin T calls
    mv_seed(S2), twin U does nothing.  Right behind the call every env of G is byte-equal to U -- snapshot, outputs, frames: the running episodes go on.
    Then, on every tick of a rollout that crosses an auto-reset of every env, a
    flagged env of G equals T's env and an unflagged one U's: state, reward bits, dones, true objectives, exact pixels."""
    scenario, A = ORACLE_CASES[case]
    params, ticks, reset_at = SHORT[case]
    if case in LONG:
        ticks, reset_at = LONG[case], None
    mask = MASKS[mask_name]
    G, T, Uu = (make_gym(scenario, A, params) for _ in range(3))
    gyms = (G, T, Uu)
    for t in range(T0):
        for g in gyms:
            act(g, A, t)
            step(g)
    G.seed_envs(seed_words(S2, mask))
    T.seed(S2)
    for e in range(N):
        assert everything(G, A, e) == everything(Uu, A, e), f"{case}: env {e} right behind the call"
    finished = np.zeros(N, int)
    split = False
    for j in range(ticks):
        if reset_at is not None and j == reset_at:
            for g in gyms:
                g.reset_envs(ALL)
            finished += 1
        else:
            for g in gyms:
                act(g, A, T0 + j)
                step(g)
            finished += Uu.get_dones() != 0
        for e in range(N):
            ref = T if mask[e] else Uu
            assert everything(G, A, e) == everything(ref, A, e), f"{case}, {mask_name}: env {e}, {j + 1} ticks behind the call"
        split = split or any(raw(T, e) != raw(Uu, e) for e in range(N))
    assert (finished >= 1).all(), f"the rollout crossed no reset of envs {np.flatnonzero(finished == 0).tolist()}"
    assert split, "mv_seed changed nothing inside the rollout: the test would prove nothing"
    for g in gyms:
        g.close()


# ---- 2. against the oracle, permuted and duplicated ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fresh_oracle(scenario, A, params_items, seed, ticks, reset_at=None):
    """a fresh oracle gym -- seed(seed), reset() -- and `ticks` ticks on action rows T0, T0 + 1, ...: [capture behind the reset, then behind every tick];
    computed once and shared"""
    U.boxoban_env()
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1, False, dict(params_items))
    og.seed(seed)
    og.reset()
    out = [capture(og, scenario, A)]
    for j in range(ticks):
        if reset_at is not None and j == reset_at:
            og.reset()
        else:
            og.set_action_masks(action_masks(rows(T0 + j, A)))
            og.step()
        out.append(capture(og, scenario, A))
    og.close()
    return out


def permuted(ref, A, perm):
    """an oracle capture with env d holding what env perm[d] held"""
    p = list(perm)
    pa = [q * A + a for q in p for a in range(A)]
    out = {"snap": [ref["snap"][q] for q in p], "rewards": ref["rewards"][pa], "dones": ref["dones"][p], "tobj": ref["tobj"][pa], "frames": ref["frames"][pa]}
    for k in ("bag", "ball"):
        if k in ref:
            out[k] = [ref[k][q] for q in p]
    return out


ORACLE2 = {k: v for k, v in ORACLE_CASES.items() if k != "sokoban"}   # (Sokoban: a re-seeded env carries its level list, a fresh oracle env has none)
ORACLE2_IDS = sorted(ORACLE2) + ["collect_device_gen", "collect_host_gen"]


@pytest.mark.parametrize("case", ORACLE2_IDS)
def test_against_the_oracle_permuted(hip, case, monkeypatch):
    """2. seeds[d] = env_seeds(S2, 8)[p[d]] with p = [3, 3, 0, 5, 5, 5, 1, 7]; start_levels at tick 7.  From then on env d, fed the action rows of p[d],
    equals env p[d] of a fresh oracle (seed(S2), reset()) on every tick, across a reset of every env (check_env's comparison: state, reward bits, dones,
    true objectives, exact pixels); envs with the same seed are byte-equal to each other.  Collect with MV_COLLECT_DEVICE_GEN both ways."""
    from megaverse_amd.megaverse_env import MegaverseEnv
    if case.startswith("collect_"):
        monkeypatch.setenv("MV_COLLECT_DEVICE_GEN", "1" if case == "collect_device_gen" else "0")
        case = "collect"
    scenario, A = ORACLE2[case]
    params, ticks, reset_at = SHORT[case]
    ref = fresh_oracle(scenario, A, tuple(sorted(params.items())), S2, ticks, reset_at)
    U.boxoban_env()
    env = MegaverseEnv(scenario, N, A, 1, False, dict(params), img_w=W, img_h=H)
    g = env.env
    g.set_pixel_mode("exact")
    env.seed(S1)
    g.reset()
    for t in range(T0):
        act(g, A, t)
        step(g)
    s2 = env_seeds(S2, N)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        env.start_levels(range(N), [int(s2[p]) for p in PERM])
    finished = np.zeros(N, int)
    for j in range(ticks + 1):
        if j > 0:
            if reset_at is not None and j - 1 == reset_at:
                g.reset_envs(ALL)
                finished += 1
            else:
                act(g, A, T0 + j - 1, PERM)
                step(g)
                finished += g.get_dones() != 0
        want = permuted(ref[j], A, PERM)
        for d in range(N):
            check_env(g, want, scenario, A, d, f"{case}: env {d} as oracle env {PERM[d]}, {j} ticks behind start_levels")
        states = [everything(g, A, d) for d in range(N)]
        for d in range(N):
            assert states[d] == states[PERM.index(PERM[d])], f"{case}: envs with the same seed differ, {j} ticks behind start_levels"
    assert (finished >= 1).all(), f"the rollout crossed no reset of envs {np.flatnonzero(finished == 0).tolist()}"
    env.close()


# ---- 3. level replay -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["TowerBuilding", "ObstaclesEasy", "HexMemory"])
def test_level_replay(hip, scenario):
    """3. start_levels(all, s), 10 ticks, start_levels(all, s) again: snapshots and frames right behind the second call equal those behind the first, and
    differ from what the envs showed in between.
    Sokoban is left out on purpose: a Sokoban env's level comes off its carried level list, and the first start_levels itself takes one level off it, so
    the condition under which a replay would hold there -- the list not advanced in between -- is never met by two start_levels calls; what holds for
    Sokoban is test 1 (a re-seeded env is mv_seed's)."""
    from megaverse_amd.megaverse_env import MegaverseEnv
    A = 1
    env = MegaverseEnv(scenario, N, A, 1, False, None, img_w=W, img_h=H)
    g = env.env
    g.set_pixel_mode("exact")
    env.seed(S1)
    g.reset()
    for t in range(3):
        act(g, A, t)
        step(g)
    s = [int(v) for v in env_seeds(S2, N)]
    env.start_levels(range(N), s)
    first = [(raw(g, e), frames(g, A, e)) for e in range(N)]
    for t in range(3, 13):
        act(g, A, t)
        step(g)
    between = [(raw(g, e), frames(g, A, e)) for e in range(N)]
    env.start_levels(range(N), s)
    second = [(raw(g, e), frames(g, A, e)) for e in range(N)]
    assert second == first
    assert all(between[e][0] != first[e][0] for e in range(N))
    env.close()


def test_sokoban_second_start_plays_the_next_level_of_the_list(hip):
    """3, Sokoban: what holds in place of a replay.  start_levels(all, s), 10 ticks, start_levels(all, s) again: the second start plays the NEXT level of
    each env's carried list -- not the first start's -- and both starts and every tick in between equal a twin that reaches the same streams through
    mv_seed(S2) + mv_reset: snapshots, outputs, frames"""
    from megaverse_amd.megaverse_env import MegaverseEnv
    A = 1
    U.boxoban_env()
    env = MegaverseEnv("Sokoban", N, A, 1, False, None, img_w=W, img_h=H)
    g, tw = env.env, make_gym("Sokoban", A)
    g.set_pixel_mode("exact")
    env.seed(S1)
    g.reset()
    s = [int(v) for v in env_seeds(S2, N)]
    starts = []
    for r in range(2):
        env.start_levels(range(N), s)
        tw.seed(S2)
        tw.reset()
        starts.append([(raw(g, e), frames(g, A, e)) for e in range(N)])
        for t in range(10 if r == 0 else 3):
            assert [everything(g, A, e) for e in range(N)] == [everything(tw, A, e) for e in range(N)], f"start {r}, {t} ticks behind it"
            for x in (g, tw):
                act(x, A, 20 * r + t)
                step(x)
    assert all(starts[1][e][0] != starts[0][e][0] for e in range(N)), "the second start replayed the first start's level"
    env.close(); tw.close()


# ---- 4. the device form --------------------------------------------------------------------------------------------------------------------------------
def test_device_form_between_batched_calls(hip):
    """4. TowerBuilding: step_n(8), the seeds written by a torch kernel on the gym's stream, seed_envs(tensor), step_n(8) with nothing synchronising in
    between; then reset_envs of every env and four more ticks.  The twin synchronises on both sides and uses the host form at the same tick: final
    snapshots, slab and episodes_consumed are equal, and the reset changed the level of exactly... every env (all were reset), the flagged ones to their new
    stream's: a third twin that seeded nobody differs from the first in the flagged envs alone."""
    import torch
    A, K = 1, 8
    words = seed_words(S2, MASK)
    out = []
    for form in ("device", "host", "none"):
        g = make_gym("TowerBuilding", A, mode="fast")
        src = torch.as_tensor(words).to("cuda:0")
        dev = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        g.step_n(K, "multidiscrete", POLICY_SEED, 0)
        if form == "device":
            torch.add(src, 0, out=dev)
            g.seed_envs(dev)
        elif form == "host":
            g.synchronize()
            g.seed_envs(words)
            g.synchronize()
        g.step_n(K, "multidiscrete", POLICY_SEED, K)
        g.reset_envs(ALL)
        g.step_n(4, "multidiscrete", POLICY_SEED, 2 * K)
        g.synchronize()
        out.append((all_raw(g), [frames(g, A, e) for e in range(N)], g.debug_episodes_consumed().tolist()))
        g.close()
        del dev, src
    d, h, u = out
    assert d == h
    assert [d[0][e] != u[0][e] for e in range(N)] == MASK.tolist()


def test_device_form_300_envs(hip):
    """4. 300 envs: the seed kernel's second block (256 lanes per block).  Flagged: envs 0, 255, 256, 299.  Device form against a host-form twin and an
    untouched twin: behind reset_envs of every env all three agree on the unflagged envs and the two forms on the flagged ones, which differ from the
    untouched twin's; envs 255 and 256 were given the same seed and are equal"""
    A, n = 1, 300
    words = np.full(n, -1, np.int32)
    words[[0, 255, 256, 299]] = [11, 4242, 4242, 2 ** 31 - 1]
    snaps = []
    for form in ("device", "host", "none"):
        g = make_gym("TowerBuilding", A, mode="fast", n=n)
        for t in range(2):
            act(g, A, t, n=n)
            step(g)
        keep = device_seeds(words) if form == "device" else None
        if form != "none":
            g.seed_envs(keep if form == "device" else words)
        g.reset_envs(np.ones(n, np.bool_))
        if form == "device":
            assert raw(g, 255) == raw(g, 256) != raw(g, 0)   # (in front of the step: the two envs get different actions)
        act(g, A, 2, n=n)
        step(g)
        snaps.append(all_raw(g, n))
        g.close()
        del keep
    d, h, u = snaps
    assert d == h
    assert [e for e in range(n) if d[e] != u[e]] == [0, 255, 256, 299]


def test_device_form_is_refused_on_a_host_fed_gym(hip):
    """4. ObstaclesEasy: the device form returns -1, the text names mv_seed_envs_host and says where the generators live; no byte of any env changes and
    the next steps equal an untouched twin's"""
    A = 1
    g, tw = make_gym("ObstaclesEasy", A), make_gym("ObstaclesEasy", A)
    for t in range(T0):
        for x in (g, tw):
            act(x, A, t)
            step(x)
    before = [everything(g, A, e) for e in range(N)]
    consumed = g.debug_episodes_consumed().tolist()
    keep = device_seeds(seed_words(S2, ALL))
    assert g._lib.mv_seed_envs(g._g, C.c_void_p(keep.data_ptr())) == -1
    text = g._lib.mv_last_error().decode()
    assert "mv_seed_envs_host" in text and "generators live on the host" in text
    with pytest.raises(RuntimeError, match="mv_seed_envs_host"):
        g.seed_envs(keep)
    assert [everything(g, A, e) for e in range(N)] == before and g.debug_episodes_consumed().tolist() == consumed
    g.reset_envs(ALL)
    tw.reset_envs(ALL)
    for t in range(T0, T0 + 5):
        for x in (g, tw):
            act(x, A, t)
            step(x)
        assert [everything(g, A, e) for e in range(N)] == [everything(tw, A, e) for e in range(N)]
    g.close(); tw.close()
    del keep


# ---- 5. never starves ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset_form", ["host", "device"])
@pytest.mark.parametrize("case", ["obstacles_easy", "hex_memory"])
def test_seed_reset_pairs_never_starve(hip, case, reset_form):
    """5. six seed_envs_host + reset_envs pairs back to back with no stepping call, the reset in the host form or in the device form; every call returns 0
    (no warning).  The level is the last seed's: every env equals a fresh oracle's (seed(S2), reset()).  Then 40 ticks (HexMemory: an auto-reset of every
    env on every tick) raise no warning either, and the envs stay the oracle's."""
    import torch
    scenario, A = ORACLE_CASES[case]
    params, _, _ = SHORT[case]
    ticks = 40
    ref = fresh_oracle(scenario, A, tuple(sorted(params.items())), S2, ticks)
    g = make_gym(scenario, A, params)
    lib = g._lib
    ones = np.ones(N, np.uint8)
    dev_ones = torch.ones(N, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for k in range(6):
        words = seed_words(S2 if k == 5 else 100 + k, ALL)
        assert lib.mv_seed_envs_host(g._g, words.ctypes.data) == 0, lib.mv_last_error()
        if reset_form == "host":
            assert lib.mv_reset_envs_host(g._g, ones.ctypes.data, 1) == 0, lib.mv_last_error()
        else:
            assert lib.mv_reset_envs(g._g, C.c_void_p(dev_ones.data_ptr()), 1) == 0, lib.mv_last_error()
    assert g.debug_episodes_consumed().tolist() == [7] * N
    for j in range(ticks + 1):
        if j > 0:
            act(g, A, T0 + j - 1)
            step(g)
        for e in range(N):
            check_env(g, ref[j], scenario, A, e, f"{case}, {reset_form} resets: env {e}, {j} ticks behind the last pair")
    g.close()
    del dev_ones


# ---- 6. identity and neighbours ------------------------------------------------------------------------------------------------------------------------
def test_a_fork_destination_plays_its_own_new_stream(hip):
    """6. Rearrange, episodes of 12 ticks.  seed_envs(env 1), then env 1 forks from env 0: env 1 is env 0's episode; at its end (tick 11, both envs') env 1
    plays ITS new stream's first episode -- it is env 1 of a twin that was re-seeded alike and forked nothing -- and not env 0's next one"""
    A, params = 1, {"episodeLengthSec": 0.8}
    fg, tw = make_gym("Rearrange", A, params), make_gym("Rearrange", A, params)
    for t in range(T0):
        for g in (fg, tw):
            act(g, A, t)
            step(g)
    for g in (fg, tw):
        g.seed_envs({1: 987654})
    fg.fork_envs([-1, 0] + [-1] * (N - 2))
    assert raw(fg, 1) == raw(fg, 0) != raw(tw, 1)
    done_at = None
    for t in range(T0, T0 + 8):
        for g in (fg, tw):
            act(g, A, t)
            step(g)
        if fg.get_dones()[1]:
            done_at = t
            assert tw.get_dones()[1]
            break
        assert raw(fg, 1) != raw(tw, 1)
    assert done_at is not None, "env 1 did not finish inside the window"
    assert raw(fg, 1) == raw(tw, 1) and frames(fg, A, 1) == frames(tw, A, 1)
    assert raw(fg, 1) != raw(fg, 0)
    assert fg.debug_episodes_consumed().tolist() == tw.debug_episodes_consumed().tolist()
    fg.close(); tw.close()


def test_the_episode_log_is_untouched(hip):
    """6. BoxAGone with the episode log on: seed_envs changes neither the running returns and lengths nor the records"""
    A = 1
    g = make_gym("BoxAGone", A, log=256)
    for t in range(T0 + 5):
        g.sample_random_actions(POLICY_SEED, t)
        step(g)
    ret, length, count = g.episode_returns_tensor().cpu().numpy().copy(), g.episode_lengths_tensor().cpu().numpy().copy(), g.episode_log_count()
    assert length.tolist() == [T0 + 5] * N
    g.seed_envs(seed_words(S2, MASK))
    assert g.episode_returns_tensor().cpu().numpy().tobytes() == ret.tobytes() and g.episode_lengths_tensor().cpu().numpy().tobytes() == length.tobytes()
    assert g.episode_log_count() == count
    g.close()


def test_same_level_same_script_same_records(hip):
    """6. Rearrange, budget 1: start_levels(all, one seed), then run_episodes under one action script that gives every env the same actions: the eight
    drained records are identical but for the agent they name"""
    from action_ring_util import make_script
    from megaverse_amd.megaverse_env import MegaverseEnv
    A = 1
    env = MegaverseEnv("Rearrange", N, A, 1, False, {"episodeLengthSec": 2.0}, img_w=W, img_h=H)
    env.seed(S1)
    env.reset()
    env.start_levels(range(N), 31337)
    script = np.repeat(make_script(24, 32, A)[:, None], N, axis=1).reshape(32, N * A, 6)
    rec = env.run_episodes(1, policy="sequence", actions=script, max_ticks=64)
    assert len(rec) == N and sorted(rec["agent"].tolist()) == list(range(N))
    for name in ("length", "end_tick", "true_objective", "ret"):
        assert len(set(rec[name].tobytes()[i * rec[name].itemsize:(i + 1) * rec[name].itemsize] for i in range(N))) == 1, name
    assert rec["length"][0] == 30
    states = all_raw(env.env)
    assert len(set(states)) == 1
    env.close()


def test_state_observations_and_draw_masks_need_nothing(hip):
    """6. TowerBuilding with state observations and a draw mask attached (env 2 is not drawn): start_levels of envs {0, 3, 7} with render refreshes the
    flagged envs' state rows and frames, every other row and frame keeps its bytes -- env 2's frame too -- and the attachments stay"""
    import torch
    from megaverse_amd.megaverse_env import MegaverseEnv
    A = 1
    env = MegaverseEnv("TowerBuilding", N, A, 1, False, None, img_w=W, img_h=H)
    g = env.env
    g.set_pixel_mode("exact")
    env.seed(S1)
    g.reset()
    buf = torch.zeros((1, N * A, 16), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    g.set_state_obs(buf)
    draw = np.ones(N, np.bool_)
    draw[2] = False
    g.set_draw_mask(draw)
    for t in range(T0):
        act(g, A, t)
        step(g)
    g.synchronize()
    rows_before, frames_before = buf.cpu().numpy().copy(), [frames(g, A, e) for e in range(N)]
    flagged = [0, 3, N - 1]
    env.start_levels(flagged, [int(env_seeds(S2, N)[e]) for e in flagged])
    g.synchronize()
    rows_after, frames_after = buf.cpu().numpy(), [frames(g, A, e) for e in range(N)]
    assert [rows_after[0, e].tobytes() != rows_before[0, e].tobytes() for e in range(N)] == MASK.tolist()
    assert [frames_after[e] != frames_before[e] for e in range(N)] == MASK.tolist()
    assert g.draw_mask() == "host"
    act(g, A, T0)
    step(g)
    g.synchronize()
    assert frames(g, A, 2) == frames_before[2]
    env.close()
    del buf


def test_multitask_seed_envs(hip):
    """members of a group are served (mv_reset_envs' rule): MultiTaskGym (TowerBuilding + ObstaclesEasy), seed_envs in the batch's numbering, then
    reset_envs of the same envs: the flagged envs are those of a twin that called seed(S2) and reset(), the others those of an untouched twin"""
    import torch
    from megaverse_amd.multitask import MultiTaskGym
    mask = mask_of([0, 3, 5])   # tasks 0, 1, 1: local envs 0 / 1, 2
    gyms = []
    for _ in range(3):
        m = MultiTaskGym(["TowerBuilding", "ObstaclesEasy"], W, H, N, 1, 1)
        m.set_pixel_mode("fast")
        m.attach(torch.device("cuda:0"))
        m.seed(S1)
        m.reset()
        m.step_n(4, "multidiscrete", POLICY_SEED, 0)
        gyms.append(m)
    gM, gR, gU = gyms
    words = seed_words(S2, mask)   # (the members share the job's master stream: seed(S2) hands global env i the i-th value)
    gM.seed_envs(words)
    gM.reset_envs(mask)
    gR.seed(S2)
    gR.reset()

    def states(m):
        return [raw(*m.locate(i)) for i in range(N)]

    for k in range(2):
        if k:
            for m in gyms:
                m.step_n(4, "multidiscrete", POLICY_SEED, 4)
        sM, sR, sU = states(gM), states(gR), states(gU)
        assert [sM[i] == (sR[i] if mask[i] else sU[i]) for i in range(N)] == [True] * N, "behind the reset" if k == 0 else "a call later"
        assert [sM[i] != sU[i] for i in range(N)] == mask.tolist()
    with pytest.raises(ValueError, match="seed_envs"):
        gM.seed_envs(np.zeros(N - 1, np.int32))
    # a tensor takes the device form, which the ObstaclesEasy member refuses: refused before the TowerBuilding member in front of it is touched
    before = states(gM)
    keep = device_seeds(seed_words(S1 + 1, ALL))
    with pytest.raises(RuntimeError, match="mv_seed_envs_host"):
        gM.seed_envs(keep)
    gM.reset_envs(ALL)
    gR.reset_envs(ALL)   # (gM's streams are still gR's in the flagged envs and gU's in the others: nobody was re-seeded)
    gU.reset_envs(ALL)
    sM, sR, sU = states(gM), states(gR), states(gU)
    assert [sM[i] == (sR[i] if mask[i] else sU[i]) for i in range(N)] == [True] * N and sM != before
    for m in gyms:
        m.close()
    del keep


def test_multitask_device_seeds_are_released(hip):
    """a MultiTaskGym of TowerBuilding members takes a tensor (per-member copies, the device form); the copies are held until the next stepping call has been
    enqueued and no longer: every stepping path of the batch lets go of them.  The re-seeded envs are those of a twin given the same words as numpy."""
    import torch
    from megaverse_amd.multitask import MultiTaskGym
    words = seed_words(S2, MASK)
    pair = []
    for form in ("device", "host"):
        m = MultiTaskGym(["TowerBuilding", "TowerBuilding"], W, H, N, 1, 1)
        m.set_pixel_mode("fast")
        m.attach(torch.device("cuda:0"))
        m.seed(S1)
        m.reset()
        m.step_n(2, "multidiscrete", POLICY_SEED, 0)
        keep = device_seeds(words) if form == "device" else None
        for _ in range(3):
            m.seed_envs(keep if form == "device" else words)
        if form == "device":
            assert [len(g._seed_held) for g in m.gyms] == [3, 3]
        m.reset_envs(ALL)
        m.step_n(2, "multidiscrete", POLICY_SEED, 2)
        assert [len(g._seed_held) for g in m.gyms] == [0, 0]
        if form == "device":
            m.seed_envs(keep)
            m.sample_random_actions(POLICY_SEED, 4)
            m.step()
            assert [len(g._seed_held) for g in m.gyms] == [0, 0]
        else:
            m.seed_envs(words)
            m.sample_random_actions(POLICY_SEED, 4)
            m.step()
        m.synchronize()
        pair.append([raw(*m.locate(i)) for i in range(N)])
        m.close()
        del keep
    assert pair[0] == pair[1]


# ---- 7. invalid input ----------------------------------------------------------------------------------------------------------------------------------
def test_errors(hip):
    """7. a null pointer, a wrong-shaped tensor or array, a closed gym: -1 with text or ValueError, nothing changes.  Before the first mv_reset the call is
    valid and acts as mv_seed for the chosen envs."""
    import torch
    A = 1
    g = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
    tw = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
    for x in (g, tw):
        x.set_pixel_mode("exact")
    lib = g._lib
    g.seed_envs(seed_words(S2, ALL))   # (before the first reset)
    tw.seed(S2)
    g.reset(); tw.reset()
    assert all_raw(g) == all_raw(tw)
    act(g, A, 0); step(g)
    before, consumed = [everything(g, A, e) for e in range(N)], g.debug_episodes_consumed().tolist()
    for fn in (lib.mv_seed_envs_host, lib.mv_seed_envs):
        assert fn(g._g, None) == -1 and b"null seeds" in lib.mv_last_error()
    for bad in (np.zeros(N + 1, np.int32), np.zeros(N, np.float32), torch.zeros(N + 1, dtype=torch.int32, device="cuda:0"),
                torch.zeros(N, dtype=torch.int64, device="cuda:0"), torch.zeros(N, dtype=torch.int32)):
        with pytest.raises(ValueError, match="seed_envs"):
            g.seed_envs(bad)
    assert [everything(g, A, e) for e in range(N)] == before and g.debug_episodes_consumed().tolist() == consumed
    handle = g._g
    words = seed_words(S2, ALL)
    lib.mv_close(handle)
    for fn in (lib.mv_seed_envs_host, lib.mv_seed_envs):
        assert fn(handle, words.ctypes.data) == -1 and b"closed" in lib.mv_last_error()
    g.close(); tw.close()
    # ... and on a host-fed gym: seed_envs before the first reset, then reset, is seed + reset
    g, tw = (MegaverseGym("ObstaclesEasy", W, H, N, A, 1, False, {}) for _ in range(2))
    for x in (g, tw):
        x.set_pixel_mode("exact")
    g.seed_envs(seed_words(S2, ALL))
    tw.seed(S2)
    g.reset(); tw.reset()
    assert [everything(g, A, e) for e in range(N)] == [everything(tw, A, e) for e in range(N)]
    g.close(); tw.close()
