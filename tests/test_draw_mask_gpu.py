"""Draw masks on the GPU (include/megaverse_hip.h: mv_set_draw_mask): the frames of the envs a mask leaves out are neither set up nor drawn, and no byte of
their rows is written.

Every test runs two gyms with the same seed: one with a draw mask, one twin without.  Before every call the masked gym's slab and ring are filled with a
sentinel byte (0xA5) by torch on the gym's stream.  Behind the call every byte of an undrawn env's rows must be the sentinel, every byte of a drawn env's rows
must equal the twin's, and rewards, dones, true objectives and the debug snapshot of EVERY env must equal the twin's bit for bit.  In exact pixel mode the drawn
rows also equal the CPU oracle's render.  Comparisons are equality of bytes; no env, tick or byte is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # (the child process of test_histogram_walk_in_a_child_process)
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import episode_log_util as U
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.rollout import action_masks, sample_actions

pytestmark = pytest.mark.gpu

ENV_SEED, POLICY_SEED = 42, 1234
SENT = 0xA5
DEV = "cuda:0"


class Rig:
    """one gym and the torch buffers its observations (slab, ring), rewards and dones go to"""

    def __init__(self, scenario, A=1, n=12, w=64, h=64, mode="fast", ring=0, layout="rgba", params=None, log=0, pipelining=True, overlap=False, reset=True):
        import torch
        U.boxoban_env()
        self.scenario, self.A, self.n, self.R, self.ticks = scenario, A, n, ring, 0
        self.g = g = MegaverseGym(scenario, w, h, n, A, 1, False, dict(params or {}))
        g.set_pixel_mode(mode)
        if layout == "chw":
            g.set_obs_layout("chw")
        if not pipelining:
            g.set_pipelining(False)
        g.seed(ENV_SEED)
        if log:
            g.set_episode_log(log)
        fs = (3, h, w) if layout == "chw" else (h, w, 4)
        self.slab = torch.full((n * A,) + fs, SENT, dtype=torch.uint8, device=DEV)
        self.obs = torch.full((ring, n * A) + fs, SENT, dtype=torch.uint8, device=DEV) if ring else None
        self.rew = torch.full((ring, n * A), -7.0, dtype=torch.float32, device=DEV) if ring else None
        self.done = torch.full((ring, n), 9, dtype=torch.uint8, device=DEV) if ring else None
        torch.cuda.synchronize()
        g.set_obs_buffer(self.slab.data_ptr())
        self.overlap = overlap
        if reset:
            self.reset()

    def reset(self):
        self.g.reset()
        if self.R:   # (attached behind the reset: tick t of the calls that follow goes to entry t % R)
            self.g.set_output_ring(self.R, self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr())
        if self.overlap:
            self.g.set_pass_overlap(True)

    def fill(self, wait=False):
        """the sentinel into every observation byte, by torch on the gym's stream (the null stream); wait: the host waits for it (overlapped passes run on
        streams of the gym's own, ordered behind what the caller had enqueued a call earlier)"""
        import torch
        self.slab.fill_(SENT)
        if self.obs is not None:
            self.obs.fill_(SENT)
        if wait:
            torch.cuda.synchronize()

    def sync(self):
        import torch
        self.g.synchronize()
        torch.cuda.synchronize()

    def step(self, act=None):
        """one mv_step on random actions of the tick's index (act: the actions themselves); 0 or a warning, never an error"""
        if act is None:
            self.g.sample_random_actions(POLICY_SEED, self.ticks)
        else:
            self.g.set_actions_batched(act)
        assert self.g._lib.mv_step(self.g._g) >= 0, self.g._lib.mv_last_error()
        self.ticks += 1

    def step_n(self, k, render="every"):
        """-> the ring entries of the call's ticks, the launches it took"""
        c0 = self.g.debug_launch_counts()
        self.g.step_n(k, "multidiscrete", POLICY_SEED, self.ticks, render=render)
        c1 = self.g.debug_launch_counts()
        entries = [(self.ticks + j) % self.R for j in range(k)] if self.R else []
        self.ticks += k
        return entries, (c1[0] - c0[0], c1[1] - c0[1])

    def close(self):
        self.sync()
        self.g.close()


def pair(*args, **kw):
    return Rig(*args, **kw), Rig(*args, **kw)


def check_rows(got, ref, drawn, A, what):
    """one slab or ring entry [n * A, ...]: the rows of undrawn envs hold the sentinel in every byte, the rows of drawn envs the twin's bytes"""
    per = np.repeat(np.asarray(drawn, bool), A)
    assert got.shape == ref.shape and per.shape == (got.shape[0],)
    bad = [int(r) for r in np.nonzero(~per)[0] if not (got[r] == SENT).all()]
    assert not bad, f"{what}: rows {bad} of undrawn envs were written"
    bad = [int(r) for r in np.nonzero(per)[0] if got[r].tobytes() != ref[r].tobytes()]
    assert not bad, f"{what}: rows {bad} of drawn envs differ from the twin's"
    assert all((ref[r] != SENT).any() for r in np.nonzero(per)[0]), f"{what}: the twin drew nothing: the comparison would prove nothing"


def same_outputs(m, t, what):
    """rewards, dones, true objectives and the snapshot of every env: the twin's, bit for bit"""
    for name in ("get_rewards_array", "get_dones", "get_true_objectives"):
        assert getattr(m.g, name)().tobytes() == getattr(t.g, name)().tobytes(), f"{what}: {name}"
    bad = [e for e in range(m.n) if m.g.debug_snapshot_bytes(e).tobytes() != t.g.debug_snapshot_bytes(e).tobytes()]
    assert not bad, f"{what}: state of envs {bad}"


def step_and_check(m, t, drawn, what, act=None):
    """one tick of mv_step into the slabs"""
    m.fill()
    m.step(act); t.step(act)
    m.sync(); t.sync()
    check_rows(m.slab.cpu().numpy(), t.slab.cpu().numpy(), drawn, m.A, what)
    same_outputs(m, t, what)


def call_and_check(m, t, drawn, k, what, render="every", fill=True, check=True):
    """one batched call into the rings: every entry of the masked gym's ring -- the call's drawn ticks by rows, all the others sentinel --, the whole reward
    and done rings, the slab (no byte written), the launches"""
    if fill:
        m.fill(wait=m.overlap)
    (entries, lm), (_, lt) = m.step_n(k, render), t.step_n(k, render)
    assert lm == lt, f"{what}: {lm} launches with a draw mask, {lt} without"
    if not check:
        return entries
    check_ring(m, t, drawn, {"every": entries, "last": entries[-1:], "none": []}[render], what)
    return entries


def check_ring_impl(m, t, drawn_of_entry, what):
    """drawn_of_entry: {entry: mask} of the ring entries written since the fill; every other entry must still hold the sentinel"""
    m.sync(); t.sync()
    got, ref = m.obs.cpu().numpy(), t.obs.cpu().numpy()
    for j in range(m.R):
        if j in drawn_of_entry:
            check_rows(got[j], ref[j], drawn_of_entry[j], m.A, f"{what}, ring entry {j}")
        else:
            assert (got[j] == SENT).all(), f"{what}: ring entry {j}, which no tick of the call draws, was written"
    assert (m.slab.cpu().numpy() == SENT).all(), f"{what}: the slab was written by a call into rings"
    assert m.rew.cpu().numpy().tobytes() == t.rew.cpu().numpy().tobytes(), f"{what}: reward ring"
    assert m.done.cpu().numpy().tobytes() == t.done.cpu().numpy().tobytes(), f"{what}: done ring"
    same_outputs(m, t, what)


def check_ring(m, t, drawn, entries, what):
    """one mask for all of the entries"""
    check_ring_impl(m, t, {j: drawn for j in entries}, what)


def alternating(n, phase=0):
    return (np.arange(n) + phase) % 2 == 0


# ---- 1. scenario families -------------------------------------------------------------------------------------------------------------------------------
N1 = 12   # (not a multiple of 8: the prologue's short last group)
FAMILIES = {
    "tower_a1": ("TowerBuilding", 1, 64, 64), "tower_a4": ("TowerBuilding", 4, 64, 64), "tower_a1_48x20": ("TowerBuilding", 1, 48, 20),
    "collect_a1": ("Collect", 1, 64, 64), "collect_a2": ("Collect", 2, 64, 64), "hex_memory": ("HexMemory", 1, 64, 64),
    "hex_memory_48x20": ("HexMemory", 1, 48, 20), "rearrange": ("Rearrange", 1, 64, 64), "obstacles_hard": ("ObstaclesHard", 1, 64, 64),
    "sokoban": ("Sokoban", 1, 64, 64), "boxagone": ("BoxAGone", 1, 64, 64), "football": ("Football", 2, 64, 64),
}


@pytest.mark.parametrize("case", sorted(FAMILIES))
def test_scenario_families(hip, case):
    """1. 24 ticks of mv_step, fast pixels, 12 envs: the even envs drawn, swapped for the odd ones every 8 ticks (host form, replaced twice)"""
    scenario, A, w, h = FAMILIES[case]
    m, t = pair(scenario, A, N1, w, h)
    for tick in range(24):
        if tick % 8 == 0:
            drawn = alternating(N1, tick // 8)
            m.g.set_draw_mask(drawn)
            assert m.g.draw_mask() == "host"
        step_and_check(m, t, drawn, f"{case}, tick {tick}")
    m.close(); t.close()


# ---- 2. every stepping entry ----------------------------------------------------------------------------------------------------------------------------
N2 = 16


def test_step_n_16_into_a_ring_of_16(hip):
    """2. two step launches of 8, the frame-order table, the one-launch pass: every ring entry of two calls"""
    m, t = pair("TowerBuilding", 1, N2, ring=16)
    drawn = alternating(N2)
    m.g.set_draw_mask(drawn)
    for c in range(2):
        entries = call_and_check(m, t, drawn, 16, f"call {c}")
        assert sorted(entries) == list(range(16))
    m.close(); t.close()


def histogram_walk():
    """MV_FRAME_ORDER=0 at mv_create: no frame-order table, every workgroup of a pass walks the tick's histogram, counts itself in (hist_done) and the last
    one zeroes it -- also when it is a skipped frame's.  step_n(8) into a ring of 8 with an alternating mask; then two all-zero calls -- every workgroup of
    those passes leaves early -- and two unmasked ones, which must find histograms and counters clean"""
    assert os.environ.get("MV_FRAME_ORDER") == "0"
    m, t = pair("TowerBuilding", 1, N2, ring=8)
    drawn = alternating(N2, 1)
    m.g.set_draw_mask(drawn)
    for c in range(2):
        call_and_check(m, t, drawn, 8, f"histogram walk, call {c}")
    m.g.set_draw_mask(np.zeros(N2, bool))
    for c in range(2):
        call_and_check(m, t, np.zeros(N2, bool), 8, f"histogram walk, all-zero call {c}")
    m.g.set_draw_mask(None)
    for c in range(2):
        call_and_check(m, t, np.ones(N2, bool), 8, f"histogram walk, unmasked call {c}")
    m.close(); t.close()


def test_histogram_walk_in_a_child_process(hip):
    """2. step_n(8) into a ring of 8 with MV_FRAME_ORDER=0 (read at mv_create), in a child process: histogram_walk above"""
    env = dict(os.environ, MV_FRAME_ORDER="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "histogram walk ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("render", ["last", "none"])
def test_render_modes(hip, render):
    """2. mv_step_n_render: LAST changes only the masked-in rows of the last entry, NONE no byte; 16 ticks (two launches) and 8"""
    m, t = pair("TowerBuilding", 1, N2, ring=16)
    drawn = alternating(N2)
    m.g.set_draw_mask(drawn)
    for k in (16, 8, 8):
        call_and_check(m, t, drawn, k, f"render={render}, k={k}", render=render)
    m.close(); t.close()


@pytest.mark.parametrize("variant", ["pipe1", "pipe0", "unpipelined"])
def test_step_kernel_variants(hip, monkeypatch, variant):
    """2. the software-pipelined two-wave step kernel (MV_STEP_PIPE=1: the tick wave waits at the barriers a skipped frame setup must still meet), the
    one-wave kernel (MV_STEP_PIPE=0), and pipelining off (mv_set_pipelining(0)): batched calls and single ticks"""
    monkeypatch.delenv("MV_STEP_PIPE", raising=False)
    if variant != "unpipelined":
        monkeypatch.setenv("MV_STEP_PIPE", variant[-1])
    m, t = pair("TowerBuilding", 1, N2, ring=8, pipelining=variant != "unpipelined")
    drawn = alternating(N2)
    m.g.set_draw_mask(drawn)
    for c in range(2):
        call_and_check(m, t, drawn, 8, f"{variant}, call {c}")
    for r in (m, t):
        r.g.set_output_ring(0)
        r.R = 0
    for tick in range(3):
        step_and_check(m, t, drawn, f"{variant}, single tick {tick}")
    m.close(); t.close()


def test_pass_overlap(hip):
    """2. mv_set_pass_overlap on ObstaclesHard, rings two calls deep: the passes of consecutive calls run on streams of the gym's own"""
    m, t = pair("ObstaclesHard", 1, N2, ring=16, overlap=True)
    drawn = alternating(N2)
    m.g.set_draw_mask(drawn)
    for c in range(2):   # (an entry is consumed before the next stepping call after the one that produced it: two calls, then the look)
        m.fill(wait=True)
        e0 = call_and_check(m, t, drawn, 8, "", fill=False, check=False)
        e1 = call_and_check(m, t, drawn, 8, "", fill=False, check=False)
        check_ring(m, t, drawn, e0 + e1, f"overlapped passes, calls {2 * c} and {2 * c + 1}")
    m.close(); t.close()


def test_planar_layout(hip):
    """2. obs_layout='chw': three planes per frame, byte stores where the width is no multiple of four (50 x 22) and dword stores (64 x 64)"""
    for w, h in ((64, 64), (50, 22)):
        m, t = pair("TowerBuilding", 1, N2, w, h, ring=8, layout="chw")
        drawn = alternating(N2)
        m.g.set_draw_mask(drawn)
        call_and_check(m, t, drawn, 8, f"chw {w}x{h}")
        for r in (m, t):
            r.g.set_output_ring(0)
            r.R = 0
        step_and_check(m, t, drawn, f"chw {w}x{h}, single tick")
        m.close(); t.close()


def test_exact_pixels_against_the_oracle(hip):
    """2. exact pixel mode (raster_kernel reads vis_count, frame_order_kernel the cost bins): 6 ticks of mv_step on given actions; the drawn rows equal the
    twin's AND the CPU oracle's render; then step_n(8), which exact mode draws tick by tick"""
    import oracle_lib
    n, A = 8, 2
    m, t = pair("TowerBuilding", A, n, 64, 64, mode="exact", ring=0)
    og = oracle_lib.OracleGym("TowerBuilding", 64, 64, n, A, 1, False, {})
    og.seed(ENV_SEED)
    og.reset()
    drawn = alternating(n, 1)
    m.g.set_draw_mask(drawn)
    for tick in range(6):
        act = sample_actions(POLICY_SEED, tick, n * A)
        og.set_action_masks(action_masks(act))
        og.step()
        step_and_check(m, t, drawn, f"exact, tick {tick}", act=act)
        got = m.slab.cpu().numpy()
        for e in np.nonzero(drawn)[0]:
            for a in range(A):
                assert np.array_equal(got[e * A + a], og.get_observation(int(e), a)), f"exact, tick {tick}: env {e} agent {a} against the oracle"
    og.close()
    m.close(); t.close()
    m, t = pair("TowerBuilding", 1, N2, mode="exact", ring=8)
    m.g.set_draw_mask(alternating(N2))
    call_and_check(m, t, alternating(N2), 8, "exact, step_n(8)")
    m.close(); t.close()


# ---- 3. masks ---------------------------------------------------------------------------------------------------------------------------------------------
def test_masks(hip):
    """3. all ones; all zeros (no observation byte, rewards and dones published all the same); one env drawn; one env undrawn; a mask replaced between
    calls; detach -- step_n(8) into a ring of 16, TowerBuilding"""
    m, t = pair("TowerBuilding", 1, N2, ring=16)
    one = np.zeros(N2, bool); one[5] = True
    for name, mask in (("all ones", np.ones(N2, bool)), ("all zeros", np.zeros(N2, bool)), ("one drawn", one), ("one undrawn", ~one),
                       ("replaced", alternating(N2)), ("replaced again", alternating(N2, 1))):
        m.g.set_draw_mask(mask.astype(np.uint8) * 255 if name == "one drawn" else mask)   # (any non-zero byte draws)
        entries = call_and_check(m, t, mask, 8, name)
        if name == "all zeros":   # the ticks' rewards and dones went out although every workgroup of the pass left early
            rew, done = m.rew.cpu().numpy()[entries], m.done.cpu().numpy()[entries]
            assert (rew != -7.0).all() and (done != 9).all()
    m.g.set_draw_mask(None)
    assert m.g.draw_mask() == "none"
    call_and_check(m, t, np.ones(N2, bool), 8, "detached")
    m.close(); t.close()


def test_all_zero_single_ticks_publish(hip):
    """3. all zeros through mv_step: the fast pass publishes rewards and dones with its first workgroups, ahead of the frame look-up"""
    m, t = pair("ObstaclesHard", 1, N1)
    m.g.set_draw_mask(np.zeros(N1, bool))
    for tick in range(4):
        step_and_check(m, t, np.zeros(N1, bool), f"all zeros, tick {tick}")
    m.close(); t.close()


def test_device_mask_without_a_host_synchronisation(hip):
    """3. the device form: the mask is written by a torch kernel on the gym's stream and attached, a batched call enqueued, the mask REWRITTEN by another
    kernel and attached again, the second call enqueued; nothing synchronises in between"""
    import torch
    m, t = pair("TowerBuilding", 1, N2, ring=16)
    masks = [alternating(N2), np.arange(N2) % 3 == 0]
    src = [torch.as_tensor(x).to(DEV) for x in masks]
    dm = torch.ones(N2, dtype=torch.bool, device=DEV)   # (would draw everybody, were it read before the kernels below have run)
    torch.cuda.synchronize()
    m.fill()
    entries = []
    for c in range(2):
        torch.logical_and(src[c], src[c], out=dm)
        m.g.set_draw_mask(dm)
        assert m.g.draw_mask() == "device"
        entries.append(call_and_check(m, t, None, 8, "", fill=False, check=False))
    check_ring_impl(m, t, {**{j: masks[0] for j in entries[0]}, **{j: masks[1] for j in entries[1]}}, "device form, two calls")
    m.close(); t.close()
    del dm


# ---- 4. no stale lists ------------------------------------------------------------------------------------------------------------------------------------
def test_first_drawn_frame_after_an_auto_reset(hip):
    """4. env 5 is undrawn for 20 ticks, through at least one auto-reset (episodes of 12 ticks), then drawn: its first drawn frame is the twin's"""
    m, t = pair("Rearrange", 1, N1, params={"episodeLengthSec": 0.8})
    drawn = np.ones(N1, bool); drawn[5] = False
    m.g.set_draw_mask(drawn)
    finished = 0
    for tick in range(20):
        step_and_check(m, t, drawn, f"tick {tick}")
        finished += int(t.g.get_dones()[5])
    assert finished >= 1, "env 5 finished no episode while it was undrawn: the test would prove nothing"
    m.g.set_draw_mask(None)
    step_and_check(m, t, np.ones(N1, bool), "the first drawn tick")
    m.close(); t.close()


# ---- 5. the pass's bookkeeping ----------------------------------------------------------------------------------------------------------------------------
def test_bookkeeping_survives_all_zero_calls(hip):
    """5. four all-zero step_n(16) calls, then four unmasked ones: every byte of the unmasked calls equals the twin's"""
    m, t = pair("TowerBuilding", 1, N2, ring=16)
    m.g.set_draw_mask(np.zeros(N2, bool))
    for c in range(4):
        call_and_check(m, t, np.zeros(N2, bool), 16, f"all-zero call {c}")
    m.g.set_draw_mask(None)
    for c in range(4):
        call_and_check(m, t, np.ones(N2, bool), 16, f"unmasked call {c}")
    m.close(); t.close()


# ---- 6. composition ---------------------------------------------------------------------------------------------------------------------------------------
def test_with_a_step_mask_and_a_budget(hip):
    """6. envs 0-3 frozen by a step mask, envs 4-7 halted by a budget of 0, the others stepping; of each kind half undrawn.  The twin carries the same
    step mask and budget and no draw mask"""
    m, t = pair("TowerBuilding", 1, N2, ring=8)
    steps = np.ones(N2, bool); steps[0:4] = False
    budget = np.full(N2, -1, np.int32); budget[4:8] = 0
    drawn = np.ones(N2, bool); drawn[[0, 1, 4, 5, 8, 9]] = False
    for r in (m, t):
        r.g.set_step_mask(steps)
        r.g.set_episode_budget(budget)
    m.g.set_draw_mask(drawn)
    for c in range(2):
        call_and_check(m, t, drawn, 8, f"frozen / halted / stepping, call {c}")
    call_and_check(m, t, drawn, 8, "frozen / halted / stepping, render=last", render="last")
    for r in (m, t):
        r.g.set_output_ring(0)
        r.R = 0
    for tick in range(3):
        step_and_check(m, t, drawn, f"frozen / halted / stepping, single tick {tick}")
    assert (m.g.step_mask(), m.g.has_episode_budget(), m.g.draw_mask()) == ("host", True, "host")
    m.close(); t.close()


def test_state_moves_and_the_mask_stays(hip):
    """6. fork, resample, save / load and reset_envs(render=True) with a mask attached: the state moves as in the twin, the mask stays with the env slot,
    the undrawn rows stay untouched"""
    m, t = pair("TowerBuilding", 1, N1)
    drawn = alternating(N1)
    m.g.set_draw_mask(drawn)
    for tick in range(3):
        step_and_check(m, t, drawn, f"tick {tick}")
    src = np.full(N1, -1, np.int32); src[1], src[2] = 0, 3   # (a drawn state into an undrawn slot and the other way round)
    for r in (m, t):
        r.g.fork_envs(src)
    step_and_check(m, t, drawn, "behind the fork")
    perm = np.arange(N1, dtype=np.int32); perm[4], perm[5], perm[6] = 5, 6, 4
    for r in (m, t):
        r.g.resample_envs(perm)
    step_and_check(m, t, drawn, "behind the resampling")
    stores = []
    save = np.full(N1, -1, np.int32); save[0:4] = np.arange(4)
    for r in (m, t):
        stores.append(r.g.new_env_store(4))
        r.g.save_envs(save, stores[-1])
    step_and_check(m, t, drawn, "behind the save")
    load = np.full(N1, -1, np.int32); load[6:10] = np.arange(4)
    for r, s in zip((m, t), stores):
        r.g.load_envs(load, s)
    step_and_check(m, t, drawn, "behind the load")
    flagged = np.zeros(N1, bool); flagged[[0, 1, 6]] = True
    m.fill()
    for r in (m, t):
        r.g.reset_envs(flagged, render=True)
    m.sync(); t.sync()
    check_rows(m.slab.cpu().numpy(), t.slab.cpu().numpy(), drawn, 1, "the frame behind reset_envs(render=True)")
    same_outputs(m, t, "behind reset_envs")
    assert m.g.draw_mask() == "host"
    step_and_check(m, t, drawn, "the tick behind reset_envs")
    m.close(); t.close()
    del stores


def test_episode_log_records(hip):
    """6. the episode log on, episodes that end every few ticks, two agents: the records equal the twin's"""
    m, t = pair("TowerBuilding", 2, N1, params={"episodeLengthSec": -200.0}, log=4096)
    drawn = alternating(N1, 1)
    m.g.set_draw_mask(drawn)
    for tick in range(12):
        step_and_check(m, t, drawn, f"tick {tick}")
    m.fill()
    for r in (m, t):
        r.g.step_n(8, "multidiscrete", POLICY_SEED, r.ticks)
    m.sync(); t.sync()
    check_rows(m.slab.cpu().numpy(), t.slab.cpu().numpy(), drawn, 2, "step_n(8) into the slab")
    a, b = m.g.drain_episode_log(), t.g.drain_episode_log()
    assert a.size > 0 and a.tobytes() == b.tobytes() and m.g.episode_log_dropped == t.g.episode_log_dropped
    m.close(); t.close()


# ---- 7. reset and render ----------------------------------------------------------------------------------------------------------------------------------
def test_reset_render_and_hires(hip):
    """7. mv_reset and mv_render with a mask attached (before the first reset: valid) write only the masked-in rows; mv_draw_hires draws every env"""
    m, t = Rig("TowerBuilding", 2, N1, reset=False), Rig("TowerBuilding", 2, N1, reset=False)
    drawn = alternating(N1)
    bytes0 = m.g.arena_bytes()
    m.g.set_draw_mask(drawn)
    assert m.g.arena_bytes() == bytes0 + N1 and m.g.draw_mask() == "host"
    m.fill()
    m.reset(); t.reset()
    m.sync(); t.sync()
    check_rows(m.slab.cpu().numpy(), t.slab.cpu().numpy(), drawn, 2, "the frame behind mv_reset")
    same_outputs(m, t, "behind mv_reset")
    for tick in range(2):
        step_and_check(m, t, drawn, f"tick {tick}")
    m.fill()
    m.g.render(); t.g.render()
    m.sync(); t.sync()
    check_rows(m.slab.cpu().numpy(), t.slab.cpu().numpy(), drawn, 2, "mv_render")
    m.fill()
    for r in (m, t):
        r.g.set_render_resolution(96, 54)
        r.g.draw_hires()
    for e in (0, 1, N1 - 1):   # (drawn, undrawn, undrawn)
        for a in range(2):
            x, y = m.g.get_hires_observation(e, a), t.g.get_hires_observation(e, a)
            assert x.tobytes() == y.tobytes() and np.unique(x).size > 1, f"hires frame of env {e}, agent {a}"
    m.sync()
    assert (m.slab.cpu().numpy() == SENT).all(), "mv_draw_hires wrote the observation slab"
    step_and_check(m, t, drawn, "the tick behind mv_draw_hires")
    m.g.reset(); t.g.reset()   # (a second reset: the mask is still attached)
    assert m.g.draw_mask() == "host"
    step_and_check(m, t, drawn, "the tick behind a second mv_reset")
    m.close(); t.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """8. a gym in a group; mv_group_create and mv_step_many with a masked member, valid again after detach; a closed gym; a wrong-shaped tensor"""
    import torch
    n = 8
    ra, rb = Rig("TowerBuilding", 1, n, 32, 32), Rig("ObstaclesEasy", 1, n, 32, 32)
    a, b = ra.g, rb.g
    lib = a._lib
    data = np.ones(n, np.uint8)
    mask = alternating(n)
    snaps = lambda g: [g.debug_snapshot_bytes(e).tobytes() for e in range(n)]   # noqa: E731
    handles = (C.c_void_p * 2)(a._g, b._g)
    a.set_draw_mask(mask)
    grp = C.c_void_p()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == -1 and b"draw mask" in lib.mv_last_error()
    before = snaps(a), snaps(b)
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) == -1 and b"draw mask" in lib.mv_last_error()
    assert (snaps(a), snaps(b)) == before, "mv_step_many stepped a gym before it refused"
    a.set_draw_mask(None)
    assert lib.mv_step_many(handles, 2, 1, 1, POLICY_SEED, 0) >= 0, lib.mv_last_error()
    assert lib.mv_group_create(handles, 2, C.byref(grp)) == 0, lib.mv_last_error()
    for g in (a, b):
        for fn in (lib.mv_set_draw_mask_host, lib.mv_set_draw_mask):
            assert fn(g._g, data.ctypes.data) == -1 and b"mv_group" in lib.mv_last_error()
        assert lib.mv_get_draw_mask(g._g) == 0
        with pytest.raises(RuntimeError, match="mv_group"):
            g.set_draw_mask(mask)
    assert lib.mv_group_destroy(grp) == 0
    for bad in (torch.zeros(n + 1, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.bool),
                torch.zeros(2 * n, dtype=torch.bool, device=DEV)[::2], np.zeros(n - 1, bool)):
        with pytest.raises(ValueError, match="set_draw_mask"):
            a.set_draw_mask(bad)
    assert a.draw_mask() == "none"
    a.set_draw_mask(mask)   # (valid again once the group is gone)
    assert a.draw_mask() == "host"
    ra.sync()
    handle = a._g
    lib.mv_close(handle)
    for fn in (lib.mv_set_draw_mask_host, lib.mv_set_draw_mask):
        assert fn(handle, data.ctypes.data) == -1 and b"closed" in lib.mv_last_error()
    assert lib.mv_get_draw_mask(handle) == -1 and b"closed" in lib.mv_last_error()
    a.close(); rb.close()


if __name__ == "__main__":
    histogram_walk()
    print("histogram walk ok")
