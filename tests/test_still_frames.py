"""Still frames without a device (include/megaverse_hip.h: mv_set_still_frames): the rule's host twin against a numpy model, the rule and the carry together
against a model in which every rendered tick writes its frame, the symbols and the Python surface.  The twins are compiled from the header the kernels use
(megaverse_amd/csrc/mv_still_frames.h)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import megaverse_amd.extension as ext
from megaverse_amd.extension import MegaverseGym
from megaverse_amd.megaverse_env import MegaverseEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_PASS, DRAWN, UNDRAWN, STILL = 0, 1, -1, -2


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "megaverse_hip.h")).read(), flags=re.S)


def test_symbols_declared_exported_bound():
    text = header()
    lib = ext.load_library()
    for name, args in (("mv_set_still_frames", 2), ("mv_get_still_frames", 1), ("mv_debug_still_rule_host", 8), ("mv_debug_still_carry_host", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == args, f"{name}: {m.group(1)}"
        assert hasattr(lib, name), f"{name} is not exported"
        bound = [s for s in ext.SYMBOLS if s[0] == name]
        assert len(bound) == 1 and len(bound[0][2]) == args and bound[0][1] is C.c_int, name
    assert lib.mv_abi_version() == 2   # (additive)
    rule_h = open(os.path.join(ROOT, "megaverse_amd", "csrc", "mv_still_frames.h")).read()
    for word in ("__host__ __device__", "still_after_tick", "still_verdict", "still_after_frames", "still_carry_plan", "FRAME_STILL = -2"):
        assert word in rule_h, word
    # no gym: -1 with a text that names the call, no crash
    assert lib.mv_set_still_frames(None, 1) == -1 and b"mv_set_still_frames" in lib.mv_last_error()
    assert lib.mv_get_still_frames(None) == -1 and b"mv_get_still_frames" in lib.mv_last_error()


def test_python_surface():
    p = inspect.signature(MegaverseGym.set_still_frames).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    assert list(inspect.signature(MegaverseGym.still_frames).parameters) == ["self"]
    assert inspect.signature(MegaverseEnv.__init__).parameters["still_frames"].default is False   # (the default is off)
    p = inspect.signature(MegaverseEnv.set_still_frames).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    from megaverse_amd.multitask import MultiTaskGym
    assert not hasattr(MultiTaskGym, "set_still_frames")
    p = inspect.signature(MegaverseEnv.run_episodes).parameters   # (run_episodes keeps its defaults)
    assert list(p) == ["self", "episodes", "policy", "render", "max_ticks", "actions", "seed"] and p["render"].default == "none"


# ---- the rule

def model_rule(steps, has_pass, mask, stale):
    k, N = steps.shape
    stale = (np.asarray(stale) != 0).astype(np.uint8).copy()
    verdict = np.zeros((k, N), np.int32)
    for t in range(k):
        for e in range(N):
            if steps[t, e]:
                stale[e] = 1
            if not has_pass[t]:
                continue
            if mask is not None and mask[e] == 0:
                verdict[t, e] = UNDRAWN
            elif stale[e]:
                verdict[t, e] = DRAWN
                stale[e] = 0
            else:
                verdict[t, e] = STILL
    return verdict, stale


@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("N", [1, 12])
def test_rule_twin_against_numpy_model(k, N):
    rng = np.random.default_rng(100 * k + N)
    masks = [None, np.zeros(N, np.uint8), np.ones(N, np.uint8), rng.integers(0, 2, N).astype(np.uint8), (rng.integers(0, 2, N) * 200).astype(np.uint8)]
    passes = [np.ones(k, np.uint8), np.zeros(k, np.uint8), np.eye(1, k, k - 1, dtype=np.uint8)[0], rng.integers(0, 2, k).astype(np.uint8)]
    seen = set()
    for trial in range(12):
        steps = (rng.random((k, N)) < (0.0, 0.15, 0.5, 1.0)[trial % 4]).astype(np.uint8)
        for mask in masks:
            for has_pass in passes:
                for stale in (np.ones(N, np.uint8), np.zeros(N, np.uint8), rng.integers(0, 2, N).astype(np.uint8), (rng.integers(0, 2, N) * 7).astype(np.uint8)):
                    v, s = ext.debug_still_rule_host(steps, has_pass, mask, stale)
                    mv, ms = model_rule(steps, has_pass, mask, stale)
                    assert v.tobytes() == mv.tobytes(), (trial, steps, has_pass, mask, stale, v, mv)
                    assert s.tobytes() == ms.tobytes()
                    seen.update(np.unique(v).tolist())
    if k > 1:
        assert seen == {NO_PASS, DRAWN, UNDRAWN, STILL}


def test_rule_prefix_suffix_within_a_call():
    """nothing but an env's own ticks makes it stale within a call: with a pass on every tick, the verdicts of a drawn env are a drawn prefix and a still
    suffix whenever the env stops stepping for good (step mask: never steps; budget or macro step: stops at some tick)"""
    rng = np.random.default_rng(5)
    k, N = 16, 12
    stop = rng.integers(0, k + 1, N)
    steps = (np.arange(k)[:, None] < stop[None, :]).astype(np.uint8)
    for stale in (np.ones(N, np.uint8), np.zeros(N, np.uint8)):
        v, s = ext.debug_still_rule_host(steps, np.ones(k, np.uint8), None, stale)
        for e in range(N):
            drawn = stop[e] if stop[e] > 0 else (1 if stale[e] else 0)   # (a stale env that never steps is drawn once, by the first pass)
            assert (v[:drawn, e] == DRAWN).all() and (v[drawn:, e] == STILL).all(), (e, stop[e], v[:, e])
        assert not s.any()


# ---- the pipeline: rule twin -> passes write the drawn rows -> carry twin, against a model in which every rendered tick writes its frame

FB = 24   # bytes of a synthetic frame


def frame_of(f, version):
    """distinct bytes for every (frame, state version)"""
    return ((np.arange(FB, dtype=np.uint32) * 7 + 131 * f + 977 * version + 13) % 251).astype(np.uint8)


@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("mult", ["k", "k+1", "2k", "3k"])
@pytest.mark.parametrize("A", [1, 2])
def test_pipeline_every_ring_byte_equals_the_always_draw_model(k, mult, A):
    R = {"k": k, "k+1": k + 1, "2k": 2 * k, "3k": 3 * k}[mult]
    N = 7
    frames = N * A
    rng = np.random.default_rng(1000 * k + 10 * R + A)
    ring = np.full((R, frames, FB), 0xA5, np.uint8)      # the gym with still frames: passes + carry
    model = ring.copy()                                   # its twin: every rendered tick writes every drawn env's frames
    home = np.full(frames, -1, np.int32)
    stale = np.ones(N, np.uint8)                          # (switching the option on)
    version = np.zeros(N, np.int64)
    budget = rng.integers(1, 40, N)                       # ticks an env may still step before it halts for good ("budget-like")
    tick = 0
    n_still = n_copies = 0
    for call in range(60):
        mode = ("every", "every", "last", "none")[int(rng.integers(0, 4))]
        kk = int(rng.integers(1, k + 1))
        step_mask = (rng.random(N) < (0.5 if call % 3 else 0.9)).astype(np.uint8)    # replaced between calls
        draw_mask = None if call % 4 else (rng.random(N) < 0.7).astype(np.uint8)
        if call % 7 == 6:                                 # an "all stale" event between calls (reset, fork, load, ...): states change, every byte set
            version += 1
            stale[:] = 1
            budget = np.maximum(budget, rng.integers(0, 20, N))
        # which envs step in which tick: frozen by the mask for the whole call; halted mid-call when the budget runs out
        steps = np.zeros((kk, N), np.uint8)
        for t in range(kk):
            for e in range(N):
                if step_mask[e] and budget[e] > 0:
                    steps[t, e] = 1
                    budget[e] -= 1
        has_pass = np.zeros(kk, np.uint8)
        if mode == "every":
            has_pass[:] = 1
        elif mode == "last":
            has_pass[kk - 1] = 1
        verdict, stale = ext.debug_still_rule_host(steps, has_pass, draw_mask, stale)
        entries_all = [(tick + t) % R for t in range(kk)]
        # the passes, in tick order: the gym's write the DRAWN rows; the model's write every row the draw mask lets through
        ver = version.copy()
        for t in range(kk):
            ver += steps[t]
            if not has_pass[t]:
                continue
            for e in range(N):
                for a in range(A):
                    f = e * A + a
                    if verdict[t, e] == DRAWN:
                        ring[entries_all[t], f] = frame_of(f, ver[e])
                    if draw_mask is None or draw_mask[e]:
                        model[entries_all[t], f] = frame_of(f, ver[e])
        version = ver
        # patterns inside a call are drawn-prefix / still-suffix, as the kernels produce them
        rendered = [t for t in range(kk) if has_pass[t]]
        for e in range(N):
            col = [int(verdict[t, e]) for t in rendered]
            if col and col[0] != UNDRAWN:
                d = sum(1 for v in col if v == DRAWN)
                assert col == [DRAWN] * d + [STILL] * (len(col) - d), col
        # the carry, on the rendered ticks: what the passes read per FRAME (a drawn frame: its list length)
        if rendered:
            vf = np.repeat(verdict[rendered], A, axis=1).astype(np.int32)
            vf[vf == DRAWN] = rng.integers(0, 200, int((vf == DRAWN).sum()))
            before = ring.copy()
            ext.debug_still_carry_host(vf, [entries_all[t] for t in rendered], ring, home)
            n_still += int((vf == STILL).sum())
            n_copies += int((ring != before).any(axis=2).sum())
        tick += kk
        assert ring.tobytes() == model.tobytes(), f"call {call} ({mode}, {kk} ticks, R = {R}): rows {np.argwhere((ring != model).any(axis=2)).tolist()}"
    assert n_still > 50 and n_copies > 20, (n_still, n_copies)   # (the comparison was about something)


def test_carry_reads_one_source_per_run():
    """a run of still ticks copies from the entry the frame was last drawn into -- not in a chain -- and skips the entry that is the source"""
    R, frames = 8, 2
    ring = np.zeros((R, frames, FB), np.uint8)
    for r in range(R):
        ring[r] = 10 + r
    home = np.array([5, -1], np.int32)
    verdict = np.array([[STILL, 17], [STILL, STILL], [STILL, STILL]], np.int32)
    ext.debug_still_carry_host(verdict, [4, 5, 6], ring, home)
    assert [int(ring[r, 0, 0]) for r in range(R)] == [10, 11, 12, 13, 15, 15, 15, 17]     # frame 0: entry 5's bytes to 4 and 6, entry 5 itself untouched
    assert [int(ring[r, 1, 0]) for r in range(R)] == [10, 11, 12, 13, 14, 14, 14, 17]     # frame 1: drawn in tick 0 (entry 4), still after it
    assert home.tolist() == [6, 6]
    # user-undrawn: nothing moves
    ring2, home2 = ring.copy(), np.array([3, 3], np.int32)
    ext.debug_still_carry_host(np.full((3, frames), UNDRAWN, np.int32), [0, 1, 2], ring2, home2)
    assert ring2.tobytes() == ring.tobytes() and home2.tolist() == [3, 3]
    # a still frame without a home (cannot happen in the gym: switching on makes every env stale) copies nothing and reads nothing out of range
    home3 = np.array([-1, 99], np.int32)
    ext.debug_still_carry_host(np.full((1, frames), STILL, np.int32), [2], ring2, home3)
    assert ring2.tobytes() == ring.tobytes() and home3.tolist() == [2, 2]
