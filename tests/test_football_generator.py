"""Football without a GPU: the host-side episode generator (mv_gen_football.cpp, through mv_debug_generate_football) against the Python
restatement in football_model.py byte for byte; the name reaching mv_create; and known answers of the stated ball model
that the GPU tests then hold the device to, tick for tick."""
import ctypes as C

import numpy as np
import pytest

import football_model as M
from megaverse_amd import extension as ext


def env_seeds(master, n):
    r = M.MT19937(master)
    return [M.rand_range(0, 1 << 30, r) for _ in range(n)]


def generated(agents, env_seed, n, base_len=60.0):
    lib = ext.load_library()
    size = lib.mv_debug_generate_football(agents, env_seed, n, base_len, None, 0)
    assert size == M.BLOB.itemsize, (size, M.BLOB.itemsize)
    buf = np.zeros(n * size, np.uint8)
    assert lib.mv_debug_generate_football(agents, env_seed, n, base_len, buf.ctypes.data, buf.size) == n
    return buf.view(M.BLOB)


def check_ranges(b, agents):
    L, W, H = int(b["length"]), int(b["width"]), int(b["height"])
    assert 14 <= L <= 23 and 12 <= W <= 23 and 3 <= H <= 6
    assert b["num_boxes"] == 5
    assert b["boxes"][0]["min"].tolist() == [0, 0, 0] and b["boxes"][0]["max"].tolist() == [L, 1, W]
    assert all(int(bx["max"][1]) == H for bx in b["boxes"][1:5])
    seen = set()
    for i in range(agents):
        x, y, z = (float(v) for v in b["spawn"][i])
        assert 1 <= x <= L - 2 and 1 <= z <= W - 2 and y == 1.0 and x == int(x) and z == int(z)
        assert (x, z) not in seen
        seen.add((x, z))
        assert 0.0 <= b["yaw_frand"][i] < 1.0
    assert not b["spawn"][agents:].any() and not b["yaw_frand"][agents:].any()


@pytest.mark.parametrize("agents", [1, 2, 4, 8])
def test_generator_matches_restatement_byte_for_byte(agents):
    for env_seed in env_seeds(77 + agents, 12):
        got = generated(agents, env_seed, 20)
        want = M.episodes(agents, env_seed, 20)
        for n in range(20):
            assert got[n].tobytes() == want[n].tobytes(), (env_seed, n)
            check_ranges(got[n], agents)


def test_every_room_size_occurs():
    blobs = [b for s in env_seeds(5, 40) for b in generated(1, s, 10)]
    assert {int(b["length"]) for b in blobs} == set(range(14, 24))
    assert {int(b["width"]) for b in blobs} == set(range(12, 24))
    assert {int(b["height"]) for b in blobs} == set(range(3, 7))


def test_params_reach_the_generator():
    assert generated(1, 5, 1, base_len=2.0)[0]["episode_len"] == 2.0


def test_episode_generator_and_feeder_hooks_keep_refusing_football():
    lib = ext.load_library()
    assert lib.mv_debug_generate_episode(b"Football", 1, 1, 1, 60.0, None, 0) < 0
    assert lib.mv_debug_feeder_selftest(b"Football", 4, 1, 2, 2) < 0


def test_create_knows_the_name():
    """whatever a machine without a GPU says next, the name itself is accepted (case-insensitive)"""
    lib = ext.load_library()
    for name in (b"Football", b"football", b"FOOTBALL"):
        cfg = ext._Config(name, 64, 64, 1, 1, 1, 0, 0, None, None, 0, 0, 0)
        h = C.c_void_p()
        rc = lib.mv_create(C.byref(cfg), C.byref(h))
        if rc == 0:
            lib.mv_close(h)
        else:
            assert b"Unknown scenario" not in lib.mv_last_error()
    cfg = ext._Config(b"NoSuchScenario", 64, 64, 1, 1, 1, 0, 0, None, None, 0, 0, 0)
    assert lib.mv_create(C.byref(cfg), C.byref(C.c_void_p())) < 0
    assert b"Football" in lib.mv_last_error()


def test_supported_scenarios_lists_football():
    from megaverse_amd.megaverse_env import SUPPORTED_SCENARIOS
    assert "Football" in SUPPORTED_SCENARIOS


# ---- the ball model's known answers ------------------------------------------------------------------------------------------------------

ROOM = [((M.F32(0), M.F32(0), M.F32(0)), (M.F32(20), M.F32(1), M.F32(16)))]   # a floor, top at y = 1
FAR = [(M.F32(100), M.F32(100), M.F32(100))]                                   # one agent, nowhere near


def test_free_fall_until_first_contact():
    s = M.reset_state()
    dt = 1.0 / 15.0
    for t in range(1, 40):
        s = M.step(s, ROOM, FAR, FAR, [0])
        want = 5.0 - 10.0 * dt * dt * t * (t + 1) / 2
        if s["contacts"]:
            break
        assert s["pos"][1] == pytest.approx(want, rel=1e-6), t
        assert s["pos"][0] == 5.0 and s["pos"][2] == 5.0 and s["radius"] == 1.0
    else:
        pytest.fail("the ball never reached the floor")
    assert t > 5   # (from y = 5 to 2: 11 ticks of free fall)


def test_ball_settles_on_the_floor():
    s = M.reset_state()
    for _ in range(60):
        s = M.step(s, ROOM, FAR, FAR, [0])
    assert abs(float(s["pos"][1]) - 2.0) <= 0.04 and np.abs(s["vel"]).max() < 1e-3


def test_ball_at_rest_stays_bit_identical():
    s = M.reset_state()
    s["pos"] = (5.0, 2.0, 5.0)
    s["radius"] = 1.0
    s0 = s.copy()
    for _ in range(900):
        s = M.step(s, ROOM, FAR, FAR, [0])
        s["contacts"] = 0
        assert s.tobytes() == s0.tobytes()


@pytest.mark.parametrize("dx,dz", [(1.5, 0.0), (0.0, -1.2), (0.9, 0.9)])
def test_one_kick_changes_the_velocity_by_force_times_dt(dx, dz):
    s = M.reset_state()
    s["pos"] = (8.0, 2.0, 8.0)
    s["radius"] = 1.0
    agent = [(M.F32(8.0 - dx), M.F32(1.75 + 0.0), M.F32(8.0 - dz))]   # on the floor: ghost origin 1 + 0.75
    s = M.kicks(s, agent, [M.ACT_INTERACT])
    assert s["kicks"] == 1
    d = np.array([dx, 2.0 - (1.75 + 0.05), dz])
    n = d / np.linalg.norm(d)
    want_f = 70.0 * np.array([n[0], 0.5, n[2]])
    assert np.allclose(s["force"], want_f, rtol=1e-6, atol=1e-5)
    v0 = s["vel"].copy()
    s1 = M.ball_step(s, [], FAR)   # (no contacts: the pure integration step)
    dt = 1.0 / 15.0
    assert np.allclose(s1["vel"] - v0, (want_f + np.array([0.0, -10.0, 0.0])) * dt, rtol=1e-6, atol=1e-6)
    assert not s1["force"].any()


def test_kick_range_is_strict():
    s = M.reset_state()
    s["pos"] = (8.0, 2.0, 8.0)
    near = [(M.F32(6.5), M.F32(1.75), M.F32(8.0))]    # horizontal 1.5: |d| = 1.5 (0.2 lower)
    far = [(M.F32(6.15), M.F32(1.75), M.F32(8.0))]    # horizontal 1.85
    assert M.kicks(s, near, [M.ACT_INTERACT])["kicks"] == 1
    assert M.kicks(s, far, [M.ACT_INTERACT])["kicks"] == 0
    assert M.kicks(s, near, [0])["kicks"] == 0


def test_a_kicked_ball_rolls_and_stays_in_the_room():
    blob = M.episodes(1, 3, 1)[0]
    boxes = M.room_boxes(blob)
    L, W = int(blob["length"]), int(blob["width"])
    s = M.reset_state()
    s["pos"] = (5.0, 2.0, 5.0)
    agent = [(M.F32(3.6), M.F32(1.75), M.F32(5.0))]
    s = M.kicks(s, agent, [M.ACT_INTERACT])
    rolled = False
    for t in range(400):
        s = M.step(s, boxes, FAR, FAR, [0])
        x, y, z = (float(v) for v in s["pos"])
        assert 1.0 + 1.0 - 0.05 <= x <= L - 1 - 1.0 + 0.05 and 1.0 + 1.0 - 0.05 <= z <= W - 1 - 1.0 + 0.05, t
        assert y >= 2.0 - 0.05
        rolled |= bool(np.abs(s["ang"]).max() > 0.5)
    assert rolled
