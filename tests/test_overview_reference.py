"""CPU: the overview cameras' reference and rule (mv_set_overview), before any kernel runs.
(a) tests/overview_reference.py -- a float64 model of a frame from any camera -- at AGENT cameras under the first-person rule, against the CPU oracle's fp32
    frames: the model and the rule are pinned to the arithmetic under test; and the conditions the free-camera cases rest on, asserted on the model alone.
(b) mv_overview_default_camera against a hand derivation from the reference's lines.
(c) mv_debug_overview_camera_host: the camera the device builds, on the host.
(d) look_at / follow records and CAMERA_DTYPE.
(e) every new symbol in the header, the ctypes table and the pybind module."""
import os
import re

import numpy as np
import pytest

import depth_reference as dr
import oracle_lib
import overview_reference as ovr
import pixel_reference as pr
from megaverse_amd import CAMERA_DTYPE, MV_CAMERA_FIRST_PERSON, extension, follow, look_at, overview_default_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ["mv_set_overview", "mv_set_overview_cameras", "mv_set_overview_cameras_host", "mv_draw_overview", "mv_get_overview_observation",
               "mv_overview_device_ptr", "mv_overview_dropped", "mv_overview_capacity", "mv_overview_default_camera", "mv_debug_overview_camera_host"]


def oracle_at(scenario, A, W, H, seed, ticks):
    og = oracle_lib.OracleGym(scenario, W, H, ovr.N_ENVS, A, 1)
    og.seed(seed); og.reset()
    for t in range(ticks):
        pr.step_oracle(og, ovr.N_ENVS, A, t)
    return og


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", ovr.SCENARIOS)
def test_model_at_agent_cameras_against_the_oracle(scenario, A, W, H):
    """first-person AGENT cameras: the model's frame against the oracle's fp32 frame of the same agent, after reset and after 40 scripted ticks"""
    N = ovr.N_ENVS
    og = oracle_at(scenario, A, W, H, ovr.CASES[scenario, (W, H)]["first_person"], 0)
    for ticks in (0, 40):
        if ticks:
            for t in range(40):
                pr.step_oracle(og, N, A, t)
        interior = excused = 0
        for e in range(N):
            og.render_env(e)
            snap = og.snapshot(e)
            for k in range(A):
                model = ovr.render(snap, follow(k, first_person=True), W, H, A)
                r = ovr.judge(og.get_observation(e, k).copy(), model)
                assert not r.failures, f"{scenario} {W}x{H} tick {ticks} env {e} agent {k}: {len(r.failures)} pixels outside the rule, first (x, y, got, model) {r.failures[:4]}"
                interior += r.interior; excused += r.excused
        pixels = N * A * W * H
        print(f"{scenario} {W}x{H} tick {ticks}: interior share {interior / pixels:.3f}, curved pixels excused {excused} (cap {pr.CAP:.0e} of {pixels})")
        assert interior / pixels >= dr.INTERIOR_SHARE
        assert excused <= pr.CAP * pixels
    og.close()


@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("scenario,A", ovr.SCENARIOS)
def test_the_free_camera_cases_meet_their_conditions(scenario, A, W, H):
    """on the model alone: every pose's frame set is at least 80 % interior, and agent 0's own capsule wins at least 20 pixels in every env of the look_at
    and chase poses -- the free-camera test provably covers own-body drawing"""
    N = ovr.N_ENVS
    for name in ovr.POSES:
        seed, ticks = ovr.CASES[scenario, (W, H)][name]
        og = oracle_at(scenario, A, W, H, seed, ticks)
        interior = 0
        for e in range(N):
            snap = og.snapshot(e)
            model = ovr.render(snap, ovr.pose(snap, name), W, H, A)
            interior += int(dr.uniform3x3(model.winner).sum())
            if name != "default":
                own = int((model.winner == ovr.capsule_id(snap, 0, A)).sum())
                assert own >= ovr.OWN_PIXELS, f"{scenario} {W}x{H} {name} env {e}: {own} pixels"
            assert (model.rgba[..., 3] == 255).all() and (model.winner >= 0).any()
        assert interior / (N * W * H) >= dr.INTERIOR_SHARE, f"{scenario} {W}x{H} {name}: {interior / (N * W * H):.3f}"
        og.close()


def test_the_model_draws_own_bodies_only_without_the_first_person_flag():
    og = oracle_at("TowerBuilding", 2, 64, 64, 11, 0)
    snap = og.snapshot(0)
    kinds = lambda hide: [d[0] for d in ovr.drawables(snap, 2, hide)]   # noqa: E731
    assert kinds(-1).count(ovr.CAPSULE) == 2 and kinds(0).count(ovr.CAPSULE) == 1 and len(kinds(-1)) - len(kinds(0)) == 2
    assert ovr.camera_of(snap, follow(1, first_person=True))[2] == 1 and ovr.camera_of(snap, follow(1, back=1.0))[2] == -1
    assert ovr.camera_of(snap, overview_default_camera())[2] == -1
    og.close()


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------------
def test_default_camera_is_the_reference_pose():
    """rendering/src/render_utils.cpp:34-55: root.rotateYLocal(225 deg).translateLocal(0.1, 20, 0.1), tilt.rotateXLocal(-40 deg); the *Local transformations
    multiply from the right: M = Ry(225) T(0.1, 20, 0.1) Rx(-40)"""
    def ry(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])

    def rx(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    R = ry(np.deg2rad(225.0))
    eye = R @ np.array([0.1, 20.0, 0.1])
    C = R @ rx(np.deg2rad(-40.0))
    cam = overview_default_camera()
    assert cam.dtype == CAMERA_DTYPE and int(cam["agent"]) == -1 and int(cam["flags"]) == 0 and not cam["pad"].any()
    got_eye, got_C = cam["eye"].astype(np.float64), cam["c"].astype(np.float64).reshape(3, 3)
    assert np.abs(got_eye - eye).max() <= 1e-6 and np.abs(got_C - C).max() <= 1e-6
    assert np.abs(got_eye - [-0.14142, 20.0, 0.0]).max() <= 1e-5            # the issue's figures
    assert np.abs(-got_C[:, 2] - [0.5417, -0.6428, 0.5417]).max() <= 1e-4   # view direction = -back
    assert np.abs(got_C.T @ got_C - np.eye(3)).max() <= 1e-6               # orthonormal
    assert abs(np.linalg.det(got_C) - 1.0) <= 1e-6                          # right-handed
    up = got_C[:, 1]; view = -got_C[:, 2]
    assert abs(np.dot(np.cross(view, [0.0, 1.0, 0.0]), up)) <= 1e-6 and up[1] > 0   # up in the plane of world up and the view direction
    assert np.array_equal(extension.debug_overview_camera_host(cam)[0], cam["eye"]) and np.array_equal(extension.debug_overview_camera_host(cam)[1].reshape(9), cam["c"])


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------
def twin_f32(pos, basis, pitch):
    """depth_reference.camera64 with every operation in float32 (depth_reference.slab_model_f32's camera lines)"""
    x, y, z = (F(v) for v in pos)
    m00, m02, m20, m22 = (F(v) for v in basis)
    sp, cp = F(np.sin(F(pitch))), F(np.cos(F(pitch)))
    eye = np.array([x, (y + F(dr.EYE_REST)) + F(dr.EYE_UP), z], F)
    C = np.array([[m00, m02 * sp, m02 * cp], [F(0), cp, -sp], [m20, m22 * sp, m22 * cp]], F)
    return eye, C


def state_record(pos, basis, pitch):
    st = np.zeros(32, F)   # the 128-byte AgentState: pos [3], yaw basis m00 m02 m20 m22, pitch, ...
    st[0:3], st[3:7], st[7] = pos, basis, pitch
    return st


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_agent_camera_on_the_host():
    """AGENT mode, zero offset: the fp32 twin of camera64, bit for bit.  The twin takes its sine and cosine from numpy, the library from its own polynomial
    (mv_math.h: sincos_poly, within an ulp of the correctly rounded value), so bits can be demanded where both are exact -- pitch 0, every yaw and position
    of the oracle's agents after reset and after 40 scripted ticks with the pitch set to 0, and synthetic yaws --; at the pitched poses the scripted ticks
    leave, every entry must lie within 2^-23 (one ulp of 1: the two sines' distance times a basis entry of at most 1), and the eye, which no sine enters, must
    still match bit for bit.  (The GPU identity test holds the device's pitched cameras to the oracle's frames byte for byte.)  With an offset: the eye is the
    zero-offset eye + ((c0 x + c1 y) + c2 z) per row, in float32, the basis unchanged."""
    poses = []
    for scenario, A in ovr.SCENARIOS:
        og = oracle_at(scenario, A, 64, 64, 11, 0)
        for ticks in (0, 40):
            if ticks:
                for t in range(40):
                    pr.step_oracle(og, ovr.N_ENVS, A, t)
            for e in range(ovr.N_ENVS):
                for a in og.snapshot(e)["agents"][:A]:
                    poses.append((a["pos"].copy(), a["basis"].copy(), F(a["pitch"])))
        og.close()
    rng = np.random.default_rng(7)
    for yaw in rng.uniform(0, 2 * np.pi, 32):
        poses.append((rng.uniform(0, 20, 3).astype(F), np.array([np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)], F), F(0)))
    assert any(p[2] != 0 for p in poses), "the scripted ticks pitch some camera"
    offset = np.array([0.25, 1.0, 2.0], F)
    for pos, basis, pitch in poses:
        for pt in {float(pitch), 0.0}:
            st = state_record(pos, basis, F(pt))
            eye, C = extension.debug_overview_camera_host(follow(0), st)
            eye2, C2 = twin_f32(pos, basis, F(pt))
            assert np.array_equal(bits(eye), bits(eye2))
            if pt == 0.0:
                assert np.array_equal(bits(C), bits(C2)), (pos, basis)
            else:
                assert np.abs(C.astype(np.float64) - C2.astype(np.float64)).max() <= 2.0 ** -23
            assert np.array_equal(bits(extension.debug_overview_camera_host(follow(0, first_person=True), st)[1]), bits(C))
            cam = follow(0); cam["eye"] = offset
            eye3, C3 = extension.debug_overview_camera_host(cam, st)
            want = np.array([eye[r] + F(F(F(C[r, 0] * offset[0]) + F(C[r, 1] * offset[1])) + F(C[r, 2] * offset[2])) for r in range(3)], F)
            assert np.array_equal(bits(eye3), bits(want)) and np.array_equal(bits(C3), bits(C))
    # FREE: the record as given; refusals
    cam = look_at((1, 2, 3), (4, 0, 5))
    eye, C = extension.debug_overview_camera_host(cam)
    assert np.array_equal(bits(eye), bits(cam["eye"])) and np.array_equal(bits(C.reshape(9)), bits(cam["c"]))
    with pytest.raises(RuntimeError, match="mv_debug_overview_camera_host.*state record"):
        extension.debug_overview_camera_host(follow(0))
    with pytest.raises(RuntimeError, match="mv_debug_overview_camera_host.*agent 8"):
        extension.debug_overview_camera_host(follow(8), state_record((0, 0, 0), (1, 0, 0, 1), 0))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------
def test_camera_records():
    assert CAMERA_DTYPE.itemsize == 64
    assert [CAMERA_DTYPE.fields[n][1] for n in ("eye", "agent", "c", "flags", "pad")] == [0, 12, 16, 52, 56]
    c = follow(3)
    assert int(c["agent"]) == 3 and int(c["flags"]) == 0 and not c["eye"].any() and not c["pad"].any()
    c = follow(1, back=2.0, up=1.0, first_person=True)
    assert c["eye"].tolist() == [0.0, 1.0, 2.0] and int(c["flags"]) == MV_CAMERA_FIRST_PERSON and int(c["agent"]) == 1
    c = look_at((0, 5, 0), (0, 5, -3))   # looking along -z with y up: the identity basis
    assert int(c["agent"]) == -1 and c["eye"].tolist() == [0.0, 5.0, 0.0] and np.array_equal(c["c"].reshape(3, 3), np.eye(3, dtype=F))
    eye, target = np.array([3.0, 6.0, 2.5]), np.array([8.0, 1.0, 8.0])
    c = look_at(eye, target)
    C = c["c"].astype(np.float64).reshape(3, 3)
    view = (target - eye) / np.linalg.norm(target - eye)
    assert np.abs(-C[:, 2] - view).max() <= 1e-6 and np.abs(C.T @ C - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(C) - 1) <= 1e-6
    assert abs(C[1, 0]) <= 1e-7 and C[1, 1] > 0   # no roll: right is horizontal, up points up
    # the stated float32 arithmetic, operation for operation
    b = (eye.astype(F) - target.astype(F)).astype(F)
    b = (b / np.sqrt(F(F(b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]))).astype(F)
    assert np.array_equal(bits(c["c"].reshape(3, 3)[:, 2]), bits(b))
    with pytest.raises(ValueError):
        look_at((1, 1, 1), (1, 1, 1))
    with pytest.raises(ValueError):
        look_at((0, 5, 0), (0, 0, 0))   # up parallel to the view direction
    arr = extension.check_overview_cameras(follow(0), 4, 2)
    assert arr.shape == (4,) and arr.dtype == CAMERA_DTYPE and arr.flags.c_contiguous
    assert extension.check_overview_cameras([follow(0), follow(1), look_at((0, 5, 0), (1, 0, 1)), follow(1)], 4, 2)["agent"].tolist() == [0, 1, -1, 1]
    with pytest.raises(ValueError, match="agent"):
        extension.check_overview_cameras(follow(2), 4, 2)
    with pytest.raises(ValueError, match="records"):
        extension.check_overview_cameras([follow(0)] * 3, 4, 2)
    bad = follow(0); bad["pad"][1] = 1
    with pytest.raises(ValueError, match="pad"):
        extension.check_overview_cameras(bad, 4, 2)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "megaverse_hip.h")).read()
    bound = {name: (res, args) for name, res, args in extension.SYMBOLS}
    lib = extension.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in include/megaverse_hip.h"
        assert name in bound, f"{name} missing from megaverse_amd.extension.SYMBOLS"
        assert getattr(lib, name) is not None
    assert "typedef struct mv_camera" in header and "MV_CAMERA_FIRST_PERSON = 1" in header
    module = open(os.path.join(ROOT, "megaverse_amd", "pybind", "megaverse_module.cpp")).read()
    for name in ("draw_overview", "set_overview", "get_overview_observation"):
        assert f'.def("{name}"' in module, f"{name} missing from the pybind module"
    for name in ("mv_set_overview(", "mv_get_overview_observation(", "mv_draw_overview("):
        assert name in module
    for name in ("set_overview", "overview_obs", "set_overview_cameras", "draw_overview", "get_overview_observation", "overview_dropped"):
        assert callable(getattr(extension.MegaverseGym, name))
    import megaverse_amd
    for name in ("CAMERA_DTYPE", "overview_default_camera", "look_at", "follow"):
        assert hasattr(megaverse_amd, name)
    from megaverse_amd.megaverse_env import MegaverseEnv
    for name in ("overview_obs", "set_overview_cameras", "render_overview"):
        assert callable(getattr(MegaverseEnv, name))
