"""CPU: scan observations (mv_set_scan_obs) without a device -- the rule's host twin mv_debug_scan_host against float64 numpy (scan_reference) on random planes
whose fragile pixels were zeroed first, byte for byte; the rule's edges on planes made for them; the hooks' refusals; the names and the Python tables."""
import re

import numpy as np
import pytest

import megaverse_amd
from megaverse_amd import extension as ext
from scan_reference import BEAMS, CAMERAS, camera, case, planes, safe_planes, scan_numpy, unproject

NAMES = ("mv_set_scan_obs", "mv_get_scan_obs", "mv_scan_obs_beams", "mv_get_scan_observation", "mv_debug_scan_host", "mv_debug_scan_device")


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("K", BEAMS)
@pytest.mark.parametrize("w,h", ((40, 24), (41, 23)))
@pytest.mark.parametrize("instance", (False, True))
@pytest.mark.parametrize("depth_dtype", (np.float32, np.float16))
def test_host_twin_equals_float64(depth_dtype, instance, w, h, K, cam):
    seg, depth, zeroed, want, cam12, band = case(w, h, depth_dtype, instance, K, cam)
    assert zeroed <= 0.10   # (a condition of the comparison, not a measurement)
    got = ext.debug_scan_host(depth, seg, cam12, K, *band)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    # part of the plane is kept and part of it is dropped; some beam is empty or every one is hit
    assert w * h // 8 < want[2].sum() < np.count_nonzero(depth) and ((want[0] == -1) == (want[2] == 0)).all()


def test_pixels_behind_the_eye_are_dropped():
    """pitched 1.2 rad down, the frame's lower rows look backwards between the viewer's feet: f <= 0 there, and those pixels enter no beam"""
    cam12, band = camera(0.3, -1.2), (-40.0, 40.0)
    depth, seg, cls = planes(7, 40, 24, np.float32, False)
    depth = safe_planes(depth, cls, cam12, 8, *band)[0]
    f = unproject(depth, cam12)[1]
    behind = (f <= 0) & (depth != 0) & (cls != 14)
    want = scan_numpy(depth, cls, cam12, 8, *band)[0]
    assert behind.sum() > 40 and want[2].sum() > 40
    assert np.array_equal(ext.debug_scan_host(depth, seg, cam12, 8, *band), want)
    assert np.array_equal(ext.debug_scan_host(np.where(behind, 0, depth).astype(np.float32), seg, cam12, 8, *band), want)   # (with or without them)


def test_nothing_inside_the_band():
    seg, depth, _, _, cam12, _ = case(40, 24, np.float32, False, 40, "level")
    got = ext.debug_scan_host(depth, seg, cam12, 40, 100.0, 200.0)
    assert (got[0] == -1).all() and not got[1:].any()


def test_nearest_wins_and_count_saturates():
    """a level camera, K = W = 8, one row band of depths: beam i is column i, the range floor(64 t sqrt(1 + x^2)), among equal ranges the greater class.
    Then 256 x 256 pixels behind ONE beam: a basis whose right column is (0.01, 0, 0) and whose back column leans right by 0.02 squeezes every column into
    0 < s * bscale < 1, beam K/2 -- 65536 > 32767 pixels"""
    level = camera(0.0, 0.0)
    depth = np.array([[4.0] * 8, [2.0] * 8, [2.0] * 8, [0.0] * 8], np.float32)
    seg = np.array([[3] * 8, [5] * 8, [9] * 8, [9] * 8], np.uint8)
    got = ext.debug_scan_host(depth, seg, level, 8, -50.0, 50.0)
    x = (((np.arange(8) + 0.5) / 8) * 2 - 1) * 1.19175359
    assert got[0].tolist() == np.floor(64 * 2.0 * np.sqrt(1 + x * x)).astype(int).tolist() and (got[1] == 9).all() and (got[2] == 3).all()
    squeezed = np.array([0, 0, 0, 0.01, 0, -0.02, 0, 1, 0, 0, 0, 1], np.float32)
    got = ext.debug_scan_host(np.full((256, 256), 6.0, np.float16), np.full((256, 256), 4 << 12 | 77, np.uint16), squeezed, 8, -50.0, 50.0)
    assert got[2].tolist() == [0, 0, 0, 0, 32767, 0, 0, 0] and got[1, 4] == 4 and got[0, 4] >= 0 and (np.delete(got[0], 4) == -1).all()


@pytest.mark.parametrize("bad", ({"beams": 12}, {"beams": 0}, {"beams": 264}, {"h_lo": 1.0, "h_hi": 1.0}, {"h_lo": 2.0}, {"h_lo": float("-inf")},
                                 {"h_hi": float("inf")}, {"h_hi": float("nan")}, {"depth_format": 2}, {"seg_format": 2}))
def test_the_hook_refuses_and_writes_nothing(bad):
    lib = ext.load_library()
    depth, seg, cam, out = np.ones((4, 8), np.float32), np.ones((4, 8), np.uint8), camera(0.0, 0.0), np.full((3, 264), 0x5A5A, np.int16)
    a = {"beams": 8, "h_lo": -1.0, "h_hi": 1.0, "depth_format": 0, "seg_format": 0, **bad}
    assert lib.mv_debug_scan_host(depth.ctypes.data, a["depth_format"], seg.ctypes.data, a["seg_format"], 8, 4, cam.ctypes.data, a["beams"], a["h_lo"], a["h_hi"],
                                  out.ctypes.data) == -1
    assert b"mv_debug_scan_host" in lib.mv_last_error() and (out == 0x5A5A).all()


def test_symbols_and_python_tables():
    header = open(ext.__file__.replace("extension.py", "../include/megaverse_hip.h")).read()
    lib, bound = ext.load_library(), {s[0] for s in ext.SYMBOLS}
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header) and name in bound and hasattr(lib, name), name
    assert ext.OBS_STREAMS["scan"].setter == "mv_set_scan_obs" and ext.MV_SCAN_OBS_PLANES == 3
    assert megaverse_amd.SCAN_OBS_FIELDS == ("range", "class", "count") and megaverse_amd.SCAN_RANGE_UNIT == 1 / 64
    tan = megaverse_amd.scan_beam_tangents(8)
    assert np.allclose(tan, (np.arange(8) - 3.5) * 1.19175359 / 4) and np.allclose(np.degrees(np.arctan(tan[[0, -1]])), [-46.2, 46.2], atol=0.05)
    with pytest.raises(ValueError, match=r"set_scan_obs: the buffer must be a contiguous int16 CUDA tensor of shape \(2, 8, 3, 64\) on device 0"):
        ext.check_scan_obs(np.zeros((2, 8, 3, 32), np.int16), 2, 8, 64, 0)
