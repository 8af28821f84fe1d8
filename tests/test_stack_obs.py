"""CPU: stack observations (mv_set_stack_obs) without a device -- the rule's host twin mv_debug_stack_host against integer numpy (stack_reference), byte for
byte; what the entry points refuse of bad arguments; the new names."""
import ctypes
import re

import numpy as np
import pytest

import megaverse_amd
from megaverse_amd import extension as ext
from stack_reference import FORMATS, SIZES, frame_of, refused, stack

NAMES = ("mv_set_stack_obs", "mv_get_stack_obs", "mv_stack_obs_shape", "mv_get_stack_observation", "mv_debug_stack_host", "mv_debug_stack_device")


@pytest.mark.parametrize("in_place", (False, True))
@pytest.mark.parametrize("clear", (0, 1))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("S", (1, 2, 8))
@pytest.mark.parametrize("factor", (1, 2, 4))
@pytest.mark.parametrize("fmt", tuple(FORMATS))
@pytest.mark.parametrize("chw", (False, True))
def test_host_twin_equals_integer_numpy(chw, fmt, factor, S, W, H, clear, in_place):
    if refused(W, H, factor):
        with pytest.raises(RuntimeError, match="mv_debug_stack_host: the stack's width.*multiple of 4"):
            ext.debug_stack_host(frame_of(1, W, H, chw), S, factor, fmt)
        return
    shape = (S, FORMATS[fmt], H // factor, W // factor)
    for full in (False, True):
        frame = frame_of(W + S + factor, W, H, chw, full)
        prev = np.random.default_rng(H + S).integers(0, 256, shape, dtype=np.uint8)
        want = stack(frame, prev, factor, fmt, clear)
        keep = prev.copy()
        got = ext.debug_stack_host(frame, S, factor, fmt, prev, clear, out=prev if in_place else None)
        assert got.dtype == np.uint8 and got.shape == shape and np.array_equal(got, want)
        assert in_place or np.array_equal(prev, keep)
        assert not full or clear == 0 or (got == 255).all()   # (16 x 255 per channel: no sum overflows, none rounds past 255)


def test_bad_arguments_are_refused():
    lib = ext.load_library()
    frame = frame_of(0, 16, 8, False)
    for text, kw in (("factor must be 1, 2 or 4", dict(frames=4, factor=3)), ("frames must lie in .1, 8.", dict(frames=0, factor=2)),
                     ("frames must lie in .1, 8.", dict(frames=9, factor=2)), ("multiples of factor", dict(frames=4, factor=4, size=(18, 8))),
                     ("multiple of 4", dict(frames=4, factor=4, size=(24, 8))), ("layout must be", dict(frames=4, factor=2, layout=2))):
        with pytest.raises(RuntimeError, match="mv_debug_stack_host: .*" + text):
            ext.debug_stack_host(frame, **kw)
    out = np.zeros(4 * 8 * 4 + 32, np.uint8)
    aligned = out.ctypes.data + (-out.ctypes.data) % 16
    for args in ((None, aligned, aligned), (frame.ctypes.data, None, aligned), (frame.ctypes.data, aligned, None)):
        assert lib.mv_debug_stack_host(args[0], 0, 16, 8, 4, 2, 0, 0, args[1], args[2]) == -1 and b"null pointer" in lib.mv_last_error()
    # a misaligned stack: refused before the device is touched
    assert lib.mv_debug_stack_device(frame.ctypes.data, 0, 16, 8, 4, 2, 0, 0, ctypes.c_void_p(aligned), ctypes.c_void_p(aligned + 4)) == -1
    assert b"16-byte aligned" in lib.mv_last_error()
    with pytest.raises(ValueError, match="factor must be 1, 2 or 4"):
        ext.stack_shape(128, 128, 4, 3)
    assert ext.stack_shape(128, 72, 4, 2, "rgb") == (4, 3, 36, 64)


def test_names():
    header = open(ext.__file__.replace("extension.py", "../include/megaverse_hip.h")).read()
    lib, bound = ext.load_library(), {s[0] for s in ext.SYMBOLS}
    for name in NAMES:
        assert re.search(rf"\b{name}\(", header) and name in bound and hasattr(lib, name), name
    assert ext.OBS_STREAMS["stack"].setter == "mv_set_stack_obs" and megaverse_amd.STACK_GRAY_WEIGHTS == (77, 150, 29)
    assert re.search(r"MV_STACK_GRAY_U8 = 0, MV_STACK_RGB_U8 = 1", header)
