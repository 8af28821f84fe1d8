"""The stack rule (include/megaverse_hip.h: mv_set_stack_obs) in plain integer numpy, int64 throughout: nothing is rounded twice, so there is nothing fragile.

A frame is uint8 [H, W, 4] (RGBA, alpha ignored) or [3, H, W] (planes); a stack is uint8 [S, C, H / factor, W / factor], plane-set S - 1 the newest."""
import numpy as np

SIZES = ((16, 8), (48, 24), (40, 24))   # (W, H); 40 x 24: w is no multiple of 16 at any factor, and no multiple of 4 at factor 4 -- refused
FORMATS = {"gray": 1, "rgb": 3}


def refused(W, H, factor):
    return W % factor != 0 or H % factor != 0 or (W // factor) % 4 != 0


def frame_of(seed, W, H, chw, full=False):
    """random bytes (full: every byte 255, the sums' headroom) in either layout"""
    rng = np.random.default_rng(seed)
    shape = (3, H, W) if chw else (H, W, 4)
    return np.full(shape, 255, np.uint8) if full else rng.integers(0, 256, shape, dtype=np.uint8)


def image(frame, factor, fmt):
    """one frame -> uint8 [C, h, w]"""
    rgb = (frame if frame.shape[0] == 3 and frame.shape[2] != 4 else np.moveaxis(frame[..., :3], 2, 0)).astype(np.int64)
    _, H, W = rgb.shape
    sums = rgb.reshape(3, H // factor, factor, W // factor, factor).sum(axis=(2, 4))   # R, G, B over each factor x factor block
    n = factor * factor
    if fmt == "rgb":
        return ((sums + n // 2) // n).astype(np.uint8)
    return ((77 * sums[0] + 150 * sums[1] + 29 * sums[2] + 128 * n) // (256 * n)).astype(np.uint8)[None]


def stack(frame, prev, factor, fmt, clear):
    """the stack behind one drawn frame: refilled on a clear, else prev shifted by one with the image last"""
    img = image(frame, factor, fmt)
    return np.repeat(img[None], prev.shape[0], 0) if clear else np.concatenate([prev[1:], img[None]])


def fold(frames, clears, S, factor, fmt, start=None):
    """a chain of frames -> the stack behind the last"""
    img = image(frames[0], factor, fmt)
    out = np.zeros((S,) + img.shape, np.uint8) if start is None else start
    for f, c in zip(frames, clears):
        out = stack(f, out, factor, fmt, c)
    return out
