"""The scan-observation rule (megaverse_amd/csrc/mv_scan_obs.h) in float64 numpy, for tests/test_scan_obs.py and tests/test_scan_obs_gpu.py.

scan_numpy(depth [h, w] float, cls [h, w] int, cam12, beams, h_lo, h_hi) -> (int16 [3, K], fragile [h, w] bool).  A hit pixel (depth != 0, not HUD) is fragile
when the fp32 evaluation could decide it differently: s * bscale or 64 r within 1e-2 of an integer, hgt within 1e-3 of h_lo or h_hi, or f within 1e-3 of 0 --
unless hgt or f alone drop it on both sides anyway (hgt more than 1e-3 outside the band, f < -1e-3), whatever its beam would have been.  The fp32 evaluation
is some ten operations of relative error 6e-8 on values of at most 64 * 50 = 3200 (the planes' depths reach 30, r at most 30 * 1.6): under 2e-3.
safe_planes zeroes the fragile pixels' depths (no hit) once."""
import functools

import numpy as np

from map_reference import HUD, TAN_X, TAN_Y, camera  # noqa: F401  (camera: for the tests)


def unproject(depth, cam12):
    """-> u, f, hgt [h, w] float64 and t: the rule as far as mv_map_obs.h goes"""
    h, w = depth.shape
    t = depth.astype(np.float64)
    c = np.asarray(cam12, np.float32).astype(np.float64)[3:].reshape(3, 3)
    x = (((np.arange(w) + 0.5) / w) * 2 - 1) * np.float64(np.float32(TAN_X))
    y = (((np.arange(h) + 0.5) / h) * 2 - 1) * np.float64(np.float32(TAN_Y))
    d = np.einsum("kj,jhw->khw", c, np.stack([x[None, :] * t, y[:, None] * t, -t]))
    return d[0] * c[0, 0] + d[2] * c[2, 0], d[0] * c[2, 0] - d[2] * c[0, 0], d[1], t


def scan_numpy(depth, cls, cam12, beams, h_lo, h_hi):
    K = int(beams)
    u, f, hgt, t = unproject(depth, cam12)
    bscale = np.float64(np.float32(K // 2) / np.float32(TAN_X))   # (the rule's own factor, formed once in fp32)
    hit = (t != 0) & (cls != HUD)
    with np.errstate(divide="ignore", invalid="ignore"):
        sb, r64 = np.where(f > 0, u / f, 0.0) * bscale, np.sqrt(u * u + f * f) * 64
    near = lambda v, eps: np.abs(v - np.rint(v)) < eps
    dropped = (hgt < h_lo - 1e-3) | (hgt > h_hi + 1e-3) | (f < -1e-3)
    fragile = hit & ~dropped & (near(sb, 1e-2) | near(r64, 1e-2) | (np.abs(hgt - h_lo) < 1e-3) | (np.abs(hgt - h_hi) < 1e-3) | (np.abs(f) < 1e-3))
    fb = np.floor(sb)
    ok = hit & (f > 0) & (hgt >= h_lo) & (hgt <= h_hi) & (fb >= -(K // 2)) & (fb < K // 2)
    beam = (fb[ok] + K // 2).astype(np.int64)
    key = (np.clip(np.floor(r64), 0, 32767).astype(np.int64)[ok] << 4) | (15 - cls.astype(np.int64)[ok])
    count, best = np.bincount(beam, minlength=K), np.full(K, 1 << 40, np.int64)
    np.minimum.at(best, beam, key)
    out = np.stack([np.where(count > 0, best >> 4, -1), np.where(count > 0, 15 - (best & 15), 0), np.minimum(count, 32767)])
    return out.astype(np.int16), fragile


def safe_planes(depth, cls, cam12, beams, h_lo, h_hi):
    """depth with its fragile pixels zeroed -> (depth, the share of pixels zeroed)"""
    fragile = scan_numpy(depth, cls, cam12, beams, h_lo, h_hi)[1]
    return np.where(fragile, depth.dtype.type(0), depth), float(fragile.mean())


def planes(seed, w, h, depth_dtype, instance):
    """random planes: depths in [0.05, 30] with nine zeros in twenty, classes in [0, 15) (HUD among them), instance words where asked.  (An unpitched camera
    has s * bscale = (px + 0.5 - w/2) K / w: at w = 40, K = 256 one column in five sits ON a beam boundary and is fragile as a whole; with this many
    zeros and the cameras' bands that is 9 % of a plane.  At K = 2 w EVERY column does: tests/test_scan_obs_gpu.py says what it does about 128 x 128, K = 256)"""
    rng = np.random.default_rng(seed)
    depth = np.where(rng.random((h, w)) < 0.45, 0.0, rng.uniform(0.05, 30.0, (h, w))).astype(depth_dtype)
    cls = rng.integers(0, 15, (h, w))
    seg = (cls << 12 | rng.integers(0, 4096, (h, w))).astype(np.uint16) if instance else cls.astype(np.uint8)
    return depth, seg, cls


# the grid both test files share: cameras (level; pitched down with a yaw: beams drift over columns; yawed only) with a height band that keeps about half of
# each one's hits; the level camera with K == W puts every pixel centre at a half-integer of s * bscale
CAMERAS = {"level": (camera(0.0, 0.0), (-7.5, 11.0)), "down": (camera(3.9, -0.4), (-14.0, -1.0)), "yaw": (camera(0.7, 0.0), (-6.0, 12.5))}
BEAMS = (8, 40, 256)


@functools.lru_cache(maxsize=None)
def case(w, h, depth_dtype, instance, K, cam):
    """one cell of the grid, computed once -> seg, safe depth, the share zeroed, the expected [3, K], cam12, band"""
    cam12, band = CAMERAS[cam]
    depth, seg, cls = planes(w * K + len(cam), w, h, depth_dtype, instance)
    depth, zeroed = safe_planes(depth, cls, cam12, K, *band)
    want, fragile = scan_numpy(depth, cls, cam12, K, *band)
    assert not fragile.any()
    return seg, depth, zeroed, want, cam12, band
