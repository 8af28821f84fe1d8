"""The short-list observation kernels come in two variants (megaverse_amd/csrc/mv_raster.hip: PixOutT<CHW, WHOLE>, picked by the launcher): one for frames
that are whole tiles -- no clamp, no compare with W or H, no masked store -- and the general one for every other size.  Both must draw what the general
path draws (MV_PLANAR=0: every tile by ray casts, read at every launch), byte for byte, stay within the fast pixels' tolerance of the exact kernel
(tests/test_fast_pixels_gpu.py), and write nothing behind the slab."""
import numpy as np
import pytest

from megaverse_amd.extension import MegaverseGym
from test_fast_pixels_gpu import compare

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

N, RING, SENTINEL = 8, 4, 0xA5
# whole tiles at the pixels per lane these sizes take (16 x 4 below 8192 pixels, 16 x 8 from there up); 16 x 8: ONE tile per tile row, the divisor whose
# reciprocal does not fit 32 bits (mv_raster.h: raster_div_magic -- 0 stands for it)
WHOLE = [(64, 64), (128, 72), (16, 8)]
RAGGED = [(72, 40), (100, 60), (20, 12)]


def rollout(monkeypatch, planar, W, H):
    """a gym drawing into a ring of RING slabs with a guard slab behind it: twelve undrawn ticks, one mv_step, one step_n(4); the ring after each"""
    import torch
    if planar is None:
        monkeypatch.delenv("MV_PLANAR", raising=False)
    else:
        monkeypatch.setenv("MV_PLANAR", planar)
    slab = N * H * W * 4
    buf = torch.zeros(RING * slab + slab, dtype=torch.uint8, device="cuda:0")
    buf[RING * slab:] = SENTINEL
    torch.cuda.synchronize()
    g = MegaverseGym("TowerBuilding", W, H, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.set_output_ring(RING, buf.data_ptr())
    g.seed(17); g.reset()
    for st in range(12):
        g.sample_random_actions(9, st); g.step_no_render()
    out = {}
    g.sample_random_actions(9, 12); g.step(); g.synchronize()
    out["step"] = buf[:RING * slab].cpu().numpy().reshape(RING, N, H, W, 4).copy()
    g.step_n(RING, "multidiscrete", 9, 13); g.synchronize()
    out["step_n"] = buf[:RING * slab].cpu().numpy().reshape(RING, N, H, W, 4).copy()
    out["last"] = np.stack([g.get_observation(e, 0) for e in range(N)])
    g.set_pixel_mode("exact"); g.render(); g.synchronize()
    out["exact"] = np.stack([g.get_observation(e, 0) for e in range(N)])
    out["guard"] = buf[RING * slab:].cpu().numpy().copy()
    g.close()
    return out


@pytest.mark.parametrize("W,H", WHOLE + RAGGED)
def test_both_variants_draw_the_general_paths_bytes(hip, monkeypatch, W, H):
    got, ref = rollout(monkeypatch, None, W, H), rollout(monkeypatch, "0", W, H)
    for o in (got, ref):
        assert (o["guard"] == SENTINEL).all(), f"{W}x{H}: {int((o['guard'] != SENTINEL).sum())} bytes behind the slab were written"
        assert o["step_n"][..., 3].min() == 255 and o["step_n"][..., :3].max() > 0   # every ring entry drawn, and not only cleared
    for what in ("step", "step_n", "last"):
        bad = (got[what] != ref[what]).any(axis=-1)
        assert not bad.any(), f"{W}x{H} {what}: {int(bad.sum())} pixels differ from the general path, first at {np.argwhere(bad)[:4].tolist()}"
    assert got["last"].tobytes() in (got["step_n"][j].tobytes() for j in range(RING))   # (the call's last tick is one of the ring's entries)
    compare(got["exact"], got["last"], f"TowerBuilding {W}x{H} exact vs fast")
