"""The fast observation pass loads its ray abscissae from a table the host filled at mv_create (GymView::ray_tab) and takes its size-only constants from
the launch's arguments, instead of dividing in every workgroup.  MV_RAY_TABLE=0 at mv_create leaves the table out -- the prologue computes the abscissae as
it always did -- so the two gyms must agree in every byte they produce; a render at another size than the gym's (hires) must not use the table at all."""
import numpy as np
import pytest

from megaverse_amd.extension import MegaverseGym
from test_fast_pixels_gpu import compare

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

K = 16


def run(monkeypatch, table, scenario, N, A, W, H):
    import torch
    if table:
        monkeypatch.delenv("MV_RAY_TABLE", raising=False)
    else:
        monkeypatch.setenv("MV_RAY_TABLE", "0")
    frames = N * A
    obs = torch.full((K, frames, H, W, 4), 1, dtype=torch.uint8, device="cuda:0")   # (a drawn pixel's alpha is 255: a frame nobody drew shows)
    rew = torch.zeros((K, frames), dtype=torch.float32, device="cuda:0")
    done = torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g = MegaverseGym(scenario, W, H, N, A, 1, False, {})
    monkeypatch.delenv("MV_RAY_TABLE", raising=False)   # (read at mv_create only)
    g.set_pixel_mode("fast")
    g.set_output_ring(K, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
    g.seed(23); g.reset()
    out = []
    for call in range(3):
        g.step_n(K, "multidiscrete", 5, K * call); g.synchronize()
        out.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()))
    g.sample_random_actions(5, 3 * K); g.step(); g.synchronize()   # (the one-tick launch, its own kernel)
    single = np.stack([g.get_observation(e, a) for e in range(N) for a in range(A)])
    arena = g.arena_bytes()
    g.close()
    return out, single, arena


@pytest.mark.parametrize("scenario,N,A,W,H", [("TowerBuilding", 12, 1, 64, 64), ("TowerBuilding", 8, 2, 128, 128), ("TowerBuilding", 12, 1, 100, 60),
                                              ("ObstaclesEasy", 16, 1, 128, 72), ("Collect", 8, 1, 64, 64)])
def test_table_and_in_kernel_abscissae_agree_in_every_byte(hip, monkeypatch, scenario, N, A, W, H):
    (got, gsingle, garena), (ref, rsingle, rarena) = run(monkeypatch, True, scenario, N, A, W, H), run(monkeypatch, False, scenario, N, A, W, H)
    assert 0 < garena - rarena <= 8192   # (the table lives in the gym's arena: W + H floats, rounded up to a page)
    for call in range(3):
        o, r, d = got[call]
        assert o[..., 3].min() == 255, f"{scenario} call {call}: a frame or pixel was not drawn"
        assert o[..., :3].max() > 0
        assert np.array_equal(o, ref[call][0]), f"{scenario} call {call}: {int((o != ref[call][0]).any(axis=-1).sum())} pixels differ"
        assert np.array_equal(r.view(np.uint32), ref[call][1].view(np.uint32)) and np.array_equal(d, ref[call][2])
    assert np.array_equal(gsingle, rsingle)


def test_a_render_at_another_size_computes_its_own(hip):
    """mv_draw_hires renders the gym's state at 256 x 144 while the table is for 128 x 72: the pass must fall back to computing, and agree with the exact
    kernel at that size to the fast pixels' tolerance"""
    g = MegaverseGym("TowerBuilding", 128, 72, 2, 1, 1, False, {})
    g.seed(3); g.reset()
    g.set_render_resolution(256, 144)
    shots = {}
    for mode in ("exact", "fast"):
        g.set_pixel_mode(mode); g.draw_hires()
        shots[mode] = np.stack([g.get_hires_observation(e, 0) for e in range(2)])
    compare(shots["exact"], shots["fast"], "hires 256x144 exact vs fast")
    g.close()
