"""GPU: the observation kernels under the pixel acceptance rule of tests/pixel_reference.py -- every pixel within 1/255 of the float64
evaluation of the render model, or explained by a probe within delta_px / a depth within eps_t of it; at most 1e-4 of a frame set explained.  The
float64 reference is the oracle's (mvo_render_f64 / mvo_explain_f64) on the state of an oracle twin stepped by the same actions, computed once per
sampled tick and shared by every kernel variant judged there.  The CPU twin (test_pixel_reference.py) holds the fp32 oracle to the same rule, shows
that the rule rejects frames the count rule of test_fast_pixels_gpu.py accepts, and that the matrix covers every primitive kind and frame class."""
import os

import pytest

import oracle_lib
import pixel_reference as pr
from hip_util import diff_snapshots, hip_snapshot
from megaverse_amd.extension import MegaverseGym

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

CELLS = [(s, a, w, h) for s, a in pr.MATRIX for w, h in pr.SIZES + ([pr.SIZES_LARGE[s]] if s in pr.SIZES_LARGE else [])]


@pytest.fixture(autouse=True)
def _boxoban(monkeypatch):
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels


class Variant:
    """one way of drawing the twin's state: a gym (made under `create_env`), a pixel mode, environment switches read at every launch (`launch_env`),
    and the rule's parameters for the kernel that draws"""

    def __init__(self, name, scenario, mode="fast", create_env=None, launch_env=None, layout=None):
        self.name, self.mode, self.create_env, self.launch_env, self.layout = name, mode, create_env or {}, launch_env or {}, layout
        fast = mode == "fast"
        self.delta, self.eps = (pr.DELTA_FAST, pr.eps_t_fast(scenario)) if fast else (pr.DELTA_ORACLE, pr.EPS_4ULP)
        self.gym, self.verdict = None, None


def run(monkeypatch, scenario, A, W, H, variants, ticks=pr.TICKS):
    """the matrix rollout of (scenario, A, W, H): an oracle twin and one HIP gym per distinct (create_env, layout), all stepped by the same scripted actions;
    after reset and every pr.EVERY ticks every variant draws and is judged against the float64 reference of the twin's state -> the variants' verdicts"""
    N = pr.N_ENVS
    og = oracle_lib.OracleGym(scenario, W, H, N, A, 1)
    og.seed(pr.SEED); og.reset()
    gyms = {}
    for v in variants:
        key = (tuple(sorted(v.create_env.items())), v.layout)
        if key not in gyms:
            with monkeypatch.context() as m:
                for k, val in v.create_env.items():
                    m.setenv(k, val)
                g = MegaverseGym(scenario, W, H, N, A, 1, False, {})
                if v.layout:
                    g.set_obs_layout(v.layout)
                g.set_pixel_mode("fast"); g.seed(pr.SEED); g.reset()
            gyms[key] = g
        v.gym = gyms[key]
        v.verdict = pr.Verdict(f"{scenario} A={A} {W}x{H} {v.name}")
    try:
        for tick in range(ticks + 1):
            if tick % pr.EVERY == 0:
                for g in gyms.values():   # the pixel mode does not touch the simulation: the twin's state is the state drawn
                    for e in range(N):
                        assert not diff_snapshots(og.snapshot(e), hip_snapshot(g, e), A), f"{scenario} tick {tick} env {e}: the twin's state differs"
                refs = {(e, a): pr.reference(og, e, a) for e in range(N) for a in range(A)}
                for v in variants:
                    with monkeypatch.context() as m:
                        for k, val in v.launch_env.items():
                            m.setenv(k, val)
                        v.gym.set_pixel_mode(v.mode)
                        v.gym.render()
                        frames = {ea: v.gym.get_observation(*ea) for ea in refs}
                    for (e, a), ref in refs.items():
                        pr.judge(v.verdict, og, e, a, frames[(e, a)], v.delta, v.eps, ref)
            if tick < ticks:
                acts, masks = pr.scripted(N, A, tick)
                og.set_action_masks(masks); og.step_norender()
                for g in gyms.values():
                    g.set_actions_batched(acts); g.step_no_render()
    finally:
        og.close()
        for g in gyms.values():
            g.close()
    return [v.verdict for v in variants]


@pytest.mark.parametrize("scenario,A,W,H", CELLS)
def test_fast_kernel_under_the_rule(hip, monkeypatch, scenario, A, W, H):
    """every pixel the fast kernel draws over the matrix is right or explained; the explained share (printed) is within the cap"""
    run(monkeypatch, scenario, A, W, H, [Variant("fast", scenario)])[0].check()


@pytest.mark.parametrize("scenario,A", pr.MATRIX)
def test_exact_kernel_under_the_rule(hip, monkeypatch, scenario, A):
    """exact mode is the oracle's fp32 bytes (asserted elsewhere); through the same helper, with the oracle's parameters: a check of the harness"""
    run(monkeypatch, scenario, A, 48, 20, [Variant("exact", scenario, mode="exact")])[0].check()


def test_launch_variants_under_the_rule(hip, monkeypatch):
    """what the launcher can choose for a short-list scenario -- one or two pixels per lane, planar tiles on or off, the channel-first layout --, each
    against the reference and not only against one another"""
    s = "TowerBuilding"
    vs = [Variant("MV_FAST_PPL=1", s, launch_env={"MV_FAST_PPL": "1"}), Variant("MV_FAST_PPL=2", s, launch_env={"MV_FAST_PPL": "2"}),
          Variant("MV_PLANAR=0", s, launch_env={"MV_PLANAR": "0"}), Variant("MV_PLANAR=1", s, launch_env={"MV_PLANAR": "1"}),
          Variant("obs_layout=chw", s, layout="chw")]
    verdicts = run(monkeypatch, s, 2, 64, 64, vs)
    for v in verdicts:
        v.check()


@pytest.mark.parametrize("scenario", ["Collect", "HexMemory"])
def test_depth_class_variants_under_the_rule(hip, monkeypatch, scenario):
    """the long lists in depth classes (MV_DEPTH_SORT=1, read at creation) and as found (0)"""
    vs = [Variant(f"MV_DEPTH_SORT={d}", scenario, create_env={"MV_DEPTH_SORT": d}) for d in ("0", "1")]
    for v in run(monkeypatch, scenario, 2, 64, 64, vs):
        v.check()


def test_hires_under_the_rule(hip):
    """draw_hires of one TowerBuilding env at a reduced target (192 x 108), fast mode"""
    W, H = 192, 108
    og = oracle_lib.OracleGym("TowerBuilding", W, H, 1, 1, 1)
    hg = MegaverseGym("TowerBuilding", 128, 72, 1, 1, 1, False, {})
    hg.set_pixel_mode("fast"); hg.set_render_resolution(W, H)
    og.seed(3); hg.seed(3); og.reset(); hg.reset()
    assert not diff_snapshots(og.snapshot(0), hip_snapshot(hg, 0), 1)
    hg.draw_hires()
    v = pr.Verdict(f"hires TowerBuilding {W}x{H}")
    pr.judge(v, og, 0, 0, hg.get_hires_observation(0, 0), pr.DELTA_FAST, pr.eps_t_fast("TowerBuilding"))
    og.close(); hg.close()
    v.check()
