"""The generic device hook (mv_debug_draw_device) over one scenario of every draw kind (megaverse_amd/csrc/mv_draw.h), at the smallest shapes that still reach
the kernels' shared frame: five envs -- a partial last workgroup of the four-wave kernels, the `k >= count` guard -- and one; two episodes -- the second one
starts from the generator state the first one published --; one and two agents -- the agent loop.  Byte-equal to the same generator on the host
(mv_debug_draw_host) over the fields each kind's own comparison uses.  The seed sweeps are test_collect_draw_gpu.py's, test_obstacles_draw_gpu.py's and
test_hex_draw_gpu.py's."""
import pytest

import test_collect_draw
import test_hex_draw
import test_obstacles_draw
from draw_util import draw_device, draw_host

pytestmark = pytest.mark.gpu

# 0, 1, 42, and two of the existing lists: test_obstacles_draw.py's first clash seed, test_collect_draw_gpu.py's / test_hex_draw_gpu.py's largest seed
SEEDS = [0, 1, 42, test_obstacles_draw.CLASH_SEEDS[0], (1 << 30) - 1]
SAME = {"Collect": test_collect_draw.assert_same_episode, "ObstaclesHard": test_obstacles_draw.assert_same_episode,
        "Empty": test_obstacles_draw.assert_same_episode, "HexMemory": test_hex_draw.assert_same_episode}


@pytest.fixture(scope="module")
def host_episodes():
    """the host twin's second episodes, drawn once per (name, agents, seed)"""
    return {(name, agents, s): draw_host(name, agents, s, 2) for name in SAME for agents in (1, 2) for s in SEEDS}


@pytest.mark.parametrize("agents", [1, 2])
@pytest.mark.parametrize("name", list(SAME))
def test_kernel_draws_its_host_twins_episodes(hip, host_episodes, name, agents):
    for seeds in (SEEDS, SEEDS[3:4]):   # count = 5, then count = 1
        got, _ = draw_device(name, agents, seeds, 2)
        assert len(got) == len(seeds)
        for i, s in enumerate(seeds):
            assert got[i]["seq"] == 2, (name, s, got[i]["seq"])
            SAME[name](got[i], host_episodes[(name, agents, s)], agents, (name, s))
