"""What mv_create reads from the scenario table (mv_scenarios.h), on the device: for each of the fifteen names and one or two agents per env (4 envs,
32 x 32 observations, no MV_* switch set) the reward-shaping keys in order and their defaults, the arena's size and the two recommendations -- literals
recorded on an MI355X from the library BEFORE the table existed -- then a reset and 8 stepped ticks without error or warning; and the group refusals."""
import os
import warnings

import numpy as np
import pytest

from megaverse_amd.extension import GymGroup, MegaverseGym

pytestmark = pytest.mark.gpu

OBSTACLES_KEYS = ['teamSpirit', 'obstaclesAgentAtExit', 'obstaclesAllAgentsAtExit', 'obstaclesExtraReward', 'obstaclesAgentCarriedObjectToExit']
# name -> (shaping keys, their defaults, mv_arena_bytes for A = 1 and A = 2, mv_recommended_ticks_per_call, mv_recommended_pass_overlap)
PINNED = {
    'TowerBuilding': (['teamSpirit', 'towerPickedUpObject', 'towerVisitedBuildingZoneWithObject', 'towerBuildingReward'], [0.1, 0.1, 0.1, 1.0],
                      (4087808, 6463488), 8, 0),
    'ObstaclesEasy': (OBSTACLES_KEYS, [0.0, 1.0, 5.0, 0.5, 0.0], (4087808, 6463488), 8, 1),
    'ObstaclesMedium': (OBSTACLES_KEYS, [0.0, 1.0, 5.0, 0.5, 0.0], (4087808, 6463488), 8, 1),
    'ObstaclesHard': (OBSTACLES_KEYS, [0.0, 1.0, 5.0, 0.5, 0.0], (4087808, 6463488), 8, 1),
    'ObstaclesWalls': (OBSTACLES_KEYS, [0.0, 1.0, 5.0, 0.5, 1.0], (4087808, 6463488), 8, 1),
    'ObstaclesSteps': (OBSTACLES_KEYS, [0.0, 1.0, 5.0, 0.5, 1.0], (4087808, 6463488), 8, 1),
    'ObstaclesLava': (OBSTACLES_KEYS, [0.0, 1.0, 5.0, 0.5, 1.0], (4087808, 6463488), 8, 1),
    'Collect': (['teamSpirit', 'collectSingleGood', 'collectSingleBad', 'collectAll', 'collectAbyss'], [0.0, 1.0, -1.0, 5.0, -0.5], (10629120, 19066880), 8, 1),
    'Sokoban': (['teamSpirit', 'sokobanBoxOnTarget', 'sokobanBoxLeavesTarget', 'sokobanAllBoxesOnTarget'], [0.0, 1.0, -1.0, 10.0], (4091904, 6467584), 8, 1),
    'HexMemory': (['teamSpirit', 'memoryCollectGood', 'memoryCollectBad'], [0.0, 1.0, -1.0], (19226624, 35692544), 8, 1),
    'HexExplore': (['teamSpirit', 'exploreSolved'], [0.0, 5.0], (19226624, 35692544), 8, 1),
    'Rearrange': (['teamSpirit', 'rearrangeOneMoreObjectCorrectPosition', 'rearrangeAllObjectsCorrectPosition'], [0.0, 1.0, 10.0], (4034560, 6410240), 8, 1),
    'Empty': (['teamSpirit'], [0.0], (4067328, 6443008), 8, 0),
    'BoxAGone': (['teamSpirit', 'boxagoneTouchedFloor', 'boxagonePerStepReward'], [0.0, -0.1, 0.01], (10436608, 18874368), 1, 0),
    'Football': (['teamSpirit'], [0.0], (4304896, 6680576), 8, 1),
}
NOT_IN_UNION = "mv_group_create: mv_group_create: {} cannot be stepped in a group of gyms; step it as a gym of its own (MultiTaskGym: MV_MULTITASK_UNION=0)"


@pytest.fixture(autouse=True)
def no_switches(hip, monkeypatch):
    for key in [k for k in os.environ if k.startswith("MV_")]:
        monkeypatch.delenv(key)
    monkeypatch.setenv("BOXOBAN_LEVELS", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban"))   # Sokoban: synthetic levels


@pytest.mark.parametrize("agents", [1, 2])
@pytest.mark.parametrize("name", list(PINNED))
def test_gym_is_what_it_was(name, agents):
    keys, defaults, arena, ticks, overlap = PINNED[name]
    g = MegaverseGym(name, 32, 32, 4, agents, 0, False, {})
    try:
        shaping = g.get_reward_shaping(3, agents - 1)
        assert list(shaping) == keys
        assert [np.float32(v) for v in shaping.values()] == [np.float32(v) for v in defaults]
        assert g.arena_bytes() == arena[agents - 1]
        assert g.recommended_ticks_per_call() == ticks
        assert int(g.recommended_pass_overlap()) == overlap
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            g.reset()
            for _ in range(8):
                g.step()
            g.synchronize()
    finally:
        g.close()


@pytest.mark.parametrize("name", ["BoxAGone", "Football"])
def test_group_refuses_what_the_union_kernels_lack(name):
    a, b = MegaverseGym("TowerBuilding", 32, 32, 4, 1, 0, False, {}), MegaverseGym(name, 32, 32, 4, 1, 0, False, {})
    try:
        for gyms in ([a, b], [b, a]):
            with pytest.raises(RuntimeError) as e:
                GymGroup(gyms)
            assert str(e.value) == NOT_IN_UNION.format(name)
    finally:
        a.close()
        b.close()
