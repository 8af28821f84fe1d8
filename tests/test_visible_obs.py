"""CPU: visible-entity observations (mv_set_visible_obs) without a device -- the rule's host twin mv_debug_visible_host against numpy (visible_reference:
entity_row_of, np.bincount, per-row minima and maxima) on hand-built instance planes of 8 x 16 words, exactly; the exported symbols."""
import numpy as np
import pytest

from megaverse_amd import VISIBLE_OBS_FIELDS, entity_layout, entity_rows
from megaverse_amd import extension as ext
from visible_reference import rows_numpy

H, W = 8, 16
SCENARIOS = ("TowerBuilding", "ObstaclesHard", "Collect", "Sokoban", "HexMemory", "Football")
ROOM_W = 7
# Sokoban's goal cells (x, z), written in no particular order; (2, 9) lies outside the room's 7 columns: it takes a k and has no instance
GOALS = ((3, 5), (1, 6), (5, 0), (1, 2), (2, 9), (0, 0))


def soko_cells():
    cells = np.zeros((32, 32), np.uint8)
    cells[0, 1] = cells[4, 4] = 1   # (walls)
    for x, z in GOALS:
        cells[x, z] = 2
    return cells


def host(words, scenario, A):
    return ext.debug_visible_host(scenario, A, words, ROOM_W, soko_cells() if scenario == "Sokoban" else None)


def numpy_rows(words, scenario, A):
    return rows_numpy(words, scenario, A, ROOM_W, soko_cells())


def word_pool(scenario, A):
    """words of every class -- the classes without rows and those of other scenarios included -- with instances inside, at and beyond every group's size"""
    sizes = sorted({0, 1, A - 1, A, 4095, 1023, 1024} | {s.stop - s.start + d for s in entity_layout(scenario, A).values() for d in (-1, 0)} - {-1})
    pool = [c << 12 | i for c in range(1, 15) for i in sizes]
    pool += [3 << 12 | x * ROOM_W + z for x, z in GOALS if z < ROOM_W] + [3 << 12 | 2 * ROOM_W + 2]   # Sokoban: every goal pad, and a cell that is none
    return np.array([0] + pool, np.uint16)


def test_symbols_and_fields():
    names = {s[0] for s in ext.SYMBOLS}
    assert {"mv_set_visible_obs", "mv_get_visible_obs", "mv_get_visible_observation", "mv_debug_visible_host"} <= names
    assert list(VISIBLE_OBS_FIELDS) == ["count", "x_min", "x_max", "y_min", "y_max"] and ext.MV_VISIBLE_OBS_INTS == 5
    assert "visible" in ext.OBS_STREAMS


@pytest.mark.parametrize("A", (1, 3))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_host_rule_equals_numpy(scenario, A):
    E = entity_rows(scenario, A)
    agent = 13 << 12 | (A - 1)                       # the last agent: a word every scenario gives a row
    row = entity_layout(scenario, A)["agents"].stop - 1
    planes = {"empty": np.zeros((H, W), np.uint16), "corner": np.zeros((H, W), np.uint16), "full": np.full((H, W), agent, np.uint16)}
    planes["corner"][H - 1, W - 1] = agent
    pool, rng = word_pool(scenario, A), np.random.default_rng(5)
    planes["pool"] = np.resize(pool, (4 * H, W + 3))   # every word of the pool at least once, at a width that is no multiple of 8
    planes["runs"] = np.repeat(rng.choice(pool, (H, 4)), 4, axis=1)   # runs of four
    planes["noise"] = rng.choice(pool, (H, W))
    for name, words in planes.items():
        got = host(words, scenario, A)
        assert got.shape == (E, 5) and got.dtype == np.int32
        assert np.array_equal(got, numpy_rows(words, scenario, A)), (scenario, A, name)
    assert not host(planes["empty"], scenario, A).any()
    assert host(planes["corner"], scenario, A)[row].tolist() == [1, W - 1, W - 1, H - 1, H - 1]
    full = host(planes["full"], scenario, A)
    assert full[row].tolist() == [H * W, 0, W - 1, 0, H - 1] and not np.delete(full, row, axis=0).any()
    assert np.count_nonzero(host(planes["pool"], scenario, A)[:, 0]) >= min(E, 3)   # (the pool reaches rows of several groups)


def test_sokoban_goal_rows_follow_cell_order():
    """row k is the k-th goal cell in ascending x * 32 + z, whatever order the plane shows the pads in; the goal outside the room takes a k"""
    order = sorted(GOALS, key=lambda g: g[0] * 32 + g[1])
    words = np.zeros((H, W), np.uint16)
    drawn = [g for g in GOALS if g[1] < ROOM_W]
    for i, (x, z) in enumerate(drawn):
        words[i, i:i + 2] = 3 << 12 | x * ROOM_W + z
    got = host(words, "Sokoban", 1)
    for i, g in enumerate(drawn):
        assert got[order.index(g)].tolist() == [2, i, i + 1, i, i]
    assert got[:, 0].sum() == 2 * len(drawn) and got[order.index((2, 9))].tolist() == [0] * 5
