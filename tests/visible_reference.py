"""the visible-entity rows in numpy, shared by tests/test_visible_obs.py and tests/test_visible_obs_gpu.py: entity_row_of, np.bincount and the per-row minima
and maxima of pixel coordinates.  Sokoban's EXIT group, which entity_row_of leaves to the caller, is placed as mv_entity_obs.h words it: row k is the k-th goal
cell in ascending x * 32 + z, the word's instance is x * W + z."""
import numpy as np

from megaverse_amd import entity_row_of, entity_rows
from megaverse_amd.extension import SEG_CLASSES, scenario_family

SOKO_DIM, SOKO_GOAL, SOKO_ROWS = 32, 2, 80


def rows_numpy(words, scenario, num_agents, room_w=0, soko_cells=None):
    """one plane's words, uint16 [h, w] -> int32 [E, 5]: count, x_min, x_max, y_min, y_max per entity row, five zeros for a row no pixel names"""
    words = np.ascontiguousarray(words, np.uint16)
    E = entity_rows(scenario, num_agents)
    row = entity_row_of(words, scenario, num_agents)
    if scenario_family(scenario) == 4:
        W = max(int(room_w), 1)
        table = np.full(4096, -1, np.int32)
        for k, c in enumerate(np.flatnonzero(np.asarray(soko_cells, np.uint8).ravel() == SOKO_GOAL)):
            x, z = divmod(int(c), SOKO_DIM)
            if k < SOKO_ROWS and z < W and x * W + z < SOKO_DIM * SOKO_DIM:
                table[x * W + z] = k
        row = np.where(words >> 12 == SEG_CLASSES["EXIT"], table[words & 4095], row)
    ys, xs = np.indices(words.shape)
    out = np.zeros((E, 5), np.int32)
    out[:, 0] = np.bincount(row[row >= 0], minlength=E)
    for r in np.flatnonzero(out[:, 0]):
        m = row == r
        out[r, 1:] = xs[m].min(), xs[m].max(), ys[m].min(), ys[m].max()
    return out
