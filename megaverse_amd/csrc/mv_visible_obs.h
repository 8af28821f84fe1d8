// megaverse_amd/csrc/mv_visible_obs.h -- visible-entity observations (include/megaverse_hip.h: mv_set_visible_obs): the rule, stated once for the kernel that
// writes the record (mv_visible_obs.hip: visible_obs_kernel) and for the host twin the tests compare it with (mv_debug_visible_host).
//
// The record: per drawn FRAME (one agent's view) E rows of VISIBLE_OBS_INTS = 5 int32, [N*A][E][5], E = entity_obs_rows (mv_entity_obs.h): row r describes the
// pixels p of the frame's instance label plane (mv_seg_obs.h: SEG_INSTANCE_U16) with row_of(word[p]) == r --
//   col 0  count: how many such pixels          col 1, 2  x_min, x_max          col 3, 4  y_min, y_max   (inclusive pixel bounds; row 0 is the bottom row,
//                                                                                                        as in the plane)
// and a row with count == 0 is five zeros.  The values are whatever the plane holds: the kernel reads the plane, not the simulator's records.
//
// row_of is the arithmetic the entity rows were laid out for (slot-addressed rows: group base + instance): the word's class names its group of entity_layout,
// the instance its row within the group; -1 where the scenario gives the class no rows (NONE, FLOOR, STRUCTURE, FURNITURE, HUD, a class of another scenario)
// or the instance lies beyond the group.  The one compacted group, Sokoban's EXIT, is resolved from the env's soko_cells: row k is the k-th SOKO_GOAL cell
// in ascending x * SOKO_DIM + z (entity_soko_goal_of), the word's instance is x * W + z (W: the room's width, EnvHeader::W) -- a 1024-byte table instance ->
// row per env (visible_soko_rows on the host; the kernel fills the same table in LDS with ballots).  A goal cell with z >= W is not drawn and has no
// instance: it counts as a goal (it takes a k) and enters no table slot.
#pragma once
#include <stdint.h>

#include "mv_entity_obs.h"
#include "mv_seg_obs.h"
#include "mv_types.h"

namespace mv {

enum : int { VISIBLE_OBS_INTS = 5, VISIBLE_NO_ROW = 255, VISIBLE_SOKO_SLOTS = SOKO_DIM * SOKO_DIM };
static_assert(ENTITY_MAX_ROWS <= VISIBLE_NO_ROW, "a row fits a byte beside the no-row value");
static_assert((SOKO_DIM - 1) * SOKO_DIM + SOKO_DIM - 1 < VISIBLE_SOKO_SLOTS, "every drawn Sokoban cell's instance x * W + z has a table slot");

// THE RULE: word -> row, or VISIBLE_NO_ROW.  soko_rows: Sokoban's instance -> row table [VISIBLE_SOKO_SLOTS] (read for Sokoban's EXIT words only).
// (the layout is indexed with constants only, as in entity_obs_row: a lane-dependent index would keep the struct out of scalar registers)
__host__ __device__ inline int visible_row_of(int scen, const EntityLayout &l, uint16_t word, const uint8_t *soko_rows)
{
    const int cls = seg_class_of(word), inst = seg_instance_of(word);
    if (scen == SCN_SOKOBAN && cls == SEG_EXIT) return inst < VISIBLE_SOKO_SLOTS ? soko_rows[inst] : (int)VISIBLE_NO_ROW;
    const bool terrain = scen == SCN_TOWER ? cls == SEG_BUILDING_ZONE : scen == SCN_OBSTACLES ? cls == SEG_EXIT || cls == SEG_LAVA
                         : scen == SCN_REARRANGE ? cls == SEG_TARGET : false;
    const bool objects = cls == SEG_MOVABLE || cls == SEG_CARRIED;
    const bool rewards = cls == SEG_BALL ? scen == SCN_FOOTBALL : cls == SEG_HAZARD ? scen == SCN_COLLECT
                         : cls == SEG_COLLECTABLE && l.cls[ENTITY_REWARDS] == SEG_COLLECTABLE;
    const bool agents = cls == SEG_AGENT;
    const int base = terrain ? l.base[ENTITY_TERRAIN] : objects ? l.base[ENTITY_OBJECTS] : rewards ? l.base[ENTITY_REWARDS] : l.base[ENTITY_AGENTS];
    const int rows = terrain ? l.rows[ENTITY_TERRAIN] : objects ? l.rows[ENTITY_OBJECTS] : rewards ? l.rows[ENTITY_REWARDS] : agents ? l.rows[ENTITY_AGENTS] : 0;
    return inst < rows ? base + inst : (int)VISIBLE_NO_ROW;
}

// Sokoban's table as a loop: cells [SOKO_DIM * SOKO_DIM] -> rows [VISIBLE_SOKO_SLOTS]; room_w: EnvHeader::W
inline void visible_soko_rows(const uint8_t *cells, int room_w, uint8_t *rows)
{
    const int W = room_w > 1 ? room_w : 1;
    for (int i = 0; i < VISIBLE_SOKO_SLOTS; ++i) rows[i] = VISIBLE_NO_ROW;
    int k = 0;
    for (int c = 0; c < SOKO_DIM * SOKO_DIM; ++c) {
        if (cells[c] != SOKO_GOAL) continue;
        const int x = c / SOKO_DIM, z = c % SOKO_DIM;
        if (z < W && x * W + z < VISIBLE_SOKO_SLOTS && k < ENTITY_SOKO_GOALS) rows[x * W + z] = (uint8_t)k;
        ++k;
    }
}

// one frame's E rows from its plane words [h][w], on the host: the loops
inline void visible_obs_host(int scen, int num_agents, int room_w, const uint8_t *soko_cells, const uint16_t *words, int w, int h, int32_t *out)
{
    const EntityLayout l = entity_layout(scen, num_agents);
    uint8_t soko[VISIBLE_SOKO_SLOTS];
    if (scen == SCN_SOKOBAN) visible_soko_rows(soko_cells, room_w, soko);
    for (int i = 0; i < l.total * VISIBLE_OBS_INTS; ++i) out[i] = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int r = visible_row_of(scen, l, words[(size_t)y * w + x], soko);
            if (r == VISIBLE_NO_ROW) continue;
            int32_t *o = out + r * VISIBLE_OBS_INTS;
            if (o[0]++ == 0) { o[1] = o[2] = x; o[3] = o[4] = y; }
            else {
                o[1] = x < o[1] ? x : o[1]; o[2] = x > o[2] ? x : o[2];
                o[3] = y < o[3] ? y : o[3]; o[4] = y > o[4] ? y : o[4];
            }
        }
}

}  // namespace mv
