// megaverse_amd/csrc/mv_entity_obs.h -- entity observations (include/megaverse_hip.h: mv_set_entity_obs): the per-OBJECT record, stated once for the kernels
// that write it (mv_step_kernels.h: entity_obs_write; mv_obs_rows.hip: the gather behind a reset or mv_render) and for the host hook the tests compare it with
// (mv_debug_entity_obs_host).  E rows of ENTITY_OBS_FLOATS = 8 float32 per env, [N][E][8], taken from the env's state AFTER the tick -- auto-reset included,
// as the state and scene rows (mv_state_obs.h, mv_scene_obs.h).
//
// E is fixed for a gym: it depends on the scenario and the agent count alone (entity_layout, from the capacities of mv_types.h).  Rows are SLOT-ADDRESSED,
// not compacted: every record has the same row for the gym's lifetime, row = its group's base + its record index, and a record that does not exist this
// episode (index >= the header's count) is a row of eight +0.0f.  So row_of(seg word) is arithmetic and a learner's tensor shapes never change.
//
//   col 0     the entity's segmentation word, (float)seg_word(class, instance) -- below 2^16, so exact -- with the classes of mv_seg_obs.h and the instance
//             seg_rule gives the same record: the value the instance plane (MV_SEG_INSTANCE_U16) shows for that drawable.  0 for an empty row.
//   col 1..3  centre, world units            col 4..6  half extents, world units            col 7  state, by class (below)
//
// The two conversions of mv_scene_obs.h and no others:  copied -- the 32 bits are moved;  int -- an integer converted with (float); the arithmetic on small
// integers below is exact in fp32.  vs is the scenario's voxel size (mv_scene_obs.h's unit note): 1, and 2 for BoxAGone and Sokoban.  A voxel box [min, max)
// has centre (min + max) * (0.5 * vs) and half extents (max - min) * (0.5 * vs); a voxel cell v is the box [v, v + 1).
//
// Groups, in the seg rule's order (terrain slots | movable objects | collectables | agents); rows per scenario:
//   TowerBuilding     building zone      1 row                 BUILDING_ZONE          x, z: EnvHeader::bz; y: the slab frame_setup_body draws, [1, 1 + 0.05]
//                                                                                     (fp32: centre (1 + 1.05f) * 0.5f, half (1.05f - 1) * 0.5f)     bz_reward, copied
//   Obstacles family  terrain[i]         MAX_TERRAIN           EXIT / LAVA by type,   the voxel box as stored                                        type, int
//                                                              as seg_rule
//   Rearrange         target item i      MAX_ITEMS             TARGET                 the voxel cell off + (RE_LEFT_X, RE_LEFT_Y, RE_LEFT_Z)         shape, int
//   Sokoban           goal cells         MAX_OBJECTS           EXIT                   the voxel cell (x, 1, z) -- the level the boxes stand on       1
//   Tower, Obstacles, Collect, Rearrange, Sokoban
//                     objects[j]         MAX_OBJECTS           MOVABLE (state <= 0)   the voxel cell (x, y, z)                                       state, int
//                                                              CARRIED (state > 0)    centre: the carrier's pos (agent state - 1), copied; a cell's   (1 + k: the
//                                                                                     half extents                                                    carrier)
//   Obstacles         rewards[i]         MAX_REWARDS           COLLECTABLE            voxel cell                                                     state, int
//   Collect           rewards[i]         COLLECT_MAX_REWARDS   COLLECTABLE / HAZARD   voxel cell                                  state, int (0: picked up; 2: red)
//   HexMemory, HexExplore
//                     hex_objs[i]        HEX_MAX_OBJS          COLLECTABLE            centre a[3], half extents b[3], copied       alive ? 1 + shape : 0, from meta
//   Football          the ball           1 row                 BALL                   pos[3], copied; radius, copied, three times                    kicks, int
//   every scenario    agent k            A rows, last group    AGENT                  pos, copied; (CAP_R, CAP_HH, CAP_R) of mv_physics.h            carrying, int
//
// Sokoban's goal cells: soko_cells has SOKO_DIM^2 = 1024 cells, too many for a fixed row each, so this ONE group is compacted: row k of the group is the k-th
// SOKO_GOAL cell in ascending cell index x * SOKO_DIM + z, and its word carries the instance the seg rule gives that cell's pad, x * W + z (W: the room's
// width, EnvHeader::W: the index of the cell among the level's drawn cells).  A Boxoban level has as many goals as boxes, and the generator keeps at most
// MAX_OBJECTS boxes (mv_gen_sokoban.cpp), but it takes the level file's word for the goals: '.' and '+' become goal cells, unchecked against the '$' and
// '*' count.  The files decide, so the bound is the group's capacity: goal cells beyond the MAX_OBJECTS-th in cell order get no row.
// HexMemory's good / bad is hidden state: the `good` bit of meta is no input of any column, as in the seg rule.
// Left out: floor, structure, furniture, BoxAGone's platforms and the HUD get no rows -- static structure, and the platforms alone would need
// BAG_MAX_PLATFORMS = 972 rows.  BoxAGone and Empty list their agents only.  Rows describe the voxel cell the scenario logic works with, not drawn sizes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mv_rearrange.h"
#include "mv_seg_obs.h"
#include "mv_types.h"

namespace mv {

enum : int { ENTITY_OBS_FLOATS = 8, ENTITY_GROUPS = 4, ENTITY_SOKO_GOALS = MAX_OBJECTS, ENTITY_MAX_ROWS = 192 };
enum : int { ENTITY_TERRAIN = 0, ENTITY_OBJECTS = 1, ENTITY_REWARDS = 2, ENTITY_AGENTS = 3 };
// the capsule's radius and half height (mv_physics.h: CAP_R, CAP_HH; asserted equal where both are visible, mv_step.hip)
constexpr float ENTITY_CAP_R = 0.33f, ENTITY_CAP_HH = 1.05f * 0.5f;
// the building zone's slab, as frame_setup_body draws it (mv_frame.h)
constexpr float ENTITY_BZ_Y0 = 1.0f, ENTITY_BZ_Y1 = 1.0f + 0.05f;

static_assert(MAX_OBJECTS + COLLECT_MAX_REWARDS + MAX_AGENTS <= ENTITY_MAX_ROWS && MAX_TERRAIN + MAX_OBJECTS + MAX_REWARDS + MAX_AGENTS <= ENTITY_MAX_ROWS
                  && HEX_MAX_OBJS + MAX_AGENTS <= ENTITY_MAX_ROWS && ENTITY_SOKO_GOALS + MAX_OBJECTS + MAX_AGENTS <= ENTITY_MAX_ROWS,
              "entity observations: every scenario's rows fit three rounds of 64 lanes");
static_assert(offsetof(HexRec, b) == 16 && offsetof(HexRec, meta) == 12 && offsetof(FootballState, radius) == 12 && offsetof(FootballState, kicks) == 28
                  && offsetof(TerrainBox, type) == 12 && offsetof(TerrainBox, max) == 16,
              "entity observations: a HexRec is a[3], meta, b[3], colour; the ball is pos[3], radius, vel[3], kicks; a terrain box min[3], type, max[3], pad");

// per group: base row, rows, the seg class of its first kind (0: the group is empty)
struct EntityLayout {
    int32_t base[ENTITY_GROUPS], rows[ENTITY_GROUPS], cls[ENTITY_GROUPS];
    int32_t total;   // E
};
__host__ __device__ inline EntityLayout entity_layout(int scen, int num_agents)
{
    const bool hex = scen == SCN_HEX_MEMORY || scen == SCN_HEX_EXPLORE;
    const bool objects = scen == SCN_TOWER || scen == SCN_OBSTACLES || scen == SCN_COLLECT || scen == SCN_REARRANGE || scen == SCN_SOKOBAN;
    EntityLayout l;
    l.rows[ENTITY_TERRAIN] = scen == SCN_TOWER ? 1 : scen == SCN_OBSTACLES ? (int)MAX_TERRAIN : scen == SCN_REARRANGE ? (int)MAX_ITEMS
                             : scen == SCN_SOKOBAN ? (int)ENTITY_SOKO_GOALS : 0;
    l.cls[ENTITY_TERRAIN] = scen == SCN_TOWER ? (int)SEG_BUILDING_ZONE : scen == SCN_OBSTACLES || scen == SCN_SOKOBAN ? (int)SEG_EXIT
                            : scen == SCN_REARRANGE ? (int)SEG_TARGET : (int)SEG_NONE;
    l.rows[ENTITY_OBJECTS] = objects ? (int)MAX_OBJECTS : 0;
    l.cls[ENTITY_OBJECTS] = objects ? (int)SEG_MOVABLE : (int)SEG_NONE;
    l.rows[ENTITY_REWARDS] = scen == SCN_OBSTACLES ? (int)MAX_REWARDS : scen == SCN_COLLECT ? (int)COLLECT_MAX_REWARDS : hex ? (int)HEX_MAX_OBJS
                             : scen == SCN_FOOTBALL ? 1 : 0;
    l.cls[ENTITY_REWARDS] = scen == SCN_FOOTBALL ? (int)SEG_BALL : l.rows[ENTITY_REWARDS] ? (int)SEG_COLLECTABLE : (int)SEG_NONE;
    l.rows[ENTITY_AGENTS] = num_agents;
    l.cls[ENTITY_AGENTS] = SEG_AGENT;
    int at = 0;
    for (int g = 0; g < ENTITY_GROUPS; ++g) { l.base[g] = at; at += l.rows[g]; }
    l.total = at;
    return l;
}
__host__ __device__ inline int entity_obs_rows(int scen, int num_agents) { return entity_layout(scen, num_agents).total; }
// the scenario's voxel size (mv_scene_obs.h: the unit note)
__host__ __device__ inline float entity_voxel_size(int scen) { return scen == SCN_SOKOBAN || scen == SCN_BOXAGONE ? 2.0f : 1.0f; }

// one env's records.  A pointer the scenario's rows do not name is never read through (entity_layout gives such a group no rows).
struct EntitySrc {
    int32_t scenario, num_agents;
    const EnvHeader *hdr;
    const TerrainBox *terrain;       // [MAX_TERRAIN]         Obstacles family
    const ArrangementItem *items;    // [MAX_ITEMS]           Rearrange
    const uint8_t *soko;             // [SOKO_DIM * SOKO_DIM] Sokoban
    const MovableObject *objects;    // [MAX_OBJECTS]
    const MovableObject *rewards;    // [the scenario's reward capacity]
    const HexRec *hex_objs;          // [HEX_MAX_OBJS]        HexMemory, HexExplore
    const FootballState *fb;         //                       Football
    const AgentState *agents;        // [num_agents]
};

__host__ __device__ inline uint32_t entity_bits_of_int(int32_t v)
{
    const float f = (float)v;
    uint32_t w;
    __builtin_memcpy(&w, &f, sizeof w);
    return w;
}
__host__ __device__ inline uint32_t entity_bits_of_float(float f)
{
    uint32_t w;
    __builtin_memcpy(&w, &f, sizeof w);
    return w;
}
__host__ __device__ inline uint32_t entity_bits_at(const void *p, int byte)
{
    uint32_t w;
    __builtin_memcpy(&w, (const char *)p + byte, sizeof w);
    return w;
}

struct EntityRow { uint32_t w[ENTITY_OBS_FLOATS]; };

// a voxel box [lo, hi) -> columns 1..6
__host__ __device__ inline void entity_voxel_box(EntityRow &r, float half_vs, int x0, int y0, int z0, int x1, int y1, int z1)
{
    r.w[1] = entity_bits_of_float((float)(x0 + x1) * half_vs); r.w[2] = entity_bits_of_float((float)(y0 + y1) * half_vs);
    r.w[3] = entity_bits_of_float((float)(z0 + z1) * half_vs);
    r.w[4] = entity_bits_of_float((float)(x1 - x0) * half_vs); r.w[5] = entity_bits_of_float((float)(y1 - y0) * half_vs);
    r.w[6] = entity_bits_of_float((float)(z1 - z0) * half_vs);
}
__host__ __device__ inline void entity_voxel_cell(EntityRow &r, float half_vs, int x, int y, int z) { entity_voxel_box(r, half_vs, x, y, z, x + 1, y + 1, z + 1); }

// Sokoban: the row of goal cell `cell` (x * SOKO_DIM + z); W: EnvHeader::W
__host__ __device__ inline EntityRow entity_soko_goal_row(int cell, int W)
{
    EntityRow r = {};
    const int x = cell / SOKO_DIM, z = cell % SOKO_DIM;
    r.w[0] = entity_bits_of_int(seg_word(SEG_EXIT, x * (W > 1 ? W : 1) + z));
    entity_voxel_cell(r, 0.5f * 2.0f, x, 1, z);
    r.w[7] = entity_bits_of_int(1);
    return r;
}

// Row `row` (0 <= row < l.total) of one env, every group but Sokoban's goal cells (whose rows the caller places: the step kernels' wave with ballots, the host
// twin and the gather with entity_soko_goal_of's loop -- both give the same integers): all zero there.  What a row is made of is decided first -- the
// scenario is uniform, the group a comparison of the row with the layout's bases -- then its record is loaded once.
__host__ __device__ inline EntityRow entity_obs_row(const EntitySrc &s, const EntityLayout &l, int row)
{
    EntityRow r = {};
    const EnvHeader *h = s.hdr;
    const int scen = s.scenario;
    const float hv = 0.5f * entity_voxel_size(scen);
    // (the layout is indexed with constants only: an index that differs by lane would keep the struct in scratch, or in LDS)
    const int bo = l.base[ENTITY_OBJECTS], br = l.base[ENTITY_REWARDS], ba = l.base[ENTITY_AGENTS];
    const int g = row < bo ? ENTITY_TERRAIN : row < br ? ENTITY_OBJECTS : row < ba ? ENTITY_REWARDS : ENTITY_AGENTS;
    const int i = row - (row < bo ? 0 : row < br ? bo : row < ba ? br : ba);
    if (g == ENTITY_AGENTS) {
        const AgentState *a = s.agents + i;
        r.w[0] = entity_bits_of_int(seg_word(SEG_AGENT, i));
        r.w[1] = entity_bits_at(a, 0); r.w[2] = entity_bits_at(a, 4); r.w[3] = entity_bits_at(a, 8);
        r.w[4] = r.w[6] = entity_bits_of_float(ENTITY_CAP_R); r.w[5] = entity_bits_of_float(ENTITY_CAP_HH);
        r.w[7] = entity_bits_of_int(a->carrying);
    } else if (g == ENTITY_OBJECTS) {
        if (i < h->num_objects) {
            const MovableObject o = s.objects[i];
            r.w[0] = entity_bits_of_int(seg_word(o.state > 0 ? SEG_CARRIED : SEG_MOVABLE, i));
            if (o.state > 0) {
                const int k = (int)o.state - 1 < s.num_agents ? (int)o.state - 1 : s.num_agents - 1;   // (a carrier is an agent of the env: never beyond its records)
                const AgentState *a = s.agents + k;
                r.w[1] = entity_bits_at(a, 0); r.w[2] = entity_bits_at(a, 4); r.w[3] = entity_bits_at(a, 8);
                r.w[4] = r.w[5] = r.w[6] = entity_bits_of_float(hv);
            } else entity_voxel_cell(r, hv, o.x, o.y, o.z);
            r.w[7] = entity_bits_of_int(o.state);
        }
    } else if (g == ENTITY_REWARDS) {
        if (scen == SCN_FOOTBALL) {
            const FootballState *b = s.fb;
            r.w[0] = entity_bits_of_int(seg_word(SEG_BALL, 0));
            r.w[1] = entity_bits_at(b, 0); r.w[2] = entity_bits_at(b, 4); r.w[3] = entity_bits_at(b, 8);
            r.w[4] = r.w[5] = r.w[6] = entity_bits_at(b, (int)offsetof(FootballState, radius));
            r.w[7] = entity_bits_of_int(b->kicks);
        } else if (i < h->num_rewards) {
            if (scen == SCN_HEX_MEMORY || scen == SCN_HEX_EXPLORE) {
                const HexRec *o = s.hex_objs + i;
                const int meta = o->meta;
                r.w[0] = entity_bits_of_int(seg_word(SEG_COLLECTABLE, i));
                r.w[1] = entity_bits_at(o, 0); r.w[2] = entity_bits_at(o, 4); r.w[3] = entity_bits_at(o, 8);
                r.w[4] = entity_bits_at(o, 16); r.w[5] = entity_bits_at(o, 20); r.w[6] = entity_bits_at(o, 24);
                r.w[7] = entity_bits_of_int((meta >> 8) & 1 ? 1 + (meta & 15) : 0);   // (alive ? 1 + shape : 0; `good`, bit 4, is not read)
            } else {
                const MovableObject o = s.rewards[i];
                r.w[0] = entity_bits_of_int(seg_word(scen == SCN_COLLECT && o.state == 2 ? SEG_HAZARD : SEG_COLLECTABLE, i));
                entity_voxel_cell(r, hv, o.x, o.y, o.z);
                r.w[7] = entity_bits_of_int(o.state);
            }
        }
    } else if (scen == SCN_TOWER) {
        r.w[0] = entity_bits_of_int(seg_word(SEG_BUILDING_ZONE, 0));
        entity_voxel_box(r, hv, h->bz[0], 0, h->bz[2], h->bz[1], 0, h->bz[3]);
        r.w[2] = entity_bits_of_float((ENTITY_BZ_Y0 + ENTITY_BZ_Y1) * 0.5f);
        r.w[5] = entity_bits_of_float((ENTITY_BZ_Y1 - ENTITY_BZ_Y0) * 0.5f);
        r.w[7] = entity_bits_at(h, (int)offsetof(EnvHeader, bz_reward));
    } else if (scen == SCN_OBSTACLES) {
        if (i < h->num_terrain) {
            const TerrainBox t = s.terrain[i];
            r.w[0] = entity_bits_of_int(seg_word(t.type == TERRAIN_EXIT ? SEG_EXIT : SEG_LAVA, i));
            entity_voxel_box(r, hv, t.min[0], t.min[1], t.min[2], t.max[0], t.max[1], t.max[2]);
            r.w[7] = entity_bits_of_int(t.type);
        }
    } else if (scen == SCN_REARRANGE) {
        if (i < h->num_terrain) {   // (Rearrange keeps its item count in num_terrain)
            const ArrangementItem it = s.items[i];
            r.w[0] = entity_bits_of_int(seg_word(SEG_TARGET, i));
            entity_voxel_cell(r, hv, it.off[0] + RE_LEFT_X, it.off[1] + RE_LEFT_Y, it.off[2] + RE_LEFT_Z);
            r.w[7] = entity_bits_of_int(it.shape);
        }
    }
    return r;
}

// Sokoban's compaction as a loop: the cell of the group's row k (the k-th SOKO_GOAL cell in ascending cell index), -1: the level has no more
__host__ __device__ inline int entity_soko_goal_of(const uint8_t *cells, int k)
{
    for (int c = 0; c < SOKO_DIM * SOKO_DIM; ++c)
        if (cells[c] == SOKO_GOAL && k-- == 0) return c;
    return -1;
}

// one env's E rows, on the host: the loops
__host__ __device__ inline void entity_obs_pack(const EntitySrc &s, uint32_t *out)
{
    const EntityLayout l = entity_layout(s.scenario, s.num_agents);
    for (int row = 0; row < l.total; ++row) {
        EntityRow r = entity_obs_row(s, l, row);
        if (s.scenario == SCN_SOKOBAN && row < l.base[ENTITY_OBJECTS]) {
            const int c = entity_soko_goal_of(s.soko, row);
            if (c >= 0) r = entity_soko_goal_row(c, s.hdr->W);
        }
        for (int f = 0; f < ENTITY_OBS_FLOATS; ++f) out[row * ENTITY_OBS_FLOATS + f] = r.w[f];
    }
}

}  // namespace mv
