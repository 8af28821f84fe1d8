// megaverse_amd/csrc/mv_hex_draw.h -- HexMemory's and HexExplore's episode generators as code that runs on the device (and, for the CPU test, on the host).
//
// Same episodes as mv_gen_hex.cpp (generate_hex_explore_episode, generate_hex_memory_episode), byte for byte over the record's header, the first num_agents
// spawn points and rotations, objs[:num_objs] and boxes[:num_boxes] (tests/test_hex_draw.py, tests/test_hex_draw_gpu.py).  This file restates THAT generator
// -- Honeycomb::lay_out and carve, draw_maze_look, build_maze_boxes, object_record, store -- with the std::vector / std::set members replaced by fixed arrays;
// what it stands for in the reference is listed there.
//
// The random stream is mt19937 through uniform_int_distribution, uniform_real_distribution<float> and std::shuffle; their restatements are mv_draw_common.h's
// (draw::Mt, mt_seed1, mt_below1, rand_range1, frand1, shuffle_walk), used unchanged.  The arithmetic is the host's, operation for operation: double where
// the host uses double, float where it rounds to float, in the host's order (the library is built with -ffp-contract=off); the corner offsets and SQRT3 are
// the same hex literals.  What is not an IEEE basic operation:
//   * sqrtf and float division go through double (sqrt_f, div_f): a double has more than 2 x 24 + 2 bits, so the second rounding changes nothing, and the
//     double forms are correctly rounded on both sides;
//   * floorf, ceilf, lround of an integral float, fabs: exact;
//   * sinf and cosf of the spawn circle (i * 2 pi / A) are NOT evaluated here -- the device's math library is not glibc's.  The launcher computes the
//     2 x MAX_AGENTS values on the host with the host generator's expressions (spawn_circle, mv_hex_draw.hip) and hands them over; the host twin uses the same
//     table.
//
// Execution model on the device: one wavefront per episode (mv_hex_draw.hip: hex_draw_kernel), four phases.
//   1. lay-out, ALL LANES: one cell per lane and round (at most 127 cells at size 7): the cell's centre and its wall list in the host's list ORDER, which is
//      computable per cell without the host's sequential push-backs -- the cell's own sides in side order where the far side is outside or a lower-numbered
//      cell, then its higher-numbered neighbours in ascending cell order (they pushed their side into this cell's list when their turn came).
//   2. carve, LANE 0: the inner-wall list in the host's order, shuffled on the Kruskal generator (seeded with the episode seed), union-find with the host's
//      path compression.  A knocked-down wall is a cleared STANDING bit on both cells' entries; the order of the others is what erase() leaves.
//   3. draws, LANE 0: the episode's stream in the host's order -- size, look, goal or the jittered places with their shuffle, colours and shapes, then the
//      walk over cells and walls: the omit draw (with the second chance an omitted inner wall gets from the other side: the host's `standing` set is the
//      EMITTED bit here), the landmark draw, the landmark count, per landmark its depth and colour.  The walk writes one WallRec per standing wall and NO
//      geometry.  Serial because every draw depends on the stream's position, which depends on every draw before it.
//   4. geometry and stores, ALL LANES: a wave prefix sum over the WallRecs gives every box its index AFTER the host's stable_partition -- the floor at 0, the
//      k-th standing wall at 1 + k, landmarks and edgings behind all colliders in walk order --, each lane computes its walls' boxes (frame by the dz / dx
//      rule, into_frame, half extents) and stores the 32-byte HexRecs straight into the record; the objects are spread over the lanes too.
//
// One generator state for two generators.  The host holds the episode's mt19937 and Kruskal's side by side; both are seeded with the episode seed, and the
// episode's has drawn one value (the size) when Kruskal's is made.  Here the one state in LDS is seeded, draws the size, is seeded AGAIN for the shuffle of
// the inner walls, and once more for the episode's stream, whose first draw (the size, again) is discarded: two more seedings for 2.5 KB less LDS per wave.
//
// Capacities.  A maze of size n has 3 n (n - 1) + 1 cells, 3 (3 n - 2) (n - 1) inner walls of which cells - 1 fall, 6 n^2 standing walls at most: 127, 342 and
// 294 at size 7, so 1 + 294 x (2 + 4) = 1765 boxes and 127 objects at most, inside HEX_MAX_BOXES and HEX_MAX_OBJS.  The stores still truncate exactly as
// store() does (the first HEX_MAX_BOXES of the partitioned order, num_colliders counted inside them) and raise the host's flags; every loop is bounded by one
// of these capacities, and a bound that is hit raises a flag and leaves the loop.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mv_draw_common.h"
#include "mv_gen.h"
#include "mv_types.h"

namespace mv {
namespace hdraw {

using namespace draw;

enum : int {
    MIN_SIZE = 2, MAX_SIZE = 7,   // rand_range(2, 8)
    MAX_CELLS = 3 * MAX_SIZE * (MAX_SIZE - 1) + 1,
    MAX_INNER = 3 * (3 * MAX_SIZE - 2) * (MAX_SIZE - 1),
    MAX_WALLS = 6 * MAX_SIZE * MAX_SIZE,
    MAX_LANDMARKS = 4,            // rand_range(2, 5)
    MAX_COLOR_DRAWS = 64,         // HexMemory's "another colour or shape" loop: each round repeats with probability 1 / 42
};
static_assert(MAX_CELLS == 127 && MAX_INNER == 342 && MAX_WALLS == 294, "the bounds DESIGN.md states");
static_assert(MAX_CELLS < 255, "a cell and 'outside' fit the low byte of a wall entry");
static_assert(1 + MAX_WALLS * (2 + MAX_LANDMARKS) <= HEX_MAX_BOXES && MAX_CELLS <= HEX_MAX_OBJS, "the largest maze fits the record");

// a cell's wall entry: what is on the far side, the side of the cell that OWNS the geometry (the cell whose turn pushed it), and two bits
enum : unsigned { OUTSIDE = 255u, E_OTHER = 255u, E_SIDE_SHIFT = 8, E_OWNER_IS_OTHER = 1u << 11, E_STANDING = 1u << 12, E_EMITTED = 1u << 13 };

struct WallRec {      // one standing wall as the walk decided it: 24 bytes
    uint16_t wall;    // owner cell << 3 | side
    uint8_t count;    // landmarks: 0, or 2 .. 4
    uint8_t pad;
    uint8_t colour[MAX_LANDMARKS];   // index into ALL_COLORS
    float depth[MAX_LANDMARKS];
};

struct Look {   // MazeLook
    float scale, wall_height, omit_walls, landmark_chance;
    unsigned bottom_edging, top_edging;
};

struct SpawnCircle { float sin_t[MAX_AGENTS], cos_t[MAX_AGENTS]; };   // sinf / cosf of float(i) * float(2 pi / A), evaluated on the host

struct Plan {   // what lane 0 leaves for the wave
    uint32_t seed;
    int size, cells, num_walls, num_boxes_drawn, num_objs_drawn;
    Look look;
    unsigned floor_color, good_color, bad_color;
    int good_shape, bad_shape, good_count;
    float target[3], landmark[3];
};

// scratch of one episode: LDS on the device, plain memory on the host
struct Scratch {
    uint32_t mt[624];
    double cx[MAX_CELLS], cy[MAX_CELLS];
    WallRec rec[MAX_WALLS + 1];      // (the last one takes the draws of a wall beyond the bound)
    float place[MAX_CELLS][2];       // HexMemory: the jittered spots' x and z (y is 0.5), shuffled
    uint16_t entry[MAX_CELLS][6];
    uint16_t inner[MAX_INNER];       // a | b << 8
    uint8_t entries[MAX_CELLS];
    uint8_t region[MAX_CELLS];       // union-find
    uint8_t order[MAX_CELLS];        // HexExplore: the shuffled cells
    Plan plan;
};

struct P3 { float x, y, z; };

MV_HD float sqrt_f(float v) { return (float)sqrt((double)v); }
MV_HD float div_f(float a, float b) { return (float)((double)a / (double)b); }

// the reference's colour lists, at file scope (constants of the code object on the device): a table inside a function would be a lane's own, and a lane's
// arrays are the compiler's to place
constexpr unsigned ALL_COLORS[22] = {0xffdd3c, 0x3bb372, 0x50c878, 0x2eb5d0, 0xadd8e6, 0x3a7fa6, 0x2c3e50, 0xffb400, 0xb3b3b3, 0x555555, 0x222222,
                                     0xffffff, 0xff0000, 0xffa770, 0xd468ee, 0xffe6e6, 0xffffe6, 0xccffcc, 0xe6ecff, 0xd9d9d9, 0xf2e6ff, 0xffebcc};   // env/include/env/const.hpp:58-83
constexpr unsigned OBJECT_COLORS[14] = {0xffdd3c, 0x3bb372, 0x50c878, 0x2eb5d0, 0xadd8e6, 0x3a7fa6, 0xffb400,
                                        0xb3b3b3, 0x555555, 0xffffff, 0xff0000, 0xffa770, 0xd468ee, 0xffe6e6};   // const.hpp:96-111
constexpr unsigned LAYOUT_COLORS[14] = {0xffffff, 0xffffe6, 0xccffcc, 0xe6ecff, 0xd9d9d9, 0xffebcc, 0xb3b3b3,
                                        0xb3b3b3, 0xb3b3b3, 0xb3b3b3, 0x555555, 0x555555, 0x555555, 0x555555};   // const.hpp:121-136
MV_HD unsigned all_color(int i) { return ALL_COLORS[i]; }
MV_HD unsigned object_color(int i) { return OBJECT_COLORS[i]; }
MV_HD unsigned layout_color(int i) { return LAYOUT_COLORS[i]; }

// ---- the honeycomb: cells (u, v) on a skewed grid, |u| < size, numbered row by row ----------------------------------------------------------------
MV_HD int num_cells(int size) { return 3 * size * (size - 1) + 1; }
MV_HD int first_v(int size, int u) { return u < 0 ? -size - u + 1 : -size + 1; }
MV_HD int last_v(int size, int u) { return u < 0 ? size - 1 : size - 1 - u; }
MV_HD bool inside(int size, int u, int v) { return u > -size && u < size && v >= first_v(size, u) && v <= last_v(size, u); }
MV_HD int cell_index(int size, int u, int v)
{
    return u <= 0 ? ((3 * size + u) * (size + u - 1)) / 2 + v : (3 * size * (size - 1) + (4 * size - u - 1) * u) / 2 + v;
}
// cell_index's inverse: the row whose numbers hold `cell` (at most 2 MAX_SIZE - 1 rows)
MV_HD void cell_uv(int size, int cell, int &u, int &v)
{
    for (u = -size + 1; u < size - 1; ++u)
        if (cell <= cell_index(size, u, last_v(size, u))) break;
    v = first_v(size, u) + (cell - cell_index(size, u, first_v(size, u)));
}
MV_HD int side_du(int side) { return side < 2 ? -1 : side == 2 || side == 5 ? 0 : 1; }    // STEP: {-1, 0}, {-1, 1}, {0, 1}, {1, 0}, {1, -1}, {0, -1}
MV_HD int side_dv(int side) { return side == 1 || side == 2 ? 1 : side == 0 || side == 3 ? 0 : -1; }

// phase 1, one cell: its centre and its wall list, every wall standing
MV_HD void lay_out_cell(Scratch &w, int size, int cell)
{
    const double SQRT3 = 0x1.bb67ae8584caap+0;
    int u, v;
    cell_uv(size, cell, u, v);
    w.cx[cell] = (SQRT3 / 2) * u + SQRT3 * v;
    w.cy[cell] = 1.5 * u + 0.0 * v;
    uint16_t *e = w.entry[cell];
    int n = 0;
    for (int side = 0; side < 6; ++side) {   // its own turn: the rim and the lower-numbered neighbours
        const int nu = u + side_du(side), nv = v + side_dv(side);
        unsigned other = OUTSIDE;
        if (inside(size, nu, nv)) {
            const int neighbour = cell_index(size, nu, nv);
            if (neighbour > cell) continue;
            other = (unsigned)neighbour;
        }
        e[n++] = (uint16_t)(other | ((unsigned)side << E_SIDE_SHIFT) | E_STANDING);
    }
    for (int last = cell, round = 0; round < 6; ++round) {   // the higher-numbered neighbours' turns, in the order they came
        int next = MAX_CELLS, nextSide = 0;
        for (int side = 0; side < 6; ++side) {
            const int nu = u + side_du(side), nv = v + side_dv(side);
            if (!inside(size, nu, nv)) continue;
            const int neighbour = cell_index(size, nu, nv);
            if (neighbour > last && neighbour < next) { next = neighbour; nextSide = (side + 3) % 6; }   // (the neighbour's side that faces this cell)
        }
        if (next == MAX_CELLS) break;
        e[n++] = (uint16_t)((unsigned)next | ((unsigned)nextSide << E_SIDE_SHIFT) | E_OWNER_IS_OTHER | E_STANDING);
        last = next;
    }
    w.entries[cell] = (uint8_t)n;
}

MV_HD void knock_down(Scratch &w, int cell, int other)
{
    uint16_t *e = w.entry[cell];
    for (int k = 0; k < (int)w.entries[cell]; ++k)
        if ((e[k] & E_OTHER) == (unsigned)other) { e[k] = (uint16_t)(e[k] & ~E_STANDING); return; }
}
MV_HD int find_region(Scratch &w, int cells, int c, int &flags)
{
    uint8_t *region = w.region;
    int r = c, steps = 0;
    for (; region[r] != r && steps < cells; ++steps) r = region[r];   // (a chain is no longer than the cell count)
    if (region[r] != r) flags |= FLAG_SLABS;
    for (steps = 0; region[c] != r && steps < cells; ++steps) { const int next = region[c]; region[c] = (uint8_t)r; c = next; }
    return r;
}
// phase 2 (serial): randomised Kruskal on the generator seeded with the episode seed.  Leaves `g` spent: the caller re-seeds it.
MV_HD void carve(Mt &g, Scratch &w, int cells, uint32_t seed, int &flags)
{
    uint16_t *inner = w.inner;
    int n = 0;
    for (int c = 0; c < cells; ++c)
        for (int k = 0; k < (int)w.entries[c]; ++k) {
            const int other = (int)(w.entry[c][k] & E_OTHER);
            if (other == (int)OUTSIDE || other <= c) continue;
            if (n >= MAX_INNER) { flags |= FLAG_SLABS; continue; }
            inner[n++] = (uint16_t)(c | (other << 8));
        }
    mt_seed1(g, seed);
    shuffle_walk(n, [&](uint32_t range) { return mt_below1(g, range); }, [&](int i, int j) { const uint16_t t = inner[i]; inner[i] = inner[j]; inner[j] = t; });
    for (int c = 0; c < cells; ++c) w.region[c] = (uint8_t)c;
    for (int i = 0; i < n; ++i) {
        const int a = inner[i] & 255, b = inner[i] >> 8;
        const int ra = find_region(w, cells, a, flags), rb = find_region(w, cells, b, flags);
        if (ra == rb) continue;
        w.region[ra] = (uint8_t)rb;
        knock_down(w, a, b);
        knock_down(w, b, a);
    }
}

// ---- phase 3 (serial): the draws --------------------------------------------------------------------------------------------------------------
MV_HD Look draw_look(Mt &g, float omit_min, float omit_max)
{
    Look k;
    k.scale = 3.5f;
    k.wall_height = frand1(g) * 0.55f + 0.85f;
    k.omit_walls = frand1(g) * (omit_max - omit_min) + omit_min;
    k.landmark_chance = frand1(g) * 0.15f + 0.15f;
    k.bottom_edging = all_color(rand_range1(g, 0, 22));
    k.top_edging = all_color(rand_range1(g, 0, 22));
    return k;
}

// build_maze_boxes' draws: the floor's colour, then the walk -- one WallRec per standing wall.  Leaves the box counts in the plan.
MV_HD void draw_walk(Mt &g, Scratch &w, int &flags)
{
    Plan &p = w.plan;
    const Look look = p.look;
    p.floor_color = layout_color(rand_range1(g, 0, 14));
    int walls = 0, others = 0;
    for (int cell = 0; cell < p.cells; ++cell)
        for (int k = 0; k < (int)w.entries[cell]; ++k) {
            const unsigned e = w.entry[cell][k];
            if (!(e & E_STANDING)) continue;
            const int other = (int)(e & E_OTHER);
            if (other != (int)OUTSIDE) {
                if (e & E_EMITTED) continue;                       // seen from the other side already
                if (frand1(g) < look.omit_walls) continue;        // randomly left out
                uint16_t *far = w.entry[other];
                for (int j = 0; j < (int)w.entries[other]; ++j)
                    if ((far[j] & E_OTHER) == (unsigned)cell) { far[j] = (uint16_t)(far[j] | E_EMITTED); break; }
            }
            WallRec &r = w.rec[walls < MAX_WALLS ? walls : MAX_WALLS];   // (written in place: a record on lane 0's stack would be moved to LDS behind DrawLds' back)
            r.wall = (uint16_t)((((e & E_OWNER_IS_OTHER) ? other : cell) << 3) | (int)((e >> E_SIDE_SHIFT) & 7u));
            r.count = 0; r.pad = 0;
            for (int i = 0; i < MAX_LANDMARKS; ++i) { r.colour[i] = 0; r.depth[i] = 0.0f; }
            if (frand1(g) < look.landmark_chance) {
                r.count = (uint8_t)rand_range1(g, 2, 5);
                for (int i = 0; i < (int)r.count; ++i) {
                    r.depth[i] = frand1(g) * 1.2f + 1.5f;
                    r.colour[i] = (uint8_t)rand_range1(g, 0, 22);
                }
            }
            if (walls >= MAX_WALLS) { flags |= FLAG_SLABS; continue; }   // (never: 6 size^2 walls stand at most; the draws went to the spare record)
            ++walls;
            others += (int)r.count + 1;
        }
    p.num_walls = walls;
    p.num_boxes_drawn = 1 + walls + others;
}

// store()'s counts and the capacity flags
MV_HD void store_counts(const Plan &p, HexBlob *out, int &flags)
{
    int nb = p.num_boxes_drawn, no = p.num_objs_drawn;
    if (nb > HEX_MAX_BOXES) { flags |= FLAG_SLABS; nb = HEX_MAX_BOXES; }
    if (no > HEX_MAX_OBJS) { flags |= FLAG_REWARDS; no = HEX_MAX_OBJS; }
    out->num_boxes = nb; out->num_objs = no;
    out->num_colliders = 1 + p.num_walls < nb ? 1 + p.num_walls : nb;   // (the partition put the colliders first)
}

// Env::reset's seed draw and the maze's size: what lane 0 does before the lay-out
MV_HD void draw_size(Mt &g, const GenState &st, Scratch &w)
{
    g.s = w.mt;
    uint32_t seed = st.seed;
    if (st.seed_is_env_seed) {   // Env::seed, then Env::reset: seed = randRange(0, 1 << 30, rng); rng.seed(seed)
        mt_seed1(g, seed);
        seed = (uint32_t)rand_range1(g, 0, 1 << 30);
    }
    mt_seed1(g, seed);
    Plan &p = w.plan;
    p.seed = seed;
    p.size = rand_range1(g, MIN_SIZE, MAX_SIZE + 1);
    p.cells = num_cells(p.size);
}

// HexExplore behind the carve.  `out` is zero on entry.  -> the value the env's NEXT Env::reset will draw for its seed
MV_HD uint32_t draw_explore(Mt &g, Scratch &w, const SpawnCircle &circle, int num_agents, float base_episode_len, HexBlob *out, int &flags)
{
    Plan &p = w.plan;
    mt_seed1(g, p.seed);
    (void)rand_range1(g, MIN_SIZE, MAX_SIZE + 1);   // (the size, drawn before the carve already)
    p.look = draw_look(g, 0.1f, 0.4f);
    const Look look = p.look;
    const int goal = rand_range1(g, 0, p.cells);
    const P3 target{float(w.cx[goal]) * look.scale, 0.0f, float(w.cy[goal]) * look.scale};
    p.target[0] = target.x; p.target[1] = target.y; p.target[2] = target.z;

    // agentStartingPositions: the first cell of a shuffled list that is further than `size` cells from the reward object, or the furthest met on the way
    uint8_t *order = w.order;
    for (int i = 0; i < p.cells; ++i) order[i] = (uint8_t)i;
    shuffle_walk(p.cells, [&](uint32_t range) { return mt_below1(g, range); }, [&](int i, int j) { const uint8_t t = order[i]; order[i] = order[j]; order[j] = t; });
    float furthest = 0;
    bool found = false;
    P3 best{0, 0, 0};
    for (int k = 0; k < p.cells; ++k) {
        const int cell = order[k];
        const P3 at{float(w.cx[cell]) * look.scale, 0.1f, float(w.cy[cell]) * look.scale};
        const float dx = target.x - at.x, dy = target.y - at.y, dz = target.z - at.z;
        const float distance = sqrt_f((dx * dx + dy * dy) + dz * dz);
        if (distance > furthest) { best = at; found = true; furthest = distance; }
        if (distance > float(p.size) * look.scale) break;
    }
    for (int i = 0; i < num_agents; ++i) {
        if (found) { out->spawn[i][0] = best.x + circle.sin_t[i]; out->spawn[i][1] = best.y + 0.0f; out->spawn[i][2] = best.z + circle.cos_t[i]; }
        else { out->spawn[i][0] = 0.0f; out->spawn[i][1] = 1.0f; out->spawn[i][2] = 0.0f; }
    }
    for (int i = 0; i < num_agents; ++i) out->yaw[i] = frand1(g) * 3.14159274f * 2;   // scenario_default.hpp:87

    draw_walk(g, w, flags);
    p.num_objs_drawn = 1;
    store_counts(p, out, flags);
    out->num_good = 0;
    out->target[0] = target.x; out->target[1] = target.z;
    out->episode_len = base_episode_len;
    return (uint32_t)rand_range1(g, 0, 1 << 30);
}

// HexMemory behind the carve
MV_HD uint32_t draw_memory(Mt &g, Scratch &w, const SpawnCircle &circle, int num_agents, float base_episode_len, HexBlob *out, int &flags)
{
    Plan &p = w.plan;
    mt_seed1(g, p.seed);
    (void)rand_range1(g, MIN_SIZE, MAX_SIZE + 1);
    p.look = draw_look(g, 0.1f, 0.95f);
    const Look look = p.look;

    int middle = 0;   // the cell closest to the centre
    float nearest = 1e9f;
    for (int cell = 0; cell < p.cells; ++cell) {
        const double d = sqrt(w.cx[cell] * w.cx[cell] + w.cy[cell] * w.cy[cell]);
        if (d < nearest) { middle = cell; nearest = float(d); }
    }
    p.landmark[0] = float(w.cx[middle] * look.scale); p.landmark[1] = 1.0f; p.landmark[2] = float(w.cy[middle] * look.scale);

    int places = 0;   // one candidate spot per other cell, jittered
    for (int cell = 0; cell < p.cells; ++cell) {
        if (cell == middle) continue;
        const float jz = frand1(g) - 0.5f;
        const float jx = frand1(g) - 0.5f;
        const float x = float(w.cx[cell]) + jx, z = float(w.cy[cell]) + jz;
        w.place[places][0] = x * look.scale; w.place[places][1] = z * look.scale;
        ++places;
    }
    float(*place)[2] = w.place;
    shuffle_walk(places, [&](uint32_t range) { return mt_below1(g, range); }, [&](int i, int j) {
        const float x = place[i][0], z = place[i][1];
        place[i][0] = place[j][0]; place[i][1] = place[j][1];
        place[j][0] = x; place[j][1] = z;
    });
    const float fraction = frand1(g) * 0.25f + 0.2f;
    const int goodCount = (int)ceilf(fraction * float(places));   // lround(ceil(.)): the value is integral
    // (the `: 0` arm is the host's, carried over and NOT reached by any test: goodCount <= ceil(0.45 places) <= places / 2 for every places a maze can have --
    // 6, 18, 36, 60, 90, 126 -- so it is dead in mv_gen_hex.cpp too)
    const int badCount = places >= 2 * goodCount ? goodCount : 0;

    const float turn = float(2 * M_PI / num_agents);   // spawnAgents: a circle of radius 1.5 around the origin, everybody facing along their own angle
    for (int i = 0; i < num_agents; ++i) {
        out->spawn[i][0] = 1.5f * circle.sin_t[i]; out->spawn[i][1] = 1.5f * 0.3f; out->spawn[i][2] = 1.5f * circle.cos_t[i];
        out->yaw[i] = turn * float(i);
    }

    const int goodColor = rand_range1(g, 0, 14);
    p.good_shape = rand_range1(g, 0, 3);
    int badColor = goodColor;
    p.bad_shape = p.good_shape;
    for (int round = 0; badColor == goodColor && p.bad_shape == p.good_shape; ++round) {
        if (round >= MAX_COLOR_DRAWS) { flags |= FLAG_REWARDS; break; }
        badColor = rand_range1(g, 0, 14);
        p.bad_shape = rand_range1(g, 0, 3);
    }
    p.good_color = object_color(goodColor); p.bad_color = object_color(badColor);
    p.good_count = goodCount;

    draw_walk(g, w, flags);
    p.num_objs_drawn = 1 + goodCount + badCount;
    store_counts(p, out, flags);
    out->num_good = goodCount;
    out->episode_len = base_episode_len + 3.0f * float(goodCount);   // scenario_hex_memory.hpp:45-49
    return (uint32_t)rand_range1(g, 0, 1 << 30);
}

// ---- phase 4: geometry ----------------------------------------------------------------------------------------------------------------------------
// (cos, sin) of the three directions a border of a honeycomb can have once rotateY(-atan(dz / dx)) is applied: +30, -30, 90 degrees
MV_HD float frame_cos(int k) { return k == 2 ? 0.0f : 0.8660254f; }
MV_HD float frame_sin(int k) { return k == 0 ? 0.5f : k == 1 ? -0.5f : 1.0f; }
MV_HD P3 into_frame(int k, P3 p) { return P3{frame_cos(k) * p.x - frame_sin(k) * p.z, p.y, frame_sin(k) * p.x + frame_cos(k) * p.z}; }

MV_HD HexRec box_record(int frame, bool collide, P3 centre, P3 half, unsigned color)
{
    HexRec r;
    r.a[0] = centre.x - half.x; r.a[1] = centre.y - half.y; r.a[2] = centre.z - half.z;
    r.b[0] = centre.x + half.x; r.b[1] = centre.y + half.y; r.b[2] = centre.z + half.z;
    r.meta = (frame + 1) | (collide ? 16 : 0);
    r.color = int32_t(color);
    return r;
}
MV_HD void put_box(HexBlob *out, int index, const HexRec &r) { if (index >= 0 && index < HEX_MAX_BOXES) out->boxes[index] = r; }

MV_HD void floor_box(const Plan &p, HexBlob *out)
{
    const double SQRT3 = 0x1.bb67ae8584caap+0;
    const double s = p.look.scale, halfWidth = SQRT3 * (p.size - 0.5), halfHeight = 1.5 * p.size - 0.5;
    const double x_min = -halfWidth * s, x_max = halfWidth * s, y_min = -halfHeight * s, y_max = halfHeight * s;
    const P3 half{float(x_max - x_min), 0.0001f, float(y_max - y_min)};   // addStaticCollidingBox: the cube [-1, 1]^3 scaled, i.e. twice the maze
    const P3 centre{float(x_max + x_min) / 2, 0.0f, float(y_max + y_min) / 2};
    put_box(out, 0, box_record(-1, true, centre, half, p.floor_color));
}

// corner offsets of side 0 .. 5: cos / sin of (n - 2.5) pi / 3 and of (n - 1.5) pi / 3 as the reference's build evaluates them (mv_gen_hex.cpp), as literals;
// switches, not arrays inside the functions: a lane's own arrays are the compiler's to place, LDS behind DrawLds' back included
MV_HD double from_x(int side)
{
    switch (side) {
        case 0: case 5: return -0x1.bb67ae8584cabp-1;
        case 1: case 4: return 0x1.1a62633145c07p-54;
        default: return 0x1.bb67ae8584cabp-1;
    }
}
MV_HD double from_y(int side)
{
    switch (side) {
        case 0: case 2: return -0x1.fffffffffffffp-2;
        case 1: return -0x1.0000000000000p+0;
        case 4: return 0x1.0000000000000p+0;
        default: return 0x1.fffffffffffffp-2;
    }
}
MV_HD double to_x(int side)
{
    switch (side) {
        case 0: return -0x1.72cece675d1fcp-53;
        case 1: return 0x1.bb67ae8584caap-1;
        case 2: return 0x1.bb67ae8584cabp-1;
        case 3: return 0x1.1a62633145c07p-54;
        case 4: return -0x1.bb67ae8584ca9p-1;
        default: return -0x1.bb67ae8584caap-1;
    }
}
MV_HD double to_y(int side)
{
    switch (side) {
        case 0: return -0x1.0000000000000p+0;
        case 1: return -0x1.0000000000000p-1;
        case 2: return 0x1.fffffffffffffp-2;
        case 3: return 0x1.0000000000000p+0;
        case 4: return 0x1.0000000000003p-1;
        default: return -0x1.0000000000001p-1;
    }
}

// the boxes of standing wall k: the wall at 1 + k, its landmarks and its edging from `first` on (behind every collider, in walk order)
MV_HD void wall_boxes(const Scratch &w, int k, int first, HexBlob *out)
{
    const Look &look = w.plan.look;
    const WallRec &r = w.rec[k];
    const int owner = r.wall >> 3, side = r.wall & 7;
    const double x = w.cx[owner], y = w.cy[owner];
    const double ax = x + from_x(side), ay = y + from_y(side), bx = x + to_x(side), by = y + to_y(side);
    const double s = look.scale;
    const double x1 = ax * s, z1 = ay * s, x2 = bx * s, z2 = by * s;
    const float length = 0.5f * sqrt_f(float((x1 - x2) * (x1 - x2) + (z1 - z2) * (z1 - z2)));
    const P3 mid{float(x1 + x2) / 2, look.wall_height, float(z1 + z2) / 2};
    const double dx = x1 - x2, dz = z1 - z2;
    const int frame = fabs(dx) > 1e-5f ? ((dz / dx) < 0 ? 0 : 1) : 2;   // EPSILON, util/macro.hpp:12
    const P3 centre = into_frame(frame, mid);
    const float lw = 0.15f, lh = div_f(lw * length, look.wall_height);
    for (int i = 0; i < (int)r.count && i < MAX_LANDMARKS; ++i) {
        const float tx = float(i % 2 == 1) * lw * 2, ty = float(i > 1) * lh * 2 - 0.2f;
        const P3 c{centre.x + length * tx, centre.y + look.wall_height * ty, centre.z};
        const P3 h{length * lw, look.wall_height * lh, 0.15f * r.depth[i]};
        put_box(out, first + i, box_record(frame, false, c, h, all_color(r.colour[i])));
    }
    put_box(out, 1 + k, box_record(frame, true, centre, P3{length, look.wall_height, 0.15f}, 0x3a7fa6));   // DARK_BLUE
    const P3 eh{length * 1.02f, look.wall_height * 0.12f, 0.2f};
    put_box(out, first + (int)r.count, box_record(frame, false, into_frame(frame, P3{mid.x, eh.y, mid.z}), eh, look.bottom_edging));
}

MV_HD HexRec object_record(int shape, unsigned color, P3 at, P3 scale, bool good, bool alive, P3 grid)
{
    HexRec r;
    r.a[0] = at.x; r.a[1] = at.y; r.a[2] = at.z;
    r.b[0] = scale.x; r.b[1] = scale.y; r.b[2] = scale.z;
    const int vx = (int)floorf(grid.x), vz = (int)floorf(grid.z);   // lround(floor(.))
    r.meta = shape | (good ? 16 : 0) | (alive ? 256 : 0) | (((vx + 128) & 255) << 12) | (((vz + 128) & 255) << 20);
    r.color = int32_t(color);
    return r;
}
MV_HD P3 scale_of(int shape)
{
    return shape == HEX_SPHERE ? P3{0.75f, 0.75f, 0.75f} : shape == HEX_PILLAR ? P3{0.5f, 2.0f, 0.5f} : P3{0.17f * 2.2f, 0.45f * 2.2f, 0.17f * 2.2f};
}
MV_HD P3 shift_of(int shape) { return shape == HEX_SPHERE ? P3{0.5f, 0.1f, 0.5f} : shape == HEX_PILLAR ? P3{0.5f, 0.05f, 0.5f} : P3{0.5f, 0.6f, 0.5f}; }

// object i of the episode (i < min(num_objs_drawn, HEX_MAX_OBJS))
MV_HD void put_object(const Scratch &w, bool memory, int i, HexBlob *out)
{
    const Plan &p = w.plan;
    if (i < 0 || i >= HEX_MAX_OBJS) return;
    if (!memory) {   // the reward object: a VIOLET diamond above the goal cell
        const float sc = 1.9f;
        const P3 t{p.target[0], p.target[1], p.target[2]};
        out->objs[i] = object_record(HEX_DIAMOND, 0xd468ee, P3{t.x + 0.0f, t.y + 1.2f, t.z + 0.0f}, P3{0.17f * sc, 0.35f * sc, 0.17f * sc}, true, true, t);
        return;
    }
    if (i == 0) {   // the object in the middle cell shows what to collect; it cannot be collected itself
        const P3 landmark{p.landmark[0], p.landmark[1], p.landmark[2]}, sh = shift_of(p.good_shape);
        out->objs[0] = object_record(p.good_shape, p.good_color, P3{landmark.x + sh.x, landmark.y + sh.y, landmark.z + sh.z}, scale_of(p.good_shape), true, false, landmark);
        return;
    }
    const float shrink = 0.6f;
    const bool good = i - 1 < p.good_count;
    const int shape = good ? p.good_shape : p.bad_shape;
    const P3 sh = shift_of(shape), sc = scale_of(shape), at{w.place[i - 1][0], 0.5f + 0.0f, w.place[i - 1][1]};
    out->objs[i] = object_record(shape, good ? p.good_color : p.bad_color, P3{at.x + sh.x * shrink, at.y + sh.y * shrink, at.z + sh.z * shrink},
                                 P3{sc.x * shrink, sc.y * shrink, sc.z * shrink}, good, true, at);
}

}  // namespace hdraw
}  // namespace mv
