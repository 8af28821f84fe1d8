// megaverse_amd/csrc/mv_obstacles_draw.h -- the Obstacles family's and Empty's episode generators as code that runs on the device (and, for the CPU test, on
// the host).
//
// Same episodes as mv_gen_obstacles.cpp (generate_obstacles_episode, generate_empty_episode), byte for byte (tests/test_obstacles_draw.py,
// tests/test_obstacles_draw_gpu.py).  This file restates THAT generator -- its platform classes, rigid motions, voxel paint, greedy merge, spawn cells and
// object scatter -- with the std::vector / std::map / std::set members replaced by fixed arrays; what it stands for in the reference is listed there.
//
// The random stream is mt19937 through uniform_int_distribution and uniform_real_distribution<float>; their restatements are mv_collect_draw.h's (cdraw::Mt,
// mt_seed1, mt_next1, rand_range1, frand1), used unchanged.  The one library algorithm restated here and not there:
//   * std::lround(float), round half AWAY from zero on both sides of zero: lround_half_away below.  floor(v + 0.5f) in float is not it -- 0.49999997f + 0.5f
//     rounds to 1.0f -- so the sum is taken in double, where it is exact for every float below 2^29.
// Everything else is integer arithmetic; the three float expressions of the generator (frand * 0.5f, fraction * float(share), the episode length) keep the
// host's operation order and the library is built with -ffp-contract=off.
//
// Execution model on the device: one wavefront per episode (mv_obstacles_draw.hip: obstacles_draw_kernel).  Everything that consumes the random stream -- the
// seed draw and re-seed, draw_walls, the up-to-20 attempts of the chain with every platform's roll / build and the `hardest` redraw loop, corners, the goal,
// the pairwise hull clash test, colours, spawn cells, box shares, the scatter of movable boxes and reward objects, yaw_frand -- is serial by nature and runs on
// LANE 0 ALONE, on a chain of at most MAX_CHAIN platforms in LDS.  The paint over the level's bounding box and the greedy merge are spread over the 64 lanes
// (draw_slabs_wave); the serial form below (draw_slabs_serial) is the host's, and what the tests hold the wave form against.
//
// The grid.  Only three cell values occur -- empty, floor, wall -- so the grid is two BIT PLANES (floor, wall) over cells numbered (y nz + z) nx + x, the
// merge's scan order; a cell the merge has covered is cleared from its plane (the planes are disjoint and a merge pass looks at one plane, so "covered" needs
// no plane of its own).  The bound on its size, from the largest configuration scenario_from_name returns (LARGEST_* below):
//   * a chain has at most 2 max_platforms + 2 members (start, goal, and a corner beside every platform): MAX_CHAIN = 16;
//   * a member's footprint is at most MAX_LEN x MAX_WIDTH = 11 x 8 (lava platforms are the longest: rand_range(6, 12); widths: rand_range(5, 9); a corner is
//     (width - 1) x width), and the members' footprints form a connected set, so the bounding box's two horizontal sides TOGETHER are at most
//     MAX_CHAIN (MAX_LEN + MAX_WIDTH) = 304 and their product at most 152 x 152;
//   * only step platforms raise the anchor, by step_h <= max_height each, and a member is at most max_height + 5 high (a wall platform:
//     rand_range(wall_h + 4, wall_h + 6)): ny <= 7 x 4 + 9 = 37.
// GRID_CELLS = 152 x 152 x 37 = 854 848 cells, two planes of 26 714 words: 213 712 bytes per episode being drawn -- more than LDS holds, so every wave of a
// draw launch owns a region of device memory that the feeder allocates once (EpisodeFeeder: DRAW_REGIONS of them, counted in mv_arena_bytes).  Levels are far
// smaller than the bound (the host generator's comment speaks of 10^5 cells, a long straight ObstaclesHard level); the kernel still checks the level's own
// size against GRID_CELLS before it touches the region.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mv_collect_draw.h"
#include "mv_gen.h"
#include "mv_types.h"

namespace mv {
namespace odraw {

using cdraw::frand1;
using cdraw::GenState;
using cdraw::Mt;
using cdraw::mt_seed1;
using cdraw::rand_range1;

// the largest ObstacleConfig scenario_from_name returns, from the table it reads (mv_gen.h: kObstaclePresets -- ObstaclesHard: 7 platforms, heights up to 4);
// a gym's float parameters can ask for more: config_fits below is checked where a config arrives
enum : int { LARGEST_PLATFORMS = largest_preset_platforms(), LARGEST_HEIGHT = largest_preset_height() };
enum : int {
    MAX_CHAIN = 2 * LARGEST_PLATFORMS + 2,
    MAX_LEN = 11, MAX_WIDTH = 8,   // rand_range(6, 12) - 1 of a lava platform; rand_range(5, 9) - 1
    MAX_FLOOR_BOXES = 3, MAX_WALL_BOXES = 4,
    GRID_SIDES = MAX_CHAIN * (MAX_LEN + MAX_WIDTH),
    GRID_NY = LARGEST_PLATFORMS * LARGEST_HEIGHT + LARGEST_HEIGHT + 5,
    GRID_CELLS = (GRID_SIDES / 2) * (GRID_SIDES - GRID_SIDES / 2) * GRID_NY,
    PLANE_WORDS = (GRID_CELLS + 31) / 32,
    GRID_WORDS = 2 * PLANE_WORDS,   // one episode's region: the floor plane, then the wall plane
    DRAW_REGIONS = 256,             // episodes a launch draws at a time (one wave each; a launch of more episodes has its waves draw several, one after the other)
};
static_assert(LARGEST_PLATFORMS == 7 && LARGEST_HEIGHT == 4, "a registered scenario grew: the chain, the grid bound and DESIGN.md 3.2 follow from these two");
static_assert(MAX_CHAIN >= 2 * largest_preset_platforms() + 2, "a chain: start, goal, and a corner beside every platform");
static_assert(MAX_CHAIN == 16 && GRID_SIDES == 304 && GRID_NY == 37 && GRID_CELLS == 854848, "the bounds DESIGN.md 3.2 states");
static_assert(MAX_CHAIN <= 64, "the hull clash test and the share table index chain members with small integers");
static_assert(MAX_CHAIN * MAX_FLOOR_BOXES + MAX_CHAIN * MAX_WALL_BOXES < 256, "a level's painted boxes");
enum : int { FLAG_SLABS = GEN_SLABS, FLAG_TERRAIN = GEN_TERRAIN, FLAG_OBJECTS = GEN_OBJECTS, FLAG_REWARDS = GEN_REWARDS, FLAG_COORDS = GEN_COORDS };

MV_HD bool config_fits(const ObstacleConfig &c)
{
    return c.min_platforms >= 0 && c.max_platforms >= c.min_platforms && c.max_platforms <= LARGEST_PLATFORMS && c.min_height >= 1 && c.max_height >= c.min_height &&
           c.max_height <= LARGEST_HEIGHT && c.num_platform_types >= 1 && c.num_platform_types <= 4;
}

struct Int3 { int x, y, z; };
struct Rigid { int k; Int3 off; };   // q = rot^k(p) + off, rot = quarter turn about +Y: (x, y, z) -> (z, y, -x)
struct Aabb { Int3 lo, hi; };

enum Kind : int { K_EMPTY, K_WALL, K_LAVA, K_STEP, K_GAP, K_START, K_EXIT, K_TRANSITION };
enum : int { SOUTH = 1, NORTH = 2, WEST = 4, EAST = 8 };

struct Plat {   // plain data: it lives in LDS
    int kind, walls, length, height, width;
    Rigid parent, own, root;
    int anchor_rise, num_floor, num_wall, terrain_type;   // terrain_type 0: no terrain box (a platform has at most one)
    int wall_h, lava_len, step_h, gap, gap_x;
    Aabb floor[MAX_FLOOR_BOXES], wall[MAX_WALL_BOXES], terrain, hull;
    uint8_t occ[MAX_LEN][MAX_WIDTH];   // occupancy[{x, z}]; absent keys read 0
};

struct Level {   // what lane 0 leaves for the wave
    Int3 lo;
    int nx, ny, nz, draw_walls, members;
};

// scratch of one episode: LDS on the device, plain memory on the host
struct Scratch {
    uint32_t mt[624];
    Plat chain[MAX_CHAIN];
    Plat roll;                            // the platform being drawn (the `hardest` redraw loop draws it again and again)
    uint8_t taken[MAX_LEN][MAX_WIDTH];    // spawn cells already given out
    int share[MAX_CHAIN];
    Level level;
};

struct Stats { int attempts, left_turns, right_turns; };   // (test hook) of the episode drawn last

// ---- rigid motions ----------------------------------------------------------------------------------------------------------------------------
MV_HD Int3 turn(int k, Int3 p)
{
    switch (k & 3) {
        case 1: return Int3{p.z, p.y, -p.x};
        case 2: return Int3{-p.x, p.y, -p.z};
        case 3: return Int3{-p.z, p.y, p.x};
        default: return p;
    }
}
MV_HD Int3 rmap(const Rigid &r, Int3 p) { const Int3 t = turn(r.k, p); return Int3{t.x + r.off.x, t.y + r.off.y, t.z + r.off.z}; }
MV_HD Rigid then(const Rigid &outer, const Rigid &inner) { return Rigid{(outer.k + inner.k) & 3, rmap(outer, inner.off)}; }
MV_HD Rigid rotate_then_shift(int quarters, Int3 v) { return Rigid{quarters & 3, turn(quarters, v)}; }
MV_HD int imin(int a, int b) { return a < b ? a : b; }
MV_HD int imax(int a, int b) { return a > b ? a : b; }
MV_HD Aabb placed(const Rigid &root, const Aabb &local)
{
    const Int3 a = rmap(root, local.lo), b = rmap(root, local.hi);
    return Aabb{{imin(a.x, b.x), imin(a.y, b.y), imin(a.z, b.z)}, {imax(a.x, b.x), imax(a.y, b.y), imax(a.z, b.z)}};
}
MV_HD bool overlap(const Aabb &a, const Aabb &b)
{
    return !(a.hi.x <= b.lo.x || a.lo.x >= b.hi.x || a.hi.y <= b.lo.y || a.lo.y >= b.hi.y || a.hi.z <= b.lo.z || a.lo.z >= b.hi.z);
}
// std::lround of a float: half away from zero, whatever the sign
MV_HD int lround_half_away(float v)
{
    const double d = (double)v;
    return d >= 0.0 ? (int)floor(d + 0.5) : -(int)floor(-d + 0.5);
}

// ---- a platform ----------------------------------------------------------------------------------------------------------------------------------
MV_HD void plat_init(Plat &p, int kind, int walls, int width)
{   // Platform(): everything zero, width -1, identity motions
    p.kind = kind; p.walls = walls; p.length = 0; p.height = 0; p.width = width;
    p.parent = Rigid{0, {0, 0, 0}}; p.own = p.parent; p.root = p.parent;
    p.anchor_rise = 0; p.num_floor = 0; p.num_wall = 0; p.terrain_type = 0;
    p.wall_h = 0; p.lava_len = 0; p.step_h = 0; p.gap = 0; p.gap_x = 0;
}
MV_HD void plat_place(Plat &p) { p.root = then(p.parent, p.own); }
MV_HD Rigid plat_next_anchor(const Plat &p) { return then(p.root, rotate_then_shift(0, Int3{p.length, p.anchor_rise, 0})); }

MV_HD void plat_roll(Plat &p, Mt &g, const ObstacleConfig &c)
{   // the init() chain of the platform classes
    if (p.kind == K_TRANSITION) { p.height = 5; return; }
    p.length = rand_range1(g, 4, 10);
    if (p.width == -1) p.width = rand_range1(g, 5, 9);
    p.height = 5;
    switch (p.kind) {
        case K_WALL:
            p.wall_h = rand_range1(g, c.min_height, c.max_height + 1);
            p.height = rand_range1(g, p.wall_h + 4, p.wall_h + 6);
            break;
        case K_LAVA: {
            p.length = rand_range1(g, 6, 12);
            const int lo = imin(c.min_lava, p.length - 2), hi = imin(c.max_lava + 1, p.length - 1);
            p.lava_len = rand_range1(g, lo, hi);
            break;
        }
        case K_STEP:
            p.step_h = rand_range1(g, c.min_height, c.max_height + 1);
            p.height = rand_range1(g, p.step_h + 2, p.step_h + 5);
            break;
        case K_GAP:
            p.gap = rand_range1(g, c.min_gap, imin(c.max_gap + 1, p.length - 1));
            p.gap_x = rand_range1(g, 1, p.length - p.gap);
            break;
        default: break;
    }
}
MV_HD void plat_floor(Plat &p, const Aabb &b) { if (p.num_floor < MAX_FLOOR_BOXES) p.floor[p.num_floor++] = b; }
MV_HD void plat_side_walls(Plat &p)
{
    const int L = p.length, H = p.height, W = p.width;
    if (p.walls & SOUTH) p.wall[p.num_wall++] = Aabb{{0, 0, 0}, {1, H, W}};
    if (p.walls & NORTH) p.wall[p.num_wall++] = Aabb{{L - 1, 0, 0}, {L, H, W}};
    if (p.walls & EAST) p.wall[p.num_wall++] = Aabb{{0, 0, 0}, {L, H, 1}};
    if (p.walls & WEST) p.wall[p.num_wall++] = Aabb{{0, 0, W - 1}, {L, H, W}};
}
MV_HD bool occ_inside(int x, int z) { return x >= 0 && x < MAX_LEN && z >= 0 && z < MAX_WIDTH; }
MV_HD void plat_build(Plat &p, Mt &g)
{   // the generate() chain
    for (int x = 0; x < MAX_LEN; ++x)
        for (int z = 0; z < MAX_WIDTH; ++z) p.occ[x][z] = 0;
    const int L = p.length, W = p.width;
    if (p.kind == K_STEP) {
        const int sx = rand_range1(g, 1, L);
        plat_floor(p, Aabb{{0, 0, 0}, {sx + 1, 1, W}});
        plat_floor(p, Aabb{{sx, p.step_h, 0}, {L, p.step_h + 1, W}});
        plat_floor(p, Aabb{{sx, 0, 0}, {sx + 1, p.step_h + 1, W}});
        p.anchor_rise = p.step_h;
        plat_side_walls(p);
        for (int x = sx + 1; x < L; ++x)
            for (int z = 1; z < W; ++z)
                if (occ_inside(x, z)) p.occ[x][z] = (uint8_t)p.step_h;
        return;
    }
    if (p.kind == K_GAP) {
        plat_floor(p, Aabb{{0, 0, 0}, {p.gap_x, 1, W}});
        plat_floor(p, Aabb{{p.gap_x + p.gap, 0, 0}, {L, 1, W}});
        plat_side_walls(p);
        return;
    }
    plat_floor(p, Aabb{{0, 0, 0}, {L, 1, W}});
    plat_side_walls(p);
    if (p.kind == K_WALL) {
        const int wx = rand_range1(g, 1, L);
        const int thick = rand_range1(g, 1, L - wx + 1);
        plat_floor(p, Aabb{{wx, 1, 1}, {wx + thick, 1 + p.wall_h, W - 1}});
        for (int x = wx; x < wx + thick; ++x)
            for (int z = 1; z < W; ++z)
                if (occ_inside(x, z)) p.occ[x][z] = (uint8_t)p.wall_h;
    } else if (p.kind == K_LAVA) {
        const int lx = rand_range1(g, 1, L - p.lava_len);
        p.terrain_type = TERRAIN_LAVA;
        p.terrain = Aabb{{lx, 1, 1}, {lx + p.lava_len, 2, W - 1}};
    } else if (p.kind == K_EXIT) {
        p.terrain_type = TERRAIN_EXIT;
        p.terrain = Aabb{{L - 3, 1, 1}, {L - 1, 3, W - 1}};
    }
}
MV_HD bool plat_hardest(const Plat &p, const ObstacleConfig &c)
{
    return (p.kind == K_WALL && p.wall_h >= c.max_height) || (p.kind == K_LAVA && p.lava_len >= c.max_lava) || (p.kind == K_STEP && p.step_h >= c.max_height);
}
MV_HD int tri(int n) { return n * (n + 1) / 2; }
MV_HD int plat_boxes_needed(const Plat &p)
{
    switch (p.kind) {
        case K_WALL: return tri(p.wall_h - 1);
        case K_LAVA: return imax(1, p.lava_len - 1);
        case K_STEP: return tri(p.step_h - 1);
        case K_GAP: return tri(imax(0, p.gap - 2));
        default: return 0;
    }
}
MV_HD void plat_hull(Plat &p)
{   // of the floor and wall boxes as placed (every platform has a floor box)
    Aabb h{{0, 0, 0}, {0, 0, 0}};
    bool first = true;
    for (int i = 0; i < p.num_floor + p.num_wall; ++i) {
        const Aabb b = placed(p.root, i < p.num_floor ? p.floor[i] : p.wall[i - p.num_floor]);
        if (first) { h = b; first = false; continue; }
        h.lo = Int3{imin(h.lo.x, b.lo.x), imin(h.lo.y, b.lo.y), imin(h.lo.z, b.lo.z)};
        h.hi = Int3{imax(h.hi.x, b.hi.x), imax(h.hi.y, b.hi.y), imax(h.hi.z, b.hi.z)};
    }
    p.hull = h;
}
MV_HD int half_floor(int v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); }
// voxel whose centre is the image of the local voxel centre (doubled coordinates; the offset is applied once too many, as the host generator has it)
MV_HD Int3 plat_to_world_voxel(const Plat &p, int x, int y, int z)
{
    const Int3 c2 = rmap(p.root, Int3{2 * x + 1, 2 * y + 1, 2 * z + 1});
    const Int3 t = p.root.off;
    return Int3{half_floor(c2.x + t.x), half_floor(c2.y + t.y), half_floor(c2.z + t.z)};
}
MV_HD int occ_bump(Plat &p, int x, int z) { return occ_inside(x, z) ? (int)++p.occ[x][z] : 1; }
// `n` cells of the platform, each passed to put(world voxel) in the order they are drawn
template <class Put>
MV_HD void plat_scatter(Plat &p, int n, Mt &g, Put put)
{
    if (p.kind == K_GAP) {
        // candidates in (x, z) order: x outside the gap, z in 1 .. width - 2; the k-th of them is found by counting, not from a list
        const int perX = p.width - 2, cand = (p.length - p.gap) * perX;
        for (int i = 0; i < n; ++i) {
            const int k = rand_range1(g, 0, cand);
            int x = k / perX;
            const int z = 1 + k % perX;
            if (x >= p.gap_x) x += p.gap;
            put(plat_to_world_voxel(p, x, occ_bump(p, x, z), z));
        }
        return;
    }
    for (int i = 0; i < n; ++i)
        for (int attempt = 0; attempt < 10; ++attempt) {
            const int x = rand_range1(g, 1, p.length - 1);
            const int z = rand_range1(g, 1, p.width - 1);
            if ((occ_inside(x, z) ? p.occ[x][z] : 0) < 2 || attempt >= 9) {
                put(plat_to_world_voxel(p, x, occ_bump(p, x, z), z));
                break;
            }
        }
}

// ---- the episode, in three parts ---------------------------------------------------------------------------------------------------------------
// head (serial): Env::reset's seed draw, draw_walls, the chain, the colours; the record's scalar fields and the level's bounding box
MV_HD void draw_chain(Mt &g, const GenState &st, const ObstacleConfig &cfg, Scratch &w, EpisodeBlob *out, Stats *stats = nullptr)
{
    g.s = w.mt;
    uint32_t seed = st.seed;
    if (st.seed_is_env_seed) {   // Env::seed, then Env::reset: seed = randRange(0, 1 << 30, rng); rng.seed(seed)
        mt_seed1(g, seed);
        seed = (uint32_t)rand_range1(g, 0, 1 << 30);
    }
    mt_seed1(g, seed);
    const bool drawWalls = rand_range1(g, 0, 2) != 0;
    Plat *chain = w.chain;
    Plat &p = w.roll;
    int members = 0, numPlatforms = 0, attempts = 0, lefts = 0, rights = 0;
    for (int attempt = 0; attempt < 20; ++attempt) {
        ++attempts; lefts = 0; rights = 0;
        members = 0;
        numPlatforms = rand_range1(g, cfg.min_platforms, cfg.max_platforms + 1);
        {
            Plat &first = chain[members++];
            plat_init(first, K_START, SOUTH | EAST | WEST, -1);
            plat_roll(first, g, cfg); plat_place(first); plat_build(first, g);
        }
        int wantWidth = chain[0].width, last = 0, hardestSoFar = 0;
        for (int i = 0; i < numPlatforms && members + 3 <= MAX_CHAIN; ++i) {
            const int turnDraw = rand_range1(g, 0, 3);   // 0 straight, 1 left, 2 right
            if (turnDraw != 0) wantWidth = -1;
            if (turnDraw == 1) ++lefts;
            if (turnDraw == 2) ++rights;
            for (bool drawn = false; !drawn || (plat_hardest(p, cfg) && hardestSoFar >= cfg.num_allowed_max_difficulty); drawn = true) {
                plat_init(p, cfg.platform_types[rand_range1(g, 0, cfg.num_platform_types)], WEST | EAST, wantWidth);
                plat_roll(p, g, cfg);
            }
            if (plat_hardest(p, cfg)) ++hardestSoFar;
            p.parent = plat_next_anchor(chain[last]);
            plat_build(p, g);
            if (turnDraw == 1) p.own = rotate_then_shift(1, Int3{-1, 0, -1});
            else if (turnDraw == 2) p.own = rotate_then_shift(3, Int3{chain[last].width - 1, 0, -p.width + 1});
            plat_place(p);
            const int me = members;
            chain[members++] = p;
            if (turnDraw != 0) {
                Plat &corner = chain[members++];
                plat_init(corner, K_TRANSITION, NORTH | (turnDraw == 1 ? WEST : EAST), chain[last].width);
                corner.length = chain[me].width - 1;
                corner.parent = plat_next_anchor(chain[last]);
                plat_place(corner); plat_roll(corner, g, cfg); plat_build(corner, g);
            }
            last = me;
            wantWidth = chain[me].width;
        }
        {
            Plat &goal = chain[members++];
            plat_init(goal, K_EXIT, NORTH | EAST | WEST, wantWidth);
            goal.parent = plat_next_anchor(chain[last]);
            plat_roll(goal, g, cfg); plat_place(goal); plat_build(goal, g);
        }
        for (int j = 0; j < members; ++j) plat_hull(chain[j]);
        bool clash = false;
        for (int j = 0; j < members && !clash; ++j)
            for (int k = 0; k < j - 2; ++k)
                if (overlap(chain[j].hull, chain[k].hull)) { clash = true; break; }
        if (!clash) break;
    }
    const unsigned kLayoutColors[14] = {0xffffff, 0xffffe6, 0xccffcc, 0xe6ecff, 0xd9d9d9, 0xffebcc, 0xb3b3b3,
                                        0xb3b3b3, 0xb3b3b3, 0xb3b3b3, 0x555555, 0x555555, 0x555555, 0x555555};   // env/const.hpp:121-136
    out->layout_color = (int)kLayoutColors[rand_range1(g, 0, 14)];
    out->wall_color = (int)kLayoutColors[rand_range1(g, 0, 14)];
    out->draw_walls = drawWalls ? 1 : 0;
    out->num_platforms = numPlatforms;
    Int3 lo{1 << 20, 1 << 20, 1 << 20}, hi{-(1 << 20), -(1 << 20), -(1 << 20)};
    for (int j = 0; j < members; ++j) {
        const Aabb h = chain[j].hull;
        lo = Int3{imin(lo.x, h.lo.x), imin(lo.y, h.lo.y), imin(lo.z, h.lo.z)};
        hi = Int3{imax(hi.x, h.hi.x), imax(hi.y, h.hi.y), imax(hi.z, h.hi.z)};
    }
    Level &lv = w.level;
    lv.lo = lo; lv.nx = hi.x - lo.x; lv.ny = hi.y - lo.y; lv.nz = hi.z - lo.z; lv.draw_walls = drawWalls ? 1 : 0; lv.members = members;
    out->dim[0] = lv.nx; out->dim[1] = lv.ny; out->dim[2] = lv.nz;
    out->org[0] = lo.x; out->org[1] = lo.y; out->org[2] = lo.z;
    if (stats) { stats->attempts = attempts; stats->left_turns = lefts; stats->right_turns = rights; }
}

// The merge's two passes in key order -- key = type << 2 | colour slot of the painted value: the floor is (SOLID | OPAQUE, slot 0) = 12, the walls are
// (SOLID | OPAQUE, slot 1) = 13 when they are drawn and (SOLID, slot 1) = 5 when not.  -> plane (0 floor, 1 wall) of pass `pass`, its box type and slot
MV_HD int merge_pass(int pass, int draw_walls, int &type, int &slot)
{
    const int plane = draw_walls ? pass : 1 - pass;
    type = plane == 0 ? (VX_SOLID | VX_OPAQUE) : (VX_SOLID | (draw_walls ? VX_OPAQUE : 0));
    slot = plane;
    return plane;
}
MV_HD bool grid_fits(const Level &lv) { return lv.nx > 0 && lv.ny > 0 && lv.nz > 0 && (long long)lv.nx * lv.ny * lv.nz <= (long long)GRID_CELLS; }

// middle, serial form: the paint -- later boxes overwrite earlier ones -- and the canonical greedy merge (scan y, z, x; grow x, then z, then y) on the
// two bit planes of `grid` (GRID_WORDS words), one cell at a time
MV_HD void draw_slabs_serial(const Scratch &w, uint32_t *grid, EpisodeBlob *out, int &flags)
{
    const Level &lv = w.level;
    out->num_boxes = 0;
    if (!grid_fits(lv)) { flags |= FLAG_SLABS; return; }
    const int nx = lv.nx, ny = lv.ny, nz = lv.nz, total = nx * ny * nz, words = (total + 31) / 32;
    uint32_t *planes[2] = {grid, grid + PLANE_WORDS};
    for (int i = 0; i < words; ++i) { planes[0][i] = 0; planes[1][i] = 0; }
    for (int j = 0; j < lv.members; ++j) {
        const Plat &p = w.chain[j];
        for (int i = 0; i < p.num_floor + p.num_wall; ++i) {
            const int plane = i < p.num_floor ? 0 : 1;
            const Aabb b = placed(p.root, plane == 0 ? p.floor[i] : p.wall[i - p.num_floor]);
            for (int x = b.lo.x; x < b.hi.x; ++x)
                for (int y = b.lo.y; y < b.hi.y; ++y)
                    for (int z = b.lo.z; z < b.hi.z; ++z) {
                        const int id = ((y - lv.lo.y) * nz + (z - lv.lo.z)) * nx + (x - lv.lo.x);
                        planes[plane][id >> 5] |= 1u << (id & 31);
                        planes[1 - plane][id >> 5] &= ~(1u << (id & 31));
                    }
        }
    }
    int nb = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int type, slot;
        uint32_t *pl = planes[merge_pass(pass, lv.draw_walls, type, slot)];
        auto is = [&](int x, int y, int z) {
            if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return false;
            const int id = (y * nz + z) * nx + x;
            return ((pl[id >> 5] >> (id & 31)) & 1u) != 0;
        };
        for (int y = 0; y < ny; ++y)
            for (int z = 0; z < nz; ++z)
                for (int x = 0; x < nx; ++x) {
                    if (!is(x, y, z)) continue;
                    int x1 = x, z1 = z, y1 = y;
                    while (is(x1 + 1, y, z)) ++x1;
                    for (bool ok = true; ok;) {
                        for (int xx = x; xx <= x1 && ok; ++xx) ok = is(xx, y, z1 + 1);
                        if (ok) ++z1;
                    }
                    for (bool ok = true; ok;) {
                        for (int zz = z; zz <= z1 && ok; ++zz)
                            for (int xx = x; xx <= x1 && ok; ++xx) ok = is(xx, y1 + 1, zz);
                        if (ok) ++y1;
                    }
                    for (int yy = y; yy <= y1; ++yy)
                        for (int zz = z; zz <= z1; ++zz)
                            for (int xx = x; xx <= x1; ++xx) { const int id = (yy * nz + zz) * nx + xx; pl[id >> 5] &= ~(1u << (id & 31)); }
                    if (nb >= MAX_BOXES) flags |= FLAG_SLABS;
                    else {
                        LayoutBox &b = out->boxes[nb++];
                        b.min[0] = x + lv.lo.x; b.min[1] = y + lv.lo.y; b.min[2] = z + lv.lo.z;
                        b.max[0] = x1 + 1 + lv.lo.x; b.max[1] = y1 + 1 + lv.lo.y; b.max[2] = z1 + 1 + lv.lo.z;
                        b.type = type; b.slot = slot;
                    }
                }
    }
    out->num_boxes = nb;
}

MV_HD bool fits_i8(int v) { return v >= -128 && v <= 127; }

// tail (serial): terrain boxes, spawn cells, movable boxes, reward objects, the episode length, the spawn rotations
// -> the value the env's NEXT Env::reset will draw for its seed (nothing consumes the env's stream in between)
MV_HD uint32_t draw_tail(Mt &g, Scratch &w, int num_agents, float base_episode_len, EpisodeBlob *out, int &flags)
{
    Plat *chain = w.chain;
    const int members = w.level.members;
    // terrain boxes in drawable order: per platform, exit pads before lava (a platform has one or the other)
    int numTerrain = 0;
    for (int j = 0; j < members; ++j) {
        const Plat &p = chain[j];
        if (!p.terrain_type) continue;
        if (numTerrain >= MAX_TERRAIN) { flags |= FLAG_TERRAIN; continue; }
        const Aabb b = placed(p.root, p.terrain);
        TerrainBox &o = out->terrain[numTerrain++];
        o.min[0] = b.lo.x; o.min[1] = b.lo.y; o.min[2] = b.lo.z; o.max[0] = b.hi.x; o.max[1] = b.hi.y; o.max[2] = b.hi.z;
        o.type = p.terrain_type; o.pad = 0;
    }
    out->num_terrain = numTerrain;
    {   // agent spawn cells on the start platform (Platform::agentSpawnPoints)
        Plat &sp = chain[0];
        for (int x = 0; x < MAX_LEN; ++x)
            for (int z = 0; z < MAX_WIDTH; ++z) w.taken[x][z] = 0;
        int n = 0;
        for (int i = 0; i < num_agents; ++i)
            for (int attempt = 0; attempt < 10; ++attempt) {
                const int x = rand_range1(g, 1, sp.length - 1), z = rand_range1(g, 1, sp.width - 1);
                if (!occ_inside(x, z) || w.taken[x][z]) continue;
                const int y = sp.occ[x][z] + 1;
                sp.occ[x][z] = (uint8_t)(sp.occ[x][z] + 2);
                out->spawn[n][0] = x; out->spawn[n][1] = y; out->spawn[n][2] = z;
                ++n;
                w.taken[x][z] = 1;
                break;
            }
        if (n == 0) { out->spawn[0][0] = 1; out->spawn[0][1] = 1; out->spawn[0][2] = 1; n = 1; }
        for (int i = n; i < num_agents; ++i)
            for (int k = 0; k < 3; ++k) out->spawn[i][k] = out->spawn[0][k];
    }
    // movable boxes and reward objects
    int *share = w.share;
    for (int i = 0; i < members; ++i) share[i] = 0;
    for (int i = 1; i < members; ++i) {
        const int need = plat_boxes_needed(chain[i]);
        for (int b = 0; b < need; ++b) ++share[rand_range1(g, imax(0, i - 2), i)];
    }
    int totalObjects = 0, numObjects = 0, numRewards = 0;
    for (int i = 0; i < members; ++i) {
        const float fraction = frand1(g) * 0.5f;
        const int extra = lround_half_away(fraction * float(share[i])) + rand_range1(g, 0, 2);
        plat_scatter(chain[i], share[i] + extra, g, [&](Int3 c) {
            if (numObjects >= MAX_OBJECTS) flags |= FLAG_OBJECTS;
            if (!fits_i8(c.x) || !fits_i8(c.y) || !fits_i8(c.z)) flags |= FLAG_COORDS;
            if (numObjects < MAX_OBJECTS) out->objects[numObjects++] = MovableObject{(int8_t)c.x, (int8_t)c.y, (int8_t)c.z, 0};
            ++totalObjects;
        });
    }
    for (int i = 1; i < members - 1; ++i) {
        const int n = rand_range1(g, 0, 2);
        plat_scatter(chain[i], n, g, [&](Int3 c) {
            if (numRewards >= MAX_REWARDS) flags |= FLAG_REWARDS;
            if (!fits_i8(c.x) || !fits_i8(c.y) || !fits_i8(c.z)) flags |= FLAG_COORDS;
            if (numRewards < MAX_REWARDS) out->rewards[numRewards++] = MovableObject{(int8_t)c.x, (int8_t)c.y, (int8_t)c.z, 1};
        });
    }
    out->num_objects = numObjects; out->num_rewards = numRewards;
    const float byLevel = float(out->num_platforms) * 35 + float(totalObjects) * 1;
    out->episode_len = base_episode_len > byLevel ? base_episode_len : byLevel;   // std::max(base, byLevel): the first unless it is smaller
    for (int i = 0; i < num_agents; ++i) out->yaw_frand[i] = frand1(g);
    return (uint32_t)rand_range1(g, 0, 1 << 30);
}

// Empty (generate_empty_episode): Env::reset's seed draw, one static slab, every agent at (1, 1, 1), the spawn rotations.  `out` is zero on entry.
MV_HD uint32_t draw_empty(Mt &g, const GenState &st, uint32_t *mt, int num_agents, float base_episode_len, EpisodeBlob *out)
{
    g.s = mt;
    uint32_t seed = st.seed;
    if (st.seed_is_env_seed) {
        mt_seed1(g, seed);
        seed = (uint32_t)rand_range1(g, 0, 1 << 30);
    }
    mt_seed1(g, seed);
    out->num_boxes = 1;
    LayoutBox &b = out->boxes[0];
    b.min[0] = -5; b.min[1] = -1; b.min[2] = -5; b.max[0] = 15; b.max[1] = 1; b.max[2] = 15;
    b.type = VX_SOLID | VX_OPAQUE; b.slot = 0;
    out->layout_color = 0x2eb5d0; out->wall_color = 0x2eb5d0; out->draw_walls = 0;   // ColorRgb::BLUE
    out->dim[0] = 20; out->dim[1] = 2; out->dim[2] = 20;
    out->episode_len = base_episode_len;
    for (int k = 0; k < num_agents; ++k) { out->spawn[k][0] = out->spawn[k][1] = out->spawn[k][2] = 1; }
    for (int i = 0; i < num_agents; ++i) out->yaw_frand[i] = frand1(g);
    return (uint32_t)rand_range1(g, 0, 1 << 30);
}

}  // namespace odraw
}  // namespace mv
