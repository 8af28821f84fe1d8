// megaverse_amd/csrc/mv_gen_boxagone.cpp -- host-side BoxAGone episode generator (reference paths relative to src/libs):
//   Env::reset                                  env/src/env.cpp:57-76 (the episode seed drawn from the env's own stream)
//   BoxAGoneScenario::reset                     scenarios/src/scenario_box_a_gone.cpp:41-95
//   BoxAGonePlatform (an EmptyPlatform)         scenario_box_a_gone.cpp:7-26, scenarios/include/scenarios/platforms.hpp:306-330
//   DefaultScenario::spawnAgents                scenarios/include/scenarios/scenario_default.hpp:80-97 (one frand per agent)
//   BoxAGoneScenario::addEpisodeDrawables       scenario_box_a_gone.cpp:175-233 (draws nothing from the stream)
// The room is fixed (24 x 8 x 24 voxels, all four walls, no random draw: BoxAGonePlatform::init overrides EmptyPlatform's); the levels of
// platforms and the shuffled spawn list are what the stream decides.
#include <algorithm>
#include <cstring>
#include <random>
#include <vector>

#include "mv_gen.h"

namespace mv {

namespace {
using Rng = std::mt19937;
inline int rand_range(int lo, int hi, Rng &rng) { return std::uniform_int_distribution<>{lo, hi - 1}(rng); }   // util.hpp:30-33
inline float frand01(Rng &rng) { return std::uniform_real_distribution<float>{0, 1}(rng); }                    // util.hpp:46-49
}  // namespace

void generate_boxagone_episode(std::mt19937 &rng, int num_agents, float base_episode_len, BoxAGoneBlob &out)
{
    std::memset(&out, 0, sizeof out);

    // Env::reset: re-seed from the env's own stream (env.cpp:61-62)
    const int episode_seed = rand_range(0, 1 << 30, rng);
    rng.seed((unsigned long)episode_seed);

    // ---- the room: floor (0, 0, 0)-(24, 1, 24) and four walls 8 high, all solid + drawn in LAYOUT_DEFAULT (vg.addPlatform(..., true)); merged as
    // every layout is (one class: seeds in (y, z, x) order, grown along x, then z, then y) -- floor, south wall strip, then the three others
    {
        constexpr int L = BAG_ROOM, H = 8, W = BAG_ROOM;
        std::vector<uint8_t> solid(size_t(L) * H * W, 0), used(solid.size(), 0);
        auto id = [&](int x, int y, int z) { return (size_t(y) * W + z) * L + x; };
        for (int x = 0; x < L; ++x)
            for (int y = 0; y < H; ++y)
                for (int z = 0; z < W; ++z)
                    solid[id(x, y, z)] = y == 0 || x == 0 || x == L - 1 || z == 0 || z == W - 1;
        auto open_cell = [&](int x, int y, int z) { return x >= 0 && x < L && y >= 0 && y < H && z >= 0 && z < W && solid[id(x, y, z)] && !used[id(x, y, z)]; };
        for (int y = 0; y < H; ++y)
            for (int z = 0; z < W; ++z)
                for (int x = 0; x < L; ++x) {
                    if (!open_cell(x, y, z)) continue;
                    int x1 = x + 1, z1 = z + 1, y1 = y + 1;
                    while (open_cell(x1, y, z)) ++x1;
                    auto row_ok = [&](int yy, int zz) { for (int xx = x; xx < x1; ++xx) if (!open_cell(xx, yy, zz)) return false; return true; };
                    while (row_ok(y, z1)) ++z1;
                    auto layer_ok = [&](int yy) { for (int zz = z; zz < z1; ++zz) if (!row_ok(yy, zz)) return false; return true; };
                    while (layer_ok(y1)) ++y1;
                    for (int yy = y; yy < y1; ++yy) for (int zz = z; zz < z1; ++zz) for (int xx = x; xx < x1; ++xx) used[id(xx, yy, zz)] = 1;
                    if (out.num_boxes < BAG_MAX_LAYOUT) {
                        LayoutBox &b = out.boxes[out.num_boxes++];
                        b.min[0] = x; b.min[1] = y; b.min[2] = z; b.max[0] = x1; b.max[1] = y1; b.max[2] = z1;
                        b.type = VX_SOLID | VX_OPAQUE; b.slot = 0;
                    } else generator_overflow_raise(GEN_SLABS);
                }
    }

    // ---- the levels (scenario_box_a_gone.cpp:59-87)
    const int num_levels = rand_range(2, 4, rng);
    std::vector<float> spawns;   // x, y, z of every top-level cell, * voxel size
    int curr_level_height = 1;
    for (int level = 0; level < num_levels; ++level) {
        curr_level_height += rand_range(2, 4, rng);
        const int offset = BAG_ROOM / 2;
        const int level_length = rand_range(10, 19, rng);
        const int level_width = rand_range(10, 19, rng);
        const int start_x = offset - level_length / 2, start_z = offset - level_width / 2;
        const float skip_prob = frand01(rng) * 0.2f;
        out.level_y[level] = curr_level_height;
        for (int x = start_x; x < start_x + level_length; ++x)
            for (int z = start_z; z < start_z + level_width; ++z) {
                if (frand01(rng) < skip_prob) continue;
                if (out.num_platforms < BAG_MAX_PLATFORMS)   // (3 x 18 x 18: cannot overflow)
                    out.platforms[out.num_platforms++] = BagPlatform{int8_t(x), int8_t(curr_level_height), int8_t(z), int8_t(level)};
                if (level == num_levels - 1) {
                    spawns.push_back((float(x) + 0.5f) * 2.0f);
                    spawns.push_back((float(curr_level_height) + 0.5f) * 2.0f);
                    spawns.push_back((float(z) + 0.5f) * 2.0f);
                }
            }
    }
    out.num_levels = num_levels;

    // ---- spawn list: padded with its first entry, then std::shuffle'd with the episode stream (:89-92).  (An empty top level -- every one of its >= 100
    // cells skipped at p <= 0.2 -- would index an empty vector in the reference; here it spawns at the room's centre.)
    struct P3 { float v[3]; };
    std::vector<P3> sp;
    for (size_t i = 0; i + 2 < spawns.size(); i += 3) sp.push_back(P3{{spawns[i], spawns[i + 1], spawns[i + 2]}});
    if (sp.empty()) sp.push_back(P3{{float(BAG_ROOM), 2.0f, float(BAG_ROOM)}});
    while (int(sp.size()) < num_agents) sp.push_back(sp[0]);
    std::shuffle(sp.begin(), sp.end(), rng);
    for (int i = 0; i < num_agents; ++i) std::memcpy(out.spawn[i], sp[size_t(i)].v, sizeof out.spawn[i]);

    out.episode_len = base_episode_len;
    for (int i = 0; i < num_agents; ++i) out.yaw_frand[i] = frand01(rng);
}

}  // namespace mv
