// megaverse_amd/csrc/mv_gen_football.cpp -- host-side Football episode generator (reference paths relative to src/libs):
//   Env::reset                                  env/src/env.cpp:57-76 (the episode seed drawn from the env's own stream)
//   FootballScenario::reset                     scenarios/src/scenario_football.cpp:112-129 (the ball draws nothing)
//   FootballLayout (an EmptyPlatform)           scenario_football.cpp:7-22, scenarios/include/scenarios/platforms.hpp:167-190,221-244,306-330
//   DefaultScenario::spawnAgents                scenarios/include/scenarios/scenario_default.hpp:80-97 (one frand per agent)
//   FootballScenario::addEpisodeDrawables       scenario_football.cpp:131-141 (draws nothing from the stream)
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "mv_gen.h"

namespace mv {

namespace {
using Rng = std::mt19937;
inline int rand_range(int lo, int hi, Rng &rng) { return std::uniform_int_distribution<>{lo, hi - 1}(rng); }   // util.hpp:30-33
inline float frand01(Rng &rng) { return std::uniform_real_distribution<float>{0, 1}(rng); }                    // util.hpp:46-49
}  // namespace

void generate_football_episode(std::mt19937 &rng, int num_agents, float base_episode_len, FootballBlob &out)
{
    std::memset(&out, 0, sizeof out);

    // Env::reset: re-seed from the env's own stream (env.cpp:61-62)
    const int episode_seed = rand_range(0, 1 << 30, rng);
    rng.seed((unsigned long)episode_seed);

    // FootballLayout::init: length, then width (EmptyPlatform's -1), then height
    const int L = rand_range(14, 24, rng), W = rand_range(12, 24, rng), H = rand_range(3, 7, rng);
    out.length = L; out.width = W; out.height = H;

    // ---- the room: floor (0, 0, 0)-(L, 1, W) and four walls H high, all solid + drawn in LAYOUT_DEFAULT (vg.addPlatform(..., true)); merged as
    // every layout is (one class: seeds in (y, z, x) order, grown along x, then z, then y) -- floor, east wall, south, north, west
    {
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
                    if (out.num_boxes < FB_MAX_LAYOUT) {
                        LayoutBox &b = out.boxes[out.num_boxes++];
                        b.min[0] = x; b.min[1] = y; b.min[2] = z; b.max[0] = x1; b.max[1] = y1; b.max[2] = z1;
                        b.type = VX_SOLID | VX_OPAQUE; b.slot = 0;
                    } else generator_overflow_raise(GEN_SLABS);
                }
    }

    // ---- Platform::agentSpawnPoints (platforms.hpp:221-244): up to 10 draws of a free (x, z) per agent, y = occupancy + 1 = 1.  (An agent without a point
    // -- ten draws all taken, impossible in a room of >= 120 cells for 8 agents unless the stream says so -- would index past the reference's vector;
    // here it takes the first agent's point.)
    std::set<std::pair<int, int>> taken;
    int found = 0;
    for (int i = 0; i < num_agents; ++i)
        for (int attempt = 0; attempt < 10; ++attempt) {
            const int x = rand_range(1, L - 1, rng), z = rand_range(1, W - 1, rng);
            if (taken.count({x, z})) continue;
            taken.emplace(x, z);
            out.spawn[found][0] = float(x); out.spawn[found][1] = 1.0f; out.spawn[found][2] = float(z);
            ++found;
            break;
        }
    for (int i = found; i < num_agents; ++i) std::memcpy(out.spawn[i], out.spawn[0], sizeof out.spawn[i]);

    out.episode_len = base_episode_len;
    for (int i = 0; i < num_agents; ++i) out.yaw_frand[i] = frand01(rng);
}

}  // namespace mv
