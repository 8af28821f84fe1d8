// megaverse_amd/csrc/mv_draw.h -- the device episode generators as the host sees them, stated once: what a draw launch takes (DrawLaunch) and one row per
// DRAW_* kind (mv_scenarios.h) -- its launcher, its host twin, its record, its grid regions, what it cannot draw and the switch mv_create reads for it.
// The episode feeder (mv_feeder.cpp), mv_create (mv_api.hip) and the test hooks (mv_draw.hip) read the row; none of them names a kind's kernel.
// Host-only: nothing here is device code.  Adding a device generator: a header, a kernel with its launcher and host twin, a row.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mv_draw_common.h"
#include "mv_obstacles_draw.h"
#include "mv_scenarios.h"
#include "mv_types.h"

namespace mv {

// One launch of a draw kernel: the envs envs[0 .. count) (null: 0 .. count - 1) draw their next episode into slots + env * slot_bytes and advance states[env].
struct DrawLaunch {
    draw::GenState *states;
    const int32_t *envs;
    int count;
    uint8_t *slots;
    size_t slot_bytes;
    int scenario;                // SCN_*: which of its kind's families (Obstacles / Empty, HexMemory / HexExplore)
    const ObstacleConfig *cfg;   // the gym's generator parameters (the Obstacles family reads them)
    int num_agents;
    float base_episode_len;
    uint32_t *grids;             // `regions` regions of the kind's region_bytes each (null where it has none)
    int regions;
    hipStream_t stream;
    int32_t *flag_word;          // FLAG_* a capacity raised are ORed in here (may be null)
    long long *timing;           // test hook, Collect's launcher alone: 8 clock reads per episode (null: none)
};

struct DrawKind {
    // false: arguments the kernel cannot take (null states or slots, a slot smaller than the record, a negative count, an agent count outside
    // 1 .. MAX_AGENTS) -- nothing was launched, and whoever waits for an episode must be told.  A launch that fails shows in hipGetLastError.
    bool (*launch)(const DrawLaunch &a);
    // the same code compiled for the CPU: the n-th episode (n >= 1) of an env seeded with env_seed into `record`, zeroed before each episode; seq = n
    void (*host)(int scenario, const ObstacleConfig &cfg, int num_agents, uint32_t env_seed, int n, float base_episode_len, void *record);
    size_t record_bytes;
    int max_regions;        // a feeder of num_envs envs holds min(num_envs, max_regions) grid regions, one per episode a launch draws at a time
    size_t region_bytes;    // 0: the kind has none
    bool (*config_fits)(const ObstacleConfig &cfg);   // null: whatever the configuration
    const char *switch_name;                          // MV_<X>_DEVICE_GEN: set and not 0 at mv_create: drawn on the device

    int regions(int num_envs) const { return region_bytes ? std::min(num_envs, max_regions) : 0; }
};

bool launch_collect_draw(const DrawLaunch &a);     // mv_collect_draw.hip
bool launch_obstacles_draw(const DrawLaunch &a);   // mv_obstacles_draw.hip: DRAW_OBSTACLES and DRAW_EMPTY (a.scenario says which)
bool launch_hex_draw(const DrawLaunch &a);         // mv_hex_draw.hip
void collect_draw_host(int scenario, const ObstacleConfig &cfg, int num_agents, uint32_t env_seed, int n, float base_episode_len, void *record);
void obstacles_draw_host(int scenario, const ObstacleConfig &cfg, int num_agents, uint32_t env_seed, int n, float base_episode_len, void *record);
void hex_draw_host(int scenario, const ObstacleConfig &cfg, int num_agents, uint32_t env_seed, int n, float base_episode_len, void *record);
// MV_DRAW_TIMING: where the episodes of a launch that was given `timing` spent their time, one line to stderr (100 MHz clock)
void print_collect_draw_timing(const long long *timing, int count);

// indexed by DRAW_*.  DRAW_TOWER's kernel is fed by no feeder and launched by mv_create's own path (mv_reset.hip): its row is empty, as DRAW_NONE's.
constexpr DrawKind kDrawKinds[DRAW_COUNT] = {
    {},
    {},
    {launch_collect_draw, collect_draw_host, sizeof(CollectBlob), 0, 0, nullptr, "MV_COLLECT_DEVICE_GEN"},
    {launch_obstacles_draw, obstacles_draw_host, sizeof(EpisodeBlob), odraw::DRAW_REGIONS, size_t(odraw::GRID_WORDS) * sizeof(uint32_t), odraw::config_fits,
     "MV_OBSTACLES_DEVICE_GEN"},
    {launch_obstacles_draw, obstacles_draw_host, sizeof(EpisodeBlob), 0, 0, nullptr, "MV_OBSTACLES_DEVICE_GEN"},   // the one-slab form: no grids
    {launch_hex_draw, hex_draw_host, sizeof(HexBlob), 0, 0, nullptr, "MV_HEX_DEVICE_GEN"},
};
static_assert(DRAW_COLLECT == 2 && DRAW_OBSTACLES == 3 && DRAW_EMPTY == 4 && DRAW_HEX == 5 && DRAW_COUNT == 6, "one row per DRAW_* kind, in enum order");

inline const DrawKind &draw_kind(int draw) { return kDrawKinds[draw]; }

// what every launcher refuses before it looks at anything of its own
inline bool draw_launch_ok(const DrawLaunch &a, size_t record_bytes)
{
    return a.count >= 0 && a.states && a.slots && a.slot_bytes >= record_bytes && a.num_agents >= 1 && a.num_agents <= MAX_AGENTS;
}

}  // namespace mv
