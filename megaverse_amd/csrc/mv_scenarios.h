// megaverse_amd/csrc/mv_scenarios.h -- what the HOST side knows about each scenario family, stated once: one row per SCN_* value (mv_types.h), in enum order.
// mv_create (mv_api.hip) reads its gym from the row, the episode feeder (mv_feeder.cpp) its generator and its draw kernel, the host-only test hooks
// (mv_api_debug.hip, mv_seed_envs.hip) their record sizes, mv_group_create (mv_api_step.hip) who may join a group.  Host-only: nothing here is device code,
// and nothing needs mv_api_internal.h.  The device-side dispatch is mv_step.hip / mv_step_union.hip.
#pragma once
#include <cstddef>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "mv_gen.h"
#include "mv_types.h"

namespace mv {

// what a generator call draws from: the env's random stream, the gym's Obstacles parameters, and Sokoban's state across episodes (the shuffled rest of the
// level file picked last, the level files found at construction); the others leave `levels` and `files` null
struct GenContext {
    std::mt19937 &rng;
    const ObstacleConfig &cfg;
    int num_agents;
    float base_episode_len;
    SokobanLevels *levels;
    const std::vector<std::string> *files;
};

// the draw kernel a family's episodes can come from instead of the host's worker threads (mv_create decides whether they do)
enum : int {
    DRAW_NONE = 0,
    DRAW_TOWER,       // always: tower_draw_kernel, no feeder at all (mv_reset.hip)
    DRAW_COLLECT,     // collect_draw_kernel (mv_collect_draw.h); its copy to the ring takes the record's used prefix
    DRAW_OBSTACLES,   // obstacles_draw_kernel over its grid regions (mv_obstacles_draw.h), for the configurations odraw::config_fits holds
    DRAW_EMPTY,       // the same kernel's one-slab form: no grids, whatever the configuration
};

// the per-env state arrays of GymView a family has besides boxes, objects and agents, which every family has (mv_api.hip: the arena's one list)
enum : unsigned {
    ARR_CHUNK = 1u << 0, ARR_TERRAIN = 1u << 1, ARR_REWARDS = 1u << 2, ARR_HEIGHTMAP = 1u << 3, ARR_ITEMS = 1u << 4, ARR_SOKO_CELLS = 1u << 5,
    ARR_HEX_BOXES = 1u << 6, ARR_HEX_OBJS = 1u << 7, ARR_BAG = 1u << 8, ARR_FB = 1u << 9,
};

struct ScenarioRow {
    int scenario;   // SCN_*: the row's own place in the table
    // the name as mv_create's error text spells it and as scenario_from_name takes it; presets: the family's names are kObstaclePresets' (mv_gen.h)
    const char *name, *lower;
    bool presets;
    // reward shaping (Scenario::init's teamSpirit first).  carried_default: the last default is ObstacleConfig::carried_object_to_exit's
    int num_shaping;
    const char *shaping_keys[NUM_SHAPING];
    float shaping_defaults[NUM_SHAPING];
    bool carried_default;
    // Resident episodes per env: two where an episode ends at its time limit only; THREE where a goal can end it early (the exit pad, every diamond collected,
    // the level solved, the arrangement matched, the maze's target found): the host's run-ahead is bounded in TICKS (refill_episodes), the status words are
    // read back every 16th, and a lucky env can finish twice inside that window -- a third resident episode covers it where two starved.
    int spares;
    // the episode record: its size, the bytes of it that travel (null: all of them), how two of them compare (null: byte for byte -- the generator clears
    // the whole record first), and the generator behind a thunk: fills `record`, false = it gave up (null: the episodes are drawn on the device alone)
    size_t record_bytes;
    size_t (*used_bytes)(const void *record);
    bool (*same)(const void *got, const void *want, int num_agents);
    bool (*generate)(const GenContext &c, void *record);
    int box_stride, reward_stride, vis_stride;
    float episode_len, look_limit;   // defaults of episodeLengthSec and verticalLookLimitRad (scenario.hpp:225-232)
    // the shortest an episode can last is min(max(episodeLengthSec, len_floor), len_cap) seconds: what decides how often the status words are read back
    float len_floor, len_cap;
    bool in_union;    // its tick is in the union kernels (mv_step_union.hip: tick_any): a group of gyms accepts it
    int draw;         // DRAW_*
    unsigned arrays;  // ARR_*
};

// ---- the thunks the rows name ----
template <class Blob, void (*Gen)(std::mt19937 &, int, float, Blob &)>
bool generate_as(const GenContext &c, void *record)
{
    Gen(c.rng, c.num_agents, c.base_episode_len, *static_cast<Blob *>(record));
    return true;
}
inline bool generate_obstacles_as(const GenContext &c, void *record)
{
    generate_obstacles_episode(c.rng, c.cfg, c.num_agents, c.base_episode_len, *static_cast<EpisodeBlob *>(record));
    return true;
}
inline bool generate_sokoban_as(const GenContext &c, void *record)
{
    return generate_sokoban_episode(c.rng, *c.levels, *c.files, c.num_agents, c.base_episode_len, *static_cast<SokobanBlob *>(record));
}
// the records whose last list is the long one: only its used prefix travels
inline size_t used_hex(const void *r) { return offsetof(HexBlob, boxes) + size_t(static_cast<const HexBlob *>(r)->num_boxes) * sizeof(HexRec); }
inline size_t used_boxagone(const void *r)
{
    return offsetof(BoxAGoneBlob, platforms) + size_t(static_cast<const BoxAGoneBlob *>(r)->num_platforms) * sizeof(BagPlatform);
}
inline size_t used_collect(const void *r) { return offsetof(CollectBlob, boxes) + size_t(static_cast<const CollectBlob *>(r)->num_boxes) * sizeof(LayoutBox); }
// the records whose generators clear what they use, not all of it: the head, then the used prefix of every list
bool same_hex(const void *got, const void *want, int num_agents);
bool same_collect(const void *got, const void *want, int num_agents);

constexpr float LEN_ANY = std::numeric_limits<float>::infinity();
constexpr unsigned ARR_HEX = ARR_REWARDS | ARR_HEX_BOXES | ARR_HEX_OBJS;

constexpr ScenarioRow kScenarios[] = {
    // scenario_tower_building.hpp:44-52; the time limit only (+ 4 s per object)
    {SCN_TOWER, "TowerBuilding", "towerbuilding", false,
     4, {"teamSpirit", "towerPickedUpObject", "towerVisitedBuildingZoneWithObject", "towerBuildingReward"}, {0.1f, 0.1f, 0.1f, 1.0f}, false,
     2, sizeof(TowerBlob), nullptr, nullptr, nullptr,
     MAX_BOXES, MAX_REWARDS, 256, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_TOWER, ARR_CHUNK},
    // scenario_obstacles.hpp:36-44, teamSpirit 0 from Scenario::init (scenario.hpp:94-103); never under 35 s per platform
    {SCN_OBSTACLES, "Obstacles", "obstacles", true,
     5, {"teamSpirit", "obstaclesAgentAtExit", "obstaclesAllAgentsAtExit", "obstaclesExtraReward", "obstaclesAgentCarriedObjectToExit"},
     {0.0f, 1.0f, 5.0f, 0.5f, 0.0f}, true,
     3, sizeof(EpisodeBlob), nullptr, nullptr, generate_obstacles_as,
     MAX_BOXES, MAX_REWARDS, 256, 60.0f, 0.2f, 35.0f, LEN_ANY, true, DRAW_OBSTACLES, ARR_TERRAIN | ARR_REWARDS},
    // scenario_collect.hpp:44-52; scenarios/init.hpp:45
    {SCN_COLLECT, "Collect", "collect", false,
     5, {"teamSpirit", "collectSingleGood", "collectSingleBad", "collectAll", "collectAbyss"}, {0.0f, 1.0f, -1.0f, 5.0f, -0.5f}, false,
     3, sizeof(CollectBlob), used_collect, same_collect, generate_as<CollectBlob, generate_collect_episode>,
     COLLECT_MAX_BOXES, COLLECT_MAX_REWARDS, 1024, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_COLLECT, ARR_REWARDS | ARR_HEIGHTMAP},
    // scenario_rearrange.hpp:96-102; scenarios/init.hpp:49
    {SCN_REARRANGE, "Rearrange", "rearrange", false,
     3, {"teamSpirit", "rearrangeOneMoreObjectCorrectPosition", "rearrangeAllObjectsCorrectPosition"}, {0.0f, 1.0f, 10.0f}, false,
     3, sizeof(RearrangeBlob), nullptr, nullptr, generate_as<RearrangeBlob, generate_rearrange_episode>,
     MAX_BOXES, MAX_REWARDS, 256, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_NONE, ARR_REWARDS | ARR_ITEMS},
    // scenario_sokoban.hpp:40-53, teamSpirit 0; scenarios/init.hpp:46
    {SCN_SOKOBAN, "Sokoban", "sokoban", false,
     4, {"teamSpirit", "sokobanBoxOnTarget", "sokobanBoxLeavesTarget", "sokobanAllBoxesOnTarget"}, {0.0f, 1.0f, -1.0f, 10.0f}, false,
     3, sizeof(SokobanBlob), nullptr, nullptr, generate_sokoban_as,
     MAX_BOXES, MAX_REWARDS, 256, 80.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_NONE, ARR_REWARDS | ARR_SOKO_CELLS},
    // EmptyScenario::defaultRewardShaping() is {} (scenario_empty.hpp:28) + Scenario::init's teamSpirit; scenarios/init.hpp:34.  The Obstacles family's record
    // and arrays (one slab, no terrain); the time limit only
    {SCN_EMPTY, "Empty", "empty", false, 1, {"teamSpirit"}, {0.0f}, false,
     2, sizeof(EpisodeBlob), nullptr, nullptr, generate_as<EpisodeBlob, generate_empty_episode>,
     MAX_BOXES, MAX_REWARDS, 256, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_EMPTY, ARR_TERRAIN | ARR_REWARDS},
    // scenario_hex_memory.hpp:37-43, scenario_hex_explore.hpp:28-31 (+ teamSpirit 0); scenarios/init.hpp:47-48
    {SCN_HEX_MEMORY, "HexMemory", "hexmemory", false, 3, {"teamSpirit", "memoryCollectGood", "memoryCollectBad"}, {0.0f, 1.0f, -1.0f}, false,
     3, sizeof(HexBlob), used_hex, same_hex, generate_as<HexBlob, generate_hex_memory_episode>,
     MAX_BOXES, MAX_REWARDS, 2048, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_NONE, ARR_HEX},
    {SCN_HEX_EXPLORE, "HexExplore", "hexexplore", false, 2, {"teamSpirit", "exploreSolved"}, {0.0f, 5.0f}, false,
     3, sizeof(HexBlob), used_hex, same_hex, generate_as<HexBlob, generate_hex_explore_episode>,
     MAX_BOXES, MAX_REWARDS, 2048, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, true, DRAW_NONE, ARR_HEX},
    // scenario_box_a_gone.hpp:82-98 (+ teamSpirit 0); scenarios/init.hpp:50.  At most 8 + 972 + 24 boxes, all in the world frame.  It ends as soon as every
    // agent is on the floor: for a random or idle agent after 30-60 ticks, never under 20 (it lands on its spawn platform, leaves it or waits for it to
    // vanish, falls at least 6.8 units -- 15 ticks from rest -- then doneWithTimer's 0.3 s): 1.3 s, whatever episodeLengthSec says
    {SCN_BOXAGONE, "BoxAGone", "boxagone", false, 3, {"teamSpirit", "boxagoneTouchedFloor", "boxagonePerStepReward"}, {0.0f, -0.1f, 0.01f}, false,
     3, sizeof(BoxAGoneBlob), used_boxagone, nullptr, generate_as<BoxAGoneBlob, generate_boxagone_episode>,
     MAX_BOXES, MAX_REWARDS, 1024, 300.0f, 0.75f, -LEN_ANY, 1.3f, false, DRAW_NONE, ARR_REWARDS | ARR_HEX_BOXES | ARR_BAG},
    // FootballScenario has no shaping of its own (+ teamSpirit 0); scenarios/init.hpp:51; the time limit only
    {SCN_FOOTBALL, "Football", "football", false, 1, {"teamSpirit"}, {0.0f}, false,
     2, sizeof(FootballBlob), nullptr, nullptr, generate_as<FootballBlob, generate_football_episode>,
     MAX_BOXES, MAX_REWARDS, 256, 60.0f, 0.2f, -LEN_ANY, LEN_ANY, false, DRAW_NONE, ARR_HEX | ARR_FB},
};
constexpr bool rows_in_enum_order()
{
    for (int i = 0; i < SCN_COUNT; ++i)
        if (kScenarios[i].scenario != i) return false;
    return true;
}
static_assert(sizeof(kScenarios) / sizeof(kScenarios[0]) == SCN_COUNT && rows_in_enum_order(), "one row per SCN_* family, in enum order");

inline const ScenarioRow &scenario_row(int scenario) { return kScenarios[scenario]; }

// scenario name (lower case) -> family + generator parameters (scenarios/init.hpp:30-52); an Obstacles name keeps oc's carried_object_to_exit where its
// preset has none
bool scenario_from_name(const std::string &lower_name, int &scenario, ObstacleConfig &oc);
// what this build accelerates, as mv_create's answer to an unknown name has always listed it (Empty, the performance-test scenario, last); a family
// whose name is not in it does not compile (mv_scenarios.cpp)
constexpr char kAccelerated[] = "TowerBuilding, ObstaclesEasy/Medium/Hard/Walls/Steps/Lava, Collect, Rearrange, Sokoban, HexMemory, HexExplore, BoxAGone, Football, Empty";

// Draws the next episode of row's family from c into `record` and numbers it `seq`: the one call behind the feeder's workers and the host-only hooks.
// Returns the bytes of the record that are used, 0 where the generator gave up (Sokoban: an unreadable level file) or the family has none.
size_t generate_episode(const ScenarioRow &row, const GenContext &c, int seq, void *record);
// got == want, as far as the family's generator defines the record (`used`: what generate_episode returned for `got`)
bool episodes_equal(const ScenarioRow &row, const void *got, const void *want, size_t used, int num_agents);

}  // namespace mv
