// megaverse_amd/csrc/mv_gen.h -- host-side episode generators (see mv_gen_obstacles.cpp)
#pragma once
#include <random>
#include <string>
#include <vector>

#include "mv_types.h"

namespace mv {

// ObstaclesScenario float params as integers (scenario_obstacles.hpp:46-68; per registered name :94-268)
struct ObstacleConfig {
    int min_platforms = 1, max_platforms = 2, min_gap = 1, max_gap = 2, min_lava = 1, max_lava = 4, min_height = 1, max_height = 3;
    int num_allowed_max_difficulty = 1;
    int platform_types[4] = {1, 2, 3, 4};   // WALL, LAVA, STEP, GAP
    int num_platform_types = 4;
    float carried_object_to_exit = 0.0f;    // default of the obstaclesAgentCarriedObjectToExit shaping key
};

// The registered Obstacles scenarios (scenario_obstacles.hpp:94-268), lower-case names: the one table scenario_from_name (mv_scenarios.cpp) reads its values from, and
// the one the device generator's capacities are asserted against at compile time (mv_obstacles_draw.h).  platform_type 0: all four types.
struct ObstaclePreset {
    const char *name;
    int min_platforms, max_platforms, min_gap, max_gap, min_lava, max_lava, min_height, max_height, platform_type;
    float carried_object_to_exit;
};
constexpr ObstaclePreset kObstaclePresets[] = {
    {"obstacleseasy", 1, 2, 1, 2, 1, 4, 1, 3, 0, 0.0f},     // :112-138 (the defaults)
    {"obstaclesmedium", 2, 4, 1, 2, 2, 5, 1, 3, 0, 0.0f},
    {"obstacleshard", 2, 7, 2, 3, 3, 10, 2, 4, 0, 0.0f},    // :164-189
    {"obstacleswalls", 1, 4, 1, 3, 2, 10, 1, 3, 1, 1.0f},   // :190-268
    {"obstaclessteps", 1, 4, 1, 3, 2, 10, 1, 3, 3, 1.0f},
    {"obstacleslava", 1, 4, 1, 3, 2, 10, 1, 3, 2, 1.0f},
};
constexpr int kNumObstaclePresets = int(sizeof(kObstaclePresets) / sizeof(kObstaclePresets[0]));
constexpr int largest_preset_platforms()
{
    int m = 0;
    for (int i = 0; i < kNumObstaclePresets; ++i) m = kObstaclePresets[i].max_platforms > m ? kObstaclePresets[i].max_platforms : m;
    return m;
}
constexpr int largest_preset_height()
{
    int m = 0;
    for (int i = 0; i < kNumObstaclePresets; ++i) m = kObstaclePresets[i].max_height > m ? kObstaclePresets[i].max_height : m;
    return m;
}
inline ObstacleConfig config_of(const ObstaclePreset &p)
{
    ObstacleConfig c;
    c.min_platforms = p.min_platforms; c.max_platforms = p.max_platforms; c.min_gap = p.min_gap; c.max_gap = p.max_gap; c.min_lava = p.min_lava;
    c.max_lava = p.max_lava; c.min_height = p.min_height; c.max_height = p.max_height; c.carried_object_to_exit = p.carried_object_to_exit;
    if (p.platform_type) { c.platform_types[0] = p.platform_type; c.num_platform_types = 1; }
    return c;
}

// Fixed capacities of the episode records (the reference has none): a generator that would exceed one drops the excess AND raises
// a flag here; mv_step / mv_reset report it (mv_api.hip: check_status_flags).  Process-wide, cleared when reported.
enum : int { GEN_SLABS = 1, GEN_TERRAIN = 2, GEN_OBJECTS = 4, GEN_REWARDS = 8, GEN_COORDS = 16 };
void generator_overflow_raise(int flags);
int generator_overflow_take();   // returns the flags raised ON THIS THREAD since the last call and clears them

// Advances `rng` exactly like Env::reset + ObstaclesScenario::reset + spawnAgents and fills `out`.
void generate_obstacles_episode(std::mt19937 &rng, const ObstacleConfig &cfg, int num_agents, float base_episode_len, EpisodeBlob &out);

// (tests) how the episode generate_obstacles_episode drew last ON THIS THREAD came about: chain attempts (each one after the first follows a hull clash),
// and the left and right turns of the chain that was kept
struct ObstacleStats { int attempts, left_turns, right_turns; };
ObstacleStats obstacles_last_stats();

// Empty (scenario_empty.{hpp,cpp}, the reference's performance-test scenario): Env::reset's seed draw + the agents' spawn rotations;
// one static 20 x 2 x 20 box as the only layout slab, every agent at (1, 1, 1).  Same record as the Obstacles family.
void generate_empty_episode(std::mt19937 &rng, int num_agents, float base_episode_len, EpisodeBlob &out);

// Advances `rng` exactly like Env::reset + CollectScenario::reset + spawnAgents + addEpisodeDrawables and fills `out`.
void generate_collect_episode(std::mt19937 &rng, int num_agents, float base_episode_len, CollectBlob &out);

// Advances `rng` exactly like Env::reset + RearrangeScenario::reset + spawnAgents + addEpisodeDrawables and fills `out`.
void generate_rearrange_episode(std::mt19937 &rng, int num_agents, float base_episode_len, RearrangeBlob &out);

// HexExplore / HexMemory: advance `rng` exactly like Env::reset + the scenario's reset + spawnAgents + addEpisodeDrawables and fill `out`
// (the maze's Kruskal is seeded with the episode seed: mv_gen_hex.cpp)
void generate_hex_explore_episode(std::mt19937 &rng, int num_agents, float base_episode_len, HexBlob &out);
void generate_hex_memory_episode(std::mt19937 &rng, int num_agents, float base_episode_len, HexBlob &out);

// Advances `rng` exactly like Env::reset + BoxAGoneScenario::reset + spawnAgents + addEpisodeDrawables and fills `out`.
void generate_boxagone_episode(std::mt19937 &rng, int num_agents, float base_episode_len, BoxAGoneBlob &out);

// Advances `rng` exactly like Env::reset + FootballScenario::reset + spawnAgents + addEpisodeDrawables and fills `out`.
void generate_football_episode(std::mt19937 &rng, int num_agents, float base_episode_len, FootballBlob &out);

// Sokoban keeps state across episodes: the shuffled levels of the file picked last (SokobanScenario::levels)
struct SokobanLevels {
    std::vector<std::vector<std::string>> pending;
};
// $BOXOBAN_LEVELS (or ~/datasets/boxoban) / unfiltered / train / 000.txt .. 999.txt that exist (scenario_sokoban.cpp:40-78)
std::vector<std::string> find_boxoban_level_files();
// Advances `rng` exactly like Env::reset + SokobanScenario::reset + spawnAgents and fills `out`; false if a level file is unreadable.
bool generate_sokoban_episode(std::mt19937 &rng, SokobanLevels &levels, const std::vector<std::string> &files, int num_agents,
                              float base_episode_len, SokobanBlob &out);

}  // namespace mv
