// megaverse_amd/csrc/mv_scenarios.cpp -- see mv_scenarios.h
#include "mv_scenarios.h"

namespace mv {

static constexpr bool every_family_listed()
{
    for (const ScenarioRow &row : kScenarios) {
        bool found = false;
        for (const char *t = kAccelerated; *t && !found; ++t) {
            int k = 0;
            while (row.name[k] && t[k] == row.name[k]) ++k;
            found = !row.name[k];
        }
        if (!found) return false;
    }
    return true;
}
static_assert(every_family_listed(), "mv_create's \"Unknown scenario\" text names every family of the table");

bool scenario_from_name(const std::string &scen, int &scenario, ObstacleConfig &oc)
{
    for (const ScenarioRow &row : kScenarios) {
        if (!row.presets) {
            if (scen != row.lower) continue;
            scenario = row.scenario;
            return true;
        }
        if (scen.rfind(row.lower, 0) != 0) continue;   // scenario_obstacles.hpp:94-268: mv_gen.h's table
        const ObstaclePreset *preset = nullptr;
        for (const ObstaclePreset &p : kObstaclePresets)
            if (scen == p.name) preset = &p;
        if (!preset) return false;
        scenario = row.scenario;
        const float carried = oc.carried_object_to_exit;
        oc = config_of(*preset);
        if (preset->carried_object_to_exit == 0.0f) oc.carried_object_to_exit = carried;
        return true;
    }
    return false;
}

// every record begins with its episode number: generate_episode writes it there, the copy kernels carry its word last
static_assert(offsetof(EpisodeBlob, seq) == 0 && offsetof(CollectBlob, seq) == 0 && offsetof(RearrangeBlob, seq) == 0 && offsetof(SokobanBlob, seq) == 0
                  && offsetof(HexBlob, seq) == 0 && offsetof(BoxAGoneBlob, seq) == 0 && offsetof(FootballBlob, seq) == 0,
              "an episode record begins with seq");

size_t generate_episode(const ScenarioRow &row, const GenContext &c, int seq, void *record)
{
    if (!row.generate || !row.generate(c, record)) return 0;
    *static_cast<int32_t *>(record) = seq;
    return row.used_bytes ? row.used_bytes(record) : row.record_bytes;
}

bool same_hex(const void *got, const void *want, int)
{   // the box list comes last and only its used prefix is meaningful
    const HexBlob &a = *static_cast<const HexBlob *>(got), &b = *static_cast<const HexBlob *>(want);
    return !std::memcmp(&a, &b, offsetof(HexBlob, objs)) && !std::memcmp(a.objs, b.objs, sizeof(HexRec) * (size_t)b.num_objs) &&
           !std::memcmp(a.boxes, b.boxes, sizeof(HexRec) * (size_t)b.num_boxes);
}

bool same_collect(const void *got, const void *want, int num_agents)
{   // its generator clears what it uses: the counts, then the used prefix of every list
    const CollectBlob &a = *static_cast<const CollectBlob *>(got), &b = *static_cast<const CollectBlob *>(want);
    return a.seq == b.seq && a.num_boxes == b.num_boxes && a.num_objects == b.num_objects && a.num_rewards == b.num_rewards &&
           a.num_positive == b.num_positive && a.layout_color == b.layout_color && a.wall_color == b.wall_color &&
           !std::memcmp(a.dim, b.dim, sizeof a.dim) && !std::memcmp(&a.episode_len, &b.episode_len, sizeof(float)) &&
           !std::memcmp(a.boxes, b.boxes, sizeof(LayoutBox) * (size_t)b.num_boxes) && !std::memcmp(a.heightmap, b.heightmap, sizeof a.heightmap) &&
           !std::memcmp(a.objects, b.objects, sizeof(MovableObject) * (size_t)b.num_objects) &&
           !std::memcmp(a.rewards, b.rewards, sizeof(MovableObject) * (size_t)b.num_rewards) &&
           !std::memcmp(a.spawn, b.spawn, sizeof a.spawn) && !std::memcmp(a.yaw_frand, b.yaw_frand, sizeof(float) * (size_t)num_agents);
}

bool episodes_equal(const ScenarioRow &row, const void *got, const void *want, size_t used, int num_agents)
{
    if (used != (row.used_bytes ? row.used_bytes(want) : row.record_bytes)) return false;
    return row.same ? row.same(got, want, num_agents) : !std::memcmp(got, want, row.record_bytes);
}

}  // namespace mv
