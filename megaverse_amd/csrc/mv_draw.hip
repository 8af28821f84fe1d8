// megaverse_amd/csrc/mv_draw.hip -- the test hooks of the device episode generators, written once over the table of draw kinds (mv_draw.h): the n-th episode
// of an env as a kind's code draws it on the host, and as its kernel draws it on the device.  The tests hold both against the host generators (mv_gen_*.cpp).
#include <cstring>
#include <string>
#include <vector>

#include "mv_api_internal.h"
#include "mv_draw.h"

using namespace mv;
using namespace mvapi;

// the scenario's family, its generator parameters and its draw kind; null (and the error set) where it has none or the kind cannot draw the configuration
static const DrawKind *kind_of(const char *hook, const char *name, int &scenario, ObstacleConfig &oc)
{
    const DrawKind *kind = name && scenario_from_name(lower(name), scenario, oc) ? &draw_kind(scenario_row(scenario).draw) : nullptr;
    if (kind && kind->launch && (!kind->config_fits || kind->config_fits(oc))) return kind;
    std::string have;   // (lower case, as scenario_from_name takes them)
    for (const ScenarioRow &row : kScenarios) {
        if (!draw_kind(row.draw).launch) continue;
        if (row.presets)
            for (const ObstaclePreset &p : kObstaclePresets) have += std::string(have.empty() ? "" : ", ") + p.name;
        else have += std::string(have.empty() ? "" : ", ") + row.lower;
    }
    fail(std::string(hook) + ": no device generator draws this scenario's episodes; the scenarios that have one: " + have);
    return nullptr;
}

extern "C" {

// Host-only test hook (no device needed): the n-th episode of an env seeded with `env_seed` as the scenario's device generator draws it ON THE HOST -- the
// same record mv_debug_generate_episode(scenario, ...) returns (its `seq` is n here, 0 there; what a generator leaves unused is zero here).
int mv_debug_draw_host(const char *scenario_name, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    const DrawKind *kind = kind_of("mv_debug_draw_host", scenario_name, scenario, oc);
    if (!kind) return -1;
    if (!out) return (int)kind->record_bytes;
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1) return fail("mv_debug_draw_host: bad arguments");
    if (out_bytes < 0 || (size_t)out_bytes < kind->record_bytes) return fail("mv_debug_draw_host: buffer too small");
    std::vector<uint8_t> record(kind->record_bytes, 0);   // (16-byte aligned, as operator new's memory is)
    kind->host(scenario, oc, num_agents, (uint32_t)env_seed, n, base_episode_len, record.data());
    std::memcpy(out, record.data(), record.size());
    return (int)record.size();
}

// Test hook: `count` envs seeded with env_seeds[i], each drawing its first n episodes ON THE DEVICE (n launches of the kind's kernel); out receives the envs'
// n-th episodes, count x the record size; *ms_per_launch (may be null) the mean time of a launch.  MV_DRAW_TIMING=1, Collect: the phases of the LAST launch's
// episodes to stderr.
int mv_debug_draw_device(int32_t device, const char *scenario_name, int32_t num_agents, const int32_t *env_seeds, int32_t count, int32_t n,
                         float base_episode_len, void *out, int64_t out_bytes, float *ms_per_launch)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    const DrawKind *kind = kind_of("mv_debug_draw_device", scenario_name, scenario, oc);
    if (!kind) return -1;
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1 || count < 1 || !env_seeds || !out) return fail("mv_debug_draw_device: bad arguments");
    const size_t bytes = (size_t)count * kind->record_bytes;
    if (out_bytes < 0 || (size_t)out_bytes < bytes) return fail("mv_debug_draw_device: buffer too small");
    HIP_TRY(hipSetDevice(device));
    std::vector<draw::GenState> st((size_t)count);
    for (int i = 0; i < count; ++i) st[(size_t)i] = draw::GenState{(uint32_t)env_seeds[i], 1, 1, 0};
    const bool timing = scenario_row(scenario).draw == DRAW_COLLECT && getenv("MV_DRAW_TIMING") != nullptr;
    std::vector<long long> tm(timing ? (size_t)count * 8 : 0);
    DrawLaunch a{nullptr, nullptr, count, nullptr, kind->record_bytes, scenario, &oc, num_agents, base_episode_len, nullptr, kind->regions(count), nullptr, nullptr, nullptr};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = hipMalloc((void **)&a.states, st.size() * sizeof(draw::GenState)) == hipSuccess && hipMalloc((void **)&a.slots, bytes) == hipSuccess &&
              (a.regions == 0 || hipMalloc((void **)&a.grids, (size_t)a.regions * kind->region_bytes) == hipSuccess) &&
              (!timing || hipMalloc((void **)&a.timing, tm.size() * sizeof(long long)) == hipSuccess) && hipMemset(a.slots, 0, bytes) == hipSuccess &&
              hipMemcpy(a.states, st.data(), st.size() * sizeof(draw::GenState), hipMemcpyHostToDevice) == hipSuccess &&
              hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess && hipEventRecord(e0, nullptr) == hipSuccess;
    for (int i = 0; i < n && ok; ++i) ok = kind->launch(a);
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
         hipMemcpy(out, a.slots, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    float ms = 0.0f;
    if (ok && ms_per_launch && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *ms_per_launch = ms / float(n);
    if (ok && timing && hipMemcpy(tm.data(), a.timing, tm.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess) print_collect_draw_timing(tm.data(), count);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (a.states) (void)hipFree(a.states);
    if (a.slots) (void)hipFree(a.slots);
    if (a.grids) (void)hipFree(a.grids);
    if (a.timing) (void)hipFree(a.timing);
    return ok ? 0 : fail("mv_debug_draw_device: a HIP call failed");
}

}  // extern "C"
