// megaverse_amd/csrc/mv_seed_envs.hip -- level seeds: the host side of mv_seed_envs / mv_seed_envs_host (include/megaverse_hip.h): Env::seed for chosen envs.
// TowerBuilding's generators live on the device: the masked seed kernel is tower_seed_envs_kernel (mv_reset.hip), next to mv_seed's.  Every other scenario's
// live in the episode feeder (mv_feeder.h: reseed_envs); of the device this file only wipes the flagged envs' rings (ring_wipe_envs_kernel below) and sends
// the new streams' first episodes up through the refill protocol (mv_api.hip: refill_episodes).  DESIGN.md 3.15 has the contract.
#include <cstddef>

#include "mv_api_internal.h"

namespace {

// Host-fed gyms: the episodes resident in a flagged env's ring were drawn from its old stream -- sequence number 0 matches nothing (every record of every
// scenario begins with its int32 seq: mv_types.h).  One lane per ring slot of every env.
__global__ void ring_wipe_envs_kernel(uint8_t *blobs, size_t blob_bytes, int spares, int num_envs, const int32_t *seeds)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_envs * spares) return;
    if (seeds[i / spares] < 0) return;
    *reinterpret_cast<int32_t *>(blobs + (size_t)i * blob_bytes) = 0;
}

int seed_envs_check(mv_gym *g, const void *seeds, const char *who)
{
    if (check(g)) return -1;
    if (!seeds) return fail(std::string(who) + ": null seeds");
    return 0;
}

// TowerBuilding, both forms, on the CALLER's stream like mv_seed's launches: behind whatever the caller enqueued there (the kernel that wrote a device
// array), behind every step launch enqueued so far (sim_join) and the last draw launch (tower_join); the next step launch waits for all of it
// (simMustWaitUser), and every later draw launch is ordered behind that step.  No host wait: the draw behind the seed kernel makes the new streams' first
// episodes resident in stream order.
int seed_envs_tower(mv_gym *g, const int32_t *device_seeds, const int32_t *host_seeds)
{
    HIP_TRY(hipSetDevice(g->device));
    if (sim_join(g) || tower_join(g)) return -1;
    if (host_seeds && g->seedEnvsPair.stage(host_seeds, (size_t)g->N * sizeof(int32_t), g->stream, &device_seeds)) return -1;
    launch_tower_seed_envs(g->gv, device_seeds, g->stream);
    launch_tower_draw(g->gv, g->stream);
    HIP_TRY(hipGetLastError());
    if (host_seeds && g->seedEnvsPair.mark(g->stream)) return -1;
    return 0;
}

// Host-fed gyms, host form.  The generators are the feeder's, and it needs the sequence number the device expects next of every flagged env: the current
// consumed counts, taken as mv_seed takes them -- with a host wait for everything enqueued.  Then, for the flagged envs alone: their rings are wiped on the
// device, they count as "consumed everything uploaded", the feeder restarts their streams (reseed_envs), and the refill pass that follows finds them with
// nothing resident and therefore WAITS for their next episode -- the first of the new stream -- and uploads it (upload_pass: `must`): a reset of either form
// that comes next finds it there, however many seed / reset pairs follow each other without a stepping call.
int seed_envs_host_fed(mv_gym *g, const int32_t *host_seeds)
{
    const int N = g->N;
    std::vector<int> envs, first;
    std::vector<uint32_t> values;
    for (int e = 0; e < N; ++e)
        if (host_seeds[e] >= 0) { envs.push_back(e); values.push_back((uint32_t)host_seeds[e]); }
    if (envs.empty()) return 0;   // nobody flagged: nothing to wait for, nothing to launch
    HIP_TRY(hipSetDevice(g->device));
    if (sim_join(g)) return -1;
    if (sync_status_words(g)) return -1;
    const int32_t *device_seeds = nullptr;
    if (g->seedEnvsPair.stage(host_seeds, (size_t)g->N * sizeof(int32_t), g->stream, &device_seeds)) return -1;
    const int slots = N * g->spares;
    hipLaunchKernelGGL(ring_wipe_envs_kernel, dim3((slots + 255) / 256), dim3(256), 0, g->stream, g->dBlobs, g->blobBytes, g->spares, N, device_seeds);
    HIP_TRY(hipGetLastError());
    if (g->seedEnvsPair.mark(g->stream)) return -1;
    HIP_TRY(hipStreamSynchronize(g->stream));   // (the uploads below travel on other streams: the wipe is done before the first of them starts)
    for (int e : envs) {
        g->uploaded[(size_t)e] = g->hStatus[e];
        first.push_back(g->hStatus[e] + 1);
    }
    g->feeder->reseed_envs(envs, values, first);
    g->refillForce = true;
    if (refill_episodes(g, 1) < 0) return -1;   // every flagged env has the first episode of its new stream resident
    return finish_with_warning(g);
}

}  // namespace

extern "C" {

int mv_seed_envs(mv_gym *g, const int32_t *device_seeds)
{
    if (seed_envs_check(g, device_seeds, "mv_seed_envs")) return -1;
    if (g->hostEpisodes())
        return fail("mv_seed_envs: this scenario's episode generators live on the host, which cannot read a device array without waiting for it: "
                    "use mv_seed_envs_host (the device form serves TowerBuilding, whose generators live on the device)");
    return seed_envs_tower(g, device_seeds, nullptr);
}

int mv_seed_envs_host(mv_gym *g, const int32_t *seeds)
{
    if (seed_envs_check(g, seeds, "mv_seed_envs_host")) return -1;
    return g->hostEpisodes() ? seed_envs_host_fed(g, seeds) : seed_envs_tower(g, nullptr, seeds);
}

// Host-only test hook: drives an EpisodeFeeder without a device through a script and checks every episode it delivers against straight sequential
// generation -- a model generator per env, re-seeded where the script re-seeds the env (Sokoban: its level list is carried across the re-seed, advanced by
// the delivered episodes alone).  script: n_ops x {op, env, value}.  op 0: take env's next episode (wait_ready, compare, copy to out, recycle).  op 1: put
// (env, value) on the pending re-seed list.  op 2: one reseed_envs call with the pending list.  out (may be null): one record of record_bytes per take, in
// script order; used_out (may be null): the bytes of each the feeder reported as used.  Returns the number of takes; out == null && script == null: the
// record size.
int mv_debug_feeder_reseed_script(const char *scenario_name, int32_t num_envs, int32_t num_agents, int32_t threads, const int32_t *env_seeds,
                                  const int32_t *script, int32_t n_ops, void *out, int64_t out_bytes, int32_t *used_out)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    if (!scenario_name || !scenario_from_name(lower(scenario_name), scenario, oc) || scenario == SCN_TOWER)
        return fail("mv_debug_feeder_reseed_script: a host-generated scenario");
    const ScenarioRow &row = scenario_row(scenario);
    const size_t bytes = row.record_bytes;
    if (!script && !out) return (int)bytes;
    if (num_envs < 1 || num_agents < 1 || num_agents > MAX_AGENTS || !env_seeds || !script || n_ops < 0)
        return fail("mv_debug_feeder_reseed_script: bad arguments");
    std::vector<std::string> files;
    if (scenario == SCN_SOKOBAN) {
        files = find_boxoban_level_files();
        if (files.empty()) return fail("mv_debug_feeder_reseed_script: no Boxoban levels found (BOXOBAN_LEVELS)");
    }
    const float len = 60.0f;
    std::vector<uint8_t> slots((size_t)num_envs * bytes, 0), want(bytes);
    std::vector<std::mt19937> rng((size_t)num_envs);
    std::vector<SokobanLevels> levels(scenario == SCN_SOKOBAN ? (size_t)num_envs : 0);
    std::vector<int> consumed((size_t)num_envs, 0);
    std::vector<uint32_t> seeds((size_t)num_envs);
    for (int i = 0; i < num_envs; ++i) {
        if (env_seeds[i] < 0) return fail("mv_debug_feeder_reseed_script: a negative seed");
        seeds[(size_t)i] = (uint32_t)env_seeds[i];
        rng[(size_t)i].seed((unsigned long)seeds[(size_t)i]);
    }
    EpisodeFeeder feeder(scenario, oc, num_envs, num_agents, len, slots.data(), bytes, 0, threads, files);
    feeder.reseed(seeds, std::vector<int>((size_t)num_envs, 1));
    std::vector<int> pendEnvs, pendFirst;
    std::vector<uint32_t> pendValues;
    int takes = 0;
    for (int k = 0; k < n_ops; ++k) {
        const int op = script[3 * k], env = script[3 * k + 1], value = script[3 * k + 2];
        if (op == 2) {
            for (size_t j = 0; j < pendEnvs.size(); ++j) rng[(size_t)pendEnvs[j]].seed((unsigned long)pendValues[j]);
            feeder.reseed_envs(pendEnvs, pendValues, pendFirst);
            pendEnvs.clear(); pendValues.clear(); pendFirst.clear();
            continue;
        }
        if (env < 0 || env >= num_envs || (op != 0 && op != 1) || (op == 1 && value < 0)) return fail("mv_debug_feeder_reseed_script: bad script entry");
        if (op == 1) {
            pendEnvs.push_back(env); pendValues.push_back((uint32_t)value); pendFirst.push_back(consumed[(size_t)env] + 1);
            continue;
        }
        const int seq = consumed[(size_t)env] + 1;
        size_t used = 0;
        const uint8_t *got = feeder.wait_ready(env, seq, &used);
        if (!got) return fail("mv_debug_feeder_reseed_script: episode not delivered");
        if (used > bytes) return fail("mv_debug_feeder_reseed_script: used bytes out of range");
        std::memset(want.data(), 0, bytes);
        SokobanLevels *lv = levels.empty() ? nullptr : &levels[(size_t)env];
        if (!generate_episode(row, GenContext{rng[(size_t)env], oc, num_agents, len, lv, &files}, seq, want.data()))
            return fail("mv_debug_feeder_reseed_script: unreadable level file");
        const bool same = episodes_equal(row, got, want.data(), used, num_agents);
        if (!same)
            return fail("mv_debug_feeder_reseed_script: episode " + std::to_string(seq) + " of env " + std::to_string(env) +
                        " differs from sequential generation (script entry " + std::to_string(k) + ")");
        if (out) {
            if ((int64_t)((size_t)(takes + 1) * bytes) > out_bytes) return fail("mv_debug_feeder_reseed_script: buffer too small");
            std::memcpy(static_cast<uint8_t *>(out) + (size_t)takes * bytes, got, bytes);
        }
        if (used_out) used_out[takes] = (int32_t)used;
        ++takes;
        ++consumed[(size_t)env];
        feeder.recycle(env, nullptr);
    }
    return takes;
}

}  // extern "C"
