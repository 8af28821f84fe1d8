// megaverse_amd/csrc/mv_scene_obs.hip -- scene observations: the host side of mv_set_scene_obs / mv_get_scene_obs / mv_get_scene_observation
// (include/megaverse_hip.h), the per-slot staging rows, the launch that carries a stepping call's rows to the caller's buffer -- the state observations' rows
// with them when both records are attached -- the gather behind a reset or mv_render, and the record's host twin mv_debug_scene_obs_host.  The record is
// mv_scene_obs.h; the MASKED step kernels write the staging rows (mv_step_kernels.h: scene_obs_write).  DESIGN.md 3.19 says where the rows are written and
// where publication stands in the streams' order.
#include "mv_api_internal.h"
#include "mv_scene_obs.h"

static_assert((int)MV_SCENE_OBS_FLOATS == (int)SCENE_OBS_FLOATS, "the header's row length is the record's");

namespace {

// The k ticks of one stepping call with ONE launch, for both records (mv_state_obs.hip: publish_state_ticks_kernel carries the state rows of a gym without
// scene observations): thread i < scene_words carries word i of every tick's staged scene rows to that tick's entry of the caller's buffer, in ascending tick
// order -- without an output ring every tick's entry is the one entry and the last tick's rows stay; the threads behind them do the same for the
// state_words words of the state rows (0: that record is off).
struct PublishRowsArgs {
    int32_t k, scene_words, state_words, pad;
    const uint32_t *scene_src[PIPE_BATCH_MAX];
    uint32_t *scene_dst[PIPE_BATCH_MAX];
    const uint32_t *state_src[PIPE_BATCH_MAX];
    uint32_t *state_dst[PIPE_BATCH_MAX];
};
static_assert(sizeof(PublishRowsArgs) <= 4096, "PublishRowsArgs must fit the 4 KB kernel-argument segment");
__global__ __launch_bounds__(256) void publish_rows_ticks_kernel(PublishRowsArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.scene_words) {
        for (int j = 0; j < a.k; ++j) a.scene_dst[j][i] = a.scene_src[j][i];
    } else if (i - a.scene_words < a.state_words) {
        const int s = i - a.scene_words;
        for (int j = 0; j < a.k; ++j) a.state_dst[j][s] = a.state_src[j][s];
    }
}

// the rows of the current state (behind mv_reset, mv_reset_envs(render = 1), mv_render): thread i packs word i of [N][32]; mask != null: only the rows of the
// envs it flags, the others keep what they hold.  The Obstacles family's columns 16..23 take the record's loops (scene_obs_scan), each thread its own: at most
// 16 boxes and the env's reward slots, behind calls that draw every frame of the gym.
__global__ __launch_bounds__(256) void scene_obs_gather_kernel(GymView gv, const uint8_t *__restrict__ mask, uint32_t *__restrict__ rows, int words)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    const int env = i / SCENE_OBS_FLOATS, f = i % SCENE_OBS_FLOATS;
    if (mask != nullptr && mask[env] == 0) return;
    const EnvHeader *h = gv.hdr + env;
    const TerrainBox *terrain = gv.terrain + (size_t)env * MAX_TERRAIN;
    const MovableObject *rewards = gv.rewards_obj + (size_t)env * gv.reward_stride;
    SceneObsScan scan = {0, -1, 0};
    if (gv.scenario == SCN_OBSTACLES && f >= SCENE_OBS_SCENARIO_COL && f <= SCENE_OBS_SCENARIO_COL + 7) scan = scene_obs_scan(h, terrain, rewards);
    rows[i] = scene_obs_word(gv.scenario, h, terrain, rewards, gv.fb + env, scan, f);
}

int scene_obs_check(mv_gym *g, const char *who)
{
    if (check(g)) { g_err = std::string(who) + ": " + g_err; return -1; }
    if (g->inGroup) return fail(std::string(who) + ": this gym belongs to an mv_group, whose union launches write no scene observations");
    return 0;
}

size_t scene_obs_words(const mv_gym *g) { return (size_t)g->N * SCENE_OBS_FLOATS; }

}  // namespace

namespace mvapi {

// tick `tick`'s entry of the caller's buffer: the entry its rewards go to (outputs_of)
float *scene_obs_entry(const mv_gym *g, unsigned long long tick)
{
    return g->sceneObs + (size_t)(tick % (unsigned long long)g->sceneEntries) * scene_obs_words(g);
}

int scene_obs_publish(mv_gym *g, int q0, float *const *scene_dst, float *const *state_dst, int k)   // on the caller's stream
{
    PublishRowsArgs a;
    a.k = k; a.pad = 0;
    a.scene_words = (int32_t)scene_obs_words(g);
    a.state_words = state_dst ? (int32_t)state_obs_words(g) : 0;
    for (int j = 0; j < (int)PIPE_BATCH_MAX; ++j) {
        const int jj = std::min(j, k - 1);
        const GymView &v = g->gvp[(size_t)(q0 + jj)];
        a.scene_src[j] = reinterpret_cast<const uint32_t *>(v.scene_obs);
        a.scene_dst[j] = reinterpret_cast<uint32_t *>(scene_dst[jj]);
        a.state_src[j] = state_dst ? reinterpret_cast<const uint32_t *>(v.state_obs) : nullptr;
        a.state_dst[j] = state_dst ? reinterpret_cast<uint32_t *>(state_dst[jj]) : nullptr;
    }
    hipLaunchKernelGGL(publish_rows_ticks_kernel, dim3((a.scene_words + a.state_words + 255) / 256), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int scene_obs_refresh(mv_gym *g, const uint8_t *device_mask)   // on the caller's stream, behind sim_join
{
    if (!g->sceneObs) return 0;
    const int words = (int)scene_obs_words(g);
    hipLaunchKernelGGL(scene_obs_gather_kernel, dim3((words + 255) / 256), dim3(256), 0, g->stream, g->gv, device_mask,
                       reinterpret_cast<uint32_t *>(scene_obs_entry(g, g->ringTick ? g->ringTick - 1 : 0)), words);
    HIP_TRY(hipGetLastError());
    return 0;
}

void scene_obs_free(mv_gym *g)
{
    if (g->sceneStage) (void)hipFree(g->sceneStage);
    g->sceneStage = nullptr; g->sceneBytes = 0;
    g->sceneObs = nullptr; g->sceneEntries = 0;
    for (GymView &v : g->gvp) v.scene_obs = nullptr;
}

}  // namespace mvapi

extern "C" {

int mv_set_scene_obs(mv_gym *g, float *device_buf)
{
    if (scene_obs_check(g, "mv_set_scene_obs")) return -1;
    if (device_buf && !g->sceneStage) {
        // The staging rows, one set per hand-over slot, an allocation of their own as the state rows are: the arena's layout and the slot stride the passes
        // derive stay what they are.  Kept until mv_close: launches in flight may still write rows after a detach.
        HIP_TRY(hipSetDevice(g->device));
        const size_t bytes = (size_t)g->slots * scene_obs_words(g) * sizeof(float);
        hipError_t e_ = hipMalloc((void **)&g->sceneStage, bytes);
        if (e_ != hipSuccess) { g->sceneStage = nullptr; return fail("mv_set_scene_obs: hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
        g->sceneBytes = bytes;
    }
    // No launch, no copy: mv_set_state_obs's ordering point.
    for (int q = 0; q < g->slots; ++q) g->gvp[(size_t)q].scene_obs = device_buf ? g->sceneStage + (size_t)q * scene_obs_words(g) : nullptr;
    g->sceneObs = device_buf;
    g->sceneEntries = device_buf ? std::max(1, g->ringCount) : 0;
    g->simMustWaitUser = true;
    return 0;
}

int mv_get_scene_obs(const mv_gym *g)
{
    if (!g) return fail("mv_get_scene_obs: null gym handle");
    if (g->closed) return fail("mv_get_scene_obs: gym is closed");
    return g->sceneObs ? g->sceneEntries : 0;
}

int mv_get_scene_observation(mv_gym *g, int32_t env, float *out32)
{
    if (check(g)) { g_err = "mv_get_scene_observation: " + g_err; return -1; }
    if (!g->sceneObs) return fail("mv_get_scene_observation: no scene observations attached (mv_set_scene_obs)");
    if (!out32) return fail("mv_get_scene_observation: null pointer");
    if (env < 0 || env >= g->N) return fail("mv_get_scene_observation: index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const float *row = scene_obs_entry(g, g->ringTick ? g->ringTick - 1 : 0) + (size_t)env * SCENE_OBS_FLOATS;
    HIP_TRY(hipMemcpyAsync(out32, row, SCENE_OBS_FLOATS * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_scene_obs_host(int32_t scenario, const void *env_header, const void *terrain16, const void *rewards, int32_t rewards_len,
                            const void *football_state, float *out32)
{
    if (!env_header || !out32) return fail("mv_debug_scene_obs_host: null pointer");
    EnvHeader h;   // (the caller's bytes need not be aligned)
    std::memcpy(&h, env_header, sizeof h);
    TerrainBox terrain[MAX_TERRAIN] = {};
    MovableObject rw[COLLECT_MAX_REWARDS] = {};
    FootballState fb = {};
    if (scenario == SCN_OBSTACLES) {
        if (rewards_len < 0 || rewards_len > (int)COLLECT_MAX_REWARDS) return fail("mv_debug_scene_obs_host: 0 <= rewards_len <= 96 required");
        if (h.num_terrain < 0 || h.num_terrain > (int)MAX_TERRAIN || (h.num_terrain > 0 && !terrain16))
            return fail("mv_debug_scene_obs_host: the header's num_terrain needs a list of 16 terrain boxes");
        if (h.num_rewards < 0 || h.num_rewards > rewards_len || (h.num_rewards > 0 && !rewards))
            return fail("mv_debug_scene_obs_host: the header's num_rewards exceeds rewards_len");
        if (terrain16) std::memcpy(terrain, terrain16, sizeof terrain);
        if (rewards && rewards_len > 0) std::memcpy(rw, rewards, (size_t)rewards_len * sizeof(MovableObject));
    }
    if (scenario == SCN_FOOTBALL) {
        if (!football_state) return fail("mv_debug_scene_obs_host: Football needs a FootballState");
        std::memcpy(&fb, football_state, sizeof fb);
    }
    uint32_t row[SCENE_OBS_FLOATS];
    scene_obs_pack(scenario, &h, terrain, rw, &fb, row);
    std::memcpy(out32, row, sizeof row);
    return 0;
}

}  // extern "C"
