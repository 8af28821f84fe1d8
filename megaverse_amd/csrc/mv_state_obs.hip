// megaverse_amd/csrc/mv_state_obs.hip -- state observations: the host side of mv_set_state_obs / mv_get_state_obs / mv_get_state_observation
// (include/megaverse_hip.h), the per-slot staging rows, the launch that carries a stepping call's rows to the caller's buffer, the gather behind a reset or
// mv_render, and the record's host twin mv_debug_state_obs_host.  The record is mv_state_obs.h; the MASKED step kernels write the staging rows
// (mv_step_kernels.h: state_obs_write).  DESIGN.md 3.14 says where the rows are written and where publication stands in the streams' order.
#include "mv_api_internal.h"
#include "mv_state_obs.h"

static_assert((int)MV_STATE_OBS_FLOATS == (int)STATE_OBS_FLOATS, "the header's row length is the record's");

namespace {

// The k ticks of one stepping call with ONE launch, publish_ticks_kernel's sibling: thread i carries word i of every tick's staged rows to that tick's entry
// of the caller's buffer, in ascending tick order -- without an output ring every tick's entry is the one entry and the last tick's rows stay.
struct PublishStateArgs {
    int32_t k, words;
    const uint32_t *src[PIPE_BATCH_MAX];
    uint32_t *dst[PIPE_BATCH_MAX];
};
__global__ __launch_bounds__(256) void publish_state_ticks_kernel(PublishStateArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.words) return;
    for (int j = 0; j < a.k; ++j) a.dst[j][i] = a.src[j][i];
}

// the rows of the current state (behind mv_reset, mv_reset_envs(render = 1), mv_render): thread i packs word i of [N*A][16]; mask != null: only the rows of
// the envs it flags, the others keep what they hold
__global__ __launch_bounds__(256) void state_obs_gather_kernel(const AgentState *__restrict__ agents, const EnvHeader *__restrict__ hdr,
                                                               const uint8_t *__restrict__ mask, uint32_t *__restrict__ rows, int A, int words)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    const int agent = i >> 4, env = agent / A;
    if (mask != nullptr && mask[env] == 0) return;
    rows[i] = state_obs_word(agents + agent, hdr + env, i & (STATE_OBS_FLOATS - 1));
}

int state_obs_check(mv_gym *g, const char *who)
{
    if (check(g)) { g_err = std::string(who) + ": " + g_err; return -1; }
    if (g->inGroup) return fail(std::string(who) + ": this gym belongs to an mv_group, whose union launches write no state observations");
    return 0;
}

}  // namespace

namespace mvapi {

size_t state_obs_words(const mv_gym *g) { return (size_t)g->N * g->A * STATE_OBS_FLOATS; }

// tick `tick`'s entry of the caller's buffer: the entry its rewards go to (outputs_of)
float *state_obs_entry(const mv_gym *g, unsigned long long tick)
{
    return g->stateObs + (size_t)(tick % (unsigned long long)g->stateEntries) * state_obs_words(g);
}

int state_obs_publish(mv_gym *g, int q0, float *const *dst, int k)   // on the caller's stream
{
    PublishStateArgs a;
    a.k = k; a.words = (int32_t)state_obs_words(g);
    for (int j = 0; j < (int)PIPE_BATCH_MAX; ++j) {
        const int jj = std::min(j, k - 1);
        a.src[j] = reinterpret_cast<const uint32_t *>(g->gvp[(size_t)(q0 + jj)].state_obs);
        a.dst[j] = reinterpret_cast<uint32_t *>(dst[jj]);
    }
    hipLaunchKernelGGL(publish_state_ticks_kernel, dim3((a.words + 255) / 256), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int state_obs_refresh(mv_gym *g, const uint8_t *device_mask)   // on the caller's stream, behind sim_join
{
    if (!g->stateObs) return 0;
    const int words = (int)state_obs_words(g);
    hipLaunchKernelGGL(state_obs_gather_kernel, dim3((words + 255) / 256), dim3(256), 0, g->stream, g->gv.agents, g->gv.hdr, device_mask,
                       reinterpret_cast<uint32_t *>(state_obs_entry(g, g->ringTick ? g->ringTick - 1 : 0)), g->A, words);
    HIP_TRY(hipGetLastError());
    return 0;
}

void state_obs_free(mv_gym *g)
{
    if (g->stateStage) (void)hipFree(g->stateStage);
    g->stateStage = nullptr;
    g->stateObs = nullptr; g->stateEntries = 0;
    for (GymView &v : g->gvp) v.state_obs = nullptr;
}

}  // namespace mvapi

extern "C" {

int mv_set_state_obs(mv_gym *g, float *device_buf)
{
    if (state_obs_check(g, "mv_set_state_obs")) return -1;
    if (device_buf && !g->stateStage) {
        // The staging rows, one set per hand-over slot, allocated here and not out of the arena: the arena's layout, its size and the slot stride the
        // passes derive stay what they are.  Kept until mv_close: launches in flight may still write rows after a detach.
        HIP_TRY(hipSetDevice(g->device));
        const size_t bytes = (size_t)g->slots * state_obs_words(g) * sizeof(float);
        hipError_t e_ = hipMalloc((void **)&g->stateStage, bytes);
        if (e_ != hipSuccess) { g->stateStage = nullptr; return fail("mv_set_state_obs: hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
    }
    // No launch, no copy.  The step launches enqueued so far keep the views they were given; the next one takes the MASKED kernels (or the unmasked ones
    // again) and is ordered behind whatever the caller's stream holds now, as behind mv_set_step_mask.
    for (int q = 0; q < g->slots; ++q) g->gvp[(size_t)q].state_obs = device_buf ? g->stateStage + (size_t)q * state_obs_words(g) : nullptr;
    g->stateObs = device_buf;
    g->stateEntries = device_buf ? std::max(1, g->ringCount) : 0;
    g->simMustWaitUser = true;
    return 0;
}

int mv_get_state_obs(const mv_gym *g)
{
    if (!g) return fail("mv_get_state_obs: null gym handle");
    if (g->closed) return fail("mv_get_state_obs: gym is closed");
    return g->stateObs ? g->stateEntries : 0;
}

int mv_get_state_observation(mv_gym *g, int32_t env, int32_t agent, float *out16)
{
    if (check(g)) { g_err = "mv_get_state_observation: " + g_err; return -1; }
    if (!g->stateObs) return fail("mv_get_state_observation: no state observations attached (mv_set_state_obs)");
    if (!out16) return fail("mv_get_state_observation: null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail("mv_get_state_observation: index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const float *row = state_obs_entry(g, g->ringTick ? g->ringTick - 1 : 0) + ((size_t)env * g->A + agent) * STATE_OBS_FLOATS;
    HIP_TRY(hipMemcpyAsync(out16, row, STATE_OBS_FLOATS * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_state_obs_host(const void *agent_state, const void *env_header, float *out16)
{
    if (!agent_state || !env_header || !out16) return fail("mv_debug_state_obs_host: null pointer");
    AgentState a;   // (the caller's bytes need not be aligned)
    EnvHeader h;
    std::memcpy(&a, agent_state, sizeof a);
    std::memcpy(&h, env_header, sizeof h);
    uint32_t row[STATE_OBS_FLOATS];
    state_obs_pack(&a, &h, row);
    std::memcpy(out16, row, sizeof row);
    return 0;
}

}  // extern "C"
