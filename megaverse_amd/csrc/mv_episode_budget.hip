// megaverse_amd/csrc/mv_episode_budget.hip -- episode budgets: the host side of mv_set_episode_budget / mv_set_episode_budget_host and their read-outs
// (include/megaverse_hip.h), the attach kernel, and the rule's host twin mv_debug_episode_budget_host.  The rule is mv_episode_budget.h; the step kernels
// apply it tick by tick (mv_step_kernels.h: env_left, after_tick) and the episode log walks a mirror of it (mv_episode_log.hip: load_done);
// DESIGN.md 3.12 says where these calls stand in the streams' order.
#include "mv_api_internal.h"
#include "mv_episode_budget.h"

namespace mv {
namespace budget {

// The attach: the caller's [N] values into the gym's array and into the log's mirror, and the number of zeros among them into the halted count (zeroed in
// front of this launch; one vector atomic per wave that holds a zero).
__global__ __launch_bounds__(256) void episode_budget_attach_kernel(const int32_t *__restrict__ src, int32_t N, int32_t *__restrict__ left,
                                                                     int32_t *__restrict__ mirror, uint32_t *halted)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool in = e < N;
    const int32_t v = in ? src[e] : -1;
    if (in) { left[e] = v; mirror[e] = v; }
    const unsigned long long zeros = __ballot(in && v == 0);
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(halted, (uint32_t)__popcll(zeros));
}

}  // namespace budget
}  // namespace mv

namespace {

int budget_alloc(mv_gym *g, const char *who)
{
    if (g->budgetLeft) return 0;
    const size_t N = (size_t)g->N, bytes = mv::budget::episode_budget_words(g->N) * sizeof(int32_t);
    hipError_t e_ = hipMalloc((void **)&g->budgetLeft, bytes);
    if (e_ != hipSuccess) { g->budgetLeft = nullptr; return fail(std::string(who) + ": hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
    g->budgetHalted = (uint32_t *)(g->budgetLeft + N);
    g->budgetMirror = g->budgetLeft + N + 1;
    g->budgetBytes = bytes;
    return 0;
}

int budget_detach(mv_gym *g)
{
    // (what is in flight keeps the pointers it was launched with; the next step launch is ordered behind this call as behind an attach)
    g->budgetOn = false;
    g->simMustWaitUser = true;
    return 0;
}

}  // namespace

void mvapi::episode_budget_free(mv_gym *g)
{
    g->budgetPool.release();
    if (g->budgetLeft) (void)hipFree(g->budgetLeft);
    g->budgetLeft = g->budgetMirror = nullptr; g->budgetHalted = nullptr;
    g->budgetBytes = 0; g->budgetOn = false;
}

// mv_set_episode_log switched the log on: while it was off nothing advanced the mirror -- it is the live array again, behind every step launch enqueued so far
int mvapi::episode_budget_seed_mirror(mv_gym *g)
{
    if (!g->budgetOn) return 0;
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(g->budgetMirror, g->budgetLeft, (size_t)g->N * sizeof(int32_t), hipMemcpyDeviceToDevice, g->stream));
    return 0;
}

extern "C" {

int mv_set_episode_budget(mv_gym *g, const int32_t *device_budget)
{
    if (attach_check(g, "mv_set_episode_budget", gym_options[OPT_EPISODE_BUDGET])) return -1;
    if (!device_budget) return budget_detach(g);
    HIP_TRY(hipSetDevice(g->device));
    if (budget_alloc(g, "mv_set_episode_budget")) return -1;
    // On the caller's stream, behind every step launch enqueued so far (sim_join: the kernels write the array this call replaces) and behind the episode log's
    // last update, which lives on that stream and reads the mirror; the next step launch waits for it (simMustWaitUser).
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemsetAsync(g->budgetHalted, 0, sizeof(uint32_t), g->stream));
    hipLaunchKernelGGL(mv::budget::episode_budget_attach_kernel, dim3((unsigned)((g->N + 255) / 256)), dim3(256), 0, g->stream, device_budget, (int32_t)g->N,
                       g->budgetLeft, g->budgetMirror, g->budgetHalted);
    HIP_TRY(hipGetLastError());
    g->budgetOn = true;
    return 0;
}

int mv_set_episode_budget_host(mv_gym *g, const int32_t *budget)
{
    if (attach_check(g, "mv_set_episode_budget_host", gym_options[OPT_EPISODE_BUDGET])) return -1;
    if (!budget) return budget_detach(g);
    HIP_TRY(hipSetDevice(g->device));
    if (budget_alloc(g, "mv_set_episode_budget_host")) return -1;
    // left [N] and the halted count lie behind each other: one copy brings both, a second one the mirror
    const size_t N = (size_t)g->N;
    StagingPool::Buffer *s = nullptr;
    if (g->budgetPool.take((N + 1) * sizeof(int32_t), "mv_set_episode_budget_host", s)) return -1;
    int32_t *host = static_cast<int32_t *>(s->host);
    std::memcpy(host, budget, N * sizeof(int32_t));
    uint32_t zeros = 0;
    for (size_t e = 0; e < N; ++e) zeros += budget[e] == 0 ? 1u : 0u;
    std::memcpy(host + N, &zeros, sizeof zeros);
    if (sim_join(g)) return -1;   // (the order: as the device form's)
    HIP_TRY(hipMemcpyAsync(g->budgetLeft, host, (N + 1) * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->budgetMirror, host, N * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(s->copied, g->stream));
    g->budgetOn = true;
    return 0;
}

int mv_get_episode_budget(const mv_gym *g) { return getter_check(g, "mv_get_episode_budget") ? -1 : g->budgetOn ? 1 : 0; }

void *mv_episode_budget_device_ptr(mv_gym *g) { return g && !g->closed && g->budgetOn ? (void *)g->budgetLeft : nullptr; }
void *mv_halted_count_device_ptr(mv_gym *g) { return g && !g->closed && g->budgetOn ? (void *)g->budgetHalted : nullptr; }

int mv_halted_count(mv_gym *g, int32_t *out)
{
    if (attach_check(g, "mv_halted_count", gym_options[OPT_EPISODE_BUDGET])) return -1;
    if (!out) return fail("mv_halted_count: null output");
    if (!g->budgetOn) return fail("mv_halted_count: no episode budget attached (mv_set_episode_budget)");
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream));   // (every stepping call leaves the caller's stream behind its step launches)
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, g->budgetHalted, sizeof n, hipMemcpyDeviceToHost));
    *out = (int32_t)n;
    return 0;
}

// The rule of mv_episode_budget.h compiled for the CPU (no device): k ticks of N envs.  dones [k][N]: what each tick would stage for an env that steps;
// mask [N] or null; left_in [N].  steps_out [k][N]: 1 where the env steps in the tick; left_out [N]: the budgets behind the last tick.
int mv_debug_episode_budget_host(const uint8_t *dones, const uint8_t *mask, const int32_t *left_in, int32_t k, int32_t N, uint8_t *steps_out, int32_t *left_out)
{
    if (!dones || !left_in || !steps_out || !left_out || k < 0 || N < 1) return fail("mv_debug_episode_budget_host: bad arguments");
    for (int32_t e = 0; e < N; ++e) left_out[e] = left_in[e];
    for (int32_t t = 0; t < k; ++t)
        for (int32_t e = 0; e < N; ++e) {
            const bool steps = mv::budget::episode_budget_steps(mask ? (int)mask[e] : 1, left_out[e]);
            steps_out[(size_t)t * N + e] = steps ? 1 : 0;
            if (steps) (void)mv::budget::episode_budget_spend(left_out[e], dones[(size_t)t * N + e]);
        }
    return 0;
}

}  // extern "C"
