// megaverse_amd/csrc/mv_step_mask.hip -- step masks: the host side of mv_set_step_mask / mv_set_step_mask_host / mv_get_step_mask (include/megaverse_hip.h).
// The bytes are read by the step kernels (mv_step_kernels.h: env_frozen, frozen_tick) and by the episode log's update (mv_episode_log.h: episode_log_steps);
// DESIGN.md 3.10 says what a frozen tick writes and where these calls stand in the streams' order.
#include "mv_api_internal.h"

namespace {

// what every form refuses: no gym, a closed one, a member of a group (the union launches read no mask)
int step_mask_check(mv_gym *g, const char *who)
{
    if (check(g)) { g_err = std::string(who) + ": " + g_err; return -1; }
    if (g->inGroup) return fail(std::string(who) + ": this gym belongs to an mv_group, whose union launches read no step mask");
    return 0;
}

// a pinned staging buffer nothing in flight reads: one whose copy has completed (asked, not waited for), else a new one
int step_mask_staging(mv_gym *g, mv_gym::MaskStaging *&out)
{
    out = nullptr;
    for (mv_gym::MaskStaging &s : g->stepMaskStaging)
        if (hipEventQuery(s.copied) == hipSuccess) { out = &s; break; }
    (void)hipGetLastError();   // (hipErrorNotReady of the queries, on every path: it must not surface in a later call's hipGetLastError)
    if (out) return 0;
    mv_gym::MaskStaging s{nullptr, nullptr};
    HIP_TRY(hipHostMalloc((void **)&s.host, (size_t)g->N, hipHostMallocDefault));
    {
        hipError_t e_ = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
        if (e_ != hipSuccess) { (void)hipHostFree(s.host); return fail(std::string("mv_set_step_mask_host: hipEventCreate: ") + hipGetErrorString(e_)); }
    }
    g->stepMaskStaging.push_back(s);
    out = &g->stepMaskStaging.back();
    return 0;
}

}  // namespace

void mvapi::step_mask_free(mv_gym *g)
{
    for (mv_gym::MaskStaging &s : g->stepMaskStaging) {
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.host) (void)hipHostFree(s.host);
    }
    g->stepMaskStaging.clear();
    if (g->dStepMask) (void)hipFree(g->dStepMask);
    g->dStepMask = nullptr; g->stepMaskBytes = 0;
    g->stepMask = nullptr; g->stepMaskForm = 0;
}

extern "C" {

int mv_set_step_mask(mv_gym *g, const uint8_t *device_mask)
{
    if (step_mask_check(g, "mv_set_step_mask")) return -1;
    // No launch, no copy: the step kernels read the caller's buffer.  This call is the ordering point, as mv_set_action_ring is: what the caller's stream holds
    // now -- the kernel that wrote the mask -- comes before the next step launch; the calls after that one pipeline freely.
    g->stepMask = device_mask;
    g->stepMaskForm = device_mask ? 1 : 0;
    g->simMustWaitUser = true;
    return 0;
}

int mv_set_step_mask_host(mv_gym *g, const uint8_t *mask)
{
    if (step_mask_check(g, "mv_set_step_mask_host")) return -1;
    if (!mask) return mv_set_step_mask(g, nullptr);
    HIP_TRY(hipSetDevice(g->device));
    const size_t N = (size_t)g->N;
    if (!g->dStepMask) {
        hipError_t e_ = hipMalloc((void **)&g->dStepMask, N);
        if (e_ != hipSuccess) { g->dStepMask = nullptr; return fail("mv_set_step_mask_host: hipMalloc of " + std::to_string(N) + " bytes: " + hipGetErrorString(e_)); }
        g->stepMaskBytes = N;
    }
    mv_gym::MaskStaging *s = nullptr;
    if (step_mask_staging(g, s)) return -1;
    std::memcpy(s->host, mask, N);
    // The copy goes to the caller's stream behind every step launch enqueued so far (sim_join: a step kernel running ahead on the simulation stream never
    // sees a half-written mask) and behind the episode log's last update, which lives on that stream; the next step launch waits for it (simMustWaitUser).
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(g->dStepMask, s->host, N, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(s->copied, g->stream));
    g->stepMask = g->dStepMask;
    g->stepMaskForm = 2;
    return 0;
}

int mv_get_step_mask(const mv_gym *g)
{
    if (!g) return fail("mv_get_step_mask: null gym handle");
    if (g->closed) return fail("mv_get_step_mask: gym is closed");
    return g->stepMaskForm;
}

}  // extern "C"
