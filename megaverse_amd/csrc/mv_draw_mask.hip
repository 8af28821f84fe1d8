// megaverse_amd/csrc/mv_draw_mask.hip -- draw masks: the host side of mv_set_draw_mask / mv_set_draw_mask_host / mv_get_draw_mask (include/megaverse_hip.h).
// The bytes are read by the frame setups -- the MASKED step kernels (mv_step_kernels.h: env_drawn) and frame_setup_kernel (mv_raster.hip) -- which take
// frame_skip (mv_frame.h) for the frames of an undrawn env; the observation pass reads no mask: the frame's header says "undrawn".  DESIGN.md 3.13 says what a
// skipped frame writes, where the pass's workgroups leave and where these calls stand in the streams' order.
#include "mv_api_internal.h"

namespace {

// what every form refuses: no gym, a closed one, a member of a group (the union launches read no mask)
int draw_mask_check(mv_gym *g, const char *who)
{
    if (check(g)) { g_err = std::string(who) + ": " + g_err; return -1; }
    if (g->inGroup) return fail(std::string(who) + ": this gym belongs to an mv_group, whose union launches read no draw mask");
    return 0;
}

// a pinned staging buffer nothing in flight reads: one whose copy has completed (asked, not waited for), else a new one
int draw_mask_staging(mv_gym *g, mv_gym::MaskStaging *&out)
{
    out = nullptr;
    for (mv_gym::MaskStaging &s : g->drawMaskStaging)
        if (hipEventQuery(s.copied) == hipSuccess) { out = &s; break; }
    (void)hipGetLastError();   // (hipErrorNotReady of the queries, on every path: it must not surface in a later call's hipGetLastError)
    if (out) return 0;
    mv_gym::MaskStaging s{nullptr, nullptr};
    HIP_TRY(hipHostMalloc((void **)&s.host, (size_t)g->N, hipHostMallocDefault));
    {
        hipError_t e_ = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
        if (e_ != hipSuccess) { (void)hipHostFree(s.host); return fail(std::string("mv_set_draw_mask_host: hipEventCreate: ") + hipGetErrorString(e_)); }
    }
    g->drawMaskStaging.push_back(s);
    out = &g->drawMaskStaging.back();
    return 0;
}

}  // namespace

void mvapi::draw_mask_free(mv_gym *g)
{
    for (mv_gym::MaskStaging &s : g->drawMaskStaging) {
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.host) (void)hipHostFree(s.host);
    }
    g->drawMaskStaging.clear();
    if (g->dDrawMask) (void)hipFree(g->dDrawMask);
    g->dDrawMask = nullptr; g->drawMaskBytes = 0;
    g->drawMask = nullptr; g->drawMaskForm = 0;
}

extern "C" {

int mv_set_draw_mask(mv_gym *g, const uint8_t *device_mask)
{
    if (draw_mask_check(g, "mv_set_draw_mask")) return -1;
    // No launch, no copy: the frame setups read the caller's buffer.  This call is the ordering point, as mv_set_step_mask is: what the caller's stream holds
    // now -- the kernel that wrote the mask -- comes before the next step launch (the frame setups of mv_render and of the frame behind a reset run on the
    // caller's stream itself); the calls after that one pipeline freely.
    g->drawMask = device_mask;
    g->drawMaskForm = device_mask ? 1 : 0;
    g->simMustWaitUser = true;
    return 0;
}

int mv_set_draw_mask_host(mv_gym *g, const uint8_t *mask)
{
    if (draw_mask_check(g, "mv_set_draw_mask_host")) return -1;
    if (!mask) return mv_set_draw_mask(g, nullptr);
    HIP_TRY(hipSetDevice(g->device));
    const size_t N = (size_t)g->N;
    if (!g->dDrawMask) {
        hipError_t e_ = hipMalloc((void **)&g->dDrawMask, N);
        if (e_ != hipSuccess) { g->dDrawMask = nullptr; return fail("mv_set_draw_mask_host: hipMalloc of " + std::to_string(N) + " bytes: " + hipGetErrorString(e_)); }
        g->drawMaskBytes = N;
    }
    mv_gym::MaskStaging *s = nullptr;
    if (draw_mask_staging(g, s)) return -1;
    std::memcpy(s->host, mask, N);
    // The copy goes to the caller's stream behind every step launch enqueued so far (sim_join: a frame setup running ahead on the simulation stream never sees
    // a half-written mask); the next step launch waits for it (simMustWaitUser, set by sim_join).
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(g->dDrawMask, s->host, N, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(s->copied, g->stream));
    g->drawMask = g->dDrawMask;
    g->drawMaskForm = 2;
    return 0;
}

int mv_get_draw_mask(const mv_gym *g)
{
    if (!g) return fail("mv_get_draw_mask: null gym handle");
    if (g->closed) return fail("mv_get_draw_mask: gym is closed");
    return g->drawMaskForm;
}

}  // extern "C"
