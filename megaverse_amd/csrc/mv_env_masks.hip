// megaverse_amd/csrc/mv_env_masks.hip -- step masks and draw masks: the host side of mv_set_step_mask / mv_set_step_mask_host / mv_get_step_mask and of
// mv_set_draw_mask / mv_set_draw_mask_host / mv_get_draw_mask (include/megaverse_hip.h).  Both are [N] bytes, attached until replaced or detached, in the
// same two forms (mv_api_internal.h: EnvMask); they differ in who reads them.
// Step mask: the step kernels (mv_step_kernels.h: env_frozen, frozen_tick) and the episode log's update (mv_episode_log.h: episode_log_steps); DESIGN.md 3.10
// says what a frozen tick writes and where these calls stand in the streams' order.
// Draw mask: the frame setups -- the MASKED step kernels (mv_step_kernels.h: env_drawn) and frame_setup_kernel (mv_raster.hip) -- which take frame_skip
// (mv_frame.h) for the frames of an undrawn env; the observation pass reads no mask: the frame's header says "undrawn".  DESIGN.md 3.13 says what a skipped
// frame writes, where the pass's workgroups leave and where these calls stand in the streams' order.
#include "mv_api_internal.h"

namespace {

// Form 1 (null: detach).  No launch, no copy: the kernels read the caller's buffer.  The call is the ordering point (the wrappers say of what).
int set_device(mv_gym *g, EnvMask &m, const uint8_t *device_mask)
{
    m.live = device_mask;
    m.form = device_mask ? 1 : 0;
    g->simMustWaitUser = true;
    return 0;
}

// Form 2: the caller's bytes into the gym's own buffer, through the pool
int set_host(mv_gym *g, EnvMask &m, const uint8_t *mask, const char *who)
{
    HIP_TRY(hipSetDevice(g->device));
    const size_t N = (size_t)g->N;
    if (!m.owned) {
        hipError_t e_ = hipMalloc((void **)&m.owned, N);
        if (e_ != hipSuccess) { m.owned = nullptr; return fail(std::string(who) + ": hipMalloc of " + std::to_string(N) + " bytes: " + hipGetErrorString(e_)); }
        m.ownedBytes = N;
    }
    StagingPool::Buffer *s = nullptr;
    if (m.pool.take(N, who, s)) return -1;
    std::memcpy(s->host, mask, N);
    // The copy goes to the caller's stream behind every step launch enqueued so far (sim_join: a step kernel or frame setup running ahead on the simulation
    // stream never sees a half-written mask) and behind the episode log's last update, which lives on that stream and reads the step mask; the next step
    // launch waits for it (simMustWaitUser, set by sim_join).
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(m.owned, s->host, N, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(s->copied, g->stream));
    m.live = m.owned;
    m.form = 2;
    return 0;
}

void release(EnvMask &m)
{
    m.pool.release();
    if (m.owned) (void)hipFree(m.owned);
    m = EnvMask{};
}

}  // namespace

void mvapi::env_masks_free(mv_gym *g)
{
    release(g->stepMask);
    release(g->drawMask);
}

extern "C" {

int mv_set_step_mask(mv_gym *g, const uint8_t *device_mask)
{
    if (attach_check(g, "mv_set_step_mask", gym_options[OPT_STEP_MASK])) return -1;
    // No launch, no copy: the step kernels read the caller's buffer.  This call is the ordering point, as mv_set_action_ring is: what the caller's stream holds
    // now -- the kernel that wrote the mask -- comes before the next step launch; the calls after that one pipeline freely.
    return set_device(g, g->stepMask, device_mask);
}

int mv_set_step_mask_host(mv_gym *g, const uint8_t *mask)
{
    if (attach_check(g, "mv_set_step_mask_host", gym_options[OPT_STEP_MASK])) return -1;
    return mask ? set_host(g, g->stepMask, mask, "mv_set_step_mask_host") : set_device(g, g->stepMask, nullptr);
}

int mv_get_step_mask(const mv_gym *g) { return getter_check(g, "mv_get_step_mask") ? -1 : g->stepMask.form; }

int mv_set_draw_mask(mv_gym *g, const uint8_t *device_mask)
{
    if (attach_check(g, "mv_set_draw_mask", gym_options[OPT_DRAW_MASK])) return -1;
    // No launch, no copy: the frame setups read the caller's buffer.  This call is the ordering point, as mv_set_step_mask is: what the caller's stream holds
    // now -- the kernel that wrote the mask -- comes before the next step launch (the frame setups of mv_render and of the frame behind a reset run on the
    // caller's stream itself); the calls after that one pipeline freely.
    return set_device(g, g->drawMask, device_mask);
}

int mv_set_draw_mask_host(mv_gym *g, const uint8_t *mask)
{
    if (attach_check(g, "mv_set_draw_mask_host", gym_options[OPT_DRAW_MASK])) return -1;
    return mask ? set_host(g, g->drawMask, mask, "mv_set_draw_mask_host") : set_device(g, g->drawMask, nullptr);
}

int mv_get_draw_mask(const mv_gym *g) { return getter_check(g, "mv_get_draw_mask") ? -1 : g->drawMask.form; }

}  // extern "C"
