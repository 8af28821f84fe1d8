// megaverse_amd/csrc/mv_depth_obs.hip -- depth observations: the host side of mv_set_depth_obs / mv_get_depth_obs / mv_get_depth_format /
// mv_get_depth_observation (include/megaverse_hip.h), the launch that follows a fast pass, and the record's host twin mv_debug_depth_pack_host.
// The record and its rule: mv_depth_obs.h.  The kernels: mv_raster.hip (raster_depth_kernel -- the exact pass with a depth plane beside the colours, or with
// the depth plane alone).  DESIGN.md 3.20 says which passes write planes and where the follower stands in the streams' order.
#include "mv_api_internal.h"
#include "mv_depth_obs.h"

static_assert((int)MV_DEPTH_F32 == (int)DEPTH_F32 && (int)MV_DEPTH_F16 == (int)DEPTH_F16, "the header's formats are the record's");

namespace mvapi {

// The planes of the frames a fast pass of v has just drawn -> `planes`, the entry the frames went to: ONE launch of the depth-only kernel on the caller's
// stream, reading v's frame lists (the call's slots: the mark that frees them is recorded behind this).  -> 1: launched, 0: nothing to do, -1: failed
int depth_obs_follow(mv_gym *g, const GymView &v, void *planes, const char *who)
{
    if (!g->depth.buf || !planes) return 0;
    if (launch_raster_depth(v, planes, g->depth.format, g->w, g->h, g->stream)) return fail(std::string(who) + ": observation size above 1024x1024");
    HIP_TRY(hipGetLastError());
    return 1;
}

}  // namespace mvapi

extern "C" {

int mv_set_depth_obs(mv_gym *g, void *device_buf, int32_t format)
{
    const GymOption &opt = gym_options[OPT_DEPTH_OBS];
    if (attach_check(g, opt.setter, opt)) return -1;
    if (!device_buf) {
        // No launch, no copy: the launches enqueued so far keep the pointers they were given; the next pass writes no plane.
        g->depth = DepthObs();
        g->simMustWaitUser = true;
        return 0;
    }
    if (!depth_format_known(format)) return fail("mv_set_depth_obs: unknown format (MV_DEPTH_F32, MV_DEPTH_F16)");
    if (g->stillOn)   // (a still frame's rows are carried from the entry that holds them; nothing carries its depth plane)
        return fail("mv_set_depth_obs: still frames are switched on (mv_set_still_frames), and a still frame's depth plane would not be carried: switch them off first");
    if ((uintptr_t)device_buf % 4) return fail("mv_set_depth_obs: the buffer must be 4-byte aligned");
    g->depth.buf = device_buf;
    g->depth.format = format;
    g->depth.entries = std::max(1, g->ringCount);
    g->depth.entryBytes = (size_t)g->N * g->A * depth_plane_bytes(g->w, g->h, format);
    g->simMustWaitUser = true;   // an ordering point, as mv_set_state_obs: the next step launch comes behind what the caller's stream holds now
    return 0;
}

int mv_get_depth_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_depth_obs")) return -1;
    return g->depth.buf ? g->depth.entries : 0;
}

int mv_get_depth_format(const mv_gym *g)
{
    if (getter_check(g, "mv_get_depth_format")) return -1;
    return g->depth.buf ? g->depth.format : -1;
}

int mv_get_depth_observation(mv_gym *g, int32_t env, int32_t agent, float *out)
{
    const std::string who = "mv_get_depth_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->depth.buf) return fail(who + ": no depth observations attached (mv_set_depth_obs)");
    if (!out) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t px = (size_t)g->w * g->h, bytes = depth_plane_bytes(g->w, g->h, g->depth.format);
    const uint8_t *src = (const uint8_t *)last_outputs(g).depth + ((size_t)env * g->A + agent) * bytes;
    if (g->depth.format == DEPTH_F32) {
        HIP_TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        return 0;
    }
    std::vector<uint16_t> halves(px);
    HIP_TRY(hipMemcpyAsync(halves.data(), src, bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    for (size_t i = 0; i < px; ++i) out[i] = depth_f16_to_f32(halves[i]);
    return 0;
}

int mv_debug_depth_pack_host(const float *t, const uint8_t *hit, int32_t n, int32_t format, void *out)
{
    if (!t || !hit || !out || n < 0) return fail("mv_debug_depth_pack_host: null pointer or n < 0");
    if (!depth_format_known(format)) return fail("mv_debug_depth_pack_host: unknown format (MV_DEPTH_F32, MV_DEPTH_F16)");
    depth_pack_host(t, hit, n, format, out);
    return 0;
}

}  // extern "C"
