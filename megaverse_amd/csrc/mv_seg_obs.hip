// megaverse_amd/csrc/mv_seg_obs.hip -- segmentation observations: the host side of mv_set_seg_obs / mv_get_seg_obs / mv_get_seg_format /
// mv_get_seg_observation / mv_seg_class_name (include/megaverse_hip.h), the ONE launch that follows a fast pass of a gym with labels attached (labels, or
// depth + labels), and the record's host twins mv_debug_seg_rule_host, mv_debug_seg_bounds_host and mv_debug_seg_pack_host.
// The record and its rule: mv_seg_obs.h.  The kernels: mv_raster.hip (raster_seg_kernel).  DESIGN.md 3.21 says which passes write planes.
#include "mv_api_internal.h"
#include "mv_seg_obs.h"

static_assert((int)MV_SEG_CLASS_U8 == (int)SEG_CLASS_U8 && (int)MV_SEG_INSTANCE_U16 == (int)SEG_INSTANCE_U16, "the header's formats are the record's");

namespace mvapi {

// The planes of the frames a fast pass of v has just drawn: the labels -> `planes` (OutPtrs::seg) and, where depth observations are attached too, the depth
// -> `depth` (OutPtrs::depth), with ONE launch on the caller's stream, reading v's frame lists (the call's slots: the mark that frees them is recorded behind
// this).  The follower of a gym with labels attached: depth_obs_follow is not called beside it.  -> 1: launched, 0: nothing to do, -1: failed
int seg_obs_follow(mv_gym *g, const GymView &v, void *depth, void *planes, const char *who)
{
    if (!g->seg.buf || !planes) return 0;
    if (launch_raster_seg(v, g->depth.buf ? depth : nullptr, g->depth.format, planes, g->seg.format, g->w, g->h, g->stream))
        return fail(std::string(who) + ": observation size above 1024x1024");
    HIP_TRY(hipGetLastError());
    return 1;
}

}  // namespace mvapi

extern "C" {

int mv_set_seg_obs(mv_gym *g, void *device_buf, int32_t format)
{
    const GymOption &opt = gym_options[OPT_SEG_OBS];
    if (attach_check(g, opt.setter, opt)) return -1;
    if (!device_buf) {
        // No launch, no copy: the launches enqueued so far keep the pointers they were given; the next pass writes no plane.
        g->seg = SegObs();
        g->simMustWaitUser = true;
        return 0;
    }
    if (!seg_format_known(format)) return fail("mv_set_seg_obs: unknown format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)");
    if (g->stillOn)   // (a still frame's rows are carried from the entry that holds them; nothing carries its label plane)
        return fail("mv_set_seg_obs: still frames are switched on (mv_set_still_frames), and a still frame's label plane would not be carried: switch them off first");
    if (format == SEG_INSTANCE_U16 && (uintptr_t)device_buf % 2) return fail("mv_set_seg_obs: a MV_SEG_INSTANCE_U16 buffer must be 2-byte aligned");
    g->seg.buf = device_buf;
    g->seg.format = format;
    g->seg.entries = std::max(1, g->ringCount);
    g->seg.entryBytes = (size_t)g->N * g->A * seg_plane_bytes(g->w, g->h, format);
    g->simMustWaitUser = true;   // an ordering point, as mv_set_depth_obs: the next step launch comes behind what the caller's stream holds now
    return 0;
}

int mv_get_seg_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_seg_obs")) return -1;
    return g->seg.buf ? g->seg.entries : 0;
}

int mv_get_seg_format(const mv_gym *g)
{
    if (getter_check(g, "mv_get_seg_format")) return -1;
    return g->seg.buf ? g->seg.format : -1;
}

int mv_get_seg_observation(mv_gym *g, int32_t env, int32_t agent, uint16_t *out)
{
    const std::string who = "mv_get_seg_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->seg.buf) return fail(who + ": no segmentation observations attached (mv_set_seg_obs)");
    if (!out) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t px = (size_t)g->w * g->h, bytes = seg_plane_bytes(g->w, g->h, g->seg.format);
    const uint8_t *src = (const uint8_t *)last_outputs(g).seg + ((size_t)env * g->A + agent) * bytes;
    if (g->seg.format == SEG_INSTANCE_U16) {
        HIP_TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        return 0;
    }
    std::vector<uint8_t> classes(px);
    HIP_TRY(hipMemcpyAsync(classes.data(), src, bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    for (size_t i = 0; i < px; ++i) out[i] = classes[i];
    return 0;
}

const char *mv_seg_class_name(int32_t cls) { return seg_class_name(cls); }

int mv_debug_seg_bounds_host(int32_t scenario, int32_t L, int32_t W, int32_t num_boxes, int32_t num_terrain, int32_t num_objects, int32_t num_rewards,
                             int32_t num_agents, int32_t *out5)
{
    if (!out5) return fail("mv_debug_seg_bounds_host: null pointer");
    const SegBounds b = seg_bounds(scenario, L, W, num_boxes, num_terrain, num_objects, num_rewards, num_agents);
    out5[0] = b.terrain; out5[1] = b.objects; out5[2] = b.rewards; out5[3] = b.agents; out5[4] = b.end;
    return 0;
}

int mv_debug_seg_rule_host(int32_t scenario, int32_t slot, const int32_t *boundaries5, int32_t subtype, int32_t format, void *out)
{
    if (!boundaries5 || !out) return fail("mv_debug_seg_rule_host: null pointer");
    if (!seg_format_known(format)) return fail("mv_debug_seg_rule_host: unknown format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)");
    const SegBounds b = {boundaries5[0], boundaries5[1], boundaries5[2], boundaries5[3], boundaries5[4]};
    const uint16_t w = seg_rule(scenario, slot, b, subtype);
    if (format == SEG_INSTANCE_U16) *reinterpret_cast<uint16_t *>(out) = w;
    else *reinterpret_cast<uint8_t *>(out) = seg_bits_u8(w);
    return 0;
}

int mv_debug_seg_pack_host(const int32_t *cls, const int32_t *instance, int32_t n, int32_t format, void *out)
{
    if (!cls || !instance || !out || n < 0) return fail("mv_debug_seg_pack_host: null pointer or n < 0");
    if (!seg_format_known(format)) return fail("mv_debug_seg_pack_host: unknown format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)");
    for (int i = 0; i < n; ++i)
        if (cls[i] < 0 || cls[i] >= SEG_NUM_CLASSES || instance[i] < 0 || instance[i] >= SEG_MAX_INSTANCES)
            return fail("mv_debug_seg_pack_host: class outside [0, 15) or instance outside [0, 4096)");
    seg_pack_host(cls, instance, n, format, out);
    return 0;
}

}  // extern "C"
