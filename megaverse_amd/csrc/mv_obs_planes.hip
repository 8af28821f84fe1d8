// megaverse_amd/csrc/mv_obs_planes.hip -- the three plane records a gym writes per drawn frame, depth observations (mv_depth_obs.h), segmentation
// observations (mv_seg_obs.h) and normal observations (mv_normal_obs.h): the host side of mv_set_*_obs / mv_get_*_obs / mv_get_*_format /
// mv_get_*_observation / mv_seg_class_name (include/megaverse_hip.h), the ONE launch that follows a fast pass of a gym with planes attached (any of the seven
// sets of depth, labels and normals), and the records' host twins mv_debug_depth_pack_host, mv_debug_seg_rule_host, mv_debug_seg_bounds_host,
// mv_debug_seg_pack_host and mv_debug_normal_pack_host.  The sibling of mv_obs_rows.hip.
// The records and their rules: mv_depth_obs.h, mv_seg_obs.h, mv_normal_obs.h.  The kernels: mv_raster.hip (raster_depth_kernel -- the exact pass with planes
// beside the colours, or with the depth plane alone; raster_seg_kernel; raster_normal_kernel).  DESIGN.md 3.20, 3.21 and 3.24 say which passes write planes
// and where the follower stands in the streams' order.
#include "mv_api_internal.h"
#include "mv_depth_obs.h"
#include "mv_seg_obs.h"
#include "mv_normal_obs.h"

static_assert((int)MV_DEPTH_F32 == (int)DEPTH_F32 && (int)MV_DEPTH_F16 == (int)DEPTH_F16, "the header's formats are the record's");
static_assert((int)MV_SEG_CLASS_U8 == (int)SEG_CLASS_U8 && (int)MV_SEG_INSTANCE_U16 == (int)SEG_INSTANCE_U16, "the header's formats are the record's");
static_assert((int)MV_NORMAL_F16 == (int)NORMAL_F16 && (int)MV_NORMAL_SNORM8 == (int)NORMAL_SNORM8, "the header's formats are the record's");

namespace {

// One record as the shared code sees it: its stream (the option with the setter's name, the nouns of the refusal texts), the gym's ObsPlanes, the OutPtrs
// field that carries a tick's entry, the record's rules.
struct Planes {
    const ObsStream &stream;
    ObsPlanes mv_gym::*planes;
    void *OutPtrs::*out;
    const char *getter, *formatGetter, *reader;   // mv_get_*_obs, mv_get_*_format, mv_get_*_observation
    bool (*known)(int format);
    const char *unknown;                          // "unknown format (...)"
    size_t (*planeBytes)(int w, int h, int format);
    size_t (*alignment)(int format);              // of the caller's buffer
    const char *misaligned;
    int native;                                   // the format a read-back hands out as it is (-1: none); every other one is widened, value by value
    void (*widen)(const uint8_t *narrow, size_t px, int format, void *out);
    const GymOption &opt() const { return gym_options[stream.opt]; }
};
const Planes DEPTH = {obs_stream(OPT_DEPTH_OBS), &mv_gym::depth, &OutPtrs::depth, "mv_get_depth_obs", "mv_get_depth_format", "mv_get_depth_observation",
                      +[](int f) { return depth_format_known(f); }, "unknown format (MV_DEPTH_F32, MV_DEPTH_F16)",
                      +[](int w, int h, int f) { return depth_plane_bytes(w, h, f); },
                      +[](int) -> size_t { return 4; }, "the buffer must be 4-byte aligned", DEPTH_F32,
                      +[](const uint8_t *narrow, size_t px, int, void *out) {   // __half -> float
                          uint16_t half;
                          for (size_t i = 0; i < px; ++i) { std::memcpy(&half, narrow + 2 * i, 2); ((float *)out)[i] = depth_f16_to_f32(half); }
                      }};
const Planes SEG = {obs_stream(OPT_SEG_OBS), &mv_gym::seg, &OutPtrs::seg, "mv_get_seg_obs", "mv_get_seg_format", "mv_get_seg_observation",
                    +[](int f) { return seg_format_known(f); }, "unknown format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)",
                    +[](int w, int h, int f) { return seg_plane_bytes(w, h, f); },
                    +[](int f) -> size_t { return f == SEG_INSTANCE_U16 ? 2 : 1; }, "a MV_SEG_INSTANCE_U16 buffer must be 2-byte aligned", SEG_INSTANCE_U16,
                    +[](const uint8_t *narrow, size_t px, int, void *out) {   // uint8 -> uint16
                        for (size_t i = 0; i < px; ++i) ((uint16_t *)out)[i] = narrow[i];
                    }};
const Planes NORMAL = {obs_stream(OPT_NORMAL_OBS), &mv_gym::normal, &OutPtrs::normal, "mv_get_normal_obs", "mv_get_normal_format", "mv_get_normal_observation",
                       +[](int f) { return normal_format_known(f); }, "unknown format (MV_NORMAL_F16, MV_NORMAL_SNORM8)",
                       +[](int w, int h, int f) { return normal_plane_bytes(w, h, f); },
                       +[](int f) -> size_t { return normal_value_bytes(f); }, "the buffer must be 8-byte aligned (MV_NORMAL_F16) or 4-byte aligned (MV_NORMAL_SNORM8)", -1,
                       +[](const uint8_t *narrow, size_t px, int f, void *out) {   // four halves / four signed bytes -> four floats
                           for (size_t i = 0; i < px; ++i) normal_widen_host(narrow + i * normal_value_bytes(f), f, (float *)out + 4 * i);
                       }};
const Planes *const ALL_PLANES[] = {&DEPTH, &SEG, &NORMAL};

int planes_attach(mv_gym *g, const Planes &rec, void *device_buf, int format)
{
    const std::string who = rec.opt().setter;
    if (attach_check(g, rec.opt().setter, rec.opt())) return -1;
    ObsPlanes &p = g->*rec.planes;
    if (!device_buf) {
        // No launch, no copy: the launches enqueued so far keep the pointers they were given; the next pass writes no plane.
        p = ObsPlanes();
        g->simMustWaitUser = true;
        return 0;
    }
    if (!rec.known(format)) return fail(who + ": " + rec.unknown);
    if (g->stillOn)   // (a still frame's rows are carried from the entry that holds them; nothing carries its plane)
        return fail(who + ": still frames are switched on (mv_set_still_frames), " + still_clause(rec.stream) + ": switch them off first");
    if ((uintptr_t)device_buf % rec.alignment(format)) return fail(who + ": " + rec.misaligned);
    p.buf = device_buf;
    p.format = format;
    p.entries = std::max(1, g->ringCount);
    p.entryBytes = (size_t)g->N * g->A * rec.planeBytes(g->w, g->h, format);
    g->simMustWaitUser = true;   // an ordering point, as mv_set_state_obs: the next step launch comes behind what the caller's stream holds now
    return 0;
}

int planes_count(const mv_gym *g, const Planes &rec)
{
    if (getter_check(g, rec.getter)) return -1;
    const ObsPlanes &p = g->*rec.planes;
    return p.buf ? p.entries : 0;
}

int planes_format(const mv_gym *g, const Planes &rec)
{
    if (getter_check(g, rec.formatGetter)) return -1;
    const ObsPlanes &p = g->*rec.planes;
    return p.buf ? p.format : -1;
}

int planes_read(mv_gym *g, const Planes &rec, int env, int agent, void *out)   // the last tick's plane of one agent, in the record's native format
{
    const std::string who = rec.reader;
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    const ObsPlanes &p = g->*rec.planes;
    if (!p.buf) return fail(who + ": no " + rec.stream.noun + " attached (" + rec.opt().setter + ")");
    if (!out) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t px = (size_t)g->w * g->h, bytes = rec.planeBytes(g->w, g->h, p.format);
    const uint8_t *src = (const uint8_t *)(last_outputs(g).*rec.out) + ((size_t)env * g->A + agent) * bytes;
    std::vector<uint8_t> narrow(p.format == rec.native ? 0 : bytes);
    HIP_TRY(hipMemcpyAsync(p.format == rec.native ? out : narrow.data(), src, bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (p.format != rec.native) rec.widen(narrow.data(), px, p.format, out);
    return 0;
}

}  // namespace

namespace mvapi {

PlaneOuts plane_outs(const mv_gym *g, const OutPtrs &o)
{
    PlaneOuts po;
    if (g->depth.buf) { po.depth = o.depth; po.depth_format = g->depth.format; }
    if (g->seg.buf) { po.seg = o.seg; po.seg_format = g->seg.format; }
    if (g->normal.buf) { po.normal = o.normal; po.normal_format = g->normal.format; }
    return po;
}

// The planes of the frames a fast pass of v has just drawn -> o's entries, the ones the frames went to: ONE launch on the caller's stream, reading v's frame
// lists (the call's slots: the mark that frees them is recorded behind this).
int planes_follow(mv_gym *g, const GymView &v, const OutPtrs &o, const char *who)
{
    const PlaneOuts po = plane_outs(g, o);
    if (!po.any()) return 0;
    if (launch_raster_planes(v, po, g->w, g->h, g->stream)) return fail(std::string(who) + ": observation size above 1024x1024");
    HIP_TRY(hipGetLastError());
    return 1;
}

void obs_planes_free(mv_gym *g)   // (the buffers are the caller's -- forgotten, not freed)
{
    for (const Planes *rec : ALL_PLANES) g->*rec->planes = ObsPlanes();
}

}  // namespace mvapi

extern "C" {

int mv_set_depth_obs(mv_gym *g, void *device_buf, int32_t format) { return planes_attach(g, DEPTH, device_buf, format); }
int mv_set_seg_obs(mv_gym *g, void *device_buf, int32_t format) { return planes_attach(g, SEG, device_buf, format); }
int mv_get_depth_obs(const mv_gym *g) { return planes_count(g, DEPTH); }
int mv_get_seg_obs(const mv_gym *g) { return planes_count(g, SEG); }
int mv_get_depth_format(const mv_gym *g) { return planes_format(g, DEPTH); }
int mv_get_seg_format(const mv_gym *g) { return planes_format(g, SEG); }
int mv_get_depth_observation(mv_gym *g, int32_t env, int32_t agent, float *out) { return planes_read(g, DEPTH, env, agent, out); }
int mv_get_seg_observation(mv_gym *g, int32_t env, int32_t agent, uint16_t *out) { return planes_read(g, SEG, env, agent, out); }
int mv_set_normal_obs(mv_gym *g, void *device_buf, int32_t format) { return planes_attach(g, NORMAL, device_buf, format); }
int mv_get_normal_obs(const mv_gym *g) { return planes_count(g, NORMAL); }
int mv_get_normal_format(const mv_gym *g) { return planes_format(g, NORMAL); }
int mv_get_normal_observation(mv_gym *g, int32_t env, int32_t agent, float *out) { return planes_read(g, NORMAL, env, agent, out); }

const char *mv_seg_class_name(int32_t cls) { return seg_class_name(cls); }

int mv_debug_depth_pack_host(const float *t, const uint8_t *hit, int32_t n, int32_t format, void *out)
{
    if (!t || !hit || !out || n < 0) return fail("mv_debug_depth_pack_host: null pointer or n < 0");
    if (!DEPTH.known(format)) return fail(std::string("mv_debug_depth_pack_host: ") + DEPTH.unknown);
    depth_pack_host(t, hit, n, format, out);
    return 0;
}

int mv_debug_normal_pack_host(const float *xyz, const uint8_t *hit, int32_t n, int32_t format, void *out)
{
    if (!xyz || !hit || !out || n < 0) return fail("mv_debug_normal_pack_host: null pointer or n < 0");
    if (!NORMAL.known(format)) return fail(std::string("mv_debug_normal_pack_host: ") + NORMAL.unknown);
    normal_pack_host(xyz, hit, n, format, out);
    return 0;
}

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
    if (!SEG.known(format)) return fail(std::string("mv_debug_seg_rule_host: ") + SEG.unknown);
    const SegBounds b = {boundaries5[0], boundaries5[1], boundaries5[2], boundaries5[3], boundaries5[4]};
    const uint16_t w = seg_rule(scenario, slot, b, subtype);
    if (format == SEG_INSTANCE_U16) *reinterpret_cast<uint16_t *>(out) = w;
    else *reinterpret_cast<uint8_t *>(out) = seg_bits_u8(w);
    return 0;
}

int mv_debug_seg_pack_host(const int32_t *cls, const int32_t *instance, int32_t n, int32_t format, void *out)
{
    if (!cls || !instance || !out || n < 0) return fail("mv_debug_seg_pack_host: null pointer or n < 0");
    if (!SEG.known(format)) return fail(std::string("mv_debug_seg_pack_host: ") + SEG.unknown);
    for (int i = 0; i < n; ++i)
        if (cls[i] < 0 || cls[i] >= SEG_NUM_CLASSES || instance[i] < 0 || instance[i] >= SEG_MAX_INSTANCES)
            return fail("mv_debug_seg_pack_host: class outside [0, 15) or instance outside [0, 4096)");
    seg_pack_host(cls, instance, n, format, out);
    return 0;
}

}  // extern "C"
