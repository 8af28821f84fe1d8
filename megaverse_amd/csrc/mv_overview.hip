// megaverse_amd/csrc/mv_overview.hip -- overview cameras: the host side of mv_set_overview / mv_set_overview_cameras / mv_set_overview_cameras_host /
// mv_draw_overview / mv_get_overview_observation / mv_overview_device_ptr / mv_overview_dropped / mv_overview_capacity (include/megaverse_hip.h), and the
// host-only mv_overview_default_camera and mv_debug_overview_camera_host.
// The rule and the arrays: mv_overview.h.  The kernels: mv_raster.hip (overview_setup_kernel: mv_frame.h's frame_setup_body in its OVERVIEW instantiation;
// overview_raster_kernel: raster_body in its).  DESIGN.md 3.23 says what shares what and where the draw stands in the streams' order.
#include "mv_api_internal.h"
#include "mv_overview.h"

namespace {

const GymOption &opt() { return gym_options[OPT_OVERVIEW]; }

mv_camera *cams_of(const mv_gym *g) { return reinterpret_cast<mv_camera *>(g->overview.arrays + g->overview.layout.cams); }

// n host records -> the gym's camera array, through the pool, on the gym's stream behind every step launch enqueued so far
int stage_cameras(mv_gym *g, const mv_camera *cams, const char *who)
{
    const size_t bytes = (size_t)g->N * sizeof(mv_camera);
    StagingPool::Buffer *s = nullptr;
    if (g->overview.pool.take(bytes, who, s)) return -1;
    std::memcpy(s->host, cams, bytes);
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(cams_of(g), s->host, bytes, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(s->copied, g->stream));
    return 0;
}

int default_cameras(mv_gym *g, const char *who)
{
    const std::vector<mv_camera> cams((size_t)g->N, overview_default_camera());
    return stage_cameras(g, cams.data(), who);
}

// the overview's arrays, at the first attach: lists of the scenario's capacity, the dropped word zero, every camera at the default pose
int allocate_arrays(mv_gym *g, const char *who)
{
    if (g->overview.arrays) return 0;
    const int cap = overview_capacity(g->gv);
    const OverviewLayout l = overview_layout(g->N, cap);
    uint8_t *mem = nullptr;
    {
        hipError_t e_ = hipMalloc((void **)&mem, l.bytes);
        if (e_ != hipSuccess) return fail(std::string(who) + ": hipMalloc of " + std::to_string(l.bytes) + " bytes: " + hipGetErrorString(e_));
    }
    g->overview.arrays = mem;
    g->overview.layout = l;
    g->overview.cap = cap;
    HIP_TRY(hipMemsetAsync(mem, 0, l.bytes, g->stream));
    if (const char *e = getenv("MV_OVERVIEW_ORDER")) g->overview.costOrder = atoi(e) != 0;
    if (!g->overview.costOrder) {   // the identity, once: what the pass reads where no frame-order launch writes
        std::vector<int32_t> ident((size_t)g->N);
        for (int e = 0; e < g->N; ++e) ident[(size_t)e] = e;
        HIP_TRY(hipMemcpyAsync(mem + l.order, ident.data(), ident.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));   // (the vector goes out of scope)
    }
    return default_cameras(g, who);
}

int release_owned(mv_gym *g)
{
    if (g->overview.owned) {
        HIP_TRY(hipStreamSynchronize(g->stream));   // (a draw into it may be in flight)
        HIP_TRY(hipFree(g->overview.owned));
    }
    g->overview.owned = nullptr;
    g->overview.ownedBytes = 0;
    return 0;
}

}  // namespace

void mvapi::overview_free(mv_gym *g)
{
    g->overview.pool.release();
    if (g->overview.owned) (void)hipFree(g->overview.owned);
    if (g->overview.arrays) (void)hipFree(g->overview.arrays);
    g->overview = OverviewState{};
}

extern "C" {

int mv_set_overview(mv_gym *g, int32_t w, int32_t h, void *device_rgba)
{
    const char *who = "mv_set_overview";
    if (attach_check(g, who, opt())) return -1;
    HIP_TRY(hipSetDevice(g->device));
    if (w == 0 && h == 0) {   // detach: the arrays and the cameras stay (mv_close frees them), the gym's own frames go
        if (release_owned(g)) return -1;
        g->overview.buf = nullptr;
        g->overview.w = g->overview.h = 0;
        return 0;
    }
    if (w < 1 || h < 1 || w > 1024 || h > 1024) return fail(std::string(who) + ": size " + std::to_string(w) + " x " + std::to_string(h) + " is outside 1 .. 1024 (w = h = 0: detach)");
    if (device_rgba && (uintptr_t)device_rgba % 4) return fail(std::string(who) + ": the buffer must be 4-byte aligned");
    if (allocate_arrays(g, who)) return -1;
    const size_t bytes = (size_t)g->N * w * h * 4;
    if (device_rgba) {
        if (release_owned(g)) return -1;
        g->overview.buf = reinterpret_cast<uint32_t *>(device_rgba);
    } else {
        if (!g->overview.owned || g->overview.ownedBytes != bytes) {
            if (release_owned(g)) return -1;
            hipError_t e_ = hipMalloc((void **)&g->overview.owned, bytes);
            if (e_ != hipSuccess) { g->overview.owned = nullptr; g->overview.buf = nullptr; return fail(std::string(who) + ": hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
            g->overview.ownedBytes = bytes;
        }
        g->overview.buf = g->overview.owned;
    }
    g->overview.w = w; g->overview.h = h;
    return 0;
}

int mv_set_overview_cameras(mv_gym *g, const mv_camera *device_cams)
{
    const char *who = "mv_set_overview_cameras";
    if (attach_check(g, who, opt())) return -1;
    HIP_TRY(hipSetDevice(g->device));
    if (!g->overview.arrays) return fail(std::string(who) + ": no overview attached yet (mv_set_overview)");
    if (!device_cams) return default_cameras(g, who);
    // behind every step launch enqueued so far and behind what the caller's stream holds now -- the kernel that wrote the records; out-of-range agent indices
    // are clamped and counted by the setup that reads them
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(cams_of(g), device_cams, (size_t)g->N * sizeof(mv_camera), hipMemcpyDeviceToDevice, g->stream));
    return 0;
}

int mv_set_overview_cameras_host(mv_gym *g, const mv_camera *cams)
{
    const char *who = "mv_set_overview_cameras_host";
    if (attach_check(g, who, opt())) return -1;
    HIP_TRY(hipSetDevice(g->device));
    if (!g->overview.arrays) return fail(std::string(who) + ": no overview attached yet (mv_set_overview)");
    if (!cams) return default_cameras(g, who);
    for (int e = 0; e < g->N; ++e) {
        const mv_camera &c = cams[e];
        if (c.agent < -1 || c.agent >= g->A)
            return fail(std::string(who) + ": record " + std::to_string(e) + ": agent " + std::to_string(c.agent) + " is outside -1 .. " + std::to_string(g->A - 1));
        if (c.pad[0] != 0 || c.pad[1] != 0) return fail(std::string(who) + ": record " + std::to_string(e) + ": the pad words must be 0");
    }
    return stage_cameras(g, cams, who);
}

int mv_draw_overview(mv_gym *g)
{
    if (check(g)) return -1;
    if (!g->overview.buf) return 0;   // no overview attached: drawOverview of a build without a window (megaverse.cpp:180-201)
    HIP_TRY(hipSetDevice(g->device));
    if (sim_join(g)) return -1;   // behind every step launch enqueued so far; the next one waits for this draw: it reads the state as it stands
    const OverviewState &o = g->overview;
    GymView v = view(g, g->parity);
    v.vis_prims = o.arrays + o.layout.prims;
    v.vis_rects = o.arrays + o.layout.rects;
    v.vis_hdr = o.arrays + o.layout.hdr;
    v.vis_count = reinterpret_cast<int32_t *>(o.arrays + o.layout.count);
    v.lpt_bucket = reinterpret_cast<int32_t *>(o.arrays + o.layout.bucket);
    v.lpt_order = reinterpret_cast<int32_t *>(o.arrays + o.layout.order);
    v.vis_stride = o.cap;
    // nothing of the stepping calls' passes: no cost histogram or list, no sort scratch, no frame-order table, no mask, no stale bytes, no observation rows
    v.lpt_hist = nullptr; v.lpt_list = nullptr; v.lpt_forder = nullptr; v.lpt_forder_on = 0; v.lpt_no_clear = 1;
    v.sort_scratch = nullptr; v.depth_sort = 0;
    v.draw_mask = nullptr; v.step_mask = nullptr; v.still = nullptr;
    v.state_obs = nullptr; v.scene_obs = nullptr; v.entity_obs = nullptr;
    v.obs_layout = MV_OBS_RGBA;
    OverviewArgs a;
    a.cams = cams_of(g);
    a.out = reinterpret_cast<OverviewCam *>(o.arrays + o.layout.out);
    a.dropped = reinterpret_cast<unsigned long long *>(o.arrays + o.layout.dropped);
    if (launch_overview(v, a, o.buf, o.w, o.h, g->stream, o.costOrder)) return fail("mv_draw_overview: overview size above 1024x1024");
    HIP_TRY(hipGetLastError());
    return 0;
}

int mv_get_overview_observation(mv_gym *g, int32_t env, uint8_t *out)
{
    const std::string who = "mv_get_overview_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->overview.buf) return fail(who + ": no overview attached (mv_set_overview)");
    if (!out) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t frameBytes = (size_t)g->overview.w * g->overview.h * 4;
    HIP_TRY(hipMemcpyAsync(out, (const uint8_t *)g->overview.buf + (size_t)env * frameBytes, frameBytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

void *mv_overview_device_ptr(mv_gym *g) { return (g && !g->closed) ? g->overview.buf : nullptr; }

int mv_overview_dropped(mv_gym *g, int64_t *out)
{
    const std::string who = "mv_overview_dropped";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!out) return fail(who + ": null pointer");
    *out = 0;
    if (!g->overview.arrays) return 0;
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipMemcpyAsync(out, g->overview.arrays + g->overview.layout.dropped, sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_overview_capacity(const mv_gym *g)
{
    if (getter_check(g, "mv_overview_capacity")) return -1;
    return overview_capacity(g->gv);
}

int mv_overview_default_camera(mv_camera *out)
{
    if (!out) return fail("mv_overview_default_camera: null pointer");
    *out = overview_default_camera();
    return 0;
}

int mv_debug_overview_camera_host(const mv_camera *cam, const void *agent_state, float *out)
{
    const char *who = "mv_debug_overview_camera_host";
    if (!cam || !out) return fail(std::string(who) + ": null pointer");
    const OverviewPlan plan = overview_plan(*cam, MAX_AGENTS);
    if (plan.clamped) return fail(std::string(who) + ": agent " + std::to_string(cam->agent) + " is outside -1 .. " + std::to_string(MAX_AGENTS - 1));
    float eye[3], c[9];
    if (plan.agent >= 0) {
        if (!agent_state) return fail(std::string(who) + ": an AGENT camera needs its agent's state record");
        AgentState a;
        std::memcpy(&a, agent_state, sizeof(a));
        // (mv_frame.h: frame_setup_body, "cameras" -- the same expressions in the same order)
        eye[0] = a.pos[0]; eye[1] = (a.pos[1] + 0.05f) + 0.41f; eye[2] = a.pos[2];
        float sp, cp;
        sincos_poly(a.pitch, sp, cp);
        c[0] = a.m00; c[1] = a.m02 * sp; c[2] = a.m02 * cp;
        c[3] = 0.0f;  c[4] = cp;         c[5] = -sp;
        c[6] = a.m20; c[7] = a.m22 * sp; c[8] = a.m22 * cp;
        if (plan.viewer == MAX_CAMS) {   // (mat_mul's order)
            const float x = cam->eye[0], y = cam->eye[1], z = cam->eye[2];
            eye[0] += (c[0] * x + c[1] * y) + c[2] * z;
            eye[1] += (c[3] * x + c[4] * y) + c[5] * z;
            eye[2] += (c[6] * x + c[7] * y) + c[8] * z;
        }
    } else {
        for (int i = 0; i < 3; ++i) eye[i] = cam->eye[i];
        for (int i = 0; i < 9; ++i) c[i] = cam->c[i];
    }
    for (int i = 0; i < 3; ++i) out[i] = eye[i];
    for (int i = 0; i < 9; ++i) out[3 + i] = c[i];
    return 0;
}

}  // extern "C"
