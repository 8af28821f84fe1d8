// megaverse_amd/csrc/mv_overview.h -- overview cameras: the rule, stated once (include/megaverse_hip.h: mv_set_overview).
//
// One camera per env (mv_camera), FREE in the world or attached to an AGENT.  Projection (100 degrees at 128/72, pixel centres), clip range [0.01, 120] and
// light (0, 4, 2) in the camera's own space are the agents' (mv_frame.h); the reference's overview range (0.1, 600) is deliberately not adopted -- the range
// is part of the shared hit tests.
//   AGENT k   the agent's eye and basis as frame_setup_body computes them (the overview's setup IS frame_setup_body, its OVERVIEW instantiation: the same
//             lines).  An all-zero offset performs no arithmetic: the viewer is frame of reference k itself, and every path of the pass that treats "the
//             viewer's own frame" specially is taken as in the agent's observation.  A non-zero offset adds C_agent . offset to the eye (mat_mul's order:
//             (c0 x + c1 y) + c2 z per row); the basis is the agent's.  MV_CAMERA_FIRST_PERSON: the agent's capsule and eyes box are not drawn.
//   FREE      eye and basis from the record, taken as given.
// A camera that is not an agent's very eye is one more frame of reference, index MAX_CAMS (no primitive lives in it); it travels beside the frame header,
// which has no spare floats, as an OverviewCam record.
// Slots, drawables, colours and the depth-tie rule are frame_setup_body's and raster_body's own: nothing of them is restated here.
#pragma once
#include <stdint.h>

#include "../../include/megaverse_hip.h"
#include "mv_types.h"

namespace mv {

// The reference's pose (rendering/src/render_utils.cpp:34-55): root = Ry(225 deg) . T(0.1, 20, 0.1), tilt = Rx(-40 deg); Magnum's *Local transformations
// multiply from the right, so eye = Ry(225) (0.1, 20, 0.1) and C = Ry(225) Rx(-40).  With c = s = -cos 45 for Ry and (cos 40, -sin 40) for Rx:
//   eye   = (c 0.1 + s 0.1, 20, -s 0.1 + c 0.1)             = (-0.14142136, 20, 0)
//   right = Ry (1, 0, 0)            = (c, 0, -s)             = (-0.70710678, 0, 0.70710678)
//   up    = Ry (0, cos 40, -sin 40) = (-s sin 40, cos 40, -c sin 40) = (0.45451948, 0.76604444, 0.45451948)
//   back  = Ry (0, sin 40, cos 40)  = (s cos 40, sin 40, c cos 40)  = (-0.54167522, 0.64278761, -0.54167522)      (view direction = -back)
constexpr float OVERVIEW_DEFAULT_EYE[3] = {-0.14142136f, 20.0f, 0.0f};
constexpr float OVERVIEW_DEFAULT_C[9] = {-0.70710678f, 0.45451948f, -0.54167522f,
                                         0.0f,         0.76604444f, 0.64278761f,
                                         0.70710678f,  0.45451948f, -0.54167522f};

__host__ __device__ inline mv_camera overview_default_camera()
{
    mv_camera cam{};
    for (int i = 0; i < 3; ++i) cam.eye[i] = OVERVIEW_DEFAULT_EYE[i];
    for (int i = 0; i < 9; ++i) cam.c[i] = OVERVIEW_DEFAULT_C[i];
    cam.agent = -1;
    return cam;
}

// What a record means for a gym of A agents per env.  agent: -1 FREE, else the agent; viewer: the frame of reference the env is seen from -- the agent's
// own (zero offset) or MAX_CAMS, the overview's; hide: the agent whose capsule and eyes box are not drawn, -1: none; clamped: the record's agent index was
// out of range and is taken as FREE (the device form counts these, the host form refuses them).
struct OverviewPlan { int agent, viewer, hide, clamped; };
__host__ __device__ inline OverviewPlan overview_plan(const mv_camera &cam, int A)
{
    OverviewPlan p;
    p.clamped = cam.agent < -1 || cam.agent >= A ? 1 : 0;
    p.agent = p.clamped ? -1 : cam.agent;
    const bool zeroOffset = cam.eye[0] == 0.0f && cam.eye[1] == 0.0f && cam.eye[2] == 0.0f;
    p.viewer = p.agent >= 0 && zeroOffset ? p.agent : (int)MAX_CAMS;
    p.hide = p.agent >= 0 && (cam.flags & MV_CAMERA_FIRST_PERSON) ? p.agent : -1;
    return p;
}

// The camera an env was set up with, beside its frame header: what overview_raster_kernel reads as frame of reference MAX_CAMS, and which one it looks from
struct alignas(16) OverviewCam {
    float eye[3];
    int32_t viewer;
    float c[9];
    int32_t hide, pad[2];
};
static_assert(sizeof(OverviewCam) == 64 && sizeof(mv_camera) == 64, "overview records: 64 bytes");

// What the overview's frame setup takes besides its view (whose vis_* / lpt_bucket / lpt_order / vis_hdr fields point at the overview's own arrays)
struct OverviewArgs {
    const mv_camera *cams;         // [N] the gym's camera array
    OverviewCam *out;              // [N]
    unsigned long long *dropped;   // low half: primitives that did not fit a list; high half: clamped agent indices
};

// List capacity: the smallest tier that holds every slot the scenario can have -- a bird's-eye view sees nearly all of them (mv_frame.h has the slot table:
// layout | terrain | movable | rewards | 3 per agent).  Above 2048 (a full Hex maze) primitives are dropped and counted.
__host__ inline int overview_max_slots(const GymView &gv)
{
    const int s = gv.scenario;
    const bool hex = s == SCN_HEX_MEMORY || s == SCN_HEX_EXPLORE || s == SCN_BOXAGONE || s == SCN_FOOTBALL;
    const int layout = hex ? (int)HEX_MAX_BOXES : gv.box_stride;
    const int terrain = s == SCN_TOWER ? 1 : s == SCN_REARRANGE ? NUM_STATIC + MAX_ITEMS : s == SCN_SOKOBAN ? SOKO_DIM * SOKO_DIM : hex ? 0 : (int)MAX_TERRAIN;
    const int rewards = s == SCN_TOWER ? 0 : hex ? 3 * HEX_MAX_OBJS : 2 * gv.reward_stride;
    return layout + terrain + (int)MAX_OBJECTS + rewards + 3 * gv.num_agents;
}
__host__ inline int overview_capacity(const GymView &gv)
{
    const int n = overview_max_slots(gv);
    return n <= 256 ? 256 : n <= 1024 ? 1024 : 2048;
}

// The overview's arrays, one allocation: every array rounded up to 256 bytes, in this order
//   prims [N][cap] 32 B | rects [N][cap] 8 B | headers [N] FRAME_HDR_BYTES | counts [N] 4 B | cost bins [N] 4 B | frame order [N] 4 B
//   | cameras [N] 64 B (mv_camera) | cameras as set up [N] 64 B (OverviewCam) | the dropped word, 8 B
struct OverviewLayout { size_t prims, rects, hdr, count, bucket, order, cams, out, dropped, bytes; };
__host__ inline OverviewLayout overview_layout(int N, int cap)
{
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    OverviewLayout l{};
    size_t at = 0;
    l.prims = at; at += up((size_t)N * cap * 32);
    l.rects = at; at += up((size_t)N * cap * 8);
    l.hdr = at; at += up((size_t)N * FRAME_HDR_BYTES);
    l.count = at; at += up((size_t)N * 4);
    l.bucket = at; at += up((size_t)N * 4);
    l.order = at; at += up((size_t)N * 4);
    l.cams = at; at += up((size_t)N * sizeof(mv_camera));
    l.out = at; at += up((size_t)N * sizeof(OverviewCam));
    l.dropped = at; at += up(8);
    l.bytes = at;
    return l;
}

}  // namespace mv
