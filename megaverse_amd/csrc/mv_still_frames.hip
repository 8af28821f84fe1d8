// megaverse_amd/csrc/mv_still_frames.hip -- still frames: the host side of mv_set_still_frames / mv_get_still_frames (include/megaverse_hip.h), the memset
// behind every call that may change what an env's frames show, and the carry launch that gives a still env's rows in an output ring the bytes of its last
// drawn frame.  The rule and the carry's plan are mv_still_frames.h; the MASKED step kernels apply the rule tick by tick (mv_step_kernels.h: env_stale) and
// mv_api_step.hip's step_gyms enqueues the carry behind a call's passes; DESIGN.md 3.18.  The host twins are in mv_api_debug.hip.
#include "mv_api_internal.h"
#include "mv_still_frames.h"

namespace mv {
namespace still {

// One workgroup per frame.  Thread 0 walks the call's rendered ticks (still_carry_plan: the frame's verdicts are the counts the step launch left in the
// slots' vis_count) and moves the frame's home; then the workgroup copies.  A run of still ticks has ONE source entry: every 16-byte piece of the row is
// loaded once and stored to each still entry of the call -- plain dwordx4 accesses, consecutive lanes consecutive pieces; the stores are plain, not
// non-temporal: the rows are about to be read by whoever consumes the observations, and either kind leaves the line in L2.  A row that is not a whole number
// of aligned 16-byte pieces (odd sizes of the planar layout) goes byte by byte.
struct CarryArgs {
    int32_t k, frames, entries, pad;
    uint32_t frame_bytes, aligned16;
    uint64_t entry_bytes;                       // frames * frame_bytes
    uint8_t *ring;                              // [entries][frames][frame_bytes]
    int32_t *home;                              // [frames]
    const int32_t *verdict[PIPE_BATCH_MAX];     // tick j's vis_count [frames]
    int32_t entry[PIPE_BATCH_MAX];
};
__global__ __launch_bounds__(256) void still_carry_kernel(CarryArgs a)
{
    __shared__ int32_t s_src[PIPE_BATCH_MAX], s_dst[PIPE_BATCH_MAX];
    __shared__ int32_t s_any;
    const int f = blockIdx.x;
    if (f >= a.frames) return;
    if (threadIdx.x == 0) {
        int32_t v[PIPE_BATCH_MAX], e[PIPE_BATCH_MAX];
        for (int j = 0; j < a.k; ++j) { v[j] = a.verdict[j][f]; e[j] = s_dst[j] = a.entry[j]; }
        const int32_t home = a.home[f];
        // (a home from before the ring was attached cannot be met -- attaching makes every env stale, and a drawn tick moves the home -- but no entry
        // outside the ring is ever read)
        const int32_t nh = still_carry_plan(v, 1, e, a.k, home >= 0 && home < a.entries ? home : -1, s_src);
        if (nh != home) a.home[f] = nh;
        int any = 0;
        for (int j = 0; j < a.k; ++j) any |= s_src[j] >= 0;
        s_any = any;
    }
    __syncthreads();
    if (!s_any) return;
    uint8_t *const row = a.ring + (size_t)f * a.frame_bytes;
    if (a.aligned16) {
        const uint32_t n16 = a.frame_bytes >> 4;
        for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) {
            int32_t last = -1;
            uint4 val = make_uint4(0u, 0u, 0u, 0u);
            for (int j = 0; j < a.k; ++j) {
                const int32_t s = s_src[j];
                if (s < 0) continue;
                if (s != last) { val = reinterpret_cast<const uint4 *>(row + (size_t)s * a.entry_bytes)[i]; last = s; }
                reinterpret_cast<uint4 *>(row + (size_t)s_dst[j] * a.entry_bytes)[i] = val;
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < a.frame_bytes; i += blockDim.x) {
            int32_t last = -1;
            uint8_t val = 0;
            for (int j = 0; j < a.k; ++j) {
                const int32_t s = s_src[j];
                if (s < 0) continue;
                if (s != last) { val = row[(size_t)s * a.entry_bytes + i]; last = s; }
                row[(size_t)s_dst[j] * a.entry_bytes + i] = val;
            }
        }
    }
}

}  // namespace still
}  // namespace mv

namespace {

int still_alloc(mv_gym *g)
{
    if (g->stillHome) return 0;
    const size_t bytes = mv::still::still_frames_bytes(g->N, g->A);
    hipError_t e_ = hipMalloc((void **)&g->stillHome, bytes);
    if (e_ != hipSuccess) { g->stillHome = nullptr; return fail("mv_set_still_frames: hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
    g->stillStale = reinterpret_cast<uint8_t *>(g->stillHome + (size_t)g->N * g->A);
    g->stillBytes = bytes;
    return 0;
}

}  // namespace

void mvapi::still_frames_free(mv_gym *g)
{
    if (g->stillHome) (void)hipFree(g->stillHome);
    g->stillHome = nullptr; g->stillStale = nullptr;
    g->stillBytes = 0;
    g->stillOn = false;
}

// Every env stale: one memset on the caller's stream, behind every step launch enqueued so far (sim_join: the step kernels write the bytes) and in front of
// the next one (simMustWaitUser).  Off: nothing, not even the join.
int mvapi::still_frames_touch(mv_gym *g)
{
    if (!g->stillOn) return 0;
    HIP_TRY(hipSetDevice(g->device));
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemsetAsync(g->stillStale, 1, (size_t)g->N, g->stream));
    return 0;
}

// The carry of one stepping call: the n rendered ticks' views (views[j * stride]: their slots' vis_count) and the ring entries their rows went to
// (obs[j * stride]); one launch on the caller's stream, behind the call's passes.
int mvapi::still_frames_carry(mv_gym *g, const GymView *views, const OutPtrs *outs, int stride, int n)
{
    mv::still::CarryArgs a;
    const size_t fb = g->frameBytes(), frames = (size_t)g->N * g->A;
    a.k = n; a.frames = (int32_t)frames; a.entries = g->ringCount; a.pad = 0;
    a.frame_bytes = (uint32_t)fb;
    a.aligned16 = ((uintptr_t)g->ringObs % 16 == 0 && fb % 16 == 0) ? 1u : 0u;
    a.entry_bytes = (uint64_t)(frames * fb);
    a.ring = g->ringObs;
    a.home = g->stillHome;
    for (int j = 0; j < (int)PIPE_BATCH_MAX; ++j) {
        const int jj = std::min(j, n - 1);
        a.verdict[j] = views[(size_t)jj * stride].vis_count;
        a.entry[j] = (int32_t)((size_t)((const uint8_t *)outs[(size_t)jj * stride].obs - g->ringObs) / (frames * fb));
    }
    hipLaunchKernelGGL(mv::still::still_carry_kernel, dim3((unsigned)frames), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int mv_set_still_frames(mv_gym *g, int32_t on)
{
    if (attach_check(g, "mv_set_still_frames", gym_options[OPT_STILL_FRAMES])) return -1;
    if (!on) {
        // The step launches enqueued so far keep the views they were given; the next one is drawn whole again.  The arrays stay until mv_close.
        g->stillOn = false;
        g->simMustWaitUser = true;
        return 0;
    }
    // (a still frame's rows are carried from the entry that holds them; nothing carries its depth or label plane)
    if (planes_attached(g, "mv_set_still_frames", still_clause)) return -1;
    HIP_TRY(hipSetDevice(g->device));
    if (still_alloc(g)) return -1;
    // Every env stale, no frame has a home: on the caller's stream, behind every step launch enqueued so far; the next step launch waits for it.  This call is
    // the ordering point, as mv_set_draw_mask is, and never waits on the host.  (Also when the option was on already: the same promise, made again.)
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemsetAsync(g->stillHome, 0xFF, (size_t)g->N * g->A * sizeof(int32_t), g->stream));
    HIP_TRY(hipMemsetAsync(g->stillStale, 1, (size_t)g->N, g->stream));
    g->stillOn = true;
    return 0;
}

int mv_get_still_frames(const mv_gym *g) { return getter_check(g, "mv_get_still_frames") ? -1 : g->stillOn ? 1 : 0; }

}  // extern "C"
