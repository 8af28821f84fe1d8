// megaverse_amd/csrc/mv_stack_obs.hip -- stack observations (mv_stack_obs.h has the record and its rule): the stacking kernel, its launch behind the pass that
// drew a tick's frames, and the host side of mv_set_stack_obs / mv_get_stack_obs / mv_stack_obs_shape / mv_get_stack_observation / mv_debug_stack_host /
// mv_debug_stack_device (include/megaverse_hip.h).  DESIGN.md 3.29.
//
// The kernel: one workgroup of 256 lanes per frame, reading the colour frame the pass wrote -- behind that launch, on the same stream -- and the agent's stack
// in the entry the previous drawn tick wrote (prev), writing the agent's stack in this tick's entry (out; with one entry prev == out).  No LDS, no atomics.
//   prologue  the byte(s) that say whether the frame is the first of a new episode (the tick's staged done[env]; a reset's mask) at workgroup-uniform addresses:
//             scalar loads; the two bases are kernel arguments.  An undrawn frame leaves here, before any load or store.
//   shift     (not on a clear, not on a frame drawn again) plane-sets 1 .. S - 1 of prev -> 0 .. S - 2 of out.  A lane owns positions of a plane-set --
//             16-byte groups where w % 16 == 0 (then every plane, plane-set and stack starts on a 16-byte boundary), else dwords -- and for each walks i
//             ascending: load position p of prev[i + 1], store position p of out[i].  In place that lane alone ever touches position p of any plane-set, so
//             it reads every value before it overwrites it.
//   barrier   the image's lanes own other positions of plane-set S - 1 than the shift's: they store only after every lane has read the old newest plane-set.
//   image     a lane owns 4 consecutive output pixels of one output row.  RGBA: `factor` rows of `factor` 16-byte quads; CHW: `factor` rows of `factor`
//             dwords per plane.  Horizontal and vertical sums in registers, the rule (stack_gray / stack_mean), four bytes packed with shifts, one dword
//             store per plane: to plane-set S - 1, or on a clear to all S.  Consecutive lanes take consecutive dwords of a row and then the next row: the
//             loads of a wave cover whole frame rows and its stores are contiguous.  Plain stores: the next tick reads them back.
// Two ticks of one agent never run concurrently -- the launches of one gym follow each other on its stream -- and the workgroups of one launch own disjoint
// stacks.
#include "mv_api_internal.h"
#include "mv_frame.h"
#include "mv_stack_obs.h"

namespace mv {

constexpr int STACK_THREADS = 256;

// When a frame is the first of a new episode -- mvapi::WorldMapClear's three cases, as world_map_obs_kernel reads them: all -- every frame (mv_reset; the debug
// hook's clear); done[env] -- the tick's staged done flags; mask[env] (and, applied given, applied[env]) -- the envs a masked reset flagged and that took
// their next episode.  Null pointers say nothing.  again: the frame is drawn again (mv_render): only the newest plane-set is written
struct StackClearArgs {
    int32_t all, again;
    const uint8_t *done, *mask, *applied;
};

// one byte at a workgroup-uniform address, read as the aligned word that holds it: a scalar load (the word lies in the byte's own 4-byte cell, so in its page)
__device__ __forceinline__ uint32_t stack_uniform_byte(const uint8_t *p)
{
    const uint32_t off = (uint32_t)((uintptr_t)p & 3u);
    return (*reinterpret_cast<const uint32_t *>(p - off) >> (8u * off)) & 0xffu;
}

// 16 bytes / F dwords that are only known to be dword-aligned (a caller's RGBA frames; a planar slab of a width that is no multiple of 16): one wide load
struct __attribute__((aligned(4))) StackQuad { uint32_t v[4]; };
template <int F> struct __attribute__((aligned(4))) StackWords { uint32_t v[F]; };

// frames: the grid.  vis_count: the tick's list lengths, null: every frame counts as drawn (mv_debug_stack_device).  frame_buf: [frames] colour frames of
// W x H pixels in LAYOUT; prev, out: [frames][S][C][h][w] bytes, 16-byte aligned; W, H multiples of 1 << LG, w = W >> LG a multiple of 4
template <int LAYOUT, int FORMAT, int LG>
__global__ __launch_bounds__(STACK_THREADS) void stack_obs_kernel(const int32_t *__restrict__ vis_count, int A, StackClearArgs clr, const uint8_t *__restrict__ frame_buf,
                                                                   const uint8_t *prev, uint8_t *out, int W, int H, int S)
{
    constexpr int F = 1 << LG, C = FORMAT == STACK_RGB_U8 ? 3 : 1;
    const int frame = blockIdx.x, tid = threadIdx.x, env = frame / A;

    // ---- prologue
    bool clear = clr.all != 0;
    if (clr.done) clear = clear || stack_uniform_byte(clr.done + env) != 0u;
    if (clr.mask) clear = clear || (stack_uniform_byte(clr.mask + env) != 0u && (!clr.applied || stack_uniform_byte(clr.applied + env) != 0u));
    if (vis_count && vis_count[frame] < 0) return;   // (uniform) an undrawn frame: nothing is read or written

    const int w = W >> LG, h = H >> LG;
    const size_t plane = (size_t)w * h, P = plane * C;   // one plane; one plane-set
    const uint8_t *pstack = prev + (size_t)frame * S * P;
    uint8_t *ostack = out + (size_t)frame * S * P;

    // ---- shift
    if (!clear && !clr.again && S > 1) {
        if ((w & 15) == 0) {
            const int groups = (int)(P >> 4);
            for (int p = tid; p < groups; p += STACK_THREADS)
                for (int i = 0; i + 1 < S; ++i)
                    reinterpret_cast<uint4 *>(ostack + (size_t)i * P)[p] = reinterpret_cast<const uint4 *>(pstack + (size_t)(i + 1) * P)[p];
        } else {
            const int words = (int)(P >> 2);
            for (int p = tid; p < words; p += STACK_THREADS)
                for (int i = 0; i + 1 < S; ++i)
                    reinterpret_cast<uint32_t *>(ostack + (size_t)i * P)[p] = reinterpret_cast<const uint32_t *>(pstack + (size_t)(i + 1) * P)[p];
        }
        __syncthreads();   // (uniform branch) the old newest plane-set has been read by every lane: the image may overwrite it
    }

    // ---- image
    const uint8_t *fr = frame_buf + (size_t)frame * W * H * (LAYOUT == STACK_CHW ? 3 : 4);
    const int wordsPerRow = w >> 2, items = wordsPerRow * h;
    const int first = clear ? 0 : S - 1;   // the plane-sets the image goes to: all of them on a clear, else the newest
    for (int it = tid; it < items; it += STACK_THREADS) {
        const int Y = it / wordsPerRow, X4 = it - Y * wordsPerRow;   // output row; output dword of the row: frame pixels 4 F X4 .. 4 F X4 + 4 F - 1
        uint32_t sum[3][4] = {};
#pragma unroll
        for (int r = 0; r < F; ++r) {
            const size_t px0 = (size_t)(Y * F + r) * W + (size_t)X4 * 4 * F;   // the row's first frame pixel of this lane
            if constexpr (LAYOUT == STACK_RGBA) {
                const StackQuad *row = reinterpret_cast<const StackQuad *>(fr + px0 * 4);
#pragma unroll
                for (int q = 0; q < F; ++q) {
                    const StackQuad v = row[q];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {   // frame pixel 4 q + j of the lane's 4 F: output pixel (4 q + j) >> LG
                        sum[0][(4 * q + j) >> LG] += v.v[j] & 0xffu;
                        sum[1][(4 * q + j) >> LG] += (v.v[j] >> 8) & 0xffu;
                        sum[2][(4 * q + j) >> LG] += (v.v[j] >> 16) & 0xffu;
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const StackWords<F> v = *reinterpret_cast<const StackWords<F> *>(fr + (size_t)c * W * H + px0);
#pragma unroll
                    for (int q = 0; q < F; ++q)
#pragma unroll
                        for (int j = 0; j < 4; ++j) sum[c][(4 * q + j) >> LG] += (v.v[q] >> (8 * j)) & 0xffu;
                }
            }
        }
        uint32_t word[C];
#pragma unroll
        for (int c = 0; c < C; ++c) word[c] = 0u;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if constexpr (FORMAT == STACK_GRAY_U8) word[0] |= stack_gray(sum[0][p], sum[1][p], sum[2][p], LG) << (8 * p);
            else {
#pragma unroll
                for (int c = 0; c < 3; ++c) word[c] |= stack_mean(sum[c][p], LG) << (8 * p);
            }
        }
        for (int i = first; i < S; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) reinterpret_cast<uint32_t *>(ostack + (size_t)i * P + (size_t)c * plane)[it] = word[c];
    }
}

// one launch of the kernel for the frames' layout, the stack's format and the factor (uniform per launch: the template axes)
static void stack_launch(hipStream_t stream, int frames, const int32_t *vis_count, int A, const StackClearArgs &clr, const void *frame_buf, int layout,
                         const void *prev, void *out, int W, int H, int S, int factor, int format)
{
    const dim3 grid((unsigned)frames), block(STACK_THREADS);
#define MV_STACK_GO(L, FM, LG) \
    hipLaunchKernelGGL((stack_obs_kernel<L, FM, LG>), grid, block, 0, stream, vis_count, A, clr, (const uint8_t *)frame_buf, (const uint8_t *)prev, (uint8_t *)out, W, H, S)
#define MV_STACK_FACTOR(L, FM) \
    do { if (factor == 1) MV_STACK_GO(L, FM, 0); else if (factor == 2) MV_STACK_GO(L, FM, 1); else MV_STACK_GO(L, FM, 2); } while (0)
    if (layout == STACK_CHW) {
        if (format == STACK_RGB_U8) MV_STACK_FACTOR(STACK_CHW, STACK_RGB_U8);
        else MV_STACK_FACTOR(STACK_CHW, STACK_GRAY_U8);
    } else {
        if (format == STACK_RGB_U8) MV_STACK_FACTOR(STACK_RGBA, STACK_RGB_U8);
        else MV_STACK_FACTOR(STACK_RGBA, STACK_GRAY_U8);
    }
#undef MV_STACK_FACTOR
#undef MV_STACK_GO
}

}  // namespace mv

namespace mvapi {

namespace {
const GymOption &opt() { return gym_options[OPT_STACK_OBS]; }
static_assert(MV_OBS_RGBA == STACK_RGBA && MV_OBS_RGB_PLANAR == STACK_CHW, "the frames' layout words");
static_assert(MV_STACK_GRAY_U8 == STACK_GRAY_U8 && MV_STACK_RGB_U8 == STACK_RGB_U8, "the stack's format words");

// what both debug hooks refuse, before either touches a byte
int stack_debug_check(const std::string &who, const void *frame, int layout, int w, int h, int frames, int factor, int format, const uint8_t *prev, const uint8_t *out)
{
    if (!frame || !prev || !out) return fail(who + ": null pointer");
    if (layout != STACK_RGBA && layout != STACK_CHW) return fail(who + ": layout must be MV_OBS_RGBA (0) or MV_OBS_RGB_PLANAR (1)");
    if (w > MAX_W || h > MAX_H) return fail(who + ": a frame is at most 1024x1024");
    if (const char *why = stack_args_refusal(w, h, frames, factor, format)) return fail(who + ": " + why);
    return 0;
}
}  // namespace

// The stacks of the frames o.obs holds -> o.stack, the same tick's entry: ONE launch on the caller's stream behind the pass that drew the frames; v: the tick's
// view (its slot says which frames were drawn).  prev: the entry the previous drawn tick wrote, which the gym remembers (stackLast); the first launch after an
// attach reads this tick's own entry -- whatever the caller's buffer holds, as a world map's grids.  clear: world_map_follow's, with its three cases read the
// same way; nothing set (mv_render): the frame is drawn AGAIN -- the newest plane-set is re-imaged and nothing shifts.  -> launches made (0: nothing attached), -1
int stack_follow(mv_gym *g, const GymView &v, const OutPtrs &o, const WorldMapClear &clear)
{
    if (!o.stack || !o.obs) return 0;
    const bool again = !clear.all && !clear.done && !clear.mask;
    const StackClearArgs clr{clear.all ? 1 : 0, again ? 1 : 0, clear.done, clear.mask, clear.applied};
    stack_launch(g->stream, g->N * g->A, (const int32_t *)v.vis_count, g->A, clr, o.obs, g->obsLayout, g->stackLast ? g->stackLast : o.stack, o.stack, g->w, g->h,
                 g->stackFrames, g->stackFactor, g->stack.format);
    HIP_TRY(hipGetLastError());
    g->stackLast = o.stack;
    return 1;
}

// What a call that would leave a tick undrawn, or move the frames under the stacks, answers while they are attached, in the streams' style.  0: none attached
int stack_refuses(const mv_gym *g, const std::string &who, const char *clause)
{
    if (!g->stack.buf) return 0;
    const std::string noun = obs_stream(OPT_STACK_OBS).noun;
    return fail(who + ": " + noun + " are attached (" + opt().setter + "), " + clause + ": detach the " + noun + " first");
}

void stack_obs_free(mv_gym *g) { g->stack = ObsPlanes(); g->stackLast = nullptr; g->stackFrames = g->stackFactor = 0; }   // (the buffer is the caller's -- forgotten, not freed)

}  // namespace mvapi

extern "C" {

int mv_set_stack_obs(mv_gym *g, void *device_buf, int32_t frames, int32_t factor, int32_t format)
{
    const std::string who = opt().setter;
    if (attach_check(g, opt().setter, opt())) return -1;
    if (!device_buf) {
        stack_obs_free(g);
        g->simMustWaitUser = true;
        return 0;
    }
    for (int which : {OPT_DRAW_MASK, OPT_STILL_FRAMES})
        if (gym_options[which].on(g))
            return fail(who + ": the gym has " + gym_options[which].has + " (" + gym_options[which].setter + "), and a frame that is not drawn would tear the stack: "
                        + gym_options[which].detach);
    if (g->w > MAX_W || g->h > MAX_H) return fail(who + ": observation size above 1024x1024");   // (the passes draw no such frame)
    if (const char *why = stack_args_refusal(g->w, g->h, frames, factor, format)) return fail(who + ": " + why);
    if ((uintptr_t)device_buf % 16) return fail(who + ": the buffer must be 16-byte aligned");
    g->stack.buf = device_buf;
    g->stack.format = format;
    g->stack.entries = std::max(1, g->ringCount);
    g->stack.entryBytes = (size_t)g->N * g->A * stack_frame_bytes(frames, format, g->w / factor, g->h / factor);
    g->stackFrames = frames;
    g->stackFactor = factor;
    g->stackLast = nullptr;
    g->simMustWaitUser = true;   // an ordering point, as the planes' setters
    return 0;
}

int mv_get_stack_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_stack_obs")) return -1;
    return g->stack.buf ? g->stack.entries : 0;
}

int mv_stack_obs_shape(const mv_gym *g, int32_t *out4)
{
    if (getter_check(g, "mv_stack_obs_shape")) return -1;
    if (!out4) return fail("mv_stack_obs_shape: null pointer");
    const bool on = g->stack.buf != nullptr;
    out4[0] = on ? g->stackFrames : 0;
    out4[1] = on ? stack_channels(g->stack.format) : 0;
    out4[2] = on ? g->h / g->stackFactor : 0;
    out4[3] = on ? g->w / g->stackFactor : 0;
    return 0;
}

int mv_get_stack_observation(mv_gym *g, int32_t env, int32_t agent, uint8_t *out_host)
{
    const std::string who = "mv_get_stack_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->stack.buf) return fail(who + ": no " + obs_stream(OPT_STACK_OBS).noun + " attached (" + opt().setter + ")");
    if (!out_host) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t bytes = stack_frame_bytes(g->stackFrames, g->stack.format, g->w / g->stackFactor, g->h / g->stackFactor);
    const uint8_t *src = (const uint8_t *)last_outputs(g).stack + ((size_t)env * g->A + agent) * bytes;
    HIP_TRY(hipMemcpyAsync(out_host, src, bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_stack_host(const void *frame, int32_t layout, int32_t w, int32_t h, int32_t frames, int32_t factor, int32_t format, int32_t clear, const uint8_t *prev,
                        uint8_t *out)
{
    if (stack_debug_check("mv_debug_stack_host", frame, layout, w, h, frames, factor, format, prev, out)) return -1;
    stack_obs_host((const uint8_t *)frame, layout, w, h, frames, factor, format, clear != 0, prev, out);
    return 0;
}

int mv_debug_stack_device(const void *frame, int32_t layout, int32_t w, int32_t h, int32_t frames, int32_t factor, int32_t format, int32_t clear, const uint8_t *prev,
                          uint8_t *out)
{
    const std::string who = "mv_debug_stack_device";
    if (stack_debug_check(who, frame, layout, w, h, frames, factor, format, prev, out)) return -1;
    if ((uintptr_t)frame % 4 || (uintptr_t)prev % 16 || (uintptr_t)out % 16) return fail(who + ": the frame must be 4-byte aligned, the stacks 16-byte aligned");
    // ONE frame, drawn
    stack_launch(nullptr, 1, nullptr, 1, StackClearArgs{clear != 0 ? 1 : 0, 0, nullptr, nullptr, nullptr}, frame, layout, prev, out, w, h, frames, factor, format);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

}  // extern "C"
