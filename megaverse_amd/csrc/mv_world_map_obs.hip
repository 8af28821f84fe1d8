// megaverse_amd/csrc/mv_world_map_obs.hip -- world map observations (mv_world_map_obs.h has the record and its rule): the merging kernel, its launch behind the
// depth and label planes of a drawn tick, and the host side of mv_set_world_map_obs / mv_get_world_map_obs / mv_world_map_obs_cells /
// mv_get_world_map_observation / mv_debug_world_map_host / mv_debug_world_map_device (include/megaverse_hip.h).  DESIGN.md 3.27.
//
// The kernel: one workgroup of 256 lanes per frame, reading the frame's depth plane and label plane [H][W] from the caller's buffers -- behind the launch that
// wrote them, on the same stream -- and merging them into the AGENT's own grid [3][M][M] int16, which it reads and writes in place.
//   prologue  the viewer's record eye(3) c(9), twelve floats of the tick's frame header, and the byte(s) that say whether the grid is cleared first (the tick's
//             staged done[env]; a reset's mask), all at workgroup-uniform addresses (scalar loads, scalar registers).  An undrawn frame leaves here, before any
//             load or store of the grid.  Then the LDS accumulators, M * M keys and M * M counts (32 KB at M = 64): zeros on a clear; otherwise the grid as it
//             stands -- three 16-byte loads per lane and round, eight cells of each plane, decoded to key and count (world_map_cell_state): map_obs_kernel's
//             epilogue run backwards.  And the W column abscissae x(px) in LDS, as map_obs_kernel builds them.
//   body      map_obs_kernel's: a lane takes 8 horizontally adjacent pixels per round with 16-byte depth and label loads (the formats are template axes; a chunk
//             that is short or off the 16-byte grid is loaded value by value), pushes each through world_map_pixel, merges consecutive pixels of one cell and
//             issues one ds_add_u32 + one ds_max_u32 per run.
//   epilogue  8 cells per lane and round, saturated and packed (map_cell_bits), three 16-byte stores back to the same grid.
// Two ticks of one agent never run concurrently -- the launches of one gym follow each other on its stream -- and the workgroups of one launch own disjoint
// grids: no global atomics.  Every lane has read its part of the grid before the first barrier and no lane stores before the second.
#include "mv_api_internal.h"
#include "mv_world_map_obs.h"

#include <cmath>

namespace mv {

constexpr int WMAP_THREADS = 256, WMAP_CHUNK = 8;
static_assert(FH_CAM == 0 && MAP_CAM_FLOATS <= FH_COUNT, "eye(3) c(9) are the first twelve floats of a camera record");
static_assert(MAP_CELLS_STEP % WMAP_CHUNK == 0, "the prologue and the epilogue take cells by eights");

// When a frame's grid is read as zeros: all -- every frame (mv_reset; the debug hook's clear); done[env] -- the tick's staged done flags; mask[env] (and,
// applied given, applied[env]) -- the envs a masked reset flagged and that took their next episode.  Null pointers say nothing.
struct WorldMapClearArgs {
    int32_t all;
    const uint8_t *done, *mask, *applied;
};

// one byte at a workgroup-uniform address, read as the aligned word that holds it: a scalar load (the word lies in the byte's own 4-byte cell, so in its page)
__device__ __forceinline__ uint32_t uniform_byte(const uint8_t *p)
{
    const uint32_t off = (uint32_t)((uintptr_t)p & 3u);   // (pointer arithmetic, not an integer's cast: the address stays a global one)
    return (*reinterpret_cast<const uint32_t *>(p - off) >> (8u * off)) & 0xffu;
}

// frames: the grid.  cams + frame * cam_stride + FH_CAM_STRIDE * (frame % A): the viewer's record eye(3) c(9) (the tick's frame headers: cam_stride =
// FRAME_HDR_BYTES / 4).  vis_count: the tick's list lengths, null: every frame counts as drawn (mv_debug_world_map_device).  depth, seg: [frames][H][W] values
// of the formats DF, SF; grids: [frames][3][M][M], 16-byte aligned, read and written; W <= MAX_W
template <int DF, int SF>
__global__ __launch_bounds__(WMAP_THREADS) void world_map_obs_kernel(const int32_t *__restrict__ vis_count, const float *__restrict__ cams, int cam_stride, int A,
                                                                      WorldMapClearArgs clr, const void *__restrict__ depth, const void *__restrict__ seg,
                                                                      int16_t *grids, int W, int H, int M, float inv, float ox, float oz)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_key[MAP_CELLS_MAX * MAP_CELLS_MAX];
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[MAP_CELLS_MAX * MAP_CELLS_MAX];
    __shared__ __attribute__((aligned(16))) float s_x[MAX_W];
    const int frame = blockIdx.x, tid = threadIdx.x, env = frame / A;

    // ---- prologue
    float cam[MAP_CAM_FLOATS];
    {
        const float *cp = cams + (size_t)frame * cam_stride + FH_CAM_STRIDE * (frame % A);
#pragma unroll
        for (int q = 0; q < MAP_CAM_FLOATS; ++q) cam[q] = cp[q];
    }
    bool clear = clr.all != 0;
    if (clr.done) clear = clear || uniform_byte(clr.done + env) != 0u;
    if (clr.mask) clear = clear || (uniform_byte(clr.mask + env) != 0u && (!clr.applied || uniform_byte(clr.applied + env) != 0u));
    if (vis_count && vis_count[frame] < 0) return;   // (uniform) an undrawn frame: the grid is neither read nor written

    const int cells = M * M;
    int16_t *grid = grids + (size_t)frame * map_frame_values(M);
    if (clear) {
        for (int i = tid; i < cells; i += WMAP_THREADS) { s_key[i] = 0u; s_cnt[i] = 0u; }
    } else {
        for (int g8 = tid; g8 < cells / WMAP_CHUNK; g8 += WMAP_THREADS) {
            uint4 pl[MAP_OBS_PLANES];
#pragma unroll
            for (int q = 0; q < MAP_OBS_PLANES; ++q) pl[q] = reinterpret_cast<const uint4 *>(grid + (size_t)q * cells)[g8];
            const uint32_t w[MAP_OBS_PLANES][WMAP_CHUNK / 2] = {{pl[0].x, pl[0].y, pl[0].z, pl[0].w}, {pl[1].x, pl[1].y, pl[1].z, pl[1].w},
                                                               {pl[2].x, pl[2].y, pl[2].z, pl[2].w}};
            uint32_t k[WMAP_CHUNK], cn[WMAP_CHUNK];
#pragma unroll
            for (int i = 0; i < WMAP_CHUNK; ++i) {
                uint32_t v[MAP_OBS_PLANES];
#pragma unroll
                for (int q = 0; q < MAP_OBS_PLANES; ++q) {
                    v[q] = (w[q][i >> 1] >> (16 * (i & 1))) & 0xffffu;
                    asm volatile("" : "+v"(v[q]));   // (as in the epilogue: the halves stay 32-bit values, out of the SLP vectoriser's <2 x i16> forms)
                }
                world_map_cell_state(v[0], v[1], v[2], k[i], cn[i]);
            }
            reinterpret_cast<uint4 *>(s_key)[2 * g8] = make_uint4(k[0], k[1], k[2], k[3]);
            reinterpret_cast<uint4 *>(s_key)[2 * g8 + 1] = make_uint4(k[4], k[5], k[6], k[7]);
            reinterpret_cast<uint4 *>(s_cnt)[2 * g8] = make_uint4(cn[0], cn[1], cn[2], cn[3]);
            reinterpret_cast<uint4 *>(s_cnt)[2 * g8 + 1] = make_uint4(cn[4], cn[5], cn[6], cn[7]);
        }
    }
    for (int i = tid; i < W; i += WMAP_THREADS) s_x[i] = map_ray_x(i, W);
    __syncthreads();

    // ---- body
    typedef typename std::conditional<DF == DEPTH_F16, uint16_t, float>::type DepthT;
    typedef typename std::conditional<SF == SEG_INSTANCE_U16, uint16_t, uint8_t>::type LabelT;
    const int chunksPerRow = (W + WMAP_CHUNK - 1) / WMAP_CHUNK, items = chunksPerRow * H;
    const DepthT *dplane = reinterpret_cast<const DepthT *>(depth) + (size_t)frame * W * H;
    const LabelT *lplane = reinterpret_cast<const LabelT *>(seg) + (size_t)frame * W * H;
    for (int it = tid; it < items; it += WMAP_THREADS) {
        const int py = it / chunksPerRow, x0 = (it - py * chunksPerRow) * WMAP_CHUNK;
        const int n = min((int)WMAP_CHUNK, W - x0);   // (the row's tail chunk holds fewer)
        const DepthT *dp = dplane + (size_t)py * W + x0;
        const LabelT *lp = lplane + (size_t)py * W + x0;
        float t[WMAP_CHUNK], x[WMAP_CHUNK];
        uint32_t l[WMAP_CHUNK];
        if (n == WMAP_CHUNK && ((uintptr_t)dp & 15u) == 0) {
            if constexpr (DF == DEPTH_F16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(dp);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < WMAP_CHUNK; ++i) t[i] = depth_f16_to_f32((uint16_t)(w[i >> 1] >> (16 * (i & 1))));
            } else {
                const float4 a = reinterpret_cast<const float4 *>(dp)[0], b = reinterpret_cast<const float4 *>(dp)[1];
                t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < WMAP_CHUNK; ++i) t[i] = i < n ? map_depth_at(dp, DF, i) : 0.0f;   // (a pixel past the row's end: no hit)
        }
        if (n == WMAP_CHUNK && ((uintptr_t)lp & (WMAP_CHUNK * sizeof(LabelT) - 1)) == 0) {
            if constexpr (SF == SEG_INSTANCE_U16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(lp);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < WMAP_CHUNK; ++i) l[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
            } else {
                const uint2 v = *reinterpret_cast<const uint2 *>(lp);
                const uint32_t w[2] = {v.x, v.y};
#pragma unroll
                for (int i = 0; i < WMAP_CHUNK; ++i) l[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
            }
        } else {
#pragma unroll
            for (int i = 0; i < WMAP_CHUNK; ++i) l[i] = i < n ? map_label_at(lp, SF, i) : 0u;
        }
        if (n == WMAP_CHUNK) {   // (x0 is a multiple of 8: 32-byte aligned in s_x)
            const float4 a = reinterpret_cast<const float4 *>(s_x + x0)[0], b = reinterpret_cast<const float4 *>(s_x + x0)[1];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < WMAP_CHUNK; ++i) x[i] = i < n ? s_x[x0 + i] : 0.0f;
        }
        const float y = map_ray_y(py, H);
        // the lane's runs: consecutive pixels of one cell are one add and one max
        int runCell = -1;
        uint32_t runKey = 0u, runCount = 0u;
#pragma unroll
        for (int i = 0; i < WMAP_CHUNK; ++i) {
            int cell;
            uint32_t key;
            if (!world_map_pixel(cam, x[i], y, t[i], map_class_of(l[i], SF), inv, ox, oz, M, cell, key)) continue;
            if (cell != runCell) {
                if (runCount) { atomicAdd(&s_cnt[runCell], runCount); atomicMax(&s_key[runCell], runKey); }
                runCell = cell; runKey = key; runCount = 1u;
            } else {
                runKey = max(runKey, key); ++runCount;
            }
        }
        if (runCount) { atomicAdd(&s_cnt[runCell], runCount); atomicMax(&s_key[runCell], runKey); }
    }
    __syncthreads();

    // ---- epilogue
    for (int g8 = tid; g8 < cells / WMAP_CHUNK; g8 += WMAP_THREADS) {
        const uint4 ka = reinterpret_cast<const uint4 *>(s_key)[2 * g8], kb = reinterpret_cast<const uint4 *>(s_key)[2 * g8 + 1];
        const uint4 ca = reinterpret_cast<const uint4 *>(s_cnt)[2 * g8], cb = reinterpret_cast<const uint4 *>(s_cnt)[2 * g8 + 1];
        const uint32_t k[WMAP_CHUNK] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w}, cn[WMAP_CHUNK] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
        uint32_t p[MAP_OBS_PLANES][WMAP_CHUNK / 2] = {};
#pragma unroll
        for (int i = 0; i < WMAP_CHUNK; ++i) {
            uint32_t v[MAP_OBS_PLANES];
            map_cell_bits(k[i], cn[i], v[0], v[1], v[2]);
#pragma unroll
            for (int q = 0; q < MAP_OBS_PLANES; ++q) {
                asm volatile("" : "+v"(v[q]));   // (mv_map_obs.hip's epilogue says why: it costs no instruction)
                p[q][i >> 1] |= v[q] << (16 * (i & 1));
            }
        }
#pragma unroll
        for (int q = 0; q < MAP_OBS_PLANES; ++q)
            reinterpret_cast<uint4 *>(grid + (size_t)q * cells)[g8] = make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
    }
}

// one launch of the kernel for the planes' formats (uniform per launch: the template axes)
static void world_map_launch(hipStream_t stream, int frames, const int32_t *vis_count, const float *cams, int cam_stride, int A, const WorldMapClearArgs &clr,
                             const void *depth, int depth_format, const void *seg, int seg_format, int16_t *grids, int W, int H, int M, float inv, float ox, float oz)
{
    const dim3 grid((unsigned)frames), block(WMAP_THREADS);
#define MV_WMAP_LAUNCH(DF, SF) \
    hipLaunchKernelGGL((world_map_obs_kernel<DF, SF>), grid, block, 0, stream, vis_count, cams, cam_stride, A, clr, depth, seg, grids, W, H, M, inv, ox, oz)
    if (depth_format == DEPTH_F16) {
        if (seg_format == SEG_INSTANCE_U16) MV_WMAP_LAUNCH(DEPTH_F16, SEG_INSTANCE_U16);
        else MV_WMAP_LAUNCH(DEPTH_F16, SEG_CLASS_U8);
    } else {
        if (seg_format == SEG_INSTANCE_U16) MV_WMAP_LAUNCH(DEPTH_F32, SEG_INSTANCE_U16);
        else MV_WMAP_LAUNCH(DEPTH_F32, SEG_CLASS_U8);
    }
#undef MV_WMAP_LAUNCH
}

}  // namespace mv

namespace mvapi {

namespace {
const GymOption &opt() { return gym_options[OPT_WORLD_MAP_OBS]; }

// what both debug hooks refuse, before either touches a byte
int world_map_args_check(const std::string &who, const void *depth, int depth_format, const void *seg, int seg_format, int w, int h, const float *cam12, int cells,
                         float cell_size, float ox, float oz, const int16_t *grid)
{
    if (!depth || !seg || !cam12 || !grid) return fail(who + ": null pointer");
    if (!depth_format_known(depth_format)) return fail(who + ": unknown depth format (MV_DEPTH_F32, MV_DEPTH_F16)");
    if (!seg_format_known(seg_format)) return fail(who + ": unknown label format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)");
    if (w < 1 || h < 1 || w > MAX_W || h > MAX_H) return fail(who + ": a plane is between 1x1 and 1024x1024");
    if (!map_cells_known(cells)) return fail(who + ": cells must be a multiple of 8 in [8, 64]");
    if (!std::isfinite(cell_size) || !(cell_size > 0.0f)) return fail(who + ": cell_size must be a finite number > 0");
    if (!std::isfinite(ox) || !std::isfinite(oz)) return fail(who + ": the origin must be finite");
    return 0;
}
}  // namespace

// The frames whose planes o.depth and o.seg hold, merged into the agents' grids: ONE launch on the caller's stream behind whatever wrote the planes and behind
// map_follow; v: the tick's view (its slot says which frames were drawn, its headers hold the cameras they were drawn with).  clear: which grids are read as
// zeros first -- the frames that are the first of a new episode:
//   a stepping call's tick    {done = the view's done}: the tick's STAGED done[env], the value the episode log reads (the env's header has run ahead in a batched
//                             call; the call stages while world maps are attached, StepCall::plan)
//   mv_reset's frame          {all}
//   mv_reset_envs(render = 1) {mask, applied}: the flagged envs that took their next episode (a starved env stays in its episode: episode_log_cut's reading)
//   mv_render                 {}: merges again, clears nothing
// -> launches made (0: nothing attached), -1
int world_map_follow(mv_gym *g, const GymView &v, const OutPtrs &o, const WorldMapClear &clear)
{
    if (!g->worldMap || !o.depth || !o.seg) return 0;
    const WorldMapClearArgs clr{clear.all ? 1 : 0, clear.done, clear.mask, clear.applied};
    world_map_launch(g->stream, g->N * g->A, (const int32_t *)v.vis_count, (const float *)v.vis_hdr, FRAME_HDR_BYTES / (int)sizeof(float), g->A, clr, o.depth,
                     g->depth.format, o.seg, g->seg.format, (int16_t *)g->worldMap, g->w, g->h, g->worldMapCells, 1.0f / g->worldMapCellSize, g->worldMapOrigin[0],
                     g->worldMapOrigin[1]);
    HIP_TRY(hipGetLastError());
    g->mapLastHdr = v.vis_hdr;   // (mv_debug_map_camera serves both map streams)
    return 1;
}

// What a call that leaves a tick undrawn answers while world maps are attached, in the streams' style: such a tick could hide an episode's end.  0: none attached
int world_map_refuses(const mv_gym *g, const std::string &who, const char *clause)
{
    if (!g->worldMap) return 0;
    const std::string noun = obs_stream(OPT_WORLD_MAP_OBS).noun;
    return fail(who + ": " + noun + " are attached (" + opt().setter + "), " + clause + ": detach the " + noun + " first");
}

void world_map_obs_free(mv_gym *g) { g->worldMap = nullptr; g->worldMapCells = 0; g->worldMapCellSize = 0.0f; g->worldMapOrigin[0] = g->worldMapOrigin[1] = 0.0f; }   // (the buffer is the caller's -- forgotten, not freed)

}  // namespace mvapi

extern "C" {

int mv_set_world_map_obs(mv_gym *g, void *device_buf, int32_t cells, float cell_size, float origin_x, float origin_z)
{
    const std::string who = opt().setter;
    if (attach_check(g, opt().setter, opt())) return -1;
    if (!device_buf) {
        world_map_obs_free(g);
        g->simMustWaitUser = true;
        return 0;
    }
    if (!g->depth.buf) return fail(who + ": the points are unprojected from the depth planes: attach them first (mv_set_depth_obs)");
    if (!g->seg.buf) return fail(who + ": the cells' classes are read from the label planes: attach them first (mv_set_seg_obs)");
    if (gym_options[OPT_DRAW_MASK].on(g))
        return fail(who + ": the gym has " + gym_options[OPT_DRAW_MASK].has + " (" + gym_options[OPT_DRAW_MASK].setter
                    + "), and a frame that is not drawn could hide an episode's end: " + gym_options[OPT_DRAW_MASK].detach);
    if (!map_cells_known(cells)) return fail(who + ": cells must be a multiple of 8 in [8, 64]");
    if (!std::isfinite(cell_size) || !(cell_size > 0.0f)) return fail(who + ": cell_size must be a finite number > 0");
    if (!std::isfinite(origin_x) || !std::isfinite(origin_z)) return fail(who + ": the origin must be finite");
    if ((uintptr_t)device_buf % 16) return fail(who + ": the buffer must be 16-byte aligned");
    if (g->w > MAX_W || g->h > MAX_H) return fail(who + ": observation size above 1024x1024");   // (the passes draw no such frame; the kernel's column table holds MAX_W)
    g->worldMap = device_buf;
    g->worldMapCells = cells;
    g->worldMapCellSize = cell_size;
    g->worldMapOrigin[0] = origin_x;
    g->worldMapOrigin[1] = origin_z;
    g->simMustWaitUser = true;   // an ordering point, as the planes' setters
    return 0;
}

int mv_get_world_map_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_world_map_obs")) return -1;
    return g->worldMap ? 1 : 0;
}

int mv_world_map_obs_cells(const mv_gym *g)
{
    if (getter_check(g, "mv_world_map_obs_cells")) return -1;
    return g->worldMap ? g->worldMapCells : 0;
}

int mv_get_world_map_observation(mv_gym *g, int32_t env, int32_t agent, int16_t *out_host)
{
    const std::string who = "mv_get_world_map_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->worldMap) return fail(who + ": no " + obs_stream(OPT_WORLD_MAP_OBS).noun + " attached (" + opt().setter + ")");
    if (!out_host) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t values = map_frame_values(g->worldMapCells);
    const int16_t *src = (const int16_t *)g->worldMap + ((size_t)env * g->A + agent) * values;
    HIP_TRY(hipMemcpyAsync(out_host, src, values * sizeof(int16_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_world_map_host(const void *depth, int32_t depth_format, const void *seg, int32_t seg_format, int32_t w, int32_t h, const float *cam12, int32_t cells,
                            float cell_size, float origin_x, float origin_z, int32_t clear, int16_t *grid_inout)
{
    if (world_map_args_check("mv_debug_world_map_host", depth, depth_format, seg, seg_format, w, h, cam12, cells, cell_size, origin_x, origin_z, grid_inout)) return -1;
    std::vector<uint32_t> scratch((size_t)2 * cells * cells);
    world_map_obs_host(depth, depth_format, seg, seg_format, w, h, cam12, cells, cell_size, origin_x, origin_z, clear != 0, scratch.data(),
                       scratch.data() + (size_t)cells * cells, grid_inout);
    return 0;
}

int mv_debug_world_map_device(const void *depth, int32_t depth_format, const void *seg, int32_t seg_format, int32_t w, int32_t h, const float *cam12, int32_t cells,
                              float cell_size, float origin_x, float origin_z, int32_t clear, int16_t *grid_inout)
{
    const std::string who = "mv_debug_world_map_device";
    if (world_map_args_check(who, depth, depth_format, seg, seg_format, w, h, cam12, cells, cell_size, origin_x, origin_z, grid_inout)) return -1;
    if ((uintptr_t)depth % depth_value_bytes(depth_format) || (uintptr_t)seg % seg_value_bytes(seg_format) || (uintptr_t)cam12 % sizeof(float)
        || (uintptr_t)grid_inout % 16)
        return fail(who + ": the planes and the camera must be aligned to their values, the grid to 16 bytes");
    // ONE frame, its camera record at cam12 itself (frame 0, agent 0), drawn
    world_map_launch(nullptr, 1, nullptr, cam12, 0, 1, WorldMapClearArgs{clear != 0 ? 1 : 0, nullptr, nullptr, nullptr}, depth, depth_format, seg, seg_format,
                     grid_inout, w, h, cells, 1.0f / cell_size, origin_x, origin_z);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

}  // extern "C"
