// megaverse_amd/csrc/mv_map_obs.hip -- map observations (mv_map_obs.h has the record and its rule): the binning kernel, its launch behind the depth and label
// planes of a drawn tick, and the host side of mv_set_map_obs / mv_get_map_obs / mv_map_obs_cells / mv_map_obs_cell_size / mv_get_map_observation /
// mv_debug_map_host / mv_debug_map_device / mv_debug_map_camera (include/megaverse_hip.h).  DESIGN.md 3.26.
//
// The kernel: one workgroup of 256 lanes per frame, reading the frame's depth plane and label plane [H][W] from the caller's buffers -- behind the launch that
// wrote them, on the same stream -- and writing the frame's [3][M][M] int16.
//   prologue  the viewer's basis, nine floats of the tick's frame header at a workgroup-uniform address (scalar loads, scalar registers); M * M key words and
//             M * M count words of LDS zeroed (32 KB at M = 64); the W column abscissae x(px) in LDS -- one correctly rounded division per column and
//             workgroup, none per pixel.
//   body      a lane takes 8 horizontally adjacent pixels per round: one 16-byte load of F16 depth or two of F32, 8 or 16 bytes of labels, two 16-byte LDS
//             reads of x; y(py) is one evaluation per lane and round.  The depth and label formats are template axes: no format test in the loop.  Each pixel
//             goes through map_pixel; the lane merges consecutive pixels of its 8 that land in the same cell (counts summed, keys maximised) and issues one
//             ds_add_u32 + one ds_max_u32 per run.  No wave-level merge on top (DESIGN.md 3.26 says why).  A chunk that is not whole (W % 8) or not 16-byte
//             aligned (an odd W's rows) is loaded value by value.
//   epilogue  every lane turns 8 cells at a time into the three planes: two 16-byte LDS reads of keys, two of counts, three 16-byte stores.
// A frame that was not drawn (mv_frame.h: frame_skip left a negative list length in the tick's slot) leaves before any store, as in visible_obs_kernel.
#include "mv_api_internal.h"
#include "mv_map_obs.h"

#include <cmath>

static_assert((int)MV_MAP_OBS_PLANES == (int)MAP_OBS_PLANES && (int)MV_MAP_HEIGHT_SCALE == (int)MAP_HEIGHT_SCALE, "the header's grid is the record's");

namespace mv {

constexpr int MAP_THREADS = 256, MAP_CHUNK = 8;
static_assert(FH_CAM == 0 && MAP_CAM_FLOATS <= FH_COUNT, "eye(3) c(9) are the first twelve floats of a camera record");
static_assert(MAP_CELLS_STEP % MAP_CHUNK == 0, "the epilogue takes cells by eights");

// frames: the grid.  cams + frame * cam_stride + FH_CAM_STRIDE * (frame % A): the viewer's record eye(3) c(9) (the tick's frame headers: cam_stride =
// FRAME_HDR_BYTES / 4).  vis_count: the tick's list lengths, null: every frame counts as drawn (mv_debug_map_device).  depth, seg: [frames][H][W] values of the
// formats DF, SF; out: [frames][3][M][M], 16-byte aligned; W <= MAX_W
template <int DF, int SF>
__global__ __launch_bounds__(MAP_THREADS) void map_obs_kernel(const int32_t *__restrict__ vis_count, const float *__restrict__ cams, int cam_stride, int A,
                                                               const void *__restrict__ depth, const void *__restrict__ seg, int16_t *__restrict__ out, int W, int H,
                                                               int M, float inv)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_key[MAP_CELLS_MAX * MAP_CELLS_MAX];
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[MAP_CELLS_MAX * MAP_CELLS_MAX];
    __shared__ __attribute__((aligned(16))) float s_x[MAX_W];
    const int frame = blockIdx.x, tid = threadIdx.x;
    if (vis_count && vis_count[frame] < 0) return;   // (uniform) an undrawn frame: nothing is written

    // ---- prologue
    float c[9];
    {
        const float *cp = cams + (size_t)frame * cam_stride + FH_CAM_STRIDE * (frame % A) + 3;
#pragma unroll
        for (int q = 0; q < 9; ++q) c[q] = cp[q];
    }
    const int cells = M * M;
    for (int i = tid; i < cells; i += MAP_THREADS) { s_key[i] = 0u; s_cnt[i] = 0u; }
    for (int i = tid; i < W; i += MAP_THREADS) s_x[i] = map_ray_x(i, W);
    __syncthreads();

    // ---- body
    typedef typename std::conditional<DF == DEPTH_F16, uint16_t, float>::type DepthT;
    typedef typename std::conditional<SF == SEG_INSTANCE_U16, uint16_t, uint8_t>::type LabelT;
    const int chunksPerRow = (W + MAP_CHUNK - 1) / MAP_CHUNK, items = chunksPerRow * H;
    const DepthT *dplane = reinterpret_cast<const DepthT *>(depth) + (size_t)frame * W * H;
    const LabelT *lplane = reinterpret_cast<const LabelT *>(seg) + (size_t)frame * W * H;
    for (int it = tid; it < items; it += MAP_THREADS) {
        const int py = it / chunksPerRow, x0 = (it - py * chunksPerRow) * MAP_CHUNK;
        const int n = min((int)MAP_CHUNK, W - x0);   // (the row's tail chunk holds fewer)
        const DepthT *dp = dplane + (size_t)py * W + x0;
        const LabelT *lp = lplane + (size_t)py * W + x0;
        float t[MAP_CHUNK], x[MAP_CHUNK];
        uint32_t l[MAP_CHUNK];
        if (n == MAP_CHUNK && ((uintptr_t)dp & 15u) == 0) {
            if constexpr (DF == DEPTH_F16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(dp);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < MAP_CHUNK; ++i) t[i] = depth_f16_to_f32((uint16_t)(w[i >> 1] >> (16 * (i & 1))));
            } else {
                const float4 a = reinterpret_cast<const float4 *>(dp)[0], b = reinterpret_cast<const float4 *>(dp)[1];
                t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < MAP_CHUNK; ++i) t[i] = i < n ? map_depth_at(dp, DF, i) : 0.0f;   // (a pixel past the row's end: no hit)
        }
        if (n == MAP_CHUNK && ((uintptr_t)lp & (MAP_CHUNK * sizeof(LabelT) - 1)) == 0) {
            if constexpr (SF == SEG_INSTANCE_U16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(lp);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < MAP_CHUNK; ++i) l[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
            } else {
                const uint2 v = *reinterpret_cast<const uint2 *>(lp);
                const uint32_t w[2] = {v.x, v.y};
#pragma unroll
                for (int i = 0; i < MAP_CHUNK; ++i) l[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
            }
        } else {
#pragma unroll
            for (int i = 0; i < MAP_CHUNK; ++i) l[i] = i < n ? map_label_at(lp, SF, i) : 0u;
        }
        if (n == MAP_CHUNK) {   // (x0 is a multiple of 8: 32-byte aligned in s_x)
            const float4 a = reinterpret_cast<const float4 *>(s_x + x0)[0], b = reinterpret_cast<const float4 *>(s_x + x0)[1];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < MAP_CHUNK; ++i) x[i] = i < n ? s_x[x0 + i] : 0.0f;
        }
        const float y = map_ray_y(py, H);
        // the lane's runs: consecutive pixels of one cell are one add and one max
        int runCell = -1;
        uint32_t runKey = 0u, runCount = 0u;
#pragma unroll
        for (int i = 0; i < MAP_CHUNK; ++i) {
            int cell;
            uint32_t key;
            if (!map_pixel(c, x[i], y, t[i], map_class_of(l[i], SF), inv, M, cell, key)) continue;
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
    int16_t *o = out + (size_t)frame * map_frame_values(M);
    for (int g8 = tid; g8 < cells / MAP_CHUNK; g8 += MAP_THREADS) {
        const uint4 ka = reinterpret_cast<const uint4 *>(s_key)[2 * g8], kb = reinterpret_cast<const uint4 *>(s_key)[2 * g8 + 1];
        const uint4 ca = reinterpret_cast<const uint4 *>(s_cnt)[2 * g8], cb = reinterpret_cast<const uint4 *>(s_cnt)[2 * g8 + 1];
        const uint32_t k[MAP_CHUNK] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w}, cn[MAP_CHUNK] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
        uint32_t p[MAP_OBS_PLANES][MAP_CHUNK / 2] = {};
#pragma unroll
        for (int i = 0; i < MAP_CHUNK; ++i) {
            uint32_t v[MAP_OBS_PLANES];
            map_cell_bits(k[i], cn[i], v[0], v[1], v[2]);
#pragma unroll
            for (int q = 0; q < MAP_OBS_PLANES; ++q) {
                // (an empty asm per value: left alone, the SLP vectoriser turns the packing into <2 x i16> operations that ROCm 7.2's instruction selection
                // crashes on; it costs no instruction)
                asm volatile("" : "+v"(v[q]));
                p[q][i >> 1] |= v[q] << (16 * (i & 1));
            }
        }
#pragma unroll
        for (int q = 0; q < MAP_OBS_PLANES; ++q)
            reinterpret_cast<uint4 *>(o + (size_t)q * cells)[g8] = make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
    }
}

// one launch of the kernel for the planes' formats (uniform per launch: the template axes)
static void map_launch(hipStream_t stream, int frames, const int32_t *vis_count, const float *cams, int cam_stride, int A, const void *depth, int depth_format,
                       const void *seg, int seg_format, int16_t *out, int W, int H, int M, float inv)
{
    const dim3 grid((unsigned)frames), block(MAP_THREADS);
    if (depth_format == DEPTH_F16) {
        if (seg_format == SEG_INSTANCE_U16)
            hipLaunchKernelGGL((map_obs_kernel<DEPTH_F16, SEG_INSTANCE_U16>), grid, block, 0, stream, vis_count, cams, cam_stride, A, depth, seg, out, W, H, M, inv);
        else hipLaunchKernelGGL((map_obs_kernel<DEPTH_F16, SEG_CLASS_U8>), grid, block, 0, stream, vis_count, cams, cam_stride, A, depth, seg, out, W, H, M, inv);
    } else {
        if (seg_format == SEG_INSTANCE_U16)
            hipLaunchKernelGGL((map_obs_kernel<DEPTH_F32, SEG_INSTANCE_U16>), grid, block, 0, stream, vis_count, cams, cam_stride, A, depth, seg, out, W, H, M, inv);
        else hipLaunchKernelGGL((map_obs_kernel<DEPTH_F32, SEG_CLASS_U8>), grid, block, 0, stream, vis_count, cams, cam_stride, A, depth, seg, out, W, H, M, inv);
    }
}

}  // namespace mv

namespace mvapi {

namespace {
const GymOption &opt() { return gym_options[OPT_MAP_OBS]; }

// what both debug hooks refuse, before either touches a byte
int map_args_check(const std::string &who, const void *depth, int depth_format, const void *seg, int seg_format, int w, int h, const float *cam12, int cells,
                   float cell_size, const int16_t *out)
{
    if (!depth || !seg || !cam12 || !out) return fail(who + ": null pointer");
    if (!depth_format_known(depth_format)) return fail(who + ": unknown depth format (MV_DEPTH_F32, MV_DEPTH_F16)");
    if (!seg_format_known(seg_format)) return fail(who + ": unknown label format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)");
    if (w < 1 || h < 1 || w > MAX_W || h > MAX_H) return fail(who + ": a plane is between 1x1 and 1024x1024");
    if (!map_cells_known(cells)) return fail(who + ": cells must be a multiple of 8 in [8, 64]");
    if (!std::isfinite(cell_size) || !(cell_size > 0.0f)) return fail(who + ": cell_size must be a finite number > 0");
    return 0;
}
}  // namespace

// The maps of the frames whose planes o.depth and o.seg hold -> o.map, the same tick's entry: ONE launch on the caller's stream behind whatever wrote the
// planes (the exact pass, or the planes' follower); v: the tick's view (its slot says which frames were drawn, its headers hold the cameras they were drawn
// with).  -> launches made (0: nothing attached), -1
int map_follow(mv_gym *g, const GymView &v, const OutPtrs &o)
{
    if (!o.map || !o.depth || !o.seg) return 0;
    map_launch(g->stream, g->N * g->A, (const int32_t *)v.vis_count, (const float *)v.vis_hdr, FRAME_HDR_BYTES / (int)sizeof(float), g->A, o.depth, g->depth.format,
               o.seg, g->seg.format, (int16_t *)o.map, g->w, g->h, g->mapCells, 1.0f / g->mapCellSize);
    HIP_TRY(hipGetLastError());
    g->mapLastHdr = v.vis_hdr;   // (mv_debug_map_camera)
    return 1;
}

void map_obs_free(mv_gym *g) { g->map = ObsPlanes(); g->mapCells = 0; g->mapCellSize = 0.0f; g->mapLastHdr = nullptr; }   // (the buffer is the caller's -- forgotten, not freed)

}  // namespace mvapi

extern "C" {

int mv_set_map_obs(mv_gym *g, void *device_buf, int32_t cells, float cell_size)
{
    const std::string who = opt().setter;
    if (attach_check(g, opt().setter, opt())) return -1;
    if (!device_buf) {
        map_obs_free(g);
        g->simMustWaitUser = true;
        return 0;
    }
    if (!g->depth.buf) return fail(who + ": the points are unprojected from the depth planes: attach them first (mv_set_depth_obs)");
    if (!g->seg.buf) return fail(who + ": the cells' classes are read from the label planes: attach them first (mv_set_seg_obs)");
    if (!map_cells_known(cells)) return fail(who + ": cells must be a multiple of 8 in [8, 64]");
    if (!std::isfinite(cell_size) || !(cell_size > 0.0f)) return fail(who + ": cell_size must be a finite number > 0");
    if ((uintptr_t)device_buf % 16) return fail(who + ": the buffer must be 16-byte aligned");
    if (g->w > MAX_W || g->h > MAX_H) return fail(who + ": observation size above 1024x1024");   // (the passes draw no such frame; the kernel's column table holds MAX_W)
    g->map.buf = device_buf;
    g->map.format = 0;
    g->map.entries = std::max(1, g->ringCount);
    g->map.entryBytes = (size_t)g->N * g->A * map_frame_values(cells) * sizeof(int16_t);
    g->mapCells = cells;
    g->mapCellSize = cell_size;
    g->mapLastHdr = nullptr;
    g->simMustWaitUser = true;   // an ordering point, as the planes' setters
    return 0;
}

int mv_get_map_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_map_obs")) return -1;
    return g->map.buf ? g->map.entries : 0;
}

int mv_map_obs_cells(const mv_gym *g)
{
    if (getter_check(g, "mv_map_obs_cells")) return -1;
    return g->map.buf ? g->mapCells : 0;
}

float mv_map_obs_cell_size(const mv_gym *g)
{
    if (getter_check(g, "mv_map_obs_cell_size")) return -1.0f;
    return g->map.buf ? g->mapCellSize : 0.0f;
}

int mv_get_map_observation(mv_gym *g, int32_t env, int32_t agent, int16_t *out_host)
{
    const std::string who = "mv_get_map_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->map.buf) return fail(who + ": no " + obs_stream(OPT_MAP_OBS).noun + " attached (" + opt().setter + ")");
    if (!out_host) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t values = map_frame_values(g->mapCells);
    const int16_t *src = (const int16_t *)last_outputs(g).map + ((size_t)env * g->A + agent) * values;
    HIP_TRY(hipMemcpyAsync(out_host, src, values * sizeof(int16_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_map_host(const void *depth, int32_t depth_format, const void *seg, int32_t seg_format, int32_t w, int32_t h, const float *cam12, int32_t cells,
                      float cell_size, int16_t *out)
{
    if (map_args_check("mv_debug_map_host", depth, depth_format, seg, seg_format, w, h, cam12, cells, cell_size, out)) return -1;
    std::vector<uint32_t> scratch((size_t)2 * cells * cells);
    map_obs_host(depth, depth_format, seg, seg_format, w, h, cam12, cells, cell_size, scratch.data(), scratch.data() + (size_t)cells * cells, out);
    return 0;
}

int mv_debug_map_device(const void *depth, int32_t depth_format, const void *seg, int32_t seg_format, int32_t w, int32_t h, const float *cam12, int32_t cells,
                        float cell_size, int16_t *out)
{
    const std::string who = "mv_debug_map_device";
    if (map_args_check(who, depth, depth_format, seg, seg_format, w, h, cam12, cells, cell_size, out)) return -1;
    if ((uintptr_t)depth % depth_value_bytes(depth_format) || (uintptr_t)seg % seg_value_bytes(seg_format) || (uintptr_t)cam12 % sizeof(float) || (uintptr_t)out % 16)
        return fail(who + ": the planes and the camera must be aligned to their values, out to 16 bytes");
    // ONE frame, its camera record at cam12 itself (frame 0, agent 0), drawn
    map_launch(nullptr, 1, nullptr, cam12, 0, 1, depth, depth_format, seg, seg_format, out, w, h, cells, 1.0f / cell_size);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

int mv_debug_map_camera(mv_gym *g, int32_t env, int32_t agent, float *out12)
{
    const std::string who = "mv_debug_map_camera";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!out12) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    if (!g->mapLastHdr)   // (either map stream's launch leaves the headers it followed: mv_world_map_obs.hip)
        return fail(who + ": no frame has been drawn with " + obs_stream(OPT_MAP_OBS).noun + " or " + obs_stream(OPT_WORLD_MAP_OBS).noun + " attached (" + opt().setter
                    + ", " + gym_options[OPT_WORLD_MAP_OBS].setter + ")");
    HIP_TRY(hipSetDevice(g->device));
    const uint8_t *src = (const uint8_t *)g->mapLastHdr + ((size_t)env * g->A + agent) * FRAME_HDR_BYTES + (size_t)(FH_CAM + FH_CAM_STRIDE * agent) * sizeof(float);
    HIP_TRY(hipMemcpyAsync(out12, src, MAP_CAM_FLOATS * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

}  // extern "C"
