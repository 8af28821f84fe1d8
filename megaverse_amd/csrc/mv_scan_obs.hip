// megaverse_amd/csrc/mv_scan_obs.hip -- scan observations (mv_scan_obs.h has the record and its rule): the binning kernel, its launch behind the depth and label
// planes of a drawn tick, and the host side of mv_set_scan_obs / mv_get_scan_obs / mv_scan_obs_beams / mv_get_scan_observation / mv_debug_scan_host /
// mv_debug_scan_device (include/megaverse_hip.h).  DESIGN.md 3.28.
//
// The kernel: one workgroup of 256 lanes per frame, reading the frame's depth plane and label plane [H][W] from the caller's buffers -- behind the launch that
// wrote them, on the same stream -- and writing the frame's [3][K] int16.  A beam gets almost exactly a pixel COLUMN (a level camera: exactly one; a pitched
// one: it drifts by a few columns over the frame's height), so the lanes own column strips and keep the beams' running values in registers:
//   prologue  the viewer's basis, nine floats of the tick's frame header at a workgroup-uniform address (scalar loads, scalar registers); K keys set to
//             SCAN_EMPTY_KEY and K counts zeroed in LDS (2 KB at K = 256).
//   body      with C = ceil(W / 8) chunks per row and R = max(1, 256 / C) row phases, strip s = phase * C + chunk: lane l takes the strips l, l + 256, ... (ONE
//             strip while C <= 256, which MAX_W = 1024 makes every frame; C * R <= 256 of the lanes have one) and in its strip the rows phase, phase + R, ...
//             The 64 lanes of a wave then hold 64 / C whole consecutive rows (C <= 64): their loads cover full lines.  Per row a lane does one 16-byte load
//             of F16 depth or two of F32 and 8 or 16 bytes of labels (the formats are template axes); a chunk that is not whole (W % 8) or not 16-byte
//             aligned (an odd W's rows) is loaded value by value.  x(px) of the lane's 8 columns is formed once per strip, y(py) once per row.  Each pixel
//             goes through scan_pixel.  Per column the lane keeps (beam, key, count) in registers: a pixel of the accumulator's beam costs one v_min_u32 and
//             one add; another beam flushes the accumulator -- one ds_min_u32 + one ds_add_u32 -- and restarts it.  The LDS atomics per lane are O(beam changes
//             down a column), not O(pixels): 8 flushes per lane and strip with a level camera.
//   epilogue  lane i < K / 8 turns beams 8 i .. 8 i + 7 into the three planes: two 16-byte LDS reads of keys, two of counts, three 16-byte stores.
// A frame that was not drawn (mv_frame.h: frame_skip left a negative list length in the tick's slot) leaves before any store, as in map_obs_kernel.
#include "mv_api_internal.h"
#include "mv_scan_obs.h"

#include <cmath>

static_assert((int)MV_SCAN_OBS_PLANES == (int)SCAN_OBS_PLANES && (int)MV_SCAN_RANGE_SCALE == (int)SCAN_RANGE_SCALE, "the header's fan is the record's");

namespace mv {

constexpr int SCAN_THREADS = 256, SCAN_CHUNK = 8;
static_assert(FH_CAM == 0 && MAP_CAM_FLOATS <= FH_COUNT, "eye(3) c(9) are the first twelve floats of a camera record");
static_assert(SCAN_BEAMS_STEP % SCAN_CHUNK == 0 && SCAN_BEAMS_MAX / SCAN_CHUNK <= SCAN_THREADS, "the epilogue takes beams by eights, one lane each");

// one accumulator -> LDS (count 0: nothing was kept since the last flush)
__device__ __forceinline__ void scan_flush(uint32_t *s_key, uint32_t *s_cnt, int beam, uint32_t key, uint32_t count)
{
    if (count) { atomicMin(&s_key[beam], key); atomicAdd(&s_cnt[beam], count); }
}

// frames: the grid.  cams + frame * cam_stride + FH_CAM_STRIDE * (frame % A): the viewer's record eye(3) c(9) (the tick's frame headers: cam_stride =
// FRAME_HDR_BYTES / 4).  vis_count: the tick's list lengths, null: every frame counts as drawn (mv_debug_scan_device).  depth, seg: [frames][H][W] values of the
// formats DF, SF; out: [frames][3][K], 16-byte aligned; K: scan_beams_known
template <int DF, int SF>
__global__ __launch_bounds__(SCAN_THREADS) void scan_obs_kernel(const int32_t *__restrict__ vis_count, const float *__restrict__ cams, int cam_stride, int A,
                                                                 const void *__restrict__ depth, const void *__restrict__ seg, int16_t *__restrict__ out, int W, int H,
                                                                 int K, float bscale, float h_lo, float h_hi)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_key[SCAN_BEAMS_MAX];
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[SCAN_BEAMS_MAX];
    const int frame = blockIdx.x, tid = threadIdx.x;
    if (vis_count && vis_count[frame] < 0) return;   // (uniform) an undrawn frame: nothing is written

    // ---- prologue
    float c[9];
    {
        const float *cp = cams + (size_t)frame * cam_stride + FH_CAM_STRIDE * (frame % A) + 3;
#pragma unroll
        for (int q = 0; q < 9; ++q) c[q] = cp[q];
    }
    if (tid < K) { s_key[tid] = SCAN_EMPTY_KEY; s_cnt[tid] = 0u; }   // (K <= SCAN_BEAMS_MAX = SCAN_THREADS)
    __syncthreads();

    // ---- body
    typedef typename std::conditional<DF == DEPTH_F16, uint16_t, float>::type DepthT;
    typedef typename std::conditional<SF == SEG_INSTANCE_U16, uint16_t, uint8_t>::type LabelT;
    const int chunksPerRow = (W + SCAN_CHUNK - 1) / SCAN_CHUNK, phases = max(1, SCAN_THREADS / chunksPerRow), strips = chunksPerRow * phases;
    const DepthT *dplane = reinterpret_cast<const DepthT *>(depth) + (size_t)frame * W * H;
    const LabelT *lplane = reinterpret_cast<const LabelT *>(seg) + (size_t)frame * W * H;
    for (int strip = tid; strip < strips; strip += SCAN_THREADS) {
        const int phase = strip / chunksPerRow, x0 = (strip - phase * chunksPerRow) * SCAN_CHUNK;
        const int n = min((int)SCAN_CHUNK, W - x0);   // (the row's tail chunk holds fewer)
        float x[SCAN_CHUNK];
        int accBeam[SCAN_CHUNK];
        uint32_t accKey[SCAN_CHUNK], accCount[SCAN_CHUNK];
#pragma unroll
        for (int i = 0; i < SCAN_CHUNK; ++i) {
            x[i] = map_ray_x(min(x0 + i, W - 1), W);   // (a column past the row's end: its depth reads 0 below)
            accBeam[i] = -1; accKey[i] = SCAN_EMPTY_KEY; accCount[i] = 0u;
        }
        for (int py = phase; py < H; py += phases) {
            const DepthT *dp = dplane + (size_t)py * W + x0;
            const LabelT *lp = lplane + (size_t)py * W + x0;
            float t[SCAN_CHUNK];
            uint32_t l[SCAN_CHUNK];
            if (n == SCAN_CHUNK && ((uintptr_t)dp & 15u) == 0) {
                if constexpr (DF == DEPTH_F16) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(dp);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < SCAN_CHUNK; ++i) t[i] = depth_f16_to_f32((uint16_t)(w[i >> 1] >> (16 * (i & 1))));
                } else {
                    const float4 a = reinterpret_cast<const float4 *>(dp)[0], b = reinterpret_cast<const float4 *>(dp)[1];
                    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < SCAN_CHUNK; ++i) t[i] = i < n ? map_depth_at(dp, DF, i) : 0.0f;   // (a pixel past the row's end: no hit)
            }
            if (n == SCAN_CHUNK && ((uintptr_t)lp & (SCAN_CHUNK * sizeof(LabelT) - 1)) == 0) {
                if constexpr (SF == SEG_INSTANCE_U16) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(lp);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < SCAN_CHUNK; ++i) l[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
                } else {
                    const uint2 v = *reinterpret_cast<const uint2 *>(lp);
                    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
                    for (int i = 0; i < SCAN_CHUNK; ++i) l[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
                }
            } else {
#pragma unroll
                for (int i = 0; i < SCAN_CHUNK; ++i) l[i] = i < n ? map_label_at(lp, SF, i) : 0u;
            }
            const float y = map_ray_y(py, H);
#pragma unroll
            for (int i = 0; i < SCAN_CHUNK; ++i) {
                int beam;
                uint32_t key;
                if (!scan_pixel(c, x[i], y, t[i], map_class_of(l[i], SF), bscale, K, h_lo, h_hi, beam, key)) continue;
                if (beam != accBeam[i]) {
                    scan_flush(s_key, s_cnt, accBeam[i], accKey[i], accCount[i]);
                    accBeam[i] = beam; accKey[i] = key; accCount[i] = 1u;
                } else {
                    accKey[i] = min(accKey[i], key); ++accCount[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < SCAN_CHUNK; ++i) scan_flush(s_key, s_cnt, accBeam[i], accKey[i], accCount[i]);
    }
    __syncthreads();

    // ---- epilogue
    if (tid < K / SCAN_CHUNK) {
        int16_t *o = out + (size_t)frame * scan_frame_values(K);
        const uint4 ka = reinterpret_cast<const uint4 *>(s_key)[2 * tid], kb = reinterpret_cast<const uint4 *>(s_key)[2 * tid + 1];
        const uint4 ca = reinterpret_cast<const uint4 *>(s_cnt)[2 * tid], cb = reinterpret_cast<const uint4 *>(s_cnt)[2 * tid + 1];
        const uint32_t k[SCAN_CHUNK] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w}, cn[SCAN_CHUNK] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
        uint32_t p[SCAN_OBS_PLANES][SCAN_CHUNK / 2] = {};
#pragma unroll
        for (int i = 0; i < SCAN_CHUNK; ++i) {
            uint32_t v[SCAN_OBS_PLANES];
            scan_beam_bits(k[i], cn[i], v[0], v[1], v[2]);
#pragma unroll
            for (int q = 0; q < SCAN_OBS_PLANES; ++q) {
                asm volatile("" : "+v"(v[q]));   // (map_obs_kernel's: keeps the SLP vectoriser off the int16 packing; it costs no instruction)
                p[q][i >> 1] |= v[q] << (16 * (i & 1));
            }
        }
#pragma unroll
        for (int q = 0; q < SCAN_OBS_PLANES; ++q)
            reinterpret_cast<uint4 *>(o + (size_t)q * K)[tid] = make_uint4(p[q][0], p[q][1], p[q][2], p[q][3]);
    }
}

// one launch of the kernel for the planes' formats (uniform per launch: the template axes)
static void scan_launch(hipStream_t stream, int frames, const int32_t *vis_count, const float *cams, int cam_stride, int A, const void *depth, int depth_format,
                        const void *seg, int seg_format, int16_t *out, int W, int H, int K, float h_lo, float h_hi)
{
    const dim3 grid((unsigned)frames), block(SCAN_THREADS);
    const float bscale = scan_bscale(K);
#define MV_SCAN_GO(DF, SF) hipLaunchKernelGGL((scan_obs_kernel<DF, SF>), grid, block, 0, stream, vis_count, cams, cam_stride, A, depth, seg, out, W, H, K, bscale, h_lo, h_hi)
    if (depth_format == DEPTH_F16) {
        if (seg_format == SEG_INSTANCE_U16) MV_SCAN_GO(DEPTH_F16, SEG_INSTANCE_U16);
        else MV_SCAN_GO(DEPTH_F16, SEG_CLASS_U8);
    } else {
        if (seg_format == SEG_INSTANCE_U16) MV_SCAN_GO(DEPTH_F32, SEG_INSTANCE_U16);
        else MV_SCAN_GO(DEPTH_F32, SEG_CLASS_U8);
    }
#undef MV_SCAN_GO
}

}  // namespace mv

namespace mvapi {

namespace {
const GymOption &opt() { return gym_options[OPT_SCAN_OBS]; }

// what the setter and both debug hooks refuse of the fan's own arguments
int scan_fan_check(const std::string &who, int beams, float h_lo, float h_hi)
{
    if (!scan_beams_known(beams)) return fail(who + ": beams must be a multiple of 8 in [8, 256]");
    if (!std::isfinite(h_lo) || !std::isfinite(h_hi) || !(h_lo < h_hi)) return fail(who + ": the height band must be two finite numbers h_lo < h_hi");
    return 0;
}

// what both debug hooks refuse, before either touches a byte
int scan_args_check(const std::string &who, const void *depth, int depth_format, const void *seg, int seg_format, int w, int h, const float *cam12, int beams,
                    float h_lo, float h_hi, const int16_t *out)
{
    if (!depth || !seg || !cam12 || !out) return fail(who + ": null pointer");
    if (!depth_format_known(depth_format)) return fail(who + ": unknown depth format (MV_DEPTH_F32, MV_DEPTH_F16)");
    if (!seg_format_known(seg_format)) return fail(who + ": unknown label format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)");
    if (w < 1 || h < 1 || w > MAX_W || h > MAX_H) return fail(who + ": a plane is between 1x1 and 1024x1024");
    return scan_fan_check(who, beams, h_lo, h_hi);
}
}  // namespace

// The fans of the frames whose planes o.depth and o.seg hold -> o.scan, the same tick's entry: ONE launch on the caller's stream behind whatever wrote the
// planes (the exact pass, or the planes' follower); v: the tick's view (its slot says which frames were drawn, its headers hold the cameras they were drawn
// with).  -> launches made (0: nothing attached), -1
int scan_follow(mv_gym *g, const GymView &v, const OutPtrs &o)
{
    if (!o.scan || !o.depth || !o.seg) return 0;
    scan_launch(g->stream, g->N * g->A, (const int32_t *)v.vis_count, (const float *)v.vis_hdr, FRAME_HDR_BYTES / (int)sizeof(float), g->A, o.depth, g->depth.format,
                o.seg, g->seg.format, (int16_t *)o.scan, g->w, g->h, g->scanBeams, g->scanBand[0], g->scanBand[1]);
    HIP_TRY(hipGetLastError());
    g->mapLastHdr = v.vis_hdr;   // (mv_debug_map_camera: the cameras this launch read)
    return 1;
}

void scan_obs_free(mv_gym *g) { g->scan = ObsPlanes(); g->scanBeams = 0; g->scanBand[0] = g->scanBand[1] = 0.0f; }   // (the buffer is the caller's -- forgotten, not freed)

}  // namespace mvapi

extern "C" {

int mv_set_scan_obs(mv_gym *g, void *device_buf, int32_t beams, float h_lo, float h_hi)
{
    const std::string who = opt().setter;
    if (attach_check(g, opt().setter, opt())) return -1;
    if (!device_buf) {
        scan_obs_free(g);
        g->simMustWaitUser = true;
        return 0;
    }
    if (!g->depth.buf) return fail(who + ": the ranges are unprojected from the depth planes: attach them first (mv_set_depth_obs)");
    if (!g->seg.buf) return fail(who + ": the beams' classes are read from the label planes: attach them first (mv_set_seg_obs)");
    if (scan_fan_check(who, beams, h_lo, h_hi)) return -1;
    if ((uintptr_t)device_buf % 16) return fail(who + ": the buffer must be 16-byte aligned");
    if (g->w > MAX_W || g->h > MAX_H) return fail(who + ": observation size above 1024x1024");   // (the passes draw no such frame)
    g->scan.buf = device_buf;
    g->scan.format = 0;
    g->scan.entries = std::max(1, g->ringCount);
    g->scan.entryBytes = (size_t)g->N * g->A * scan_frame_values(beams) * sizeof(int16_t);
    g->scanBeams = beams;
    g->scanBand[0] = h_lo;
    g->scanBand[1] = h_hi;
    g->simMustWaitUser = true;   // an ordering point, as the planes' setters
    return 0;
}

int mv_get_scan_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_scan_obs")) return -1;
    return g->scan.buf ? g->scan.entries : 0;
}

int mv_scan_obs_beams(const mv_gym *g)
{
    if (getter_check(g, "mv_scan_obs_beams")) return -1;
    return g->scan.buf ? g->scanBeams : 0;
}

int mv_get_scan_observation(mv_gym *g, int32_t env, int32_t agent, int16_t *out_host)
{
    const std::string who = "mv_get_scan_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->scan.buf) return fail(who + ": no " + obs_stream(OPT_SCAN_OBS).noun + " attached (" + opt().setter + ")");
    if (!out_host) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t values = scan_frame_values(g->scanBeams);
    const int16_t *src = (const int16_t *)last_outputs(g).scan + ((size_t)env * g->A + agent) * values;
    HIP_TRY(hipMemcpyAsync(out_host, src, values * sizeof(int16_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_scan_host(const void *depth, int32_t depth_format, const void *seg, int32_t seg_format, int32_t w, int32_t h, const float *cam12, int32_t beams,
                       float h_lo, float h_hi, int16_t *out)
{
    if (scan_args_check("mv_debug_scan_host", depth, depth_format, seg, seg_format, w, h, cam12, beams, h_lo, h_hi, out)) return -1;
    std::vector<uint32_t> scratch((size_t)2 * beams);
    scan_obs_host(depth, depth_format, seg, seg_format, w, h, cam12, beams, h_lo, h_hi, scratch.data(), scratch.data() + beams, out);
    return 0;
}

int mv_debug_scan_device(const void *depth, int32_t depth_format, const void *seg, int32_t seg_format, int32_t w, int32_t h, const float *cam12, int32_t beams,
                         float h_lo, float h_hi, int16_t *out)
{
    const std::string who = "mv_debug_scan_device";
    if (scan_args_check(who, depth, depth_format, seg, seg_format, w, h, cam12, beams, h_lo, h_hi, out)) return -1;
    if ((uintptr_t)depth % depth_value_bytes(depth_format) || (uintptr_t)seg % seg_value_bytes(seg_format) || (uintptr_t)cam12 % sizeof(float) || (uintptr_t)out % 16)
        return fail(who + ": the planes and the camera must be aligned to their values, out to 16 bytes");
    // ONE frame, its camera record at cam12 itself (frame 0, agent 0), drawn
    scan_launch(nullptr, 1, nullptr, cam12, 0, 1, depth, depth_format, seg, seg_format, out, w, h, beams, h_lo, h_hi);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

}  // extern "C"
