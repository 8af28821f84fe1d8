// megaverse_amd/csrc/mv_visible_obs.hip -- visible-entity observations (mv_visible_obs.h has the record and its rule): the reduction kernel, its launch behind
// the label planes of a drawn tick, and the host side of mv_set_visible_obs / mv_get_visible_obs / mv_get_visible_observation / mv_debug_visible_host
// (include/megaverse_hip.h).  DESIGN.md 3.25.
//
// The kernel: one workgroup of 256 lanes per frame, reading the frame's instance label plane [H][W] from the caller's label buffer -- behind the launch that
// wrote it, on the same stream -- and writing the frame's [E][5] rows.
//   prologue  the env's EntityLayout from the launch's uniform arguments (scalar registers); Sokoban: the instance -> row table of the env's goal cells, 1024
//             bytes of LDS, filled from soko_cells in four rounds of 256 cells with wave ballots and a cross-wave prefix; the accumulator [192][5] in LDS:
//             count 0, the minima at INT_MAX, the maxima at -1.
//   body      a lane takes 8 words of one plane row per step, one 16-byte load where the chunk is whole and aligned, and maps them to row bytes packed
//             into one 64-bit register.  Labels come in long runs: the lane first merges its own equal neighbours into (row, first x, length), then the
//             wave merges by leader -- the first lane that still holds a run names the row, the lanes that hold the same row are reduced with shuffles
//             (count, x_min, x_max, y_min, y_max), and the leader alone issues the row's five LDS atomics.  LDS atomics per step are bounded by the distinct
//             rows a wave sees, and pixels that belong to no row cost none.
//   epilogue  E x 5 ints with plain vector stores; a row nobody counted is stored as five zeros, whatever its minima and maxima started as.
// A frame that was not drawn (mv_frame.h: frame_skip left a negative list length in the tick's slot) writes no byte, as its planes.
#include "mv_api_internal.h"
#include "mv_visible_obs.h"

static_assert((int)MV_VISIBLE_OBS_INTS == (int)VISIBLE_OBS_INTS, "the header's row is the record's");

namespace mv {

constexpr int VIS_THREADS = 256, VIS_WAVES = VIS_THREADS / 64, VIS_CHUNK = 8;
static_assert(VISIBLE_SOKO_SLOTS == 4 * VIS_THREADS, "the Sokoban table: one dword per lane, four rounds of cells");

__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// frames: N * A.  seg: [frames][H][W] words, out: [frames][E][5], both of the entry the tick's frames went to.
__global__ __launch_bounds__(VIS_THREADS) void visible_obs_kernel(const int32_t *__restrict__ vis_count, const EnvHeader *__restrict__ hdr,
                                                                   const uint8_t *__restrict__ soko_cells, int scen, int A, const uint16_t *__restrict__ seg,
                                                                   int32_t *__restrict__ out, int W, int H)
{
    __shared__ int32_t s_acc[ENTITY_MAX_ROWS * VISIBLE_OBS_INTS];
    __shared__ uint32_t s_soko32[VISIBLE_SOKO_SLOTS / 4];
    __shared__ int32_t s_wave[VIS_WAVES];
    uint8_t *const s_soko = reinterpret_cast<uint8_t *>(s_soko32);
    const int frame = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (vis_count[frame] < 0) return;   // (uniform) an undrawn or still frame: nothing is written
    const EntityLayout l = entity_layout(scen, A);

    // ---- prologue
    if (scen == SCN_SOKOBAN) {
        const int env = frame / A;
        const int roomW = max(hdr[env].W, 1);
        const uint8_t *cells = soko_cells + (size_t)env * (SOKO_DIM * SOKO_DIM);
        s_soko32[tid] = 0xffffffffu;   // VISIBLE_NO_ROW four times
        int running = 0;               // goal cells in the rounds before this one
        for (int j = 0; j < 4; ++j) {
            const int c = j * VIS_THREADS + tid;
            const bool goal = cells[c] == SOKO_GOAL;
            const unsigned long long b = __ballot(goal);
            const int before = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) s_wave[wave] = __popcll(b);
            __syncthreads();   // (round 0: also behind the table's fill)
            int below = 0, all = 0;
            for (int w2 = 0; w2 < VIS_WAVES; ++w2) {
                const int t = s_wave[w2];
                all += t;
                below += w2 < wave ? t : 0;
            }
            const int k = running + below + before, x = c / SOKO_DIM, z = c % SOKO_DIM;
            if (goal && z < roomW && x * roomW + z < VISIBLE_SOKO_SLOTS && k < ENTITY_SOKO_GOALS) s_soko[x * roomW + z] = (uint8_t)k;
            running += all;
            __syncthreads();   // (s_wave is rewritten by the next round)
        }
    }
    for (int i = tid; i < ENTITY_MAX_ROWS * VISIBLE_OBS_INTS; i += VIS_THREADS) {
        const int f = i % VISIBLE_OBS_INTS;
        s_acc[i] = f == 0 ? 0 : (f & 1) ? INT32_MAX : -1;   // count | x_min, y_min | x_max, y_max
    }
    __syncthreads();

    // ---- body
    const int chunksPerRow = (W + VIS_CHUNK - 1) / VIS_CHUNK, items = chunksPerRow * H;
    const uint16_t *plane = seg + (size_t)frame * W * H;
    for (int it0 = 0; it0 < items; it0 += VIS_THREADS) {   // (uniform trip count: the wave merge below needs every lane)
        const int it = it0 + tid;
        unsigned long long q = ~0ull;   // the chunk's rows, one byte per word, word 0 lowest
        int x = 0, y = 0, left = 0;
        if (it < items) {
            y = it / chunksPerRow;
            x = (it - y * chunksPerRow) * VIS_CHUNK;
            const int n = min((int)VIS_CHUNK, W - x);   // (the row's tail chunk holds fewer)
            const uint16_t *p = plane + (size_t)y * W + x;
            uint32_t w[4] = {0u, 0u, 0u, 0u};   // two words each; a word past the row's end stays 0, which names no row
            if (n == VIS_CHUNK && ((uintptr_t)p & 15u) == 0) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < VIS_CHUNK; ++i)
                    if (i < n) w[i >> 1] |= (uint32_t)p[i] << (16 * (i & 1));
            }
            q = 0;
#pragma unroll
            for (int i = 0; i < VIS_CHUNK; ++i) {
                const uint16_t word = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
                q |= (unsigned long long)visible_row_of(scen, l, word, s_soko) << (8 * i);
            }
            left = q == ~0ull ? 0 : VIS_CHUNK;
        }
        while (__ballot(left > 0)) {
            // the lane's next run: skip the words of no row, then take the equal neighbours
            while (left > 0 && (int)(q & 0xffu) == VISIBLE_NO_ROW) { q >>= 8; ++x; --left; }
            int row = -1, first = x, len = 0;
            if (left > 0) {
                row = (int)(q & 0xffu);
                do { q >>= 8; ++len; --left; } while (left > 0 && (int)(q & 0xffu) == row);
                x += len;
            }
            // the wave's merge, leader by leader
            unsigned long long active = __ballot(row >= 0);
            while (active) {
                const int leader = __ffsll(active) - 1;
                const int lr = __builtin_amdgcn_readlane(row, leader);
                const bool mine = row == lr;
                const int cnt = wave_sum(mine ? len : 0);
                const int x0 = wave_min(mine ? first : INT32_MAX), x1 = wave_max(mine ? first + len - 1 : -1);
                const int y0 = wave_min(mine ? y : INT32_MAX), y1 = wave_max(mine ? y : -1);
                if (lane == leader) {
                    int32_t *a = s_acc + lr * VISIBLE_OBS_INTS;
                    atomicAdd(a + 0, cnt);
                    atomicMin(a + 1, x0); atomicMax(a + 2, x1);
                    atomicMin(a + 3, y0); atomicMax(a + 4, y1);
                }
                active &= ~__ballot(mine);
            }
        }
    }
    __syncthreads();

    // ---- epilogue
    int32_t *o = out + (size_t)frame * l.total * VISIBLE_OBS_INTS;
    for (int i = tid; i < l.total * VISIBLE_OBS_INTS; i += VIS_THREADS) o[i] = s_acc[i / VISIBLE_OBS_INTS * VISIBLE_OBS_INTS] ? s_acc[i] : 0;
}

}  // namespace mv

namespace mvapi {

namespace {
const GymOption &opt() { return gym_options[OPT_VISIBLE_OBS]; }
size_t frame_ints(const mv_gym *g) { return (size_t)entity_obs_rows(g->gv.scenario, g->A) * VISIBLE_OBS_INTS; }
}  // namespace

// The rows of the frames whose label planes o.seg holds -> o.visible, the same tick's entry: ONE launch on the caller's stream behind whatever wrote the
// planes (the exact pass, or the planes' follower); v: the tick's view (its slot says which frames were drawn).  -> launches made (0: nothing attached), -1
int visible_follow(mv_gym *g, const GymView &v, const OutPtrs &o)
{
    if (!o.visible || !o.seg) return 0;
    hipLaunchKernelGGL(visible_obs_kernel, dim3((unsigned)(g->N * g->A)), dim3(VIS_THREADS), 0, g->stream, (const int32_t *)v.vis_count, (const EnvHeader *)v.hdr,
                       (const uint8_t *)v.soko_cells, (int)v.scenario, g->A, (const uint16_t *)o.seg, (int32_t *)o.visible, g->w, g->h);
    HIP_TRY(hipGetLastError());
    return 1;
}

void visible_obs_free(mv_gym *g) { g->visible = ObsPlanes(); }   // (the buffer is the caller's -- forgotten, not freed)

}  // namespace mvapi

extern "C" {

int mv_set_visible_obs(mv_gym *g, void *device_buf)
{
    const std::string who = opt().setter;
    if (attach_check(g, opt().setter, opt())) return -1;
    if (!device_buf) {
        g->visible = ObsPlanes();
        g->simMustWaitUser = true;
        return 0;
    }
    if (!g->seg.buf || g->seg.format != SEG_INSTANCE_U16)
        return fail(who + ": the rows are counted in an instance-format label plane: attach one first (mv_set_seg_obs with MV_SEG_INSTANCE_U16)");
    if ((uintptr_t)device_buf % sizeof(int32_t)) return fail(who + ": the buffer must be 4-byte aligned");
    g->visible.buf = device_buf;
    g->visible.format = 0;
    g->visible.entries = std::max(1, g->ringCount);
    g->visible.entryBytes = (size_t)g->N * g->A * frame_ints(g) * sizeof(int32_t);
    g->simMustWaitUser = true;   // an ordering point, as the planes' setters
    return 0;
}

int mv_get_visible_obs(const mv_gym *g)
{
    if (getter_check(g, "mv_get_visible_obs")) return -1;
    return g->visible.buf ? g->visible.entries : 0;
}

int mv_get_visible_observation(mv_gym *g, int32_t env, int32_t agent, int32_t *out_host)
{
    const std::string who = "mv_get_visible_observation";
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    if (!g->visible.buf) return fail(who + ": no " + obs_stream(OPT_VISIBLE_OBS).noun + " attached (" + opt().setter + ")");
    if (!out_host) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t ints = frame_ints(g);
    const int32_t *src = (const int32_t *)last_outputs(g).visible + ((size_t)env * g->A + agent) * ints;
    HIP_TRY(hipMemcpyAsync(out_host, src, ints * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_visible_host(int32_t scenario, int32_t num_agents, int32_t room_w, const uint8_t *soko_cells, const uint16_t *words, int32_t w, int32_t h,
                          int32_t *out)
{
    if (!words || !out || w < 0 || h < 0) return fail("mv_debug_visible_host: null pointer or a negative size");
    if (scenario < 0 || scenario >= SCN_COUNT || num_agents < 1 || num_agents > MAX_AGENTS)
        return fail("mv_debug_visible_host: unknown scenario, or num_agents outside [1, 8]");
    if (scenario == SCN_SOKOBAN && !soko_cells) return fail("mv_debug_visible_host: Sokoban needs its 1024 cell bytes");
    visible_obs_host(scenario, num_agents, room_w, soko_cells, words, w, h, out);
    return 0;
}

}  // extern "C"
