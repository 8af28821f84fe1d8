// megaverse_amd/csrc/mv_hex_draw.hip -- HexMemory and HexExplore episodes generated on the device (mv_hex_draw.h): the kernel, its launcher and the host twin
// that the test hooks (mv_draw.hip) hold against mv_gen_hex.cpp (the host generator, which tests/test_host_generators.py holds against the oracle).  The staging-to-ring copy
// of the records is episode_blob_copy_kernel's (mv_collect_draw.hip): the whole record, `seq`'s word last.
#include <cmath>
#include <cstring>
#include <memory>

#include "mv_api_internal.h"
#include "mv_draw.h"
#include "mv_hex_draw.h"
#include "mv_math.h"

namespace mv {

using namespace hdraw;

// HDRAW_WAVES episodes at a time per workgroup, one per wave; nothing in the kernel crosses a wave.
constexpr int HDRAW_WAVES = 4;
struct DrawLds {
    Scratch w[HDRAW_WAVES];
};
static_assert(sizeof(DrawLds) <= 65536, "ALL static LDS of hex_draw_kernel (the kernel declares no other __shared__ object)");
static_assert(sizeof(HexBlob) % 16 == 0 && alignof(HexBlob) == 16 && offsetof(HexBlob, seq) == 0 && sizeof(HexRec) == 32,
              "the record is cleared and copied in 16-byte words, seq's word last");

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ int wave_prefix_sum(int v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int below = __shfl_up(v, (unsigned)d, 64);
        if (lane >= d) v += below;
    }
    return v;
}

__global__ __launch_bounds__(64 * HDRAW_WAVES) void hex_draw_kernel(GenState *states, const int32_t *envs, int count, uint8_t *slots, size_t slot_bytes, int memory,
                                                                     SpawnCircle circle, int num_agents, float base_episode_len, int32_t *flag_word)
{
    __shared__ DrawLds s;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k = (int)blockIdx.x * HDRAW_WAVES + wave;
    if (k >= count) return;
    __builtin_amdgcn_s_setprio(3);   // (as collect_draw_kernel: a few dozen waves of dependent instructions, out of flight as soon as their latencies allow)
    const int lane = lane_id();
    Scratch &w = s.w[wave];
    const int env = envs ? envs[k] : k;
    HexBlob *out = reinterpret_cast<HexBlob *>(slots + (size_t)env * slot_bytes);
    GenState st = states[env];
    clear_record(out, sizeof(HexBlob), lane);
    Mt g{w.mt, 624};
    int flags = 0;
    uint32_t nextSeed = 0;
    // 1. the size (lane 0), then the lay-out: one cell per lane and round
    if (lane == 0) draw_size(g, st, w);
    wave_sync();
    const int size = w.plan.size, cells = w.plan.cells;
    for (int cell = lane; cell < cells; cell += 64) lay_out_cell(w, size, cell);
    wave_sync();
    // 2. and 3. the carve and the draws: lane 0 alone
    if (lane == 0) {
        carve(g, w, cells, w.plan.seed, flags);
        nextSeed = memory ? draw_memory(g, w, circle, num_agents, base_episode_len, out, flags) : draw_explore(g, w, circle, num_agents, base_episode_len, out, flags);
    }
    wave_sync();
    // 4. every box's place behind the partition, its geometry, the objects
    const int walls = w.plan.num_walls;
    int next = 1 + walls;   // the first box that does not collide
    for (int first = 0; first < walls; first += 64) {
        const int mine = first + lane;
        const int len = mine < walls ? (int)w.rec[mine].count + 1 : 0;   // its landmarks and its edging
        const int upto = wave_prefix_sum(len, lane);
        if (mine < walls) wall_boxes(w, mine, next + upto - len, out);
        next += __builtin_amdgcn_readlane(upto, 63);
    }
    if (lane == 0) floor_box(w.plan, out);
    const int objs = min(w.plan.num_objs_drawn, (int)HEX_MAX_OBJS);
    for (int i = lane; i < objs; i += 64) put_object(w, memory != 0, i, out);
    publish_episode(&out->seq, states, env, st, nextSeed, flags, flag_word, lane);
}

// sinf / cosf of the spawn circle with the host generator's expressions (mv_gen_hex.cpp: float(i) * turn, turn = float(2 pi / A)), on the host's math library
static SpawnCircle spawn_circle(int num_agents)
{
    SpawnCircle c;
    const float turn = float(2 * M_PI / num_agents);
    for (int i = 0; i < MAX_AGENTS; ++i) { c.sin_t[i] = sinf(float(i) * turn); c.cos_t[i] = cosf(float(i) * turn); }
    return c;
}

bool launch_hex_draw(const DrawLaunch &a)
{
    if (a.count == 0) return true;
    if (!draw_launch_ok(a, sizeof(HexBlob))) return false;   // (the agent count indexes the sine table)
    hipLaunchKernelGGL(hex_draw_kernel, dim3((a.count + HDRAW_WAVES - 1) / HDRAW_WAVES), dim3(64 * HDRAW_WAVES), 0, a.stream, a.states, a.envs, a.count, a.slots,
                       a.slot_bytes, a.scenario == SCN_HEX_MEMORY ? 1 : 0, spawn_circle(a.num_agents), a.num_agents, a.base_episode_len, a.flag_word);
    return true;
}

// the same episode on the host: the code of mv_hex_draw.h compiled for the CPU, the parallel phases in their serial form
static void hex_draw_host1(int scenario, GenState &st, Scratch &w, int num_agents, float base_episode_len, HexBlob &out)
{
    std::memset(&out, 0, sizeof out);
    const bool memory = scenario == SCN_HEX_MEMORY;
    const SpawnCircle circle = spawn_circle(num_agents);
    Mt g{w.mt, 624};
    int flags = 0;
    draw_size(g, st, w);
    for (int cell = 0; cell < w.plan.cells; ++cell) lay_out_cell(w, w.plan.size, cell);
    carve(g, w, w.plan.cells, w.plan.seed, flags);
    const uint32_t next = memory ? draw_memory(g, w, circle, num_agents, base_episode_len, &out, flags) : draw_explore(g, w, circle, num_agents, base_episode_len, &out, flags);
    for (int k = 0, first = 1 + w.plan.num_walls; k < w.plan.num_walls; first += (int)w.rec[k].count + 1, ++k) wall_boxes(w, k, first, &out);
    floor_box(w.plan, &out);
    for (int i = 0; i < w.plan.num_objs_drawn && i < HEX_MAX_OBJS; ++i) put_object(w, memory, i, &out);
    out.seq = st.next_seq;
    st.seed = next; st.seed_is_env_seed = 0; st.next_seq += 1; st.flags |= flags;
}

void hex_draw_host(int scenario, const ObstacleConfig &, int num_agents, uint32_t env_seed, int n, float base_episode_len, void *record)
{
    auto w = std::make_unique<Scratch>();
    GenState st{env_seed, 1, 1, 0};
    for (int i = 0; i < n; ++i) hex_draw_host1(scenario, st, *w, num_agents, base_episode_len, *static_cast<HexBlob *>(record));
}

}  // namespace mv
