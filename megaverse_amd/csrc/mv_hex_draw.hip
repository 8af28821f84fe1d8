// megaverse_amd/csrc/mv_hex_draw.hip -- HexMemory and HexExplore episodes generated on the device (mv_hex_draw.h): the kernel, its launcher and the test hooks
// that hold the kernel against mv_gen_hex.cpp (the host generator, which tests/test_host_generators.py holds against the oracle).  The staging-to-ring copy
// of the records is episode_blob_copy_kernel's (mv_collect_draw.hip): the whole record, `seq`'s word last.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mv_api_internal.h"
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
    for (int i = lane; i < (int)(sizeof(HexBlob) / 16); i += 64) reinterpret_cast<uint4 *>(out)[i] = uint4{0u, 0u, 0u, 0u};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // (the zeros are in place before any lane writes a record over them)
    wave_sync();
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    wave_sync();
    if (lane == 0) {
        __hip_atomic_store(&out->seq, st.next_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st.seed = nextSeed; st.seed_is_env_seed = 0; st.next_seq += 1; st.flags |= flags;
        states[env] = st;
        if (flags && flag_word) atomicOr(flag_word, flags);   // (a capacity of the episode record was hit: reported once by the next stepping call)
    }
}

// sinf / cosf of the spawn circle with the host generator's expressions (mv_gen_hex.cpp: float(i) * turn, turn = float(2 pi / A)), on the host's math library
static SpawnCircle spawn_circle(int num_agents)
{
    SpawnCircle c;
    const float turn = float(2 * M_PI / num_agents);
    for (int i = 0; i < MAX_AGENTS; ++i) { c.sin_t[i] = sinf(float(i) * turn); c.cos_t[i] = cosf(float(i) * turn); }
    return c;
}

// -> false, nothing launched: arguments the kernel cannot take (a slot smaller than the record, an agent count outside the sine table).  The caller reports it:
// no episode was drawn, and whoever waits for one must not wait for ever.  A launch that fails shows in hipGetLastError, as the other launchers' do.
bool launch_hex_draw(void *states, const int32_t *envs, int count, uint8_t *slots, size_t slot_bytes, int scenario, int num_agents, float base_episode_len,
                     hipStream_t stream, int32_t *flag_word)
{
    if (count == 0) return true;
    if (count < 0 || !states || !slots || slot_bytes < sizeof(HexBlob) || num_agents < 1 || num_agents > MAX_AGENTS) return false;
    hipLaunchKernelGGL(hex_draw_kernel, dim3((count + HDRAW_WAVES - 1) / HDRAW_WAVES), dim3(64 * HDRAW_WAVES), 0, stream, static_cast<GenState *>(states), envs, count,
                       slots, slot_bytes, scenario == SCN_HEX_MEMORY ? 1 : 0, spawn_circle(num_agents), num_agents, base_episode_len, flag_word);
    return true;
}

// the same episode on the host: the code of mv_hex_draw.h compiled for the CPU, the parallel phases in their serial form
static void hex_draw_host(int scenario, GenState &st, Scratch &w, int num_agents, float base_episode_len, HexBlob &out)
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

}  // namespace mv

using namespace mv;
using namespace mvapi;

static bool hex_scenario(const char *name, int &scenario)
{
    ObstacleConfig oc;
    return name && scenario_from_name(lower(name), scenario, oc) && (scenario == SCN_HEX_MEMORY || scenario == SCN_HEX_EXPLORE);
}

extern "C" {

// Host-only test hook (no device needed): the n-th episode of an env seeded with `env_seed` as mv_hex_draw.h's code generates it ON THE HOST -- the same
// record mv_debug_generate_episode(scenario, ...) returns (its `seq` is n here, 0 there).
int mv_debug_hex_draw_host(const char *scenario_name, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes)
{
    int scenario = SCN_TOWER;
    if (!hex_scenario(scenario_name, scenario)) return fail("mv_debug_hex_draw_host: HexMemory and HexExplore");
    if (!out) return (int)sizeof(HexBlob);
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1) return fail("mv_debug_hex_draw_host: bad arguments");
    if ((size_t)out_bytes < sizeof(HexBlob)) return fail("mv_debug_hex_draw_host: buffer too small");
    auto w = std::make_unique<hdraw::Scratch>();
    auto blob = std::make_unique<HexBlob>();
    cdraw::GenState st{(uint32_t)env_seed, 1, 1, 0};
    for (int i = 0; i < n; ++i) hex_draw_host(scenario, st, *w, num_agents, base_episode_len, *blob);
    std::memcpy(out, blob.get(), sizeof(HexBlob));
    return (int)sizeof(HexBlob);
}

// Test hook: `count` envs seeded with env_seeds[i], each drawing its first n episodes ON THE DEVICE (n launches of hex_draw_kernel); out receives the envs'
// n-th episodes, count x sizeof(HexBlob) bytes; *ms_per_launch (may be null) the mean time of a launch.
int mv_debug_hex_draw_device(int32_t device, const char *scenario_name, int32_t num_agents, const int32_t *env_seeds, int32_t count, int32_t n,
                             float base_episode_len, void *out, int64_t out_bytes, float *ms_per_launch)
{
    int scenario = SCN_TOWER;
    if (!hex_scenario(scenario_name, scenario)) return fail("mv_debug_hex_draw_device: HexMemory and HexExplore");
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1 || count < 1 || !env_seeds || !out) return fail("mv_debug_hex_draw_device: bad arguments");
    if ((size_t)out_bytes < (size_t)count * sizeof(HexBlob)) return fail("mv_debug_hex_draw_device: buffer too small");
    HIP_TRY(hipSetDevice(device));
    std::vector<cdraw::GenState> st((size_t)count);
    for (int i = 0; i < count; ++i) st[(size_t)i] = cdraw::GenState{(uint32_t)env_seeds[i], 1, 1, 0};
    cdraw::GenState *dSt = nullptr;
    uint8_t *dSlots = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const size_t bytes = (size_t)count * sizeof(HexBlob);
    bool ok = hipMalloc((void **)&dSt, (size_t)count * sizeof(cdraw::GenState)) == hipSuccess && hipMalloc((void **)&dSlots, bytes) == hipSuccess &&
              hipMemset(dSlots, 0, bytes) == hipSuccess &&
              hipMemcpy(dSt, st.data(), (size_t)count * sizeof(cdraw::GenState), hipMemcpyHostToDevice) == hipSuccess &&
              hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (ok) {
        ok = hipEventRecord(e0, nullptr) == hipSuccess;
        for (int i = 0; i < n && ok; ++i) ok = launch_hex_draw(dSt, nullptr, count, dSlots, sizeof(HexBlob), scenario, num_agents, base_episode_len, nullptr, nullptr);
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipMemcpy(out, dSlots, bytes, hipMemcpyDeviceToHost) == hipSuccess;
        float ms = 0.0f;
        if (ok && ms_per_launch && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *ms_per_launch = ms / float(n);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (dSt) (void)hipFree(dSt);
    if (dSlots) (void)hipFree(dSlots);
    return ok ? 0 : fail("mv_debug_hex_draw_device: a HIP call failed");
}

}  // extern "C"
