// megaverse_amd/csrc/mv_obstacles_draw.hip -- Obstacles-family and Empty episodes generated on the device (mv_obstacles_draw.h): the kernel, its launcher, the
// staging-to-ring copy of EpisodeBlob records, and the test hooks that hold the kernel against mv_gen_obstacles.cpp (the host generator, which
// tests/test_host_generators.py holds against the oracle).
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mv_api_internal.h"
#include "mv_math.h"
#include "mv_obstacles_draw.h"

namespace mv {

using namespace odraw;

// ---- the grid's bit planes in device memory ---------------------------------------------------------------------------------------------------
// The lanes of a wave change words of the planes with atomics (several lanes' rows can share a word) and read them back with agent-scope loads, a fence and a
// wave barrier between the two: every read is served by L2, behind every change made before the barrier.
__device__ __forceinline__ uint32_t grid_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void grid_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}
// how many of the cells id, id + 1, ... are set, counted up to `limit` (a run along x is a run of bits: word loads, not cell loads)
__device__ __forceinline__ int ones_from(const uint32_t *plane, int id, int limit)
{
    int n = 0;
    while (n < limit) {
        const int i = id + n, avail = min(32 - (i & 31), limit - n);
        const uint32_t gaps = ~(grid_load(&plane[i >> 5]) >> (i & 31));   // (the shifted-in zeros read as gaps: a run ends at the word's end at the latest)
        const int run = gaps ? __ffs((int)gaps) - 1 : 32;
        if (run < avail) return n + run;
        n += avail;
    }
    return n;
}
__device__ __forceinline__ uint32_t run_mask(int bit, int n) { return (n >= 32 ? ~0u : ((1u << n) - 1u)) << bit; }
__device__ __forceinline__ void run_set(uint32_t *plane, int id, int len)
{
    for (; len > 0;) {
        const int bit = id & 31, n = min(32 - bit, len);
        atomicOr(&plane[id >> 5], run_mask(bit, n));
        id += n; len -= n;
    }
}
__device__ __forceinline__ void run_clear(uint32_t *plane, int id, int len)
{
    for (; len > 0;) {
        const int bit = id & 31, n = min(32 - bit, len);
        atomicAnd(&plane[id >> 5], ~run_mask(bit, n));
        id += n; len -= n;
    }
}
__device__ __forceinline__ int trailing_ones64(unsigned long long m) { return m == ~0ull ? 64 : __ffsll((long long)~m) - 1; }

// draw_slabs_serial (mv_obstacles_draw.h) by all 64 lanes of the episode's wave -- the same paint and the same greedy walk, box for box.
//   paint: the boxes one after the other (later boxes overwrite), a box's rows (y, z) spread over the lanes, a row one run of bits set in its plane and
//          cleared in the other;
//   scan:  64 words = 2048 cells per round, a ballot finds the first word with a cell left, its lowest bit is the seed;
//   grow:  along x the run of bits from the seed (every lane walks the same words); along z and then y one ballot per 64 rows / layers -- lane k tests the k-th
//          row / layer beyond the box, the run of ones from lane 0 is the growth;
//   mark:  the box's rows cleared by the lanes together.
__device__ __forceinline__ void draw_slabs_wave(const Scratch &w, uint32_t *grid, EpisodeBlob *out, int &flags)
{
    const int lane = lane_id();
    const Level lv = w.level;
    if (!grid_fits(lv)) {   // (never, by the bound GRID_CELLS is derived from: the region is not touched)
        flags |= FLAG_SLABS;
        if (lane == 0) out->num_boxes = 0;
        return;
    }
    const int nx = lv.nx, ny = lv.ny, nz = lv.nz, total = nx * ny * nz, words = (total + 31) / 32;
    uint32_t *planes[2] = {grid, grid + PLANE_WORDS};
    for (int i = lane; i < words; i += 64) {
        __hip_atomic_store(&planes[0][i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&planes[1][i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    grid_sync();
    for (int j = 0; j < lv.members; ++j) {
        const Plat &p = w.chain[j];
        const int numBoxes = p.num_floor + p.num_wall;
        for (int i = 0; i < numBoxes; ++i) {
            const int plane = i < p.num_floor ? 0 : 1;
            const Aabb b = placed(p.root, plane == 0 ? p.floor[i] : p.wall[i - p.num_floor]);
            const int bx = b.hi.x - b.lo.x, bz = b.hi.z - b.lo.z, rows = (b.hi.y - b.lo.y) * bz;
            for (int r = lane; r < rows; r += 64) {
                const int y = b.lo.y + r / bz - lv.lo.y, z = b.lo.z + r % bz - lv.lo.z, id = (y * nz + z) * nx + (b.lo.x - lv.lo.x);
                if (id < 0 || bx <= 0 || id + bx > total) continue;   // (a box lies inside the hull it was counted into)
                run_set(planes[plane], id, bx);
                run_clear(planes[1 - plane], id, bx);
            }
            grid_sync();
        }
    }
    int numBoxes = 0, found = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int type, slot;
        uint32_t *pl = planes[merge_pass(pass, lv.draw_walls, type, slot)];
        for (int base = 0; base < words; base += 64) {
            const int word = base + lane;
            uint32_t mine = word < words ? grid_load(&pl[word]) : 0u;
            unsigned long long m = __ballot(mine != 0u);
            while (m && found < GRID_CELLS) {
                ++found;
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)mine, src);
                const int seed = (base + src) * 32 + __ffs((int)bits) - 1;
                const int x = seed % nx, t = seed / nx, z = t % nz, y = t / nz;
                const int wx = ones_from(pl, seed, nx - x);
                int zEnd = z + 1, yEnd = y + 1;
                for (;;) {
                    const int zz = zEnd + lane;
                    const bool ok = zz < nz && ones_from(pl, (y * nz + zz) * nx + x, wx) == wx;
                    const int grown = trailing_ones64(__ballot(ok));
                    zEnd += grown;
                    if (grown < 64) break;
                }
                for (;;) {
                    const int yy = yEnd + lane;
                    bool ok = yy < ny;
                    for (int zz = z; ok && zz < zEnd; ++zz) ok = ones_from(pl, (yy * nz + zz) * nx + x, wx) == wx;
                    const int grown = trailing_ones64(__ballot(ok));
                    yEnd += grown;
                    if (grown < 64) break;
                }
                grid_sync();   // (every lane's reads of the bits before they change)
                const int wz = zEnd - z, rows = wz * (yEnd - y);
                for (int r = lane; r < rows; r += 64) run_clear(pl, ((y + r / wz) * nz + z + r % wz) * nx + x, wx);
                grid_sync();
                if (numBoxes >= MAX_BOXES) flags |= FLAG_SLABS;
                else {
                    if (lane == 0) {
                        LayoutBox b;
                        b.min[0] = x + lv.lo.x; b.min[1] = y + lv.lo.y; b.min[2] = z + lv.lo.z;
                        b.max[0] = x + wx + lv.lo.x; b.max[1] = yEnd + lv.lo.y; b.max[2] = zEnd + lv.lo.z;
                        b.type = type; b.slot = slot;
                        out->boxes[numBoxes] = b;
                    }
                    ++numBoxes;
                }
                mine = word < words ? grid_load(&pl[word]) : 0u;
                m = __ballot(mine != 0u);
            }
        }
    }
    if (found >= GRID_CELLS) flags |= FLAG_SLABS;   // (the walk was cut short -- it cannot be while covered cells are cleared: said, not hidden)
    if (lane == 0) out->num_boxes = numBoxes;
}

// ODRAW_WAVES episodes at a time per workgroup, one per wave (nothing in the kernel crosses a wave); a wave draws episodes r, r + waves, r + 2 waves, ... of
// the launch's list in the grid region r, `waves` = min(count, regions) -- so a launch never needs more regions than the feeder holds.
constexpr int ODRAW_WAVES = 4;
struct DrawLds {
    Scratch w[ODRAW_WAVES];
};
static_assert(sizeof(DrawLds) <= 65536, "ALL static LDS of obstacles_draw_kernel (the kernel declares no other __shared__ object)");

__global__ __launch_bounds__(64 * ODRAW_WAVES) void obstacles_draw_kernel(GenState *states, const int32_t *envs, int count, uint8_t *slots, size_t slot_bytes, int empty,
                                                                           ObstacleConfig cfg, int num_agents, float base_episode_len, uint32_t *grids, int waves,
                                                                           int32_t *flag_word)
{
    __shared__ DrawLds s;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int region = (int)blockIdx.x * ODRAW_WAVES + wave;
    if (region >= waves) return;
    __builtin_amdgcn_s_setprio(3);   // (as collect_draw_kernel: a few dozen waves of dependent instructions, out of flight as soon as their latencies allow)
    const int lane = lane_id();
    Scratch &w = s.w[wave];
    uint32_t *grid = grids ? grids + (size_t)region * GRID_WORDS : nullptr;
    for (int k = region; k < count; k += waves) {
        const int env = envs ? envs[k] : k;
        EpisodeBlob *out = reinterpret_cast<EpisodeBlob *>(slots + (size_t)env * slot_bytes);
        GenState st = states[env];
        for (int i = lane; i < (int)(sizeof(EpisodeBlob) / 16); i += 64) reinterpret_cast<uint4 *>(out)[i] = uint4{0u, 0u, 0u, 0u};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // (the zeros are in place before lane 0 writes fields over them)
        wave_sync();
        Mt g{w.mt, 624};
        int flags = 0;
        uint32_t nextSeed = 0;
        if (empty || !grid) {
            if (lane == 0) nextSeed = draw_empty(g, st, w.mt, num_agents, base_episode_len, out);
        } else {
            if (lane == 0) draw_chain(g, st, cfg, w, out);
            wave_sync();
            draw_slabs_wave(w, grid, out, flags);
            wave_sync();
            if (lane == 0) nextSeed = draw_tail(g, w, num_agents, base_episode_len, out, flags);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        wave_sync();
        if (lane == 0) {
            __hip_atomic_store(&out->seq, st.next_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st.seed = nextSeed; st.seed_is_env_seed = 0; st.next_seq += 1; st.flags |= flags;
            states[env] = st;
            if (flags && flag_word) atomicOr(flag_word, flags);   // (a capacity of the episode record was hit: reported once by the next stepping call)
        }
        wave_sync();   // (lane 0 is done with the wave's scratch before the next episode's chain goes there)
    }
}

int obstacles_draw_regions(int scenario, int num_envs) { return scenario == SCN_EMPTY ? 0 : std::min(num_envs, (int)DRAW_REGIONS); }
size_t obstacles_draw_region_bytes() { return (size_t)GRID_WORDS * sizeof(uint32_t); }

void launch_obstacles_draw(void *states, const int32_t *envs, int count, uint8_t *slots, size_t slot_bytes, int scenario, const ObstacleConfig &cfg, int num_agents,
                           float base_episode_len, uint32_t *grids, int regions, hipStream_t stream, int32_t *flag_word)
{
    if (count <= 0) return;
    const int empty = scenario == SCN_EMPTY ? 1 : 0;
    const int waves = empty ? count : std::min(count, regions);
    if (waves <= 0) return;
    hipLaunchKernelGGL(obstacles_draw_kernel, dim3((waves + ODRAW_WAVES - 1) / ODRAW_WAVES), dim3(64 * ODRAW_WAVES), 0, stream, static_cast<GenState *>(states), envs, count,
                       slots, slot_bytes, empty, cfg, num_agents, base_episode_len, empty ? nullptr : grids, waves, flag_word);
}

// the same episode on the host: the code of mv_obstacles_draw.h compiled for the CPU, the merge in its serial form
struct HostDraw {
    Scratch w;
    std::vector<uint32_t> grid = std::vector<uint32_t>((size_t)GRID_WORDS, 0u);
};
static void obstacles_draw_host(int scenario, const ObstacleConfig &cfg, GenState &st, HostDraw &h, int num_agents, float base_episode_len, EpisodeBlob &out,
                                Stats *stats)
{
    std::memset(&out, 0, sizeof out);
    Mt g{h.w.mt, 624};
    int flags = 0;
    uint32_t next;
    if (scenario == SCN_EMPTY) {
        next = draw_empty(g, st, h.w.mt, num_agents, base_episode_len, &out);
        if (stats) *stats = Stats{1, 0, 0};
    } else {
        draw_chain(g, st, cfg, h.w, &out, stats);
        draw_slabs_serial(h.w, h.grid.data(), &out, flags);
        next = draw_tail(g, h.w, num_agents, base_episode_len, &out, flags);
    }
    out.seq = st.next_seq;
    st.seed = next; st.seed_is_env_seed = 0; st.next_seq += 1; st.flags |= flags;
}

}  // namespace mv

using namespace mv;
using namespace mvapi;

static bool obstacles_scenario(const char *name, int &scenario, ObstacleConfig &oc)
{
    return name && scenario_from_name(lower(name), scenario, oc) && (scenario == SCN_OBSTACLES || scenario == SCN_EMPTY) && odraw::config_fits(oc);
}

extern "C" {

// Host-only test hook (no device needed): the n-th episode of an env seeded with `env_seed` as mv_obstacles_draw.h's code generates it ON THE HOST -- the
// same record mv_debug_generate_episode(scenario, ...) returns (its `seq` is n here, 0 there).
int mv_debug_obstacles_draw_host(const char *scenario_name, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    if (!obstacles_scenario(scenario_name, scenario, oc)) return fail("mv_debug_obstacles_draw_host: the Obstacles family and Empty");
    if (!out) return (int)sizeof(EpisodeBlob);
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1) return fail("mv_debug_obstacles_draw_host: bad arguments");
    if ((size_t)out_bytes < sizeof(EpisodeBlob)) return fail("mv_debug_obstacles_draw_host: buffer too small");
    auto h = std::make_unique<HostDraw>();
    auto blob = std::make_unique<EpisodeBlob>();
    cdraw::GenState st{(uint32_t)env_seed, 1, 1, 0};
    for (int i = 0; i < n; ++i) obstacles_draw_host(scenario, oc, st, *h, num_agents, base_episode_len, *blob, nullptr);
    std::memcpy(out, blob.get(), sizeof(EpisodeBlob));
    return (int)sizeof(EpisodeBlob);
}

// Host-only test hook: how the n-th episode came about, on both sides.  out[0 .. 3]: the host generator's chain attempts, left turns, right turns and the
// capacity flags (GEN_*) it raised for that episode; out[4 .. 7]: the same four of mv_obstacles_draw.h's code on the host.
int mv_debug_obstacles_draw_stats_host(const char *scenario_name, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, int32_t *out)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    if (!obstacles_scenario(scenario_name, scenario, oc) || !out) return fail("mv_debug_obstacles_draw_stats_host: the Obstacles family and Empty");
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1) return fail("mv_debug_obstacles_draw_stats_host: bad arguments");
    auto blob = std::make_unique<EpisodeBlob>();
    std::mt19937 rng;
    rng.seed((unsigned long)env_seed);
    (void)generator_overflow_take();
    for (int i = 0; i < n; ++i) {
        (void)generator_overflow_take();
        if (scenario == SCN_EMPTY) generate_empty_episode(rng, num_agents, base_episode_len, *blob);
        else generate_obstacles_episode(rng, oc, num_agents, base_episode_len, *blob);
    }
    const ObstacleStats hs = scenario == SCN_EMPTY ? ObstacleStats{1, 0, 0} : obstacles_last_stats();
    out[0] = hs.attempts; out[1] = hs.left_turns; out[2] = hs.right_turns; out[3] = generator_overflow_take();
    auto h = std::make_unique<HostDraw>();
    cdraw::GenState st{(uint32_t)env_seed, 1, 1, 0};
    odraw::Stats ds{0, 0, 0};
    for (int i = 0; i < n; ++i) {
        st.flags = 0;
        obstacles_draw_host(scenario, oc, st, *h, num_agents, base_episode_len, *blob, &ds);
    }
    out[4] = ds.attempts; out[5] = ds.left_turns; out[6] = ds.right_turns; out[7] = st.flags;
    return 0;
}

// Test hook: `count` envs seeded with env_seeds[i], each drawing its first n episodes ON THE DEVICE (n launches of obstacles_draw_kernel); out receives the
// envs' n-th episodes, count x sizeof(EpisodeBlob) bytes; *ms_per_launch (may be null) the mean time of a launch.
int mv_debug_obstacles_draw_device(int32_t device, const char *scenario_name, int32_t num_agents, const int32_t *env_seeds, int32_t count, int32_t n,
                                   float base_episode_len, void *out, int64_t out_bytes, float *ms_per_launch)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    if (!obstacles_scenario(scenario_name, scenario, oc)) return fail("mv_debug_obstacles_draw_device: the Obstacles family and Empty");
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1 || count < 1 || !env_seeds || !out) return fail("mv_debug_obstacles_draw_device: bad arguments");
    if ((size_t)out_bytes < (size_t)count * sizeof(EpisodeBlob)) return fail("mv_debug_obstacles_draw_device: buffer too small");
    HIP_TRY(hipSetDevice(device));
    std::vector<cdraw::GenState> st((size_t)count);
    for (int i = 0; i < count; ++i) st[(size_t)i] = cdraw::GenState{(uint32_t)env_seeds[i], 1, 1, 0};
    cdraw::GenState *dSt = nullptr;
    uint8_t *dSlots = nullptr;
    uint32_t *dGrids = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const size_t bytes = (size_t)count * sizeof(EpisodeBlob);
    const int regions = obstacles_draw_regions(scenario, count);
    bool ok = hipMalloc((void **)&dSt, (size_t)count * sizeof(cdraw::GenState)) == hipSuccess && hipMalloc((void **)&dSlots, bytes) == hipSuccess &&
              (regions == 0 || hipMalloc((void **)&dGrids, (size_t)regions * obstacles_draw_region_bytes()) == hipSuccess) &&
              hipMemset(dSlots, 0, bytes) == hipSuccess &&
              hipMemcpy(dSt, st.data(), (size_t)count * sizeof(cdraw::GenState), hipMemcpyHostToDevice) == hipSuccess &&
              hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (ok) {
        ok = hipEventRecord(e0, nullptr) == hipSuccess;
        for (int i = 0; i < n && ok; ++i)
            launch_obstacles_draw(dSt, nullptr, count, dSlots, sizeof(EpisodeBlob), scenario, oc, num_agents, base_episode_len, dGrids, regions, nullptr, nullptr);
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipMemcpy(out, dSlots, bytes, hipMemcpyDeviceToHost) == hipSuccess;
        float ms = 0.0f;
        if (ok && ms_per_launch && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *ms_per_launch = ms / float(n);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (dSt) (void)hipFree(dSt);
    if (dSlots) (void)hipFree(dSlots);
    if (dGrids) (void)hipFree(dGrids);
    return ok ? 0 : fail("mv_debug_obstacles_draw_device: a HIP call failed");
}

}  // extern "C"
