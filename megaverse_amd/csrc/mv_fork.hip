// megaverse_amd/csrc/mv_fork.hip -- env forks: the gather-copy kernel and the C ABI in front of it (include/megaverse_hip.h: mv_fork_envs, mv_fork_envs_host,
// mv_debug_fork_plan_host), and the C ABI of env resampling (mv_resample_envs*: any map, through a staged copy in two launches -- the kernels are
// mv_resample.hip's), which shares the fork's checks, its copy of a host map and its place in the streams' order.  The rules of both maps and the table of an
// env's episode state are mv_fork.h's; DESIGN.md 3.8 says what moves and what stays.
#include "mv_api_internal.h"

namespace mv {
namespace fork {

template <class T>
__device__ __forceinline__ void copy_units(const T *__restrict__ src, T *__restrict__ dst, uint32_t n)
{
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) dst[i] = src[i];
}

// One workgroup per (destination env d, range r of RANGES): rows [lo, hi) of the env's row space (Table::first16), env s's -> env d's, the threads side by
// side.  The map's rule is mv_fork.h's: an entry that leaves its env alone exits at once, an invalid one raises ST_FORK and stores nothing.  A workgroup is
// short -- TowerBuilding: two rows per thread -- so what it costs is its chain of dependent memory round trips, and the kernel keeps that at two: src_of[d];
// then, together, the source's own entry, the scan of the map for "is d somebody's source" and the first BATCH rows of env s (read before the entry is known
// to be valid: s is in range, and reading an env is harmless); then the stores.  Which array holds row u is a count over the table's few row offsets
// (uniform values against the lane's row); where that array's slice of an env begins is looked up in LDS, worked out once per workgroup.  Sources are
// never written by the launch (an env that is both is what the rule calls invalid), so the gather is in place.
__global__ __launch_bounds__(THREADS) void fork_kernel(const Table t, const int32_t *__restrict__ src_of, int32_t N, int32_t *status)
{
    __shared__ uint64_t s_from[MAX_ARRAYS], s_to[MAX_ARRAYS];   // array k: address of row 0 of the row SPACE in env s / env d (the slice's base - first16[k] rows)
    const int32_t d = (int32_t)(blockIdx.x / RANGES), r = (int32_t)(blockIdx.x % RANGES);
    const int32_t e = __builtin_amdgcn_readfirstlane(src_of[d]);
    if (leaves_alone(e, d)) return;
    const int32_t from = e >= 0 && e < N ? e : d;   // (an index out of range: nothing is read through it)
    if (threadIdx.x < MAX_ARRAYS) {
        const int k = (int)threadIdx.x;
        const uint64_t row0 = (uint64_t)(uintptr_t)t.a[k].base - (uint64_t)t.first16[k] * 16u;
        s_from[k] = row0 + (uint64_t)from * t.a[k].bytes;
        s_to[k] = row0 + (uint64_t)d * t.a[k].bytes;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)((uint64_t)t.total16 * (uint32_t)r / RANGES), hi = (uint32_t)((uint64_t)t.total16 * (uint32_t)(r + 1) / RANGES);
    typedef uint32_t Row __attribute__((ext_vector_type(4)));   // 16 bytes, read and written through global (not flat) addresses
    typedef const Row __attribute__((address_space(1))) *GlobalSrc;
    typedef Row __attribute__((address_space(1))) *GlobalDst;
    auto array_of = [&](uint32_t u) {   // the array that holds row u: how many of the table's row offsets lie at or below it
        int k = 0;
        for (int j = 1; j < t.count; ++j) k += u >= t.first16[j] ? 1 : 0;
        return k;
    };
    const bool hdrLane = r == 0 && threadIdx.x < 32 && !((IDENTITY_DWORDS >> threadIdx.x) & 1u);
    uint32_t hv = 0;
    if (hdrLane) hv = reinterpret_cast<const uint32_t *>(t.hdr + from)[threadIdx.x];
    // the first BATCH rows of every thread (rows lo + q * THREADS + thread; a q whose rows all lie beyond hi is skipped by the whole workgroup): all of an
    // env's state up to 96 KB
    // (one variable per row, not an array: hipcc merges an array of vectors into one wide value and then waits for each load where it is inserted)
#define MV_FORK_LOAD(q)                                                                               \
    Row v##q;                                                                                         \
    int a##q = 0;                                                                                     \
    if (lo + (uint32_t)(q) * THREADS < hi) {                                                          \
        const uint32_t u = lo + (uint32_t)(q) * THREADS + threadIdx.x;                                \
        a##q = array_of(u);                                                                           \
        if (u < hi) v##q = *(GlobalSrc)(s_from[a##q] + (uint64_t)u * 16u);                            \
    }
#define MV_FORK_STORE(q)                                                                              \
    {                                                                                                 \
        const uint32_t u = lo + (uint32_t)(q) * THREADS + threadIdx.x;                                \
        if (u < hi) *(GlobalDst)(s_to[a##q] + (uint64_t)u * 16u) = v##q;                              \
    }
    static_assert(BATCH == 6, "six rows per thread are written out below");
    MV_FORK_LOAD(0) MV_FORK_LOAD(1) MV_FORK_LOAD(2) MV_FORK_LOAD(3) MV_FORK_LOAD(4) MV_FORK_LOAD(5)
    int32_t s = __builtin_amdgcn_readfirstlane(entry_source(src_of, N, d));   // (the same for every thread: it depends on d alone)
    const int named = __syncthreads_or(named_as_source(src_of, N, d, (int32_t)threadIdx.x, THREADS) ? 1 : 0);
    if (s >= 0 && named) s = INVALID;
    if (s < 0) {
        if (r == 0 && threadIdx.x == 0) atomicOr(status + N + 1, (int)ST_FORK);
        return;
    }
    if (hdrLane) reinterpret_cast<uint32_t *>(t.hdr + d)[threadIdx.x] = hv;
    MV_FORK_STORE(0) MV_FORK_STORE(1) MV_FORK_STORE(2) MV_FORK_STORE(3) MV_FORK_STORE(4) MV_FORK_STORE(5)
#undef MV_FORK_LOAD
#undef MV_FORK_STORE
    for (uint32_t u = lo + BATCH * THREADS + threadIdx.x; u < hi; u += THREADS) {   // (a larger state: the rest row by row)
        const int k = array_of(u);
        *(GlobalDst)(s_to[k] + (uint64_t)u * 16u) = *(GlobalSrc)(s_from[k] + (uint64_t)u * 16u);
    }
    if (r != 0) return;
    for (int k = 0; k < t.count; ++k) {   // arrays that are no 16-byte rows (the episode log's accumulators with an odd agent count): a few dwords or bytes
        const Array a = t.a[k];
        const uint8_t *src = a.base + (size_t)s * a.bytes;
        uint8_t *dst = a.base + (size_t)d * a.bytes;
        if (a.unit == 4) copy_units(reinterpret_cast<const uint32_t *>(src), reinterpret_cast<uint32_t *>(dst), a.bytes / 4);
        else if (a.unit == 1) copy_units(src, dst, a.bytes);
    }
}

void launch_fork(const Table &t, const int32_t *device_src_of, int32_t N, int32_t *status, hipStream_t stream)
{
    hipLaunchKernelGGL(fork_kernel, dim3((unsigned)N * RANGES), dim3(THREADS), 0, stream, t, device_src_of, N, status);
}

}  // namespace fork
}  // namespace mv

namespace mvapi {

// what every form refuses: no gym, a closed one, a null map, a gym that was never reset, a member of a group   (shared with mv_env_store.hip)
int fork_check(mv_gym *g, const void *map, const char *who, const char *what)
{
    if (check(g)) return -1;
    if (!map) return fail(std::string(who) + ": null map");
    if (!g->wasReset) return fail(std::string(who) + ": call mv_reset first (there is no episode to continue)");
    if (g->inGroup) return fail(std::string(who) + ": the gym belongs to an mv_group (its streams are the group's): " + what + " inside groups are not supported");
    return 0;
}

}  // namespace mvapi

namespace {

// The launch.
// A DEVICE map was written by something on the caller's stream, so the copy runs there: behind everything the caller enqueued (the kernel that wrote the
// map), behind every step launch enqueued so far (sim_join: the stream waits for the simulation stream's last event) and behind the episode log's last update,
// which lives on this stream; the next step launch waits for all of it (simMustWaitUser), as after mv_set_actions_device.  Being on that stream it also sits
// behind the observation passes of the last call -- not because it needs them (they read their hand-over slots, never the state) but because the map's
// writer does.  No host synchronisation.
// A HOST map depends on nothing the caller enqueued: where the steps are pipelined and nothing on the caller's stream feeds the simulation (no reset, render or
// setter since the last step; no episode log, whose accumulators are the caller's stream's), map and copy go to the SIMULATION stream itself, in order
// between the step launches -- the passes of the last call are not waited for, and the next call pipelines as if nothing had happened.
// mv_resample_envs takes the same path with its own launches (RESAMPLE: both phases; RESAMPLE_UNSTAGED: the host form saw that no env is staged); its first
// call allocates the staging arena, sized for the episode log whether it is on or not, so that switching it on later changes nothing here.
enum LaunchKind { FORK, RESAMPLE, RESAMPLE_UNSTAGED };
int fork_launch(mv_gym *g, const int32_t *device_map, const int32_t *host_map, LaunchKind kind = FORK)
{
    HIP_TRY(hipSetDevice(g->device));
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    if (kind != FORK && !g->resampleArena) {
        const size_t bytes = fork::staging_bytes(g->forkTable, g->N, (size_t)g->A * sizeof(double), sizeof(int32_t));
        hipError_t e_ = hipMalloc((void **)&g->resampleArena, bytes);
        if (e_ != hipSuccess) { g->resampleArena = nullptr; return fail("mv_resample_envs: hipMalloc of " + std::to_string(bytes) + " bytes of staging: " + hipGetErrorString(e_)); }
        g->resampleBytes = bytes;
    }
    const bool onSim = host_map && g->pipelined && g->simOnOwnStream && g->simDoneValid && !g->simMustWaitUser && g->logCapacity == 0;
    hipStream_t s = onSim ? g->simStream : g->stream;
    if (!onSim && sim_join(g)) return -1;
    if (host_map && g->forkMapPair.stage(host_map, (size_t)g->N * sizeof(int32_t), s, &device_map)) return -1;
    fork::Table t = g->forkTable;
    if (g->logCapacity > 0) {   // the running returns and lengths: a fork's record covers the episode from its source's start (mv_episode_log.h)
        fork::table_add(t, g->logRet, (size_t)g->A * sizeof(double));
        fork::table_add(t, g->logLen, sizeof(int32_t));
    }
    if (kind == FORK) fork::launch_fork(t, device_map, g->N, g->dStatus, s);
    else fork::launch_resample(t, fork::staging_carve(t, g->N, g->resampleArena), device_map, g->N, g->dStatus, kind == RESAMPLE, s);
    HIP_TRY(hipGetLastError());
    if (host_map && g->forkMapPair.mark(s)) return -1;
    if (onSim) HIP_TRY(hipEventRecord(g->simDone, s));   // (what the caller's stream, a reset or a render waits for: now behind the copy)
    if (!host_map) {
        // Only the kernel knows whether it skipped an entry.  The status words travel back behind it, and the next stepping call waits for them
        // (refill_episodes), so that it is that call which reports ST_FORK / ST_RESAMPLE: a host wait there, none here.
        HIP_TRY(hipEventRecord(g->userNow, g->stream));
        if (read_back_status(g, g->userNow)) return -1;
        g->statusReportDue = true;
    }
    return 0;
}

}  // namespace

extern "C" {

int mv_debug_fork_plan_host(const int32_t *src_of, int32_t N, int32_t *resolved, int32_t *invalid)
{
    if (!src_of || N < 0 || !resolved || !invalid) return fail("mv_debug_fork_plan_host: null argument");
    std::vector<int32_t> plan((size_t)N);
    std::vector<uint8_t> named;
    fork::fork_plan(src_of, N, plan.data(), named);   // (the host form's tabulated rule)
    for (int32_t d = 0; d < N; ++d) {
        const int32_t s = fork::fork_resolve(src_of, N, d);   // (the kernel's)
        if (s != plan[(size_t)d]) return fail("mv_debug_fork_plan_host: fork_plan and fork_resolve disagree on entry " + std::to_string(d));
        resolved[d] = s >= 0 ? s : -1;
        invalid[d] = s == fork::INVALID ? 1 : 0;
    }
    return 0;
}

// Test hook: how many episodes of its own sequence every env has taken (EnvHeader::episodes_consumed, one of the fields a fork leaves to the destination),
// after everything enqueued so far.
int mv_debug_episodes_consumed(mv_gym *g, int32_t *out)
{
    if (check(g)) return -1;
    if (!out) return fail("mv_debug_episodes_consumed: null pointer");
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->simStream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    std::vector<EnvHeader> h((size_t)g->N);
    HIP_TRY(hipMemcpy(h.data(), g->gv.hdr, h.size() * sizeof(EnvHeader), hipMemcpyDeviceToHost));
    for (int i = 0; i < g->N; ++i) out[i] = h[(size_t)i].episodes_consumed;
    return 0;
}

int64_t mv_fork_bytes_per_env(const mv_gym *g)
{
    if (!g || g->closed) return -1;
    size_t b = fork::table_bytes_per_env(g->forkTable) - 4 * (size_t)__builtin_popcount(fork::IDENTITY_DWORDS);
    if (g->logCapacity > 0) b += (size_t)g->A * sizeof(double) + sizeof(int32_t);
    return (int64_t)b;
}

int mv_fork_envs(mv_gym *g, const int32_t *device_src_of)
{
    if (fork_check(g, device_src_of, "mv_fork_envs")) return -1;
    return fork_launch(g, device_src_of, nullptr);
}

int mv_fork_envs_host(mv_gym *g, const int32_t *src_of)
{
    if (fork_check(g, src_of, "mv_fork_envs_host")) return -1;
    const int32_t N = g->N;
    bool any = false;
    static thread_local std::vector<int32_t> plan;
    static thread_local std::vector<uint8_t> named;
    plan.resize((size_t)N);
    fork::fork_plan(src_of, N, plan.data(), named);
    for (int32_t d = 0; d < N; ++d) {
        const int32_t s = plan[(size_t)d];
        if (s == fork::INVALID) {
            const int32_t e = src_of[d];
            return fail("mv_fork_envs_host: entry " + std::to_string(d) + " = " + std::to_string(e)
                        + (e < -1 || e >= N ? " is out of range (-1, or 0 .. " + std::to_string(N - 1) + ")"
                                            : " makes a chain: a source may not be a destination in the same call") + "; nothing was forked");
        }
        any = any || s >= 0;
    }
    if (!any) return 0;
    return fork_launch(g, nullptr, src_of);
}

int mv_debug_resample_plan_host(const int32_t *src_of, int32_t N, int32_t *resolved, int32_t *staged, int32_t *invalid)
{
    if (!src_of || N < 0 || !resolved || !staged || !invalid) return fail("mv_debug_resample_plan_host: null argument");
    std::vector<int32_t> plan((size_t)N);
    std::vector<uint8_t> target;
    fork::resample_plan(src_of, N, plan.data(), target);   // (the host form's tabulated rule)
    for (int32_t d = 0; d < N; ++d) {
        int32_t s = 0;
        const int tgt = fork::resample_resolve(src_of, N, d, &s);   // (the kernel's)
        if (s != plan[(size_t)d] || tgt != (int)target[(size_t)d])
            return fail("mv_debug_resample_plan_host: resample_plan and resample_resolve disagree on entry " + std::to_string(d));
        resolved[d] = s >= 0 ? s : -1;
        staged[d] = fork::phase2_copies(tgt) ? 1 : 0;
        invalid[d] = s == fork::INVALID ? 1 : 0;
    }
    return 0;
}

// The two phases over a host byte array, one "env" of bytes_per_env bytes after the other, with a temporary staging array and plan: where phase 1 writes and
// what phase 2 copies is decided by the functions the kernels use (mv_fork.h: resample_resolve -> phase1_target, phase2_copies).  The envs of each phase are
// visited in ascending (0), descending (1) or a fixed pseudo-random (2) order: the phases' hazard argument says the result cannot depend on it.
int mv_debug_resample_apply_host(const int32_t *src_of, int32_t N, int32_t bytes_per_env, uint8_t *state, int32_t order)
{
    if (!src_of || N < 0 || bytes_per_env < 0 || !state) return fail("mv_debug_resample_apply_host: null argument");
    if (order < 0 || order > 2) return fail("mv_debug_resample_apply_host: order is 0 (ascending), 1 (descending) or 2 (pseudo-random)");
    std::vector<int32_t> visit((size_t)N);
    for (int32_t i = 0; i < N; ++i) visit[(size_t)i] = order == 1 ? N - 1 - i : i;
    if (order == 2) {
        uint32_t x = 0x9E3779B9u;
        for (int32_t i = N - 1; i > 0; --i) {   // Fisher-Yates with a fixed LCG
            x = x * 1664525u + 1013904223u;
            std::swap(visit[(size_t)i], visit[(size_t)((x >> 8) % (uint32_t)(i + 1))]);
        }
    }
    const size_t B = (size_t)bytes_per_env;
    std::vector<uint8_t> staging((size_t)N * B), plan((size_t)N, (uint8_t)fork::TO_NOWHERE);
    for (int32_t d : visit) {   // phase 1
        int32_t s = 0;
        const int tgt = fork::resample_resolve(src_of, N, d, &s);
        plan[(size_t)d] = (uint8_t)tgt;
        if (tgt == fork::TO_NOWHERE) continue;
        std::memcpy((tgt == fork::TO_STAGING ? staging.data() : state) + (size_t)d * B, state + (size_t)s * B, B);
    }
    for (int32_t d : visit)     // phase 2
        if (fork::phase2_copies(plan[(size_t)d])) std::memcpy(state + (size_t)d * B, staging.data() + (size_t)d * B, B);
    return 0;
}

int64_t mv_resample_staging_bytes(const mv_gym *g) { return !g || g->closed ? -1 : (int64_t)g->resampleBytes; }

int mv_resample_envs(mv_gym *g, const int32_t *device_src_of)
{
    if (fork_check(g, device_src_of, "mv_resample_envs")) return -1;
    return fork_launch(g, device_src_of, nullptr, RESAMPLE);
}

int mv_resample_envs_host(mv_gym *g, const int32_t *src_of)
{
    if (fork_check(g, src_of, "mv_resample_envs_host")) return -1;
    const int32_t N = g->N;
    bool any = false, staged = false;
    static thread_local std::vector<int32_t> plan;
    static thread_local std::vector<uint8_t> target;
    plan.resize((size_t)N);
    fork::resample_plan(src_of, N, plan.data(), target);
    for (int32_t d = 0; d < N; ++d) {
        if (plan[(size_t)d] == fork::INVALID)
            return fail("mv_resample_envs_host: entry " + std::to_string(d) + " = " + std::to_string(src_of[d]) + " is out of range (-1, or 0 .. "
                        + std::to_string(N - 1) + "); nothing was copied");
        any = any || plan[(size_t)d] >= 0;
        staged = staged || fork::phase2_copies(target[(size_t)d]);
    }
    if (!any) return 0;
    return fork_launch(g, nullptr, src_of, staged ? RESAMPLE : RESAMPLE_UNSTAGED);
}

}  // extern "C"
