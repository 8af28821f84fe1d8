// megaverse_amd/csrc/mv_env_store.hip -- env stores: the two kernels that move an env's episode state into a record of a caller-owned store and back, the C
// ABI in front of them (include/megaverse_hip.h: mv_env_record_bytes, mv_env_record_layout, mv_save_envs*, mv_load_envs*) and the host-only hooks
// (mv_debug_env_store_plan_host, mv_debug_env_record_pack_host, mv_debug_env_record_unpack_host).  The record's layout, its header and the rules of the
// two maps are mv_env_store.h's; what moves and what stays is the fork's (mv_fork.h); DESIGN.md 3.11 has the rest.
#include "mv_api_internal.h"
#include "mv_env_store.h"

namespace mv {
namespace store {

using fork::Array;
using fork::BATCH;
using fork::MAX_ARRAYS;
using fork::RANGES;
using fork::Table;
using fork::THREADS;

typedef uint32_t Row __attribute__((ext_vector_type(4)));   // 16 bytes, read and written through global (not flat) addresses
typedef const Row __attribute__((address_space(1))) *GlobalSrc;
typedef Row __attribute__((address_space(1))) *GlobalDst;
typedef const uint32_t __attribute__((address_space(1))) *GlobalSrc32;
typedef uint32_t __attribute__((address_space(1))) *GlobalDst32;

// Rows [lo, hi) of an env's row space (Table::first16) from one side to the other, the threads side by side: fork_kernel's copy.  s_from[k] / s_to[k]: the
// address of row 0 of the row space on either side, for array k -- in an env the slice's base less first16[k] rows, in a record the record's base plus the
// array's offset less first16[k] rows: row u of a record sits at a fixed offset, whichever env it came from.  The first BATCH rows of every thread are in
// flight before `verdict` is asked -- the workgroup's one decision, the same for every thread -- and nothing is stored unless it says yes.
template <class Verdict>
__device__ __forceinline__ bool copy_rows(const Table &t, const uint64_t *s_from, const uint64_t *s_to, uint32_t lo, uint32_t hi, Verdict verdict)
{
    auto array_of = [&](uint32_t u) {   // the array that holds row u: how many of the table's row offsets lie at or below it
        int k = 0;
        for (int j = 1; j < t.count; ++j) k += u >= t.first16[j] ? 1 : 0;
        return k;
    };
    // (one variable per row, not an array: hipcc merges an array of vectors into one wide value and then waits for each load where it is inserted)
#define MV_STORE_LOAD(q)                                                                              \
    Row v##q;                                                                                         \
    int a##q = 0;                                                                                     \
    if (lo + (uint32_t)(q) * THREADS < hi) {                                                          \
        const uint32_t u = lo + (uint32_t)(q) * THREADS + threadIdx.x;                                \
        a##q = array_of(u);                                                                           \
        if (u < hi) v##q = *(GlobalSrc)(s_from[a##q] + (uint64_t)u * 16u);                            \
    }
#define MV_STORE_STORE(q)                                                                             \
    {                                                                                                 \
        const uint32_t u = lo + (uint32_t)(q) * THREADS + threadIdx.x;                                \
        if (u < hi) *(GlobalDst)(s_to[a##q] + (uint64_t)u * 16u) = v##q;                              \
    }
    static_assert(BATCH == 6, "six rows per thread are written out below");
    MV_STORE_LOAD(0) MV_STORE_LOAD(1) MV_STORE_LOAD(2) MV_STORE_LOAD(3) MV_STORE_LOAD(4) MV_STORE_LOAD(5)
    if (!verdict()) return false;
    MV_STORE_STORE(0) MV_STORE_STORE(1) MV_STORE_STORE(2) MV_STORE_STORE(3) MV_STORE_STORE(4) MV_STORE_STORE(5)
#undef MV_STORE_LOAD
#undef MV_STORE_STORE
    for (uint32_t u = lo + BATCH * THREADS + threadIdx.x; u < hi; u += THREADS) {   // (a larger state: the rest row by row)
        const int k = array_of(u);
        *(GlobalDst)(s_to[k] + (uint64_t)u * 16u) = *(GlobalSrc)(s_from[k] + (uint64_t)u * 16u);
    }
    return true;
}

// the table's arrays that are no 16-byte rows, by the workgroup of range 0: dwords or bytes; towards a record the slice is filled up to its 16-byte boundary
__device__ __forceinline__ void copy_odd_arrays(const Table &t, const Layout &L, int32_t env, uint8_t *record, bool to_record)
{
    for (int k = 0; k < t.count; ++k) {
        const Array a = t.a[k];
        if (a.unit == 16) continue;
        uint8_t *live = a.base + (size_t)env * a.bytes, *rec = record + L.off[k];
        if (!to_record) {
            if (a.unit == 4) for (uint32_t i = threadIdx.x; i < a.bytes / 4; i += THREADS) reinterpret_cast<uint32_t *>(live)[i] = reinterpret_cast<const uint32_t *>(rec)[i];
            else for (uint32_t i = threadIdx.x; i < a.bytes; i += THREADS) live[i] = rec[i];
        } else if (a.unit == 4) {
            for (uint32_t i = threadIdx.x; i < up16(a.bytes) / 4; i += THREADS) reinterpret_cast<uint32_t *>(rec)[i] = i < a.bytes / 4 ? reinterpret_cast<const uint32_t *>(live)[i] : 0u;
        } else {
            for (uint32_t i = threadIdx.x; i < up16(a.bytes); i += THREADS) rec[i] = i < a.bytes ? live[i] : (uint8_t)0;
        }
    }
}

// One workgroup per (env e, range r of RANGES): rows [lo, hi) of env e's row space -> record slot_of[e] of the store.  The map's rule is mv_env_store.h's:
// -1 exits at once; an index out of range, or a slot that another env names too, raises ST_ENV_STORE and stores nothing -- the scan of the map for "who
// else names my slot" is shared out over the threads, and the env's first BATCH rows per thread are read while it runs (reading an env is harmless).  The
// workgroup of range 0 also stores the record header, the whole EnvHeader and the accumulators of the episode log (zero where the log is off), so a record
// is written whole by the workgroups of its env, or not at all.  Nothing in the gym is written but the status bit.
__global__ __launch_bounds__(THREADS) void save_kernel(const Table t, const Layout L, uint64_t word, const double *__restrict__ log_ret,
                                                       const int32_t *__restrict__ log_len, const int32_t *__restrict__ slot_of, int32_t N, uint8_t *store,
                                                       int32_t slots, int32_t *status)
{
    __shared__ uint64_t s_from[MAX_ARRAYS], s_to[MAX_ARRAYS];
    const int32_t e = (int32_t)(blockIdx.x / RANGES), r = (int32_t)(blockIdx.x % RANGES);
    const int32_t m = __builtin_amdgcn_readfirstlane(slot_of[e]);
    if (m == -1) return;
    const bool inRange = slot_in_range(m, slots);
    uint8_t *rec = store + (uint64_t)(inRange ? m : 0) * L.bytes;   // (an index out of range: nothing is written through it)
    if (threadIdx.x < MAX_ARRAYS) {
        const int k = (int)threadIdx.x;
        s_from[k] = (uint64_t)(uintptr_t)t.a[k].base - (uint64_t)t.first16[k] * 16u + (uint64_t)e * t.a[k].bytes;
        s_to[k] = (uint64_t)(uintptr_t)rec + L.off[k] - (uint64_t)t.first16[k] * 16u;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)((uint64_t)t.total16 * (uint32_t)r / RANGES), hi = (uint32_t)((uint64_t)t.total16 * (uint32_t)(r + 1) / RANGES);
    const bool hdrLane = r == 0 && threadIdx.x < 32;
    uint32_t hv = 0;
    if (hdrLane) hv = reinterpret_cast<const uint32_t *>(t.hdr + e)[threadIdx.x];
    const bool written = copy_rows(t, s_from, s_to, lo, hi, [&]() {
        const int again = __syncthreads_or(inRange && slot_named_again(slot_of, N, e, m, (int32_t)threadIdx.x, THREADS) ? 1 : 0);
        return inRange && !again;
    });
    if (!written) {
        if (r == 0 && threadIdx.x == 0) atomicOr(status + N + 1, (int)ST_ENV_STORE);
        return;
    }
    if (r != 0) return;
    const bool logOn = log_ret != nullptr;
    if (hdrLane) ((GlobalDst32)(uintptr_t)(rec + L.env_hdr))[threadIdx.x] = hv;
    if (threadIdx.x < HEADER_DWORDS) ((GlobalDst32)(uintptr_t)rec)[threadIdx.x] = header_dword((int)threadIdx.x, word, L.bytes, logOn ? (uint32_t)FLAG_LOG : 0u);
    // the accumulators and what lies between and behind them up to the record's end
    for (uint32_t o = L.ret + 4u * threadIdx.x; o < L.bytes; o += 4u * THREADS) {
        const int j = o < L.ret + 8u * (uint32_t)L.A ? (int)((o - L.ret) / 4u) : o == L.len ? 2 * L.A : -1;
        uint32_t live = 0;
        if (logOn && j >= 0) live = j < 2 * L.A ? reinterpret_cast<const uint32_t *>(log_ret + (size_t)e * L.A)[j] : (uint32_t)log_len[e];
        *(GlobalDst32)(uintptr_t)(rec + o) = j >= 0 ? saved_log_dword(logOn, live) : 0u;
    }
    copy_odd_arrays(t, L, e, rec, true);
}

// One workgroup per (env d, range r of RANGES): record slot_of[d] of the store -> rows [lo, hi) of env d's row space: fork_kernel with a record for a
// source.  -1 exits at once; an index out of range raises ST_ENV_STORE before anything is read through it.  Then every thread reads one of the record
// header's checked dwords (thread & 7) and, while that is under way, its first BATCH rows of the record (the slot is in range: reading it is harmless); the
// verdict is the AND over the workgroup of "my dword is what this gym's records carry" (mv_env_store.h: header_dword_matches) -- every workgroup of an env
// reads the same seven words and so reaches the same verdict.  A record that fails raises ST_ENV_STORE and changes no byte of its env: what keeps foreign
// bytes out of arrays that the step kernels index by stored counts.  The workgroup of range 0 also stores the EnvHeader without the identity's dwords and,
// where the gym's log is on, the accumulators -- the record's if it was saved with the log on, else zero.
__global__ __launch_bounds__(THREADS) void load_kernel(const Table t, const Layout L, uint64_t word, double *log_ret, int32_t *log_len,
                                                       const int32_t *__restrict__ slot_of, int32_t N, const uint8_t *__restrict__ store, int32_t slots,
                                                       int32_t *status)
{
    __shared__ uint64_t s_from[MAX_ARRAYS], s_to[MAX_ARRAYS];
    const int32_t d = (int32_t)(blockIdx.x / RANGES), r = (int32_t)(blockIdx.x % RANGES);
    const int32_t m = __builtin_amdgcn_readfirstlane(slot_of[d]);
    if (m == -1) return;
    if (!slot_in_range(m, slots)) {
        if (r == 0 && threadIdx.x == 0) atomicOr(status + N + 1, (int)ST_ENV_STORE);
        return;
    }
    const uint8_t *rec = store + (uint64_t)m * L.bytes;
    const int hd = (int)(threadIdx.x & 7u);
    const uint32_t have = ((GlobalSrc32)(uintptr_t)rec)[hd];
    if (threadIdx.x < MAX_ARRAYS) {
        const int k = (int)threadIdx.x;
        s_from[k] = (uint64_t)(uintptr_t)rec + L.off[k] - (uint64_t)t.first16[k] * 16u;
        s_to[k] = (uint64_t)(uintptr_t)t.a[k].base - (uint64_t)t.first16[k] * 16u + (uint64_t)d * t.a[k].bytes;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)((uint64_t)t.total16 * (uint32_t)r / RANGES), hi = (uint32_t)((uint64_t)t.total16 * (uint32_t)(r + 1) / RANGES);
    const bool hdrLane = r == 0 && threadIdx.x < 32 && loads_header_dword((int)threadIdx.x);
    uint32_t hv = 0;
    if (hdrLane) hv = ((GlobalSrc32)(uintptr_t)(rec + L.env_hdr))[threadIdx.x];
    const bool loaded = copy_rows(t, s_from, s_to, lo, hi, [&]() {
        return __syncthreads_and(hd >= HD_CHECKED || header_dword_matches(hd, have, word, L.bytes) ? 1 : 0) != 0;
    });
    if (!loaded) {
        if (r == 0 && threadIdx.x == 0) atomicOr(status + N + 1, (int)ST_ENV_STORE);
        return;
    }
    if (r != 0) return;
    if (hdrLane) reinterpret_cast<uint32_t *>(t.hdr + d)[threadIdx.x] = hv;
    if (log_ret && (int)threadIdx.x <= 2 * L.A) {
        const int j = (int)threadIdx.x;
        const uint32_t flags = ((GlobalSrc32)(uintptr_t)rec)[HD_FLAGS];
        const uint32_t v = loaded_log_dword(flags, *(GlobalSrc32)(uintptr_t)(rec + log_dword_offset(L, j)));
        if (j < 2 * L.A) reinterpret_cast<uint32_t *>(log_ret + (size_t)d * L.A)[j] = v;
        else log_len[d] = (int32_t)v;
    }
    copy_odd_arrays(t, L, d, const_cast<uint8_t *>(rec), false);
}

void launch_save(const Table &t, const Layout &L, uint64_t layout_word, const double *log_ret, const int32_t *log_len, const int32_t *device_slot_of, int32_t N,
                 uint8_t *store, int32_t slots, int32_t *status, hipStream_t stream)
{
    hipLaunchKernelGGL(save_kernel, dim3((unsigned)N * RANGES), dim3(THREADS), 0, stream, t, L, layout_word, log_ret, log_len, device_slot_of, N, store, slots, status);
}
void launch_load(const Table &t, const Layout &L, uint64_t layout_word, double *log_ret, int32_t *log_len, const int32_t *device_slot_of, int32_t N,
                 const uint8_t *store, int32_t slots, int32_t *status, hipStream_t stream)
{
    hipLaunchKernelGGL(load_kernel, dim3((unsigned)N * RANGES), dim3(THREADS), 0, stream, t, L, layout_word, log_ret, log_len, device_slot_of, N, store, slots, status);
}

}  // namespace store
}  // namespace mv

namespace mvapi {

// mv_create: the gym's layout word, once its table and its parameters are known
uint64_t env_record_layout_word(const mv_gym *g, const std::string &scenario_name, const mv_config *cfg)
{
    store::Hash h;
    h.u32(store::FORMAT_VERSION);
    h.u32((uint32_t)g->scenario);
    h.u32((uint32_t)scenario_name.size()); h.bytes(scenario_name.data(), scenario_name.size());
    h.u32((uint32_t)g->A); h.u32((uint32_t)g->w); h.u32((uint32_t)g->h);
    std::vector<std::pair<std::string, float>> params;
    for (int k = 0; k < cfg->num_params; ++k) params.emplace_back(cfg->param_keys[k] ? cfg->param_keys[k] : "", cfg->param_vals[k]);
    std::stable_sort(params.begin(), params.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    h.u32((uint32_t)params.size());
    for (const auto &p : params) {
        h.u32((uint32_t)p.first.size()); h.bytes(p.first.data(), p.first.size());
        h.bytes(&p.second, sizeof(float));
    }
    h.u32((uint32_t)g->forkTable.count);
    for (int k = 0; k < g->forkTable.count; ++k) h.u32(g->forkTable.a[k].bytes);
    return h.word();
}

}  // namespace mvapi

namespace {

// what every form refuses: fork_check's list, and a null store, no slots, a store off its 16-byte rows
int store_check(mv_gym *g, const void *map, const void *device_store, int32_t slots, const char *who)
{
    if (fork_check(g, map, who, "env stores")) return -1;
    if (!device_store) return fail(std::string(who) + ": null store");
    if (slots <= 0) return fail(std::string(who) + ": slots must be positive, got " + std::to_string(slots));
    if ((uintptr_t)device_store % 16 != 0) return fail(std::string(who) + ": the store must be 16-byte aligned (its records are copied in 16-byte rows)");
    return 0;
}

// The launch.  The store is the caller's memory, written and read by the caller's kernels, so every form runs on the CALLER'S stream: behind everything the
// caller enqueued (the kernel that wrote the map, whatever filled or still reads the store), behind every step launch enqueued so far (sim_join) and behind
// the episode log's last update, which lives on this stream.  The next step launch waits for it (simMustWaitUser: it overwrites what a save reads and reads
// what a load writes); nothing else is ordered behind a save, and the caller's stream sees the record complete.  No host synchronisation.  A host map
// travels through the forks' staging pair (mv_staging.h).
int store_launch(mv_gym *g, bool save, const int32_t *device_map, const int32_t *host_map, void *device_store, int32_t slots, bool read_back)
{
    HIP_TRY(hipSetDevice(g->device));
    if (sim_join(g)) return -1;
    if (!save && still_frames_touch(g)) return -1;   // (mv_set_still_frames: a load makes every env stale)
    if (host_map && g->forkMapPair.stage(host_map, (size_t)g->N * sizeof(int32_t), g->stream, &device_map)) return -1;
    const store::Layout L = store::layout_of(g->forkTable, g->A);
    const bool logOn = g->logCapacity > 0;
    if (save) store::launch_save(g->forkTable, L, g->envRecordLayout, logOn ? g->logRet : nullptr, logOn ? g->logLen : nullptr, device_map, g->N,
                                 (uint8_t *)device_store, slots, g->dStatus, g->stream);
    else store::launch_load(g->forkTable, L, g->envRecordLayout, logOn ? g->logRet : nullptr, logOn ? g->logLen : nullptr, device_map, g->N,
                            (const uint8_t *)device_store, slots, g->dStatus, g->stream);
    HIP_TRY(hipGetLastError());
    if (host_map && g->forkMapPair.mark(g->stream)) return -1;
    if (read_back) {
        // Only the kernel knows whether it skipped an entry -- of a device map, or (both load forms) one whose record's header does not match.  The status
        // words travel back behind it, and the next stepping call waits for them and reports ST_ENV_STORE: a host wait there, none here.
        HIP_TRY(hipEventRecord(g->userNow, g->stream));
        if (read_back_status(g, g->userNow)) return -1;
        g->statusReportDue = true;
    }
    return 0;
}

// the host forms' validation: -1 with text for the first invalid entry; *any: whether an entry names a slot at all
int validate_host_map(const char *who, bool save, const int32_t *slot_of, int32_t N, int32_t slots, bool *any)
{
    static thread_local std::vector<int32_t> plan;
    static thread_local std::vector<uint8_t> times;
    plan.resize((size_t)N);
    if (save) store::save_plan(slot_of, N, slots, plan.data(), times);
    else store::load_plan(slot_of, N, slots, plan.data());
    *any = false;
    for (int32_t e = 0; e < N; ++e) {
        if (plan[(size_t)e] == store::INVALID) {
            const int32_t m = slot_of[e];
            return fail(std::string(who) + ": entry " + std::to_string(e) + " = " + std::to_string(m)
                        + (!store::slot_in_range(m, slots) ? " is out of range (-1, or 0 .. " + std::to_string(slots - 1) + ")"
                                                           : " names a slot that another env names too: two envs cannot be saved into one record")
                        + "; nothing was copied");
        }
        *any = *any || plan[(size_t)e] >= 0;
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t mv_env_record_bytes(const mv_gym *g) { return !g || g->closed ? -1 : (int64_t)store::layout_of(g->forkTable, g->A).bytes; }

uint64_t mv_env_record_layout(const mv_gym *g) { return !g || g->closed ? 0 : g->envRecordLayout; }

int mv_save_envs(mv_gym *g, const int32_t *device_slot_of, void *device_store, int32_t slots)
{
    if (store_check(g, device_slot_of, device_store, slots, "mv_save_envs")) return -1;
    return store_launch(g, true, device_slot_of, nullptr, device_store, slots, true);
}

int mv_save_envs_host(mv_gym *g, const int32_t *slot_of, void *device_store, int32_t slots)
{
    if (store_check(g, slot_of, device_store, slots, "mv_save_envs_host")) return -1;
    bool any = false;
    if (validate_host_map("mv_save_envs_host", true, slot_of, g->N, slots, &any)) return -1;
    if (!any) return 0;
    return store_launch(g, true, nullptr, slot_of, device_store, slots, false);   // (everything that can be wrong with a save was looked at above)
}

int mv_load_envs(mv_gym *g, const int32_t *device_slot_of, const void *device_store, int32_t slots)
{
    if (store_check(g, device_slot_of, device_store, slots, "mv_load_envs")) return -1;
    return store_launch(g, false, device_slot_of, nullptr, const_cast<void *>(device_store), slots, true);
}

int mv_load_envs_host(mv_gym *g, const int32_t *slot_of, const void *device_store, int32_t slots)
{
    if (store_check(g, slot_of, device_store, slots, "mv_load_envs_host")) return -1;
    bool any = false;
    if (validate_host_map("mv_load_envs_host", false, slot_of, g->N, slots, &any)) return -1;
    if (!any) return 0;
    // (the records' headers are visible on the device only: the status words come back behind the launch -- the one host wait this form costs, paid in the
    // next stepping call)
    return store_launch(g, false, nullptr, slot_of, const_cast<void *>(device_store), slots, true);
}

int mv_debug_env_store_plan_host(const int32_t *slot_of, int32_t N, int32_t slots, int32_t is_save, int32_t *resolved, int32_t *invalid)
{
    if (!slot_of || N < 0 || !resolved || !invalid) return fail("mv_debug_env_store_plan_host: null argument");
    std::vector<int32_t> plan((size_t)N);
    std::vector<uint8_t> times;
    if (is_save) store::save_plan(slot_of, N, slots, plan.data(), times);   // (the host forms' tabulated rule)
    else store::load_plan(slot_of, N, slots, plan.data());
    for (int32_t e = 0; e < N; ++e) {
        const int32_t m = is_save ? store::save_resolve(slot_of, N, slots, e) : store::load_resolve(slot_of, slots, e);   // (the kernels')
        if (m != plan[(size_t)e]) return fail("mv_debug_env_store_plan_host: the tabulated rule and the per-entry rule disagree on entry " + std::to_string(e));
        resolved[e] = m >= 0 ? m : -1;
        invalid[e] = m == store::INVALID ? 1 : 0;
    }
    return 0;
}

// An env in host memory, for the two hooks below: the EnvHeader, then `count` arrays of array_bytes[k] bytes, then double ret[A] and int32 len, one behind
// the other without gaps.  offsets [count + 3]: where the EnvHeader, each array and the two accumulators lie in a record -> the record's bytes.
int64_t mv_debug_env_record_layout_host(const uint32_t *array_bytes, int32_t count, int32_t A, uint32_t *offsets)
{
    if (!array_bytes || count < 0 || count > fork::MAX_ARRAYS || A < 1 || !offsets) return fail("mv_debug_env_record_layout_host: bad argument");
    const store::Layout L = store::layout_of(array_bytes, count, A);
    offsets[0] = L.env_hdr;
    for (int32_t k = 0; k < count; ++k) offsets[1 + k] = L.off[k];
    offsets[1 + count] = L.ret;
    offsets[2 + count] = L.len;
    return (int64_t)L.bytes;
}

int mv_debug_env_record_pack_host(const uint32_t *array_bytes, int32_t count, int32_t A, uint64_t layout_word, int32_t log_on, const uint8_t *env_state_in,
                                  uint8_t *record_out)
{
    if (!array_bytes || count < 0 || count > fork::MAX_ARRAYS || A < 1 || !env_state_in || !record_out) return fail("mv_debug_env_record_pack_host: bad argument");
    const store::Layout L = store::layout_of(array_bytes, count, A);
    std::memset(record_out, 0, L.bytes);
    uint32_t *hd = reinterpret_cast<uint32_t *>(record_out);
    for (int i = 0; i < (int)store::HEADER_DWORDS; ++i) hd[i] = store::header_dword(i, layout_word, L.bytes, log_on ? (uint32_t)store::FLAG_LOG : 0u);
    const uint8_t *p = env_state_in;
    std::memcpy(record_out + L.env_hdr, p, sizeof(EnvHeader));
    p += sizeof(EnvHeader);
    for (int32_t k = 0; k < count; ++k) { std::memcpy(record_out + L.off[k], p, array_bytes[k]); p += array_bytes[k]; }
    for (int j = 0; j <= 2 * A; ++j) {
        uint32_t live;
        std::memcpy(&live, p + 4 * (size_t)j, 4);
        const uint32_t v = store::saved_log_dword(log_on != 0, live);
        std::memcpy(record_out + store::log_dword_offset(L, j), &v, 4);
    }
    return 0;
}

int mv_debug_env_record_unpack_host(const uint32_t *array_bytes, int32_t count, int32_t A, uint64_t layout_word, int32_t log_on, const uint8_t *record_in,
                                    uint8_t *env_state_inout)
{
    if (!array_bytes || count < 0 || count > fork::MAX_ARRAYS || A < 1 || !record_in || !env_state_inout) return fail("mv_debug_env_record_unpack_host: bad argument");
    const store::Layout L = store::layout_of(array_bytes, count, A);
    uint32_t hd[store::HEADER_DWORDS];
    std::memcpy(hd, record_in, sizeof(hd));
    if (!store::header_matches(hd, layout_word, L.bytes)) return 1;
    uint8_t *p = env_state_inout;
    for (int i = 0; i < 32; ++i)
        if (store::loads_header_dword(i)) std::memcpy(p + 4 * (size_t)i, record_in + L.env_hdr + 4 * (size_t)i, 4);
    p += sizeof(EnvHeader);
    for (int32_t k = 0; k < count; ++k) { std::memcpy(p, record_in + L.off[k], array_bytes[k]); p += array_bytes[k]; }
    if (log_on)
        for (int j = 0; j <= 2 * A; ++j) {
            uint32_t recorded;
            std::memcpy(&recorded, record_in + store::log_dword_offset(L, j), 4);
            const uint32_t v = store::loaded_log_dword(hd[store::HD_FLAGS], recorded);
            std::memcpy(p + 4 * (size_t)j, &v, 4);
        }
    return 0;
}

}  // extern "C"
