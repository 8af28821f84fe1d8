// megaverse_amd/csrc/mv_episode_log.hip -- episode_log_kernel: the ordered reduction behind mv_set_episode_log (mv_episode_log.h has the per-tick body
// and the record), and its host twin mv_debug_episode_log_host.
//
// One launch covers the ticks of one stepping call (up to 16) and is ONE workgroup of 1024 threads: the log's order -- ascending (end_tick, agent) --
// then needs no ordering between workgroups and no atomics.  Thread t owns agents t, t + 1024, ... (a "chunk" of 1024 agents per round), so within
// a chunk wave w holds agents 64 w .. 64 w + 63 in lane order, and a record's place in the log is
//     records before the launch + records of the cells before (tick, chunk, wave) + finished lanes below this one in the wave.
//   1. every wave ballots "my agent's env finished in tick j" for each tick and chunk and leaves the population count in its LDS cell; a thread's
//      loads are all issued before the first is used (load_agent: no chain of memory round trips from tick to tick);
//   2. the cells, laid out tick-major, are scanned once by the whole workgroup (shuffles within a wave, the 16 wave totals through LDS): the running
//      count is carried from tick to tick by the scan itself, not by k dependent scans;
//   3. every thread walks its agents through the ticks in registers (the float64 sum is the only chain: 16 adds) and stores the records of the
//      finishing ticks at cell + mbcnt(ballot);
//   4. behind a barrier, one thread per env writes the env's new length (len is per env, read by all of its agents in 3).
// At 1024 agents x 16 ticks that is 16 x (4 + 1 + 4) KiB read, four barriers and 256 cells: a launch's latency.
#include "mv_api_internal.h"
#include "mv_episode_log.h"
#include "mv_episode_budget.h"
#include "mv_macro_step.h"

namespace mv {
namespace elog {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// what one agent reads for the ticks of a launch.  Every load is issued before the first use -- unconditionally, a tick beyond k reads tick k - 1
// again -- so that a thread waits for memory once, not once per tick.
template <int KT>
struct AgentTicks {
    uint32_t done;              // bit t: the agent's env finished in tick t
    uint32_t steps;             // bit t: the agent's env stepped in tick t (mv_set_episode_budget; without a budget: every bit)
    float reward[KT], objective[KT];
    double ret;
    int32_t len;
};

// The done bits of env e over the launch's ticks and, BUDGET (mv_set_episode_budget): the ticks the env stepped in -- the rule of mv_episode_budget.h walked
// over the staged dones from the log's mirror of the env's budget; left: the mirror behind the launch's last tick.  A tick the env did not step in staged
// done 0 (mv_step_kernels.h: frozen_tick); its bit is cleared all the same.
// RULE_MACRO (mv_macro_step: the call's ticks are a macro step's): the rule of mv_macro_step.h walked in the same way from the log's mirror of the envs' ticks
// left, beside the budget's (a.budget: null when the gym has none); tl: that mirror behind the launch's last tick.
enum : int { RULE_NONE = 0, RULE_BUDGET = 1, RULE_MACRO = 2 };
template <int KT, int RULE>
__device__ __forceinline__ void load_done(const Args &a, int e, bool in, uint32_t &done, uint32_t &steps, int32_t &left, int32_t &tl)
{
    uint8_t d[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) d[t] = a.done[t < a.k ? t : a.k - 1][e];
    done = 0; steps = ~0u; left = -1; tl = -1;
    if constexpr (RULE == RULE_BUDGET) { left = a.budget[e]; steps = 0; }
    if constexpr (RULE == RULE_MACRO) { left = a.budget ? a.budget[e] : -1; tl = a.macro_tl[e]; steps = 0; }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        if constexpr (RULE == RULE_BUDGET) {
            if (t < a.k && budget::episode_budget_steps(1, left)) {
                steps |= 1u << t;
                (void)budget::episode_budget_spend(left, d[t]);
            }
        }
        if constexpr (RULE == RULE_MACRO) {
            if (t < a.k && macro::macro_steps(1, left, tl)) {
                steps |= 1u << t;
                (void)budget::episode_budget_spend(left, d[t]);
                tl = macro::macro_after_tick(tl, d[t]);
            }
        }
        if (in && t < a.k && d[t] && ((steps >> t) & 1u)) done |= 1u << t;
    }
}

template <int KT, int RULE>
__device__ __forceinline__ void load_agent(const Args &a, int i, int e, bool in, AgentTicks<KT> &v)
{
    const int ii = in ? i : 0;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int tt = t < a.k ? t : a.k - 1;
        v.reward[t] = a.rewards[tt][ii];
        v.objective[t] = a.true_objective[tt][ii];
    }
    v.ret = a.ret[ii];
    v.len = a.len[e];
    int32_t left, tl;
    load_done<KT, RULE>(a, e, in, v.done, v.steps, left, tl);
}

// KT: the ticks the launch is compiled for (k <= KT; 1: a single-tick call, 16: a batched call's worth)
// RULE: RULE_BUDGET: the gym has an episode budget attached (a.budget: the log's mirror); RULE_MACRO: the ticks belong to a macro step (a.macro_tl: the log's
// mirror of the ticks left; a.budget or null); RULE_NONE: neither -- the instantiations without contain no line of either
template <int KT, int RULE>
__global__ __launch_bounds__(THREADS) void episode_log_kernel(const Args a)
{
    __shared__ uint32_t cell[MAX_GROUPS];   // [tick][chunk][wave]: finished agents, then (after the scan) records in the cells before
    __shared__ uint32_t wave_total[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NA = a.N * a.A, chunks = (NA + THREADS - 1) / THREADS;
    const uint32_t base = a.hdr->count;     // (thread 0 rewrites the header behind the last barrier)
    // the first chunk -- the only one up to 1024 agents -- is read once, here, for both passes over it
    // (mv_set_step_mask) `in` below: the agent exists AND its env steps in this launch (episode_log_steps) -- the agents of a frozen env are passed over like
    // the threads beyond the last agent: no done bit, no tick, and their running return is not written
    AgentTicks<KT> first_chunk;
    load_agent<KT, RULE>(a, tid, tid < NA ? tid / a.A : 0, tid < NA && episode_log_steps(a.step_mask, tid / a.A), first_chunk);

    // ---- 1. finished agents per (tick, chunk, wave)
    for (int c = 0; c < chunks; ++c) {
        const int i = c * THREADS + tid;
        const bool in = i < NA && episode_log_steps(a.step_mask, i / a.A);
        const int e = in ? i / a.A : 0;
        uint32_t done = first_chunk.done;
        if (c > 0) {
            uint32_t steps;
            int32_t left, tl;
            load_done<KT, RULE>(a, e, in, done, steps, left, tl);
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const unsigned long long b = __ballot((done >> t) & 1u);
            if (lane == 0 && t < a.k) cell[(t * chunks + c) * WAVES + wave] = (uint32_t)__popcll(b);
        }
    }
    __syncthreads();

    // ---- 2. exclusive scan of the cells in (tick, chunk, wave) order
    const int cells = a.k * chunks * WAVES, per = (cells + THREADS - 1) / THREADS, first = tid * per;
    uint32_t mine = 0;
    for (int q = 0; q < per; ++q)
        if (first + q < cells) mine += cell[first + q];
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t run = incl - mine, total = 0;
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t v = wave_total[w];
        if (w < wave) run += v;
        total += v;
    }
    for (int q = 0; q < per; ++q)
        if (first + q < cells) {
            const uint32_t v = cell[first + q];
            cell[first + q] = run;
            run += v;
        }
    __syncthreads();

    // ---- 3. the ticks of every agent, in order; the records of the finishing ones
    for (int c = 0; c < chunks; ++c) {
        const int i = c * THREADS + tid;
        const bool in = i < NA && episode_log_steps(a.step_mask, i / a.A);
        const int e = in ? i / a.A : 0;
        AgentTicks<KT> v = first_chunk;
        if (c > 0) load_agent<KT, RULE>(a, i, e, in, v);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const bool d = ((v.done >> t) & 1u) != 0;
            const unsigned long long b = __ballot(d);
            Record rec;
            if (in && t < a.k && ((v.steps >> t) & 1u) && episode_log_tick(v.ret, v.len, v.reward[t], d ? 1 : 0, i, a.first_tick + (uint32_t)t, v.objective[t], rec))
                episode_log_store(a.records, a.capacity, (uint64_t)base + cell[(t * chunks + c) * WAVES + wave] + lanes_below(b), rec);
        }
        if (in) a.ret[i] = v.ret;
    }
    // ---- 4. the lengths, per ENV.  An env's agents may sit in different waves and chunks (agents per env that do not divide 64, more than 1024 agents),
    // and every one of them read len[e] above: nobody stores it before all have (the barrier), then one thread per env walks the env's ticks again.
    __syncthreads();
    for (int e = tid; e < a.N; e += THREADS) {
        if (!episode_log_steps(a.step_mask, e)) continue;   // (a frozen env's length stays)
        uint32_t done, steps;
        int32_t left, tl;
        load_done<KT, RULE>(a, e, true, done, steps, left, tl);
        int32_t len = a.len[e];
#pragma unroll
        for (int t = 0; t < KT; ++t)
            if (t < a.k && ((steps >> t) & 1u)) len = ((done >> t) & 1u) ? 0 : len + 1;
        a.len[e] = len;
        if constexpr (RULE == RULE_BUDGET) a.budget[e] = left;   // (the mirror: what the step kernels' array held behind the launch's last tick)
        if constexpr (RULE == RULE_MACRO) {                      // (both mirrors)
            if (a.budget) a.budget[e] = left;
            a.macro_tl[e] = tl;
        }
    }
    if (tid == 0) {
        Header h = *a.hdr;
        if (episode_log_commit(h, a.capacity, total) && a.status) atomicOr(a.status, (int)ST_EPISODE_LOG);
        *a.hdr = h;
    }
}

void launch_episode_log(const Args &a, hipStream_t stream)
{
    if (a.k < 1 || a.k > MAX_TICKS) return;   // (load_agent reads tick k - 1 for the ticks beyond k)
    const dim3 grid(1), block(THREADS);
    if (a.macro_tl) {
        if (a.k == 1) hipLaunchKernelGGL((episode_log_kernel<1, RULE_MACRO>), grid, block, 0, stream, a);
        else if (a.k <= 4) hipLaunchKernelGGL((episode_log_kernel<4, RULE_MACRO>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((episode_log_kernel<MAX_TICKS, RULE_MACRO>), grid, block, 0, stream, a);
    } else if (a.budget) {
        if (a.k == 1) hipLaunchKernelGGL((episode_log_kernel<1, RULE_BUDGET>), grid, block, 0, stream, a);
        else if (a.k <= 4) hipLaunchKernelGGL((episode_log_kernel<4, RULE_BUDGET>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((episode_log_kernel<MAX_TICKS, RULE_BUDGET>), grid, block, 0, stream, a);
    } else {
        if (a.k == 1) hipLaunchKernelGGL((episode_log_kernel<1, RULE_NONE>), grid, block, 0, stream, a);
        else if (a.k <= 4) hipLaunchKernelGGL((episode_log_kernel<4, RULE_NONE>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((episode_log_kernel<MAX_TICKS, RULE_NONE>), grid, block, 0, stream, a);
    }
}

// mv_reset_envs with the log on: one thread per agent clears what the mask flags (mv_episode_log.h: episode_log_cut).  ret is doubles, len dwords, an agent's
// slot is its own whatever the agent count: nothing here depends on A being even.
__global__ __launch_bounds__(256) void episode_log_cut_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ applied, int32_t N, int32_t A, double *ret, int32_t *len)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < N * A) episode_log_cut(mask, applied, A, i, ret, len);
}

void launch_episode_log_cut(const uint8_t *mask, const uint8_t *applied, int32_t N, int32_t A, double *ret, int32_t *len, hipStream_t stream)
{
    const int n = N * A;
    hipLaunchKernelGGL(episode_log_cut_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mask, applied, N, A, ret, len);
}

}  // namespace elog
}  // namespace mv

namespace mvapi {
using namespace mv::elog;

int episode_log_update(mv_gym *g, const GymView *views, int stride, int k)
{
    int per = max_ticks_per_launch((int64_t)g->N * g->A);
    // (tests: MV_EPISODE_LOG_TICKS=n caps the ticks of one launch, so that a call is split as it is for gyms of more than 32768 agents)
    if (const char *e = getenv("MV_EPISODE_LOG_TICKS")) per = std::min(per, std::max(1, atoi(e)));
    if (per < 1) return fail("episode log: too many agents for one launch (internal: mv_set_episode_log refuses such a gym)");
    for (int j0 = 0; j0 < k; j0 += per) {
        Args a{};
        a.k = std::min(per, k - j0);
        for (int t = 0; t < a.k; ++t) {
            const GymView &v = views[(size_t)(j0 + t) * stride];
            a.rewards[t] = v.rewards; a.done[t] = v.done; a.true_objective[t] = v.true_objective;
        }
        a.N = g->N; a.A = g->A;
        a.capacity = (uint32_t)g->logCapacity;
        a.first_tick = g->ticksSinceReset + (uint32_t)j0;
        a.hdr = g->logHdr; a.ret = g->logRet; a.len = g->logLen; a.records = g->logRecords;
        a.status = g->dStatus ? g->dStatus + g->N + 1 : nullptr;
        a.step_mask = g->stepMask.live;
        a.budget = g->budgetOn ? g->budgetMirror : nullptr;
        a.macro_tl = g->macroCall ? g->macroMirror : nullptr;   // (mv_macro_step: the ticks of a macro step)
        launch_episode_log(a, g->stream);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int episode_log_reset(mv_gym *g)
{
    g->ticksSinceReset = 0;
    if (g->logCapacity > 0)   // ret and len lie behind each other
        HIP_TRY(hipMemsetAsync(g->logRet, 0, (size_t)((uint8_t *)g->logRecords - (uint8_t *)g->logRet), g->stream));
    return 0;
}

void episode_log_free(mv_gym *g)
{
    if (g->logMem) (void)hipFree(g->logMem);
    g->logMem = nullptr; g->logBytes = 0; g->logCapacity = 0;
    g->logHdr = nullptr; g->logRet = nullptr; g->logLen = nullptr; g->logRecords = nullptr;
}

// the caller's stream drained, the header on the host
static int log_header(mv_gym *g, const char *who, Header &h)
{
    if (check(g)) return -1;
    if (g->logCapacity <= 0) return fail(std::string(who) + ": the episode log is off (mv_set_episode_log)");
    HIP_TRY(hipSetDevice(g->device));
    if (mv_flush_episode_log(g) < 0) return -1;
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(&h, g->logHdr, sizeof h, hipMemcpyDeviceToHost));
    return 0;
}
}  // namespace mvapi

extern "C" {

int mv_set_episode_log(mv_gym *g, int32_t capacity)
{
    if (capacity < 0) return fail("mv_set_episode_log: capacity >= 0 required");
    if (check(g)) return -1;
    if (capacity > 0 && max_ticks_per_launch((int64_t)g->N * g->A) < 1)
        return fail("mv_set_episode_log: more than " + std::to_string((int)MAX_GROUPS / WAVES * THREADS) + " agents in one gym");
    HIP_TRY(hipSetDevice(g->device));
    // (the log's kernels run on the caller's stream only: nothing of the log is in flight once it has drained)
    if (g->logMem) HIP_TRY(hipStreamSynchronize(g->stream));
    episode_log_free(g);
    if (capacity == 0) return 0;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t NA = (size_t)g->N * g->A;
    const size_t szHdr = up(sizeof(Header)), szRet = NA * sizeof(double), szLen = up(szRet + (size_t)g->N * sizeof(int32_t)) - szRet;
    const size_t total = szHdr + szRet + szLen + (size_t)capacity * sizeof(Record);
    {
        hipError_t e_ = hipMalloc((void **)&g->logMem, total);
        if (e_ != hipSuccess) { g->logMem = nullptr; return fail("mv_set_episode_log: hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(e_)); }
    }
    g->logBytes = total;
    g->logHdr = (Header *)g->logMem;
    g->logRet = (double *)(g->logMem + szHdr);
    g->logLen = (int32_t *)(g->logMem + szHdr + szRet);
    g->logRecords = (Record *)(g->logMem + szHdr + szRet + szLen);
    HIP_TRY(hipMemsetAsync(g->logMem, 0, szHdr + szRet + szLen, g->stream));
    g->logCapacity = capacity;
    return episode_budget_seed_mirror(g);   // (mv_set_episode_budget: a budget attached while the log was off)
}

int mv_get_episode_log_capacity(const mv_gym *g) { return g && !g->closed ? g->logCapacity : -1; }

int mv_flush_episode_log(mv_gym *g)
{   // every stepping call enqueues its own update behind its publication: nothing is deferred, nothing to enqueue here
    if (check(g)) return -1;
    if (g->logCapacity <= 0) return fail("mv_flush_episode_log: the episode log is off (mv_set_episode_log)");
    return 0;
}

int mv_episode_log_count(mv_gym *g, uint32_t *count, uint32_t *dropped)
{
    Header h;
    if (log_header(g, "mv_episode_log_count", h)) return -1;
    if (count) *count = h.count;
    if (dropped) *dropped = h.dropped;
    return 0;
}

int mv_drain_episode_log(mv_gym *g, mv_episode_record *out_host, int32_t max_records, uint32_t *dropped)
{
    static_assert(sizeof(mv_episode_record) == sizeof(Record), "the ABI's record is the kernel's");
    if (max_records < 0 || (max_records > 0 && !out_host)) return fail("mv_drain_episode_log: max_records >= 0 and a buffer required");
    Header h;
    if (log_header(g, "mv_drain_episode_log", h)) return -1;
    if (dropped) *dropped = h.dropped;
    const uint32_t n = std::min(h.count, (uint32_t)max_records), rest = h.count - n;
    if (n == 0) return 0;
    HIP_TRY(hipMemcpy(out_host, g->logRecords, (size_t)n * sizeof(Record), hipMemcpyDeviceToHost));
    if (rest) {   // the rest moves to the front, order kept (through the host: the two ranges may overlap)
        std::vector<Record> keep(rest);
        HIP_TRY(hipMemcpy(keep.data(), g->logRecords + n, (size_t)rest * sizeof(Record), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(g->logRecords, keep.data(), (size_t)rest * sizeof(Record), hipMemcpyHostToDevice));
    }
    h.count = rest;
    h.overflowing = 0;   // room again: the next drop is reported anew
    HIP_TRY(hipMemcpy(g->logHdr, &h, sizeof h, hipMemcpyHostToDevice));
    return (int)n;
}

void *mv_episode_log_records_device_ptr(mv_gym *g) { return g && !g->closed ? (void *)g->logRecords : nullptr; }
void *mv_episode_log_count_device_ptr(mv_gym *g) { return g && !g->closed ? (void *)g->logHdr : nullptr; }
void *mv_episode_returns_device_ptr(mv_gym *g) { return g && !g->closed ? (void *)g->logRet : nullptr; }
void *mv_episode_lengths_device_ptr(mv_gym *g) { return g && !g->closed ? (void *)g->logLen : nullptr; }
int64_t mv_ticks_since_reset(const mv_gym *g) { return g && !g->closed ? (int64_t)g->ticksSinceReset : -1; }


// The kernel's per-tick body compiled for the CPU (no device): k ticks of N envs x A agents through episode_log_tick in (tick, agent) order.
// count, dropped, ret [N*A] and len [N] in and out; records: the buffer of `capacity` records, *count of them valid on entry.  step_mask [N] or null: the
// envs it freezes skip every one of the k ticks (episode_log_steps).  left [N] or null (mv_set_episode_budget), in and out: the log's mirror of the budgets,
// advanced tick by tick by the rule of mv_episode_budget.h -- a tick of a halted env is skipped like a frozen one's.
// (tl [N] or null, in and out: mv_macro_step -- the log's mirror of the ticks left in the macro step the k ticks belong to, mv_macro_step.h)
int mv_debug_episode_log_macro_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A, int32_t capacity,
                                    uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped, const uint8_t *step_mask,
                                    int32_t *left, int32_t *tl)
{
    using namespace mv::elog;
    if (!rewards || !dones || !true_objectives || !ret || !len || !records || !count || !dropped || k < 0 || N < 1 || A < 1 || capacity < 1)
        return fail("mv_debug_episode_log_host: bad arguments");
    if (*count > (uint32_t)capacity) return fail("mv_debug_episode_log_host: count above capacity");
    Record *out = (Record *)records;
    const size_t NA = (size_t)N * A;
    Header h{*count, *dropped, 0u, 0u};
    for (int t = 0; t < k; ++t) {
        uint32_t placed = 0;
        for (int e = 0; e < N; ++e) {
            if (!episode_log_steps(step_mask, e)) continue;
            if (left && !mv::budget::episode_budget_steps(1, left[e])) continue;
            if (tl && !mv::macro::macro_steps(1, -1, tl[e])) continue;
            int32_t after = len[e];
            for (int a = 0; a < A; ++a) {
                const size_t i = (size_t)e * A + a;
                int32_t l = len[e];
                Record rec;
                if (episode_log_tick(ret[i], l, rewards[(size_t)t * NA + i], dones[(size_t)t * N + e], (int32_t)i, first_tick + (uint32_t)t,
                                     true_objectives[(size_t)t * NA + i], rec))
                    episode_log_store(out, (uint32_t)capacity, (uint64_t)h.count + placed++, rec);
                after = l;
            }
            len[e] = after;
            if (left) (void)mv::budget::episode_budget_spend(left[e], dones[(size_t)t * N + e]);
            if (tl) tl[e] = mv::macro::macro_after_tick(tl[e], dones[(size_t)t * N + e]);
        }
        (void)episode_log_commit(h, (uint32_t)capacity, placed);
    }
    *count = h.count;
    *dropped = h.dropped;
    return 0;
}

// ... outside a macro step
int mv_debug_episode_log_budget_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A, int32_t capacity,
                                     uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped, const uint8_t *step_mask,
                                     int32_t *left)
{
    return mv_debug_episode_log_macro_host(rewards, dones, true_objectives, k, N, A, capacity, first_tick, ret, len, records, count, dropped, step_mask, left, nullptr);
}

// ... without a budget
int mv_debug_episode_log_masked_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A, int32_t capacity,
                                     uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped, const uint8_t *step_mask)
{
    return mv_debug_episode_log_budget_host(rewards, dones, true_objectives, k, N, A, capacity, first_tick, ret, len, records, count, dropped, step_mask, nullptr);
}

// ... without a step mask: every env steps
int mv_debug_episode_log_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A, int32_t capacity,
                              uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped)
{
    return mv_debug_episode_log_masked_host(rewards, dones, true_objectives, k, N, A, capacity, first_tick, ret, len, records, count, dropped, nullptr);
}

// The masked clear of mv_reset_envs compiled for the CPU (no device): episode_log_cut over every agent of N envs x A agents.
int mv_debug_episode_log_cut_host(const uint8_t *mask, int32_t N, int32_t A, double *ret, int32_t *len)
{
    if (!mask || !ret || !len || N < 1 || A < 1) return fail("mv_debug_episode_log_cut_host: bad arguments");
    for (int32_t i = 0; i < N * A; ++i) mv::elog::episode_log_cut(mask, nullptr, A, i, ret, len);
    return 0;
}

}  // extern "C"
