// megaverse_amd/csrc/mv_episode_log.h -- the episode log (include/megaverse_hip.h: mv_set_episode_log): per-agent returns and per-env lengths summed on the
// device, one record per agent of every finished env, appended in ascending (end_tick, agent) order.  No reference counterpart in the simulator: the
// reference's learner wrapper sums rewards on the host, tick by tick (megaverse_rl/megaverse_utils.py:61-86; restated in megaverse_amd/rl.py:
// Wrapper._finish_episodes).  The arithmetic is that wrapper's, operation for operation: a float64 running sum of float32 rewards.
//
// What one agent does in one tick (episode_log_tick), where a record goes (episode_log_store) and how a launch's total is committed
// (episode_log_commit) are written once, here, for the kernel (mv_episode_log.hip) and for its host twin (mv_debug_episode_log_host), which places the
// records with a plain running count where the kernel uses ballots and a scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mv {
namespace elog {

#define MV_ELOG_HD __host__ __device__ inline

enum : int { MAX_TICKS = 16 };            // ticks of one launch (= PIPE_BATCH_MAX: a stepping call's worth)
enum : int { THREADS = 1024, WAVES = THREADS / 64 };
enum : int { MAX_GROUPS = 8192 };         // (tick, chunk of 1024 agents, wave) cells a launch scans in LDS: 32 KiB; the host splits a launch that needs more
enum : int { ST_EPISODE_LOG = 16 };       // raised in the gym's status word beside ST_STARVED .. ST_CHUNK (mv_types.h) when the log starts dropping records

// mv_episode_record of the C ABI
struct Record {
    int32_t agent;            // env * A + a, local to the gym
    int32_t length;           // ticks, the finishing tick included
    uint32_t end_tick;        // ticks stepped since the last mv_reset, before the finishing tick
    float true_objective;     // what the finishing tick staged
    double ret;               // float64 sum of the episode's float32 rewards
};
static_assert(sizeof(Record) == 24, "mv_episode_record is 24 bytes");

struct Header {
    uint32_t count;           // records in the buffer
    uint32_t dropped;         // records that did not fit, since the log was switched on
    uint32_t overflowing;     // the buffer has dropped a record since records were last removed (the warning is raised once per such spell)
    uint32_t pad;
};

// one agent, one tick: true when the agent's env finished with this tick -- rec is its record, ret and len are zero again
MV_ELOG_HD bool episode_log_tick(double &ret, int32_t &len, float reward, uint8_t done, int32_t agent, uint32_t tick, float true_objective, Record &rec)
{
    ret += (double)reward;
    len += 1;
    if (!done) return false;
    rec.agent = agent;
    rec.length = len;
    rec.end_tick = tick;
    rec.true_objective = true_objective;
    rec.ret = ret;
    ret = 0.0;
    len = 0;
    return true;
}

// mv_set_step_mask: whether env e steps in the ticks of this launch.  A frozen env's tick adds nothing to the running returns of its agents or to its running
// length, and writes no record (its staged rewards are +0.0f and its staged done 0, mv_step_kernels.h: frozen_tick -- the length is what would move): the
// kernel and the host twin skip episode_log_tick, and the kernel's length pass, where this says no.  One mask per launch: it does not change within a call.
// (An episode budget, mv_set_episode_budget, halts an env in the middle of a call: the log walks a mirror of the budgets through the call's staged dones by
// the rule of mv_episode_budget.h and skips the halted ticks in the same way -- Args::budget, mv_episode_log.hip: load_done.)
MV_ELOG_HD bool episode_log_steps(const uint8_t *step_mask, int32_t e) { return !step_mask || step_mask[e] != 0; }

// mv_reset_envs, one agent i of a gym with A agents per env: where the mask flags the agent's env -- and, applied given, the env did take its next episode
// (mv_step_kernels.h: reset_masked_body) -- the episode is cut: the agent's running return goes to zero, the env's running length too (stored by the env's
// first agent), and no record is written; every other env keeps both
MV_ELOG_HD void episode_log_cut(const uint8_t *mask, const uint8_t *applied, int32_t A, int32_t i, double *ret, int32_t *len)
{
    const int32_t e = i / A;
    if (!mask[e] || (applied && !applied[e])) return;
    ret[i] = 0.0;
    if (i == e * A) len[e] = 0;
}

// the record of place `pos` in the log's order: kept if the buffer holds it
MV_ELOG_HD void episode_log_store(Record *records, uint32_t capacity, uint64_t pos, const Record &rec)
{
    if (pos < (uint64_t)capacity) records[pos] = rec;
}

// `total` records were placed behind h.count: the new count, the dropped ones; true when this is the first drop of a spell
MV_ELOG_HD bool episode_log_commit(Header &h, uint32_t capacity, uint32_t total)
{
    const uint64_t want = (uint64_t)h.count + total;
    const uint32_t kept = want < (uint64_t)capacity ? (uint32_t)want : capacity;
    const uint32_t lost = (uint32_t)(want - kept);
    h.count = kept;
    h.dropped += lost;
    if (lost == 0 || h.overflowing) return false;
    h.overflowing = 1;
    return true;
}

// One launch: up to MAX_TICKS ticks in tick order.  The staged outputs of each tick -- the hand-over slots the step kernels wrote, never the public
// arrays or the caller's rings (without a ring only the last tick is public).
struct Args {
    const float *rewards[MAX_TICKS];          // [N*A]
    const uint8_t *done[MAX_TICKS];           // [N]
    const float *true_objective[MAX_TICKS];   // [N*A], valid where done
    int32_t k, N, A;
    uint32_t capacity, first_tick;
    Header *hdr;
    double *ret;       // [N*A]
    int32_t *len;      // [N]
    Record *records;   // [capacity]
    int *status;       // the gym's status word (ST_EPISODE_LOG), or null
    const uint8_t *step_mask;   // [N] the call's step mask (episode_log_steps), or null
    int32_t *budget;            // [N] the log's mirror of the episode budgets (mv_set_episode_budget), advanced by the launch tick by tick, or null
    int32_t *macro_tl;          // [N] the log's mirror of the ticks left in a macro step (mv_macro_step, mv_macro_step.h), advanced likewise, or null
};

// ticks one launch may cover for N*A agents (the LDS cells of MAX_GROUPS)
inline int max_ticks_per_launch(int64_t agents)
{
    const int64_t chunks = (agents + THREADS - 1) / THREADS;
    const int64_t t = MAX_GROUPS / (chunks * WAVES);
    return (int)(t < 1 ? 0 : t > MAX_TICKS ? MAX_TICKS : t);
}

void launch_episode_log(const Args &a, hipStream_t stream);   // mv_episode_log.hip
void launch_episode_log_cut(const uint8_t *mask, const uint8_t *applied, int32_t N, int32_t A, double *ret, int32_t *len, hipStream_t stream);   // the masked clear of mv_reset_envs

}  // namespace elog
}  // namespace mv
