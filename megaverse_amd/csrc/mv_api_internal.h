// megaverse_amd/csrc/mv_api_internal.h -- what the host side of libmegaverse_hip.so shares between its translation units:
//   mv_api.hip        create / close, seeding, reset, actions, output rings, getters, reward shaping (MegaverseGym's methods but step)
//   mv_scenarios.h / .cpp  the scenario families, one row each: names, reward shaping, episode record and generator, strides, defaults, state arrays (host-only,
//                     needs nothing of this file: mv_feeder.cpp reads it too)
//   mv_api_step.hip   stepping: pipelining, batched calls, overlapped passes, groups (union launches), in-stream profiling
//   mv_api_debug.hip  test hooks: snapshots, pose setters, host-side generators, RNG / arithmetic probes
//   mv_fork.hip       env forks: the gather-copy kernel and its entry points; the entry points of env resampling
//   mv_resample.hip   env resampling: the two kernels of the staged copy
//   mv_reset_envs.hip masked env resets: the host protocol around the reset_masked kernels (mv_step_kernels.h)
//   mv_seed_envs.hip  level seeds: Env::seed for chosen envs -- the two launch protocols (device-drawn, host-fed), the feeder's host-only hook
//   mv_env_store.hip  env stores: the save / load kernels, their entry points and host-only hooks
//   mv_env_masks.hip  step masks and draw masks: attaching and detaching the bytes that freeze envs (mv_step_kernels.h: frozen_tick) and the bytes that leave
//                     envs' frames out of the observation passes (mv_frame.h: frame_skip)
//   mv_obs_rows.hip   state and scene observations: attaching the caller's buffers, the staging rows, the one publication launch both records share, their
//                     refresh (mv_state_obs.h, mv_scene_obs.h: the records)
//   mv_obs_planes.hip  depth, segmentation and normal observations: attaching the caller's buffers, the ONE launch behind a fast pass that writes whatever of
//                     depth, labels and normals is attached (mv_depth_obs.h, mv_seg_obs.h, mv_normal_obs.h: the records and their rules; mv_raster.hip: the kernels)
//   mv_episode_budget.hip  episode budgets: attaching, detaching and reading the per-env counts that halt envs (mv_episode_budget.h: the rule)
//   mv_macro_step.hip macro steps: the launch that starts a call's per-env tick counts, the accumulating publication, the entry points (mv_macro_step.h: the rule)
//   mv_overview.hip   overview cameras: attaching the buffer, the overview's own arrays, the cameras' two forms, mv_draw_overview (mv_overview.h: the rule;
//                     mv_raster.hip: the kernels)
//   mv_still_frames.hip  still frames: switching the option, the memset behind calls that change what frames show, the carry launch (mv_still_frames.h: the rule)
// The persistent per-gym options are stated once, below mv_gym: gym_options (who refuses what, in which words) and fill_view_options (what a view carries).
// mv_staging.h holds the two ways the host forms' values reach the device (StagingPool, StagingPair).
// The C ABI itself is include/megaverse_hip.h; nothing here is exported under a C name.
#pragma once
#include <hip/hip_runtime.h>

#include <sched.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/megaverse_hip.h"
#include "mv_feeder.h"
#include "mv_actions.h"
#include "mv_gen.h"
#include "mv_scenarios.h"
#include "mv_raster.h"
#include "mv_math.h"
#include "mv_rng.h"
#include "mv_types.h"
#include "mv_union.h"
#include "mv_episode_log.h"
#include "mv_episode_budget.h"
#include "mv_macro_step.h"
#include "mv_fork.h"
#include "mv_overview.h"

namespace mv {
// TowerBuilding: tops every env's ring of drawn episodes up (mv_reset.hip)
void launch_tower_draw(const GymView &gv, hipStream_t stream);
void launch_tower_seed(const GymView &gv, const uint32_t *seeds, hipStream_t stream);   // Env::seed for every env's generator
void launch_tower_seed_envs(const GymView &gv, const int32_t *seeds, hipStream_t stream);   // mv_seed_envs: ... for the envs whose seeds[env] >= 0
// Device-drawn episodes (mv_collect_draw.hip): staging slots of envs[i] -> their ring slots slots[i], one launch per 64 episodes, with the copy kernel of the
// family's draw (mv_scenarios.h: DRAW_*) -- Collect's takes the record's used prefix, the other takes records of any size whole
void launch_blob_copy(int draw, const int32_t *envs, const int32_t *slots, int count, const uint8_t *staging, uint8_t *ring, size_t blob_bytes, int spares,
                      hipStream_t stream);
// The step and reset kernels of gv's scenario (mv_step.hip).  One tick: one workgroup per env = the tick (wave 0) + the frame setup of the env's frames
// for a W x H observation (render = 0: tick only); done: an event carried by the launch's dispatch packet (TowerBuilding only) -> whether it was.
bool launch_step(const GymView &gv, hipStream_t stream, int W, int H, int render, hipEvent_t done = nullptr);
// k <= 8 ticks + frame setups of every env, one launch (one agent per env; several: TowerBuilding); done: completed by the launch
void launch_step_ticks(const GymView *views, int k, hipStream_t stream, int W, int H, hipEvent_t done = nullptr);
// k <= 8 ticks of every env, one launch; frame setups only for the ticks whose bit is set in frame_mask (mv_step_n_render: MV_RENDER_NONE / MV_RENDER_LAST)
void launch_step_ticks_sim(const GymView *views, int k, unsigned frame_mask, hipStream_t stream, int W, int H, hipEvent_t done = nullptr);
// every finished (force_all: every) env swaps its next resident episode in
void launch_reset_episodes(const GymView &gv, int force_all, hipStream_t stream);
// mv_reset_envs: the envs mask [num_envs] flags take their next resident episode; applied [num_envs]: 1 / 0 for every flagged env, whether it did
void launch_reset_envs(const GymView &gv, const uint8_t *mask, uint8_t *applied, hipStream_t stream);
}  // namespace mv

using namespace mv;


namespace mvapi {
// the bytes of one w x h observation frame in a layout (include/megaverse_hip.h: mv_set_obs_layout)
inline size_t frame_bytes(int w, int h, int layout) { return (size_t)w * h * (layout == MV_OBS_RGB_PLANAR ? 3 : 4); }
// the alignment a planar slab of w-pixel rows needs: its 16-byte stores (w % 16 == 0: whole tile rows), its dword stores (w % 4 == 0), else bytes
inline size_t planar_alignment(int w) { return w % 16 == 0 ? 16 : w % 4 == 0 ? 4 : 1; }
extern thread_local std::string g_err;   // mv_last_error()
inline int fail(const std::string &msg)
{
    g_err = msg;
    return -1;
}
}  // namespace mvapi
using namespace mvapi;
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

#include "mv_staging.h"

namespace mvapi {
// An attached per-env byte mask (mv_env_masks.hip: step masks, draw masks).  live: the [N] bytes the kernels read, null: no mask.  Form 1: the caller's
// buffer.  Form 2: owned, the gym's, allocated at the host form's first use and counted in mv_arena_bytes; its bytes travel through the pool.
struct EnvMask {
    const uint8_t *live = nullptr;
    int form = 0;
    uint8_t *owned = nullptr;
    size_t ownedBytes = 0;
    StagingPool pool;
};
}  // namespace mvapi

namespace mvapi {
// One chunk of a macro step (mv_macro_step; mv_api_step.hip: step_gyms): the actions every tick of the call holds, and where the chunk stands in the call --
// the first chunk starts the call's one output entry, the last one completes it.
struct MacroCall {
    const int32_t *actions;   // [N*A][6] device memory
    bool first, last;
};
}  // namespace mvapi

namespace mvapi {
// One row record of a gym (mv_obs_rows.hip: state observations [N*A][16], scene observations [N][32], entity observations [N][E][8]).  buf: the caller's [entries][words] float32 buffer (null:
// off; entries: the output ring's count when it was attached, or 1); stage: the gym's staging rows [slots][words], allocated at the first attach and kept
// until mv_close (stageBytes; not part of the arena).  While attached, the record's field of gvp[q] points at slot q's rows: the stepping calls' views carry it
// to the MASKED step kernels.
struct ObsRows {
    float *buf = nullptr, *stage = nullptr;
    int entries = 0;
    size_t stageBytes = 0, words = 0;   // words: of one entry, the whole gym's rows
    // tick `tick`'s entry of the caller's buffer: the entry its rewards go to (outputs_of)
    float *entry(unsigned long long tick) const { return buf + (size_t)(tick % (unsigned long long)entries) * words; }
};
}  // namespace mvapi

namespace mvapi {
// One plane record of a gym (mv_obs_planes.hip: depth, segmentation and normal observations).  buf: the caller's [entries][N*A][H][W] buffer -- depth: of
// float or __half, labels: of bytes or 16-bit words, normals: of four halves or four signed bytes (null: off; entries: the output ring's count when it was attached, or 1); format: MV_DEPTH_F32 /
// MV_DEPTH_F16, MV_SEG_CLASS_U8 / MV_SEG_INSTANCE_U16, MV_NORMAL_F16 / MV_NORMAL_SNORM8; entryBytes: one entry, the whole gym's planes.
struct ObsPlanes {
    void *buf = nullptr;
    int format = 0, entries = 0;
    size_t entryBytes = 0;
    // tick `tick`'s entry of the caller's buffer: the entry its frames go to (outputs_of)
    void *entry(unsigned long long tick) const { return buf ? (uint8_t *)buf + (size_t)(tick % (unsigned long long)entries) * entryBytes : nullptr; }
};
}  // namespace mvapi

namespace mvapi {
// The overview of a gym (mv_overview.hip).  buf: the [N][h][w] RGBA8 frames mv_draw_overview writes (null: not attached) -- the caller's, or `owned`, the gym's;
// arrays: the overview's own lists, rectangles, headers, counts, cost bins, frame order, cameras and dropped word (mv_overview.h: overview_layout), allocated
// by the first attach, kept until mv_close and counted in mv_arena_bytes, as the owned frames are while they exist.  The host form's records travel through the pool.
struct OverviewState {
    uint32_t *buf = nullptr, *owned = nullptr;
    int w = 0, h = 0, cap = 0;
    bool costOrder = true;   // MV_OVERVIEW_ORDER=0 at the first attach: frames are drawn in env order, no frame-order launch (profiles/overview_measured.txt)
    size_t ownedBytes = 0;
    uint8_t *arrays = nullptr;
    OverviewLayout layout{};
    StagingPool pool;
};
}  // namespace mvapi

static_assert(PIPE_GROUPS == 3, "userMark events are created one by one in mv_create");
struct mv_gym;
struct mv_group {
    std::vector<mv_gym *> gyms;   // gyms[0] is the leader; empty once a member was closed
};
struct mv_gym {
    int device = 0;
    int w = 0, h = 0, renderW = 768, renderH = 432;   // megaverse.cpp:261
    int N = 0, A = 0, envOffset = 0, envStride = 1, totalEnvs = 0;
    bool samplePending = false;                  // mv_sample_random_actions: the next step draws its own actions
    int samplePolicy = POLICY_MULTIDISCRETE;     // mv_set_sample_policy: which generator mv_sample_random_actions requests
    bool closed = false, wasReset = false;
    hipStream_t stream = nullptr;                // the caller's stream: observation passes, published outputs, everything it may consume
    // One-step-ahead pipelining: the step kernels run on an internal stream.  A step only waits for what the caller had
    // enqueued on its stream when the PREVIOUS mv_step began (consumers of outputs two steps old), so step t + 1 overlaps the observation
    // pass of step t whenever nothing on the caller's stream feeds it (device-sampled or host-provided actions).  Everything a step
    // hands to the observation pass or to the caller exists PIPE_BUFS times: frame lists / headers / cost lists, and the rewards /
    // dones / true objectives, which the observation pass (on the caller's stream) publishes into the stable public arrays.
    // Slots: PIPE_GROUPS groups of `batch` hand-over buffers.  One call -- mv_step (one tick) or mv_step_n (up to `batch` ticks) -- takes the
    // next group; its step kernels wait for the mark recorded PIPE_GROUPS - 1 calls ago.  With k ticks per call the two cross-queue
    // hand-overs (mark -> simulation stream, simDone -> caller's stream, ~10 us of command-processor time each) are paid once per k ticks.
    hipStream_t simStream = nullptr;
    int pipelined = 1;                           // mv_set_pipelining / MV_PIPELINE: 0 = everything on the caller's stream, in order
    bool simOnOwnStream = false;                 // where the last step ran
    hipEvent_t userMark[PIPE_GROUPS] = {};       // completed when the last observation pass of a stepping call is, round-robin over the calls
    hipEvent_t userNow = nullptr;                // recorded on `stream` when the simulation must wait for all of it
    long dbgCalls = 0;                           // (instrumented builds)
    unsigned long long markCount = 0;             // (64 bits: a training run takes 2^31 steps in a day and a half)
    bool simMustWaitUser = true;                 // the caller's stream holds work the next step depends on (reset, render, device actions, ...)
    hipEvent_t simDone = nullptr;                // after the last kernel on simStream
    bool simDoneValid = false;
    // slots per group (ticks per call: set by mv_create from the slots' footprint, or MV_PIPE_BATCH), slots, cost histograms
    int batch = 8, slots = PIPE_GROUPS * 8, hists = PIPE_GROUPS * 8 + 1;
    int group = 0;                               // slot group of the last stepping call
    int parity = 0, hist3 = 0;                   // hand-over slot of the last tick; cost histogram of the last pass
    // histClean[h]: cost histogram h is (or, in stream order, will be) all zero when the next frame setup counts into it.  A pass drawn by the
    // one-launch observation kernel clears its histogram itself once its last workgroup has looked its frame up (mv_raster.hip: hist_done); a
    // tick of the one-launch-per-tick path clears the NEXT pass's in its frame setup (mv_frame.h); what neither covers -- the hand-over between
    // the two paths -- is cleared by take_hist with a memset.
    std::vector<uint8_t> histClean;
    std::vector<GymView> gvp;                    // [slots] gv with the buffers of each slot swapped in
    GymView gv{};
    const int32_t *mdActions = nullptr;          // mv_set_actions_device: the caller's multi-discrete buffer, read by the next step kernel
    // mv_set_action_ring: the caller's [actRingCount][N*A][6] multi-discrete actions; an MV_POLICY_SEQUENCE call reads entry (first_step_index + j) % count in tick j
    const int32_t *actRing = nullptr;
    int actRingCount = 0;
    // mv_debug_launch_counts: step launches and observation launches the stepping calls have enqueued (kept on the leader of a group)
    long long launchCount[2] = {0, 0};
    // mv_set_pass_overlap(1), ring at least two calls deep: the one-launch observation passes of consecutive batched calls go to two internal streams
    // in turn, so that the passes of call c + 1 start -- their step launch permitting -- while those of call c drain (a launch ends with its last
    // workgroups finishing alone, and the next one could not begin before: ~7 % of a 1024-env call).  The caller's stream waits for every call's
    // passes as before; what the passes of call c wait for on the caller's side is what was enqueued before call c - 1 began (callStart).
    int passOverlap = 0;
    hipStream_t passStream[2] = {nullptr, nullptr};
    hipEvent_t callStart[2] = {nullptr, nullptr};
    unsigned long long overlapCalls = 0;   // consecutive calls that took the overlapped path (0: the last call's passes ran on the caller's stream)
    // mv_set_output_ring: tick number t (since the ring was set) leaves its observations / rewards / dones in entry t % ringCount
    int ringCount = 0;
    unsigned long long ringTick = 0;
    uint8_t *ringObs = nullptr, *ringDone = nullptr;
    float *ringRewards = nullptr;
    std::string warning;                         // soft conditions (capacity flags) of the last call: returned as 1, not as an error
    // mv_group: the gyms of a group share the leader's simulation stream and events; a member keeps its own handles here until it leaves
    mv_group *inGroup = nullptr;
    hipStream_t ownSimStream = nullptr, ownCopyStream = nullptr;
    hipEvent_t ownUserMark[PIPE_GROUPS] = {}, ownSimDone = nullptr, ownStepDone = nullptr;
    uint8_t *arena = nullptr;
    size_t arenaBytes = 0;
    uint32_t *obs = nullptr, *ownedObs = nullptr, *hiresObs = nullptr;
    int hiresW = 0, hiresH = 0;
    int fastPixels = 1;                          // mv_set_pixel_mode: 1 = raster_fast_kernel (default), 0 = bit-exact raster_kernel
    // mv_set_obs_layout: MV_OBS_RGBA (default) or MV_OBS_RGB_PLANAR; fixed by the first reset / render / obs buffer / output ring (layoutFixed)
    int obsLayout = MV_OBS_RGBA;
    bool layoutFixed = false;
    size_t frameBytes() const { return frame_bytes(w, h, obsLayout); }   // one observation frame in this gym's layout
    // host mirrors
    int32_t *hActions[2] = {nullptr, nullptr};   // pinned staging, double buffered
    hipEvent_t actionsCopied[2] = {nullptr, nullptr};
    int stage = 0;
    bool actionsDirty = false;
    int32_t *dMultiDiscrete = nullptr;           // [N*A*6] scratch for batched host actions
    std::vector<float> hRewards, hTrueObj;
    std::vector<uint8_t> hDone;
    bool mirrorsFresh = false;
    std::mt19937 rng{std::random_device{}()};    // megaverse.cpp:253
    // scenario
    int scenario = SCN_TOWER;
    std::string scenarioName;                       // as given to mv_create, lower case (messages)
    int numShaping = 4;
    const char *const *shapingKeys = nullptr;
    ObstacleConfig obst;
    float baseEpisodeLen = 60.0f;
    // Obstacles / Collect: background episode feeder + one resident episode per env (refill protocol below)
    std::unique_ptr<EpisodeFeeder> feeder;
    int feederThreads = 1;
    std::vector<int> consumedSeen;                  // the consumed counts of the last status read-back that was looked at (host copy)
    std::vector<int> uploaded, uploadBatch;         // episodes uploaded per env; envs of the current upload batch
    uint8_t *dBlobs = nullptr, *hBlobs = nullptr;   // device [N][blobBytes], pinned feeder slots [N][blobBytes]
    bool blobsOnDevice = false;                     // the feeder runs in device mode (Collect, the Obstacles family, Empty): hBlobs is device memory, filled by the scenario's draw kernel (mv_feeder.cpp)
    size_t blobBytes = 0;                           // the scenario's record size (mv_scenarios.h: record_bytes)
    bool hostEpisodes() const { return scenario != SCN_TOWER; }
    // TowerBuilding: the episode generator's serial half (tower_draw_kernel, ~47 us of one wavefront per finished env) runs on a stream of its own,
    // behind the step launch whose finished envs it refills and beside everything else; a stepping call waits for the draw launch BEFORE the last one
    // (two episodes are resident per env: what the last launch is still drawing is not needed yet).  drawPeriod: ticks between draw launches -- 8 where
    // episodes last at least 64 ticks, every call where they can be a few ticks long (those calls are one tick each: mv_step_n).
    hipStream_t genStream = nullptr;
    hipEvent_t drawDone[2] = {nullptr, nullptr};
    unsigned long long drawCount = 0, drawWaitedCount = 0;   // draw launches so far; the count at the last tower_draw_before wait ...
    hipStream_t drawWaitedOn = nullptr;                       // ... and the stream that waited
    int ticksSinceDraw = 0, drawPeriod = 1;
    int *dStatus = nullptr, *hStatus = nullptr;     // [N + 2]: consumed per env, total, error flags (device, pinned mirror)
    int lastTotalSeen = 0;
    bool statusPending = false, refillForce = true;
    int pendingAge = 0;                             // ticks enqueued since the pending read-back was issued
    int stepsSinceStatus = 0;
    int spares = 2;                                 // resident episodes per env (ring); the host keeps uploaded <= consumed + spares
    int statusPeriod = 16;                          // steps between status read-backs (1 when episodes can be only a few ticks long)
    int deficit = 0;                                // spares still to be uploaded (their episodes were not generated yet at the last look)
    hipEvent_t stepDone = nullptr;                  // after the last step kernel: uploads never overlap a kernel that may read the ring
    hipStream_t copyStream = nullptr;               // status read-back + episode uploads, off the step path
    hipEvent_t statusCopied = nullptr;
    // the event behind the last kernel that may read the ring (a step launch's simDone / stepDone, mv_reset's stepDone)
    hipEvent_t lastStep = nullptr;
    std::vector<hipEvent_t> uploadEvents;           // ring, one per upload batch
    hipEvent_t lastUpload = nullptr;                // the most recent batch (mv_reset: the caller's stream waits for it too)
    bool uploadNotOnUser = false;                   // ... and a step that runs on the caller's stream has not waited for it yet
    size_t uploadRing = 0;
    // mv_set_episode_log: returns / lengths summed on the device, one record per agent of a finished env (mv_episode_log.h).  One allocation:
    // header, ret [N*A], len [N], records [logCapacity]; updated by one launch per stepping call on the caller's stream.
    int logCapacity = 0;                         // 0: off
    uint8_t *logMem = nullptr;
    size_t logBytes = 0;
    elog::Header *logHdr = nullptr;
    double *logRet = nullptr;
    int32_t *logLen = nullptr;
    elog::Record *logRecords = nullptr;
    uint32_t ticksSinceReset = 0;                // ticks stepped since the last mv_reset: a record's end_tick
    // mv_fork_envs: the per-env arrays that make up an env's episode state (filled by mv_create where it carves the arena; mv_fork.h), the host forms' way to
    // the device for their [N] map words (also mv_resample_envs_host's and the env stores')
    fork::Table forkTable{};
    StagingPair forkMapPair;
    // mv_resample_envs: the staging arena (fork::Staging: a second slice per env of every array of the table, the episode log's included, and one plan byte
    // per env), allocated at the first call and counted in mv_arena_bytes from then on
    uint8_t *resampleArena = nullptr;
    size_t resampleBytes = 0;
    // mv_save_envs / mv_load_envs: the layout word of this gym's records (mv_env_store.h); the gym owns no store
    uint64_t envRecordLayout = 0;
    // "the next stepping call waits for the status words" (refill_episodes): something only a kernel saw has to be reported by that call -- a fork's device map
    // may have held invalid entries (ST_FORK), a masked reset from a device mask may have found a host-fed env without a resident episode (ST_STARVED)
    bool statusReportDue = false;
    // mv_reset_envs: the host form's [N] mask bytes on their way to the device, and `applied` [N] (which flagged envs took an episode: device bytes of both
    // forms, allocated at the first use)
    StagingPair resetMaskPair;
    uint8_t *resetApplied = nullptr;
    // mv_seed_envs_host: its [N] seed words on their way to the device
    StagingPair seedEnvsPair;
    // mv_set_step_mask: the bytes the step kernels read (GymView::step_mask through the stepping calls' views)
    EnvMask stepMask;
    // mv_set_draw_mask: the bytes the frame setups read (GymView::draw_mask through the views of the stepping calls and of mv_render)
    EnvMask drawMask;
    // mv_set_state_obs, mv_set_scene_obs, mv_set_entity_obs (ObsRows).  The scene and entity rows' staging is counted in mv_arena_bytes from its allocation
    // on, the state rows' is not.
    ObsRows stateRows, sceneRows, entityRows;
    // mv_set_depth_obs: the caller's depth planes, written by the passes of a gym in exact pixel mode and by a launch behind the passes of one in fast mode
    ObsPlanes depth;
    // mv_set_seg_obs: the caller's label planes, written by the passes of a gym in exact pixel mode and -- fast mode -- by the one launch behind its passes,
    // which then writes the depth planes too
    ObsPlanes seg;
    // mv_set_normal_obs: the caller's normal planes, written as the other two: by the exact pass itself, or by the one launch behind a fast pass
    ObsPlanes normal;
    // mv_set_overview: the overview cameras' frames and arrays
    OverviewState overview;
    // mv_set_episode_budget: one gym-owned allocation (mv_episode_budget.h: episode_budget_words), made at first use and counted in mv_arena_bytes --
    // budgetLeft [N], what the step kernels read and write (GymView::budget, through the stepping calls' views, while budgetOn); budgetHalted, the count of
    // zeros in it; budgetMirror [N], the episode log's own copy, advanced by the log's update tick by tick.  The host form's values travel through a pool of
    // N + 1 words: the budgets and the halted count.
    int32_t *budgetLeft = nullptr, *budgetMirror = nullptr;
    uint32_t *budgetHalted = nullptr;
    bool budgetOn = false;
    size_t budgetBytes = 0;
    StagingPool budgetPool;
    // mv_macro_step: one gym-owned allocation (mv_macro_step.h: macro_step_words), made at first use and counted in mv_arena_bytes -- macroTl [N], the ticks
    // each env may still step in the call in flight, what the step kernels read and write (GymView::macro_tl, through the views of a macro step's ticks only);
    // macroMirror [N], the episode log's own copy; macroTicks [N] and macroActions [N*A][6], where the host form's values land (through a pool of N + 6 N A
    // words).  macroCall: the chunk that is being enqueued, null outside mv_macro_step.
    int32_t *macroTl = nullptr, *macroMirror = nullptr, *macroTicks = nullptr, *macroActions = nullptr;
    size_t macroBytes = 0;
    StagingPool macroPool;
    const MacroCall *macroCall = nullptr;
    // mv_set_still_frames: one gym-owned allocation (mv_still_frames.h: still_frames_bytes), made when the option is first switched on, kept until mv_close
    // and counted in mv_arena_bytes -- stillHome [N*A], the ring entry that holds each frame's latest drawn bytes (the carry launch's own), and stillStale [N],
    // what the step kernels read and write (GymView::still, through the stepping calls' views, while stillOn).
    int32_t *stillHome = nullptr;
    uint8_t *stillStale = nullptr;
    size_t stillBytes = 0;
    bool stillOn = false;
    // in-stream profiling
    std::vector<hipEvent_t> profEvents;          // 5 per profiled tick: [0] [1] around the step kernel (its stream), [2] [3] [4] before the
                                                 // observation pass, between frame sort and raster, after the raster (the caller's stream)
    int profMax = 0, profCount = 0;
    std::vector<int> profTicks;                  // ticks an entry covers: 1, or the k ticks of a batched call whose launches are timed as a whole
};

namespace mvapi {
// ---- The persistent per-gym options, stated once: one descriptor each, in the order every refusal walks them.  A new option is one row here and one line in
// fill_view_options.
struct GymOption {
    const char *setter;       // the entry point that attaches it
    const char *has;          // mv_group_create / mv_step_many: "a gym has <has> (<setter>)"
    const char *unionNone;    // mv_group_create: "the union launches <unionNone>"
    const char *detach;       // mv_group_create: "<detach>"
    const char *detachMany;   // mv_step_many: "step it on its own, or <detachMany>"
    const char *memberNone;   // attach_check: "whose union launches <memberNone>"
    bool (*on)(const mv_gym *);
};
enum : int { OPT_STEP_MASK = 0, OPT_DRAW_MASK, OPT_STILL_FRAMES, OPT_EPISODE_BUDGET, OPT_STATE_OBS, OPT_SCENE_OBS, OPT_DEPTH_OBS, OPT_SEG_OBS, OPT_NORMAL_OBS, OPT_ENTITY_OBS, OPT_OVERVIEW, OPT_COUNT };
#define MV_OPT_ON(expr) +[](const mv_gym *g) -> bool { return expr; }
inline constexpr GymOption gym_options[OPT_COUNT] = {
    {"mv_set_step_mask", "a step mask attached", "read none", "detach it first", "detach the mask first", "read no step mask", MV_OPT_ON(g->stepMask.live)},
    {"mv_set_draw_mask", "a draw mask attached", "read none", "detach it first", "detach the mask first", "read no draw mask", MV_OPT_ON(g->drawMask.live)},
    {"mv_set_still_frames", "still frames switched on", "read no stale bytes", "switch them off first", "switch them off first", "read no stale bytes", MV_OPT_ON(g->stillOn)},
    {"mv_set_episode_budget", "an episode budget attached", "read none", "detach it first", "detach the budget first", "read no episode budget", MV_OPT_ON(g->budgetOn)},
    {"mv_set_state_obs", "state observations attached", "write none", "detach them first", "detach them first", "write no state observations", MV_OPT_ON(g->stateRows.buf)},
    {"mv_set_scene_obs", "scene observations attached", "write none", "detach them first", "detach them first", "write no scene observations", MV_OPT_ON(g->sceneRows.buf)},
    {"mv_set_depth_obs", "depth observations attached", "write none", "detach them first", "detach them first", "write no depth observations", MV_OPT_ON(g->depth.buf)},
    {"mv_set_seg_obs", "segmentation observations attached", "write none", "detach them first", "detach them first", "write no segmentation observations", MV_OPT_ON(g->seg.buf)},
    {"mv_set_normal_obs", "normal observations attached", "write none", "detach them first", "detach them first", "write no normal observations", MV_OPT_ON(g->normal.buf)},
    {"mv_set_entity_obs", "entity observations attached", "write none", "detach them first", "detach them first", "write no entity observations", MV_OPT_ON(g->entityRows.buf)},
    {"mv_set_overview", "an overview attached", "draw none", "detach it first", "detach it first", "draw no overview", MV_OPT_ON(g->overview.buf)},
};
#undef MV_OPT_ON
// The six per-tick observation streams, stated once, in the order mv_set_output_ring refuses them: the option that attaches the stream, the noun the refusal
// texts name it by and, for the three plane streams (mv_obs_planes.hip), the name of one plane; null: a row stream (mv_obs_rows.hip).  A new stream is one row
// here, one in gym_options and one descriptor in its file.
struct ObsStream {
    int opt;
    const char *noun, *plane;
};
inline constexpr ObsStream obs_streams[] = {
    {OPT_STATE_OBS, "state observations", nullptr},
    {OPT_DEPTH_OBS, "depth observations", "depth plane"},
    {OPT_SEG_OBS, "segmentation observations", "label plane"},
    {OPT_NORMAL_OBS, "normal observations", "normal plane"},
    {OPT_SCENE_OBS, "scene observations", nullptr},
    {OPT_ENTITY_OBS, "entity observations", nullptr},
};
constexpr const ObsStream &obs_stream(int opt, int i = 0) { return obs_streams[i].opt == opt ? obs_streams[i] : obs_stream(opt, i + 1); }
// a plane stream is attached: a fast pass of g is followed by the planes' launch
inline bool any_planes_on(const mv_gym *g)
{
    for (const ObsStream &s : obs_streams)
        if (s.plane && gym_options[s.opt].on(g)) return true;
    return false;
}
// What a stepping call's view of g carries of the options (the rows of the two records are fields of the per-slot views already: mv_gym::gvp); macro: the view
// belongs to a macro step's tick (mv_macro_step) and carries the envs' ticks left.  A group's members have none of them (mv_group_create).
inline void fill_view_options(GymView &v, const mv_gym *g, bool macro)
{
    v.step_mask = g->stepMask.live;
    v.draw_mask = g->drawMask.live;
    if (g->budgetOn) { v.budget = g->budgetLeft; v.halted = g->budgetHalted; }
    if (g->stillOn) v.still = g->stillStale;
    if (macro) v.macro_tl = g->macroTl;
}

// Where a tick's public outputs go: the observation slab and the reward / done arrays -- or, with mv_set_output_ring, entry (tick % count)
// of the caller's rings.  true_objective is state (only a finishing env records it, vector_env.cpp:96-101): never ringed.
// depth (mv_set_depth_obs): the entry's depth planes, null with no buffer attached.
// seg (mv_set_seg_obs), normal (mv_set_normal_obs): the entry's label planes and normal planes, likewise.
struct OutPtrs { uint32_t *obs; float *rewards; uint8_t *done; void *depth = nullptr; void *seg = nullptr; void *normal = nullptr; };
// the planes of one tick's entry and their formats, as the observation pass takes them (mv_raster.h: PlaneOuts; null: not attached)
PlaneOuts plane_outs(const mv_gym *g, const OutPtrs &o);
std::string lower(const char *s);
int check(mv_gym *g);
// what every form of a persistent attachment refuses: no gym, a closed one, a member of a group (the union launches read or write none of what opt attaches)
int attach_check(mv_gym *g, const char *who, const GymOption &opt);
int getter_check(const mv_gym *g, const char *who);   // the mv_get_* form getters: no gym, a closed one
OutPtrs outputs_of(const mv_gym *g, unsigned long long tick);
OutPtrs last_outputs(const mv_gym *g);   // of the last tick (reset / render / getters)
int refresh_mirrors(mv_gym *g);
int take_hist(mv_gym *g, hipStream_t s, bool setupClearsNext);
GymView view(const mv_gym *g, int q, const OutPtrs *direct = nullptr);   // direct: the step writes the public output arrays itself (not pipelined)
int sim_join(mv_gym *g);
int tower_join(mv_gym *g);
int tower_draw_before(mv_gym *g, hipStream_t sim);
int tower_draw_after(mv_gym *g, hipEvent_t after, int ticks);
int publish_outputs(mv_gym *g, int q, const OutPtrs &o);   // on the caller's stream
// the staged outputs of the k ticks in slots q0 .. q0 + k - 1 -> outs[j * stride], one launch on the caller's stream (calls that draw no tick, or the last)
int publish_ticks(mv_gym *g, int q0, const OutPtrs *outs, int stride, int k);
int check_status_flags(mv_gym *g);
int finish_with_warning(mv_gym *g);
int refill_episodes(mv_gym *g, int k);   // k: the ticks of the stepping call that is about to be enqueued
int read_back_status(mv_gym *g, hipEvent_t after);   // after: an event recorded behind the kernel whose status words are wanted
// the current consumed counts, not the last periodic read-back: a host wait for everything enqueued, the status words copied, no read-back pending
int sync_status_words(mv_gym *g);
int flush_device_actions(mv_gym *g);
void group_detach(mv_gym *g);   // (mv_api_step.hip)
// the episode log of g brought up to the k ticks just enqueued: views[j * stride] is tick j's view (its staged outputs); on the caller's stream (mv_episode_log.hip)
int episode_log_update(mv_gym *g, const GymView *views, int stride, int k);
int episode_log_reset(mv_gym *g);   // mv_reset: accumulators to zero, the records stay
void episode_log_free(mv_gym *g);   // mv_close
void env_masks_free(mv_gym *g);     // mv_close (mv_env_masks.hip)
void episode_budget_free(mv_gym *g);   // mv_close (mv_episode_budget.hip)
void macro_step_free(mv_gym *g);       // mv_close (mv_macro_step.hip)
// mv_still_frames.hip.  touch: every env stale -- one memset on the caller's stream, for every call that can change an env's state or what or where the gym
// draws (off: nothing).  carry: the rows of the still frames of one stepping call's n rendered ticks (views[j * stride], outs[j * stride]) from the ring
// entries that hold them, one launch on the caller's stream behind the call's passes
void still_frames_free(mv_gym *g);     // mv_close
void overview_free(mv_gym *g);         // mv_close (mv_overview.hip)
int still_frames_touch(mv_gym *g);
int still_frames_carry(mv_gym *g, const GymView *views, const OutPtrs *outs, int stride, int n);
// mv_macro_step.hip: the staged outputs of the k ticks in slots q0 .. q0 + k - 1 folded into ONE entry o -- rewards summed in tick order (mv_macro_step.h:
// macro_fold), dones OR-ed, true objectives as publish_ticks -- with one launch on the caller's stream; cont: the entry holds the fold of the call's earlier chunks
int publish_macro(mv_gym *g, int q0, const OutPtrs &o, int k, bool cont);
// mv_api_step.hip: one chunk (<= batch ticks) of a macro step of kCall ticks; quiet: QUIET_NONE / QUIET_LAST of step_gyms
int step_macro_chunk(mv_gym *g, int k, int kCall, bool draw_last, const MacroCall &mc);
// mv_obs_rows.hip.  publish: the stepping call's ONE publication launch for all three row records -- the staged rows of the k ticks in slots q0 .. q0 + k - 1 -> the
// entries of ticks tick0 .. tick0 + k - 1 of the caller's buffers, on the caller's stream; -> 1: launched, 0: no record attached.  refresh: the last tick's
// entries gathered from the current state (mask: device bytes [N], only the flagged envs' rows; null: every row; nothing attached: no launch), on the caller's
// stream behind sim_join
int obs_rows_publish(mv_gym *g, int q0, unsigned long long tick0, int k);
int obs_rows_refresh(mv_gym *g, const uint8_t *device_mask);
void obs_rows_free(mv_gym *g);         // mv_close
// mv_obs_planes.hip: the one follower behind a FAST pass of view v, whatever is attached (an exact pass stores the planes itself: launch_raster's planes
// argument) -- the depth planes (o.depth), label planes (o.seg) and normal planes (o.normal) of the frames the pass has just drawn, each where its stream
// is attached, with ONE launch on the caller's stream; -> launches made (0: nothing attached or planes null), -1
int planes_follow(mv_gym *g, const GymView &v, const OutPtrs &o, const char *who);
void obs_planes_free(mv_gym *g);       // mv_close
// What the calls that an attached stream forbids answer (mv_api.hip), each walking obs_streams and composing "<who>: <noun> are attached (<setter>), <clause>:
// detach the <noun> first" for the first stream that is on; -> -1 with that text, 0: none is.  ring_sized_attached: all six, sized by the ring count they
// were attached under.  planes_attached: the three plane streams, with the caller's clause.  still_clause: why still frames and a plane stream exclude each other
// (mv_set_still_frames; the plane setters' own refusal)
int ring_sized_attached(const mv_gym *g, const char *who);
int planes_attached(const mv_gym *g, const char *who, std::string (*clause)(const ObsStream &));
std::string still_clause(const ObsStream &s);
int render_frames(mv_gym *g);          // mv_render without the state rows' refresh (mv_api.hip; mv_reset_envs refreshes the flagged envs' rows only)
int episode_budget_seed_mirror(mv_gym *g);   // mv_set_episode_log: the log's mirror from the live array (mv_episode_budget.hip)
// mv_fork.hip, shared with mv_env_store.hip: what every fork / resample / env-store form refuses (what: "forks", "env stores": for the text about groups)
int fork_check(mv_gym *g, const void *map, const char *who, const char *what = "forks");
// mv_env_store.hip: the layout word of g's records (mv_create, once the table and the parameters are known)
uint64_t env_record_layout_word(const mv_gym *g, const std::string &scenario_name, const mv_config *cfg);
}  // namespace mvapi
