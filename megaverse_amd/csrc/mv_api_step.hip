// megaverse_amd/csrc/mv_api_step.hip -- stepping: MegaverseGym::step (megaverse.cpp:118-121 -> VectorEnv::step, vector_env.cpp:89-108) as kernel sequencing on
// two streams -- one-step-ahead pipelining, batched calls (mv_step_n: one step launch + one observation launch per call; mv_step_n_render: the same ticks with
// none of them drawn, or the last only), overlapped passes, groups of gyms stepped with union launches (mv_group_*), several gyms per call (mv_step_many) --
// and the in-stream kernel timing (mv_profile_*).  DESIGN.md 3.4, 3.6.
// A stepping call is a plan (StepCall::plan: every decision, nothing enqueued) followed by its phases, each a function of its own: step_gyms lists them.
#include "mv_api_internal.h"

namespace {

// One stepping call = k ticks (mv_step: 1; mv_step_n: up to `batch`) of n gyms that share one pair of streams (n = 1: a gym on its own;
// n > 1: an mv_group, stepped by union launches).  gs[0] is the leader: the stream state that changes with every call -- marks, which stream
// the last step ran on -- is kept on it and mirrored to the others.  policy != POLICY_NONE: tick j draws its actions inside the step kernel
// from (seed, first_index + j); POLICY_NONE: the first tick acts on what mv_set_actions* left, the following ones on cleared actions
// (env.cpp:141-142 clears them after every tick).  POLICY_SEQUENCE: tick j acts on entry (first_index + j) % count of every gym's action ring
// (mv_set_action_ring) -- to the kernels a POLICY_NONE tick with a multi-discrete pointer of its own, so every launch path the random policies open is open.
// kCall: the ticks of the CALLER's call this chunk belongs to (mv_step_n splits a call of more than `batch` ticks): what the ring contract of
// the overlapped passes is stated in (include/megaverse_hip.h).
// quiet (mv_step_n_render; one gym, render = false): QUIET_NONE: no tick of the chunk is drawn; QUIET_LAST: tick k - 1 alone is (the last chunk of an
// MV_RENDER_LAST call) -- its frame setup in the step launch, one observation launch for it.  Either way the ticks go out as ONE launch per 8 that sets no other
// frame up (launch_step_ticks_sim) wherever the rendered call has its one-launch step, and their rewards / dones / true objectives are published by ONE launch
// for the chunk (publish_ticks).  QUIET_OFF: everything as `render` says, launch for launch.
// mc (mv_macro_step; one gym, a quiet mode, POLICY_SEQUENCE): the chunk belongs to a macro step.  Every tick holds mc->actions -- to the kernels an action ring
// of count 1; the gym's own ring is not looked at -- every view carries the gym's ticks-left array, so the MASKED kernels are launched; all k ticks share ONE
// output entry, which publish_macro folds the chunk's slots into in publish_ticks' place, and the ring's position moves on by one behind the call's last chunk.
enum : int { QUIET_OFF = 0, QUIET_NONE = 1, QUIET_LAST = 2 };
struct StepRequest { bool render; int k, policy; uint32_t seed, first_index; int kCall, quiet = QUIET_OFF; const MacroCall *mc = nullptr; };

// How the chunk's ticks are launched and how its observation passes are: one function of StepCall per path, which says what it launches; plan() has the
// conditions, DESIGN.md 3.4.0 lists them.
enum StepPath : int { STEP_SINGLE, STEP_TICKS, STEP_TICKS_SIM, STEP_UNION, STEP_UNION_TICKS };
enum PassPath : int { PASS_TICK, PASS_BATCH, PASS_UNION_BATCH, PASS_QUIET };

// One stepping call: the request, the plan -- every decision taken from the request and the gyms' state -- and the phases that enqueue it (step_gyms).
struct StepCall {
    mv_gym *const *gs;        // the n gyms; L = gs[0], the leader
    mv_gym *L;
    StepRequest r;
    int n, k;
    bool mustWait = false, allFast = true, anyHostEpisodes = false, anyLog = false;   // over the gyms, as the call found them
    bool own;                 // the ticks run on the simulation stream (sim), not on the caller's
    hipStream_t sim;
    bool staged;              // the step kernels stage rewards / dones / true objectives in their slot; the caller's stream publishes them
    StepPath step;
    PassPath pass;
    bool drawLast;            // QUIET_LAST: tick k - 1 is drawn
    bool sideWaits;           // (not pipelined) a draw launch, a status read-back or an upload will wait for this call: an event behind the ticks
    bool overlap;             // the one pass launch goes to a pass stream (mv_set_pass_overlap): passOn
    bool rows, carry, depth;  // followers: the row records' publication, the still frames' carry, the depth, label and normal planes behind fast passes -- ONE launch per
                              // drawn tick for whichever of the three are attached (the log: per gym, logCapacity)
    bool timeCall, timeTicks;   // timing (mv_profile_begin): ONE entry for the whole call (callEv), or one per tick for the first tickEvs ticks (tickEv);
    hipEvent_t *callEv = nullptr, *tickEv = nullptr;   // reserve_timing takes the entries, behind the checks and the refill as always
    int tickEvs = 0;
    std::vector<GymView> views;   // [k][n] tick j's view of gym i (tick_views)
    std::vector<OutPtrs> outs;    // [k][n] ... and where its outputs go
    bool rode = false;        // the event behind the ticks was completed by the last step launch's own dispatch packet: no marker behind it
    hipStream_t passOn = nullptr;

    hipEvent_t *ev(int j) const { return j < tickEvs ? tickEv + (size_t)j * 5 : nullptr; }
    // the call's last pass completes this call's mark (what the simulation stream waits for before it reuses the slot group)
    hipEvent_t mark() const { return own ? L->userMark[L->markCount % PIPE_GROUPS] : nullptr; }
    PublishTo publish_to(size_t q) const { return PublishTo{outs[q].rewards, outs[q].done, gs[q % (size_t)n]->gv.true_objective}; }

    // ---- phase 1: the checks and the plan
    int plan(mv_gym *const *gyms, int count, const StepRequest &req)
    {
        gs = gyms; n = count; L = gs[0]; r = req; k = r.k;
        int batch = L->batch;
        for (int i = 0; i < n; ++i) {
            mv_gym *g = gs[i];
            if (check(g)) return -1;
            if (!g->wasReset) return fail("mv_step: call mv_reset first");
            batch = std::min(batch, g->batch);
            mustWait = mustWait || g->simMustWaitUser;
            allFast = allFast && g->fastPixels != 0;
            anyHostEpisodes = anyHostEpisodes || g->hostEpisodes();
            anyLog = anyLog || g->logCapacity > 0;
            if (r.policy == POLICY_SEQUENCE && !r.mc && (!g->actRing || g->actRingCount < 1))
                return fail(n > 1 ? "mv_group_step: MV_POLICY_SEQUENCE: gym " + std::to_string(i) + " of the group has no action ring (mv_set_action_ring)"
                                  : std::string("mv_step_n: MV_POLICY_SEQUENCE: the gym has no action ring (mv_set_action_ring)"));
        }
        if (k < 1 || k > batch) return fail("mv_step_n: 1 <= k <= " + std::to_string(batch) + " (MV_PIPE_BATCH) required");
        // Not pipelined (mv_set_pipelining(0)), or ONE tick whose inputs come from the caller's stream (a policy in the loop: nothing can overlap,
        // the two queue hand-overs, ~10 us each, would be pure cost): the step runs on the caller's stream like everything else.
        own = L->pipelined != 0 && !(mustWait && k == 1);
        sim = own ? L->simStream : L->stream;
        // The step kernels stage rewards / dones / true objectives in their hand-over slot and the caller's stream publishes them -- or, not pipelined, write the
        // public arrays themselves.  With an episode log (mv_set_episode_log) they always stage: the log reads every tick of the call from the slots.
        // A macro step always stages: its publication folds the slots of the call's ticks into one entry.
        staged = own || anyLog || r.mc != nullptr;
        drawLast = r.quiet == QUIET_LAST;
        // A batched call hands over ONCE: all k step kernels, then all k observation passes.  (Handing over tick by tick when the caller's stream is
        // found idle -- the first call after a synchronisation -- was built and measured on 20-step runs: 15.0-15.6 M obs/s against 16.2 M without;
        // short runs use short calls instead, bench.py's --batch.)
        // One gym, several ticks with device-drawn actions, nothing timed per tick: ONE step launch runs the k ticks of every env (MV_STEP_TICKS=0: k launches).
        static const bool ticksOff = getenv("MV_STEP_TICKS") && atoi(getenv("MV_STEP_TICKS")) == 0;
        // (every scenario with one agent per env; several agents: TowerBuilding only -- two waves per env, launch_step_ticks)
        const bool oneGymTicks = !ticksOff && n == 1 && (L->A == 1 || L->scenario == SCN_TOWER) && k >= 2 && k <= MAX_STEP_TICKS && r.policy != POLICY_NONE && !L->gv.dbg;
        // ... every tick's observations in a slab of its own (an output ring at least k deep): the observation passes of up to MAX_STEP_TICKS ticks go out as
        // ONE launch (launch_raster_batch: the next tick's expensive frames fill the tail of the previous tick's pass).
        // (the one-launch observation passes only beside the one-launch step: k separate step kernels starve beside a pass that long -- 70-190 us each, r04l)
        const bool batchRaster = oneGymTicks && r.render && allFast && L->ringObs && L->ringCount >= k;
        // timing (mv_profile_begin): a batched call that takes both one-launch paths is timed as a whole -- one entry, events around the step launch and around
        // the raster launch, k ticks -- so that the figures are those of the launches the product runs; otherwise tick by tick, which takes no one-launch path
        const bool profiling = r.render && L->profCount < L->profMax;
        timeCall = profiling && batchRaster; timeTicks = profiling && !batchRaster;
        // A group (n > 1), several rendered ticks with device-drawn actions, every member with an observation ring at least k deep and one agent per env: ONE
        // union step launch runs the k ticks of every env of every gym (step_union_ticks_kernel) and ONE launch draws their k x n observation passes
        // (raster_union_batch_kernel) -- two launches per call where the tick-by-tick path takes 2 k (BASELINE configs[4]: the scenarios of a multi-task batch).
        bool groupBatch = n > 1 && !ticksOff && own && r.render && allFast && k >= 2 && k <= MAX_STEP_TICKS && r.policy != POLICY_NONE
                && !profiling && raster_union_batch_applicable(k, n, L->w, L->h);
        // ... and all of the group's envs resident at once: the union step launch keeps a workgroup per env alive for the whole call (four waves of 168 VGPRs
        // for the long-list gyms); beyond one round of the chip the tick-by-tick launches win (Mixed 64 x 64, batched / tick by tick: 512 envs 12.2 / 8.6 M
        // obs/s, 1024: 17.6 / 16.2, 2048: 16.1 / 20.5; r08z_rules)
        int envs = 0;
        for (int i = 0; i < n; ++i) {
            groupBatch = groupBatch && gs[i]->A == 1 && gs[i]->ringObs && gs[i]->ringCount >= k && !gs[i]->gv.dbg;
            envs += gs[i]->N;
        }
        groupBatch = groupBatch && envs <= 1024;
        step = oneGymTicks && r.render && (!profiling || timeCall) ? STEP_TICKS : oneGymTicks && r.quiet != QUIET_OFF ? STEP_TICKS_SIM : n == 1 ? STEP_SINGLE
               : groupBatch ? STEP_UNION_TICKS : STEP_UNION;
        pass = batchRaster ? PASS_BATCH : groupBatch ? PASS_UNION_BATCH : r.quiet != QUIET_OFF ? PASS_QUIET : PASS_TICK;
        // not pipelined: the caller's stream needs no event behind the step launches; the side streams do when a draw launch, a status read-back or an upload
        // will wait for this call
        sideWaits = anyHostEpisodes;
        for (int i = 0; i < n; ++i)
            sideWaits = sideWaits || (gs[i]->genStream && gs[i]->ticksSinceDraw + k >= gs[i]->drawPeriod) || gs[i]->stepsSinceStatus + k >= gs[i]->statusPeriod;
        rows = n == 1 && (L->stateRows.buf != nullptr || L->sceneRows.buf != nullptr || L->entityRows.buf != nullptr);   // (a group's members have none)
        // (mv_set_still_frames with an output ring: the calls run in order -- pass c + 1 on its side stream could draw into the entry that carry c, on the
        // caller's stream, is still reading when the ring is exactly two calls deep)
        carry = n == 1 && L->stillOn && L->ringObs != nullptr && (r.render || drawLast);
        // (mv_set_depth_obs, fast pixels: one depth launch per drawn tick behind the call's passes, reading the tick's frame lists from the call's slots -- an exact
        // pass stores the planes itself, one_pass; a group's members have none)
        // (mv_set_seg_obs, mv_set_normal_obs: the same follower, which then stores every attached plane)
        depth = n == 1 && any_planes_on(L) && L->fastPixels != 0 && (r.render || drawLast);
        // overlapped passes (mv_set_pass_overlap): this call's one launch goes to an internal stream
        // (an env must not finish in two consecutive calls: their passes may publish its true objective in either order -- episodes of at least
        // baseEpisodeLen seconds, 15 ticks each)
        // The ring is two CALLS deep, in the caller's ticks per call (a call of 16 ticks runs as two chunks of 8: the second-next chunk's passes would overwrite
        // what the consumer of the previous CALL -- enqueued after both of its chunks -- may still be reading), and rewards / dones have rings of
        // their own (two passes in flight would both publish the single arrays, in either order).
        // (no depth follower either: its reads of the call's slots and the next call's reuse of them stay ordered by the mark on the caller's stream)
        overlap = pass == PASS_BATCH && own && !timeCall && !carry && !depth && L->passOverlap && L->passStream[0]
                && L->ringCount >= 2 * std::max(k, r.kCall) && L->ringRewards && L->ringDone && L->baseEpisodeLen * 15.0f > float(2 * k + 2);
        views.resize((size_t)n * k); outs.resize((size_t)n * k);
        return 0;
    }

    void reserve_timing()
    {
        hipEvent_t *first = timeCall || timeTicks ? &L->profEvents[(size_t)L->profCount * 5] : nullptr;
        if (timeCall) { callEv = first; L->profTicks[(size_t)L->profCount++] = k; }
        if (timeTicks) { tickEv = first; tickEvs = std::min(k, L->profMax - L->profCount); }
        for (int j = 0; j < tickEvs; ++j) L->profTicks[(size_t)L->profCount++] = 1;
    }

    // ---- phase 2: what the simulation stream must wait for, the action upload, TowerBuilding's draw launch, the next slot group
    int order_sim_stream()
    {
        if (own) {
            // The simulation stream may reuse a slot group once the observation passes that read it are done: the END of the call PIPE_GROUPS calls
            // ago (userMark, completed by that call's last pass).  When the caller's stream feeds the simulation (reset / render / device
            // actions / test hooks since the last step), or the last step ran there: everything enqueued on it so far.  (Both raster kernels read nothing but
            // the frame lists and headers of their tick: the simulator state may move on underneath them.)
            if (mustWait || !L->simOnOwnStream) {
                HIP_TRY(hipEventRecord(L->userNow, L->stream));
                HIP_TRY(hipStreamWaitEvent(sim, L->userNow, 0));
            } else if (L->markCount >= PIPE_GROUPS) HIP_TRY(hipStreamWaitEvent(sim, L->userMark[L->markCount % PIPE_GROUPS], 0));
        } else {
            if (L->simOnOwnStream && L->simDoneValid) HIP_TRY(hipStreamWaitEvent(sim, L->simDone, 0));   // the last step ran on the other stream
            for (int i = 0; i < n; ++i) {   // (episode uploads make the simulation stream wait)
                if (gs[i]->uploadNotOnUser && gs[i]->lastUpload) HIP_TRY(hipStreamWaitEvent(sim, gs[i]->lastUpload, 0));
                gs[i]->uploadNotOnUser = false;
            }
            L->markCount = 0;
        }
        for (int i = 0; i < n; ++i) {
            mv_gym *g = gs[i];
            if (tower_draw_before(g, sim)) return -1;
            g->simMustWaitUser = false;
            g->simOnOwnStream = own;
            g->markCount = L->markCount;
            if (g->actionsDirty) {
                const int s = g->stage;
                HIP_TRY(hipMemcpyAsync(g->gv.actions, g->hActions[s], (size_t)g->N * g->A * sizeof(int32_t), hipMemcpyHostToDevice, sim));
                HIP_TRY(hipEventRecord(g->actionsCopied[s], sim));
                g->stage = 1 - s;
                HIP_TRY(hipEventSynchronize(g->actionsCopied[g->stage]));   // long done: recorded one step ago
                std::memset(g->hActions[g->stage], 0, (size_t)g->N * g->A * sizeof(int32_t));   // actions are cleared every tick (env.cpp:141-142)
                g->actionsDirty = false;
            }
            g->group = (g->group + 1) % PIPE_GROUPS;
        }
        // (instrumented builds: MV_TICK_TIMING_SKIP=n starts the statistics after n stepping calls -- the steady state, not the first ticks of fresh episodes)
        if (L->gv.dbg) {
            static const long skip = getenv("MV_TICK_TIMING_SKIP") ? atol(getenv("MV_TICK_TIMING_SKIP")) : 0;
            if (skip > 0 && ++L->dbgCalls == skip) HIP_TRY(hipMemsetAsync(L->gv.dbg, 0, (size_t)L->N * 64 * sizeof(unsigned long long), sim));
        }
        return 0;
    }

    // ---- phase 3: the k ticks, back to back on the simulation stream.  Shared by every step path: the views and outputs of ticks j0 .. j1 - 1 of the n gyms, and
    // the cost histograms of their passes (take_hist: its memset, where one is needed, goes to the simulation stream here -- between the launches of the paths
    // that launch tick by tick, whose frame setups also clear the histogram after the one they fill).
    int tick_views(int j0, int j1)
    {
        for (int j = j0; j < j1; ++j)
            for (int i = 0; i < n; ++i) {
                mv_gym *g = gs[i];
                if (r.policy == POLICY_SEQUENCE) g->gv.sample_on = POLICY_NONE;
                else if (r.policy != POLICY_NONE) { g->gv.sample_on = r.policy; g->gv.sample_seed = r.seed; g->gv.sample_step = r.first_index + (uint32_t)j; }
                else { g->gv.sample_on = (j == 0 && g->samplePending) ? g->samplePolicy : (int)POLICY_NONE; }
                g->parity = g->group * g->batch + j;
                if ((r.render || (drawLast && j == k - 1)) && take_hist(g, sim, step == STEP_SINGLE || step == STEP_UNION)) return -1;
                OutPtrs &o = outs[(size_t)j * n + i];
                o = outputs_of(g, r.mc ? g->ringTick : g->ringTick++);   // (mv_macro_step: one entry for the whole call; the position moves on behind its last chunk)
                GymView &v = views[(size_t)j * n + i];
                v = view(g, g->parity, staged ? nullptr : &o);
                fill_view_options(v, g, r.mc != nullptr);
                if (r.mc) v.md_actions = r.mc->actions;   // (the held actions)
                else if (r.policy == POLICY_SEQUENCE)
                    v.md_actions = g->actRing + (size_t)action_ring_entry(r.first_index, j, (uint32_t)g->actRingCount) * ((size_t)g->N * g->A * 6);
                else if (j == 0 && g->gv.sample_on == POLICY_NONE) v.md_actions = g->mdActions;
                if (step == STEP_UNION_TICKS) v.lpt_no_clear = 1;   // (the passes clear their histograms themselves: mv_raster.hip, hist_done)
            }
        return 0;
    }

    int ticks_single()   // STEP_SINGLE: one gym, a launch per tick (launch_step); a quiet call's ticks with render = 0, 1 for the drawn one
    {
        for (int j = 0; j < k; ++j) {
            if (tick_views(j, j + 1)) return -1;
            hipEvent_t *e = ev(j);
            if (e) HIP_TRY(hipEventRecord(e[0], sim));
            hipEvent_t rides = j == k - 1 && !e ? (own ? L->simDone : sideWaits ? L->stepDone : nullptr) : nullptr;
            // (render = 1: the step kernel also builds the frame lists, when an observation pass follows)
            rode = launch_step(views[(size_t)j], sim, L->w, L->h, r.render || (drawLast && j == k - 1) ? 1 : 0, rides);
            ++L->launchCount[0];
            if (e) HIP_TRY(hipEventRecord(e[1], sim));
        }
        return 0;
    }

    int ticks_resident()   // STEP_TICKS: one gym, every tick rendered: ONE launch per 8 ticks, with their frame setups (launch_step_ticks)
    {
        if (tick_views(0, k)) return -1;
        for (int j = 0; j < k; ++j) views[(size_t)j].lpt_no_clear = 1;
        // (the cost histograms of the call's passes are clean: take_hist.  In the steady state of batched calls nothing is cleared here at
        // all -- every pass of the one-launch observation kernel leaves its histogram zero -- where r06l's kernel traces showed two fill
        // kernels in front of every step launch, the second one waiting 30 us for a wave slot beside the observation passes: the chain
        // of step launches is what bounds a batched call's rate at 1024 envs, 344 + 39 us per call against 288 us of passes.)
        if (callEv) HIP_TRY(hipEventRecord(callEv[0], sim));
        hipEvent_t rides = own && !callEv ? L->simDone : nullptr;
        const bool frameOrder = allFast && views[0].lpt_forder != nullptr;   // (fast pixels: the exact kernel has its own sort; MV_FRAME_ORDER=0: no table)
        for (int j0 = 0; j0 < k; j0 += 8) {   // (a launch holds the views of up to 8 ticks as its arguments, mv_types.h: StepTicksArgs8)
            const int kk = std::min(8, k - j0);
            // (with the frame-order table its kernel is the call's last on this stream: the event rides on that packet)
            launch_step_ticks(views.data() + j0, kk, sim, L->w, L->h, j0 + kk == k && !frameOrder ? rides : nullptr);
            ++L->launchCount[0];
        }
        // one frame-order table per tick, once, where every workgroup of the call's passes used to derive its frame from the tick's histogram
        // (mv_raster.h); the kernel also zeroes the histograms: the passes neither count themselves in nor clear (histClean: set where they are enqueued)
        if (frameOrder) launch_frame_order_ticks(views.data(), k, sim, rides);
        if (callEv) HIP_TRY(hipEventRecord(callEv[1], sim));
        rode = rides != nullptr;
        return 0;
    }

    int ticks_resident_sim()   // STEP_TICKS_SIM: the same shapes, no tick drawn or the last only: launches whose ticks set no frame up (launch_step_ticks_sim)
    {
        if (tick_views(0, k)) return -1;
        if (drawLast) views[(size_t)k - 1].lpt_no_clear = 1;   // (the drawn tick's pass clears its histogram itself, as behind launch_step_ticks)
        hipEvent_t rides = own ? L->simDone : nullptr;
        for (int j0 = 0; j0 < k; j0 += 8) {   // (StepTicksArgs8)
            const int kk = std::min(8, k - j0);
            const bool last = j0 + kk == k;
            launch_step_ticks_sim(views.data() + j0, kk, last && drawLast ? 1u << (kk - 1) : 0u, sim, L->w, L->h, last ? rides : nullptr);
            ++L->launchCount[0];
        }
        rode = rides != nullptr;
        return 0;
    }

    int ticks_union()   // STEP_UNION: a group, one union launch per tick (launch_step_union)
    {
        for (int j = 0; j < k; ++j) {
            if (tick_views(j, j + 1)) return -1;
            UnionStepArgs ua;
            ua.n = n;
            int envs = 0;
            for (int i = 0; i < n; ++i) { ua.first[i] = envs; ua.gv[i] = views[(size_t)j * n + i]; envs += gs[i]->N; }
            for (int i = n; i <= MAX_UNION; ++i) ua.first[i] = envs;
            hipEvent_t *e = ev(j);
            if (e) HIP_TRY(hipEventRecord(e[0], sim));
            launch_step_union(ua, sim, L->w, L->h, r.render ? 1 : 0);
            ++L->launchCount[0];
            if (e) HIP_TRY(hipEventRecord(e[1], sim));
        }
        return 0;
    }

    int ticks_union_resident()   // STEP_UNION_TICKS: one launch for the k ticks of all n gyms (pipelined only)
    {
        if (tick_views(0, k)) return -1;
        UnionTicksArgs ta;
        ta.n = n; ta.k = k; ta.act_first = r.first_index;
        int envs = 0;
        for (int i = 0; i < n; ++i) {
            mv_gym *g = gs[i];
            ta.first[i] = envs; envs += g->N;
            ta.gv[i] = views[(size_t)i];   // tick 0's
            ta.slot_stride[i] = (int64_t)((const uint8_t *)views[(size_t)n + i].vis_prims - (const uint8_t *)views[(size_t)i].vis_prims);
            const bool seq = r.policy == POLICY_SEQUENCE;   // (the kernel derives tick j's entry itself: it holds tick 0's view only)
            ta.act_base[i] = seq ? g->actRing : nullptr;
            ta.act_count[i] = seq ? (uint32_t)g->actRingCount : 0u;
            ta.act_stride[i] = g->N * g->A * 6;
        }
        for (int i = n; i <= MAX_UNION; ++i) ta.first[i] = envs;
        for (int i = n; i < MAX_UNION; ++i) {
            ta.gv[i] = views[0]; ta.slot_stride[i] = 0;
            ta.act_base[i] = nullptr; ta.act_count[i] = 0; ta.act_stride[i] = 0;
        }
        launch_step_union_ticks(ta, sim, L->w, L->h, L->simDone);
        ++L->launchCount[0];
        rode = true;
        return 0;
    }

    // ---- phase 4: the event behind the ticks, TowerBuilding's draw launch, the status read-backs.
    // ONE event behind the call's step launches -- simDone (pipelined: often completed by the last launch's own dispatch packet), else stepDone -- is what
    // the caller's stream, the episode draws / uploads and the status read-backs wait for.  (There used to be up to 2 + n event records here -- simDone,
    // stepDone, TowerBuilding's stepForDraw, a resetDone per member whose status was due; every one is a marker packet the simulation queue works off before
    // it reaches the NEXT call's step launch, while that call's observation launch -- one wait on the caller's queue -- was already taking the chip: a step
    // launch that starts behind the observation launch it runs beside waits for that launch's workgroups to drain, r08q timeline.)
    int behind_ticks()
    {
        hipEvent_t after = own ? L->simDone : sideWaits ? L->stepDone : nullptr;
        if (after && !rode) HIP_TRY(hipEventRecord(after, sim));
        for (int i = 0; i < n; ++i)
            if (tower_draw_after(gs[i], after, k)) return -1;
        // (every step kernel regenerates / swaps the next episode into the envs it finishes)
        // An env needs a fresh resident episode only at its NEXT reset, normally hundreds of steps away, and two are resident: the status
        // words are read back -- and the refill considered -- every statusPeriod-th step (16; 1 when episodes can be a few ticks long).
        for (int i = 0; i < n; ++i) {
            mv_gym *g = gs[i];
            g->samplePending = false;
            g->mdActions = nullptr;
            if (own) g->simDoneValid = true;
            if (after) g->lastStep = after;   // (uploads never overlap a kernel that may read the ring: refill_episodes; host-generated scenarios always have one)
            g->stepsSinceStatus += k;
            if (g->stepsSinceStatus >= g->statusPeriod) {   // (TowerBuilding: the error flags)
                if (read_back_status(g, after)) return -1;
                g->stepsSinceStatus = 0;
            }
            g->mirrorsFresh = false;
        }
        return 0;
    }

    // ---- phase 5: the caller's stream.  First it waits for the ticks, and the pass stream of an overlapped call is ordered ...
    int order_user_stream()
    {
        // (before this call enqueues anything there)
        if (L->passOverlap && L->callStart[0]) HIP_TRY(hipEventRecord(L->callStart[(int)(L->overlapCalls & 1ull)], L->stream));
        if (own) HIP_TRY(hipStreamWaitEvent(L->stream, L->simDone, 0));
        passOn = L->stream;
        if (overlap) {
            const int me = (int)(L->overlapCalls & 1ull);
            passOn = L->passStream[me];
            HIP_TRY(hipStreamWaitEvent(passOn, L->simDone, 0));                                      // this call's ticks
            if (L->overlapCalls >= 1) HIP_TRY(hipStreamWaitEvent(passOn, L->callStart[1 - me], 0));   // what the caller had enqueued when the previous call began
            // (first overlapped call: everything so far)
            else { HIP_TRY(hipEventRecord(L->userNow, L->stream)); HIP_TRY(hipStreamWaitEvent(passOn, L->userNow, 0)); }
        }
        return 0;
    }

    // ... then publication and passes, by pass path.  One gym's pass of one tick, its lists set up inside the step launch (a fast pass whose view says
    // lpt_no_clear leaves its cost histogram zero: self_clear, mv_raster.hip):
    // (mv_set_depth_obs: an EXACT pass stores the tick's depth planes itself -- planes: OutPtrs::depth of the tick; a fast pass gets none, followers_and_mark)
    // (mv_set_seg_obs, mv_set_normal_obs: and its label and normal planes -- planes: the tick's OutPtrs, whose plane entries go with it)
    int one_pass(mv_gym *g, const GymView &v, uint32_t *obs, hipEvent_t between, const PublishTo *pub, hipEvent_t done, const char *who, const OutPtrs *planes = nullptr)
    {
        const PlaneOuts po = planes ? plane_outs(g, *planes) : PlaneOuts();
        if (launch_raster(v, obs, L->w, L->h, L->stream, between, g->fastPixels, /*setup_done=*/1, pub, done, g->fastPixels ? nullptr : &po))
            return fail(std::string(who) + ": observation size above 1024x1024");
        ++L->launchCount[1];
        if (v.lpt_no_clear && g->fastPixels) g->histClean[(size_t)v.lpt_parity] = 1;
        return 0;
    }

    int passes_tick()   // PASS_TICK: tick by tick: the outputs the passes do not publish themselves, then the tick's passes (render = 0: none)
    {
        const bool pubInRaster = staged && allFast;   // (the fast observation pass publishes with its first workgroups)
        PublishTo pubs[MAX_UNION];
        uint32_t *obsPtrs[MAX_UNION];
        for (int j = 0; j < k; ++j) {
            hipEvent_t *e = ev(j);
            if (e) HIP_TRY(hipEventRecord(e[2], L->stream));
            const GymView *vj = views.data() + (size_t)j * n;
            for (int i = 0; i < n; ++i) {
                const OutPtrs &o = outs[(size_t)j * n + i];
                pubs[i] = publish_to((size_t)j * n + i);
                obsPtrs[i] = o.obs;
                if (staged && (!r.render || !allFast) && publish_outputs(gs[i], gs[i]->group * gs[i]->batch + j, o)) return -1;
            }
            hipEvent_t done = j == k - 1 ? mark() : nullptr;
            if (!r.render) { if (done) HIP_TRY(hipEventRecord(done, L->stream)); }
            else if (n > 1 && allFast) {
                if (launch_raster_union(vj, obsPtrs, pubInRaster ? pubs : nullptr, n, L->w, L->h, L->stream, e ? e[3] : nullptr, done))
                    return fail("mv_step: observation size above 1024x1024");
                ++L->launchCount[1];
            } else
                for (int i = 0; i < n; ++i)
                    if (one_pass(gs[i], vj[i], obsPtrs[i], e && i == 0 ? e[3] : nullptr, pubInRaster ? &pubs[i] : nullptr, i == n - 1 ? done : nullptr, "mv_step",
                                 &outs[(size_t)j * n + i])) return -1;
            if (e) HIP_TRY(hipEventRecord(e[4], L->stream));
        }
        return 0;
    }

    int passes_batch()   // PASS_BATCH: one gym; the ticks go out chunkMax at a time (one chunk unless MV_RASTER_BATCH says otherwise; 0: off, launch_raster_batch declines)
    {
        static const int chunkMax = getenv("MV_RASTER_BATCH") ? std::min((int)MAX_STEP_TICKS, std::max(1, atoi(getenv("MV_RASTER_BATCH")))) : (int)MAX_STEP_TICKS;
        static_assert(MAX_STEP_TICKS <= PIPE_BATCH_MAX, "a chunk's pointers");
        PublishTo pubs[PIPE_BATCH_MAX];
        uint32_t *obs[PIPE_BATCH_MAX];
        for (int first = 0; first < k; first += chunkMax) {
            const int cn = std::min(chunkMax, k - first);
            const GymView *v = views.data() + first;
            for (int q = 0; q < cn; ++q) { pubs[q] = publish_to((size_t)first + q); obs[q] = outs[(size_t)first + q].obs; }
            hipEvent_t done = first + cn == k ? mark() : nullptr;
            const bool over = overlap && cn == k;
            if (callEv) { HIP_TRY(hipEventRecord(callEv[2], L->stream)); HIP_TRY(hipEventRecord(callEv[3], L->stream)); }
            const int rc = cn >= 2 ? launch_raster_batch(v, obs, staged ? pubs : nullptr, cn, L->w, L->h, over ? passOn : L->stream, done) : 1;
            if (rc < 0) return fail("mv_step: observation size above 1024x1024");
            if (rc == 0) {
                ++L->launchCount[1];
                if (over) HIP_TRY(hipStreamWaitEvent(L->stream, done, 0));   // the caller's stream sees the call's outputs as always
                for (int q = 0; q < cn; ++q) L->histClean[(size_t)v[q].lpt_parity] = 1;   // (every pass of the one-launch kernel leaves its cost histogram zero)
            } else   // (not applicable to this gym -- long lists -- or a chunk of one tick: tick by tick; PASS_BATCH means fast pixels, so one_pass draws with fast = 1)
                for (int q = 0; q < cn; ++q)
                    if (one_pass(L, v[q], obs[q], nullptr, staged ? &pubs[q] : nullptr, q == cn - 1 ? done : nullptr, "mv_step")) return -1;
            if (callEv) HIP_TRY(hipEventRecord(callEv[4], L->stream));
        }
        return 0;
    }

    int passes_union_batch()   // PASS_UNION_BATCH: the k x n observation passes of the call with one launch
    {
        const size_t total = (size_t)n * k;
        std::vector<PublishTo> allPubs(total);
        std::vector<uint32_t *> allObs(total);
        for (size_t q = 0; q < total; ++q) { allPubs[q] = publish_to(q); allObs[q] = outs[q].obs; }
        const int rc = launch_raster_union_batch(views.data(), allObs.data(), allPubs.data(), k, n, L->w, L->h, L->stream, mark());
        if (rc != 0) return fail(rc == -2 ? "mv_group_step: the hand-over slots of a batched call are not one slot apart (internal)"
            : "mv_group_step: observation size above 1024x1024");
        ++L->launchCount[1];
        for (size_t q = 0; q < total; ++q) gs[q % (size_t)n]->histClean[(size_t)views[q].lpt_parity] = 1;   // (every pass leaves its cost histogram zero)
        return 0;
    }

    // PASS_QUIET (one gym): no tick drawn, or the last only -- the chunk's staged outputs with one launch, in front of the drawn tick's pass, which publishes
    // nothing (mv_macro_step: folded into the call's one entry)
    int passes_quiet()
    {
        const int q0 = L->group * L->batch;
        if (staged && (r.mc ? publish_macro(L, q0, outs[0], k, !r.mc->first) : publish_ticks(L, q0, outs.data(), n, k))) return -1;
        if (drawLast) return one_pass(L, views[(size_t)k - 1], outs[(size_t)k - 1].obs, nullptr, nullptr, mark(), "mv_step_n_render", &outs[(size_t)k - 1]);
        if (own) HIP_TRY(hipEventRecord(mark(), L->stream));
        return 0;
    }

    // ---- phase 6: what follows the passes on the caller's stream, and the call's mark.  Every follower reads the call's slots, so the mark that lets the
    // simulation stream reuse them is recorded again behind them (with overlapped passes the mark was completed on the pass stream, and the slot group could be
    // reused under a follower's copy).
    int followers_and_mark()
    {
        const MacroCall *mc = r.mc;
        for (int i = 0; i < n; ++i) {   // the episode logs: one launch per gym for the call's k ticks
            if (gs[i]->logCapacity > 0 && episode_log_update(gs[i], views.data() + i, n, k)) return -1;
            gs[i]->ticksSinceReset += (uint32_t)k;
        }
        // the row records (mv_set_state_obs, mv_set_scene_obs, mv_set_entity_obs): ONE launch for the call's k ticks and all attached records, staged rows -> the caller's buffers; every
        // stepping call stages and publishes this way, pipelined or not.  It is counted with the call's pass launches (mv_debug_launch_counts).
        // (mv_macro_step: one entry per call -- the rows behind the call's last tick, with its last chunk)
        if (rows && (!mc || mc->last)) {
            const int q0 = L->group * L->batch;
            const int rc = mc ? obs_rows_publish(L, q0 + k - 1, L->ringTick, 1) : obs_rows_publish(L, q0, L->ringTick - (unsigned)k, k);
            if (rc < 0) return -1;
            L->launchCount[1] += rc;
        }
        // the still frames' carry (mv_set_still_frames, an output ring): one launch for the call's rendered ticks, behind their passes -- it reads the
        // verdicts from the call's slots
        if (carry) {
            const int first = r.render ? 0 : k - 1;   // (MV_RENDER_LAST, a macro step: the one rendered tick)
            if (still_frames_carry(L, views.data() + first, outs.data() + first, 1, k - first)) return -1;
            ++L->launchCount[1];
        }
        // the depth planes behind fast passes (mv_set_depth_obs): one launch per drawn tick, the exact trace without the shading over the tick's frame lists in
        // the call's slots, into the entry the tick's frames went to
        if (depth)
            for (int j = r.render ? 0 : k - 1; j < k; ++j) {
                const int rc = planes_follow(L, views[(size_t)j], outs[(size_t)j], "mv_step");
                if (rc < 0) return -1;
                L->launchCount[1] += rc;
            }
        if (mc && mc->last) ++L->ringTick;
        if ((anyLog || rows || carry || depth) && own) HIP_TRY(hipEventRecord(mark(), L->stream));
        if (own) {
            ++L->markCount;
            for (int i = 0; i < n; ++i) gs[i]->markCount = L->markCount;
        }
        L->overlapCalls = overlap ? L->overlapCalls + 1 : 0;
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- phase 7: the soft conditions the gyms collected (capacity flags): returned as 1 with their texts, not as an error
    int collect_warnings()
    {
        int rc = 0;
        std::string text;
        for (int i = 0; i < n; ++i)
            if (!gs[i]->warning.empty()) {
                text += (text.empty() ? "" : " | ") + (n > 1 ? "gym " + std::to_string(i) + ": " : std::string()) + gs[i]->warning;
                gs[i]->warning.clear();
                rc = 1;
            }
        if (rc) g_err = text;
        return rc;
    }
};

int (StepCall::*const STEP_PATHS[])() = {&StepCall::ticks_single, &StepCall::ticks_resident, &StepCall::ticks_resident_sim, &StepCall::ticks_union,
                                         &StepCall::ticks_union_resident};   // by StepPath
int (StepCall::*const PASS_PATHS[])() = {&StepCall::passes_tick, &StepCall::passes_batch, &StepCall::passes_union_batch, &StepCall::passes_quiet};   // by PassPath

int step_gyms(mv_gym *const *gs, int n, const StepRequest &r)
{
    StepCall c;
    if (c.plan(gs, n, r)) return -1;                        // 1. the checks, the plan ...
    HIP_TRY(hipSetDevice(c.L->device));
    for (int i = 0; i < n; ++i)
        if (refill_episodes(gs[i], r.k) < 0) return -1;     //    ... and the episodes the ticks may need
    c.reserve_timing();
    if (c.order_sim_stream()) return -1;                    // 2.
    if ((c.*STEP_PATHS[c.step])()) return -1;               // 3.
    if (c.behind_ticks() || c.order_user_stream()) return -1;   // 4., 5. ...
    if ((c.*PASS_PATHS[c.pass])()) return -1;               //    ... the passes
    if (c.followers_and_mark()) return -1;                  // 6.
    return c.collect_warnings();                            // 7.
}

int step_impl(mv_gym *g, bool render, int k, int policy, uint32_t seed, uint32_t first_index, int kCall = 0, int quiet = QUIET_OFF)
{
    if (g && g->inGroup) return fail("this gym belongs to an mv_group: step the group (mv_group_step)");
    return step_gyms(&g, 1, StepRequest{render, k, policy, seed, first_index, kCall > 0 ? kCall : k, quiet, nullptr});
}

}  // namespace

extern "C" {

int mv_step(mv_gym *g) { return step_impl(g, true, 1, POLICY_NONE, 0, 0); }
int mv_step_no_render(mv_gym *g) { return step_impl(g, false, 1, POLICY_NONE, 0, 0); }

int mv_step_n(mv_gym *g, int32_t k, int32_t policy, uint32_t seed, uint32_t first_step_index)
{
    return mv_step_n_render(g, k, policy, seed, first_step_index, MV_RENDER_EVERY);
}

int mv_step_n_render(mv_gym *g, int32_t k, int32_t policy, uint32_t seed, uint32_t first_step_index, int32_t render_mode)
{
    const bool every = render_mode == MV_RENDER_EVERY;
    const char *const me = every ? "mv_step_n" : "mv_step_n_render";   // (MV_RENDER_EVERY is mv_step_n, its texts included)
    if (check(g)) { if (!every) g_err = "mv_step_n_render: " + g_err; return -1; }
    if (render_mode != MV_RENDER_EVERY && render_mode != MV_RENDER_LAST && render_mode != MV_RENDER_NONE)
        return fail("mv_step_n_render: unknown render mode (MV_RENDER_EVERY, MV_RENDER_LAST, MV_RENDER_NONE)");
    if (policy < MV_POLICY_NONE || policy > MV_POLICY_SEQUENCE) return fail(std::string(me) + ": unknown policy");
    if (k < 1) return fail(std::string(me) + ": k >= 1 required");
    if (!every) {
        if (g->inGroup) return fail("mv_step_n_render: this gym belongs to an mv_group: step the group (mv_group_step keeps its own render flag)");
        if (!g->wasReset) return fail("mv_step_n_render: call mv_reset first");
    }
    int rc = 0;
    // Episodes that can end within a few ticks (statusPeriod 1: the refill protocol looks at the consumed counts after every tick) are
    // stepped one tick per call; otherwise `batch` ticks at a time.
    const int chunk = g->statusPeriod <= 1 ? 1 : g->batch;
    for (int done = 0; done < k; done += chunk) {
        const int n = std::min(chunk, k - done);
        // (MV_RENDER_LAST: tick k - 1 of the whole call is the one drawn -- the last tick of the last chunk)
        const int quiet = every ? QUIET_OFF : render_mode == MV_RENDER_LAST && done + n == k ? QUIET_LAST : QUIET_NONE;
        const int r = step_impl(g, every, n, policy, seed, first_step_index + (uint32_t)done, k, quiet);
        if (r < 0) { if (!every && g_err.compare(0, 17, "mv_step_n_render:") != 0) g_err = "mv_step_n_render: " + g_err; return -1; }
        if (r > 0) { g->warning += (g->warning.empty() ? "" : " | ") + g_err; rc = 1; }   // (every chunk's warning text is kept)
    }
    if (rc) { g_err = g->warning; g->warning.clear(); }
    return rc;
}

// ---- groups: several gyms of one job stepped with union launches (mv_step_union.hip, mv_raster.hip: launch_raster_union)
}  // extern "C"
// mv_macro_step (mv_macro_step.hip): one chunk of its ticks.  The episode log's update finds the chunk through the gym (mv_episode_log.hip).
int mvapi::step_macro_chunk(mv_gym *g, int k, int kCall, bool draw_last, const MacroCall &mc)
{
    g->macroCall = &mc;
    const int r = step_gyms(&g, 1, StepRequest{false, k, POLICY_SEQUENCE, 0, 0, kCall, draw_last ? QUIET_LAST : QUIET_NONE, &mc});
    g->macroCall = nullptr;
    return r;
}
void mvapi::group_detach(mv_gym *g)
{   // back to the gym's own simulation stream and events (they were kept aside while it was a member)
    if (!g->inGroup) return;
    mv_group *grp = g->inGroup;
    for (mv_gym *m : grp->gyms) {
        if (m != grp->gyms[0]) {
            m->simStream = m->ownSimStream; m->simDone = m->ownSimDone; m->stepDone = m->ownStepDone;
            for (int q = 0; q < PIPE_GROUPS; ++q) m->userMark[q] = m->ownUserMark[q];
            if (m->ownCopyStream) {
                (void)hipStreamSynchronize(m->copyStream);   // (the leader's: this member's uploads and read-backs are on it)
                if (m->genStream) m->genStream = m->ownCopyStream;
                m->copyStream = m->ownCopyStream; m->ownCopyStream = nullptr;
            }
        }
        m->inGroup = nullptr;
        m->simMustWaitUser = true; m->simOnOwnStream = false; m->simDoneValid = false; m->lastStep = nullptr; m->markCount = 0;
    }
    grp->gyms.clear();   // (the handle stays valid until mv_group_destroy; stepping it is an error from now on)
}
extern "C" {

int mv_group_create(mv_gym *const *gyms, int32_t n, mv_group **out)
{
    if (!gyms || !out || n < 1 || n > MAX_UNION) return fail("mv_group_create: 1 <= n <= 8 gyms required");
    *out = nullptr;
    mv_gym *L = gyms[0];
    for (int i = 0; i < n; ++i) {
        mv_gym *g = gyms[i];
        if (check(g)) return -1;
        if (g->inGroup) return fail("mv_group_create: a gym already belongs to a group");
        for (const GymOption &o : gym_options)
            if (o.on(g)) return fail(std::string("mv_group_create: a gym has ") + o.has + " (" + o.setter + "): the union launches " + o.unionNone + "; " + o.detach);
        for (int j = 0; j < i; ++j) if (gyms[j] == g) return fail("mv_group_create: the same gym twice");
        if (!scenario_row(g->scenario).in_union)   // (its tick is not in the union kernels, mv_step_union.hip: tick_any)
            return fail(std::string("mv_group_create: ") + scenario_row(g->scenario).name
                        + " cannot be stepped in a group of gyms; step it as a gym of its own (MultiTaskGym: MV_MULTITASK_UNION=0)");
        if (g->device != L->device || g->w != L->w || g->h != L->h || g->A != L->A || g->stream != L->stream || g->pipelined != L->pipelined)
            return fail("mv_group_create: the gyms of a group share device, observation size, agents per env, stream (mv_set_stream first) and pipelining");
        if (g->obsLayout != L->obsLayout) return fail("mv_group_create: the gyms of a group share their observation layout (mv_set_obs_layout)");
    }
    HIP_TRY(hipSetDevice(L->device));
    for (int i = 0; i < n; ++i) {   // nothing in flight on the streams a member is about to leave
        HIP_TRY(hipStreamSynchronize(gyms[i]->simStream));
        HIP_TRY(hipStreamSynchronize(gyms[i]->stream));
        if (gyms[i]->copyStream) HIP_TRY(hipStreamSynchronize(gyms[i]->copyStream));
    }
    mv_group *grp = new mv_group();
    grp->gyms.assign(gyms, gyms + n);
    for (int i = 0; i < n; ++i) {
        mv_gym *g = gyms[i];
        g->inGroup = grp;
        if (i > 0) {
            g->ownSimStream = g->simStream; g->ownSimDone = g->simDone; g->ownStepDone = g->stepDone;
            g->simStream = L->simStream; g->simDone = L->simDone; g->stepDone = L->stepDone;
            for (int q = 0; q < PIPE_GROUPS; ++q) { g->ownUserMark[q] = g->userMark[q]; g->userMark[q] = L->userMark[q]; }
            // ONE copy stream for the group's status read-backs and episode uploads.  A device has four hardware queues and HIP deals its streams over
            // them: with a copy stream per member some of them shared a queue with the caller's stream or the simulation stream, and a read-back that
            // waits there for the step launch holds up the observation launch queued behind it (60-180 us gaps every other call in the traces of r08k;
            // Mixed 64 x 64, a copy stream per member / one for the group: 14.1 / 17.3 M obs/s, r08r).
            if (L->copyStream && g->copyStream) {
                g->ownCopyStream = g->copyStream; g->copyStream = L->copyStream;
                if (g->genStream) g->genStream = g->copyStream;
            }
        }
        g->simMustWaitUser = true; g->simOnOwnStream = false; g->simDoneValid = false; g->lastStep = nullptr; g->markCount = 0;
    }
    *out = grp;
    return 0;
}

int mv_group_destroy(mv_group *grp)
{
    if (!grp) return 0;
    if (!grp->gyms.empty()) {
        mv_gym *L = grp->gyms[0];
        (void)hipSetDevice(L->device);
        (void)hipStreamSynchronize(L->simStream);
        (void)hipStreamSynchronize(L->stream);
        group_detach(L);
    }
    delete grp;
    return 0;
}

int mv_group_step(mv_group *grp, int32_t k, int32_t render, int32_t policy, uint32_t seed, uint32_t first_step_index)
{
    if (!grp || grp->gyms.empty()) return fail("mv_group_step: the group is gone (a member was closed)");
    if (policy < MV_POLICY_NONE || policy > MV_POLICY_SEQUENCE) return fail("mv_group_step: unknown policy");
    if (k < 1) return fail("mv_group_step: k >= 1 required");
    // A call's chunks: what every member's slot groups hold, and at most MAX_GROUP_TICKS -- the two-launch batched path's limit
    // (raster_union_batch_applicable): a chunk
    // of 9..16 ticks would fall back to two launches per TICK.
    int chunk = (int)MAX_GROUP_TICKS;
    for (mv_gym *g : grp->gyms) chunk = std::min(chunk, g->batch);
    for (mv_gym *g : grp->gyms)
        if (!g->closed && g->statusPeriod <= 1) chunk = 1;   // (episodes of a few ticks: the refill protocol looks at the consumed counts after every tick)
    int rc = 0;
    std::string text;
    for (int done = 0; done < k; done += chunk) {
        const int r = step_gyms(grp->gyms.data(), (int)grp->gyms.size(),
                                StepRequest{render != 0, std::min(chunk, k - done), policy, seed, first_step_index + (uint32_t)done, k});
        if (r < 0) return -1;
        if (r > 0) { text += (text.empty() ? "" : " | ") + g_err; rc = 1; }
    }
    if (rc) g_err = text;
    return rc;
}

// the measured rules bench.py used to carry (r08p / r08y: 16 against 8 ticks per call, M obs/s: TowerBuilding 1024 envs 28.5 / 26.8, ObstaclesHard 1024 24.5 /
// 22.7, Rearrange 23.7 / 21.5,
// Collect 15.0 / 14.5; 512 envs 16.2 / 19.3, ObstaclesHard 512 13.2 / 18.8, Sokoban 19.9 / 25.9, 512 envs x 4 agents 19.5 / 26.0, 4096 envs 28.4 / 30.5;
// overlap r07a/b/j)
int mv_recommended_ticks_per_call(const mv_gym *g)
{
    if (!g || g->closed) return 1;
    if (g->statusPeriod <= 1) return 1;
    const int frames = g->N * g->A;
    int k = frames >= 1024 && frames < 2048 && g->scenario != SCN_SOKOBAN ? 16 : 8;
    if (g->inGroup) k = std::min(k, (int)MAX_GROUP_TICKS);
    return std::max(1, std::min(k, g->batch));
}

int mv_host_generator_threads(const mv_gym *g)
{
    if (!g || g->closed) return -1;
    return g->feeder && !g->feeder->device_gen() ? g->feeder->num_threads() : 0;
}

int mv_recommended_pass_overlap(const mv_gym *g)
{
    if (!g || g->closed || g->inGroup) return 0;
    if (g->statusPeriod <= 1) return 0;   // (episodes of a few ticks: stepped tick by tick, and two passes in flight may not both publish an env's true objective)
    // Measured on / off, M obs/s (r10za, r10zb, r10zc; the Obstacles family and Sokoban: r07j): wherever the passes are what a call waits for, the next call's
    // begin in the tail of this one's -- Rearrange 25.6 -> 28.6, HexMemory 9.5 -> 9.8, HexExplore 10.8 -> 11.0, Collect 16.6 -> 16.9; TowerBuilding 512 envs 25.4 ->
    // 26.9, 1024: 32.5 -> 34.4, 2048: 33.7 -> 35.0, 4096: 34.9 -> 35.6, 512 x 2 agents 22.1 -> 23.7 -- but 256 envs 17.1 -> 16.6 and 512 x 4 agents 28.8 -> 24.5
    // (their step launches, not their passes, bound them), Empty 46.9 -> 46.3.
    if (g->scenario == SCN_EMPTY) return 0;
    if (g->scenario == SCN_TOWER) return g->A <= 2 && g->N * g->A >= 512 ? 1 : 0;
    return 1;
}

int mv_device_generator(const mv_gym *g)
{
    if (!g || g->closed) return -1;
    return !g->feeder || g->feeder->device_gen() ? 1 : 0;   // (no feeder: TowerBuilding, drawn by tower_draw_kernel)
}

int64_t mv_arena_bytes(const mv_gym *g) { return g ? (int64_t)(g->arenaBytes + g->logBytes + g->resampleBytes + g->stepMask.ownedBytes + g->drawMask.ownedBytes + g->budgetBytes + g->macroBytes + g->stillBytes + g->sceneRows.stageBytes + g->entityRows.stageBytes + g->overview.layout.bytes + g->overview.ownedBytes) : 0; }

int mv_step_many(mv_gym *const *gyms, int32_t n, int32_t render, int32_t sample, uint32_t seed, uint32_t step_index)
{   // several gyms of one job (MultiTaskGym: one per scenario, one stream each) stepped by one call: at eight sub-gyms the per-call cost of
    // the language binding is a third of the step.  EVERY gym is stepped, whatever another one reports: a failure (or a warning) is
    // collected and returned after the loop, so the sub-gyms never get out of step with each other.
    if (!gyms || n < 0) return fail("mv_step_many: bad arguments");
    int rc = 0;
    std::string msgs;
    for (const GymOption &o : gym_options)   // (refused before any gym is stepped: the sub-gyms never get out of step with each other)
        for (int i = 0; i < n; ++i)
            if (gyms[i] && !gyms[i]->closed && o.on(gyms[i]))
                return fail("mv_step_many: gym " + std::to_string(i) + " has " + o.has + " (" + o.setter + "): step it on its own, or " + o.detachMany);
    for (int i = 0; i < n; ++i) {
        int r = sample ? mv_sample_random_actions(gyms[i], seed, step_index) : 0;
        if (r == 0) r = step_impl(gyms[i], render != 0, 1, POLICY_NONE, 0, 0);
        if (r != 0) {
            msgs += (msgs.empty() ? "gym " : " | gym ") + std::to_string(i) + ": " + g_err;
            if (r < 0 || rc == 0) rc = r < 0 ? -1 : 1;
        }
    }
    if (rc) g_err = msgs;
    return rc;
}

int mv_profile_begin(mv_gym *g, int32_t max_steps)
{
    if (check(g)) return -1;
    if (max_steps < 0) return fail("mv_profile_begin: max_steps < 0");
    HIP_TRY(hipSetDevice(g->device));
    while ((int)g->profEvents.size() < max_steps * 5) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        g->profEvents.push_back(e);
    }
    g->profTicks.assign((size_t)max_steps, 1);
    g->profMax = max_steps;
    g->profCount = 0;
    return 0;
}

int mv_profile_end(mv_gym *g, float *avg_ms4, int32_t *counts4)
{
    if (check(g)) return -1;
    HIP_TRY(hipStreamSynchronize(g->simStream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    // every interval lies on ONE stream: [0] step kernel = events 0 -> 1 (the stream the step ran on); [2] publish / frame sort = 2 -> 3 and
    // [3] raster = 3 -> 4 (the caller's stream).  [1] (the old status read-back gap) is gone: it spanned two streams when pipelined.
    double sum[4] = {0, 0, 0, 0};
    static const int FROM[4] = {0, -1, 2, 3};
    for (int i = 0; i < g->profCount; ++i)
        for (int k = 0; k < 4; ++k) {
            if (FROM[k] < 0) continue;
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, g->profEvents[(size_t)i * 5 + FROM[k]], g->profEvents[(size_t)i * 5 + FROM[k] + 1]));
            sum[k] += ms;
        }
    int ticks = 0;   // (an entry of a batched call covers its k ticks: the averages are per tick)
    for (int i = 0; i < g->profCount; ++i) ticks += g->profTicks[(size_t)i];
    for (int k = 0; k < 4; ++k) {
        avg_ms4[k] = ticks ? (float)(sum[k] / ticks) : 0.0f;
        counts4[k] = ticks;
    }
    g->profMax = 0;
    g->profCount = 0;
    return 0;
}

}  // extern "C"
