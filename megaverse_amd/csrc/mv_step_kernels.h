// megaverse_amd/csrc/mv_step_kernels.h -- the bodies of the step and reset kernels, shared by every scenario.
// A scenario's tick lives in its mv_tick_<scenario>.h, together with a small trait S the bodies are instantiated on:
//   S::tick<A_MAX>(gv, env[, pipe_wait])   the tick (pipe_wait: scenarios with a software-pipelined kernel only)
//   S::swap_in(gv, env, force_all)         the episode swap-in of a finished (or forced) env
//   S::long_lists                          frame lists long enough for the depth sort (mv_frame.h: DepthSortScratch)
//   S::par_agents                          several agents: every wave of the workgroup takes part in the tick (TowerBuilding)
// No tick knows about step masks (mv_set_step_mask) or episode budgets (mv_set_episode_budget): the MASKED instantiations of the bodies choose between
// S::tick and frozen_tick, below.  They also choose between frame_setup_body and frame_skip (mv_frame.h) for the envs a draw mask (mv_set_draw_mask) leaves out
// and for the envs that did not change since their frames were drawn last (mv_set_still_frames: env_stale),
// and store the agents' state rows behind every tick of a view that carries staging rows for them (mv_set_state_obs: state_obs_write), and the env's scene
// row likewise (mv_set_scene_obs: scene_obs_write), and the env's entity rows (mv_set_entity_obs: entity_obs_write).
// Every __global__ is a one-line entry point over a body in its scenario's mv_step_<scenario>.hip (a launch bound that depends on a template
// parameter is not applied, and the profiles name the kernels); StepKernels lists them for the launchers (mv_step.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "mv_entity_obs.h"
#include "mv_episode_budget.h"
#include "mv_frame.h"
#include "mv_macro_step.h"
#include "mv_scene_obs.h"
#include "mv_state_obs.h"
#include "mv_still_frames.h"
#include "mv_types.h"

// the register budget of the one-wave-per-env multi-tick kernels (512 / n VGPRs).  Their waves stay resident for a whole batched call beside the
// observation passes, and what they hold the passes cannot have: left to itself hipcc takes 236 VGPRs for the TowerBuilding tick (launch bound 64:
// nothing asks it to be frugal), the one-launch-per-tick kernel does the same work in 97.
#ifndef MV_STEP_TICKS_WAVES_PER_SIMD
#define MV_STEP_TICKS_WAVES_PER_SIMD 4
#endif

namespace mv {

// the depth sort's LDS (N per workgroup), declared only in the instantiations of scenarios with long lists: LDS size sets occupancy
template <class S, int N>
__device__ __forceinline__ DepthSortScratch *depth_sort_scratch(int i)
{
    if constexpr (S::long_lists) {
        __shared__ DepthSortScratch s_ds[N];
        return &s_ds[i];
    } else {
        return nullptr;
    }
}

// ---- mv_set_step_mask: frozen envs.  Whether the mask lets env step in the ticks of this launch: its mask byte, loaded once and made uniform (as
// reset_masked_body's).  The env is the workgroup, so every wave of it takes the same side of a choice and every barrier stays workgroup-uniform.  Every view
// of a multi-tick launch carries the same mask (mv_api_step.hip; the buffer does not change while a call that reads it is in flight: include/megaverse_hip.h),
// so the BYTE is asked once per launch, through the first view.  The choice between the scenario's tick and frozen_tick is made per tick (env_left, below:
// mask and episode budget decide together); an env the mask freezes takes the frozen side on every tick of the launch.
// Every body has a template parameter MASKED, and every step kernel two instantiations: the one a gym without mask or budget launches (MASKED = false)
// contains no line of this -- it is the kernel it was, instruction for instruction -- and the one the launchers pick when the view carries a mask or a budget
// (mv_step.hip: kernels_of).  profiles/step_mask_resources.txt and profiles/episode_budget_resources.txt have both instantiations' registers, scratch and LDS.
__device__ __forceinline__ bool env_frozen(const GymView &gv, int env)
{
    return gv.step_mask != nullptr && __builtin_amdgcn_readfirstlane((int)gv.step_mask[env]) == 0;
}

// The tick of a frozen env, for every scenario: what a tick stages for its consumers says "nothing happened" -- the A rewards +0.0f, done 0 -- and the
// actions the tick would have consumed are cleared as a tick clears them (env.cpp:141-142: they do not wait for the thaw).  No byte of the env's state, its
// status word or its ring of episodes is read or written.  Called by every thread of the workgroup; the env's first threads store.
__device__ __forceinline__ void frozen_tick(const GymView &gv, int env)
{
    const int A = gv.num_agents;
    if ((int)threadIdx.x < A) {
        gv.rewards[(size_t)env * A + threadIdx.x] = 0.0f;
        gv.actions[(size_t)env * A + threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) gv.done[env] = 0;
}

// ---- mv_set_episode_budget: envs that halt themselves (mv_episode_budget.h has the rule).  Where a step mask is one answer per launch, a budget is one
// PER TICK: an env whose tick j staged done with one episode left does not step in tick j + 1 of the same resident launch.  The MASKED bodies therefore carry
// one uniform register through the launch's ticks, read once at the top (env_left):
//     0    the env does not step in the next tick: frozen by the mask for the whole launch, or halted;
//   < 0    it steps and has nothing to spend (no budget attached, or unlimited);
//   > 0    it steps and may still finish that many episodes.
// and choose per tick between S::tick and frozen_tick, between the same barriers.  Behind a tick that stepped, after_tick reads the done that tick
// staged and spends.  Every wave of the workgroup keeps its own copy and sees the same dones behind the same barriers, so the choice stays workgroup-uniform;
// nobody reads left[env] from memory again within the launch, and the next launch on the stream reads what thread 0 stored.
__device__ __forceinline__ int32_t env_left(const GymView &gv, int env)
{
    if (env_frozen(gv, env)) return 0;   // (never stored: after_tick runs behind stepped ticks only)
    return gv.budget != nullptr ? __builtin_amdgcn_readfirstlane(gv.budget[env]) : -1;
}

// ---- mv_macro_step: envs whose macro step is over (mv_macro_step.h has the rule).  A second uniform value beside `left`, carried through the launch's ticks in
// the same way and read once at the top (env_tl):
//     0    the env's macro step is over -- its own k ticks are spent, or a tick of this call finished its episode: it does not step in the next tick;
//   < 0    no macro step in flight (the view carries no array): nothing to count;
//   > 0    it may step in that many more ticks of the call.
// An env steps in a tick when left != 0 and tl != 0 (env_steps); behind a tick that stepped, after_tick counts tl down, or clears it where the tick staged
// done, and thread 0 stores it for the next launch of the call.
__device__ __forceinline__ int32_t env_tl(const GymView &gv, int env)
{
    return gv.macro_tl != nullptr ? __builtin_amdgcn_readfirstlane(gv.macro_tl[env]) : -1;
}
__device__ __forceinline__ bool env_steps(int32_t left, int32_t tl) { return macro::macro_steps(1, left, tl); }   // (the mask: inside left, env_left)

// after_tick's macro half for the one-tick-per-launch kernels, which keep nothing of it across the tick: one thread reads tl and the staged done again and
// stores.  Not inlined, for state_obs_store's reason (below): inlined, it cost the Obstacles family's kernel six VGPRs and a wave per SIMD.
static __device__ __attribute__((noinline)) void macro_tick_store(int32_t *tl, const uint8_t *done)
{
    *tl = macro::macro_after_tick(*tl, (int)*done);
}

// Behind a tick of `gv` that env stepped in, and behind what orders that tick's stores before this load (wave_sync: one wave; the workgroup's barrier:
// several): the staged done, uniform (as reset_masked_body reads a count back); thread 0 stores the ticks the env's macro step has left (mv_macro_step) and,
// where the budget spends, the env's budget and, when this tick halted the env, counts it (a vector atomic).
__device__ __forceinline__ void after_tick(const GymView &gv, int env, int32_t &left, int32_t &tl)
{
    if (left <= 0 && tl <= 0) return;
    const int done = __builtin_amdgcn_readfirstlane((int)gv.done[env]);
    if (tl > 0) {
        tl = macro::macro_after_tick(tl, done);
        if (threadIdx.x == 0) gv.macro_tl[env] = tl;
    }
    if (!done || left <= 0) return;
    const bool halted = budget::episode_budget_spend(left, done);
    if (threadIdx.x == 0) {
        gv.budget[env] = left;
        if (halted) atomicAdd(gv.halted, 1u);
    }
}

// ---- mv_set_draw_mask: undrawn envs.  Whether env's A frames are set up in this launch: its mask byte, loaded once per launch and made uniform, as
// env_frozen's -- the env is the workgroup, so every wave takes the same side and every barrier stays workgroup-uniform; every view of a multi-tick launch
// carries the same mask, so the byte is asked through the first view.  Only the MASKED instantiations ask (the launchers pick them for a view with a step
// mask, a budget or a draw mask): an undrawn env's frames take frame_skip (mv_frame.h) between the barriers frame_setup_body would have met.  Nothing of the
// tick depends on it: rewards, dones, state, status words and the episode log are those of a drawn env.
__device__ __forceinline__ bool env_drawn(const GymView &gv, int env)
{
    return gv.draw_mask == nullptr || __builtin_amdgcn_readfirstlane((int)gv.draw_mask[env]) != 0;
}

// every frame of an undrawn env, in the shape the body's frame setups have: ONE = true: the workgroup (THREADS threads; WAVE_LOCAL: its one wave) shares the
// env's one frame; false: every wave takes its share of the env's A frames
// marker: FRAME_UNDRAWN, or FRAME_STILL (mv_set_still_frames, below)
template <bool ONE, int THREADS, bool WAVE_LOCAL>
__device__ __forceinline__ void env_frames_skip(const GymView &gv, int env, int marker = FRAME_UNDRAWN)
{
    if constexpr (ONE) frame_skip<THREADS, WAVE_LOCAL>(gv, env, marker);
    else {
        const int A = gv.num_agents, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
        for (int a = wave; a < A; a += nw) frame_skip<64, true>(gv, env * A + a, marker);
    }
}

// ---- mv_set_still_frames: envs whose frames are not drawn again (mv_still_frames.h has the rule).  A third uniform value beside `left` and `tl`, carried
// through the launch's ticks in the same way and read once at the top (env_stale):
//   < 0    the option is off (the view carries no array): the env is drawn on every pass, nothing is stored;
//     0    the env's state is what its frames were last drawn from: a pass of this launch takes frame_skip with FRAME_STILL;
//   > 0    the state may have changed: the next pass sets the frames up and draws them.
// It is updated behind the tick's `steps` choice (still_after_tick) and behind the frame choice (still_after_frames); thread 0 stores it at the launch's end
// where it changed -- the env is the workgroup, nobody else reads or writes its byte, and the next launch on the stream reads what was stored.  An env the
// draw mask leaves out stays as stale as it was.  The store is a call that is not inlined, for state_obs_store's reason.
__device__ __forceinline__ int env_stale(const GymView &gv, int env)
{
    return gv.still != nullptr ? __builtin_amdgcn_readfirstlane((int)gv.still[env]) : -1;
}
static __device__ __attribute__((noinline)) void still_store(uint8_t *stale, int v) { *stale = (uint8_t)v; }
// the marker of the frames of an env that is not set up in a pass: the draw mask's, else the still frames'
__device__ __forceinline__ int skip_marker(bool drawn) { return drawn ? still::FRAME_STILL : FRAME_UNDRAWN; }

// ---- mv_set_state_obs: the agents' state rows of this tick (mv_state_obs.h has the record).  Called by every thread of the workgroup BEHIND what orders the
// tick's stores before the frame setup's loads (wave_sync: one wave; the workgroup's barrier: several) -- the rows are loads of the same state -- and on either
// side of every choice above: a frozen or halted env reports its unchanged state, an undrawn env what a drawn one reports, a tick without frame setup what one
// with it does.  One exception needs no such ordering: the frozen path of step_body calls it straight behind frozen_tick, with no barrier -- frozen_tick
// writes rewards, actions and done only, and the state the rows load was written by an earlier launch.
// gv.state_obs is a kernel argument, so the branch is uniform; the env's first wave stores, lane l the word l of the env's 16 A (one round of 64 lanes up to
// four agents, two up to eight): consecutive lanes, consecutive dwords.  Nothing waits for the stores: the launch's end publishes them to the copy on the
// caller's stream.  Only the MASKED instantiations call it (the launchers pick them for a view with non-null rows).
// The store itself is a function of its own that is NOT inlined: inlined, its few registers were live across the tick loop of kernels that are held to 128
// (168) VGPRs by their launch bounds, and the allocator answered with up to 80 bytes more scratch per lane -- for every user of the MASKED kernels, with or
// without rows attached (TowerBuilding's one-agent MV_RENDER_LAST kernel: 168 -> 248 bytes); as a call behind the uniform branch it costs those kernels at
// most 16 bytes (profiles/state_obs_resources.txt).
static __device__ __attribute__((noinline)) void state_obs_store(uint32_t *rows, const AgentState *agents, const EnvHeader *hdr, int words)
{
    for (int l = threadIdx.x; l < words; l += 64) rows[l] = state_obs_word(agents + (l >> 4), hdr, l & (STATE_OBS_FLOATS - 1));
}
template <int A_MAX>
__device__ __forceinline__ void state_obs_write(const GymView &gv, int env)
{
    if (gv.state_obs == nullptr || threadIdx.x >= 64) return;
    const int A = A_MAX == 1 ? 1 : gv.num_agents, words = STATE_OBS_FLOATS * A;   // (one agent: known when the kernel is compiled)
    state_obs_store(reinterpret_cast<uint32_t *>(gv.state_obs) + (size_t)env * words, gv.agents + (size_t)env * A, gv.hdr + env, words);
}

// ---- mv_set_scene_obs: the env's scene row of this tick (mv_scene_obs.h has the record): 32 words per ENV, at exactly the sites of state_obs_write and under
// its ordering rule -- the row is loads of the state the tick wrote.  gv.scene_obs is a kernel argument, so the branch is uniform; the env's first wave writes,
// lanes 0..31 one column each: one 128-byte store per env.  The Obstacles family's two reductions are the wave's: every lane tests one terrain box (at most
// MAX_TERRAIN = 16) and one ballot gives the exit count (popcount) and the first exit (first set lane); the diamonds are counted in rounds of 64 lanes (at most
// COLLECT_MAX_REWARDS = 96 reward slots: two rounds), a ballot and a popcount each.  The results are uniform integers, the ones scene_obs_scan's loops give.
// The store is a call that is NOT inlined, for state_obs_store's reason.  Only the MASKED instantiations call it.
static __device__ __attribute__((noinline)) void scene_obs_store(uint32_t *row, int scenario, const EnvHeader *hdr, const TerrainBox *terrain,
                                                                 const MovableObject *rewards, const FootballState *fb)
{
    const int lane = threadIdx.x;   // (the env's first wave: 0..63, all of them here)
    SceneObsScan scan = {0, -1, 0};
    if (scenario == SCN_OBSTACLES) {   // (uniform)
        const int nt = min(hdr->num_terrain, (int)MAX_TERRAIN), nr = min(hdr->num_rewards, (int)COLLECT_MAX_REWARDS);
        const unsigned long long ex = __ballot(lane < nt && scene_obs_is_exit(terrain[lane].type));
        scan.exits = __popcll(ex);
        scan.first_exit = ex ? __ffsll(ex) - 1 : -1;
        for (int base = 0; base < nr; base += 64)
            scan.diamonds += __popcll(__ballot(base + lane < nr && scene_obs_diamond_there(rewards[base + lane].state)));
    }
    if (lane < SCENE_OBS_FLOATS) row[lane] = scene_obs_word(scenario, hdr, terrain, rewards, fb, scan, lane);
}
__device__ __forceinline__ void scene_obs_write(const GymView &gv, int env)
{
    if (gv.scene_obs == nullptr || threadIdx.x >= 64) return;
    scene_obs_store(reinterpret_cast<uint32_t *>(gv.scene_obs) + (size_t)env * SCENE_OBS_FLOATS, gv.scenario, gv.hdr + env, gv.terrain + (size_t)env * MAX_TERRAIN,
                    gv.rewards_obj + (size_t)env * gv.reward_stride, gv.fb + env);
}
// ---- mv_set_entity_obs: the env's entity rows of this tick (mv_entity_obs.h has the record): E rows of 8 words per ENV, at exactly the sites of
// scene_obs_write and under its ordering rule.  gv.entity_obs is a kernel argument, so the branch is uniform; the env's first wave writes, every lane one
// row per round -- at most three rounds of 64 lanes (ENTITY_MAX_ROWS) -- as two 16-byte vector stores: a round is a contiguous 2 KB per wave.  Sokoban's goal
// cells are the one compacted group: 16 rounds of 64 cells, a ballot each; a goal cell's lane takes the row its rank names (the goals of the rounds before +
// the goal lanes below it: __popcll(ballot & lanemask_lt)) -- the integers entity_soko_goal_of's loop gives -- and the rows behind the last goal are zeroed.
// Every row is stored by exactly one lane.  No LDS, no atomics.  The store is a call that is NOT inlined, for state_obs_store's reason.  Only the MASKED
// instantiations call it.
// (The two stores are plain: the optimiser keeps most of them 16 bytes wide and splits the rows of two branches into dword stores.  Forcing every row to
// stay two 16-byte stores -- volatile vectors -- was built and measured, and removed: 1024 envs, render='none', us per tick with the rows on: TowerBuilding
// 12.69 -> 13.78, Sokoban 16.59 -> 22.42; ObstaclesHard rendered 44.46 -> 48.27.)
__device__ __forceinline__ void entity_row_store(uint32_t *rows, int row, const EntityRow &r)
{
    uint4 *dst = reinterpret_cast<uint4 *>(rows + (size_t)row * ENTITY_OBS_FLOATS);
    dst[0] = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    dst[1] = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
}
static __device__ __attribute__((noinline)) void entity_obs_store(uint32_t *rows, int scenario, int A, const EnvHeader *hdr, const TerrainBox *terrain,
                                                                  const ArrangementItem *items, const uint8_t *soko, const MovableObject *objects,
                                                                  const MovableObject *rewards, const HexRec *hex_objs, const FootballState *fb,
                                                                  const AgentState *agents)
{
    const int lane = threadIdx.x;   // (the env's first wave: 0..63, all of them here)
    const EntityLayout l = entity_layout(scenario, A);
    const EntitySrc s = {scenario, A, hdr, terrain, items, soko, objects, rewards, hex_objs, fb, agents};
    const int first = scenario == SCN_SOKOBAN ? l.base[ENTITY_OBJECTS] : 0;   // (uniform: the goal rows are placed below)
    for (int row = first + lane; row < l.total; row += 64) entity_row_store(rows, row, entity_obs_row(s, l, row));
    if (scenario == SCN_SOKOBAN) {   // (uniform)
        const int W = hdr->W;
        int count = 0;
        for (int base = 0; base < SOKO_DIM * SOKO_DIM; base += 64) {
            const int cell = base + lane;
            const bool goal = soko[cell] == SOKO_GOAL;
            const unsigned long long m = __ballot(goal);
            const int k = count + __popcll(m & ((1ull << lane) - 1ull));
            if (goal && k < ENTITY_SOKO_GOALS) entity_row_store(rows, k, entity_soko_goal_row(cell, W));
            count += __popcll(m);
        }
        const EntityRow zero = {};
        for (int k = min(count, (int)ENTITY_SOKO_GOALS) + lane; k < ENTITY_SOKO_GOALS; k += 64) entity_row_store(rows, k, zero);
    }
}
__device__ __forceinline__ void entity_obs_write(const GymView &gv, int env)
{
    if (gv.entity_obs == nullptr || threadIdx.x >= 64) return;
    const int A = gv.num_agents;
    entity_obs_store(reinterpret_cast<uint32_t *>(gv.entity_obs) + (size_t)env * entity_obs_rows(gv.scenario, A) * ENTITY_OBS_FLOATS, gv.scenario, A,
                     gv.hdr + env, gv.terrain + (size_t)env * MAX_TERRAIN, gv.items + (size_t)env * MAX_ITEMS, gv.soko_cells + (size_t)env * (SOKO_DIM * SOKO_DIM),
                     gv.objects + (size_t)env * MAX_OBJECTS, gv.rewards_obj + (size_t)env * gv.reward_stride, gv.hex_objs + (size_t)env * HEX_MAX_OBJS,
                     gv.fb + env, gv.agents + (size_t)env * A);
}
// whether a view carries rows of any record (uniform): the extra barriers of the ticks without frame setup
__device__ __forceinline__ bool obs_rows_on(const GymView &gv) { return gv.state_obs != nullptr || gv.scene_obs != nullptr || gv.entity_obs != nullptr; }

// One workgroup per env: wave 0 runs the tick (one wave per env: physics, scenario logic, auto-reset), the others wait at the barrier (S::par_agents:
// they take their share of the character controllers first); then the workgroup builds the lists of the env's frames (mv_frame.h).  `render` = 0:
// mv_step_no_render.
//   one agent:  STEP_THREADS (128) threads work on the env's one frame together.  The tick needs ~150 VGPRs, i.e. 3 waves per SIMD: with
//               2 waves per env 1024 envs are resident at once (with 4 they take two rounds, and a launch lasts as long as its slowest
//               tick PER ROUND: measured 41 us vs 25 us);
//   A agents:   64 min(A, 4) threads, every wave sets up its own frame(s): a frame setup is a chain of dependent loads (~6 us), A of them
//               one after the other would cost more than the launch the fusion saves.
// step_body's frame setup, on its frozen path and on its stepping one: STEP_THREADS threads on the env's one frame, or up to four waves over its A frames
template <class S, int A_MAX>
__device__ __forceinline__ void step_frames_setup(const GymView &gv, int env, int W, int H, FrameScratch *s_fs)
{
    constexpr int NS = A_MAX == 1 ? 1 : 4;
    if constexpr (A_MAX == 1) frame_setup_body<STEP_THREADS, false>(gv, env, W, H, s_fs[0], depth_sort_scratch<S, NS>(0));
    else {
        const int A = gv.num_agents, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
        for (int a = wave; a < A; a += nw) frame_setup_body<64, true>(gv, env * A + a, W, H, s_fs[wave], depth_sort_scratch<S, NS>(wave));
    }
}

template <class S, int A_MAX, bool MASKED = false>
__device__ __forceinline__ void step_body(const GymView &gv, const int env, int W, int H, int render)
{
    constexpr int NS = A_MAX == 1 ? 1 : 4;
    __shared__ FrameScratch s_fs[NS];
#ifdef MV_STEP_PRIO
    __builtin_amdgcn_s_setprio(MV_STEP_PRIO);
#endif
    [[maybe_unused]] int32_t left = -1;
    if constexpr (MASKED) if ((left = env_tl(gv, env) == 0 ? 0 : env_left(gv, env)) == 0) {   // (mv_set_step_mask, mv_set_episode_budget) the frozen tick, then the env's frames as below, from the unchanged state
        frozen_tick(gv, env);
        state_obs_write<A_MAX>(gv, env); scene_obs_write(gv, env); entity_obs_write(gv, env);   // (mv_set_state_obs: the unchanged state, as the last launch left it)
        if (!render) return;
        // (mv_set_still_frames) read by every wave IN FRONT of the barrier, stored by thread 0 behind it: no wave reads what this launch stored
        const int stale = env_stale(gv, env);
        __syncthreads();
        if (!env_drawn(gv, env)) { env_frames_skip<A_MAX == 1, STEP_THREADS, false>(gv, env); return; }   // (mv_set_draw_mask; uniform)
        if (stale == 0) { env_frames_skip<A_MAX == 1, STEP_THREADS, false>(gv, env, still::FRAME_STILL); return; }   // (mv_set_still_frames; uniform)
        if (stale > 0 && threadIdx.x == 0) still_store(gv.still + env, 0);
        step_frames_setup<S, A_MAX>(gv, env, W, H, s_fs);
        return;
    }
    MV_T_BEGIN
#ifdef MV_TICK_TIMING
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
#endif
    if constexpr (S::par_agents && A_MAX > 1) S::template tick<A_MAX, true>(gv, env);
    else if (threadIdx.x < 64) S::template tick<A_MAX>(gv, env);
    if constexpr (MASKED) if (left > 0 || gv.macro_tl != nullptr) {   // (mv_set_episode_budget, mv_macro_step; uniform)
        __syncthreads();   // every wave has read left[env] and tl[env] before thread 0 stores them, and the tick's staged done is written
        [[maybe_unused]] int32_t none = -1;
        after_tick(gv, env, left, none);
        // (one tick per launch: tl is not kept across the tick -- this kernel's registers are the tick's -- but read again behind it, by the one thread that
        // stores it)
        if (gv.macro_tl != nullptr && threadIdx.x == 0) macro_tick_store(gv.macro_tl + env, gv.done + env);
    }
#ifdef MV_TICK_TIMING
    if (!render && gv.dbg && threadIdx.x == 0) {
        const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime();
        unsigned long long *d = gv.dbg + (size_t)env * 64;
        d[48] += rt1 - rt0; d[49] += 1; d[50] = rt0; d[51] = rt1;
        // (tick-only launches: 52..55 = ticks that regenerated the env, longest other tick)
        if (gv.hdr[env].num_frames == 0) { d[52] += rt1 - rt0; d[53] += 1; }
        else if (rt1 - rt0 > d[54]) { d[54] = rt1 - rt0; for (int k = 0; k < 16; ++k) d[32 + k] = d[16 + k]; }
    }
#endif
    if (!render) {
        if constexpr (MASKED) if (gv.still != nullptr && threadIdx.x == 0) still_store(gv.still + env, 1);   // (mv_set_still_frames: the env stepped, no pass follows)
        if constexpr (MASKED) if (obs_rows_on(gv)) {   // (mv_set_state_obs, mv_set_scene_obs; uniform) a tick without frame setup reports its rows too
            __syncthreads();   // the tick's stores before the rows' loads
            state_obs_write<A_MAX>(gv, env); scene_obs_write(gv, env); entity_obs_write(gv, env);
        }
        return;
    }
    __syncthreads();   // the tick's stores (same CU: same L1) before the frame setup's loads
    MV_T(6);           // the whole tick as wave 0 saw it (incl. the generator of a finished env), up to the barrier
    if constexpr (MASKED) { state_obs_write<A_MAX>(gv, env); scene_obs_write(gv, env); entity_obs_write(gv, env); }   // (mv_set_state_obs, mv_set_scene_obs)
    // (mv_set_still_frames: the env stepped -- stale where the draw mask leaves it out, drawn and fresh otherwise; nobody reads the byte in this launch)
    if constexpr (MASKED) if (!env_drawn(gv, env)) {   // (mv_set_draw_mask; uniform)
        if (gv.still != nullptr && threadIdx.x == 0) still_store(gv.still + env, 1);
        env_frames_skip<A_MAX == 1, STEP_THREADS, false>(gv, env);
        return;
    }
    if constexpr (MASKED) if (gv.still != nullptr && threadIdx.x == 0) still_store(gv.still + env, 0);
    step_frames_setup<S, A_MAX>(gv, env, W, H, s_fs);
    if constexpr (A_MAX == 1) {
        MV_T(7);   // frame setup
#ifdef MV_TICK_TIMING
        if (gv.dbg && threadIdx.x == 0) {
            const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime();
            unsigned long long *d = gv.dbg + (size_t)env * 64;
            if (!d[49]) { d[52] += rt1 - rt0; d[53] += 1; d[54] = rt0; d[55] = rt1; }
        }
#endif
    }
}

// ---- the resident multi-tick bodies' per-env option state: the uniform values above (env_left, env_tl, env_drawn, env_stale), loaded once per launch through
// its first view, carried through its ticks -- every wave of the workgroup its own copy, the same behind the same barriers -- and stored where they changed:
// left and tl by after_tick behind the tick that changed them, stale at the launch's end (env_options_store).  An instantiation that does not use a member
// leaves nothing of it behind: neither the load nor the register (the kernels without frame setup never ask for drawn).
struct EnvOptions {
    int32_t left = -1, tl = -1;    // (mv_set_step_mask, mv_set_episode_budget: env_left; mv_macro_step: env_tl)
    bool drawn = true;             // (mv_set_draw_mask: env_drawn)
    int stale = -1, stale0 = -1;   // (mv_set_still_frames: env_stale; stale0: what the launch found)
};
template <bool MASKED>
__device__ __forceinline__ EnvOptions env_options_load(const GymView &gv, int env)
{
    EnvOptions o;
    if constexpr (MASKED) { o.left = env_left(gv, env); o.tl = env_tl(gv, env); o.drawn = env_drawn(gv, env); o.stale = o.stale0 = env_stale(gv, env); }
    return o;
}
// in front of a tick: whether env steps in it (uniform; without MASKED: a constant), and stale behind that choice
template <bool MASKED>
__device__ __forceinline__ bool env_options_tick(EnvOptions &o)
{
    const bool steps = !MASKED || env_steps(o.left, o.tl);
    if constexpr (MASKED) o.stale = still::still_after_tick(o.stale, steps);
    return steps;
}
// (every wave read the byte in front of the loop's first barrier)
template <bool MASKED>
__device__ __forceinline__ void env_options_store(const GymView &gv, int env, const EnvOptions &o)
{
    if constexpr (MASKED) if (o.stale != o.stale0 && threadIdx.x == 0) still_store(gv.still + env, o.stale);
}

// ---- where the agent count enters a resident body: the tick's template arguments (in the body itself: a tick that is inlined through one more function comes
// out of hipcc with its instructions in another order, and a few unmasked kernels with another s_waitcnt count), and the helpers below.
// The barrier behind a tick: the tick's stores before the frame setup's / the next tick's loads.  One wave: no barrier needed; several: the workgroup's (same
// CU: same L1)
template <int A_MAX>
__device__ __forceinline__ void tick_barrier()
{
    if constexpr (A_MAX == 1) wave_sync();
    else __syncthreads();
}
// FrameScratch (N per workgroup), declared only in the instantiations that can set a frame up: LDS held by resident step waves is what the passes lose
template <int N>
__device__ __forceinline__ FrameScratch &frame_scratch(int i)
{
    __shared__ FrameScratch s_fs[N];
    return s_fs[i];
}
// The env's frames of one tick: the one wave on the env's one frame, or every wave on its share of the env's A frames; an env the draw mask leaves out or whose
// state did not change takes env_frames_skip instead (uniform), and a drawn setup clears stale
template <class S, int A_MAX, bool MASKED>
__device__ __forceinline__ void env_frames(const GymView &gv, int env, int W, int H, EnvOptions &o)
{
    constexpr int NS = A_MAX == 1 ? 1 : 4;
    if (!MASKED || (o.drawn && o.stale != 0)) {
        if constexpr (A_MAX == 1) frame_setup_body<64, true>(gv, env, W, H, frame_scratch<NS>(0), depth_sort_scratch<S, NS>(0));
        else {
            const int A = gv.num_agents, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
            for (int q = wave; q < A; q += nw) frame_setup_body<64, true>(gv, env * A + q, W, H, frame_scratch<NS>(wave), depth_sort_scratch<S, NS>(wave));
        }
        if constexpr (MASKED) o.stale = still::still_after_frames(o.stale, still::VERDICT_DRAWN);
    } else env_frames_skip<A_MAX == 1, 64, true>(gv, env, skip_marker(o.drawn));
}

// which ticks of a resident launch set their frames up
enum : int {
    FRAMES_NONE,      // none (the launch's mask is zero: a call that draws nothing, or a chunk in front of the drawn tick's)
    FRAMES_BY_MASK,   // tick j where bit j of the launch's mask (StepTicksArgs8::pad: a kernel argument, uniform) is set: the last chunk of an MV_RENDER_LAST call
    FRAMES_ALL        // every tick (mv_step_n with MV_RENDER_EVERY)
};

// k consecutive ticks of every env with ONE launch (a batched open-loop call, mv_step_n with a device-side random policy): the envs are
// independent and every tick draws its own actions, so nothing orders env A's tick j + 1 behind env B's tick j -- only k launches did, each as
// long as its slowest env, and each having to find room for 1024 two-wave workgroups of ~150 VGPRs beside the observation pass of the previous
// call (kernel traces, r04l: 70-190 us per step kernel while a pass runs, 20 us alone; the chain of step kernels, not the pass, set the pipelined
// rate).  Here an env's workgroup becomes resident once and runs tick, frame setup (into slot j's lists), tick, ...: gv[j] is tick j's view
// (its hand-over slot, its staging outputs, its action index, its cost histogram).  The frame setups of such a launch do not clear the next pass's
// histogram (lpt_no_clear: inside one launch env 0's clearing would race with the envs that are a tick ahead): every pass that draws from one clears it
// when its last workgroup has looked its frame up (mv_raster.hip: hist_done; mv_api.hip: take_hist).  An env that finishes swaps its next resident
// episode in at the tail of its tick as always -- a batched call only ever spans ticks of gyms whose episodes are long (mv_step_n steps the others
// tick by tick), so the resident episodes outlast it.
// One agent: ONE wave per env (the single-tick kernel's second wave only helps with the frame setup, and idles through the tick): the
// workgroups stay resident for the whole call beside the observation passes of the previous one, and every wave of ~150 VGPRs they hold is
// two or three waves the pass cannot have (measured: 21.1 M obs/s with two waves per env, 22.3 M with one).
// Several agents (S::par_agents): every wave of the workgroup ticks, then sets up its share of the env's frames.
// FRAMES (mv_step_n_render: MV_RENDER_NONE / MV_RENDER_LAST simulate ticks that set no frame up): FRAMES_NONE declares neither FrameScratch nor the depth
// sort's LDS, since LDS and registers held by resident step waves are what the passes beside them lose; with several agents the barrier behind the frame setups
// guards nothing and is gone, the one behind the tick stays (tick j + 1 reads what the other waves' tick j wrote).  An env that is frozen or halted when such a
// launch starts leaves behind the loads of env_left and n tiny stores.
template <class S, int A_MAX, class Args, int FRAMES, bool MASKED = false>
__device__ __forceinline__ void step_ticks_body(const Args &a, int W, int H)
{
    const int env = blockIdx.x;
#ifdef MV_STEP_PRIO
    __builtin_amdgcn_s_setprio(MV_STEP_PRIO);
#endif
    EnvOptions o = env_options_load<MASKED>(a.view(0), env);
    [[maybe_unused]] const uint32_t mask = FRAMES == FRAMES_ALL ? ~0u : (uint32_t)a.pad;
    for (int j = 0; j < a.n; ++j) {
        const GymView &gv = a.view(j);
        const bool frames = FRAMES != FRAMES_NONE && ((mask >> j) & 1u);   // (uniform; FRAMES_NONE, FRAMES_ALL: a constant)
        const bool steps = env_options_tick<MASKED>(o);
        if (!steps) frozen_tick(gv, env);
        else if constexpr (A_MAX == 1) S::template tick<1>(gv, env);
        else S::template tick<A_MAX, true>(gv, env);   // (S::par_agents: every wave of the workgroup ticks)
        tick_barrier<A_MAX>();
        if constexpr (MASKED) if (steps) after_tick(gv, env, o.left, o.tl);
        // (mv_set_state_obs, mv_set_scene_obs) the ticks of a launch without any frame setup reach their rows only where the view carries some (uniform)
        if constexpr (MASKED) if (FRAMES != FRAMES_NONE || obs_rows_on(gv)) { state_obs_write<A_MAX>(gv, env); scene_obs_write(gv, env); entity_obs_write(gv, env); }
        if (frames) {
            env_frames<S, A_MAX, MASKED>(gv, env, W, H, o);
            if constexpr (A_MAX > 1) __syncthreads();   // every frame of the env is set up (the state they read) before the next tick changes it
        } else if constexpr (MASKED && A_MAX > 1) {
            if (obs_rows_on(gv)) __syncthreads();   // (uniform) the rows' loads before the other waves' next tick changes the state
        }
    }
    env_options_store<MASKED>(a.view(0), env, o);
}

// Software-pipelined (one agent per env): TWO waves per env.  Wave 0 runs tick j + 1 while wave 1 sets tick j's frame up (mv_frame.h) -- the two halves of a
// tick's work that step_ticks_body runs back to back in one wave, each a chain of dependent loads and a few thousand vector instructions of ONE wave on its
// SIMD (48 % of the resident wave's cycles were spent in s_waitcnt, r08z_pmc_SQ2.csv).  The frame setup reads the simulator state in place, so the two waves
// meet at two workgroup barriers per tick:
//   A(j): tick j's state is written (wave 0: behind its write-back and the episode swap-in of a finished env; wave 1: before it reads anything)
//   B(j): tick j's state is read    (wave 1: behind the record loads of its last round of slots; wave 0: before tick j + 1's write-back, the tick's
// pipe_wait) An iteration lasts max(tick, frame setup) instead of their sum; the last frame setup runs alone.
template <class S, bool MASKED = false, class Args>
__device__ __forceinline__ void step_ticks_pipe_body(const Args &a, int W, int H)
{
    __shared__ FrameScratch s_fs;
    const int env = blockIdx.x;
#ifdef MV_STEP_PRIO
    __builtin_amdgcn_s_setprio(MV_STEP_PRIO);
#endif
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) {
        // (mv_set_step_mask, mv_set_episode_budget: env_left) a tick that does not step is the frozen tick at the barriers of a stepping one -- both barriers
        // of the iteration on either side of the choice; wave 1 sets the frames up as always, and only this wave needs to know what is left (mv_macro_step:
        // env_tl, likewise; never launched with still frames: mv_step.hip)
        EnvOptions o = env_options_load<MASKED>(a.view(0), env);
        for (int j = 0; j < a.n; ++j) {
            if (env_options_tick<MASKED>(o)) {
                S::template tick<1>(a.view(j), env, j > 0);   // (j > 0: B(j - 1) inside, before the write-back)
                if constexpr (MASKED) if (o.left > 0 || o.tl > 0) { wave_sync(); after_tick(a.view(j), env, o.left, o.tl); }   // (this wave's own stores)
            } else {
                if (j > 0) __syncthreads();               // B(j - 1): inside a tick (pipe_wait), here in the open
                frozen_tick(a.view(j), env);
            }
            __syncthreads();                              // A(j)
            // (mv_set_state_obs, mv_set_scene_obs) tick j's rows: behind A(j), in front of tick j + 1, whose write-back comes behind B(j) and is this wave's own
            if constexpr (MASKED) { state_obs_write<1>(a.view(j), env); scene_obs_write(a.view(j), env); entity_obs_write(a.view(j), env); }
        }
        __syncthreads();                                  // B(n - 1): the last frame setup's
    } else {
        const bool drawn = env_options_load<MASKED>(a.view(0), env).drawn;   // (mv_set_draw_mask: env_drawn; only this wave needs to know)
        for (int j = 0; j < a.n; ++j) {
            __syncthreads();                              // A(j)
            if (drawn) frame_setup_body<64, true, true>(a.view(j), env, W, H, s_fs);   // B(j) inside
            else frame_skip<64, true, true>(a.view(j), env);                                      // ... likewise
        }
    }
}

// mv_reset / the refill of a forced reset: every finished (force_all: every) env takes its next resident episode
template <class S>
__device__ __forceinline__ void reset_body(const GymView &gv, int force_all)
{
    const int env = blockIdx.x;
    if (env >= gv.num_envs) return;
    if (!force_all && !gv.hdr[env].done) return;
    S::swap_in(gv, env, force_all);
}

// mv_reset_envs: the envs a mask [num_envs] flags leave their episode and take their next resident one, as every env does under mv_reset (force_all = 1).
// One wavefront per env.  The env's mask byte is loaded once and made uniform; an unflagged wave leaves behind that one load, so a sparse mask costs a launch
// of waves that exit, not mv_reset's.  applied [num_envs]: a flagged env's wave leaves 1 where it took an episode, 0 where none was resident (ST_STARVED: the
// env stays as it was) -- what the episode log's masked clear goes by; the bytes of unflagged envs are not written.
template <class S>
__device__ __forceinline__ void reset_masked_body(const GymView &gv, const uint8_t *__restrict__ mask, uint8_t *__restrict__ applied)
{
    const int env = blockIdx.x;
    if (env >= gv.num_envs) return;
    if (__builtin_amdgcn_readfirstlane((int)mask[env]) == 0) return;
    const int before = gv.hdr[env].episodes_consumed;
    S::swap_in(gv, env, 1);
    if (threadIdx.x == 0) applied[env] = gv.hdr[env].episodes_consumed != before ? 1 : 0;   // (lane 0 stored the count: its own store, read back in order)
}

// one scenario's entry points (its mv_step_<scenario>.hip); null: the scenario has no such kernel
struct StepKernels {
    void (*step)(GymView, int, int, int);                // one agent per env
    void (*step_agents)(GymView, int, int, int);         // several (agent loops are real loops: one multi-agent build)
    void (*ticks)(StepTicksArgs8, int, int);             // k ticks, one agent per env
    void (*ticks_pipe)(StepTicksArgs8, int, int);        // ... software-pipelined
    void (*ticks_agents)(StepTicksArgs8, int, int);      // k ticks, several agents per env
    void (*reset)(GymView, int);
    void (*reset_masked)(GymView, const uint8_t *, uint8_t *);   // mv_reset_envs: the envs a mask flags
    // k ticks that set no frame up, and k ticks whose frame setups follow a mask (step_ticks_body: FRAMES_NONE, FRAMES_BY_MASK): one agent per env; several (TowerBuilding)
    void (*ticks_sim)(StepTicksArgs8, int, int);
    void (*ticks_sim_frames)(StepTicksArgs8, int, int);
    void (*ticks_sim_agents)(StepTicksArgs8, int, int);
    void (*ticks_sim_agents_frames)(StepTicksArgs8, int, int);
};
// (<scenario>_kernels_masked: the MASKED instantiations of the step entries, for views with a step mask; the reset entries are the same kernels)
extern const StepKernels tower_kernels, obstacles_kernels, collect_kernels, rearrange_kernels, sokoban_kernels, hex_kernels, boxagone_kernels,
                          football_kernels;
extern const StepKernels tower_kernels_masked, obstacles_kernels_masked, collect_kernels_masked, rearrange_kernels_masked, sokoban_kernels_masked,
                          hex_kernels_masked, boxagone_kernels_masked, football_kernels_masked;

}  // namespace mv
