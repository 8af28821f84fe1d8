// megaverse_amd/csrc/mv_step.hip -- the step and reset kernels of TowerBuilding: entry points over the shared bodies (mv_step_kernels.h) for the
// scenario's tick (mv_tick_tower.h: what it replaces, how it maps onto a wavefront); and the launchers of every scenario's step and reset kernels.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

#include "mv_step_kernels.h"
#include "mv_tick_tower.h"

static_assert(mv::ENTITY_CAP_R == mv::CAP_R && mv::ENTITY_CAP_HH == mv::CAP_HH, "entity observations: an agent's half extents are the capsule's of mv_physics.h");

namespace mv {

using S = tick_tower::Scenario;

template <int A_MAX> __global__ __launch_bounds__(256) void step_kernel(GymView gv, int W, int H, int render) { step_body<S, A_MAX>(gv, blockIdx.x, W, H, render); }
template <class Args> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_ticks_kernel(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES_ALL>(a, W, H); }
template <class Args> __global__ __launch_bounds__(256, 3) void step_ticks_agents_kernel(Args a, int W, int H) { step_ticks_body<S, MAX_AGENTS, Args, FRAMES_ALL>(a, W, H); }
template <class Args> __global__ __launch_bounds__(128, MV_STEP_TICKS_WAVES_PER_SIMD) void step_ticks_pipe_kernel(Args a, int W, int H) { step_ticks_pipe_body<S>(a, W, H); }
// (ticks that set no frame up; FRAMES: a mask says which ticks do -- step_ticks_body: FRAMES_NONE, FRAMES_BY_MASK)
template <class Args, bool FRAMES> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_ticks_sim_kernel(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES ? FRAMES_BY_MASK : FRAMES_NONE>(a, W, H); }
template <class Args, bool FRAMES> __global__ __launch_bounds__(256, 3) void step_ticks_sim_agents_kernel(Args a, int W, int H) { step_ticks_body<S, MAX_AGENTS, Args, FRAMES ? FRAMES_BY_MASK : FRAMES_NONE>(a, W, H); }
// (the draws that refill the rings run in front of it: tower_draw_kernel, mv_reset.hip)
__global__ __launch_bounds__(64) void reset_kernel(GymView gv, int force_all) { reset_body<S>(gv, force_all); }
__global__ __launch_bounds__(64) void reset_masked_kernel(GymView gv, const uint8_t *mask, uint8_t *applied) { reset_masked_body<S>(gv, mask, applied); }

// the same entry points for views with a step mask (mv_set_step_mask): the MASKED instantiations of the bodies (mv_step_kernels.h)
template <int A_MAX> __global__ __launch_bounds__(256) void step_kernel_masked(GymView gv, int W, int H, int render) { step_body<S, A_MAX, true>(gv, blockIdx.x, W, H, render); }
template <class Args> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_ticks_kernel_masked(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES_ALL, true>(a, W, H); }
template <class Args> __global__ __launch_bounds__(256, 3) void step_ticks_agents_kernel_masked(Args a, int W, int H) { step_ticks_body<S, MAX_AGENTS, Args, FRAMES_ALL, true>(a, W, H); }
template <class Args> __global__ __launch_bounds__(128, MV_STEP_TICKS_WAVES_PER_SIMD) void step_ticks_pipe_kernel_masked(Args a, int W, int H) { step_ticks_pipe_body<S, true>(a, W, H); }
template <class Args, bool FRAMES> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_ticks_sim_kernel_masked(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES ? FRAMES_BY_MASK : FRAMES_NONE, true>(a, W, H); }
template <class Args, bool FRAMES> __global__ __launch_bounds__(256, 3) void step_ticks_sim_agents_kernel_masked(Args a, int W, int H) { step_ticks_body<S, MAX_AGENTS, Args, FRAMES ? FRAMES_BY_MASK : FRAMES_NONE, true>(a, W, H); }

const StepKernels tower_kernels = {step_kernel<1>, step_kernel<MAX_AGENTS>, step_ticks_kernel<StepTicksArgs8>, step_ticks_pipe_kernel<StepTicksArgs8>,
                                   step_ticks_agents_kernel<StepTicksArgs8>, reset_kernel, reset_masked_kernel,
                                   step_ticks_sim_kernel<StepTicksArgs8, false>, step_ticks_sim_kernel<StepTicksArgs8, true>,
                                   step_ticks_sim_agents_kernel<StepTicksArgs8, false>, step_ticks_sim_agents_kernel<StepTicksArgs8, true>};
const StepKernels tower_kernels_masked = {step_kernel_masked<1>, step_kernel_masked<MAX_AGENTS>, step_ticks_kernel_masked<StepTicksArgs8>, step_ticks_pipe_kernel_masked<StepTicksArgs8>,
                                   step_ticks_agents_kernel_masked<StepTicksArgs8>, reset_kernel, reset_masked_kernel,
                                   step_ticks_sim_kernel_masked<StepTicksArgs8, false>, step_ticks_sim_kernel_masked<StepTicksArgs8, true>,
                                   step_ticks_sim_agents_kernel_masked<StepTicksArgs8, false>, step_ticks_sim_agents_kernel_masked<StepTicksArgs8, true>};

// masked: view_has_options (mv_types.h)
static const StepKernels &kernels_of(int scenario, bool masked = false)
{
    switch (scenario) {
    case SCN_TOWER: return masked ? tower_kernels_masked : tower_kernels;
    case SCN_OBSTACLES:
    case SCN_EMPTY: return masked ? obstacles_kernels_masked : obstacles_kernels;
    case SCN_COLLECT: return masked ? collect_kernels_masked : collect_kernels;
    case SCN_REARRANGE: return masked ? rearrange_kernels_masked : rearrange_kernels;
    case SCN_SOKOBAN: return masked ? sokoban_kernels_masked : sokoban_kernels;
    case SCN_BOXAGONE: return masked ? boxagone_kernels_masked : boxagone_kernels;
    case SCN_FOOTBALL: return masked ? football_kernels_masked : football_kernels;
    default: return masked ? hex_kernels_masked : hex_kernels;   // SCN_HEX_MEMORY, SCN_HEX_EXPLORE
    }
}

// When the two-wave kernels run.  ALONE on the chip their launch is a quarter shorter (TowerBuilding 16.6 -> 12.3 us per tick: 98 us per 8 ticks, Empty 16.9 ->
// 14.5, r09a); beside the observation passes of a FULL chip -- 1024 envs: a resident wave on every SIMD -- its length follows the passes' vector load, not its
// own dependent chains, and the second wave per env is registers the passes lose: TowerBuilding 32.8 / 32.1 M obs/s (one wave / two), ObstaclesHard 28.6 / 26.1
// (r09z, r10r).  With fewer envs than SIMDs the second wave is free and the step launch is what a call waits for (r10s, one wave / two, M obs/s):
//   envs           256            512            768
//   TowerBuilding  11.6 / 16.9    24.0 / 25.2    28.5 / 28.2
//   ObstaclesHard  11.6 / 14.0    20.7 / 23.1    26.0 / 26.3      (512: one GPU's share of BASELINE configs[2])
//   ObstaclesEasy  12.3 / 14.0    21.3 / 23.8    26.5 / 27.3
//   Empty          15.4 / 17.9    26.1 / 33.1    35.4 / 44.6      (1024: 45.8 / 47.0)
// So: up to 512 envs always, the Obstacles family up to 768, Empty at any size.  MV_STEP_PIPE=0 / 1 forces one or the other (read at every launch: tests switch).
static bool step_pipe_enabled(const GymView &gv)
{
    const char *e = getenv("MV_STEP_PIPE");
    if (e && *e) return atoi(e) != 0;
    const bool obstFamily = gv.scenario == SCN_OBSTACLES || gv.scenario == SCN_EMPTY;
    return gv.num_envs <= 512 || (obstFamily && gv.num_envs <= 768) || gv.scenario == SCN_EMPTY;
}

void launch_step_ticks(const GymView *views, int k, hipStream_t stream, int W, int H, hipEvent_t done)
{
    const GymView &gv = views[0];
    const StepKernels &K = kernels_of(gv.scenario, view_has_options(gv));
    StepTicksArgs8 a;   // (k <= 8: the views are the launch's arguments)
    a.n = k; a.pad = 0;
    for (int j = 0; j < 8; ++j) a.gv[j] = views[std::min(j, k - 1)];
    // several agents (TowerBuilding): TWO waves per env (measured at 512 envs x 4 agents: one wave 20.3 M obs/s, two 21.7, four 16.1 -- four waves of ~180
    // VGPRs per env, resident for the whole call, are what the observation passes beside them cannot have; one-launch-per-tick: 19.4)
    if (gv.num_agents > 1) hipExtLaunchKernelGGL(K.ticks_agents, dim3(gv.num_envs), dim3(64 * std::min(gv.num_agents, 2)), 0, stream, nullptr, done, 0, a, W, H);
    // (mv_set_still_frames: never the two-wave kernel -- its frame wave would need the tick wave's per-tick answer)
    else if (K.ticks_pipe && gv.still == nullptr && step_pipe_enabled(gv)) hipExtLaunchKernelGGL(K.ticks_pipe, dim3(gv.num_envs), dim3(128), 0, stream, nullptr, done, 0, a, W, H);
    else hipExtLaunchKernelGGL(K.ticks, dim3(gv.num_envs), dim3(64), 0, stream, nullptr, done, 0, a, W, H);
}

// k <= 8 ticks of every env with one launch, frame setups only for the ticks whose bit is set in frame_mask (0: the kernels without any frame setup).  The
// shapes launch_step_ticks has, but for the two-wave pipelined kernels: they exist to overlap a tick with the previous tick's frame setup.
void launch_step_ticks_sim(const GymView *views, int k, unsigned frame_mask, hipStream_t stream, int W, int H, hipEvent_t done)
{
    const GymView &gv = views[0];
    const StepKernels &K = kernels_of(gv.scenario, view_has_options(gv));
    StepTicksArgs8 a;
    a.n = k; a.pad = (int32_t)(frame_mask & ((1u << k) - 1u));
    for (int j = 0; j < 8; ++j) a.gv[j] = views[std::min(j, k - 1)];
    if (gv.num_agents > 1)
        hipExtLaunchKernelGGL(a.pad ? K.ticks_sim_agents_frames : K.ticks_sim_agents, dim3(gv.num_envs), dim3(64 * std::min(gv.num_agents, 2)), 0, stream,
                              nullptr, done, 0, a, W, H);
    else hipExtLaunchKernelGGL(a.pad ? K.ticks_sim_frames : K.ticks_sim, dim3(gv.num_envs), dim3(64), 0, stream, nullptr, done, 0, a, W, H);
}

// done: an event that completes with the launch, carried by its dispatch packet (cf. mv_raster.h) -- TowerBuilding's launch only; -> whether it rides
bool launch_step(const GymView &gv, hipStream_t stream, int W, int H, int render, hipEvent_t done)
{
    const StepKernels &K = kernels_of(gv.scenario, view_has_options(gv));
    if (gv.scenario != SCN_TOWER) done = nullptr;
    const dim3 grid(gv.num_envs), block(gv.num_agents == 1 ? STEP_THREADS : 64 * std::min(gv.num_agents, 4));
    hipExtLaunchKernelGGL(gv.num_agents == 1 ? K.step : K.step_agents, grid, block, 0, stream, nullptr, done, 0, gv, W, H, render);
    return done != nullptr;
}

void launch_reset_episodes(const GymView &gv, int force_all, hipStream_t stream)
{
    hipLaunchKernelGGL(kernels_of(gv.scenario).reset, dim3(gv.num_envs), dim3(64), 0, stream, gv, force_all);
}

void launch_reset_envs(const GymView &gv, const uint8_t *mask, uint8_t *applied, hipStream_t stream)
{
    hipLaunchKernelGGL(kernels_of(gv.scenario).reset_masked, dim3(gv.num_envs), dim3(64), 0, stream, gv, mask, applied);
}

}  // namespace mv
