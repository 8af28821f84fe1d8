// megaverse_amd/csrc/mv_step_boxagone.hip -- the step and reset kernels of BoxAGone: entry points over the shared bodies (mv_step_kernels.h)
// for the scenario's tick (mv_tick_boxagone.h: what it replaces, how it maps onto a wavefront).
#include <hip/hip_runtime.h>

#include "mv_step_kernels.h"
#include "mv_tick_boxagone.h"

namespace mv {

using S = tick_boxagone::Scenario;

template <int A_MAX> __global__ __launch_bounds__(256) void step_boxagone_kernel(GymView gv, int W, int H, int render) { step_body<S, A_MAX>(gv, blockIdx.x, W, H, render); }
template <class Args> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_boxagone_ticks_kernel(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES_ALL>(a, W, H); }
// (ticks that set no frame up; FRAMES: a mask says which ticks do -- step_ticks_body: FRAMES_NONE, FRAMES_BY_MASK)
template <class Args, bool FRAMES> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_boxagone_ticks_sim_kernel(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES ? FRAMES_BY_MASK : FRAMES_NONE>(a, W, H); }
__global__ __launch_bounds__(64) void reset_boxagone_kernel(GymView gv, int force_all) { reset_body<S>(gv, force_all); }
__global__ __launch_bounds__(64) void reset_masked_boxagone_kernel(GymView gv, const uint8_t *mask, uint8_t *applied) { reset_masked_body<S>(gv, mask, applied); }

// the same entry points for views with a step mask (mv_set_step_mask): the MASKED instantiations of the bodies (mv_step_kernels.h)
template <int A_MAX> __global__ __launch_bounds__(256) void step_boxagone_kernel_masked(GymView gv, int W, int H, int render) { step_body<S, A_MAX, true>(gv, blockIdx.x, W, H, render); }
template <class Args> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_boxagone_ticks_kernel_masked(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES_ALL, true>(a, W, H); }
template <class Args, bool FRAMES> __global__ __launch_bounds__(64, MV_STEP_TICKS_WAVES_PER_SIMD) void step_boxagone_ticks_sim_kernel_masked(Args a, int W, int H) { step_ticks_body<S, 1, Args, FRAMES ? FRAMES_BY_MASK : FRAMES_NONE, true>(a, W, H); }

const StepKernels boxagone_kernels = {step_boxagone_kernel<1>, step_boxagone_kernel<MAX_AGENTS>, step_boxagone_ticks_kernel<StepTicksArgs8>,
                                      nullptr, nullptr, reset_boxagone_kernel, reset_masked_boxagone_kernel,
                                      step_boxagone_ticks_sim_kernel<StepTicksArgs8, false>, step_boxagone_ticks_sim_kernel<StepTicksArgs8, true>, nullptr, nullptr};
const StepKernels boxagone_kernels_masked = {step_boxagone_kernel_masked<1>, step_boxagone_kernel_masked<MAX_AGENTS>, step_boxagone_ticks_kernel_masked<StepTicksArgs8>,
                                      nullptr, nullptr, reset_boxagone_kernel, reset_masked_boxagone_kernel,
                                      step_boxagone_ticks_sim_kernel_masked<StepTicksArgs8, false>, step_boxagone_ticks_sim_kernel_masked<StepTicksArgs8, true>, nullptr, nullptr};

}  // namespace mv
