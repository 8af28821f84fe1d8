// megaverse_amd/csrc/mv_episode_budget.h -- episode budgets (include/megaverse_hip.h: mv_set_episode_budget): the rule, written once for the step kernels
// (mv_step_kernels.h: the MASKED bodies), the episode log's update (mv_episode_log.hip), and the host twin mv_debug_episode_budget_host.
// No reference counterpart: VectorEnv::step steps every env and resets the finished ones on the spot (vector_env.cpp:89-108).
//
// Per env the gym owns an int32 `left`:   < 0 unlimited,   > 0 the env may still finish that many episodes,   0 HALTED.
// Tick t, env e, `left` as it stands BEFORE the tick:
//   the env steps  <=>  (no step mask attached or mask[e] != 0) and left != 0;
//   an env that steps runs the tick it always ran; if that tick staged done and left > 0, left goes down by one;
//   an env that does not step runs the frozen tick of the step masks (mv_step_kernels.h: frozen_tick) and left stays.
// So an env with budget b finishes exactly b episodes and then stands, frozen, on the first frame of its next one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mv {
namespace budget {

#define MV_BUDGET_HD __host__ __device__ inline

// whether an env steps in a tick: its mask byte (1 where no mask is attached) and its budget before the tick
MV_BUDGET_HD bool episode_budget_steps(int mask_byte, int32_t left) { return mask_byte != 0 && left != 0; }

// the budget behind a tick the env stepped in, `done` being what that tick staged; -> true when this tick halted the env (left went 1 -> 0)
MV_BUDGET_HD bool episode_budget_spend(int32_t &left, int done)
{
    if (!done || left <= 0) return false;
    left -= 1;
    return left == 0;
}

// what a gym with N envs keeps in device memory, one allocation: left [N], the halted count, the episode log's mirror of left [N]
MV_BUDGET_HD size_t episode_budget_words(int32_t N) { return 2 * (size_t)N + 1; }

}  // namespace budget
}  // namespace mv
