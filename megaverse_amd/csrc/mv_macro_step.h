// megaverse_amd/csrc/mv_macro_step.h -- macro steps (include/megaverse_hip.h: mv_macro_step): the rule and the fold, written once for the step kernels
// (mv_step_kernels.h: the MASKED bodies), the episode log's update (mv_episode_log.hip), the accumulating publication (mv_macro_step.hip) and the host twins
// mv_debug_macro_rule_host / mv_debug_macro_fold_host.
// No reference counterpart: it is the action-repeat wrapper a learner writes around VectorEnv::step (vector_env.cpp:89-108),
//     for _ in range(k): obs, r, d = env.step(a); total += r; if d: break
// per env, as one operation.
//
// Per env the gym owns an int32 `tl` (ticks left), set at the call's start to clamp(ticks[e], 0, k) (no ticks given: k).
// Tick t of the call, env e, `left` (mv_episode_budget.h) and `tl` as they stand BEFORE the tick:
//   the env steps  <=>  mv_episode_budget.h's rule lets it (mask and budget, unchanged) and tl > 0;
//   behind a tick the env stepped in: tl goes down by one, and to 0 if that tick staged done; the budget is spent as always;
//   an env that does not step runs the frozen tick of the step masks (mv_step_kernels.h: frozen_tick) and tl stays.
// So an env's macro step ends with the tick that finished its episode -- that tick ran whole, auto-reset included -- and the env waits, frozen, on the first
// frame of its next episode for the rest of the call.
// In the kernels a NEGATIVE tl says "no macro step in flight": such an env steps whenever mask and budget let it, and nothing is stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mv_episode_budget.h"

namespace mv {
namespace macro {

#define MV_MACRO_HD __host__ __device__ inline

// tl at the call's start: the caller's ticks[e] (has_ticks) clamped to [0, k], else k
MV_MACRO_HD int32_t macro_ticks_begin(bool has_ticks, int32_t ticks, int32_t k) { return !has_ticks ? k : ticks < 0 ? 0 : ticks > k ? k : ticks; }

// whether an env steps in a tick: its mask byte (1 where no mask is attached), its budget and its ticks left before the tick (tl < 0: no macro step)
MV_MACRO_HD bool macro_steps(int mask_byte, int32_t left, int32_t tl) { return budget::episode_budget_steps(mask_byte, left) && tl != 0; }

// tl behind a tick the env stepped in, `done` being what that tick staged
MV_MACRO_HD int32_t macro_after_tick(int32_t tl, int done) { return tl <= 0 ? tl : done ? 0 : tl - 1; }

// The fold of a call's per-tick rewards: s = r_0; s = s + r_j, in tick order -- one IEEE fp32 addition per tick, nothing reassociated, nothing contracted
// (the library is built with -ffp-contract=off and without fast-math, and an addition alone has nothing to contract).  The first value is taken as it is,
// not added to zero: -0.0f stays -0.0f.
MV_MACRO_HD float macro_fold(float s, float r) { return s + r; }

// what a gym with N envs of A agents keeps in device memory for macro steps, one allocation: tl [N], the episode log's mirror of it [N], and where the host
// form's values land: ticks [N], actions [N*A][6]
MV_MACRO_HD size_t macro_step_words(int32_t N, int32_t A) { return 3 * (size_t)N + 6 * (size_t)N * (size_t)A; }

}  // namespace macro
}  // namespace mv
