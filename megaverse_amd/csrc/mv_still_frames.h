// megaverse_amd/csrc/mv_still_frames.h -- still frames (include/megaverse_hip.h: mv_set_still_frames): the rule and the carry, written once for the step
// kernels (mv_step_kernels.h: the MASKED bodies), the carry launch (mv_still_frames.hip) and the host twins mv_debug_still_rule_host /
// mv_debug_still_carry_host.
// No reference counterpart: the reference draws every env on every tick.  An env that did not step -- frozen by a step mask, halted by its episode budget,
// stopped inside a macro step -- has the state it had, so drawing it again leaves the bytes the last drawing left.  While the option is on the gym draws an
// env's A frames only where its state may have changed since they were drawn last.
//
// Per env the gym owns one byte `stale` (all 1 when the option is switched on).  The verdict of a tick that has an observation pass, in this order:
//   user-undrawn  the env's draw-mask byte is 0: FRAME_UNDRAWN as always, the rows are untouched, stale stays;
//   drawn         stale != 0: the frames are set up and drawn as always, stale becomes 0;
//   still         stale == 0: the frames take frame_skip (mv_frame.h) with FRAME_STILL -- no setup, no ray cast; the rows keep the last drawn frame (a single
//                 observation slab), or take it from the ring entry that holds it (an output ring: still_carry_plan).
// stale is set by every tick the env stepped in, with or without a pass (the ticks of MV_RENDER_NONE, the undrawn ticks of MV_RENDER_LAST), and left alone by a
// frozen, halted or macro-stopped tick.  On the host every call that can change an env's state, or what or where the gym draws, sets ALL bytes (mv_reset,
// mv_reset_envs, mv_fork_envs, mv_resample_envs, mv_load_envs, mv_seed, mv_render, mv_set_obs_buffer, mv_set_output_ring, mv_set_obs_layout,
// mv_set_pixel_mode, mv_set_render_resolution, the mv_debug_set_* setters): conservative on purpose -- a planner that forks every iteration redraws its
// frozen root once per iteration.
// Within one stepping call nothing but an env's own ticks can make it stale, and a tick that stepped is drawn by its own pass: an env's verdicts within a
// call are a drawn prefix followed by a still suffix (or user-undrawn throughout: the mask does not change under a call).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mv {
namespace still {

#define MV_STILL_HD __host__ __device__ inline

// the second negative frame marker beside mv_frame.h's FRAME_UNDRAWN (-1): every pass kernel leaves on a negative count
constexpr int FRAME_STILL = -2;

// what the twins report per (tick, env)
enum : int { VERDICT_NO_PASS = 0, VERDICT_DRAWN = 1, VERDICT_UNDRAWN = -1, VERDICT_STILL = -2 };

// In the kernels the stale byte travels as an int, negative where the option is off (the view carries no array): such an env is drawn on every pass and
// nothing is stored.

// stale behind the tick's `steps` choice
MV_STILL_HD int still_after_tick(int stale, bool steps) { return stale >= 0 && steps ? 1 : stale; }

// the verdict of a pass, from the env's draw-mask byte (1 where no mask is attached) and stale behind still_after_tick
MV_STILL_HD int still_verdict(int mask_byte, int stale) { return mask_byte == 0 ? VERDICT_UNDRAWN : stale != 0 ? VERDICT_DRAWN : VERDICT_STILL; }

// stale behind the frame choice
MV_STILL_HD int still_after_frames(int stale, int verdict) { return stale >= 0 && verdict == VERDICT_DRAWN ? 0 : stale; }

// ---- the carry (an output ring).  One frame's walk over the k rendered ticks of a call, in order: verdict[j * vstride] is tick j's verdict for the frame as
// the passes read it (>= 0: a drawn frame's list length; FRAME_UNDRAWN; FRAME_STILL), entry[j] the ring entry tick j's rows are in, home the entry that holds
// the frame's latest drawn bytes (< 0: none yet).  src[j]: the entry tick j's rows are to be copied FROM, or -1 for none -- a still tick takes the bytes of the
// entry they were last DRAWN into, not of the tick before it, so that a run of still ticks reads one source; a still tick whose entry is that source copies
// nothing.  Returns the new home: the entry of the last tick that was drawn or still.
MV_STILL_HD int32_t still_carry_plan(const int32_t *verdict, size_t vstride, const int32_t *entry, int k, int32_t home, int32_t *src)
{
    int32_t from = home;
    for (int j = 0; j < k; ++j) {
        const int32_t v = verdict[(size_t)j * vstride];
        src[j] = -1;
        if (v >= 0) from = home = entry[j];
        else if (v == FRAME_STILL) {
            if (from >= 0 && from != entry[j]) src[j] = from;
            home = entry[j];
        }
    }
    return home;
}

// what a gym with N envs of A agents keeps in device memory for still frames, one allocation: home [N*A] int32, then stale [N] bytes
MV_STILL_HD size_t still_frames_bytes(int32_t N, int32_t A) { return (size_t)N * (size_t)A * sizeof(int32_t) + (size_t)N; }

}  // namespace still
}  // namespace mv
