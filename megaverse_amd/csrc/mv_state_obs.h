// megaverse_amd/csrc/mv_state_obs.h -- state observations (include/megaverse_hip.h: mv_set_state_obs): the record, stated once for the kernels that write
// it (mv_step_kernels.h: state_obs_write; mv_obs_rows.hip: the gather behind a reset or mv_render) and for the host hook the tests compare it with
// (mv_debug_state_obs_host).  One row of MV_STATE_OBS_FLOATS = 16 float32 per agent, agent-major [N*A][16], taken from the env's state AFTER the tick --
// auto-reset included: a tick that finished an episode shows the first state of the next one, as its frame does:
//    0..2   pos[0..2]                 AgentState          8, 9   hvx, hvz                        AgentState
//    3..6   m00, m02, m20, m22        AgentState          10     vvel                            AgentState
//    7      pitch                     AgentState          11     carrying >= 0 ? 1.0f : 0.0f     AgentState
//    12,13  episode_sec, episode_len  the env's EnvHeader 14     total_reward                    AgentState
//    15     +0.0f (reserved)
// Values are copied, not recomputed: the functions below move 32-bit words, so every bit -- a -0.0f, a NaN's payload, a denormal -- is the state's bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mv_types.h"

namespace mv {

enum : int { STATE_OBS_FLOATS = 16 };

// columns 0..10 are the first eleven words of an AgentState, in its order
static_assert(offsetof(AgentState, pos) == 0 && offsetof(AgentState, m00) == 12 && offsetof(AgentState, m02) == 16 && offsetof(AgentState, m20) == 20
              && offsetof(AgentState, m22) == 24 && offsetof(AgentState, pitch) == 28 && offsetof(AgentState, hvx) == 32 && offsetof(AgentState, hvz) == 36
              && offsetof(AgentState, vvel) == 40, "state observations: columns 0..10 are AgentState's words 0..10");

static_assert(offsetof(EnvHeader, episode_len) == offsetof(EnvHeader, episode_sec) + 4, "state observations: columns 12, 13 are adjacent words of EnvHeader");

// column f (0..15) of one agent's row, as its 32 bits.  One load from the agent's record for every column (the columns that are not the agent's load a word
// they do not use: the lanes of a wave stay together), a second one from the header for columns 12 and 13; bytes are moved, not floats.
__host__ __device__ inline uint32_t state_obs_word(const AgentState *a, const EnvHeader *h, int f)
{
    const int at = f <= 10 ? 4 * f : f == 11 ? (int)offsetof(AgentState, carrying) : (int)offsetof(AgentState, total_reward);
    uint32_t w;
    __builtin_memcpy(&w, (const char *)a + at, sizeof w);
    if (f == 11) w = (int32_t)w >= 0 ? 0x3f800000u : 0u;   // carrying >= 0 ? 1.0f : +0.0f
    if (f == 12 || f == 13) __builtin_memcpy(&w, (const char *)h + offsetof(EnvHeader, episode_sec) + 4 * (f - 12), sizeof w);
    if (f == 15) w = 0u;
    return w;
}

// one agent's row
__host__ __device__ inline void state_obs_pack(const AgentState *a, const EnvHeader *h, uint32_t *out16)
{
    for (int f = 0; f < STATE_OBS_FLOATS; ++f) out16[f] = state_obs_word(a, h, f);
}

}  // namespace mv
