// megaverse_amd/csrc/mv_tick_boxagone.h -- the BoxAGone tick as a device function (namespace mv::tick_boxagone), for the scenario's step kernels
// (mv_step_boxagone.hip).  Not in the union kernels: a group refuses BoxAGone members (mv_api_step.hip: mv_group_create).
//
// Replaces, per env (reference paths relative to src/libs):
//   Env::step                                   env/src/env.cpp:83-152            (shared pieces: mv_physics.h)
//   BoxAGoneScenario::step                      scenarios/src/scenario_box_a_gone.cpp:97-168
//   BoxAGoneScenario::addDisappearingPlatforms  scenario_box_a_gone.cpp:187-233     (drawing: mv_frame.h, the same world-space records as the Hex scenarios)
//   BoxAGoneScenario::trueObjective             scenarios/include/scenarios/scenario_box_a_gone.hpp:64-80
//   Scenario::rewardTeam / doneWithTimer        env/include/env/scenario.hpp:114-117,259-307 (teamAffinity(i) = i: every agent is a team of one)
//   VectorEnv::step done bookkeeping + Env::reset of finished envs (env/src/vector_env.cpp:93-105): the swap-in below takes the episode the host
//   generator (mv_gen_boxagone.cpp) left resident in HBM.
//
// One wavefront per env, NC = 2 colliders per lane: k = 0 the room's merged slabs (lanes 0..7); k = 1 what is near the agent being stepped -- the
// 3 x 3 cells around it on every level (lanes 0..26, through the cell map: a present platform is a box), every temporary platform that stands
// somewhere (lanes 27..50) -- and the other agents' capsules (lanes 51..58).  Slot order (lane + 64 k) is the reference's collision-object order
// (room, platforms in generation order, temporary platforms, agents), which decides sweep ties and which penetration is recovered first.  A capsule moves less than a cell per tick (<= 0.3 horizontally) and a
// platform, grown or not, reaches at most 1.03 from its cell's centre: nothing outside those cells can be touched.
// The platforms' state -- the reference's std::map<RigidBody *, PlatformState> and std::deque of temporary platforms -- is BoxAGoneState
// (mv_types.h): the scenario logic runs on lane 0, agent by agent, as the reference does; the timers then count down 16 platforms per lane.
// FallDetectionComponent (scenario_box_a_gone.cpp:34) is not restated: the room's walls are closed, so no agent can fall out of it -- and if one
// did, the reference would read its empty agentInitialPositions.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mv_actions.h"
#include "mv_agents.h"
#include "mv_frame.h"
#include "mv_math.h"
#include "mv_physics.h"
#include "mv_types.h"

namespace mv {
namespace tick_boxagone {

constexpr int NC = 2;
constexpr float VOXEL = 2.0f;                               // BoxAGoneScenario::voxelSize (scenario_box_a_gone.hpp:114)
constexpr float PLAT_HXZ = 0.42f * VOXEL;                   // objSize: a platform is btBoxShape(1, 1, 1) scaled by (objSize, objSize * 0.045, objSize)
constexpr float PLAT_HY = PLAT_HXZ * 0.045f;                //   (scenario_box_a_gone.cpp:189-191)
constexpr float AWAY = 300.0f * VOXEL;                      // "basically remove from the scene" (:137, :150)
constexpr int TEMP_TICKS = 15;                              // PlatformState::remainingTicks of a new state (:126)
constexpr int NEAR_LANES = 27, TEMP_LANE0 = 27, CAP_LANE0 = TEMP_LANE0 + BAG_MAX_TEMPS;
static_assert(CAP_LANE0 + MAX_AGENTS <= 64, "BoxAGone: the capsules' lanes");
__device__ constexpr unsigned LEVEL_COLORS[3] = {0xffb400u, 0x2eb5d0u, 0xd468eeu};   // ORANGE, BLUE, VIOLET (:63)
constexpr unsigned GREEN = 0x3bb372u, LAYOUT_WHITE = 0xffffffu;                      // env/const.hpp:26-51

__device__ __forceinline__ V3 platform_centre(const BagPlatform p)
{
    return v3((float(p.x) + 0.5f) * VOXEL, (float(p.y) + 0.5f) * VOXEL, (float(p.z) + 0.5f) * VOXEL);
}
__device__ __forceinline__ HexRec box_rec(V3 c, float sxz, float sy, unsigned color)
{
    HexRec r;
    r.a[0] = c.x - sxz; r.a[1] = c.y - sy; r.a[2] = c.z - sxz; r.meta = 1 << 4;   // world frame, collides
    r.b[0] = c.x + sxz; r.b[1] = c.y + sy; r.b[2] = c.z + sxz; r.color = (int)color;
    return r;
}
// where temporary platform t stands: on the platform it took the place of last, or where addDisappearingPlatforms put it; + AWAY per expiry since
__device__ __forceinline__ V3 temp_centre(const BoxAGoneState *st, const BagTemp t)
{
    V3 c = t.plat >= 0 ? platform_centre(st->plat[t.plat]) : v3(AWAY, AWAY, AWAY);
    for (int k = 0; k < t.away; ++k) c = v3(c.x + AWAY, c.y + AWAY, c.z + AWAY);
    return c;
}
__device__ __forceinline__ void box_col(Col &c, const HexRec &r)
{
    c.kind = 1;
    c.lo = v3(r.a[0], r.a[1] - CAP_HH, r.a[2]);
    c.hi = v3(r.b[0], r.b[1] + CAP_HH, r.b[2]);
}

// Episode swap-in: Env::reset of one env from its resident BoxAGoneBlob (called by the env's whole wavefront)
__device__ __forceinline__ void swap_in_episode(const GymView &gv, const BoxAGoneBlob *blobs, int *status, int env, int force_all)
{
    const int lane = lane_id();
    EnvHeader *gh = gv.hdr + env;
    const int consumed = gh->episodes_consumed;
    const BoxAGoneBlob *b = blobs + (size_t)env * gv.spares + consumed % gv.spares;   // ring slot of episode number consumed + 1
    if (b->seq != consumed + 1) {   // the host has not delivered the next episode (mv_api.hip keeps it ahead): reported, recovered
        if (lane == 0) { gh->starved |= 1; atomicOr(&status[gv.num_envs + 1], (int)ST_STARVED); }
        return;
    }
    const int A = gv.num_agents, nb = b->num_boxes, np = b->num_platforms, nt = 3 * A;
    BoxAGoneState *st = gv.bag + env;
    HexRec *recs = gv.hex_boxes + (size_t)env * HEX_MAX_BOXES;
    // the cell map: cleared, then (below, behind a wave_sync) every platform's cell
    {
        uint4 *cm = reinterpret_cast<uint4 *>(&st->cell[0][0][0]);
        for (int i = lane; i < (int)(sizeof st->cell / 16); i += 64) cm[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    for (int i = lane; i < BAG_TABLE; i += 64) {
        BagPlatform p = BagPlatform{0, 0, 0, 0};
        if (i < np) {
            p = b->platforms[i];
            recs[nb + i] = box_rec(platform_centre(p), PLAT_HXZ, PLAT_HY, LEVEL_COLORS[p.state % 3]);
        }
        st->plat[i] = p;   // (state = level | BAG_PRESENT << 4)
    }
    for (int i = lane; i < BAG_TABLE / 16; i += 64) {
        reinterpret_cast<uint4 *>(st->ticks)[i] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4 *>(st->tslot)[i] = make_uint4(0, 0, 0, 0);
    }
    if (lane < nb) {   // the room's slabs, scaled by the voxel size (addDrawablesAndCollisionObjectsFromVoxelGrid)
        const LayoutBox lb = b->boxes[lane];
        HexRec r;
        r.a[0] = float(lb.min[0]) * VOXEL; r.a[1] = float(lb.min[1]) * VOXEL; r.a[2] = float(lb.min[2]) * VOXEL; r.meta = 1 << 4;
        r.b[0] = float(lb.max[0]) * VOXEL; r.b[1] = float(lb.max[1]) * VOXEL; r.b[2] = float(lb.max[2]) * VOXEL; r.color = (int)LAYOUT_WHITE;
        recs[lane] = r;
    }
    if (lane < nt) {   // the temporary platforms: 600 away, at the platforms' scale (:220-231)
        BagTemp t;
        t.plat = -1; t.away = 0; t.sxz = PLAT_HXZ; t.sy = PLAT_HY;
        st->temps[lane] = t;
        recs[nb + np + lane] = box_rec(v3(AWAY, AWAY, AWAY), PLAT_HXZ, PLAT_HY, GREEN);
    }
    if (lane < MAX_AGENTS) { st->sec_before[lane] = 0.0f; st->last_platform[lane] = -1; }
    if (lane == 0) {
        st->num_platforms = np; st->num_levels = b->num_levels; st->takes = 0; st->finished = 0;
        for (int k = 0; k < 4; ++k) st->level_y[k] = b->level_y[k];
    }
    wave_sync();
    for (int i = lane; i < np; i += 64) {
        const BagPlatform p = b->platforms[i];
        st->cell[p.state][p.x][p.z] = (int16_t)i;
    }
    for (int k = 0; k < A; ++k) {
        float cs, sn;
        yaw_matrix(b->yaw_frand[k] * 3.14159274f * 2, cs, sn);
        if (lane == 0) {
            AgentState *a = gv.agents + (size_t)env * A + k;
            const float sx = b->spawn[k][0], sy = b->spawn[k][1], sz = b->spawn[k][2];   // agentStartingPositions: cell centres * voxel size
            a->pos[0] = sx + 0.5f; a->pos[1] = sy + 0.0f + 1.75f; a->pos[2] = sz + 0.5f;
            a->m00 = cs; a->m02 = sn; a->m20 = -sn; a->m22 = cs;
            a->pitch = 0.0f; a->hvx = 0.0f; a->hvz = 0.0f; a->vvel = 0.0f; a->voffset = 0.0f; a->step_offset = 0.0f;
            a->jump_speed = 10.0f; a->was_jumping = 0; a->carrying = -1; a->picked_up = 0; a->visited_zone = 0;
            a->spawn[0] = (int)floorf(sx); a->spawn[1] = (int)floorf(sy); a->spawn[2] = (int)floorf(sz);
            a->last_reward = 0.0f; a->total_reward = 0.0f;
            gv.rewards[(size_t)env * A + k] = 0.0f;
            gv.actions[(size_t)env * A + k] = 0;
        }
    }
    if (lane == 0) {
        gh->L = BAG_ROOM; gh->H = 8; gh->W = BAG_ROOM;
        gh->bz[0] = gh->bz[1] = gh->bz[2] = gh->bz[3] = 0;
        gh->layout_color = (int)LAYOUT_WHITE; gh->wall_color = (int)LAYOUT_WHITE; gh->draw_walls = 1;
        gh->num_objects = 0; gh->num_boxes = nb + np + nt; gh->num_terrain = nb; gh->num_rewards = 0; gh->num_platforms = np;
        gh->num_frames = 0; gh->done = 0; gh->highest_tower = 0; gh->solved = 0;
        gh->episode_sec = 0.0f; gh->episode_len = b->episode_len; gh->bz_reward = 0.0f; gh->bar_half_width = 0.24f;
        gh->episodes_consumed = consumed + 1;
        status[env] = consumed + 1;
        atomicAdd(&status[gv.num_envs], 1);
        if (force_all) gv.done[env] = 0;
    }
}

template <int A_MAX>
__device__ __forceinline__ void boxagone_tick(const GymView &gv, const int env)
{
    const int lane = lane_id();
    if (env >= gv.num_envs) return;
    const int A = gv.num_agents, nt = 3 * A;

    // ---- header fields as scalars (never copy the record: see mv_step.hip)
    EnvHeader *gh = gv.hdr + env;
    const int nb = gh->num_terrain, np = gh->num_platforms;
    int numFrames = gh->num_frames, done = gh->done;
    float episodeSec = gh->episode_sec;
    const float episodeLen = gh->episode_len, lookLimit = gh->p_vertical_look_limit;
    BoxAGoneState *st = gv.bag + env;
    HexRec *recs = gv.hex_boxes + (size_t)env * HEX_MAX_BOXES;

    // ---- wave-resident scene: the room's slabs (k = 0, lanes < nb); per agent below: what is near, then the capsules (k = 1)
    Col col[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) { col[k].kind = 0; col[k].lo = col[k].hi = v3(0, 0, 0); }
    if (lane < nb) box_col(col[0], recs[lane]);

    // ---- agents: records in LDS (mv_agents.h), one agent's physics fields in registers at a time
    __shared__ AgentState s_ag[A_MAX];
    __shared__ int s_act[A_MAX];
    __shared__ int s_grow[BAG_MAX_TEMPS], s_away[BAG_MAX_TEMPS];
    agents_load(gv, env, A, s_ag, s_act);
    const float dt = DT;
    if (lane < A) {   // actions -> intents: agents are independent here, one lane each
        AgentState a;
        phys_load(a, s_ag[lane]);
        apply_actions(a, s_act[lane], dt, lookLimit);
        phys_store(s_ag[lane], a);
    }
    if (lane < BAG_MAX_TEMPS) { s_grow[lane] = 0; s_away[lane] = 0; }
    wave_sync();

    // ---- physics, agent by agent (nothing moves but the agents during this phase)
#pragma unroll 1
    for (int i = 0; i < A; ++i) {
        col[1].kind = 0;
        if (lane < NEAR_LANES) {   // the 3 x 3 cells around the agent on every level: present platforms
            const int level = lane / 9, cx = (int)floorf(s_ag[i].pos[0] / VOXEL) + (lane % 9) / 3 - 1, cz = (int)floorf(s_ag[i].pos[2] / VOXEL) + lane % 3 - 1;
            if (level < BAG_MAX_LEVELS && cx >= 0 && cx < BAG_ROOM && cz >= 0 && cz < BAG_ROOM) {
                const int p = st->cell[level][cx][cz];
                if (p >= 0) {
                    const BagPlatform bp = st->plat[p];
                    if ((bp.state >> 4) == BAG_PRESENT) box_col(col[1], recs[nb + p]);
                }
            }
        } else if (lane < TEMP_LANE0 + nt) {   // temporary platforms that stand on a platform's cell
            const BagTemp t = st->temps[lane - TEMP_LANE0];
            if (t.plat >= 0 && t.away == 0) box_col(col[1], recs[nb + np + (lane - TEMP_LANE0)]);
        } else if (A_MAX > 1 && lane >= CAP_LANE0 && lane < CAP_LANE0 + A) {   // the other agents' capsules
            const int j = lane - CAP_LANE0;
            if (j != i) {
                col[1].kind = 2;
                col[1].lo = v3(s_ag[j].pos[0], s_ag[j].pos[1], s_ag[j].pos[2]);
                col[1].hi = v3(2 * CAP_HH, 0.0f, 0.0f);
            }
        }
        AgentState a;
        phys_load(a, s_ag[i]);
        player_step<NC>(a, col, dt);
        if (lane == 0) phys_store(s_ag[i], a);
        wave_sync();
    }

    // ---- BoxAGoneScenario::step, agent by agent (scenario_box_a_gone.cpp:99-143): rewards on every agent's lane, the platform logic on lane 0
    int touching = 0;
#pragma unroll 1
    for (int i = 0; i < A; ++i) {
        const float tx = s_ag[i].pos[0], ty = s_ag[i].pos[1] + 0.05f, tz = s_ag[i].pos[2];   // the agent's translation
        const int cx = (int)floorf(tx / VOXEL), cy = (int)floorf(ty / VOXEL), cz = (int)floorf(tz / VOXEL);
        const bool touchesFloor = cy < 3;
        touching += touchesFloor ? 1 : 0;
        if (lane == i) {   // rewardTeam(key, i, 1) with a team of one
            const int key = touchesFloor ? 1 : 2;   // boxagoneTouchedFloor / boxagonePerStepReward
            s_ag[i].last_reward += s_ag[i].shaping[key] * (1.0f * (1 - s_ag[i].shaping[0]));
            s_ag[i].last_reward += s_ag[i].shaping[key] * s_ag[i].shaping[0] * 1.0f / float(1);
        }
        if (lane == 0) {
            if (!touchesFloor) st->sec_before[i] = episodeSec;
            // vg.grid.get(coords): a platform's voxel until its timer has run out
            int p = -1;
            for (int l = 0; l < st->num_levels; ++l)
                if (st->level_y[l] == cy && cx >= 0 && cx < BAG_ROOM && cz >= 0 && cz < BAG_ROOM) p = st->cell[l][cx][cz];
            AgentState a;
            phys_load(a, s_ag[i]);
            if (p >= 0 && (st->plat[p].state >> 4) != BAG_REMOVED && on_ground(a) && p != st->last_platform[i]) {
                const int lp = st->last_platform[i];
                if (lp >= 0 && st->ticks[lp] > 0) st->ticks[lp] = (uint8_t)min((int)st->ticks[lp], 3);
                if ((st->plat[p].state >> 4) == BAG_PRESENT) {   // a new PlatformState: the back of the deque goes to its front
                    const int takes = st->takes, slot = nt - 1 - takes % nt;
                    st->takes = takes + 1;
                    st->ticks[p] = (uint8_t)TEMP_TICKS;
                    st->tslot[p] = (uint8_t)slot;
                    BagPlatform bp = st->plat[p];
                    bp.state = (int8_t)((bp.state & 15) | (BAG_VISITED << 4));
                    st->plat[p] = bp;
                    BagTemp t;
                    t.plat = p; t.away = 0; t.sxz = PLAT_HXZ * 1.05f; t.sy = PLAT_HY * 1.05f;
                    st->temps[slot] = t;
                    const V3 c = platform_centre(bp);   // the platform itself: translated away
                    recs[nb + p] = box_rec(v3(c.x + AWAY, c.y + AWAY, c.z + AWAY), PLAT_HXZ, PLAT_HY, LEVEL_COLORS[(bp.state & 15) % 3]);
                }
                st->last_platform[i] = p;
            }
        }
        wave_sync();
    }
    wave_sync();   // lane 0's table stores before every lane's loads

    // ---- the timers (:145-166), 16 platforms per lane: every live state counts down; at 0 its temporary platform is sent away and its cell leaves
    // the grid, in its last 5 ticks the temporary platform grows by 1.03 (per state that holds it: a re-used one can be held by two)
    if (lane < BAG_TABLE / 16 && lane * 16 < np) {
        uint4 tk = reinterpret_cast<const uint4 *>(st->ticks)[lane];
        if (tk.x | tk.y | tk.z | tk.w) {
            const uint4 ts = reinterpret_cast<const uint4 *>(st->tslot)[lane];
            unsigned w[4] = {tk.x, tk.y, tk.z, tk.w};
            const unsigned s4[4] = {ts.x, ts.y, ts.z, ts.w};
            for (int q = 0; q < 16; ++q) {
                const unsigned t = (w[q >> 2] >> (8 * (q & 3))) & 255u;
                if (!t) continue;
                const int slot = (int)((s4[q >> 2] >> (8 * (q & 3))) & 255u);
                const unsigned nt1 = t - 1;
                w[q >> 2] = (w[q >> 2] & ~(255u << (8 * (q & 3)))) | (nt1 << (8 * (q & 3)));
                if (nt1 == 0) {
                    atomicAdd(&s_away[slot], 1);
                    const int p = lane * 16 + q;
                    BagPlatform bp = st->plat[p];
                    bp.state = (int8_t)((bp.state & 15) | (BAG_REMOVED << 4));
                    st->plat[p] = bp;
                } else if (nt1 <= 5) atomicAdd(&s_grow[slot], 1);
            }
            reinterpret_cast<uint4 *>(st->ticks)[lane] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    wave_sync();
    if (lane < nt) {   // every temporary platform's record: where it stands, its scale (the tick's placements and growth)
        BagTemp t = st->temps[lane];
        for (int g = 0; g < s_grow[lane]; ++g) { t.sxz = t.sxz * 1.03f; t.sy = t.sy * 1.03f; }
        t.away += s_away[lane];
        st->temps[lane] = t;
        recs[nb + np + lane] = box_rec(temp_centre(st, t), t.sxz, t.sy, GREEN);
    }

    // ---- every agent on the floor: doneWithTimer(), once (:167-170); timers / done
    int finished = st->finished;
    if (touching >= A && !finished) {
        finished = 1;
        episodeSec = fmax_sel(episodeSec, episodeLen - 0.3f);
    }
    episodeSec += dt;
    const float bar = fmax_sel(0.0f, (episodeLen - episodeSec) / episodeLen) * 0.24f;
    if (episodeSec >= episodeLen) done = 1;
    ++numFrames;

    // ---- write back
    if (lane == 0) {
        st->finished = finished;
        gh->num_frames = numFrames; gh->done = done; gh->solved = finished;
        gh->episode_sec = episodeSec; gh->bar_half_width = bar;
        gv.done[env] = (uint8_t)done;
    }
    agents_store(gv, env, A, s_ag);
    if (done && lane < A) {   // trueObjective (scenario_box_a_gone.hpp:64-80): one agent -- the fraction of the episode above the floor; several -- the
                              // last one standing (the first with the largest secondsBeforeTouchedFloor) gets 1
        float obj;
        if (A > 1) {
            float best = 0.0f;
            int bestAgent = 0;
            for (int j = 0; j < A; ++j)
                if (st->sec_before[j] > best) { bestAgent = j; best = st->sec_before[j]; }
            obj = lane == bestAgent ? 1.0f : 0.0f;
        } else obj = st->sec_before[0] / gh->p_episode_len_sec;
        gv.true_objective[(size_t)env * A + lane] = obj;
    }

    // ---- the auto-reset of VectorEnv::step: the wave of a finished env swaps the next episode in right here
    if (done) {
        wave_sync();   // one wave per env: orders the stores above before the swap-in's
        swap_in_episode(gv, static_cast<const BoxAGoneBlob *>(gv.blobs), gv.episode_status, env, 0);
    }
}

// the step and reset kernels' view of the scenario (mv_step_kernels.h)
struct Scenario {
    static constexpr bool long_lists = true, par_agents = false;
    template <int A_MAX> __device__ __forceinline__ static void tick(const GymView &gv, int env) { boxagone_tick<A_MAX>(gv, env); }
    __device__ __forceinline__ static void swap_in(const GymView &gv, int env, int force_all)
    {
        swap_in_episode(gv, static_cast<const BoxAGoneBlob *>(gv.blobs), gv.episode_status, env, force_all);
    }
};

}  // namespace tick_boxagone
}  // namespace mv
