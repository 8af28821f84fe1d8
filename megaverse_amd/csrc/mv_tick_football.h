// megaverse_amd/csrc/mv_tick_football.h -- the Football tick as a device function (namespace mv::tick_football), for the scenario's step kernels
// (mv_step_football.hip).  Not in the union kernels: a group refuses Football members (mv_api_step.hip: mv_group_create).
//
// Replaces, per env (reference paths relative to src/libs):
//   Env::step                                   env/src/env.cpp:83-152            (shared pieces: mv_physics.h)
//   btDiscreteDynamicsWorld::stepSimulation     [3P] Bullet 2.89, for the one dynamic body: the ball -- restated as a STATED sequential-impulse model
//                                               (DESIGN.md section 7), not Bullet's bits
//   FootballScenario::step                      scenarios/src/scenario_football.cpp:143-163 (the kicks)
//   FootballScenario::addEpisodeDrawables       scenario_football.cpp:131-141 (drawing: mv_frame.h, world-space HexRec records like the Hex scenarios')
//   VectorEnv::step done bookkeeping + Env::reset of finished envs (env/src/vector_env.cpp:93-105): the swap-in below takes the episode the host
//   generator (mv_gen_football.cpp) left resident in HBM.
//
// One wavefront per env.  stepSimulation's order: the ball first (velocity, contacts at the start pose, the solver, the pose: lane 0, contact after
// contact as the solver does), then the agents' controllers, agent by agent, against the ball's NEW pose.  NC = 1 collider per lane, slot = lane in
// the reference's collision-object order (Env::reset: the ball in FootballScenario::reset, the agents in spawnAgents, the room's boxes in
// addEpisodeDrawables): lane 0 the ball (a sphere collider, mv_physics.h: COL_BALL), lanes 1..8 the other agents' capsules, lanes 9.. the room's boxes.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

#include "mv_actions.h"
#include "mv_agents.h"
#include "mv_frame.h"
#include "mv_math.h"
#include "mv_physics.h"
#include "mv_types.h"

namespace mv {
namespace tick_football {

constexpr int NC = 1;
constexpr int CAP_LANE0 = 1, BOX_LANE0 = 1 + MAX_AGENTS, MAX_CONTACTS = MAX_AGENTS + FB_MAX_LAYOUT;
static_assert(BOX_LANE0 + FB_MAX_LAYOUT <= 64, "Football: the colliders' lanes");
constexpr unsigned ORANGE = 0xffb400u, LAYOUT_WHITE = 0xffffffu;   // env/const.hpp:26-51

// ---- the ball model ([3P, from memory]: Bullet 2.89's defaults as the reference leaves them)
constexpr float BALL_R = 1.0f;                  // btSphereShape(2.0) scaled by 0.5 (syncPose)
constexpr float BALL_X0 = 5.0f, BALL_Y0 = 5.0f, BALL_Z0 = 5.0f;
constexpr float BALL_G = -10.0f;                // btDiscreteDynamicsWorld's default gravity, (0, -10, 0)
constexpr float BALL_I = 1.6f;                  // 2/5 m r^2 of the UNSCALED shape (radius 2): calculateLocalInertia runs before the scaling
constexpr float BALL_INV_I = 1.0f / BALL_I;     // (mass 1: the inverse mass is 1 and is left out)
constexpr float BALL_MU = 0.5f * 0.5f;          // combined friction: ball 0.5 x box / capsule 0.5 (btManifoldResult::calculateCombinedFriction)
constexpr float BALL_MU_ROLL = 0.1f * 0.5f;     // combined rolling friction: 0.1 x 0.5 + 0 x 0.5 (calculateCombinedRollingFriction)
constexpr float BALL_MU_SPIN = 0.1f * 0.5f;     // combined spinning friction: the same rule
constexpr float BALL_BREAK = 0.02f;             // contact breaking threshold (gContactBreakingThreshold)
constexpr float BALL_ERP = 0.2f, BALL_ERP2 = 0.8f, BALL_SPLIT = -0.04f;   // btContactSolverInfo: m_erp, m_erp2, m_splitImpulsePenetrationThreshold
constexpr int BALL_ITERS = 10;                  // btContactSolverInfo::m_numIterations
constexpr float BALL_CAP_R = BALL_R + CAP_R;    // ball against an agent's capsule: the sum of the radii
constexpr float PLANE_SQRT12 = 0.7071067811865475244f;   // SIMDSQRT12 (btPlaneSpace1)
constexpr float KICK_DIST = 1.8f, KICK_FORCE = 70.0f;   // scenario_football.cpp:150-156

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// one contact of the ball, set up at the start pose: the normal n (from the other body to the ball) and the gap; the friction direction t, r x t
// (r = -R n: the contact point from the centre) and the row's inverse effective mass; the rolling axes p, q (btPlaneSpace1(n)); velocity targets
// of the normal row and of the split-impulse push; the accumulated impulses
struct BallContact {
    V3 n, t, rt, p, q;
    float dist, jf, bias, pbias;
    float ln, lf, lp, lr[3];
};

__device__ __forceinline__ void plane_space(V3 n, V3 &p, V3 &q)
{
    if (fabsf(n.z) > PLANE_SQRT12) {
        const float a = n.y * n.y + n.z * n.z, k = 1.0f / sqrtf(a);
        p = v3(0.0f, -n.z * k, n.y * k);
        q = v3(a * k, -n.x * p.z, n.x * p.y);
    } else {
        const float a = n.x * n.x + n.y * n.y, k = 1.0f / sqrtf(a);
        p = v3(-n.y * k, n.x * k, 0.0f);
        q = v3(-n.z * p.y, n.z * p.x, a * k);
    }
}

// the gap between the ball (centre c) and a box (unexpanded bounds) / an agent's capsule (ghost origin o); false: farther than BALL_BREAK
__device__ __forceinline__ bool ball_box(V3 c, V3 lo, V3 hi, V3 &n, float &dist)
{
    const Raw r = raw_box(c, lo, hi, BALL_R);
    dist = r.dist;
    n = r.v * (1.0f / r.d);
    return dist <= BALL_BREAK;
}
__device__ __forceinline__ bool ball_capsule(V3 c, V3 o, V3 &n, float &dist)
{
    const Raw r = raw_capsule(c, o, CAP_HH, BALL_CAP_R);
    dist = r.dist;
    n = r.v * (1.0f / r.d);
    return dist <= BALL_BREAK;
}

__device__ __forceinline__ void contact_setup(BallContact &c, V3 n, float dist, V3 v, V3 w)
{
    c.n = n; c.dist = dist;
    const V3 r = v3(-n.x, -n.y, -n.z);   // (R = 1)
    const V3 vc = v + cross(w, r);
    const V3 slip = vc - n * dot(n, vc);
    const float s2 = len2(slip);
    plane_space(n, c.p, c.q);
    if (s2 > FLT_EPSILON) c.t = slip * (1.0f / sqrtf(s2));
    else c.t = c.p;
    c.rt = cross(r, c.t);
    c.jf = 1.0f / (1.0f + BALL_INV_I * len2(c.rt));
    c.bias = dist > 0.0f ? -dist / DT : dist > BALL_SPLIT ? -dist * BALL_ERP / DT : 0.0f;
    c.pbias = dist > BALL_SPLIT ? 0.0f : -dist * BALL_ERP2 / DT;
    c.ln = 0.0f; c.lf = 0.0f; c.lp = 0.0f; c.lr[0] = 0.0f; c.lr[1] = 0.0f; c.lr[2] = 0.0f;
}

// one tick of the ball (one lane): integrate the velocity with the pending force, find the contacts at the start pose (the agents' capsules at
// their pose from the end of the previous tick, then the room's boxes), BALL_ITERS iterations of normal rows, friction rows and rolling rows,
// BALL_ITERS iterations of split-impulse pushes, then the pose.  `cs`: the contacts (LDS).
__device__ __forceinline__ void ball_step(FootballState &b, const HexRec *recs, int nb, const AgentState *s_ag, int A, BallContact *cs)
{
    V3 v = v3(b.vel[0], b.vel[1], b.vel[2]), w = v3(b.ang[0], b.ang[1], b.ang[2]);
    v = v3(v.x + (b.force[0] + 0.0f) * DT, v.y + (b.force[1] + BALL_G) * DT, v.z + (b.force[2] + 0.0f) * DT);
    b.force[0] = 0.0f; b.force[1] = 0.0f; b.force[2] = 0.0f;
    const V3 c = v3(b.pos[0], b.pos[1], b.pos[2]);
    int nc = 0, bits = 0;
    for (int j = 0; j < A; ++j) {
        V3 n; float dist;
        if (ball_capsule(c, v3(s_ag[j].pos[0], s_ag[j].pos[1], s_ag[j].pos[2]), n, dist)) { contact_setup(cs[nc++], n, dist, v, w); bits |= 1 << j; }
    }
    for (int k = 0; k < nb; ++k) {
        const HexRec r = recs[k];
        V3 n; float dist;
        if (ball_box(c, v3(r.a[0], r.a[1], r.a[2]), v3(r.b[0], r.b[1], r.b[2]), n, dist)) { contact_setup(cs[nc++], n, dist, v, w); bits |= 1 << (8 + k); }
    }
    for (int it = 0; it < BALL_ITERS; ++it) {
        for (int j = 0; j < nc; ++j) {   // normal rows: restitution 0, accumulated impulse clamped at 0
            BallContact &k = cs[j];
            const float dl = k.bias - dot(k.n, v);
            const float sum = fmax_sel(k.ln + dl, 0.0f);
            const float d = sum - k.ln;
            k.ln = sum;
            v = v + k.n * d;
        }
        for (int j = 0; j < nc; ++j) {   // friction rows: |impulse| <= mu x the contact's normal impulse
            BallContact &k = cs[j];
            if (!(k.ln > 0.0f)) continue;
            const float lim = BALL_MU * k.ln;
            const float vt = dot(k.t, v) + dot(k.rt, w);
            const float sum = fmin_sel(fmax_sel(k.lf + (0.0f - vt * k.jf), -lim), lim);
            const float d = sum - k.lf;
            k.lf = sum;
            v = v + k.t * d;
            w = w + k.rt * (BALL_INV_I * d);
        }
        for (int j = 0; j < nc; ++j) {   // spinning (about n) and rolling (about p, q) rows: |impulse| <= min(mu_r x normal impulse, mu_r)
            BallContact &k = cs[j];
            if (!(k.ln > 0.0f)) continue;
            for (int a = 0; a < 3; ++a) {
                const V3 ax = a == 0 ? k.n : a == 1 ? k.p : k.q;
                const float mu = a == 0 ? BALL_MU_SPIN : BALL_MU_ROLL;
                const float lim = fmin_sel(mu * k.ln, mu);
                const float va = dot(ax, w);
                const float sum = fmin_sel(fmax_sel(k.lr[a] + (0.0f - va * BALL_I), -lim), lim);
                const float d = sum - k.lr[a];
                k.lr[a] = sum;
                w = w + ax * (BALL_INV_I * d);
            }
        }
    }
    V3 vp = v3(0.0f, 0.0f, 0.0f);
    for (int it = 0; it < BALL_ITERS; ++it)
        for (int j = 0; j < nc; ++j) {   // split-impulse pushes of the deep contacts: position only
            BallContact &k = cs[j];
            if (!(k.pbias > 0.0f)) continue;
            const float dl = k.pbias - dot(k.n, vp);
            const float sum = fmax_sel(k.lp + dl, 0.0f);
            const float d = sum - k.lp;
            k.lp = sum;
            vp = vp + k.n * d;
        }
    const V3 p = v3((c.x + vp.x * DT) + v.x * DT, (c.y + vp.y * DT) + v.y * DT, (c.z + vp.z * DT) + v.z * DT);
    b.pos[0] = p.x; b.pos[1] = p.y; b.pos[2] = p.z;
    b.vel[0] = v.x; b.vel[1] = v.y; b.vel[2] = v.z;
    b.ang[0] = w.x; b.ang[1] = w.y; b.ang[2] = w.z;
    b.contacts = bits;
    b.radius = BALL_R;   // MotionState::setWorldTransform rebuilt the transformation without the 0.5 scale
}

__device__ __forceinline__ HexRec ball_rec(const FootballState &b)
{
    HexRec r;
    r.a[0] = b.pos[0]; r.a[1] = b.pos[1]; r.a[2] = b.pos[2]; r.meta = HEX_SPHERE;
    r.b[0] = b.radius; r.b[1] = b.radius; r.b[2] = b.radius; r.color = (int)ORANGE;
    return r;
}
__device__ __forceinline__ void box_col(Col &c, const HexRec &r)
{
    c.kind = 1;
    c.lo = v3(r.a[0], r.a[1] - CAP_HH, r.a[2]);
    c.hi = v3(r.b[0], r.b[1] + CAP_HH, r.b[2]);
}

// Episode swap-in: Env::reset of one env from its resident FootballBlob (called by the env's whole wavefront)
__device__ __forceinline__ void swap_in_episode(const GymView &gv, const FootballBlob *blobs, int *status, int env, int force_all)
{
    const int lane = lane_id();
    EnvHeader *gh = gv.hdr + env;
    const int consumed = gh->episodes_consumed;
    const FootballBlob *b = blobs + (size_t)env * gv.spares + consumed % gv.spares;   // ring slot of episode number consumed + 1
    if (b->seq != consumed + 1) {   // the host has not delivered the next episode (mv_api.hip keeps it ahead): reported, recovered
        if (lane == 0) { gh->starved |= 1; atomicOr(&status[gv.num_envs + 1], (int)ST_STARVED); }
        return;
    }
    const int A = gv.num_agents, nb = b->num_boxes;
    HexRec *recs = gv.hex_boxes + (size_t)env * HEX_MAX_BOXES;
    if (lane < nb) {   // the room's slabs at voxel size 1 (addDrawablesAndCollisionObjectsFromVoxelGrid)
        const LayoutBox lb = b->boxes[lane];
        HexRec r;
        r.a[0] = float(lb.min[0]); r.a[1] = float(lb.min[1]); r.a[2] = float(lb.min[2]); r.meta = 1 << 4;   // world frame, collides
        r.b[0] = float(lb.max[0]); r.b[1] = float(lb.max[1]); r.b[2] = float(lb.max[2]); r.color = (int)LAYOUT_WHITE;
        recs[lane] = r;
    }
    if (lane == 0) {   // the ball at rest at (5, 5, 5), no pending force; drawn at its 0.5 scale until the first tick
        FootballState s;
        s.pos[0] = BALL_X0; s.pos[1] = BALL_Y0; s.pos[2] = BALL_Z0; s.radius = 0.5f;
        s.vel[0] = 0.0f; s.vel[1] = 0.0f; s.vel[2] = 0.0f; s.kicks = 0;
        s.ang[0] = 0.0f; s.ang[1] = 0.0f; s.ang[2] = 0.0f; s.contacts = 0;
        s.force[0] = 0.0f; s.force[1] = 0.0f; s.force[2] = 0.0f; s.pad = 0;
        gv.fb[env] = s;
        gv.hex_objs[(size_t)env * HEX_MAX_OBJS] = ball_rec(s);
    }
    for (int k = 0; k < A; ++k) {
        float cs, sn;
        yaw_matrix(b->yaw_frand[k] * 3.14159274f * 2, cs, sn);
        if (lane == 0) {
            AgentState *a = gv.agents + (size_t)env * A + k;
            const float sx = b->spawn[k][0], sy = b->spawn[k][1], sz = b->spawn[k][2];
            a->pos[0] = sx + 0.5f; a->pos[1] = sy + 0.0f + 1.75f; a->pos[2] = sz + 0.5f;   // scenario_default.hpp:89, agent.cpp:45
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
        gh->L = b->length; gh->H = b->height; gh->W = b->width;
        gh->bz[0] = gh->bz[1] = gh->bz[2] = gh->bz[3] = 0;
        gh->layout_color = (int)LAYOUT_WHITE; gh->wall_color = (int)LAYOUT_WHITE; gh->draw_walls = 1;
        gh->num_objects = 0; gh->num_boxes = nb; gh->num_terrain = nb; gh->num_rewards = 1; gh->num_platforms = 0;
        gh->num_frames = 0; gh->done = 0; gh->highest_tower = 0; gh->solved = 0;
        gh->episode_sec = 0.0f; gh->episode_len = b->episode_len; gh->bz_reward = 0.0f; gh->bar_half_width = 0.24f;
        gh->episodes_consumed = consumed + 1;
        status[env] = consumed + 1;
        atomicAdd(&status[gv.num_envs], 1);
        if (force_all) gv.done[env] = 0;
    }
}

template <int A_MAX>
__device__ __forceinline__ void football_tick(const GymView &gv, const int env)
{
    const int lane = lane_id();
    if (env >= gv.num_envs) return;
    const int A = gv.num_agents;

    // ---- header fields as scalars (never copy the record: see mv_step.hip)
    EnvHeader *gh = gv.hdr + env;
    const int nb = gh->num_terrain;
    int numFrames = gh->num_frames, done = gh->done;
    float episodeSec = gh->episode_sec;
    const float episodeLen = gh->episode_len, lookLimit = gh->p_vertical_look_limit;
    FootballState *fs = gv.fb + env;
    HexRec *recs = gv.hex_boxes + (size_t)env * HEX_MAX_BOXES;

    __shared__ AgentState s_ag[A_MAX];
    __shared__ int s_act[A_MAX];
    __shared__ BallContact s_ct[MAX_CONTACTS];
    __shared__ float s_ball[3];
    agents_load(gv, env, A, s_ag, s_act);
    const float dt = DT;
    if (lane < A) {   // actions -> intents: agents are independent here, one lane each
        AgentState a;
        phys_load(a, s_ag[lane]);
        apply_actions(a, s_act[lane], dt, lookLimit);
        phys_store(s_ag[lane], a);
    }
    wave_sync();

    // ---- the ball's dynamics: the first part of stepSimulation (one lane)
    FootballState ball;
    if (lane == 0) {
        ball = *fs;
        ball_step(ball, recs, nb, s_ag, A, s_ct);
        s_ball[0] = ball.pos[0]; s_ball[1] = ball.pos[1]; s_ball[2] = ball.pos[2];
    }
    wave_sync();

    // ---- the agents' controllers against the ball's new pose, agent by agent
    Col col[NC];
    col[0].kind = 0; col[0].lo = col[0].hi = v3(0, 0, 0);
    if (lane == 0) { col[0].kind = COL_BALL; col[0].lo = v3(s_ball[0], s_ball[1], s_ball[2]); col[0].hi = v3(CAP_HH, CAP_R + BALL_R, 0.0f); }
    else if (lane >= BOX_LANE0 && lane < BOX_LANE0 + nb) box_col(col[0], recs[lane - BOX_LANE0]);
#pragma unroll 1
    for (int i = 0; i < A; ++i) {
        if (lane >= CAP_LANE0 && lane < CAP_LANE0 + MAX_AGENTS) {   // the other agents' capsules
            const int j = lane - CAP_LANE0;
            col[0].kind = 0;
            if (A_MAX > 1 && j < A && j != i) {
                col[0].kind = 2;
                col[0].lo = v3(s_ag[j].pos[0], s_ag[j].pos[1], s_ag[j].pos[2]);
                col[0].hi = v3(2 * CAP_HH, 0.0f, 0.0f);
            }
        }
        AgentState a;
        phys_load(a, s_ag[i]);
        player_step<NC, false, true>(a, col, dt);
        if (lane == 0) phys_store(s_ag[i], a);
        wave_sync();
    }

    // ---- FootballScenario::step: the kicks, agent by agent, at the agents' new translations (ghost origin + (0, 0.05, 0)); applied in the next tick
    if (lane == 0) {
        int kicks = 0;
        for (int i = 0; i < A; ++i) {
            if (!(s_act[i] & ACT_INTERACT)) continue;
            const V3 d = v3(ball.pos[0] - s_ag[i].pos[0], ball.pos[1] - (s_ag[i].pos[1] + 0.05f), ball.pos[2] - s_ag[i].pos[2]);
            const float len = sqrtf(len2(d));
            if (len < KICK_DIST) {
                const float inv = 1.0f / len;
                ball.force[0] = ball.force[0] + KICK_FORCE * (d.x * inv);
                ball.force[1] = ball.force[1] + KICK_FORCE * 0.5f;
                ball.force[2] = ball.force[2] + KICK_FORCE * (d.z * inv);
                ++kicks;
            }
        }
        ball.kicks = kicks;
        *fs = ball;
        gv.hex_objs[(size_t)env * HEX_MAX_OBJS] = ball_rec(ball);
    }

    // ---- timers / done: the time limit only
    episodeSec += dt;
    const float bar = fmax_sel(0.0f, (episodeLen - episodeSec) / episodeLen) * 0.24f;
    if (episodeSec >= episodeLen) done = 1;
    ++numFrames;

    // ---- write back
    if (lane == 0) {
        gh->num_frames = numFrames; gh->done = done;
        gh->episode_sec = episodeSec; gh->bar_half_width = bar;
        gv.done[env] = (uint8_t)done;
    }
    agents_store(gv, env, A, s_ag);
    if (done && lane < A) gv.true_objective[(size_t)env * A + lane] = 0.0f;   // FootballScenario::trueObjective

    // ---- the auto-reset of VectorEnv::step: the wave of a finished env swaps the next episode in right here
    if (done) {
        wave_sync();   // one wave per env: orders the stores above before the swap-in's
        swap_in_episode(gv, static_cast<const FootballBlob *>(gv.blobs), gv.episode_status, env, 0);
    }
}

// the step and reset kernels' view of the scenario (mv_step_kernels.h)
struct Scenario {
    static constexpr bool long_lists = false, par_agents = false;
    template <int A_MAX> __device__ __forceinline__ static void tick(const GymView &gv, int env) { football_tick<A_MAX>(gv, env); }
    __device__ __forceinline__ static void swap_in(const GymView &gv, int env, int force_all)
    {
        swap_in_episode(gv, static_cast<const FootballBlob *>(gv.blobs), gv.episode_status, env, force_all);
    }
};

}  // namespace tick_football
}  // namespace mv
