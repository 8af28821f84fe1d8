// megaverse_amd/csrc/mv_api_debug.hip -- test hooks of the C ABI (include/megaverse_hip.h: mv_debug_*): state snapshots in the oracle's layout, pose setters,
// the host-side episode generators and the feeder without a device, the device's RNG helpers and single fp32 operations.  Used by tests/ only.
#include "mv_api_internal.h"
#include "mv_still_frames.h"
#include "mv_tick_tower.h"

__global__ void set_agent_pos_kernel(AgentState *agents, int idx, float x, float y,
                                     float z) { agents[idx].pos[0] = x; agents[idx].pos[1] = y; agents[idx].pos[2] = z; }
__global__ void set_agent_yaw_kernel(AgentState *agents, int idx, float c,
                                     float s) { agents[idx].m00 = c; agents[idx].m02 = s; agents[idx].m20 = -s; agents[idx].m22 = c; }
__global__ void set_agent_velocity_kernel(AgentState *agents, int idx, float hvx, float hvz,
                                          float vvel) { agents[idx].hvx = hvx; agents[idx].hvz = hvz; agents[idx].vvel = vvel; }

__global__ void set_agent_pitch_kernel(AgentState *agents, int idx, float pitch) { agents[idx].pitch = pitch; }

// mv_debug_set_objects: the env's bz_reward from its records as they stand -- one wave holds them the way tower_tick does (lane l: objects l - 16 and
// 48 + l) and runs the tick's own tower_reward
__global__ void set_objects_reward_kernel(GymView gv, int env)
{
    const int lane = lane_id();
    EnvHeader *gh = gv.hdr + env;
    tick_tower::Hdr h;
    h.num_objects = gh->num_objects;
    h.bz0 = gh->bz[0]; h.bz1 = gh->bz[1]; h.bz2 = gh->bz[2]; h.bz3 = gh->bz[3];
    const MovableObject *gobj = gv.objects + (size_t)env * MAX_OBJECTS;
    const int oi[2] = {lane - 16, lane < 32 ? 48 + lane : -1};
    tick_tower::ObjRegs ob;
    for (int k = 0; k < 2; ++k) {
        ob.valid[k] = oi[k] >= 0 && oi[k] < h.num_objects;
        ob.x[k] = ob.y[k] = ob.z[k] = 0; ob.state[k] = 0;
        if (ob.valid[k]) { const MovableObject o = gobj[oi[k]]; ob.x[k] = o.x; ob.y[k] = o.y; ob.z[k] = o.z; ob.state[k] = o.state; }
    }
    const float r = tick_tower::tower_reward(h, ob);
    if (lane == 0) gh->bz_reward = r;
}

__global__ void debug_rng_kernel(uint32_t seed, int what, const int32_t *lo, const int32_t *hi, int n, void *out)
{
    __shared__ uint32_t s_mt[624];
    __shared__ uint16_t s_items[4096];
    Mt19937 g{s_mt, 624};
    mt_seed(g, seed);
    const int lane = threadIdx.x & 63;
    if (what == 0) {
        for (int i = 0; i < n; ++i) { const uint32_t v = mt_next(g); if (lane == 0) ((uint32_t *)out)[i] = v; }
    } else if (what == 1) {
        for (int i = 0; i < n; ++i) { const int v = rand_range(g, lo[i], hi[i]); if (lane == 0) ((int32_t *)out)[i] = v; }
    } else if (what == 2) {
        for (int i = 0; i < n; ++i) { const float v = frand(g); if (lane == 0) ((float *)out)[i] = v; }
    } else if (what == 3) {
        for (int i = lane; i < n; i += 64) s_items[i] = (uint16_t)i;
        __syncthreads();
        shuffle_u16(g, s_items, n);
        for (int i = lane; i < n; i += 64) ((int32_t *)out)[i] = s_items[i];
    }
}

__global__ void debug_math_kernel(int what, const float *a, const float *b, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (what == 0) out[i] = a[i] / b[i];
    else if (what == 1) out[i] = sqrtf(a[i]);
    else if (what == 2) { float s, c; sincos_poly(a[i], s, c); out[2 * i] = s; out[2 * i + 1] = c; }
    else if (what == 3) out[i] = a[i] * b[i] + a[i];   // must NOT be contracted into an fma
    else if (what == 4) out[i] = floorf(a[i]);
}

extern "C" {

// ---- test hooks ---------------------------------------------------------------------------------
#pragma pack(push, 4)
struct SnapAgent {
    float pos[3], basis[4], pitch, hv[2], vvel, voffset, step_offset, jump_speed;
    int32_t was_jumping, carrying, picked_up, visited_zone, spawn[3];
    float last_reward, total_reward, shaping[NUM_SHAPING];
};
struct Snap {
    int32_t scenario, L, H, W, bz[4], layout_color, wall_color, draw_walls, num_objects, num_boxes, num_frames, done, highest_tower,
        num_agents, num_terrain, num_rewards, num_platforms, solved;
    float episode_sec, episode_len, bz_reward, bar_half_width;
    int32_t boxes[COLLECT_MAX_BOXES][8];
    int32_t terrain[MAX_TERRAIN][8];
    int8_t objects[MAX_OBJECTS][4];
    int8_t rewards[COLLECT_MAX_REWARDS][4];
    SnapAgent agents[MAX_AGENTS];
    uint8_t chunk[CHUNK_BYTES];
    int8_t heightmap[HM_DIM * HM_DIM];
    int32_t num_items, items[MAX_ITEMS][5];
    uint8_t soko[32 * 32];   // Sokoban level cells
    int32_t hex_num_boxes, hex_num_objs;
    float hex_target[3];
    HexRec hex_boxes[HEX_MAX_BOXES], hex_objs[HEX_MAX_OBJS];
};
#pragma pack(pop)

int mv_debug_launch_counts(mv_gym *g, int64_t out[2])
{
    if (check(g)) return -1;
    if (!out) return fail("mv_debug_launch_counts: null pointer");
    const mv_gym *c = g->inGroup && !g->inGroup->gyms.empty() ? g->inGroup->gyms[0] : g;   // (a group's launches are counted on its leader)
    out[0] = c->launchCount[0]; out[1] = c->launchCount[1];
    return 0;
}

int mv_debug_set_agent_pos(mv_gym *g, int32_t env, int32_t agent, float x, float y, float z)
{
    if (check(g)) return -1;
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail("mv_debug_set_agent_pos: index out of range");
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    hipLaunchKernelGGL(set_agent_pos_kernel, dim3(1), dim3(1), 0, g->stream, g->gv.agents, env * g->A + agent, x, y, z);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mv_debug_set_agent_yaw(mv_gym *g, int32_t env, int32_t agent, float c, float s)
{
    if (check(g)) return -1;
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail("mv_debug_set_agent_yaw: index out of range");
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    hipLaunchKernelGGL(set_agent_yaw_kernel, dim3(1), dim3(1), 0, g->stream, g->gv.agents, env * g->A + agent, c, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mv_debug_set_agent_velocity(mv_gym *g, int32_t env, int32_t agent, float hvx, float hvz, float vvel)
{
    if (check(g)) return -1;
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail("mv_debug_set_agent_velocity: index out of range");
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    hipLaunchKernelGGL(set_agent_velocity_kernel, dim3(1), dim3(1), 0, g->stream, g->gv.agents, env * g->A + agent, hvx, hvz, vvel);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mv_debug_set_agent_pitch(mv_gym *g, int32_t env, int32_t agent, float pitch)
{
    if (check(g)) return -1;
    if (env < 0 || env >= g->N || agent < 0 || agent >= g->A) return fail("mv_debug_set_agent_pitch: index out of range");
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    hipLaunchKernelGGL(set_agent_pitch_kernel, dim3(1), dim3(1), 0, g->stream, g->gv.agents, env * g->A + agent, pitch);
    HIP_TRY(hipGetLastError());
    return 0;
}

// TowerBuilding: env `env`'s movable boxes as a test states them -- records, count, the chunk's VX_OBJECT bits, who carries what, bz_reward.  The episode's
// timers, highest_tower, the agents' picked_up / visited_zone and the generator's ring stay as they are.
int mv_debug_set_objects(mv_gym *g, int32_t env, const int8_t (*objs)[4], int32_t n)
{
    if (check(g)) return -1;
    if (g->scenario != SCN_TOWER || !g->gv.chunk) return fail("mv_debug_set_objects: not a TowerBuilding gym");
    if (env < 0 || env >= g->N || n < 0 || n > (int)MAX_OBJECTS || (n > 0 && !objs)) return fail("mv_debug_set_objects: bad arguments");
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    HIP_TRY(hipStreamSynchronize(g->stream));
    std::vector<uint8_t> chunk(CHUNK_BYTES);
    std::vector<AgentState> ag(g->A);
    HIP_TRY(hipMemcpy(chunk.data(), g->gv.chunk + (size_t)env * CHUNK_BYTES, CHUNK_BYTES, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ag.data(), g->gv.agents + (size_t)env * g->A, g->A * sizeof(AgentState), hipMemcpyDeviceToHost));
    auto cell = [](int x, int y, int z) { return (y * CZ + z) * CX + x; };
    auto inside = [](int x, int y, int z) { return x >= 0 && x < CX && y >= 0 && y < CY && z >= 0 && z < CZ; };
    std::vector<MovableObject> rec(MAX_OBJECTS, MovableObject{0, 0, 0, 0});
    std::vector<int> carried(g->A, -1);
    for (auto &c : chunk) c &= (uint8_t)~VX_OBJECT;
    for (int i = 0; i < n; ++i) {
        const int x = objs[i][0], y = objs[i][1], z = objs[i][2], st = objs[i][3];
        rec[i] = MovableObject{(int8_t)x, (int8_t)y, (int8_t)z, (int8_t)st};
        if (st < 0) return fail("mv_debug_set_objects: an object's state is 0 (placed) or 1 + the agent that carries it");
        if (st > 0) {
            if (st - 1 >= g->A) return fail("mv_debug_set_objects: an object is carried by an agent the env does not have");
            if (carried[st - 1] >= 0) return fail("mv_debug_set_objects: two objects are carried by one agent");
            carried[st - 1] = i;
            continue;
        }
        for (int j = 0; j < i; ++j)
            if (objs[j][3] == 0 && objs[j][0] == x && objs[j][1] == y && objs[j][2] == z) return fail("mv_debug_set_objects: two placed objects share a voxel");
        if (!inside(x, y, z)) continue;
        if (chunk[cell(x, y, z)] & VX_SOLID) return fail("mv_debug_set_objects: a placed object is in a solid voxel");
        chunk[cell(x, y, z)] |= VX_OBJECT;
    }
    for (int a = 0; a < g->A; ++a) ag[a].carrying = carried[a];
    HIP_TRY(hipMemcpy(g->gv.objects + (size_t)env * MAX_OBJECTS, rec.data(), MAX_OBJECTS * sizeof(MovableObject), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->gv.chunk + (size_t)env * CHUNK_BYTES, chunk.data(), CHUNK_BYTES, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->gv.agents + (size_t)env * g->A, ag.data(), g->A * sizeof(AgentState), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(&g->gv.hdr[env].num_objects, &n, sizeof n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(set_objects_reward_kernel, dim3(1), dim3(64), 0, g->stream, g->gv, env);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

int mv_debug_snapshot_size(const mv_gym *) { return (int)sizeof(Snap); }

int mv_debug_snapshot(mv_gym *g, int32_t env, void *out)
{
    if (check(g)) return -1;
    if (env < 0 || env >= g->N) return fail("mv_debug_snapshot: index out of range");
    HIP_TRY(hipStreamSynchronize(g->simStream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    EnvHeader h;
    std::vector<LayoutBox> boxes(g->gv.box_stride);
    std::vector<MovableObject> objs(MAX_OBJECTS);
    std::vector<AgentState> ag(g->A);
    Snap *s = new Snap();
    std::memset(s, 0, sizeof *s);
    hipError_t e = hipMemcpy(&h, g->gv.hdr + env, sizeof h, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(boxes.data(), g->gv.boxes + (size_t)env * g->gv.box_stride, g->gv.box_stride * sizeof(LayoutBox), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(objs.data(), g->gv.objects + (size_t)env * MAX_OBJECTS, MAX_OBJECTS * sizeof(MovableObject), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ag.data(), g->gv.agents + (size_t)env * g->A, g->A * sizeof(AgentState), hipMemcpyDeviceToHost);
    if (e == hipSuccess && g->gv.chunk) e = hipMemcpy(s->chunk, g->gv.chunk + (size_t)env * CHUNK_BYTES, CHUNK_BYTES, hipMemcpyDeviceToHost);
    std::vector<TerrainBox> terr(MAX_TERRAIN);
    std::vector<MovableObject> rew(g->gv.reward_stride);
    if (e == hipSuccess && g->gv.terrain) e = hipMemcpy(terr.data(), g->gv.terrain + (size_t)env * MAX_TERRAIN,
        MAX_TERRAIN * sizeof(TerrainBox), hipMemcpyDeviceToHost);
    if (e == hipSuccess && g->gv.rewards_obj) e = hipMemcpy(rew.data(), g->gv.rewards_obj + (size_t)env * g->gv.reward_stride,
        g->gv.reward_stride * sizeof(MovableObject), hipMemcpyDeviceToHost);
    if (e == hipSuccess && g->gv.items) {
        std::vector<ArrangementItem> its(MAX_ITEMS);
        e = hipMemcpy(its.data(), g->gv.items + (size_t)env * MAX_ITEMS, MAX_ITEMS * sizeof(ArrangementItem), hipMemcpyDeviceToHost);
        s->num_items = h.num_terrain;
        for (int i = 0; i < h.num_terrain && i < MAX_ITEMS; ++i) {
            s->items[i][0] = its[i].shape; s->items[i][1] = its[i].color;
            s->items[i][2] = its[i].off[0]; s->items[i][3] = its[i].off[1]; s->items[i][4] = its[i].off[2];
        }
    }
    if (e == hipSuccess && g->gv.soko_cells) e = hipMemcpy(s->soko, g->gv.soko_cells + (size_t)env * (SOKO_DIM * SOKO_DIM),
        SOKO_DIM * SOKO_DIM, hipMemcpyDeviceToHost);
    std::memset(s->heightmap, 0xff, sizeof s->heightmap);
    if (e == hipSuccess && g->gv.heightmap) e = hipMemcpy(s->heightmap, g->gv.heightmap + (size_t)env * HM_BYTES, sizeof s->heightmap, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { delete s; return fail(std::string("mv_debug_snapshot: ") + hipGetErrorString(e)); }
    if (h.scenario == SCN_REARRANGE) h.num_terrain = 0;   // (the header reuses it for the item count, reported as num_items)
    if (e == hipSuccess && g->gv.hex_boxes) {   // Hex*, BoxAGone: the header's box / collider / reward counts describe the hex lists
        s->hex_num_boxes = h.num_boxes; s->hex_num_objs = h.num_rewards;
        s->hex_target[0] = h.hex_target[0]; s->hex_target[1] = 0.0f; s->hex_target[2] = h.hex_target[1];
        e = hipMemcpy(s->hex_boxes, g->gv.hex_boxes + (size_t)env * HEX_MAX_BOXES,
                      (size_t)std::min(h.num_boxes, (int)HEX_MAX_BOXES) * sizeof(HexRec), hipMemcpyDeviceToHost);
        if (e == hipSuccess && g->gv.hex_objs) e = hipMemcpy(s->hex_objs, g->gv.hex_objs + (size_t)env * HEX_MAX_OBJS,
            (size_t)std::min(h.num_rewards, (int)HEX_MAX_OBJS) * sizeof(HexRec), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { delete s; return fail(std::string("mv_debug_snapshot: ") + hipGetErrorString(e)); }
        h.num_boxes = 0; h.num_rewards = 0; h.num_terrain = 0;
    }
    s->scenario = h.scenario; s->num_terrain = h.num_terrain; s->num_rewards = h.num_rewards; s->num_platforms = h.num_platforms; s->solved = h.solved;
    for (int i = 0; i < h.num_terrain && i < MAX_TERRAIN; ++i) {
        const TerrainBox &t = terr[i];
        int32_t *o = s->terrain[i];
        o[0] = t.min[0]; o[1] = t.min[1]; o[2] = t.min[2]; o[3] = t.max[0]; o[4] = t.max[1]; o[5] = t.max[2]; o[6] = t.type; o[7] = 0;
    }
    for (int i = 0; i < h.num_rewards && i < g->gv.reward_stride; ++i) {
        s->rewards[i][0] = rew[i].x; s->rewards[i][1] = rew[i].y; s->rewards[i][2] = rew[i].z; s->rewards[i][3] = rew[i].state;
    }
    s->L = h.L; s->H = h.H; s->W = h.W;
    for (int i = 0; i < 4; ++i) s->bz[i] = h.bz[i];
    s->layout_color = h.layout_color; s->wall_color = h.wall_color; s->draw_walls = h.draw_walls;
    s->num_objects = h.num_objects; s->num_boxes = h.num_boxes; s->num_frames = h.num_frames; s->done = h.done;
    s->highest_tower = h.highest_tower; s->num_agents = g->A;
    s->episode_sec = h.episode_sec; s->episode_len = h.episode_len; s->bz_reward = h.bz_reward; s->bar_half_width = h.bar_half_width;
    for (int i = 0; i < h.num_boxes && i < g->gv.box_stride; ++i) {
        const LayoutBox &b = boxes[i];
        int32_t *o = s->boxes[i];
        o[0] = b.min[0]; o[1] = b.min[1]; o[2] = b.min[2]; o[3] = b.max[0]; o[4] = b.max[1]; o[5] = b.max[2]; o[6] = b.type; o[7] = b.slot;
    }
    for (int i = 0; i < h.num_objects && i < MAX_OBJECTS; ++i) {
        s->objects[i][0] = objs[i].x; s->objects[i][1] = objs[i].y; s->objects[i][2] = objs[i].z; s->objects[i][3] = objs[i].state;
    }
    for (int i = 0; i < g->A; ++i) {
        const AgentState &a = ag[i];
        SnapAgent &o = s->agents[i];
        o.pos[0] = a.pos[0]; o.pos[1] = a.pos[1]; o.pos[2] = a.pos[2];
        o.basis[0] = a.m00; o.basis[1] = a.m02; o.basis[2] = a.m20; o.basis[3] = a.m22;
        o.pitch = a.pitch; o.hv[0] = a.hvx; o.hv[1] = a.hvz; o.vvel = a.vvel; o.voffset = a.voffset;
        o.step_offset = a.step_offset; o.jump_speed = a.jump_speed; o.was_jumping = a.was_jumping; o.carrying = a.carrying;
        o.picked_up = a.picked_up; o.visited_zone = a.visited_zone;
        for (int k = 0; k < 3; ++k) o.spawn[k] = a.spawn[k];
        o.last_reward = a.last_reward; o.total_reward = a.total_reward;
        for (int k = 0; k < NUM_SHAPING; ++k) o.shaping[k] = a.shaping[k];
    }
    std::memcpy(out, s, sizeof *s);
    delete s;
    return 0;
}

// Host-only test hook (no device needed): the n-th episode an env seeded with `env_seed` generates, as the raw
// blob the reset kernel consumes (EpisodeBlob for the Obstacles family, CollectBlob for Collect).
int mv_debug_generate_episode(const char *scenario_name, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len,
                              void *out, int32_t out_bytes)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    if (!scenario_name || !scenario_from_name(lower(scenario_name), scenario, oc) || scenario == SCN_TOWER || scenario == SCN_SOKOBAN
        || scenario == SCN_FOOTBALL)
        return fail("mv_debug_generate_episode: the Obstacles family, Empty, Collect, Rearrange, HexMemory, HexExplore and BoxAGone (Sokoban: mv_debug_generate_sokoban, Football: mv_debug_generate_football)");
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1) return fail("mv_debug_generate_episode: bad arguments");
    const ScenarioRow &row = scenario_row(scenario);
    const size_t bytes = row.record_bytes;
    if (!out) return (int)bytes;
    if ((size_t)out_bytes < bytes) return fail("mv_debug_generate_episode: buffer too small");
    std::mt19937 rng;
    rng.seed((unsigned long)env_seed);
    std::vector<uint8_t> buf(bytes, 0);
    for (int i = 0; i < n; ++i) {
        std::memset(buf.data(), 0, bytes);
        generate_episode(row, GenContext{rng, oc, num_agents, base_episode_len, nullptr, nullptr}, 0, buf.data());   // (`seq` stays 0 here)
    }
    std::memcpy(out, buf.data(), bytes);
    return (int)bytes;
}

// Test hook: env `env`'s BoxAGoneState (mv_types.h: platform table, temporary ring, timers, cell map) as the device holds it, after everything
// enqueued so far.  out = null: returns the record's size.
int mv_debug_boxagone_state(mv_gym *g, int32_t env, void *out)
{
    if (check(g)) return -1;
    if (g->scenario != SCN_BOXAGONE || !g->gv.bag) return fail("mv_debug_boxagone_state: not a BoxAGone gym");
    if (!out) return (int)sizeof(BoxAGoneState);
    if (env < 0 || env >= g->N) return fail("mv_debug_boxagone_state: bad env");
    HIP_TRY(hipStreamSynchronize(g->simStream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(out, g->gv.bag + env, sizeof(BoxAGoneState), hipMemcpyDeviceToHost));
    return (int)sizeof(BoxAGoneState);
}

// Host-only test hook: drives an EpisodeFeeder (worker pool, per-env ordering, recycle) without a device and checks
// every episode it delivers against a straight sequential generation from the same seeds.  Returns 0 when equal.
int mv_debug_feeder_selftest(const char *scenario_name, int32_t num_envs, int32_t num_agents, int32_t threads, int32_t rounds)
{
    int scenario = SCN_TOWER;
    ObstacleConfig oc;
    if (!scenario_name || !scenario_from_name(lower(scenario_name), scenario, oc) || scenario == SCN_TOWER || scenario == SCN_SOKOBAN || scenario == SCN_EMPTY
        || scenario == SCN_FOOTBALL)
        return fail("mv_debug_feeder_selftest: the Obstacles family, Collect, Rearrange, HexMemory and HexExplore");
    const ScenarioRow &row = scenario_row(scenario);
    const size_t bytes = row.record_bytes;
    std::vector<uint8_t> slots((size_t)num_envs * bytes, 0), want(bytes);
    std::vector<uint32_t> seeds(num_envs);
    for (int i = 0; i < num_envs; ++i) seeds[i] = 1000u + 7u * (uint32_t)i;
    std::vector<std::mt19937> rng(num_envs);
    for (int i = 0; i < num_envs; ++i) rng[i].seed((unsigned long)seeds[i]);
    EpisodeFeeder feeder(scenario, oc, num_envs, num_agents, 60.0f, slots.data(), bytes, 0, threads);
    feeder.reseed(seeds, std::vector<int>(num_envs, 1));
    for (int r = 1; r <= rounds; ++r)
        for (int k = 0; k < num_envs; ++k) {
            const int i = (r & 1) ? k : num_envs - 1 - k;   // consume in varying order
            size_t used = 0;
            const uint8_t *got = feeder.wait_ready(i, r, &used);
            if (!got) return fail("feeder selftest: episode not delivered");
            std::memset(want.data(), 0, bytes);
            generate_episode(row, GenContext{rng[i], oc, num_agents, 60.0f, nullptr, nullptr}, r, want.data());
            if (!episodes_equal(row, got, want.data(), used, num_agents))
                return fail(std::string("feeder selftest: ") + row.name + " episode differs from sequential generation");
            feeder.recycle(i, nullptr);
        }
    return 0;
}

// Host-only test hook for the Sokoban generator: the first `n` episodes an env
// seeded with env_seed generates from the level files under $BOXOBAN_LEVELS, as n consecutive SokobanBlob records.
// Host-only test hook: episodes 1..n an env seeded with `env_seed` generates for Football, as the FootballBlob records the reset kernel consumes.
// out = null: returns the record's size.
int mv_debug_generate_football(int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes)
{
    if (!out) return (int)sizeof(FootballBlob);
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1 || (size_t)out_bytes < (size_t)n * sizeof(FootballBlob))
        return fail("mv_debug_generate_football: bad arguments");
    std::mt19937 rng;
    rng.seed((unsigned long)env_seed);
    for (int i = 0; i < n; ++i) generate_football_episode(rng, num_agents, base_episode_len, reinterpret_cast<FootballBlob *>(out)[i]);
    return n;
}

// Test hooks: env `env`'s FootballState (mv_types.h: the ball) as the device holds it after everything enqueued so far; and a ball placed by a test
// (position, velocity, angular velocity, pending force; its drawing record follows).  out = null: returns the record's size.
int mv_debug_football_state(mv_gym *g, int32_t env, void *out)
{
    if (check(g)) return -1;
    if (g->scenario != SCN_FOOTBALL || !g->gv.fb) return fail("mv_debug_football_state: not a Football gym");
    if (!out) return (int)sizeof(FootballState);
    if (env < 0 || env >= g->N) return fail("mv_debug_football_state: bad env");
    HIP_TRY(hipStreamSynchronize(g->simStream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(out, g->gv.fb + env, sizeof(FootballState), hipMemcpyDeviceToHost));
    return (int)sizeof(FootballState);
}

int mv_debug_set_football_state(mv_gym *g, int32_t env, const void *in)
{
    if (check(g)) return -1;
    if (g->scenario != SCN_FOOTBALL || !g->gv.fb) return fail("mv_debug_set_football_state: not a Football gym");
    if (env < 0 || env >= g->N || !in) return fail("mv_debug_set_football_state: bad arguments");
    FootballState s;
    std::memcpy(&s, in, sizeof s);
    HexRec r;
    r.a[0] = s.pos[0]; r.a[1] = s.pos[1]; r.a[2] = s.pos[2]; r.meta = HEX_SPHERE;
    r.b[0] = s.radius; r.b[1] = s.radius; r.b[2] = s.radius; r.color = 0xffb400;   // (mv_tick_football.h: ball_rec)
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    HIP_TRY(hipMemcpyAsync(g->gv.fb + env, &s, sizeof s, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->gv.hex_objs + (size_t)env * HEX_MAX_OBJS, &r, sizeof r, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));   // (s, r: host stack)
    return 0;
}

int mv_debug_generate_sokoban(int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes)
{
    if (!out) return (int)sizeof(SokobanBlob);
    if (num_agents < 1 || num_agents > MAX_AGENTS || n < 1 || (size_t)out_bytes < (size_t)n * sizeof(SokobanBlob))
        return fail("mv_debug_generate_sokoban: bad arguments");
    const std::vector<std::string> files = find_boxoban_level_files();
    if (files.empty()) return fail("mv_debug_generate_sokoban: no Boxoban levels found (BOXOBAN_LEVELS)");
    std::mt19937 rng;
    rng.seed((unsigned long)env_seed);
    SokobanLevels levels;
    for (int i = 0; i < n; ++i)
        if (!generate_sokoban_episode(rng, levels, files, num_agents, base_episode_len, reinterpret_cast<SokobanBlob *>(out)[i]))
            return fail("mv_debug_generate_sokoban: unreadable level file");
    return n;
}

int mv_debug_rng(int32_t device, uint32_t seed, int32_t what, const int32_t *lo, const int32_t *hi, int32_t n, void *out)
{
    HIP_TRY(hipSetDevice(device));
    if (what == 3 && n > 4096) return fail("mv_debug_rng: shuffle n <= 4096");
    int32_t *dlo = nullptr, *dhi = nullptr;
    void *dout = nullptr;
    HIP_TRY(hipMalloc(&dout, (size_t)n * 4));
    if (what == 1) {
        HIP_TRY(hipMalloc((void **)&dlo, (size_t)n * 4));
        HIP_TRY(hipMalloc((void **)&dhi, (size_t)n * 4));
        HIP_TRY(hipMemcpy(dlo, lo, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dhi, hi, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(debug_rng_kernel, dim3(1), dim3(64), 0, nullptr, seed, what, dlo, dhi, n, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dout); (void)hipFree(dlo); (void)hipFree(dhi);
    return 0;
}

int mv_debug_math(int32_t device, int32_t what, const float *a, const float *b, int32_t n, float *out)
{
    HIP_TRY(hipSetDevice(device));
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t outN = (what == 2) ? 2 * (size_t)n : (size_t)n;
    HIP_TRY(hipMalloc((void **)&da, (size_t)n * 4));
    HIP_TRY(hipMalloc((void **)&db, (size_t)n * 4));
    HIP_TRY(hipMalloc((void **)&dout, outN * 4));
    HIP_TRY(hipMemcpy(da, a, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b ? b : a, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, what, da, db, n, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, outN * 4, hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return 0;
}

int mv_debug_raster_consts_host(int32_t W, int32_t H, float *consts, uint32_t *tiles_x_inv, float *dcx, float *dcy)
{
    if (W < 1 || H < 1 || W > 1024 || H > 1024) return fail("mv_debug_raster_consts_host: size must be within 1..1024");
    const RasterConsts rc = raster_launch_consts(W, H);
    if (consts) { consts[0] = rc.sx; consts[1] = rc.ox; consts[2] = rc.sy; consts[3] = rc.oy; }
    if (tiles_x_inv) *tiles_x_inv = rc.tiles_x_inv;
    if (dcx && dcy) {
        std::vector<float> tab((size_t)(W + H));
        raster_ray_table(W, H, tab.data());
        std::memcpy(dcx, tab.data(), (size_t)W * sizeof(float));
        std::memcpy(dcy, tab.data() + W, (size_t)H * sizeof(float));
    }
    return 0;
}

int mv_debug_raster_div_host(uint32_t d, uint32_t n_end, uint32_t *magic, uint32_t *q)
{
    if (d < 1) return fail("mv_debug_raster_div_host: d >= 1");
    const uint32_t m = raster_div_magic(d);
    if (magic) *magic = m;
    if (q) for (uint32_t n = 0; n < n_end; ++n) q[n] = raster_div_by_magic(n, m);   // (the kernels' div_magic: __umulhi)
    return 0;
}

// The rule of mv_still_frames.h compiled for the CPU (no device): k ticks of N envs, in the order the MASKED step bodies apply it -- behind the tick's `steps`
// choice, then behind the frame choice of a tick that has a pass.
int mv_debug_still_rule_host(const uint8_t *steps, const uint8_t *has_pass, const uint8_t *draw_mask, const uint8_t *stale_in, int32_t k, int32_t N,
                             int32_t *verdict_out, uint8_t *stale_out)
{
    if (!steps || !has_pass || !stale_in || !verdict_out || !stale_out || k < 0 || N < 1) return fail("mv_debug_still_rule_host: bad arguments");
    for (int32_t e = 0; e < N; ++e) {
        int stale = stale_in[e] != 0 ? 1 : 0;
        for (int32_t t = 0; t < k; ++t) {
            stale = mv::still::still_after_tick(stale, steps[(size_t)t * N + e] != 0);
            int v = mv::still::VERDICT_NO_PASS;
            if (has_pass[t]) {
                v = mv::still::still_verdict(draw_mask ? (int)draw_mask[e] : 1, stale);
                stale = mv::still::still_after_frames(stale, v);
            }
            verdict_out[(size_t)t * N + e] = v;
        }
        stale_out[e] = (uint8_t)stale;
    }
    return 0;
}

// The carry of mv_still_frames.h compiled for the CPU (no device): every frame's plan, then its copies in tick order, each from the plan's source entry.
int mv_debug_still_carry_host(const int32_t *verdict, const int32_t *entries, int32_t k, int32_t frames, int32_t R, int32_t frame_bytes,
                              uint8_t *ring_bytes, int32_t *home)
{
    if (!verdict || !entries || !ring_bytes || !home || k < 0 || k > (int32_t)PIPE_BATCH_MAX || frames < 1 || R < 1 || frame_bytes < 1)
        return fail("mv_debug_still_carry_host: bad arguments (k <= 16)");
    for (int32_t j = 0; j < k; ++j)
        if (entries[j] < 0 || entries[j] >= R) return fail("mv_debug_still_carry_host: entry out of range");
    const size_t fb = (size_t)frame_bytes, eb = (size_t)frames * fb;
    for (int32_t f = 0; f < frames; ++f) {
        int32_t src[PIPE_BATCH_MAX];
        const int32_t h = home[f];
        home[f] = mv::still::still_carry_plan(verdict + f, (size_t)frames, entries, k, h >= 0 && h < R ? h : -1, src);
        for (int32_t j = 0; j < k; ++j)
            if (src[j] >= 0) std::memcpy(ring_bytes + (size_t)entries[j] * eb + (size_t)f * fb, ring_bytes + (size_t)src[j] * eb + (size_t)f * fb, fb);
    }
    return 0;
}

}  // extern "C"
