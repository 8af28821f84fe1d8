// megaverse_amd/csrc/mv_obs_rows.hip -- the three row records a gym publishes per tick, state observations (per agent, mv_state_obs.h), scene observations
// (per env, mv_scene_obs.h) and entity observations (per object, E rows per env, mv_entity_obs.h): the host side of mv_set_* / mv_get_*_obs /
// mv_get_*_observation (include/megaverse_hip.h), the per-slot staging rows, the ONE launch that carries a stepping call's rows to the caller's buffers,
// the gathers behind a reset or mv_render, and the records' host twins mv_debug_state_obs_host / mv_debug_scene_obs_host / mv_debug_entity_obs_host.  The MASKED step kernels write the staging rows (mv_step_kernels.h:
// state_obs_write, scene_obs_write, entity_obs_write).
// DESIGN.md 3.14, 3.19 and 3.22 say where the rows are written and where publication stands in the streams' order.
#include "mv_api_internal.h"
#include "mv_state_obs.h"
#include "mv_scene_obs.h"
#include "mv_entity_obs.h"

static_assert((int)MV_STATE_OBS_FLOATS == (int)STATE_OBS_FLOATS, "the header's row length is the record's");
static_assert((int)MV_SCENE_OBS_FLOATS == (int)SCENE_OBS_FLOATS, "the header's row length is the record's");
static_assert((int)MV_ENTITY_OBS_FLOATS == (int)ENTITY_OBS_FLOATS && (int)MV_ENTITY_OBS_GROUPS == (int)ENTITY_GROUPS, "the header's row length and group count are the record's");

namespace {

// The k ticks of one stepping call with ONE launch, for all three records, publish_ticks_kernel's sibling: thread i < scene_words carries word i of every tick's
// staged scene rows to that tick's entry of the caller's buffer, in ascending tick order -- without an output ring every tick's entry is the one entry and the
// last tick's rows stay; the threads behind them do the same for the state_words words of the state rows, and those behind them for the entity_words words
// of the entity rows.  A record that is off has 0 words.
struct PublishRowsArgs {
    int32_t k, scene_words, state_words, entity_words;
    const uint32_t *scene_src[PIPE_BATCH_MAX];
    uint32_t *scene_dst[PIPE_BATCH_MAX];
    const uint32_t *state_src[PIPE_BATCH_MAX];
    uint32_t *state_dst[PIPE_BATCH_MAX];
    const uint32_t *entity_src[PIPE_BATCH_MAX];
    uint32_t *entity_dst[PIPE_BATCH_MAX];
};
static_assert(sizeof(PublishRowsArgs) <= 4096, "PublishRowsArgs must fit the 4 KB kernel-argument segment");
__global__ __launch_bounds__(256) void publish_rows_ticks_kernel(PublishRowsArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.scene_words) {
        for (int j = 0; j < a.k; ++j) a.scene_dst[j][i] = a.scene_src[j][i];
    } else if (i - a.scene_words < a.state_words) {
        const int s = i - a.scene_words;
        for (int j = 0; j < a.k; ++j) a.state_dst[j][s] = a.state_src[j][s];
    } else if (i - a.scene_words - a.state_words < a.entity_words) {
        const int s = i - a.scene_words - a.state_words;
        for (int j = 0; j < a.k; ++j) a.entity_dst[j][s] = a.entity_src[j][s];
    }
}

// the rows of the current state (behind mv_reset, mv_reset_envs(render = 1), mv_render): thread i packs word i of [N*A][16]; mask != null: only the rows of
// the envs it flags, the others keep what they hold
__global__ __launch_bounds__(256) void state_obs_gather_kernel(const AgentState *__restrict__ agents, const EnvHeader *__restrict__ hdr,
                                                               const uint8_t *__restrict__ mask, uint32_t *__restrict__ rows, int A, int words)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    const int agent = i >> 4, env = agent / A;
    if (mask != nullptr && mask[env] == 0) return;
    rows[i] = state_obs_word(agents + agent, hdr + env, i & (STATE_OBS_FLOATS - 1));
}

// ... thread i packs word i of [N][32].  The Obstacles family's columns 16..23 take the record's loops (scene_obs_scan), each thread its own: at most
// 16 boxes and the env's reward slots, behind calls that draw every frame of the gym.
__global__ __launch_bounds__(256) void scene_obs_gather_kernel(GymView gv, const uint8_t *__restrict__ mask, uint32_t *__restrict__ rows, int words)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    const int env = i / SCENE_OBS_FLOATS, f = i % SCENE_OBS_FLOATS;
    if (mask != nullptr && mask[env] == 0) return;
    const EnvHeader *h = gv.hdr + env;
    const TerrainBox *terrain = gv.terrain + (size_t)env * MAX_TERRAIN;
    const MovableObject *rewards = gv.rewards_obj + (size_t)env * gv.reward_stride;
    SceneObsScan scan = {0, -1, 0};
    if (gv.scenario == SCN_OBSTACLES && f >= SCENE_OBS_SCENARIO_COL && f <= SCENE_OBS_SCENARIO_COL + 7) scan = scene_obs_scan(h, terrain, rewards);
    rows[i] = scene_obs_word(gv.scenario, h, terrain, rewards, gv.fb + env, scan, f);
}

// ... thread i packs row i of [N][E][8] and stores it as two 16-byte words (mv_set_entity_obs refuses a buffer that is not 16-byte aligned).  Sokoban's goal
// rows take the record's loop (entity_soko_goal_of), each thread its own: at most 1024 cell bytes, behind calls that draw every frame of the gym.
__global__ __launch_bounds__(256) void entity_obs_gather_kernel(GymView gv, const uint8_t *__restrict__ mask, uint4 *__restrict__ rows, int E, int total)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int env = i / E, row = i - env * E;
    if (mask != nullptr && mask[env] == 0) return;
    const int A = gv.num_agents;
    const EntityLayout l = entity_layout(gv.scenario, A);
    const EntitySrc s = {gv.scenario, A, gv.hdr + env, gv.terrain + (size_t)env * MAX_TERRAIN, gv.items + (size_t)env * MAX_ITEMS,
                         gv.soko_cells + (size_t)env * (SOKO_DIM * SOKO_DIM), gv.objects + (size_t)env * MAX_OBJECTS,
                         gv.rewards_obj + (size_t)env * gv.reward_stride, gv.hex_objs + (size_t)env * HEX_MAX_OBJS, gv.fb + env, gv.agents + (size_t)env * A};
    EntityRow r = entity_obs_row(s, l, row);
    if (gv.scenario == SCN_SOKOBAN && row < l.base[ENTITY_OBJECTS]) {
        const int c = entity_soko_goal_of(s.soko, row);
        if (c >= 0) r = entity_soko_goal_row(c, s.hdr->W);
    }
    rows[2 * (size_t)i] = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    rows[2 * (size_t)i + 1] = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
}

// One record as the shared code sees it: its option (the setter's name, the refusal texts), the gym's ObsRows, the view field that carries a slot's rows.
struct Record {
    const GymOption &opt;
    ObsRows mv_gym::*rows;
    float *GymView::*field;
    const char *getter, *reader, *noun;   // mv_get_*_obs, mv_get_*_observation, "state observations"
    int floats;                           // of one row; 0: E rows of ENTITY_OBS_FLOATS, E the gym's (rec_floats)
    bool perAgent;                        // a row per agent, [N*A]; else per env, [N]
};
const Record STATE = {gym_options[OPT_STATE_OBS], &mv_gym::stateRows, &GymView::state_obs, "mv_get_state_obs", "mv_get_state_observation", obs_stream(OPT_STATE_OBS).noun,
                      STATE_OBS_FLOATS, true};
const Record SCENE = {gym_options[OPT_SCENE_OBS], &mv_gym::sceneRows, &GymView::scene_obs, "mv_get_scene_obs", "mv_get_scene_observation", obs_stream(OPT_SCENE_OBS).noun,
                      SCENE_OBS_FLOATS, false};
const Record ENTITY = {gym_options[OPT_ENTITY_OBS], &mv_gym::entityRows, &GymView::entity_obs, "mv_get_entity_obs", "mv_get_entity_observation",
                       obs_stream(OPT_ENTITY_OBS).noun, 0, false};
int entity_rows_of(const mv_gym *g) { return entity_obs_rows(g->gv.scenario, g->A); }
int rec_floats(const mv_gym *g, const Record &rec) { return rec.floats ? rec.floats : entity_rows_of(g) * (int)ENTITY_OBS_FLOATS; }

// the last tick's entry: what a refresh writes and a single-row read-back reads
float *last_entry(const mv_gym *g, const ObsRows &r) { return r.entry(g->ringTick ? g->ringTick - 1 : 0); }

int rows_attach(mv_gym *g, const Record &rec, float *device_buf)
{
    if (attach_check(g, rec.opt.setter, rec.opt)) return -1;
    ObsRows &r = g->*rec.rows;
    const size_t words = (size_t)g->N * (rec.perAgent ? g->A : 1) * rec_floats(g, rec);
    if (device_buf && !rec.floats && (uintptr_t)device_buf % 16)   // (the gather stores rows as 16-byte words)
        return fail(std::string(rec.opt.setter) + ": the buffer must be 16-byte aligned");
    if (device_buf && !r.stage) {
        // The staging rows, one set per hand-over slot, allocated here and not out of the arena: the arena's layout, its size and the slot stride the
        // passes derive stay what they are.  Kept until mv_close: launches in flight may still write rows after a detach.
        HIP_TRY(hipSetDevice(g->device));
        const size_t bytes = (size_t)g->slots * words * sizeof(float);
        hipError_t e_ = hipMalloc((void **)&r.stage, bytes);
        if (e_ != hipSuccess) { r.stage = nullptr; return fail(std::string(rec.opt.setter) + ": hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
        r.stageBytes = bytes;
    }
    // No launch, no copy.  The step launches enqueued so far keep the views they were given; the next one takes the MASKED kernels (or the unmasked ones
    // again) and is ordered behind whatever the caller's stream holds now, as behind mv_set_step_mask.
    r.words = words;
    for (int q = 0; q < g->slots; ++q) g->gvp[(size_t)q].*rec.field = device_buf ? r.stage + (size_t)q * words : nullptr;
    r.buf = device_buf;
    r.entries = device_buf ? std::max(1, g->ringCount) : 0;
    g->simMustWaitUser = true;
    return 0;
}

int rows_count(const mv_gym *g, const Record &rec)
{
    if (getter_check(g, rec.getter)) return -1;
    const ObsRows &r = g->*rec.rows;
    return r.buf ? r.entries : 0;
}

int rows_read(mv_gym *g, const Record &rec, int env, int agent, float *out)   // the last tick's row of one env (perAgent: of one of its agents)
{
    const std::string who = rec.reader;
    if (check(g)) { g_err = who + ": " + g_err; return -1; }
    const ObsRows &r = g->*rec.rows;
    if (!r.buf) return fail(who + ": no " + rec.noun + " attached (" + rec.opt.setter + ")");
    if (!out) return fail(who + ": null pointer");
    if (env < 0 || env >= g->N || (rec.perAgent && (agent < 0 || agent >= g->A))) return fail(who + ": index out of range");
    HIP_TRY(hipSetDevice(g->device));
    const size_t row = rec.perAgent ? (size_t)env * g->A + agent : (size_t)env;
    const size_t floats = (size_t)rec_floats(g, rec);
    HIP_TRY(hipMemcpyAsync(out, last_entry(g, r) + row * floats, floats * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return 0;
}

void rows_free(mv_gym *g, const Record &rec)
{
    ObsRows &r = g->*rec.rows;
    if (r.stage) (void)hipFree(r.stage);
    r = ObsRows();
    for (GymView &v : g->gvp) v.*rec.field = nullptr;
}

}  // namespace

namespace mvapi {

// The staged rows of the ticks in slots q0 .. q0 + k - 1 -> the entries of ticks tick0 .. tick0 + k - 1 (the entries outputs_of gives their rewards), both
// records (all three) with one launch on the caller's stream; -> 1: launched, 0: no record is attached
int obs_rows_publish(mv_gym *g, int q0, unsigned long long tick0, int k)
{
    const ObsRows &sc = g->sceneRows, &st = g->stateRows, &en = g->entityRows;
    if (!sc.buf && !st.buf && !en.buf) return 0;
    PublishRowsArgs a;
    a.k = k;
    a.entity_words = en.buf ? (int32_t)en.words : 0;
    a.scene_words = sc.buf ? (int32_t)sc.words : 0;
    a.state_words = st.buf ? (int32_t)st.words : 0;
    for (int j = 0; j < (int)PIPE_BATCH_MAX; ++j) {
        const int jj = std::min(j, k - 1);
        const GymView &v = g->gvp[(size_t)(q0 + jj)];
        a.scene_src[j] = sc.buf ? reinterpret_cast<const uint32_t *>(v.scene_obs) : nullptr;
        a.scene_dst[j] = sc.buf ? reinterpret_cast<uint32_t *>(sc.entry(tick0 + (unsigned long long)jj)) : nullptr;
        a.state_src[j] = st.buf ? reinterpret_cast<const uint32_t *>(v.state_obs) : nullptr;
        a.state_dst[j] = st.buf ? reinterpret_cast<uint32_t *>(st.entry(tick0 + (unsigned long long)jj)) : nullptr;
        a.entity_src[j] = en.buf ? reinterpret_cast<const uint32_t *>(v.entity_obs) : nullptr;
        a.entity_dst[j] = en.buf ? reinterpret_cast<uint32_t *>(en.entry(tick0 + (unsigned long long)jj)) : nullptr;
    }
    hipLaunchKernelGGL(publish_rows_ticks_kernel, dim3((a.scene_words + a.state_words + a.entity_words + 255) / 256), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    return 1;
}

// the last tick's entries gathered from the current state, on the caller's stream behind sim_join (mask: device bytes [N], only the flagged envs' rows;
// null: every row; a record that is not attached: no launch)
int obs_rows_refresh(mv_gym *g, const uint8_t *device_mask)
{
    if (g->stateRows.buf) {
        const int words = (int)g->stateRows.words;
        hipLaunchKernelGGL(state_obs_gather_kernel, dim3((words + 255) / 256), dim3(256), 0, g->stream, g->gv.agents, g->gv.hdr, device_mask,
                           reinterpret_cast<uint32_t *>(last_entry(g, g->stateRows)), g->A, words);
        HIP_TRY(hipGetLastError());
    }
    if (g->sceneRows.buf) {
        const int words = (int)g->sceneRows.words;
        hipLaunchKernelGGL(scene_obs_gather_kernel, dim3((words + 255) / 256), dim3(256), 0, g->stream, g->gv, device_mask,
                           reinterpret_cast<uint32_t *>(last_entry(g, g->sceneRows)), words);
        HIP_TRY(hipGetLastError());
    }
    if (g->entityRows.buf) {
        const int E = entity_rows_of(g), total = g->N * E;
        hipLaunchKernelGGL(entity_obs_gather_kernel, dim3((total + 255) / 256), dim3(256), 0, g->stream, g->gv, device_mask,
                           reinterpret_cast<uint4 *>(last_entry(g, g->entityRows)), E, total);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

void obs_rows_free(mv_gym *g) { rows_free(g, STATE); rows_free(g, SCENE); rows_free(g, ENTITY); }

}  // namespace mvapi

extern "C" {

int mv_set_state_obs(mv_gym *g, float *device_buf) { return rows_attach(g, STATE, device_buf); }
int mv_set_scene_obs(mv_gym *g, float *device_buf) { return rows_attach(g, SCENE, device_buf); }
int mv_get_state_obs(const mv_gym *g) { return rows_count(g, STATE); }
int mv_get_scene_obs(const mv_gym *g) { return rows_count(g, SCENE); }
int mv_get_state_observation(mv_gym *g, int32_t env, int32_t agent, float *out16) { return rows_read(g, STATE, env, agent, out16); }
int mv_get_scene_observation(mv_gym *g, int32_t env, float *out32) { return rows_read(g, SCENE, env, 0, out32); }

int mv_set_entity_obs(mv_gym *g, float *device_buf) { return rows_attach(g, ENTITY, device_buf); }
int mv_get_entity_obs(const mv_gym *g) { return rows_count(g, ENTITY); }
int mv_get_entity_observation(mv_gym *g, int32_t env, float *out) { return rows_read(g, ENTITY, env, 0, out); }

int mv_entity_obs_rows(const mv_gym *g)
{
    if (getter_check(g, "mv_entity_obs_rows")) return -1;
    return entity_rows_of(g);
}

int mv_entity_obs_layout(const mv_gym *g, int32_t out[MV_ENTITY_OBS_GROUPS][3])
{
    if (getter_check(g, "mv_entity_obs_layout")) return -1;
    if (!out) return fail("mv_entity_obs_layout: null pointer");
    const EntityLayout l = entity_layout(g->gv.scenario, g->A);
    for (int k = 0; k < (int)ENTITY_GROUPS; ++k) { out[k][0] = l.base[k]; out[k][1] = l.rows[k]; out[k][2] = l.cls[k]; }
    return 0;
}

int mv_debug_entity_obs_host(int32_t scenario, int32_t num_agents, const void *env_header, const void *terrain16, const void *items8, const void *soko_cells,
                             const void *objects80, const void *rewards, int32_t rewards_len, const void *hex_objs128, const void *football_state,
                             const void *agent_states, float *out)
{
    const char *who = "mv_debug_entity_obs_host";
    if (!env_header || !agent_states || !out) return fail(std::string(who) + ": null pointer (an EnvHeader, num_agents AgentStates and the output are required)");
    if (scenario < 0 || scenario >= SCN_COUNT) return fail(std::string(who) + ": unknown scenario");
    if (num_agents < 1 || num_agents > (int)MAX_AGENTS) return fail(std::string(who) + ": 1 <= num_agents <= 8 required");
    const EntityLayout l = entity_layout(scenario, num_agents);
    EnvHeader h;   // (the caller's bytes need not be aligned)
    std::memcpy(&h, env_header, sizeof h);
    std::vector<AgentState> agents((size_t)num_agents);
    std::memcpy(agents.data(), agent_states, agents.size() * sizeof(AgentState));
    TerrainBox terrain[MAX_TERRAIN] = {};
    ArrangementItem items[MAX_ITEMS] = {};
    std::vector<uint8_t> soko(SOKO_DIM * SOKO_DIM, 0);
    MovableObject objects[MAX_OBJECTS] = {}, rw[COLLECT_MAX_REWARDS] = {};
    std::vector<HexRec> hex(HEX_MAX_OBJS);
    std::memset(hex.data(), 0, hex.size() * sizeof(HexRec));
    FootballState fb = {};
    const bool hexScen = scenario == SCN_HEX_MEMORY || scenario == SCN_HEX_EXPLORE;
    if (l.rows[ENTITY_OBJECTS]) {
        if (h.num_objects < 0 || h.num_objects > (int)MAX_OBJECTS || (h.num_objects > 0 && !objects80))
            return fail(std::string(who) + ": the header's num_objects needs a list of 80 movable objects");
        if (objects80) std::memcpy(objects, objects80, sizeof objects);
    }
    if (scenario == SCN_OBSTACLES || scenario == SCN_REARRANGE) {
        const int cap = scenario == SCN_OBSTACLES ? (int)MAX_TERRAIN : (int)MAX_ITEMS;
        const void *list = scenario == SCN_OBSTACLES ? terrain16 : items8;
        if (h.num_terrain < 0 || h.num_terrain > cap || (h.num_terrain > 0 && !list))
            return fail(std::string(who) + ": the header's num_terrain needs a list of 16 terrain boxes (Rearrange: of 8 arrangement items)");
        if (terrain16 && scenario == SCN_OBSTACLES) std::memcpy(terrain, terrain16, sizeof terrain);
        if (items8 && scenario == SCN_REARRANGE) std::memcpy(items, items8, sizeof items);
    }
    if (scenario == SCN_SOKOBAN) {
        if (!soko_cells) return fail(std::string(who) + ": Sokoban needs its 1024 level cells");
        std::memcpy(soko.data(), soko_cells, soko.size());
    }
    if (scenario == SCN_OBSTACLES || scenario == SCN_COLLECT) {
        const int cap = l.rows[ENTITY_REWARDS];   // (a longer list is accepted: a debug snapshot's has 96 slots for every scenario)
        if (rewards_len < 0 || rewards_len > (int)COLLECT_MAX_REWARDS) return fail(std::string(who) + ": 0 <= rewards_len <= 96 required");
        if (h.num_rewards < 0 || h.num_rewards > std::min(rewards_len, cap) || (h.num_rewards > 0 && !rewards))
            return fail(std::string(who) + ": the header's num_rewards exceeds rewards_len or the scenario's " + std::to_string(cap) + " reward slots");
        if (rewards && rewards_len > 0) std::memcpy(rw, rewards, (size_t)rewards_len * sizeof(MovableObject));
    }
    if (hexScen) {
        if (h.num_rewards < 0 || h.num_rewards > (int)HEX_MAX_OBJS || (h.num_rewards > 0 && !hex_objs128))
            return fail(std::string(who) + ": the header's num_rewards needs a list of 128 HexRec records");
        if (hex_objs128) std::memcpy(hex.data(), hex_objs128, hex.size() * sizeof(HexRec));
    }
    if (scenario == SCN_FOOTBALL) {
        if (!football_state) return fail(std::string(who) + ": Football needs a FootballState");
        std::memcpy(&fb, football_state, sizeof fb);
    }
    const EntitySrc s = {scenario, num_agents, &h, terrain, items, soko.data(), objects, rw, hex.data(), &fb, agents.data()};
    std::vector<uint32_t> rows((size_t)l.total * ENTITY_OBS_FLOATS);
    entity_obs_pack(s, rows.data());
    std::memcpy(out, rows.data(), rows.size() * sizeof(uint32_t));
    return 0;
}

int mv_debug_state_obs_host(const void *agent_state, const void *env_header, float *out16)
{
    if (!agent_state || !env_header || !out16) return fail("mv_debug_state_obs_host: null pointer");
    AgentState a;   // (the caller's bytes need not be aligned)
    EnvHeader h;
    std::memcpy(&a, agent_state, sizeof a);
    std::memcpy(&h, env_header, sizeof h);
    uint32_t row[STATE_OBS_FLOATS];
    state_obs_pack(&a, &h, row);
    std::memcpy(out16, row, sizeof row);
    return 0;
}

int mv_debug_scene_obs_host(int32_t scenario, const void *env_header, const void *terrain16, const void *rewards, int32_t rewards_len,
                            const void *football_state, float *out32)
{
    if (!env_header || !out32) return fail("mv_debug_scene_obs_host: null pointer");
    EnvHeader h;   // (the caller's bytes need not be aligned)
    std::memcpy(&h, env_header, sizeof h);
    TerrainBox terrain[MAX_TERRAIN] = {};
    MovableObject rw[COLLECT_MAX_REWARDS] = {};
    FootballState fb = {};
    if (scenario == SCN_OBSTACLES) {
        if (rewards_len < 0 || rewards_len > (int)COLLECT_MAX_REWARDS) return fail("mv_debug_scene_obs_host: 0 <= rewards_len <= 96 required");
        if (h.num_terrain < 0 || h.num_terrain > (int)MAX_TERRAIN || (h.num_terrain > 0 && !terrain16))
            return fail("mv_debug_scene_obs_host: the header's num_terrain needs a list of 16 terrain boxes");
        if (h.num_rewards < 0 || h.num_rewards > rewards_len || (h.num_rewards > 0 && !rewards))
            return fail("mv_debug_scene_obs_host: the header's num_rewards exceeds rewards_len");
        if (terrain16) std::memcpy(terrain, terrain16, sizeof terrain);
        if (rewards && rewards_len > 0) std::memcpy(rw, rewards, (size_t)rewards_len * sizeof(MovableObject));
    }
    if (scenario == SCN_FOOTBALL) {
        if (!football_state) return fail("mv_debug_scene_obs_host: Football needs a FootballState");
        std::memcpy(&fb, football_state, sizeof fb);
    }
    uint32_t row[SCENE_OBS_FLOATS];
    scene_obs_pack(scenario, &h, terrain, rw, &fb, row);
    std::memcpy(out32, row, sizeof row);
    return 0;
}

}  // extern "C"
