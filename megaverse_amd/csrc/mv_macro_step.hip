// megaverse_amd/csrc/mv_macro_step.hip -- macro steps: the host side of mv_macro_step / mv_macro_step_host (include/megaverse_hip.h), the launch that sets the
// envs' ticks left at a call's start, the accumulating publication of a call's rewards and dones, and the host twins mv_debug_macro_rule_host /
// mv_debug_macro_fold_host.  The rule and the fold are mv_macro_step.h; the step kernels apply the rule tick by tick (mv_step_kernels.h: env_tl, after_tick),
// the episode log walks a mirror of it (mv_episode_log.hip: load_done), and mv_api_step.hip's step_gyms enqueues a call's chunks; DESIGN.md 3.17.
#include "mv_api_internal.h"
#include "mv_macro_step.h"

namespace mv {
namespace macro {

// The call's start: every env's ticks left -- the caller's ticks [N] clamped to [0, k], or k -- into the gym's array and into the log's mirror.
__global__ __launch_bounds__(256) void macro_begin_kernel(const int32_t *__restrict__ ticks, int32_t k, int32_t N, int32_t *__restrict__ tl,
                                                           int32_t *__restrict__ mirror)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= N) return;
    const int32_t v = macro_ticks_begin(ticks != nullptr, ticks != nullptr ? ticks[e] : 0, k);
    tl[e] = v;
    mirror[e] = v;
}

// The accumulating form of publish_ticks_kernel (mv_api.hip): the k staged ticks of one chunk of a macro step go into ONE entry.  Thread i folds agent i's
// rewards in tick order -- from the first tick's value, or (cont: a later chunk of a split call) from what the entry holds -- ORs env i's dones, and records
// the true objective of every tick that finished the env, the latest last.
struct PublishArgs {
    int32_t k, n_envs, A, cont;
    const float *s_rew[PIPE_BATCH_MAX];
    const uint8_t *s_done[PIPE_BATCH_MAX];
    const float *s_true[PIPE_BATCH_MAX];
    float *rew;
    uint8_t *done;
    float *true_obj;
};
__global__ __launch_bounds__(256) void macro_publish_kernel(PublishArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_envs * a.A) return;
    const int e = i / a.A;
    float s = a.cont ? a.rew[i] : a.s_rew[0][i];
    for (int j = a.cont ? 0 : 1; j < a.k; ++j) s = macro_fold(s, a.s_rew[j][i]);
    a.rew[i] = s;
    for (int j = 0; j < a.k; ++j)
        if (a.s_done[j][e]) a.true_obj[i] = a.s_true[j][i];
    if (i < a.n_envs) {
        uint8_t d = a.cont ? a.done[i] : (uint8_t)0;
        for (int j = 0; j < a.k; ++j) d |= a.s_done[j][i];
        a.done[i] = d ? 1 : 0;
    }
}

}  // namespace macro
}  // namespace mv

namespace {

int macro_alloc(mv_gym *g, const char *who)
{
    if (g->macroTl) return 0;
    const size_t N = (size_t)g->N, bytes = mv::macro::macro_step_words(g->N, g->A) * sizeof(int32_t);
    hipError_t e_ = hipMalloc((void **)&g->macroTl, bytes);
    if (e_ != hipSuccess) { g->macroTl = nullptr; return fail(std::string(who) + ": hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e_)); }
    g->macroMirror = g->macroTl + N;
    g->macroTicks = g->macroTl + 2 * N;
    g->macroActions = g->macroTl + 3 * N;
    g->macroBytes = bytes;
    return 0;
}

// what both forms refuse, in mv_step_n_render's order
int macro_check(mv_gym *g, const char *who, int32_t k, const void *actions, int32_t render_mode)
{
    if (check(g)) { g_err = std::string(who) + ": " + g_err; return -1; }
    if (render_mode == MV_RENDER_EVERY) return fail(std::string(who) + ": MV_RENDER_EVERY is refused: a macro step has one frame (MV_RENDER_LAST, MV_RENDER_NONE)");
    if (render_mode != MV_RENDER_LAST && render_mode != MV_RENDER_NONE) return fail(std::string(who) + ": unknown render mode (MV_RENDER_LAST, MV_RENDER_NONE)");
    if (k < 1) return fail(std::string(who) + ": k >= 1 required");
    if (!actions) return fail(std::string(who) + ": null actions");
    if (g->inGroup) return fail(std::string(who) + ": this gym belongs to an mv_group, whose union launches know no macro steps");
    if (!g->wasReset) return fail(std::string(who) + ": call mv_reset first");
    return 0;
}

// the call itself, actions and ticks in device memory and ordered on the caller's stream
int macro_run(mv_gym *g, const char *who, int32_t k, const int32_t *device_actions, const int32_t *device_ticks, int32_t render_mode)
{
    // The ticks left, on the caller's stream: behind every step launch enqueued so far (sim_join: the kernels of the last macro step wrote the array) and
    // behind the episode log's last update, which lives on that stream and reads the mirror; the call's step launches wait for it, as they wait for the
    // caller's actions (simMustWaitUser).
    if (sim_join(g)) return -1;
    hipLaunchKernelGGL(mv::macro::macro_begin_kernel, dim3((unsigned)((g->N + 255) / 256)), dim3(256), 0, g->stream, device_ticks, k, (int32_t)g->N, g->macroTl,
                       g->macroMirror);
    HIP_TRY(hipGetLastError());
    int rc = 0;
    // (mv_step_n_render's chunks: gyms whose episodes can end within a few ticks are stepped one tick per call)
    const int chunk = g->statusPeriod <= 1 ? 1 : g->batch;
    for (int done = 0; done < k; done += chunk) {
        const int n = std::min(chunk, k - done);
        const MacroCall mc{device_actions, done == 0, done + n == k};
        const int r = step_macro_chunk(g, n, k, render_mode == MV_RENDER_LAST && mc.last, mc);
        if (r < 0) { if (g_err.compare(0, std::strlen(who), who) != 0) g_err = std::string(who) + ": " + g_err; return -1; }
        if (r > 0) { g->warning += (g->warning.empty() ? "" : " | ") + g_err; rc = 1; }   // (every chunk's warning text is kept)
    }
    if (rc) { g_err = g->warning; g->warning.clear(); }
    return rc;
}

}  // namespace

void mvapi::macro_step_free(mv_gym *g)
{
    g->macroPool.release();
    if (g->macroTl) (void)hipFree(g->macroTl);
    g->macroTl = g->macroMirror = g->macroTicks = g->macroActions = nullptr;
    g->macroBytes = 0;
}

int mvapi::publish_macro(mv_gym *g, int q0, const OutPtrs &o, int k, bool cont)   // on the caller's stream
{
    mv::macro::PublishArgs a;
    a.k = k; a.n_envs = g->N; a.A = g->A; a.cont = cont ? 1 : 0;
    for (int j = 0; j < (int)PIPE_BATCH_MAX; ++j) {
        const GymView &v = g->gvp[q0 + std::min(j, k - 1)];
        a.s_rew[j] = v.rewards; a.s_done[j] = v.done; a.s_true[j] = v.true_objective;
    }
    a.rew = o.rewards; a.done = o.done; a.true_obj = g->gv.true_objective;
    const int n = g->N * g->A;
    hipLaunchKernelGGL(mv::macro::macro_publish_kernel, dim3((n + 255) / 256), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int mv_macro_step(mv_gym *g, int32_t k, const int32_t *device_actions, const int32_t *device_ticks, int32_t render_mode)
{
    if (macro_check(g, "mv_macro_step", k, device_actions, render_mode)) return -1;
    HIP_TRY(hipSetDevice(g->device));
    if (macro_alloc(g, "mv_macro_step")) return -1;
    return macro_run(g, "mv_macro_step", k, device_actions, device_ticks, render_mode);
}

int mv_macro_step_host(mv_gym *g, int32_t k, const int32_t *actions, const int32_t *ticks, int32_t render_mode)
{
    if (macro_check(g, "mv_macro_step_host", k, actions, render_mode)) return -1;
    HIP_TRY(hipSetDevice(g->device));
    if (macro_alloc(g, "mv_macro_step_host")) return -1;
    // actions [N*A][6] and ticks [N] lie behind each other in the pool's buffer as in the gym's allocation (ticks first): one copy brings both.  The copy is
    // on the caller's stream, which every earlier call's step launches have been waited for on (the call's end), so the device copies are free to be written.
    const size_t N = (size_t)g->N, words = N + 6 * N * (size_t)g->A;
    StagingPool::Buffer *s = nullptr;
    if (g->macroPool.take(words * sizeof(int32_t), "mv_macro_step_host", s)) return -1;
    int32_t *host = static_cast<int32_t *>(s->host);
    if (ticks) std::memcpy(host, ticks, N * sizeof(int32_t));
    else std::memset(host, 0, N * sizeof(int32_t));
    std::memcpy(host + N, actions, (words - N) * sizeof(int32_t));
    if (sim_join(g)) return -1;
    HIP_TRY(hipMemcpyAsync(g->macroTicks, host, words * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(s->copied, g->stream));
    return macro_run(g, "mv_macro_step_host", k, g->macroActions, ticks ? g->macroTicks : nullptr, render_mode);
}

// The rule of mv_macro_step.h compiled for the CPU (no device): one macro step of k ticks of N envs.  dones [k][N]: what each tick would stage for an env that
// steps; mask [N] or null; left_in [N] (the episode budgets; -1: none); ticks_in [N] or null (every env: k).
int mv_debug_macro_rule_host(const uint8_t *dones, const uint8_t *mask, const int32_t *left_in, const int32_t *ticks_in, int32_t k, int32_t N,
                             uint8_t *steps_out, int32_t *left_out, int32_t *ticks_out)
{
    if (!dones || !left_in || !steps_out || !left_out || !ticks_out || k < 0 || N < 1) return fail("mv_debug_macro_rule_host: bad arguments");
    for (int32_t e = 0; e < N; ++e) {
        left_out[e] = left_in[e];
        ticks_out[e] = mv::macro::macro_ticks_begin(ticks_in != nullptr, ticks_in ? ticks_in[e] : 0, k);
    }
    for (int32_t t = 0; t < k; ++t)
        for (int32_t e = 0; e < N; ++e) {
            const bool steps = mv::macro::macro_steps(mask ? (int)mask[e] : 1, left_out[e], ticks_out[e]);
            steps_out[(size_t)t * N + e] = steps ? 1 : 0;
            if (!steps) continue;
            const int done = dones[(size_t)t * N + e];
            (void)mv::budget::episode_budget_spend(left_out[e], done);
            ticks_out[e] = mv::macro::macro_after_tick(ticks_out[e], done);
        }
    return 0;
}

// The fold of mv_macro_step.h compiled for the CPU (no device): values [k][n] -> out [n], in tick order.
int mv_debug_macro_fold_host(const float *values, int32_t k, int32_t n, float *out)
{
    if (!values || !out || k < 1 || n < 1) return fail("mv_debug_macro_fold_host: bad arguments");
    for (int32_t i = 0; i < n; ++i) {
        float s = values[i];
        for (int32_t t = 1; t < k; ++t) s = mv::macro::macro_fold(s, values[(size_t)t * n + i]);
        out[i] = s;
    }
    return 0;
}

}  // extern "C"
