// megaverse_amd/csrc/mv_reset_envs.hip -- masked env resets: the host side of mv_reset_envs / mv_reset_envs_host (include/megaverse_hip.h).  The kernels are
// the scenario families' reset_masked entry points (mv_step_kernels.h: reset_masked_body) and the episode log's masked clear (mv_episode_log.h:
// episode_log_cut); DESIGN.md 3.9 says which bytes change, where the call stands in the streams' order and where a flagged env's next episode comes from.
#include "mv_api_internal.h"

namespace {

// what both forms refuse: no gym, a closed one, a null mask, a gym that was never reset
int reset_envs_check(mv_gym *g, const void *mask, const char *who)
{
    if (check(g)) return -1;
    if (!mask) return fail(std::string(who) + ": null mask");
    if (!g->wasReset) return fail(std::string(who) + ": call mv_reset first (there is no episode to leave)");
    return 0;
}

// The launches, on the CALLER's stream like mv_reset's: behind whatever the caller enqueued there (the kernel that wrote a device mask), behind every step
// launch enqueued so far (sim_join) and behind the episode log's last update, which lives on that stream; the next step launch waits for all of it
// (simMustWaitUser).  The swap-in writes the public rewards / dones of the last tick (the current output-ring entry), as mv_reset's does.
// Where the next episodes come from:
//   device-drawn (TowerBuilding): the rings are topped up in front of the swap-in and again behind it, on the stream, as in mv_reset: no host wait in either form.
//   host-fed, host mask: the current consumed counts are taken synchronously and every env short of a resident episode gets one (refill_episodes, as in
//     mv_reset): a flagged env never starves, however many calls follow each other.
//   host-fed, device mask: no host wait, so only what is resident counts.  A flagged env whose ring holds no unconsumed episode stays as it is and raises
//     ST_STARVED (the swap-in's own rule); the status words travel back behind the launch, the next stepping call waits for them, reports the starvation as
//     a warning and recovers the ring (refill_episodes), and a refill pass is forced so that the consumed episodes are replaced at once.
int reset_envs_launch(mv_gym *g, const uint8_t *device_mask, const uint8_t *host_mask, int render)
{
    HIP_TRY(hipSetDevice(g->device));
    if (sim_join(g)) return -1;
    if (still_frames_touch(g)) return -1;   // (mv_set_still_frames: every env stale)
    if (flush_device_actions(g)) return -1;   // (a buffer handed over before the call is read now, as in mv_reset; the swap-in clears the flagged envs' actions only)
    const size_t N = (size_t)g->N;
    if (host_mask) {   // nobody flagged: nothing to do, nothing to wait for
        bool any = false;
        for (size_t e = 0; e < N && !any; ++e) any = host_mask[e] != 0;
        if (!any) return 0;
    }
    // (first use; not cleared: `applied[e]` is written for every flagged env and read for flagged envs only)
    if (!g->resetApplied) HIP_TRY(hipMalloc((void **)&g->resetApplied, N));
    if (g->hostEpisodes() && host_mask) {
        // (the periodic read-back may be ticks old, and an earlier masked reset may have consumed episodes since: the current counts, then the uploads)
        if (sync_status_words(g)) return -1;
        g->refillForce = true;
        if (refill_episodes(g, 1) < 0) return -1;   // every env has an unconsumed episode resident
    }
    if (host_mask && g->resetMaskPair.stage(host_mask, N, g->stream, &device_mask)) return -1;
    const OutPtrs outs = last_outputs(g);
    const GymView v = view(g, g->parity, &outs);
    if (g->hostEpisodes()) {
        if (g->lastUpload) HIP_TRY(hipStreamWaitEvent(g->stream, g->lastUpload, 0));   // (uploads in flight: a stream wait, not a host wait)
        launch_reset_envs(v, device_mask, g->resetApplied, g->stream);
        HIP_TRY(hipEventRecord(g->stepDone, g->stream));   // (the kernel reads the ring: no upload overlaps it)
        g->lastStep = g->stepDone;
        if (read_back_status(g, g->stepDone)) return -1;
        g->refillForce = true;   // the flagged envs' rings are an episode short: the pass that sees these words tops them up
        if (!host_mask) g->statusReportDue = true;   // (only the kernel knows whether an env starved: the next stepping call waits for the words and says so)
    } else {
        if (tower_join(g)) return -1;
        launch_tower_draw(v, g->stream);
        launch_reset_envs(v, device_mask, g->resetApplied, g->stream);
        launch_tower_draw(v, g->stream);
    }
    HIP_TRY(hipGetLastError());
    if (host_mask && g->resetMaskPair.mark(g->stream)) return -1;
    if (g->logCapacity > 0) {   // the cut episodes write no record: their running returns and lengths go to zero, nothing else of the log moves
        elog::launch_episode_log_cut(device_mask, g->resetApplied, g->N, g->A, g->logRet, g->logLen, g->stream);
        HIP_TRY(hipGetLastError());
    }
    g->mirrorsFresh = false;
    // every frame of the gym: the unflagged envs' state did not change, so their frames come out as they were; of the state rows (mv_set_state_obs) and scene rows (mv_set_scene_obs) only the
    // flagged envs' are refreshed (device_mask: the caller's, or the half this call's copy went to -- read in stream order)
    if (render && (render_frames(g) || obs_rows_refresh(g, device_mask))) return -1;
    return finish_with_warning(g);
}

}  // namespace

extern "C" {

int mv_reset_envs(mv_gym *g, const uint8_t *device_mask, int32_t render)
{
    if (reset_envs_check(g, device_mask, "mv_reset_envs")) return -1;
    return reset_envs_launch(g, device_mask, nullptr, render);
}

int mv_reset_envs_host(mv_gym *g, const uint8_t *mask, int32_t render)
{
    if (reset_envs_check(g, mask, "mv_reset_envs_host")) return -1;
    return reset_envs_launch(g, nullptr, mask, render);
}

}  // extern "C"
