/*
 * include/megaverse_hip.h -- C ABI of libmegaverse_hip.so, the MI355X-native drop-in for the
 * reference's MegaverseGym hot path.
 *
 * Every entry point replaces one method of class MegaverseGym in the reference's pybind11 module
 * (reference: src/libs/bindings/megaverse.cpp; the Python-visible table is at :267-292).  A
 * maintainer binds these from the existing pybind shim or via ctypes
 * (megaverse_amd/extension.py does exactly that).  Plain pointers and sizes only; no torch, no
 * STL, no exceptions.  Return value: 0 = ok, negative = error (mv_last_error() has the text);
 * the reference instead logs and calls exit(-1) (src/libs/util/src/tiny_logger.cpp:109-113).
 * mv_step* / mv_reset may also return 1 = done, with a WARNING in mv_last_error(): a fixed capacity this build has and the
 * reference has not (visible primitives per frame, collision candidates, the voxel chunk, an episode record, a starved episode
 * ring) was hit since the last report.  The call did all of its work; the condition is reported once.
 *
 * Threading: like the reference every call is made from one host thread per gym.
 * All device work is enqueued on one HIP stream (mv_set_stream; default: the null stream);
 * mv_step() returns without synchronising, host getters synchronise that stream.
 */
#ifndef MEGAVERSE_HIP_H
#define MEGAVERSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mv_gym mv_gym;

typedef struct mv_config {
    const char *scenario;          /* case-insensitive registered name (scenarios/init.hpp:26-57); "TowerBuilding" */
    int32_t obs_width, obs_height; /* megaverse.cpp:38 w, h */
    int32_t num_envs;              /* envs simulated by THIS process (one process per GPU) */
    int32_t num_agents_per_env;
    int32_t num_simulation_threads;/* worker threads of the background episode generator (every scenario but TowerBuilding, whose generator runs on the device);
                                      <= 0: this process's share of the host's cores (cores it may use / ranks of the job, at most 16); MV_FEEDER_THREADS overrides;
                                      stepping itself has no threads */
    int32_t use_vulkan;            /* accepted for signature parity; ignored */
    int32_t device;                /* HIP device ordinal */
    const char *const *param_keys; /* FloatParams (megaverse.cpp:45, scenario.hpp:225-242) */
    const float *param_vals;
    int32_t num_params;
    /* env sharding across GPUs: this process owns global envs [env_offset, env_offset+num_envs)
     * of total_envs; mv_seed() draws the per-env seeds for the whole job so that a sharded run is
     * bit-identical to the single-process run.  0 / 0 = not sharded. */
    int32_t env_offset, total_envs;
    /* 0 or 1: this process owns a contiguous block.  k > 1: it owns every k-th env starting at env_offset
     * (global index of local env j = env_offset + j * env_stride): the layout of a multi-task job that deals
     * scenarios round-robin by env index (megaverse_env.py:27-39, one gym per scenario). */
    int32_t env_stride;
} mv_config;

const char *mv_last_error(void);
int mv_device_count(void);   /* HIP devices this process can see (0 when there is none or the runtime cannot start) */
/* Version of this ABI.  2: mv_step* / mv_reset / mv_step_many / mv_group_step return 1 for "done, with a warning" (version 1 returned -1 for the same
 * conditions BEFORE doing the work): callers written as `if (mv_step(g)) fail();` must test `< 0` instead -- ask here which contract the library has. */
int mv_abi_version(void);

/* MegaverseGym::MegaverseGym (megaverse.cpp:38-58) / close (:227-243).  mv_close is idempotent
 * and valid before the first reset (megaverse/tests/test_env.py:28-30). */
int mv_create(const mv_config *cfg, mv_gym **out);
int mv_close(mv_gym *g);
int mv_destroy(mv_gym *g); /* mv_close + free the handle */

int mv_num_agents(const mv_gym *g);                 /* numAgents(), megaverse.cpp:71-74 */
int mv_action_space_sizes(int32_t *out6);           /* actionSpaceSizes(), :95-98 -> {3,3,3,2,2,3} */
int mv_seed(mv_gym *g, int32_t seed);               /* seed(), :60-69 */
int mv_reset(mv_gym *g);                            /* reset(), :76-93 (+ first render) */

/* setActions(), :100-116: multi-discrete -> Action bitmask for one agent (host staging) */
int mv_set_actions(mv_gym *g, int32_t env_idx, int32_t agent_idx, const int32_t *actions, int32_t n);
/* batched forms the reference lacks (SURVEY.md 3.2 hot loop iii): [N*A][6] multi-discrete.  The device form launches nothing: the buffer
 * is read by the NEXT step kernel, in the order of the caller's stream (keep it unchanged until that mv_step has been enqueued). */
int mv_set_actions_batched(mv_gym *g, const int32_t *host_actions);
int mv_set_actions_device(mv_gym *g, const int32_t *device_actions);
/* benchmark policy: i.i.d. uniform per head, counter-based (seed, step, agent, head) -> action;
 * same stream as megaverse_amd.rollout.sample_actions() on the host */
int mv_sample_random_actions(mv_gym *g, uint32_t seed, uint32_t step_index);
/* which generator mv_sample_random_actions / mv_step_n draw from: MV_POLICY_MULTIDISCRETE (default; = action_space.sample(),
 * megaverse_env.py:110-112) or MV_POLICY_SINGLE_BIT = Action(1 << randRange(0, NumActions)), the reference's own benchmark policy
 * (src/apps/megaverse_test_app.cpp:140-147); host twins: megaverse_amd/rollout.py */
enum { MV_POLICY_NONE = 0, MV_POLICY_MULTIDISCRETE = 1, MV_POLICY_SINGLE_BIT = 2,
       MV_POLICY_SEQUENCE = 3 };   /* mv_step_n / mv_group_step only: replay the action ring, mv_set_action_ring */
int mv_set_sample_policy(mv_gym *g, int32_t policy);
/* Action rings (no reference counterpart: its callers set every agent's action every tick, megaverse.cpp:100-116): the one INPUT of a batched call, as
 * mv_set_output_ring holds its outputs.  device_actions: [count][N*A][6] int32 multi-discrete actions in device memory, encoding and agent order as for
 * mv_set_actions_device; count = 0 detaches.  Nothing is launched and nothing is copied: the step kernels of a call with policy MV_POLICY_SEQUENCE read the
 * caller's buffer -- tick j of mv_step_n / mv_group_step(k, MV_POLICY_SEQUENCE, seed, first_step_index) acts on entry (first_step_index + j) % count, in
 * uint32 arithmetic (the stateless indexing the random policies use for (seed, first_step_index + j); seed is ignored; count = 1 is action repeat).  Such a
 * call takes every batched launch path the random policies take, under the same conditions, and falls back to tick-by-tick launches where they do; a
 * pending mv_set_actions* buffer is superseded for its ticks, as the random policies supersede it.  Without a ring (in a group: on every member, each
 * keeps its own) the call is an error.  mv_step, mv_step_many, MV_POLICY_NONE and the random policies ignore the ring; mv_set_sample_policy does not accept
 * MV_POLICY_SEQUENCE.
 * Ordering: this call is the one ordering point.  Whatever the caller enqueued on the gym's stream before it -- the kernel that filled the ring -- is ordered
 * before the next step launch; the calls after that one pipeline freely (replaying a static script costs no dependency).  A caller that rewrites entries
 * calls mv_set_action_ring again with the same arguments.  An entry a call reads must stay unchanged until the caller's stream has passed the end of that
 * call.  The buffer is the caller's; mv_reset leaves the ring attached. */
int mv_set_action_ring(mv_gym *g, int32_t count, const int32_t *device_actions);
/* Forks (no reference counterpart: its envs are separate objects that cannot be copied, env.hpp).  src_of: int32 [N].  src_of[d] = s, 0 <= s < N, s != d:
 * env d leaves its running episode and continues env s's, from s's current state.  src_of[d] = -1 or d: env d is left alone.  One launch gathers, for
 * every such d, env s's EPISODE STATE -- every per-env array a tick or a frame setup reads or writes, whole strides: EnvHeader (but the fields below),
 * boxes, objects, every agent's AgentState (reward-shaping coefficients and total_reward included: a fork inherits its source's reward function), the
 * scenario's own arrays (voxel chunk, terrain, reward objects, heightmap, arrangement items, Sokoban cells, hex boxes and objects, BoxAGoneState,
 * FootballState) and, with the episode log on, the agents' running returns and the env's running length (env d's cut episode writes no record, as with
 * mv_reset; the record at the fork's end covers the episode from s's start).  Env d keeps its IDENTITY: next_seed, seed_is_env_seed, episodes_consumed and
 * starved of its header, its status words, its ring of resident next episodes and its generator -- when the forked episode ends, env d takes the next
 * episode of its OWN sequence, the one it would have taken had its own episode ended; the episode feeder and the refill protocol see nothing unusual.
 * Not touched: the public rewards / dones / true objectives, the output rings and the observation slab (they describe the last stepped tick; mv_render after
 * a fork draws the forked envs' current views), pending actions.
 * Ordering: the call is an ordering point, as mv_set_actions_device is.  The copy runs behind every step launch enqueued so far and behind whatever the
 * caller enqueued on the gym's stream (the kernel that wrote the map); the next step launch runs behind the copy.  The device form never synchronises
 * with the host, and the map is read when the copy runs: keep it unchanged until then (in stream order: until the next stepping call has been enqueued).
 * Invalid entries: a source may serve any number of destinations but may not itself be a destination in the same call (an in-place gather cannot honour a
 * chain), and an index must be -1 or 0 .. N - 1.  mv_fork_envs_host validates on the host: -1 with text, nothing forked.  The device form cannot: the
 * kernel skips every entry involved (those envs stay as they were), applies the valid ones and raises a status bit, which the NEXT stepping call reports
 * once as return 1 with a warning, like every capacity condition -- that call waits for the status words behind the fork (the one host wait the device
 * form costs, paid there; the host form costs none).
 * Refused (-1): no gym, a closed gym, before the first mv_reset, a null map, and a gym that belongs to an mv_group (its streams are the group's; forks
 * inside groups and across gyms are out of scope; a map in which a source is also a destination -- a chain, a swap, a cycle -- is what mv_resample_envs
 * below takes). */
int mv_fork_envs(mv_gym *g, const int32_t *device_src_of);   /* map in device memory, read in the order of the gym's stream */
int mv_fork_envs_host(mv_gym *g, const int32_t *src_of);     /* map in host memory: validated here, copied, then as above */
int64_t mv_fork_bytes_per_env(const mv_gym *g);              /* bytes a fork reads and writes per destination (the episode log's included when it is on); -1: no gym */
/* Resampling (no reference counterpart): a fork map without the fork's restriction.  src_of: int32 [N], read as by mv_fork_envs, and
 *     new state of env d = the state env src_of[d] had BEFORE the call
 * for ANY map: chains, swaps, cycles, a source that serves many envs, a source that is overwritten itself -- what a population method (sequential Monte
 * Carlo, Go-Explore's selection, evolutionary search) does when it resamples N envs from the same N envs.  src_of[d] = -1 or d: env d is left alone.
 * What moves is the fork's EPISODE STATE, what stays is the fork's IDENTITY (above): after a swap each of the two envs continues the other's episode and,
 * when that ends, takes the next episode of its OWN sequence.  Not touched, as under a fork: the public rewards / dones / true objectives, the output rings,
 * the observation slab, pending actions.
 * How: two launches on one stream.  An env is STAGED when its entry is valid and another valid entry names it as a source: its old state is still needed
 * while its new one arrives.  Phase 1 reads, for every valid d, env src_of[d] from the live arrays and writes env d's live arrays -- or, where d is staged,
 * slot d of a staging arena; phase 2 copies every staged env's slot to its live arrays.  No live env that phase 1 reads is written in phase 1 (whoever is
 * read is named, and a named env with a valid entry is staged), phase 2 touches no other env, and the launch boundary is the barrier.  A map that is a valid
 * fork map stages nobody and leaves exactly what mv_fork_envs leaves.
 * Memory: the staging arena holds N x (bytes per env, header and the episode log's accumulators included -- whether the log is on or not, so that switching
 * it on later needs nothing) plus a byte per env.  The first call on a gym -- either form -- allocates it: that one call may wait on the host inside the
 * allocator, no later one does.  It is counted in mv_arena_bytes from then on and freed by mv_close.
 * Ordering: that of mv_fork_envs, word for word.  The call is an ordering point; the copy runs behind every step launch enqueued so far and behind whatever
 * the caller enqueued on the gym's stream (the kernel that wrote the map -- torch.multinomial, say); the next step launch runs behind the copy.  The device
 * form runs on the caller's stream, never synchronises with the host and always enqueues both launches; keep the map unchanged until the next stepping call
 * has been enqueued.  The host form sees the whole plan: a map that leaves every env alone launches nothing, one that stages nobody launches phase 1 alone;
 * where mv_fork_envs_host may go to the simulation stream, so may it.
 * Invalid entries: an index that is neither -1 nor 0 .. N - 1, and nothing else.  An invalid entry names nobody.  mv_resample_envs_host: -1 with text,
 * nothing copied.  The device form skips that entry -- the env stays as it was, and every entry that names that env still receives its pre-call state --
 * and raises a status bit of its own, which the NEXT stepping call reports once as return 1 with a warning that names mv_resample_envs (that call waits
 * for the status words, as after mv_fork_envs).
 * Refused (-1 with text): no gym, a closed gym, before the first mv_reset, a null map, a gym that belongs to an mv_group. */
int mv_resample_envs(mv_gym *g, const int32_t *device_src_of);   /* map [N] in device memory, read in the order of the gym's stream */
int mv_resample_envs_host(mv_gym *g, const int32_t *src_of);     /* map [N] in host memory: validated here, copied, then as above */
int64_t mv_resample_staging_bytes(const mv_gym *g);              /* 0 before the first call; -1: no gym */
/* Masked resets (no reference counterpart: VectorEnv::reset resets every env, vector_env.cpp:110-120).  mask: one byte per env, [N]; a torch.bool tensor is
 * such a mask.  mask[e] != 0: env e abandons its running episode and takes the NEXT EPISODE OF ITS OWN SEQUENCE -- the one it would have taken had its
 * episode ended at this point: episodes_consumed + 1, its own seed chain, its own ring slot (a fork destination keeps its identity, so this is how it hands
 * a forked episode back).  mask[e] == 0: env e is untouched, byte for byte.
 * State: a flagged env ends up exactly where mv_reset would have put it at this moment -- every per-env array the scenario's swap-in writes under mv_reset
 * (header, boxes, objects, agents, the scenario's own arrays) and its status word; its entries of the public rewards and dones (the current entry of an
 * output ring where one is attached) and its pending actions are cleared as mv_reset clears them; its true objectives stay what they were, as under
 * mv_reset.  A pending mv_set_actions_device buffer is read first, as in mv_reset; unflagged envs keep their actions.  An all-zero mask changes no byte of
 * the gym; an all-ones mask leaves every env as mv_reset does.
 * What it is not: a whole-gym reset.  mv_ticks_since_reset keeps counting, output rings stay attached and their tick count is not rewound.
 * Episode log (when on): the cut episode of a flagged env writes no record; its agents' running returns and its running length go to zero; nothing else in
 * the log changes, neither records nor counts.
 * Observation: render != 0: behind the swap-in the call runs the observation pass where mv_render would draw, so flagged envs show their new episode's first
 * view as an auto-reset tick's observation does; the pass draws every frame of the gym, and the unflagged envs' frames come out byte-identical because their
 * state did not change.  render == 0: the slab is not touched.
 * Ordering: the call is an ordering point, as mv_fork_envs is.  It runs behind every step launch enqueued so far and behind whatever the caller enqueued on
 * the gym's stream (the kernel that wrote the mask); the next step launch runs behind it.  The device form never waits on the host: the mask is read when
 * the kernel runs -- keep it unchanged until then (in stream order: until the next stepping call has been enqueued).
 * Episodes, three cases.  (1) Device-drawn episodes (TowerBuilding): the rings are topped up in front of the swap-in and behind it, as in mv_reset, on the
 * stream, in both forms: no host wait, no starvation.  (2) Host-fed gyms (every other scenario; Collect too, wherever its episodes are drawn: they reach the
 * ring through the host's refill protocol), host form: the call takes the current consumed counts synchronously, as mv_reset does, and makes sure every
 * flagged env has an unconsumed episode resident before the launch: it never starves, however often it is repeated.  (3) Host-fed gyms, device form: no
 * host wait, so only resident episodes count (two or three per env; right behind mv_reset one, the rest arrive with the next stepping calls).  A flagged env whose ring holds no unconsumed episode is LEFT AS IT IS (its log
 * accumulators too) and the starvation bit is raised; the next stepping call waits for the status words behind the launch, reports it once as return 1 with a
 * warning and recovers the ring, as it does for an env that finished twice; a refill pass is forced so that the host replaces the consumed episodes promptly.
 * An all-zero mask: the host form sees it on the host and returns behind the flush of pending device actions -- nothing is launched, nothing drawn; the device
 * form cannot know, so it launches as always (every wave exits) and, with render != 0, redraws the whole gym, byte for byte what it was.
 * The first call on a gym -- either form -- allocates 3 N bytes of device memory and 2 N pinned bytes (the host form's copy of its mask, which flagged envs
 * took an episode): that one call may wait on the host inside the allocator; "never waits on the host" holds for every call after it.
 * Members of an mv_group are supported: the call follows mv_reset's path, which is valid for them.
 * Refused (-1 with text): no gym, a closed gym, before the first mv_reset, a null mask. */
int mv_reset_envs(mv_gym *g, const uint8_t *device_mask, int32_t render);   /* mask [N] in device memory, read in the order of the gym's stream */
int mv_reset_envs_host(mv_gym *g, const uint8_t *mask, int32_t render);     /* mask [N] in host memory */
/* Level seeds (the per-env form of mv_seed; no reference counterpart: MegaverseGym::seed re-seeds every env from one master stream, megaverse.cpp:60-69).
 * seeds: int32 [N].  seeds[e] >= 0: env e receives Env::seed(seeds[e]) (env.cpp:52-55) -- the value mv_seed hands an env from its master stream ([0, 2^30)
 * there, any non-negative int32 here; megaverse_amd.distributed.env_seeds(S, N) lists mv_seed(S)'s).  seeds[e] < 0: env e is left alone, byte for byte: its
 * resident episodes and its place in the refill protocol do not move.
 * Meaning, in both forms: exactly mv_seed's, per env.  The env's RUNNING episode goes on untouched; the episodes drawn ahead from its old stream are
 * dropped; its generator restarts, so that its next reset -- an auto-reset, mv_reset, mv_reset_envs -- plays the first episode of the new stream and the ones
 * after it follow that chain.  Two envs given the same seed play the same level sequence; mv_seed_envs* followed by mv_reset_envs* on the same envs means
 * "start level s in env d now".  Valid before the first mv_reset, where it acts as mv_seed for the chosen envs.
 * IDENTITY: an env slot's episode stream is what forks, resampling, loads and masked resets leave alone (mv_fork_envs above); this call is the one that
 * REPLACES it.  Nothing else of the slot moves: episodes_consumed keeps counting, the episode log's running returns, masks, budgets and state observations
 * need nothing.
 * Sokoban keeps its per-env shuffled level list (SokobanScenario::levels) across Env::seed, as under mv_seed and in the reference: only what the flagged
 * envs' ahead-of-time draws took from it is put back.  A Sokoban env's levels therefore depend on how far its list was advanced, not on the seed alone.
 * Ordering: both forms are ordering points on the gym's stream, like mv_reset_envs: behind every step launch enqueued so far and behind whatever the caller
 * enqueued there (the kernel that wrote a device array), in front of the next step launch and the next episode draw.
 * Device-drawn gyms (TowerBuilding), both forms: no host wait.  One launch re-seeds the flagged envs' generators and empties their rings, the draw launch
 * behind it makes the new streams' first episodes resident in stream order.  The device array is read when the kernel runs: keep it unchanged until then
 * (in stream order: until the next stepping call has been enqueued).  The host form copies its array through a pinned staging pair (allocated by the first
 * call, which may wait inside the allocator).
 * Host-fed gyms (every other scenario), host form: the generators live in the host's episode feeder, which needs the flagged envs' current consumed
 * counts: the call WAITS ON THE HOST for everything enqueued on the gym's streams, as mv_seed does.  It then wipes the flagged envs' rings alone, restarts
 * their streams in the feeder (every other env's queued, in-flight and ready episodes are untouched) and, before it returns, uploads the first episode of
 * the new stream for every flagged env: a reset of either form that follows never starves, however many seed / reset pairs follow each other without a
 * stepping call.  With every entry negative the call returns 0, waits for nothing and launches nothing.  Returns 1 with a warning like a stepping call
 * where the refill pass meets a capacity flag.
 * Host-fed gyms, device form: refused (-1 with text, nothing changed): the generators live on the host -- use mv_seed_envs_host.
 * Members of an mv_group are supported, as by mv_reset_envs.
 * Refused (-1 with text): no gym, a closed gym, a null array. */
int mv_seed_envs(mv_gym *g, const int32_t *device_seeds);   /* seeds [N] in device memory, read in the order of the gym's stream */
int mv_seed_envs_host(mv_gym *g, const int32_t *seeds);     /* seeds [N] in host memory */
/* Step masks (no reference counterpart: VectorEnv::step steps every env, vector_env.cpp:89-108).  mask: one byte per env, [N]; a torch.bool tensor is such a
 * mask, as in mv_reset_envs.  mask[e] != 0: env e steps.  mask[e] == 0: env e is FROZEN.  The mask stays attached, like an action ring, until it is detached
 * (NULL) or replaced, and every tick of every later stepping call reads it: mv_step, mv_step_no_render, mv_step_n, mv_step_n_render in all three render modes,
 * every policy.  With no mask attached everything is what it is without these calls, byte for byte and launch for launch.
 * A frozen env on a tick: no byte of its episode state changes -- header (episode clock included), boxes, objects, agents, the scenario's own arrays, its
 * status word, episodes_consumed, its ring of resident episodes, TowerBuilding's generator.  It takes no episode and cannot starve; a pending starved swap-in
 * stays pending.  Its rewards are +0.0f and its done is 0, in the public arrays and in every ring entry of that tick; its true objectives stay what they were.
 * Its actions for that tick -- pending mv_set_actions*, the action-ring entry, the random draw (counter-based: nothing to advance) -- are ignored and
 * discarded: they do not wait for the thaw.  Tick indices stay the gym's: tick j of a call uses first_step_index + j for the envs that step, whatever is
 * frozen; mv_ticks_since_reset and the output rings' tick count advance as always.
 * Episode log (when on): a frozen tick adds nothing to the env's running returns or length and writes no record; a record written later has length = the
 * ticks the env actually stepped, end_tick in the gym's tick count.
 * Observation: drawn as always where the mode draws at all, from the unchanged state: a frozen env's frame is its current view, byte-identical to its
 * previous one, time bar included.  (The frame setup and the raster of a frozen frame are not skipped; mv_set_draw_mask, below, skips both.)
 * Everything else acts regardless of the mask: mv_reset resets every env and leaves the mask attached; mv_reset_envs, mv_fork_envs* and mv_resample_envs*
 * treat frozen envs like any other -- a frozen env as a fork source is a savepoint that keeps.
 * Ordering: the call is an ordering point, as mv_set_action_ring is: whatever the caller enqueued on the gym's stream before it is ordered before the next
 * step launch; the calls after that one pipeline freely.  Neither form waits on the host.  Device form: nothing is copied; the buffer is the caller's and
 * stays unchanged until the caller's stream has passed the end of the last call that reads it; after rewriting it, call mv_set_step_mask again.  Host form:
 * the bytes go to a gym-owned device buffer (allocated at first use, counted in mv_arena_bytes, freed by mv_close), by a copy ordered behind every step
 * launch enqueued so far: a step kernel running ahead on the simulation stream never sees a half-written mask.
 * Valid before the first mv_reset.  Refused (-1 with text): no gym, a closed gym, a gym in an mv_group; mv_group_create and mv_step_many refuse a gym with a
 * mask attached (the union launches read none). */
int mv_set_step_mask(mv_gym *g, const uint8_t *device_mask);   /* [N] in device memory; NULL detaches */
int mv_set_step_mask_host(mv_gym *g, const uint8_t *mask);     /* [N] in host memory; NULL detaches */
int mv_get_step_mask(const mv_gym *g);                         /* 0: none, 1: device form, 2: host form; -1: no gym */
/* Draw masks (no reference counterpart: the reference draws every env of every step).  mask: one byte per env, [N]; a torch.bool tensor is such a mask.
 * mask[e] != 0: env e is drawn as it is without these calls.  mask[e] == 0: env e is UNDRAWN: in every observation pass the gym enqueues while the mask is
 * attached, none of env e's A frames is set up or drawn, and no byte of their rows is written, in either observation layout (mv_set_obs_layout).  The rows keep
 * whatever they held: in an output ring the entry of `count` ticks ago, in the slab the last frame drawn there, or the caller's own bytes -- stale rows are
 * the caller's to tell apart; the gym carries nothing over between hand-over slots or ring entries.
 * Which passes: mv_step; mv_step_n and mv_step_n_render in every mode and policy (MV_RENDER_LAST draws the masked-in envs of the last tick; MV_RENDER_NONE
 * draws nothing, as always); the frame behind mv_reset; mv_reset_envs(..., render = 1); mv_render.  mv_draw_hires ignores the mask: it draws every env.
 * Nothing else changes.  Physics, scenario logic, auto-reset and refill; rewards, dones and true objectives, and where and when they are published (the fast
 * pass publishes them with its first workgroups, whatever the mask says: also with an all-zero mask); the episode log, the status words and the capacity
 * flags are the bytes an unmasked twin produces.  An undrawn frame has no list and so raises no ST_VISIBLE.
 * The mask belongs to the env SLOT, like a budget: mv_fork_envs*, mv_resample_envs*, mv_load_envs*, mv_reset and mv_reset_envs move or replace state and leave
 * the mask alone.  It composes with step masks and budgets: a frozen and undrawn env costs one mask load in the step launch and workgroups that leave behind
 * their frame look-up in the pass.  The mask stays attached until it is detached (NULL) or replaced.  With no mask attached (and neither step mask nor budget)
 * the gym launches the step kernels it launched before; the pass kernels differ by one uniform branch per workgroup.
 * Scheduling only, not pixels: undrawn frames are the cheapest in the pass's cost order and fill its finely cut tail segment first.
 * Ordering: mv_set_step_mask's.  Both forms are ordering points: whatever the caller enqueued on the gym's stream before the call is ordered before the next
 * step launch; neither form waits on the host.  Device form: nothing is copied; the buffer is the caller's and stays unchanged until the caller's stream has
 * passed the end of the last call that reads it; after rewriting it, call mv_set_draw_mask again.  Host form: the bytes go to a gym-owned device buffer
 * (allocated at first use, counted in mv_arena_bytes, freed by mv_close) through pinned staging, by a copy ordered behind every step launch enqueued so far.
 * Valid before the first mv_reset.  Refused (-1 with text): no gym, a closed gym, a gym in an mv_group; mv_group_create and mv_step_many refuse a gym with a
 * draw mask attached (the union launches read none). */
int mv_set_draw_mask(mv_gym *g, const uint8_t *device_mask);   /* [N] in device memory, read in place; NULL detaches */
int mv_set_draw_mask_host(mv_gym *g, const uint8_t *mask);     /* [N] in host memory, copied through a pinned staging buffer; NULL detaches */
int mv_get_draw_mask(const mv_gym *g);                         /* 0: none, 1: device form, 2: host form; -1: no gym */
/* Still frames (no reference counterpart: the reference draws every env of every step).  An env that did not step -- frozen by a step mask, halted by its
 * episode budget, stopped inside a macro step -- has the state it had, and drawing it again leaves the bytes the last drawing left.  on != 0: in every later
 * observation pass of the stepping calls (mv_step; mv_step_n and mv_step_n_render in every mode and policy; mv_macro_step) an env's A frames are set up and
 * drawn only where the env's state may have changed since its frames were drawn last.  Otherwise no frame is set up and no ray is cast, and the env's rows
 * show the frame drawn last: in the single observation slab they are left alone; in an output ring (mv_set_output_ring with an observation ring) the rows of
 * the tick's entry are copied on the device from the entry that holds the env's latest frame, by ONE launch per stepping call behind the call's passes (a
 * source row is read once and stored to every still entry of the call).
 * The promise: rewards, dones, true objectives, state, status words, the episode log, state observations and EVERY BYTE of every observation row are those
 * of a twin gym with the option off.  Undrawn rows of a draw mask (mv_set_draw_mask) stay untouched as always, and such an env counts as not drawn.
 * The rule (megaverse_amd/csrc/mv_still_frames.h states it for kernels and host alike): one byte `stale` per env, all 1 when the option is switched on.  A
 * tick the env stepped in sets it, with or without a pass (MV_RENDER_NONE ticks, the undrawn ticks of MV_RENDER_LAST); a pass that draws the env clears it; a
 * frozen, halted or macro-stopped tick leaves it alone.  Every call that can change an env's state, or what or where the gym draws, sets ALL bytes with one
 * memset on the gym's stream: mv_reset, mv_reset_envs*, mv_fork_envs*, mv_resample_envs*, mv_load_envs*, mv_seed, mv_render, mv_set_obs_buffer,
 * mv_set_output_ring, mv_set_obs_layout, mv_set_pixel_mode, mv_set_render_resolution and the mv_debug_set_* setters.  Conservative on purpose: a planner that
 * forks every iteration redraws its frozen root once per iteration.  Within one call an env's passes are a drawn prefix followed by a still suffix.
 * A caller that writes into observation rows itself must not expect a still env's rows to be drawn over.
 * Default: off, and a gym that never switches it on launches the kernels it launched, argument for argument.  While on, the step launches are the MASKED
 * kernels, never the two-wave software-pipelined one, and with an observation ring attached overlapped passes (mv_set_pass_overlap) are not taken: pass c + 1
 * on its side stream could draw into the entry the carry of call c is still reading when the ring is exactly two calls deep.  mv_set_pass_overlap stays
 * accepted; the calls simply run in order.  mv_draw_hires ignores the option.
 * Ordering: mv_set_draw_mask's.  Switching it on or off is an ordering point and never waits on the host.  The gym's arrays (N bytes and N*A int32) are
 * allocated when the option is first switched on, counted in mv_arena_bytes and freed by mv_close.
 * Refused (-1 with text): no gym, a closed gym, a gym in an mv_group; mv_group_create and mv_step_many refuse a gym that has it on. */
int mv_set_still_frames(mv_gym *g, int32_t on);
int mv_get_still_frames(const mv_gym *g);                      /* 0: off, 1: on; -1: no gym */
/* State observations (no reference counterpart: the reference hands out pixels, rewards and dones).  One row of MV_STATE_OBS_FLOATS = 16 float32 per agent,
 * agent-major [N*A][16], taken from the env's state AFTER the tick, auto-reset included: a tick that finished an episode shows the first state of the next
 * episode, as its frame does.  Columns (megaverse_amd/csrc/mv_state_obs.h states them for kernels and host alike):
 *    0..2  position x, y, z      3..6  yaw basis m00, m02, m20, m22      7  pitch      8, 9  horizontal velocity x, z      10  vertical velocity
 *    11  1.0f while the agent carries an object, else 0.0f      12, 13  the env's episode time and episode length in seconds      14  the agent's total
 *    reward of the episode      15  +0.0f (reserved)
 * Values are copied, not recomputed: every bit is the bit of the simulator's state.
 * The buffer is one more ring beside mv_set_output_ring's three: [entries][N*A][16], entries = the output ring's count at the moment of the call, or 1 without
 * a ring; tick t goes to the entry its rewards go to.  While a buffer is attached mv_set_output_ring is refused: detach the state observations first.
 * Which ticks: every tick of every stepping call -- mv_step, mv_step_no_render, mv_step_n and mv_step_n_render in every mode and policy, MV_RENDER_NONE
 * included -- whether the env stepped or was frozen (mv_set_step_mask) or halted (mv_set_episode_budget: it reports its unchanged state) and whether it is drawn
 * (mv_set_draw_mask) or not.  The rows are visible on the gym's stream when the call's rewards and dones are; nothing waits on the host.  mv_reset,
 * mv_reset_envs(..., render = 1) and mv_render refresh the rows of the last tick's entry from the current state (mv_reset_envs: the flagged envs' rows only;
 * the others keep theirs).  Forks, resampling and loads move state and touch no output: the next stepping call or mv_render shows it, as for frames.
 * Nothing else changes: rewards, dones, true objectives, pixels, the episode log and the status words are those of a gym without a buffer.  With a buffer
 * attached the step launches are the instantiations a step mask selects, and every stepping call enqueues one more small launch on the gym's stream; a gym that
 * never attaches one launches exactly what it launched before.
 * Ordering: mv_set_step_mask's.  The call is an ordering point and never waits on the host; the buffer is the caller's and must stay valid until the caller's
 * stream has passed the end of the last call that writes it.  Attaching again replaces the buffer; NULL detaches.  Valid before the first mv_reset.
 * Refused (-1 with text): no gym, a closed gym, a gym in an mv_group; mv_group_create and mv_step_many refuse a gym with state observations attached (the
 * union launches write none).  mv_get_state_observation: the last tick's row of one agent, after waiting for the gym's stream; refused with nothing attached.
 * mv_debug_state_obs_host: the record on the CPU, from the bytes of one AgentState (128) and one EnvHeader (128) of megaverse_amd/csrc/mv_types.h: no device. */
enum { MV_STATE_OBS_FLOATS = 16 };
int mv_set_state_obs(mv_gym *g, float *device_buf);   /* [max(1, ring count)][N*A][16] float32 in device memory; NULL detaches */
int mv_get_state_obs(const mv_gym *g);                /* 0: none, else the number of entries; -1: no gym */
int mv_get_state_observation(mv_gym *g, int32_t env_idx, int32_t agent_idx, float *out_host16);  /* last tick's row; waits for the gym's stream */
int mv_debug_state_obs_host(const void *agent_state, const void *env_header, float *out16);      /* the pack function, on the host */
/* Scene observations (no reference counterpart), the per-ENV counterpart of the state observations: one row of MV_SCENE_OBS_FLOATS = 32 float32 per env,
 * [N][32], taken from the env's state AFTER the tick, auto-reset included -- the level, the goal and the ball that the per-agent rows leave out.  Two
 * conversions: "copied" moves the 32 bits (a -0.0f or a NaN's payload survives); "int" converts an int32 with (float), exactly (every value is far below 2^24).
 * Columns (megaverse_amd/csrc/mv_scene_obs.h states them for kernels and host alike, with the units):
 *    0  the scenario family id (SCN_*), int      1..3  the room's L, H, W in voxels, int      4  num_frames, int      5, 6  episode time and length in seconds,
 *    copied      7  the env's episode counter: it changes exactly on the ticks the env takes a new episode, int      8  solved, int      9  highest_tower
 *    (TowerBuilding: the tower; Collect: the +1 diamonds collected), int      10  bz_reward, copied      11..14  num_objects, num_rewards, num_platforms,
 *    num_terrain, int      15  +0.0f (reserved)
 *    16..31 by scenario, +0.0f wherever nothing is listed and for every scenario not listed:
 *      TowerBuilding   16..19  the building zone: min x, max x, min z, max z, int
 *      Obstacles*      16  the number of exit terrain boxes, int      17..19, 20..22  min and max (exclusive) of the first one in voxels, zeros when there is
 *                      none, int      23  the diamonds still there, int
 *      HexExplore      16, 17  x, z of the target, copied
 *      Football        16..18  the ball's position      19  its drawn radius      20..22  its velocity, all copied      23  this tick's kicks, int
 *                      24..26  its angular velocity, copied      27  this tick's contact bits, int      28..30  the pending force, copied
 * Buffer, ticks, visibility, refresh (mv_reset, mv_reset_envs(..., render = 1): the flagged envs' rows only, mv_render), what forks / resampling / loads / seeds
 * leave alone, ordering and refusals are mv_set_state_obs's, with [entries][N][32] for [entries][N*A][16]: frozen, halted, macro-stopped, undrawn and still envs
 * report too; mv_macro_step leaves its last tick's rows; mv_set_output_ring is refused while attached; mv_group_create and mv_step_many refuse a gym that has
 * it attached.  A stepping call enqueues ONE publication launch on the gym's stream for whichever of the two records are attached, both included
 * (mv_debug_launch_counts counts it in out[1]).  A gym that attaches neither launches exactly what it launched before.  The staging rows are counted in
 * mv_arena_bytes from the first attach on.
 * mv_debug_scene_obs_host: the record on the CPU, from the bytes of one EnvHeader (128), 16 TerrainBox (32 each), rewards_len <= 96 MovableObject (4 each) and
 * one FootballState (64) of megaverse_amd/csrc/mv_types.h; inputs the scenario does not read may be NULL: no device. */
enum { MV_SCENE_OBS_FLOATS = 32 };
int mv_set_scene_obs(mv_gym *g, float *device_buf);     /* [max(1, ring count)][N][32] float32 in device memory; NULL detaches */
int mv_get_scene_obs(const mv_gym *g);                  /* 0: none, else the number of entries; -1: no gym */
int mv_get_scene_observation(mv_gym *g, int32_t env_idx, float *out_host32);   /* last tick's row; waits for the gym's stream */
int mv_debug_scene_obs_host(int32_t scenario, const void *env_header, const void *terrain16, const void *rewards, int32_t rewards_len,
                            const void *football_state, float *out32);         /* the pack function on the host; unused inputs may be NULL */
/* Entity observations (no reference counterpart): the objects themselves -- E rows of MV_ENTITY_OBS_FLOATS = 8 float32 per env, [N][E][8], taken from the env's
 * state AFTER the tick, auto-reset included.  They are the table the instance labels of mv_set_seg_obs (MV_SEG_INSTANCE_U16) index into.
 * E (mv_entity_obs_rows) is fixed for a gym: it depends on the scenario and the agent count alone.  Rows are slot-addressed, not compacted: every record has a
 * fixed row for the gym's lifetime, row = its group's base + its record index (mv_entity_obs_layout), and a record that does not exist this episode is a row of
 * eight +0.0f.  Columns (megaverse_amd/csrc/mv_entity_obs.h states them for kernels and host alike, with the table of every scenario's rows):
 *    0  the entity's segmentation word class << 12 | instance as a float (exact: below 2^16), the value the instance plane shows for that drawable; 0: an empty
 *    row      1..3  centre, world units      4..6  half extents, world units      7  state, by class
 * with mv_set_scene_obs's two conversions, "copied" and "int".  Groups, in the label rule's order:
 *    0  "terrain": TowerBuilding's building zone (1 row; state: bz_reward), Obstacles*' terrain boxes (16; EXIT / LAVA; state: type), Rearrange's target
 *       items (8; state: shape), Sokoban's goal cells (80; compacted: row k is the k-th goal cell in cell order, the word carries the pad's instance; state 1)
 *    1  movable objects (80: TowerBuilding, Obstacles*, Collect, Rearrange, Sokoban): MOVABLE at its voxel cell, or CARRIED at its carrier's position;
 *       state: the object's state byte (1 + k: carried by agent k)
 *    2  collectables: Obstacles*' diamonds (16), Collect's (96; HAZARD: a red one), the Hex scenarios' (128; state: alive ? 1 + shape : 0 -- HexMemory's good /
 *       bad stays hidden), Football's ball (1; BALL; half extents: its radius; state: this tick's kicks); a diamond's state: 0 picked up, 2 red
 *    3  agents (A rows, every scenario): AGENT k at its position with the capsule's radius and half height; state: the index of the object it carries, -1 none
 * Floor, structure, furniture, BoxAGone's platforms and the HUD get no rows.
 * mv_entity_obs_layout: out[group] = {base row, rows, the class of the group's first kind (0: the group is empty)}.
 * Buffer, ticks, visibility, refresh, what forks / resampling / loads / seeds leave alone, ordering and refusals are mv_set_scene_obs's, with [entries][N][E][8]
 * for [entries][N][32]; the buffer must be 16-byte aligned.  The stepping call's ONE publication launch carries whichever of the three row records are
 * attached.  A gym that attaches none launches exactly what it launched before.  The staging rows (slots x N x E x 32 bytes) are counted in mv_arena_bytes
 * from the first attach on.
 * mv_debug_entity_obs_host: the record on the CPU, from the bytes of one EnvHeader (128), 16 TerrainBox (32 each), 8 ArrangementItem (32 each), 1024 Sokoban
 * cell bytes, 80 MovableObject (4 each), rewards_len MovableObject, 128 HexRec (32 each), one FootballState (64) and num_agents AgentState (128 each) of
 * megaverse_amd/csrc/mv_types.h -> out[E][8]; inputs the scenario does not read may be NULL: no device. */
enum { MV_ENTITY_OBS_FLOATS = 8, MV_ENTITY_OBS_GROUPS = 4 };
int mv_entity_obs_rows(const mv_gym *g);                                          /* E; -1: no gym */
int mv_entity_obs_layout(const mv_gym *g, int32_t out[MV_ENTITY_OBS_GROUPS][3]);  /* per group: base row, rows, seg class of its first kind */
int mv_set_entity_obs(mv_gym *g, float *device_buf);    /* [max(1, ring count)][N][E][8] float32 in device memory, 16-byte aligned; NULL detaches */
int mv_get_entity_obs(const mv_gym *g);                 /* 0: none, else the number of entries; -1: no gym */
int mv_get_entity_observation(mv_gym *g, int32_t env_idx, float *out_host);       /* last tick's E rows; waits for the gym's stream */
int mv_debug_entity_obs_host(int32_t scenario, int32_t num_agents, const void *env_header, const void *terrain16, const void *items8, const void *soko_cells,
                             const void *objects80, const void *rewards, int32_t rewards_len, const void *hex_objs128, const void *football_state,
                             const void *agent_states, float *out);               /* the pack function on the host; unused inputs may be NULL */
/* Depth observations (no reference counterpart: the reference reads colours back and leaves its depth buffer on the card).  One value per pixel of every frame
 * an observation pass draws: the ray parameter t of the pixel's nearest hit, the very float the shading works from.  Every ray has the camera-space direction
 * (x, y, -1) and every primitive frame keeps t, so t is the PLANAR camera-space depth -z_cam in world units, within [0.01, 120]; 0 where the ray hits nothing
 * (the black background).  A frame's record is ONE plane [H][W] in the frame's own pixel order -- row 0 is the bottom row -- whatever mv_set_obs_layout says.
 * Formats: MV_DEPTH_F32, the bits of t; MV_DEPTH_F16, t rounded to nearest-even.  megaverse_amd/csrc/mv_depth_obs.h states the rule for kernels and host alike.
 * The buffer is one more ring beside mv_set_output_ring's three: [entries][N*A][H][W] of float or __half, 4-byte aligned, entries = the output ring's count at
 * the moment of the call, or 1 without a ring; a frame's plane goes to the entry the frame goes to.  While a buffer is attached mv_set_output_ring is refused.
 * Which passes: every one that draws frames -- mv_step, every tick of mv_step_n, the last tick of MV_RENDER_LAST and of mv_macro_step(..., MV_RENDER_LAST), the
 * frame behind mv_reset and mv_reset_envs*(..., render = 1), mv_render.  Where no frame is drawn no byte of the buffer is written: mv_step_no_render,
 * MV_RENDER_NONE, the undrawn ticks of MV_RENDER_LAST; an env a draw mask leaves out keeps its planes as it keeps its rows.  Forks, resampling, loads and seeds
 * touch no plane; mv_draw_hires ignores the option.
 * How: in exact pixel mode the pass itself stores both outputs, one trace and no further launch.  In fast pixel mode (the default) the fast kernels stay what
 * they are and ONE launch per drawn tick follows the call's passes on the gym's stream (counted in out[1] of mv_debug_launch_counts): the exact trace without
 * the shading, frames in identity order.  Both forms give the same bits.  With a buffer attached a call's passes are not overlapped with the next call's
 * (mv_set_pass_overlap stays accepted).  Colours, rewards, dones, rows and the log are those of a gym without a buffer, and a gym that never attaches one
 * launches exactly what it launched before.
 * Ordering: mv_set_state_obs's.  The call is an ordering point and never waits on the host; the buffer is the caller's, written in place, and must stay valid
 * until the caller's stream has passed the end of the last call that writes it.  Attaching again replaces it; NULL detaches.  mv_close forgets the pointer.
 * Refused (-1 with text): no gym, a closed gym, a gym in an mv_group, an unknown format, a gym with still frames switched on (and mv_set_still_frames while a
 * buffer is attached: nothing carries a still frame's plane between ring entries); mv_set_output_ring and mv_set_render_resolution while attached;
 * mv_group_create and mv_step_many refuse a gym that has one attached (the union launches write none).
 * mv_get_depth_observation: one agent's plane in the LAST TICK's entry, widened to float32, after waiting for the gym's stream -- where that tick drew no
 * frame (MV_RENDER_NONE, mv_step_no_render) the entry holds what it held: an older tick's plane in a ring, or the caller's bytes.
 * mv_debug_depth_pack_host: the pack rule on the CPU: n values t with hit[i] != 0 where the ray hit -> n float32 or n half words; no device. */
enum { MV_DEPTH_F32 = 0, MV_DEPTH_F16 = 1 };
int mv_set_depth_obs(mv_gym *g, void *device_buf, int32_t format);   /* [max(1, ring count)][N*A][H][W] float / __half in device memory; NULL detaches */
int mv_get_depth_obs(const mv_gym *g);                               /* 0: none, else the number of entries; -1: no gym */
int mv_get_depth_format(const mv_gym *g);                            /* MV_DEPTH_*; -1: none attached */
int mv_get_depth_observation(mv_gym *g, int32_t env_idx, int32_t agent_idx, float *out_host);   /* [H][W] float32; waits for the gym's stream */
int mv_debug_depth_pack_host(const float *t, const uint8_t *hit, int32_t n, int32_t format, void *out);   /* the pack function, on the host */
/* Segmentation observations (no reference counterpart).  One label per pixel of every frame an observation pass draws: which drawable the pixel's nearest hit
 * belongs to -- the hit whose t the depth plane holds.  A frame's record is ONE plane [H][W] in the frame's own pixel order -- row 0 is the bottom row --
 * whatever mv_set_obs_layout says.  Formats: MV_SEG_CLASS_U8, one byte, the class; MV_SEG_INSTANCE_U16, one 16-bit word class << 12 | instance, instance =
 * the index of the drawable's record within its class's record array (< 4096): the indices mv_debug_set_objects, the snapshot and the state / scene records
 * use.  The whole word is 0 where the ray hits nothing -- exactly where the depth is 0 -- and its class nibble is the U8 byte.
 * Classes (megaverse_amd/csrc/mv_seg_obs.h states the rule for kernels and host alike; mv_seg_class_name gives the names):
 *   0 NONE   1 FLOOR (layout box in the layout colour; box index)   2 STRUCTURE (every other layout box, every box of the Hex scenarios, BoxAGone, Football; box
 *   index)   3 EXIT (exit pad, Sokoban goal pad; terrain / cell index)   4 LAVA (terrain index)   5 BUILDING_ZONE (0)   6 FURNITURE (Rearrange's raised floor
 *   and pedestals, Sokoban's wall caps; static / cell index)   7 TARGET (Rearrange's target arrangement; item index)   8 MOVABLE (a movable object at rest;
 *   object index)   9 CARRIED (one in an agent's hands; object index)   10 COLLECTABLE (Obstacles' and Collect's +1 diamonds, every Hex collectable, all of its
 *   parts; record index -- HexMemory's good / bad is hidden state and NOT in the label)   11 HAZARD (Collect's red -1 diamonds; reward index)   12 BALL
 *   (Football's; 0)   13 AGENT (another agent's capsule and eye box; agent k)   14 HUD (the time bar; agent k whose camera frame it sits in).
 * The buffer is one more ring beside mv_set_output_ring's three, [entries][N*A][H][W] of uint8_t or uint16_t (2-byte aligned), entries = the output ring's
 * count at the moment of the call, or 1; a frame's plane goes to the entry the frame goes to.  Everything else is mv_set_depth_obs's, line for line: which passes
 * write planes (every one that draws frames; no byte where no frame is drawn; a draw-masked env keeps its planes; mv_draw_hires ignores the option), the ordering
 * point, NULL detaches, mv_close forgets the pointer, the refusals (groups and mv_step_many, still frames in either order, mv_set_output_ring and
 * mv_set_render_resolution while attached, an unknown format, a misaligned buffer).  Depth and labels attach and detach independently, in either order.
 * How: in exact pixel mode the pass itself stores every attached output, one trace and no further launch.  In fast pixel mode ONE launch per drawn tick follows
 * the call's passes -- the depth follower, which now stores labels, or depth + labels: never two traces (counted in out[1] of mv_debug_launch_counts).  Both
 * forms give the same bytes.  The follower repeats the EXACT trace: at silhouette pixels a fast frame's colour and its label may come from different
 * primitives, within the fast mode's pixel rule.  Colours, rewards, dones, rows, depth planes and the log are those of a gym without labels.
 * The label kernels read the group boundaries (the env header's counts) and a layout box's floor / wall flag from the env's records when they RUN: a frame
 * whose env began a new episode in a later tick of the same batched call is labelled by the new episode's boundaries.
 * mv_get_seg_observation: one agent's plane in the LAST TICK's entry as uint16 [H][W], a U8 plane widened (the class, no shift), after waiting for the gym's
 * stream.  mv_debug_seg_bounds_host: the group boundaries {terrain, objects, rewards, agents, end} from an env header's counts.  mv_debug_seg_rule_host: the
 * rule on the CPU, one slot -> one uint8 / uint16 in *out; subtype: LayoutBox.slot, TerrainBox.type, the Sokoban cell byte or MovableObject.state of the record
 * the slot names.  mv_debug_seg_pack_host: n (class, instance) pairs -> n bytes / words. */
enum { MV_SEG_CLASS_U8 = 0, MV_SEG_INSTANCE_U16 = 1 };
int mv_set_seg_obs(mv_gym *g, void *device_buf, int32_t format);     /* [max(1, ring count)][N*A][H][W] uint8 / uint16 in device memory; NULL detaches */
int mv_get_seg_obs(const mv_gym *g);                                 /* 0: none, else the number of entries; -1: no gym */
int mv_get_seg_format(const mv_gym *g);                              /* MV_SEG_*; -1: none attached */
int mv_get_seg_observation(mv_gym *g, int32_t env_idx, int32_t agent_idx, uint16_t *out_host);   /* [H][W] uint16; waits for the gym's stream */
const char *mv_seg_class_name(int32_t cls);                          /* "FLOOR", ...; NULL outside [0, 15) */
int mv_debug_seg_bounds_host(int32_t scenario, int32_t L, int32_t W, int32_t num_boxes, int32_t num_terrain, int32_t num_objects, int32_t num_rewards,
                             int32_t num_agents, int32_t *out5);
int mv_debug_seg_rule_host(int32_t scenario, int32_t slot, const int32_t *boundaries5, int32_t subtype, int32_t format, void *out);
int mv_debug_seg_pack_host(const int32_t *cls, const int32_t *instance, int32_t n, int32_t format, void *out);
/* Normal observations (no reference counterpart).  One value of four components per pixel of every frame an observation pass draws: the unit outward normal of
 * the surface the pixel shows -- of the hit whose t the depth plane holds -- in the viewer's camera frame: x right, y up, z back, the columns of the camera
 * matrix.  It is the very vector the exact pass shades with, the same floats; only entry faces are hit, so it faces the viewer.  The 4th component is 1 where
 * there is a surface; a pixel whose ray hits nothing is four zeros, exactly where the depth is 0 and the label is 0.  A frame's record is ONE plane [H][W][4]
 * in the frame's own pixel order -- row 0 is the bottom row -- whatever mv_set_obs_layout says; depth and normal together unproject to oriented points.
 * Formats: MV_NORMAL_F16, four halves (x, y, z, 1), each rounded to nearest-even, 8 bytes; MV_NORMAL_SNORM8, four signed bytes (q(x), q(y), q(z), 127) with
 * q(v) = (int)(127 clamp(v, -1, 1) + (v >= 0 ? 0.5f : -0.5f)), 4 bytes, read back as b / 127.  megaverse_amd/csrc/mv_normal_obs.h states the rule for kernels
 * and host alike.
 * The buffer is one more ring beside mv_set_output_ring's three, [entries][N*A][H][W][4] of __half (8-byte aligned) or int8_t (4-byte aligned), entries = the
 * output ring's count at the moment of the call, or 1; a frame's plane goes to the entry the frame goes to.  Everything else is mv_set_depth_obs's, line for
 * line: which passes write planes (every one that draws frames; no byte where no frame is drawn; a draw-masked env keeps its planes; mv_draw_hires ignores the
 * option), the ordering point, NULL detaches, mv_close forgets the pointer, the refusals (groups and mv_step_many, still frames in either order,
 * mv_set_output_ring and mv_set_render_resolution while attached, an unknown format, a misaligned buffer).  Depth, labels and normals attach and detach
 * independently, in any order.
 * How: in exact pixel mode the pass itself stores every attached output, one trace and no further launch.  In fast pixel mode ONE launch per drawn tick follows
 * the call's passes and stores every attached plane, whichever of the seven subsets of {depth, labels, normals} is attached: never two traces (counted in
 * out[1] of mv_debug_launch_counts).  Both forms give the same bytes, and a plane's bytes do not depend on what is attached beside it.  Colours, rewards,
 * dones, rows, the other planes and the log are those of a gym without normals.
 * Unlike the labels, the normals read nothing outside the frame's own list and header: an env that begins a new episode in a later tick of the same batched
 * call changes no earlier frame's normals.
 * mv_get_normal_observation: one agent's plane in the LAST TICK's entry as float32 [H][W][4], halves widened exactly and bytes as b / 127.0f, after waiting
 * for the gym's stream.  mv_debug_normal_pack_host: the pack rule on the CPU: n vectors xyz[3 i ..] with hit[i] != 0 where the ray hit -> n values of 8 or 4
 * bytes; no device. */
enum { MV_NORMAL_F16 = 0, MV_NORMAL_SNORM8 = 1 };
int mv_set_normal_obs(mv_gym *g, void *device_buf, int32_t format);  /* [max(1, ring count)][N*A][H][W][4] __half / int8 in device memory; NULL detaches */
int mv_get_normal_obs(const mv_gym *g);                              /* 0: none, else the number of entries; -1: no gym */
int mv_get_normal_format(const mv_gym *g);                           /* MV_NORMAL_*; -1: none attached */
int mv_get_normal_observation(mv_gym *g, int32_t env_idx, int32_t agent_idx, float *out_host);   /* [H][W][4] float32; waits for the gym's stream */
int mv_debug_normal_pack_host(const float *xyz, const uint8_t *hit, int32_t n, int32_t format, void *out);   /* the pack function, on the host */
/* Episode budgets (no reference counterpart: VectorEnv::step resets a finished env on the spot and steps on, vector_env.cpp:89-108).  Per env e the gym owns an
 * int32 left[e]:  < 0: unlimited -- what every env is without these calls;  > 0: the env may still finish that many episodes;  0: the env is HALTED.
 * Tick t, env e, left[e] as it stands before the tick (megaverse_amd/csrc/mv_episode_budget.h states the rule for kernels and host alike):
 *   the env steps  <=>  (no step mask attached or mask[e] != 0) and left[e] != 0.
 *   An env that steps runs today's tick, byte for byte: rewards, done = 1, the true objective, the auto-reset swap-in, episodes_consumed; the observation is
 *   the first frame of the next episode, as always.  If that tick staged done and left[e] > 0, left[e] goes down by one.
 *   An env that does not step runs the frozen tick of the step masks, word for word (above): rewards +0.0f, done 0, its action entries cleared, no other byte
 *   of the env, its status word, its resident episodes or TowerBuilding's generator read or written; frames, where the mode draws, from the unchanged state.
 * So an env with budget b finishes exactly b episodes and then waits, frozen, on the first frame of its next episode -- also in the middle of a resident
 * multi-tick launch: a mask changes at an ordering point, a budget inside the kernel.  A halted env takes nothing from the refill protocol and cannot starve.
 * Every stepping entry and policy honours it: mv_step, mv_step_no_render, mv_step_n, mv_step_n_render in all three render modes.
 * The values are COPIED into a gym-owned device array (allocated at first use with the halted count and the episode log's mirror, counted in mv_arena_bytes,
 * freed by mv_close): the kernels write that array, the caller's buffer is read once, in the order of the gym's stream.  NULL detaches: every env is
 * unlimited again and the gym launches what it launched before.  Attaching again replaces every value (the "resume" operation).  A value of 0 halts the env
 * from the next tick.
 * Episode log (when on): a halted tick adds nothing to returns or length and writes no record; the finishing tick's record is written as always; after a
 * re-attach the next episode's length counts from its own first stepped tick.  Switching the log on with a budget attached is fine.
 * Nothing else touches a budget: mv_reset resets every env and leaves budgets attached and unchanged; mv_reset_envs, mv_fork_envs*, mv_resample_envs* and
 * mv_load_envs* treat halted envs like any other and do not change left -- an episode cut by a reset or overwritten by a fork or load reported no done and is
 * not counted; a halted fork destination stays frozen on its new state.
 * Ordering: mv_set_step_mask's.  The call is an ordering point behind every step launch enqueued so far and behind the episode log's last update, and in
 * front of the next step launch; neither form waits on the host; the host form goes through pinned staging buffers of the gym's.
 * Valid before the first mv_reset.  Refused (-1 with text): no gym, a closed gym, a gym in an mv_group; mv_group_create and mv_step_many refuse a gym with a
 * budget attached (the union launches read none). */
int mv_set_episode_budget(mv_gym *g, const int32_t *device_budget);   /* [N] int32 in device memory; NULL detaches */
int mv_set_episode_budget_host(mv_gym *g, const int32_t *budget);     /* [N] int32 in host memory; NULL detaches */
int mv_get_episode_budget(const mv_gym *g);                           /* 0: none, 1: attached; -1: no gym */
/* the gym-owned int32 [N] of remaining budgets, valid on the gym's stream after any stepping call; NULL when no budget is attached */
void *mv_episode_budget_device_ptr(mv_gym *g);
/* a uint32: the number of envs with left == 0 -- set by the attach, kept by the step kernels: one 4-byte read decides "everybody is done"; NULL likewise */
void *mv_halted_count_device_ptr(mv_gym *g);
int mv_halted_count(mv_gym *g, int32_t *out);                         /* the same value on the host; waits for the gym's stream, like mv_episode_log_count */
/* Env stores (no reference counterpart): an env's episode state saved into a RECORD of a caller-owned store, and a record loaded back into any env -- of
 * this gym, or of another gym of the same configuration.  A savepoint no longer costs a live env: a search keeps as many states as the store has slots, and
 * a state can leave its gym -- to another gym, another GPU's shard, host memory or a file (the store is plain memory: copy it).
 * A STORE is caller-owned device memory: `slots` records of mv_env_record_bytes(g) bytes each, 16-byte aligned; a torch.uint8 tensor [slots, record_bytes]
 * is one.  The gym never allocates, frees or remembers it, and mv_arena_bytes counts nothing for it.
 * A RECORD (megaverse_amd/csrc/mv_env_store.h states the layout once): a 64-byte record header {magic, format version, layout word, record bytes, flags};
 * the whole EnvHeader (the identity's dwords are stored too; a load ignores them); every per-env array of the fork's episode state, in the table's order,
 * each from a 16-byte boundary with its whole stride; the episode log's accumulators, double ret[A] and int32 len -- always present; a header flag says
 * whether the log was on at save time, and they are written as zero when it was off.
 * The LAYOUT WORD is a hash of the format version, the scenario (id and name: the six Obstacles variants differ), the agents per env, the observation width
 * and height, every float parameter's key and value, and every state array's bytes per env.  Two gyms with the same word can exchange records.  It does not
 * depend on num_envs, the seed, the pixel mode, the observation layout, the env sharding or the episode log.
 * slot_of: int32 [N].
 * mv_save_envs: slot_of[e] = m, 0 <= m < slots, writes env e's current episode state into record m; -1: env e is not saved.  Nothing in the gym changes, not
 * one byte.  Invalid: an index out of range, and two envs that name one slot -- both entries are invalid, neither is written.  A record is written whole or
 * not at all.
 * mv_load_envs: slot_of[d] = m makes env d leave its running episode and continue record m's; -1 leaves env d alone; any number of envs may load one record.
 * What is written is what mv_fork_envs writes into a destination -- the header without the identity's dwords, every state array, and, where the gym's log
 * is on, the accumulators: the record's if it was saved with the log on, else zero, so that the episode counts from the load, as when the log is switched
 * on mid-episode.  What stays is the fork's identity list, word for word (above).  Not touched: the public rewards, dones and true objectives, the output
 * rings, the observation slab, pending actions, the step mask -- a frozen env can be loaded into, like a fork destination.  Invalid: an index out of range,
 * and a RECORD THAT DOES NOT START WITH the magic, this format version, this gym's layout word and this record size -- a slot never written, a record of
 * another configuration.  Such an entry changes no byte of its env.  Only the kernel can make that check, so both load forms rely on it.  The header is a
 * guard against accidents, not an authenticator: the bytes behind a header that matches are trusted.
 * Invalid entries: the host forms validate the map on the host (-1 with text, nothing copied; a map of -1s launches nothing).  A kernel skips an invalid
 * entry and raises a status bit; the NEXT stepping call reports it once as return 1 with a warning that names mv_save_envs / mv_load_envs.  That call waits
 * for the status words behind the launch: the one host wait the device forms cost -- and mv_load_envs_host too, since record headers are visible on the
 * device only.  mv_save_envs_host validates everything on the host and costs none.
 * Ordering: mv_fork_envs' rules.  Every form runs on the gym's (the caller's) stream -- the store is the caller's memory -- behind every step launch
 * enqueued so far and behind the episode log's last update; the next step launch runs behind it (it overwrites what a save reads and reads what a load
 * writes).  Nothing else is ordered behind a save: the caller's stream sees the record complete.  No form waits on the host.  Map and store stay unchanged
 * until the launch has run -- in stream order: until the next stepping call has been enqueued.  Host maps travel through the forks' pinned double buffer.
 * Refused (-1 with text): no gym, a closed gym, before the first mv_reset, a null map or store, slots <= 0, a store that is not 16-byte aligned, a gym in an
 * mv_group.  Out of scope: groups, records across format versions, compression. */
int64_t mv_env_record_bytes(const mv_gym *g);    /* a multiple of 16; -1: no gym */
uint64_t mv_env_record_layout(const mv_gym *g);  /* two gyms with the same word can exchange records; 0: no gym */
int mv_save_envs(mv_gym *g, const int32_t *device_slot_of, void *device_store, int32_t slots);
int mv_save_envs_host(mv_gym *g, const int32_t *slot_of, void *device_store, int32_t slots);
int mv_load_envs(mv_gym *g, const int32_t *device_slot_of, const void *device_store, int32_t slots);
int mv_load_envs_host(mv_gym *g, const int32_t *slot_of, const void *device_store, int32_t slots);
/* step several gyms of one job with one call (no reference counterpart: its multi-task runs are separate processes,
 * the scripts under megaverse_rl/runs): for each gym, optionally mv_sample_random_actions(seed, step_index), then mv_step / mv_step_no_render */
int mv_step_many(mv_gym *const *gyms, int32_t n, int32_t render, int32_t sample, uint32_t seed, uint32_t step_index);

/* Groups: up to 8 gyms of one job -- one per scenario of a multi-task batch, the reference's layout (megaverse/megaverse_env.py:27-39: one
 * MegaverseGym per task) -- stepped TOGETHER: one step launch and one observation launch per tick for all of them -- per CALL of 2..8 ticks
 * when every member has output rings (mv_set_output_ring) at least that deep and the group holds at most 1024 envs (all resident at once; a longer call is split into chunks of 8) -- on one shared pair of streams (BASELINE.json configs[4]: scenarios dealt round-robin over the envs of one batch; every gym keeps its env_offset /
 * env_stride, so seeds and sampled actions are the job-wide ones).  The members must share device, observation size, agents per env and
 * stream.  While grouped a gym is stepped through the group only; everything else (reset, seed, getters, shaping) stays per gym.
 * mv_group_step: k ticks like mv_step_n (render = 0: no observation pass).  Closing a member dissolves the group. */
typedef struct mv_group mv_group;
int mv_group_create(mv_gym *const *gyms, int32_t n, mv_group **out);
int mv_group_step(mv_group *grp, int32_t k, int32_t render, int32_t policy, uint32_t seed, uint32_t first_step_index);
int mv_group_destroy(mv_group *grp);

int mv_step(mv_gym *g);                             /* step(), :118-121: VectorEnv::step incl. auto-reset + render */
int mv_step_no_render(mv_gym *g);                   /* physics/logic/auto-reset only */
/* k open-loop ticks with one call = k iterations of the reference's benchmark loop body "for every agent setAction(random); venv.step()"
 * (megaverse_test_app.cpp:140-147 + vector_env.cpp:89-108): tick j draws its actions from (policy, seed, first_step_index + j) inside the
 * step kernel and renders every agent's observation.  Exactly the ticks k calls of mv_sample_random_actions + mv_step make -- but the
 * simulation stream and the caller's stream hand over to each other once per call instead of once per tick.  policy
 * MV_POLICY_NONE: the first tick acts on what mv_set_actions* left, the others on cleared actions.  The public arrays hold the LAST tick's
 * outputs -- or, with mv_set_output_ring, every tick's.  k may exceed the internal batch (mv_recommended_ticks_per_call; MV_PIPE_BATCH overrides its sizing): the call splits it. */
int mv_step_n(mv_gym *g, int32_t k, int32_t policy, uint32_t seed, uint32_t first_step_index);
/* Render modes of a batched call (no reference counterpart: VectorEnv::step always renders, vector_env.cpp:103-107).  A planner that scores candidates by
 * return reads none of the k frames mv_step_n draws, one that feeds a value net only the last; the observation pass is the larger half of a call.
 * MV_RENDER_EVERY: mv_step_n, call for call and launch for launch.
 * MV_RENDER_NONE: the k ticks run -- physics, scenario logic, auto-reset, episode swap-in, refill protocol, status read-backs, episode log -- and nothing is
 * drawn.  Rewards and dones of every tick go where mv_step_n puts them: entry t % count of attached rings, else the public arrays (the last tick's stay); the
 * true objectives of envs that finished are published in tick order.  The observation slab and every entry of an observation ring are not written, not one
 * byte; the ring's tick count advances by k as always, so a later rendered call lands in the entries it would have.  mv_render afterwards draws the current state.
 * MV_RENDER_LAST: as MV_RENDER_NONE, and tick k - 1 of the whole call (also where the call is split into chunks) is drawn into its own place -- ring entry
 * t % count, or the slab -- in the gym's pixel mode and layout, byte for byte what MV_RENDER_EVERY would have left there.
 * Launches: one step launch per 8 ticks that sets no frame up (MV_RENDER_LAST: the drawn tick's frame setup runs inside the last one), one launch that
 * publishes the rewards / dones / true objectives of all the call's ticks, MV_RENDER_LAST: one observation launch (it publishes nothing).  Shapes without a
 * multi-tick step kernel -- several agents outside TowerBuilding, MV_POLICY_NONE, MV_STEP_TICKS=0, gyms stepped tick by tick because their episodes can end
 * within a few ticks -- take one tick-only launch per tick, as mv_step_no_render does.  Every scenario and every policy works in every mode.
 * Ordering: mv_step_n's.  The caller's stream sees the call's rewards and dones behind the call; the simulation stream reuses the call's hand-over slots only
 * after the publication and the episode log's update have read them.  mv_set_pass_overlap does not apply to MV_RENDER_LAST / MV_RENDER_NONE calls: they run
 * as without it, and a following MV_RENDER_EVERY call starts a new overlapped sequence.
 * Groups: mv_group_step keeps its own render flag (0 / 1); render modes for groups are not provided.
 * Refused (-1 with text): an unknown mode; everything mv_step_n refuses; a gym in a group. */
enum { MV_RENDER_EVERY = 0, MV_RENDER_LAST = 1, MV_RENDER_NONE = 2 };
int mv_step_n_render(mv_gym *g, int32_t k, int32_t policy, uint32_t seed, uint32_t first_step_index, int32_t render_mode);
/* Macro steps (no reference counterpart: it is the action-repeat / frame-skip wrapper a learner writes around VectorEnv::step, vector_env.cpp:89-108 --
 * "for _ in range(k): obs, r, d = env.step(a); total += r; if d: break" -- per env, as one operation).  One decision is held for up to k ticks, every env
 * stops at its own first done, and the call leaves ONE reward (the sum), ONE done and ONE frame.
 * device_actions: [N*A][6] int32, encoded as for mv_set_actions_device, held on every tick of the call the env steps in -- to the kernels an action ring of
 * count 1; the caller's attached ring (mv_set_action_ring), if any, stays attached and untouched; a pending mv_set_actions* buffer is superseded as
 * MV_POLICY_SEQUENCE supersedes it.  The kernels read it in place: it stays unchanged until the caller's stream has passed the end of the call.
 * device_ticks: NULL (every env: k) or int32 [N], clamped to [0, k]; 0: the env does not step in this call.  Copied once, in stream order, into a gym-owned
 * array tl [N] (allocated at first use, counted in mv_arena_bytes, freed by mv_close): the kernels write that array.
 * The rule (megaverse_amd/csrc/mv_macro_step.h states it for kernels and host alike), tl[e] set at the call's start:
 *   env e steps in a tick  <=>  mask and budget let it (mv_set_step_mask, mv_set_episode_budget: their rule, unchanged) and tl[e] > 0;
 *   behind a tick the env stepped in, tl[e] goes down by one, and to 0 if that tick staged done; the budget is spent as always -- a user budget keeps
 *   counting episodes over macro steps;
 *   an env that does not step runs the frozen tick of the step masks, word for word.
 * So an env's macro step ends on the tick that finished its episode; that tick ran whole, auto-reset included, and the env stands on the first frame of its
 * next episode -- also in the middle of a resident multi-tick launch, across the launches of one chunk and across the chunks of a call whose k exceeds the
 * internal batch (the call splits as mv_step_n does).
 * Outputs, one set per CALL: reward[a] is the fp32 left fold s = r_0; s = s + r_j over the call's k per-tick values in tick order (a frozen tick's is +0.0f;
 * nothing reassociated or contracted: a float32 loop reproduces it bit for bit); done[e] is the OR over the call's ticks; true objectives are published for
 * the envs that finished, as MV_RENDER_NONE / MV_RENDER_LAST calls publish them.  MV_RENDER_LAST draws the frame of the call's last tick for every env, the
 * ones that stopped early included (their new episode's first frame), in the gym's pixel mode and layout; MV_RENDER_NONE writes no byte of the slab or an
 * observation ring.  With an output ring attached the call fills ONE entry and the ring's position advances by one -- a ring of 16 holds 16 consecutive
 * decisions; every stepping call advances the position by the entries it wrote, so interleaving with mv_step_n stays well defined.  mv_ticks_since_reset
 * advances by k.  State observations (mv_set_state_obs): each agent's row goes into that same entry and holds the state behind the call's last tick.
 * Episode log: a tick the env did not step in adds nothing to returns or length; records as always.
 * Launches: the MASKED step kernels, as one launch per 8 ticks wherever mv_step_n_render has its one-launch step; one launch that sets tl, one that folds
 * the call's hand-over slots into the entry (per chunk; a later chunk continues the fold from the entry, in order); MV_RENDER_LAST: one observation launch.
 * Ordering: mv_step_n_render's.  The device form never waits on the host; the host form goes through pinned staging buffers of the gym's.
 * Refused (-1 with text): everything mv_step_n_render refuses; a gym in an mv_group; k < 1; MV_RENDER_EVERY (a decision has one frame); null actions.
 * Out of scope: groups, discounting inside the fold, reward clipping. */
int mv_macro_step(mv_gym *g, int32_t k, const int32_t *device_actions, const int32_t *device_ticks, int32_t render_mode);
int mv_macro_step_host(mv_gym *g, int32_t k, const int32_t *actions, const int32_t *ticks, int32_t render_mode);
/* Rollout rings (no reference counterpart: its learner copies each step's observation out of the gym, megaverse_env.py:121-130): tick
 * number t since this call leaves its observations in obs[t % count] ([count][N*A][h][w][4]; planar layout: [count][N*A][3][h][w]), its rewards in rewards[t % count] ([count][N*A])
 * and its dones in dones[t % count] ([count][N]); a NULL ring keeps that output where it was.  count = 0 switches back to the single
 * slab / arrays.  Host getters (mv_get_observation, mv_get_last_rewards, ...) read the entry of the last tick. */
int mv_set_output_ring(mv_gym *g, int32_t count, void *obs, float *rewards, uint8_t *dones);
int mv_get_output_ring(const mv_gym *g);   /* the ring's count, 0: no ring (what mv_set_state_obs sizes its buffer by); -1: no gym */
/* Overlapped observation passes (opt-in).  With rings for all three outputs at least TWO calls deep (count >= 2 k, k = the ticks of one mv_step_n call,
 * also where k exceeds the internal batch; otherwise the call runs as without the option) the one-launch observation passes of consecutive
 * mv_step_n calls run on two internal streams in turn: the passes of call c + 1 begin while the last workgroups of call c's drain.  The caller's
 * stream still waits for every call's passes before anything enqueued after the call runs.  The price is the ring's contract: an entry must be
 * consumed -- the consumer enqueued on the caller's stream -- before the NEXT stepping call after the one that produced it is issued (without
 * overlap: before the call that overwrites it).  on = 0 also releases the two internal streams (a HIP process shares few hardware queues among its streams:
 * GPU_MAX_HW_QUEUES, 4 by default).  No reference counterpart (the reference renders synchronously, vector_env.cpp:112-118). */
int mv_set_pass_overlap(mv_gym *g, int32_t on);
/* What a caller who just wants throughput should ask mv_step_n for -- the measured rules that used to live in bench.py (no reference counterpart):
 * mv_recommended_ticks_per_call: 16 (one tail of the one-launch observation pass per 16 ticks) for 1024 .. 2047 agent frames per tick where the gym's slot groups hold
 * 16 (mv_create sizes them by footprint: 16 where the 48 hand-over slots that takes stay under 2.25 GiB, else 8; MV_PIPE_BATCH overrides) and the scenario is not Sokoban; 8 otherwise; 1 where episodes can end within a few ticks
 * (such gyms are stepped tick by tick whatever k says).  A gym in a group: at most 8 (the two-launch group call's limit, and only while the group's envs are
 * all resident at once: 1024).  mv_recommended_pass_overlap: 1 wherever the
 * observation passes are what a call waits for (the next call's begin in the tail of this one's) -- every scenario but Empty; TowerBuilding with one or two agents per
 * env from 512 frames per tick on (with fewer frames, or four agents per env, the step launch bounds the call and the second pass stream only costs) --, 0 for
 * gyms whose episodes last a few ticks (the library declines to overlap there) and in groups.
 * mv_arena_bytes: the device memory this gym holds (state + the hand-over slots of PIPE_GROUPS x ticks-per-call ticks + its own observation slab). */
int mv_recommended_ticks_per_call(const mv_gym *g);
int mv_recommended_pass_overlap(const mv_gym *g);
int64_t mv_arena_bytes(const mv_gym *g);
/* Who draws this gym's episodes (Env::reset, env.cpp:57-76, off the step path in every case): the number of host threads of its episode feeder, or 0 when the
 * episodes are drawn on the device -- TowerBuilding always (tower_draw_kernel); Collect where the process's share of the host is under three cores and the gym has 256 envs and more, or
 * MV_COLLECT_DEVICE_GEN=1 (collect_draw_kernel: the host generator's episodes, byte for byte).  -1: no such gym. */
int mv_host_generator_threads(const mv_gym *g);
/* Are this gym's episodes drawn on the device?  1: TowerBuilding, and every gym whose feeder runs in device mode -- Collect as above; the Obstacles family
 * (ObstaclesEasy / Medium / Hard / Walls / Steps / Lava) and Empty with MV_OBSTACLES_DEVICE_GEN=1 in the environment at mv_create (obstacles_draw_kernel,
 * megaverse_amd/csrc/mv_obstacles_draw.h: the host generator's episodes, byte for byte; unset or 0: host-fed, no automatic choice).  0: host-fed.  -1: no gym.
 * mv_host_generator_threads is 0 exactly where this is 1.  The device form of mv_seed_envs stays refused on a device-fed gym as on a host-fed one.
 * Under the switch mv_create refuses an Obstacles gym whose obstacles* float parameters exceed the device generator's fixed arrays (7 platforms, heights 1..4). */
int mv_device_generator(const mv_gym *g);
int mv_render(mv_gym *g);                           /* observation pass only */

int mv_is_done(mv_gym *g, int32_t env_idx);         /* isDone(), :123-126 -> 0/1, <0 on error */
int mv_get_dones(mv_gym *g, uint8_t *out);          /* [N] */
int mv_get_last_rewards(mv_gym *g, float *out);     /* getLastRewards(), :128-137 -> [N*A] env-major */
int mv_true_objective(mv_gym *g, int32_t env_idx, int32_t agent_idx, float *out); /* :203-206 */
int mv_get_true_objectives(mv_gym *g, float *out);  /* [N*A] */

/* getObservation(), :139-143: (h, w, 4) uint8, rows bottom-up like glReadPixels.  The reference
 * returns a view of host memory; here the frame lives in HBM: copy one frame out ... */
int mv_get_observation(mv_gym *g, int32_t env_idx, int32_t agent_idx, uint8_t *out_host);
/* ... or take the device slab [N*A][h][w][4] -- [N*A][3][h][w] in the planar layout, mv_set_obs_layout (valid until mv_close; rewritten by every step) */
void *mv_obs_device_ptr(mv_gym *g);
void *mv_rewards_device_ptr(mv_gym *g);             /* float [N*A] */
void *mv_dones_device_ptr(mv_gym *g);               /* uint8 [N] */
void *mv_true_objectives_device_ptr(mv_gym *g);     /* float [N*A] */
/* let the caller own the observation slab (e.g. a torch tensor / an RCCL gather buffer) */
int mv_set_obs_buffer(mv_gym *g, void *device_ptr);
int mv_set_stream(mv_gym *g, void *hip_stream);

/* Pixel arithmetic of the observation pass (MagnumEnvRenderer::draw, magnum_env_renderer.cpp:288-330, is a GPU
 * rasteriser: its pixels are defined up to fp32 rounding).  MV_PIXELS_FAST (default): hardware reciprocal / rsqrt,
 * within the tolerance DESIGN.md "pixel tolerance" states (<= 1 of 255 per channel except for a <= 1e-4 fraction of
 * silhouette / depth-tie pixels).  MV_PIXELS_EXACT: every fp32 operation correctly rounded, RGBA8 bit-identical to
 * the CPU oracle (parity tests).  Env var MV_PIXEL_MODE=exact|fast sets the default of new gyms. */
enum { MV_PIXELS_EXACT = 0, MV_PIXELS_FAST = 1 };
int mv_set_pixel_mode(mv_gym *g, int32_t mode);
int mv_get_pixel_mode(const mv_gym *g);

/* Layout of the observation slab (no reference counterpart: its learner drops alpha and transposes every frame, megaverse_env.py:121-130).
 * MV_OBS_RGBA (default): [N*A][h][w][4] RGBA8, alpha 255.  MV_OBS_RGB_PLANAR: [N*A][3][h][w] uint8, planes R, G, B -- what a learner's conv net
 * consumes, written by the observation pass itself (3 bytes per pixel instead of 4); rows bottom-up in both.  The layout sets the frame's size
 * everywhere one appears: the owned slab, what mv_set_obs_buffer expects, the entry stride of mv_set_output_ring's observation ring (planar buffers:
 * 16-byte aligned where w % 16 == 0, 4-byte where w % 4 == 0).  mv_get_observation returns (h, w, 4) RGBA with alpha 255 in both layouts; the hires frames (mv_draw_hires) stay RGBA.
 * Valid before the gym's first mv_reset, mv_render, mv_set_obs_buffer or mv_set_output_ring, and not on a gym in a group; mv_group_create
 * refuses gyms whose layouts differ.  mv_get_obs_layout: the layout, -1 for no gym. */
enum { MV_OBS_RGBA = 0, MV_OBS_RGB_PLANAR = 1 };
int mv_set_obs_layout(mv_gym *g, int32_t layout);
int mv_get_obs_layout(const mv_gym *g);

/* One-step-ahead pipelining (no reference counterpart).  On (default): the step kernels run on an internal stream,
 * and the step of tick t + 1 may overlap the observation pass of tick t whenever nothing the caller enqueued on its stream feeds
 * it (device-sampled or host-provided actions).  Nothing observable changes: rewards / dones / true objectives are published into
 * the arrays above ON THE CALLER'S STREAM, ordered with the observations, and a step never overwrites what a consumer enqueued
 * before the previous mv_step may still be reading.  mv_set_actions_device makes the next step wait (a policy in the loop is a true
 * dependency).  Off: everything runs on the caller's stream in order -- cheaper when several gyms already overlap each other
 * (MultiTaskGym).  Env var MV_PIPELINE=0|1 sets the default of new gyms. */
int mv_set_pipelining(mv_gym *g, int32_t on);
int mv_get_pipelining(const mv_gym *g);

/* setRenderResolution/drawHires/getHiresObservation (:145-178,203-207); drawOverview with no overview attached is a no-op
 * exactly like a reference build without WITH_GUI (:180-201) */
int mv_set_render_resolution(mv_gym *g, int32_t w, int32_t h);
int mv_draw_hires(mv_gym *g);
int mv_get_hires_observation(mv_gym *g, int32_t env_idx, int32_t agent_idx, uint8_t *out_host);
int mv_draw_overview(mv_gym *g);

/* Overview cameras (opt-in; the reference's Overview camera, rendering/src/render_utils.cpp:34-55, without its window).  One camera per env,
 * free in the world or attached to an agent, drawn by mv_draw_overview into a buffer of its own with the exact pass's arithmetic -- whatever the pixel mode,
 * the observation layout, the draw mask or the still-frame option say, as mv_draw_hires.  Projection, clip range [0.01, 120] and light are the agents'
 * (horizontal 100 degrees at aspect 128/72 whatever w and h; the reference's overview range (0.1, 600) is not adopted: DESIGN.md 7).  Nothing a stepping call
 * launches, reads or writes changes: the overview owns its lists, rectangles, headers, counts, cost bins and cameras (csrc/mv_overview.h has the rule and the
 * arrays, counted in mv_arena_bytes from the first attach on and freed by mv_close).
 * mv_camera: agent = -1, FREE: eye is the world position, c the row-major 3x3 whose columns are the camera's right / up / back axes in the world, taken as
 * given.  agent = k, AGENT: the camera is agent k's own, built from its state on the device at draw time exactly as its observation's; eye is then an offset
 * in that camera's axes (right, up, back) -- all zero: no arithmetic at all, the agent's very eye -- and c is ignored.  MV_CAMERA_FIRST_PERSON (AGENT only):
 * the agent's capsule and eyes box are not drawn (its time bar and what it carries are): the rule of its own observation.  Without it, and in FREE mode,
 * every part of every agent is drawn.
 * mv_set_overview: attach (device_rgba: the caller's [N][h][w] RGBA8, row 0 the bottom row; NULL: gym-owned), 1 <= w, h <= 1024; w = h = 0: detach.  Before
 * any camera is set every env has the reference's pose (mv_overview_default_camera).  mv_set_overview_cameras: [N] device records, copied on the gym's stream
 * (NULL: back to the default pose); an agent index outside [-1, A) is taken as FREE with the record's pose and counted.  mv_set_overview_cameras_host: the
 * same from host memory (free again on return), refusing such records.  mv_draw_overview: attached, the frame setup and the pass of all N envs from the
 * state as it stands, behind every step launch enqueued so far, on the gym's stream, no host wait; not attached: nothing, returns 0.
 * mv_overview_dropped: low 32 bits: primitives that did not fit an env's list (capacity 256 / 1024 / 2048 by the scenario's slot count: mv_overview_capacity)
 * since the attach; high 32 bits: clamped agent indices; one host wait.  Refused for a gym of an mv_group. */
enum { MV_CAMERA_FIRST_PERSON = 1 };
typedef struct mv_camera {
    float   eye[3];   /* FREE: world position.  AGENT: offset from the agent's eye in the agent camera's axes (right, up, back) */
    int32_t agent;    /* -1: FREE;  0 .. A-1: AGENT -- the camera is that agent's own, built from its state on the device at draw time */
    float   c[9];     /* FREE: row-major 3x3, columns = right / up / back in world axes (taken as given, not normalised).  AGENT: ignored */
    int32_t flags;    /* bit 0 MV_CAMERA_FIRST_PERSON (AGENT only) */
    int32_t pad[2];   /* 0 */
} mv_camera;
int mv_set_overview(mv_gym *g, int32_t w, int32_t h, void *device_rgba);
int mv_set_overview_cameras(mv_gym *g, const mv_camera *device_cams);
int mv_set_overview_cameras_host(mv_gym *g, const mv_camera *cams);
int mv_get_overview_observation(mv_gym *g, int32_t env_idx, uint8_t *out_host);
void *mv_overview_device_ptr(mv_gym *g);
int mv_overview_dropped(mv_gym *g, int64_t *out);
int mv_overview_capacity(const mv_gym *g);                                   /* list capacity per env of this gym's scenario: 256, 1024 or 2048 */
int mv_overview_default_camera(mv_camera *out);                              /* the derived reference pose, host only */
/* the camera the device would build from cam (and, AGENT mode, from the 128-byte state record of its agent), on the host: eye[3] then c[9] */
int mv_debug_overview_camera_host(const mv_camera *cam, const void *agent_state, float *out_eye3_c9);

/* getRewardShaping/setRewardShaping (:208-217); one key at a time across the C boundary */
int mv_num_reward_shaping_keys(const mv_gym *g);
const char *mv_reward_shaping_key(const mv_gym *g, int32_t i);
int mv_get_reward_shaping(mv_gym *g, int32_t env_idx, int32_t agent_idx, const char *key, float *out);
int mv_set_reward_shaping(mv_gym *g, int32_t env_idx, int32_t agent_idx, const char *key, float value);

int mv_synchronize(mv_gym *g);

/* Episode log (opt-in; no reference counterpart in the simulator: the reference's learner wrapper sums every agent's rewards on the host, tick by tick, and
 * reports them when the env is done -- megaverse_rl/megaverse_utils.py:61-86).  With the log on a gym keeps, on the device, a running return per agent
 * (double ret[N*A]) and a running length per env (int32 len[N]), both zero after mv_set_episode_log and after every mv_reset.  Every stepped tick (mv_step,
 * mv_step_no_render, each tick of mv_step_n / mv_step_many / mv_group_step), in tick order: ret[i] += (double)reward[i], len[e] += 1; then every env that
 * is done appends one record per agent, in agent order, and its ret and len go back to zero.  Records therefore stand in ascending (end_tick, agent) order,
 * and the log of a run is reproducible byte for byte.  end_tick counts the ticks stepped since the last mv_reset (the first tick after it is 0);
 * true_objective is what the finishing tick recorded.  Episodes cut by mv_reset are not logged; an episode that was running when the log was switched on is
 * counted from that tick.  The log is a linear device buffer of `capacity` records: a record that does not fit is dropped and counted (the accumulators
 * are reset all the same), and -- like every fixed capacity here -- reported once, by a later stepping call that returns 1; draining makes room and
 * re-arms the report.
 * mv_set_episode_log: capacity > 0 allocates and switches on (again: from zero accumulators and an empty buffer), 0 switches off and frees; valid between
 * calls at any time, also on a gym in a group (every member keeps its own log).  Rewards, dones, true objectives and observations are what they are
 * without the log.
 * Currency: every stepping call leaves the log up to date at its end, ordered on the caller's stream with the call's other outputs (one small launch per
 * call and gym; a call of more ticks than the internal batch: one per chunk).  Nothing is deferred -- the deferral bound is 0 ticks -- so
 * mv_flush_episode_log has nothing to enqueue today; callers that read the device pointers should still call it, it is where a deferred update would go.
 * mv_episode_log_count / mv_drain_episode_log flush, synchronise the caller's stream and read; drain copies the oldest max_records records out, removes
 * them (the rest moves to the front) and returns how many it copied.  dropped: records lost since the log was switched on.
 * Device pointers (valid until mv_set_episode_log / mv_close): the records, the header {uint32 count, uint32 dropped, 2 x uint32 internal}, ret, len.
 * mv_arena_bytes includes the log. */
typedef struct mv_episode_record {
    int32_t agent;          /* env * A + agent, local to the gym */
    int32_t length;         /* ticks, the finishing tick included */
    uint32_t end_tick;      /* ticks stepped since the last mv_reset, before the finishing tick */
    float true_objective;
    double ret;             /* float64 sum of the episode's float32 rewards */
} mv_episode_record;       /* 24 bytes */
int mv_set_episode_log(mv_gym *g, int32_t capacity);
int mv_get_episode_log_capacity(const mv_gym *g);   /* 0: off; -1: no gym */
int mv_flush_episode_log(mv_gym *g);
int mv_episode_log_count(mv_gym *g, uint32_t *count, uint32_t *dropped);
int mv_drain_episode_log(mv_gym *g, mv_episode_record *out_host, int32_t max_records, uint32_t *dropped);
void *mv_episode_log_records_device_ptr(mv_gym *g);   /* mv_episode_record [capacity] */
void *mv_episode_log_count_device_ptr(mv_gym *g);     /* uint32 [4]: count, dropped, internal */
void *mv_episode_returns_device_ptr(mv_gym *g);       /* double [N*A] */
void *mv_episode_lengths_device_ptr(mv_gym *g);       /* int32 [N] */
int64_t mv_ticks_since_reset(const mv_gym *g);        /* what the next tick's end_tick would be; -1: no gym */

/* In-stream kernel timing with HIP events on the gym's own stream (bench.py roofline leg, in a loop of its own: never inside
 * the timed region).  After mv_profile_begin the next max_steps calls of mv_step record events around the launches;
 * mv_profile_end synchronises and returns the mean milliseconds and sample count per interval: [0] step kernel (physics + logic +
 * auto-reset of finished envs + frame setup of the env's frames), [1] always 0 (retired), [2] output publish + frame sort (exact
 * pixel mode; ~0 in the fast mode), [3] raster.  Every interval is taken between two events of ONE stream.  The counterpart in the reference is the TinyProfiler timers around venv.step()
 * (src/apps/megaverse_test_app.cpp:68-74). */
int mv_profile_begin(mv_gym *g, int32_t max_steps);
int mv_profile_end(mv_gym *g, float *avg_ms4, int32_t *counts4);

/* test hooks: packed state snapshot of one env (layout in DESIGN.md, same bytes as the oracle's
 * mvo_snapshot) and the raw device RNG streams */
int mv_debug_set_agent_pos(mv_gym *g, int32_t env_idx, int32_t agent_idx, float x, float y, float z); /* teleport (fall-detection tests) */
/* out[0] / out[1]: the step launches / observation launches (one per launcher call: a batched pass is one, an exact-mode pass with its frame sort is one; the
 * still frames' carry and the one publication launch of state / scene observations count here too) that stepping calls have enqueued for this gym so far; for a member of a group: the group's.  Tells the batched paths from the tick-by-tick ones, whose bytes are the same. */
int mv_debug_launch_counts(mv_gym *g, int64_t out[2]);
/* scripted single-step physics cases (tests/test_canonical_poses*.py): the yaw basis from (cos, sin) as DefaultKinematicAgent's spawn builds it
 * (agent.cpp:42-46), and the controller's velocities */
int mv_debug_set_agent_yaw(mv_gym *g, int32_t env_idx, int32_t agent_idx, float c, float s);
int mv_debug_set_agent_velocity(mv_gym *g, int32_t env_idx, int32_t agent_idx, float hvx, float hvz, float vvel);
/* scripted TowerBuilding cases (tests/tower_cases.py).  The pitch of an agent's record: interact points depend on it.  The movable boxes of one env of a
 * TowerBuilding gym (others are refused): objs[i] = {x, y, z, state}, state 0 placed, 1 + k carried by agent k; 0 <= n <= 80.  Writes the records (zero
 * beyond n) and num_objects, clears every object bit of the env's chunk and sets it for each placed object inside the chunk, sets each agent's `carrying`
 * from the states (-1 where none) and recomputes bz_reward with the step kernel's own sum; episode_len, highest_tower, picked_up, visited_zone and the
 * generator's ring are left alone.  Refused with a text: two objects carried by one agent, a carrier the env does not have, two placed objects in one
 * voxel, a placed object in a solid voxel. */
int mv_debug_set_agent_pitch(mv_gym *g, int32_t env_idx, int32_t agent_idx, float pitch);
int mv_debug_set_objects(mv_gym *g, int32_t env_idx, const int8_t (*objs)[4], int32_t n);
int mv_debug_snapshot_size(const mv_gym *g);
int mv_debug_snapshot(mv_gym *g, int32_t env_idx, void *out_host);
/* BoxAGone: env env_idx's platform table, temporary ring, timers and cell map (BoxAGoneState, mv_types.h); out_host == NULL: its size */
int mv_debug_boxagone_state(mv_gym *g, int32_t env_idx, void *out_host);
/* Football: env env_idx's ball (FootballState, mv_types.h); out_host == NULL: its size.  The setter places the ball (position, drawn radius, velocity,
   angular velocity, pending force) for known-answer tests. */
int mv_debug_football_state(mv_gym *g, int32_t env_idx, void *out_host);
int mv_debug_set_football_state(mv_gym *g, int32_t env_idx, const void *in_host);
int mv_debug_rng(int32_t device, uint32_t seed, int32_t what, const int32_t *lo, const int32_t *hi, int32_t n, void *out_host);
int mv_debug_math(int32_t device, int32_t what, const float *a, const float *b, int32_t n, float *out_host);
/* The character controller's physics (megaverse_amd/csrc/mv_physics.h) on caller-given colliders, without a gym: one 64-lane wave per record runs the
 * templates the step kernels run, in the instantiation `variant` names -- MV_PHYS_NC1 Rearrange, MV_PHYS_NC2 TowerBuilding / Collect / BoxAGone,
 * MV_PHYS_NC4 Obstacles / Sokoban, MV_PHYS_HEX the Hex scenarios (boxes in wall frames), MV_PHYS_BALL Football (the ball).  Packed host records, 4-byte
 * fields.  cols: n_cols <= 64 NC of {int32 kind; float lo[3]; float hi[3]} in slot order (lane l of the wave holds slots l + 64 k; the lowest slot wins
 * ties): kind 0 none, 1 a box whose bounds are already grown by the capsule's half height in y, 2 another agent's capsule (lo = centre, hi[0] = segment
 * half length), 3 + f (MV_PHYS_HEX only) a box in hex wall frame f = 0..2, 7 (MV_PHYS_BALL only) the ball (lo = centre, hi[0] = the capsule's half
 * height, hi[1] = capsule radius + ball radius).  A kind the variant's kernels never hold is refused.
 *   mv_debug_sweep: {from[3], to[3], up[3], minSlopeDot} -> {int32 hit; float fraction; float normal[3]} (a miss: 0, 1.0, zeros);
 *   mv_debug_recover: a position [3] -> {int32 pushes; float pos_after_each[5][3]}, the push-out's at most five pushes (entries from `pushes` on repeat
 *     the last position);
 *   mv_debug_player_step: {pos[3], hvx, hvz, vvel, voffset, step_offset, jump_speed, int32 was_jumping, float reach2} -> the same record after one
 *     controller step of 1/15 s (reach2 is ignored on input).
 * Each call allocates, launches once, synchronises, copies back and frees.  All inputs must be finite. */
enum { MV_PHYS_NC1 = 0, MV_PHYS_NC2 = 1, MV_PHYS_NC4 = 2, MV_PHYS_HEX = 3, MV_PHYS_BALL = 4 };
int mv_debug_sweep(int32_t device, int32_t variant, const void *cols, int32_t n_cols, const void *queries, int32_t n_queries, void *out_host);
int mv_debug_recover(int32_t device, int32_t variant, const void *cols, int32_t n_cols, const float *positions, int32_t n, void *out_host);
int mv_debug_player_step(int32_t device, int32_t variant, const void *cols, int32_t n_cols, const void *agents_in, int32_t n, void *agents_out_host);
/* Host-only (no device): what the observation pass takes from the host per launch instead of computing it per workgroup (megaverse_amd/csrc/mv_raster.h:
 * RasterConsts, raster_ray_table) for a W x H observation -- consts[4] = sx, ox, sy, oy (ray abscissa = sx i + ox, sy j + oy), *tiles_x_inv =
 * the reciprocal of the tiles per row (mv_debug_raster_div_host's magic), dcx[W] / dcy[H] the abscissae of every column / row as the gym's
 * device table holds them.  Any pointer may be NULL (dcx and dcy are written together or not at all). */
int mv_debug_raster_consts_host(int32_t W, int32_t H, float *consts, uint32_t *tiles_x_inv, float *dcx, float *dcy);
/* Host-only: the reciprocal form of the pass's integer divisions -- *magic = ceil(2^32 / d) (0 for d = 1, which has none in 32 bits), q[n] = (n * magic) >> 32
 * (n where magic is 0) for n < n_end: == n / d in the kernels' range, tile indices below 2^16 and d <= 64. */
int mv_debug_raster_div_host(uint32_t d, uint32_t n_end, uint32_t *magic, uint32_t *q);
/* Host-only (no device): the n-th (1-based) episode an env seeded with env_seed generates for a host-generated
 * scenario (Obstacles family, Collect), as the raw blob the reset kernel swaps in.  Returns the blob size in
 * bytes (out == NULL: size query only), -1 on error.  Replaces Env::reset's scenario->reset() + spawnAgents
 * draws (env.cpp:57-76). */
int mv_debug_generate_episode(const char *scenario, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len,
                              void *out, int32_t out_bytes);
/* Host-only: runs the background episode feeder (worker pool that keeps every env's next episode generated ahead of
 * time; replaces the serial Env::reset inside VectorEnv::step, vector_env.cpp:93-105) for `rounds` episodes per env
 * and compares each delivered episode with sequential generation.  0 = identical. */
int mv_debug_feeder_selftest(const char *scenario, int32_t num_envs, int32_t num_agents, int32_t threads, int32_t rounds);
/* Host-only (no device): drives the episode feeder through a script of re-seeds (EpisodeFeeder::reseed_envs, what mv_seed_envs_host calls) and takes, and
 * compares every delivered episode with straight sequential generation from the same seeds (Sokoban: with the level list carried across a re-seed).
 * env_seeds [num_envs]: the initial Env::seed values.  script: n_ops x {op, env, value} -- op 0: take env's next episode (wait_ready, compare, recycle);
 * op 1: put (env, value) on the pending re-seed list; op 2: one reseed_envs call with that list.  out (or NULL): the delivered records, one per take in
 * script order; used_out (or NULL): the bytes of each the feeder reports as used.  Returns the number of takes, -1 with text on a difference or an error;
 * script == NULL and out == NULL: the record size. */
int mv_debug_feeder_reseed_script(const char *scenario, int32_t num_envs, int32_t num_agents, int32_t threads, const int32_t *env_seeds,
                                  const int32_t *script, int32_t n_ops, void *out, int64_t out_bytes, int32_t *used_out);
/* Host-only: the first n episodes of the Sokoban level generator (scenario_sokoban.cpp:80-170; its kernels come next) as n
 * packed records; out == NULL: record size.  Returns n, -1 on error. */
int mv_debug_generate_sokoban(int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes);
/* Host-only (no device): Football's episodes 1..n of an env seeded with env_seed, as n FootballBlob records (mv_types.h); out == NULL: one record's
   size.  Returns n. */
int mv_debug_generate_football(int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes);

/* Collect's episode generator as it runs on the DEVICE (megaverse_amd/csrc/mv_collect_draw.h; the product's feeder uses it where mv_host_generator_threads
 * says 0 for a Collect gym).  _host: the same code compiled for the CPU, no device needed -- the n-th episode of an env seeded
 * with env_seed, the record mv_debug_generate_episode("Collect", ...) returns (seq = n).  _device: `count` envs draw their first n episodes on the GPU, out
 * receives the n-th of each (count x the record size), *ms_per_launch the mean duration of a launch of `count` wavefronts.  Replaces CollectScenario::reset +
 * createLandscape + addEpisodeDrawables (scenario_collect.cpp:20-161,190-214), siv::PerlinNoise (perlin_noise.hpp:118-126,315-318). */
int mv_debug_collect_draw_host(int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes);
/* The Obstacles family's and Empty's generator as it runs on the DEVICE (megaverse_amd/csrc/mv_obstacles_draw.h; the feeder uses it where
 * mv_device_generator says 1 for such a gym), with the semantics of the two Collect hooks.  `scenario`: one of the six Obstacles names or "Empty".
 * _host: the same code compiled for the CPU (the merge in its serial form), the record mv_debug_generate_episode(scenario, ...) returns (seq = n); out == NULL:
 * the record's size.  _device: `count` envs draw their first n episodes on the GPU.  _stats_host: out[0 .. 3] = chain attempts, left turns, right turns and
 * GEN_* capacity flags of the n-th episode as mv_gen_obstacles.cpp draws it, out[4 .. 7] = the same four of mv_obstacles_draw.h's code on the CPU. */
int mv_debug_obstacles_draw_host(const char *scenario, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, void *out, int32_t out_bytes);
int mv_debug_obstacles_draw_stats_host(const char *scenario, int32_t num_agents, int32_t env_seed, int32_t n, float base_episode_len, int32_t *out8);
int mv_debug_obstacles_draw_device(int32_t device, const char *scenario, int32_t num_agents, const int32_t *env_seeds, int32_t count, int32_t n,
                                   float base_episode_len, void *out, int64_t out_bytes, float *ms_per_launch);
/* Host-only (no device): the episode log's per-tick body (megaverse_amd/csrc/mv_episode_log.h, the source the kernel runs) over k ticks of N envs x A
 * agents: rewards [k][N*A], dones [k][N], true_objectives [k][N*A]; first_tick: the first tick's end_tick.  In and out: ret [N*A], len [N], *count, *dropped,
 * and records, a buffer of `capacity` mv_episode_record of which *count are valid on entry. */
int mv_debug_episode_log_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A, int32_t capacity,
                              uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped);
/* ... with a step mask (mv_set_step_mask): step_mask [N] or NULL; the envs it freezes skip all k ticks.  NULL: mv_debug_episode_log_host, byte for byte. */
int mv_debug_episode_log_masked_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A,
                                     int32_t capacity, uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped,
                                     const uint8_t *step_mask /* [N] or NULL */);
/* ... and an episode budget (mv_set_episode_budget): left [N] or NULL, in and out -- the log's mirror of the budgets, advanced by the rule tick by tick; the
 * ticks of a halted env are skipped like a frozen env's.  left = NULL: mv_debug_episode_log_masked_host, byte for byte. */
int mv_debug_episode_log_budget_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A,
                                     int32_t capacity, uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped,
                                     const uint8_t *step_mask /* [N] or NULL */, int32_t *left /* [N] or NULL */);
/* ... and a macro step (mv_macro_step): tl [N] or NULL, in and out -- the log's mirror of the ticks left in the macro step the k ticks belong to (the caller
 * sets it to the call's clamped ticks), advanced by the rule of megaverse_amd/csrc/mv_macro_step.h; a tick the env does not step in is skipped.  tl = NULL:
 * mv_debug_episode_log_budget_host, byte for byte. */
int mv_debug_episode_log_macro_host(const float *rewards, const uint8_t *dones, const float *true_objectives, int32_t k, int32_t N, int32_t A,
                                    int32_t capacity, uint32_t first_tick, double *ret, int32_t *len, void *records, uint32_t *count, uint32_t *dropped,
                                    const uint8_t *step_mask /* [N] or NULL */, int32_t *left /* [N] or NULL */, int32_t *tl /* [N] or NULL */);
/* Host-only (no device): the rule of episode budgets (megaverse_amd/csrc/mv_episode_budget.h) over k ticks of N envs.  dones [k][N]: what tick t stages for
 * env e if it steps; mask [N] or NULL; left_in [N].  steps_out [k][N]: 1 where the env steps in the tick; left_out [N]: the budgets behind the last tick. */
int mv_debug_episode_budget_host(const uint8_t *dones, const uint8_t *mask, const int32_t *left_in, int32_t k, int32_t N, uint8_t *steps_out,
                                 int32_t *left_out);
/* Host-only (no device): the rule of macro steps (megaverse_amd/csrc/mv_macro_step.h) over the k ticks of one call of N envs.  dones, mask, left_in as above
 * (left_in: -1 where there is no budget); ticks_in [N] or NULL (every env: k), clamped to [0, k].  steps_out [k][N]: 1 where the env steps in the tick;
 * left_out [N], ticks_out [N]: the budgets and the ticks left behind the last tick. */
int mv_debug_macro_rule_host(const uint8_t *dones, const uint8_t *mask, const int32_t *left_in, const int32_t *ticks_in, int32_t k, int32_t N,
                             uint8_t *steps_out, int32_t *left_out, int32_t *ticks_out);
/* Host-only (no device): the fold of a macro step's rewards (mv_macro_step.h: macro_fold): values [k][n] -> out [n], s = v_0; s = s + v_t in tick order. */
int mv_debug_macro_fold_host(const float *values, int32_t k, int32_t n, float *out);
/* Host-only (no device): the rule of still frames (megaverse_amd/csrc/mv_still_frames.h) over k ticks of N envs.  steps [k][N]: 1 where the env steps in the
 * tick; has_pass [k]: 1 where the tick has an observation pass; draw_mask [N] or NULL; stale_in [N].  verdict_out [k][N]: 0 no pass, 1 drawn, -1 user-undrawn,
 * -2 still; stale_out [N]: the bytes behind the last tick. */
int mv_debug_still_rule_host(const uint8_t *steps, const uint8_t *has_pass, const uint8_t *draw_mask, const uint8_t *stale_in, int32_t k, int32_t N,
                             int32_t *verdict_out, uint8_t *stale_out);
/* Host-only (no device): the carry of still frames (mv_still_frames.h: still_carry_plan, the plan mv_set_still_frames' carry launch walks) over the k rendered
 * ticks of one call.  verdict [k][frames]: what the passes read for the frame (>= 0: drawn, -1: user-undrawn, -2: still); entries [k]: the ring entry of each
 * tick, 0 .. R - 1; ring_bytes [R][frames][frame_bytes], copied in place; home [frames], in and out: the entry that holds each frame's latest bytes (-1:
 * none). */
int mv_debug_still_carry_host(const int32_t *verdict, const int32_t *entries, int32_t k, int32_t frames, int32_t R, int32_t frame_bytes,
                              uint8_t *ring_bytes, int32_t *home);
/* Host-only (no device): the episode log's masked clear (megaverse_amd/csrc/mv_episode_log.h: episode_log_cut, the source mv_reset_envs' kernel runs) over N
 * envs x A agents: where mask[e] != 0, ret[e * A .. e * A + A - 1] and len[e] go to zero; everything else stays. */
int mv_debug_episode_log_cut_host(const uint8_t *mask, int32_t N, int32_t A, double *ret, int32_t *len);
/* Host-only (no device): the rule of a fork map (megaverse_amd/csrc/mv_fork.h, the source the kernel and mv_fork_envs_host run) applied to every entry of
 * src_of [N]: resolved[d] = the source env d would continue from, or -1 (left alone, or skipped); invalid[d] = 1 where the entry is invalid. */
int mv_debug_fork_plan_host(const int32_t *src_of, int32_t N, int32_t *resolved /* [N]: s or -1 */, int32_t *invalid /* [N]: 0/1 */);
/* Host-only (no device): the rule of a resampling map (megaverse_amd/csrc/mv_fork.h, the source the kernels and mv_resample_envs_host run) applied to every
 * entry of src_of [N]: resolved[d] = the source whose pre-call state env d takes, or -1 (left alone, or skipped); staged[d] = 1 where env d's new state goes
 * through the staging arena; invalid[d] = 1 where the entry is out of range.  The tabulated O(N) plan is checked against the per-entry form. */
int mv_debug_resample_plan_host(const int32_t *src_of, int32_t N, int32_t *resolved /* [N]: s or -1 */, int32_t *staged /* [N]: 0/1 */,
                                int32_t *invalid /* [N]: 0/1 */);
/* Host-only (no device): the two phases of mv_resample_envs over state[N][bytes_per_env] in host memory, with a temporary staging array, decided per env by
 * the code the kernels use; invalid entries are skipped.  order: the envs of each phase are visited ascending (0), descending (1) or in a fixed
 * pseudo-random order (2) -- the result does not depend on it. */
int mv_debug_resample_apply_host(const int32_t *src_of, int32_t N, int32_t bytes_per_env, uint8_t *state, int32_t order);
/* Host-only (no device): the rule of an env-store map (megaverse_amd/csrc/mv_env_store.h, the source the kernels and the host forms run) applied to every
 * entry of slot_of [N] for a store of `slots` records: is_save != 0: mv_save_envs' rule (out of range, or a slot named twice: invalid), else mv_load_envs'
 * (out of range only).  resolved[e] = the slot, or -1 (not named, or skipped).  The tabulated host rule is checked against the per-entry rule. */
int mv_debug_env_store_plan_host(const int32_t *slot_of, int32_t N, int32_t slots, int32_t is_save, int32_t *resolved /* [N] */, int32_t *invalid /* [N] */);
/* Host-only (no device): a record's layout for `count` state arrays of array_bytes[k] bytes per env and A agents: offsets [count + 3] = where the EnvHeader,
 * each array, ret and len lie -> the record's bytes. */
int64_t mv_debug_env_record_layout_host(const uint32_t *array_bytes, int32_t count, int32_t A, uint32_t *offsets);
/* Host-only (no device): an env in host memory -- its 128-byte EnvHeader, its `count` arrays, double ret[A], int32 len, one behind the other -- packed into
 * a record / a record unpacked into such an env, by the functions the kernels use.  log_on: whether the (saving / loading) gym's episode log is on.  Unpack
 * returns 1 and changes nothing when the record's header does not match (layout_word, the record size these arrays imply, the format). */
int mv_debug_env_record_pack_host(const uint32_t *array_bytes, int32_t count, int32_t A, uint64_t layout_word, int32_t log_on, const uint8_t *env_state_in,
                                  uint8_t *record_out);
int mv_debug_env_record_unpack_host(const uint32_t *array_bytes, int32_t count, int32_t A, uint64_t layout_word, int32_t log_on, const uint8_t *record_in,
                                    uint8_t *env_state_inout);
/* out_host [N]: how many episodes of its own sequence every env has taken so far (a fork leaves the destination's count alone) */
int mv_debug_episodes_consumed(mv_gym *g, int32_t *out_host);
int mv_debug_collect_draw_device(int32_t device, int32_t num_agents, const int32_t *env_seeds, int32_t count, int32_t n, float base_episode_len, void *out,
                                 int64_t out_bytes, float *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif
