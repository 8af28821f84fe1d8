"""Multi-task batches: several scenarios stepped side by side on one GPU.

Reference: megaverse/megaverse_env.py:11-39.  The reference runs a multi-task job as one MegaverseGym per scenario
(``make_env_multitask`` picks ``tasks[task_idx % len(tasks)]`` per worker); BASELINE.json configs[4] deals the scenarios
round-robin by env index.  ``MultiTaskGym`` owns one HIP gym per scenario -- own state, own episode feeder -- and steps them
as ONE group (``mv_group``): one step launch whose workgroups run their own scenario's tick, at most two observation launches
(the short-list and the long-list raster variant), one pair of streams, pipelined like a single gym; three launches per tick
instead of sixteen.  All of them write into ONE observation slab, scenario-major: frames of scenario k are rows
[k * n_k * A, (k + 1) * n_k * A).  (``MV_MULTITASK_UNION=0``: the round-2 scheme, one stream per scenario and one launch pair
per gym, kept for comparison.)

Global env index i  <->  (scenario i % S, local env i // S).  Seeds and the benchmark's random actions are drawn per
GLOBAL env index (mv_config.env_stride), so the job is bit-identical to S separately seeded single-scenario jobs that
share one master stream -- and every sub-gym is bit-exact against the oracle by the single-scenario parity tests.
"""
import os

import numpy as np

from .extension import EPISODE_RECORD_DTYPE, MEGAVERSE8, GymGroup, MegaverseGym, check_env_seeds

# MultiTaskGym.drain_episode_log: a sub-gym's record (extension.EPISODE_RECORD_DTYPE) + the task it came from; agent in the batch's numbering
MULTITASK_EPISODE_DTYPE = np.dtype([("task", "<i4")] + [(n, EPISODE_RECORD_DTYPE.fields[n][0]) for n in EPISODE_RECORD_DTYPE.names])

# megaverse_env.py:18-21 of the reference: the eight scenarios of its multi-task benchmark, all available on the HIP path
# (Sokoban reads Boxoban level files: $BOXOBAN_LEVELS, as in the reference)
MEGAVERSE_IN_SCOPE = MEGAVERSE8   # (older name)


def split_action_ring(actions, num_scenarios, agents_per_env):
    """[count, num_envs * A, 6] actions in the batch's global env numbering -> one [count, n_k * A, 6] array per sub-gym, by MultiTaskGym.locate's rule (global
    env i is local env i // S of sub-gym i % S).  numpy arrays and torch tensors alike (views: the caller makes them contiguous)."""
    S, A = int(num_scenarios), int(agents_per_env)
    count = actions.shape[0]
    per_task = actions.shape[1] // (S * A)
    byenv = actions.reshape(count, per_task, S, A, 6)
    return [byenv[:, :, k].reshape(count, per_task * A, 6) for k in range(S)]


def check_action_ring(actions, num_envs, agents_per_env):
    """MultiTaskGym.set_action_ring's argument check (no device needed): a [count >= 1, num_envs * A, 6] int32 numpy array or tensor -> count"""
    shape = tuple(getattr(actions, "shape", ()))
    if len(shape) != 3 or shape[0] < 1 or shape[1:] != (int(num_envs) * int(agents_per_env), 6):
        raise ValueError(f"set_action_ring: actions must be [count >= 1, num_envs * agents_per_env = {int(num_envs) * int(agents_per_env)}, 6], got {shape}")
    if str(actions.dtype).split(".")[-1] != "int32":
        raise ValueError(f"set_action_ring: actions must be int32, got {actions.dtype}")
    return int(shape[0])


def _per_gym(setter, what, verb):
    """-> the RuntimeError of a MultiTaskGym method whose option is per gym: `what` is attached by mv_<setter>, and a group's union launches `verb` none"""
    return RuntimeError(f"MultiTaskGym.{setter}: mv_group_create and mv_step_many refuse a gym with {what} attached "
                        f"(mv_{setter}): the union launches {verb} none; step such a gym on its own")


class MultiTaskGym:
    def __init__(self, scenarios, w, h, num_envs, num_agents_per_env, num_simulation_threads=4, float_params=None, device=0,
                 env_offset=0, total_envs=0, obs_layout="rgba"):
        """obs_layout: 'rgba' -- frames [h, w, 4] -- or 'chw' -- [3, h, w], written so by the observation pass (include/megaverse_hip.h:
        mv_set_obs_layout); attach / attach_tensor / set_output_ring allocate and check frames of that shape"""
        S = len(scenarios)
        if obs_layout not in ("rgba", "chw"):
            raise ValueError("obs_layout must be 'rgba' or 'chw'")
        self.obs_layout = obs_layout
        if num_envs % S:
            raise ValueError("num_envs must be a multiple of the number of scenarios")
        self.scenarios = list(scenarios)
        union = os.environ.get("MV_MULTITASK_UNION", "1") != "0" and S <= 8
        for name in ("BoxAGone", "Football"):   # (mv_group_create refuses them as well)
            if union and any(str(n).casefold() == name.casefold() for n in self.scenarios):
                raise ValueError(f"MultiTaskGym: {name} cannot be stepped in a group of gyms (the union kernels have no {name} tick); "
                                 "set MV_MULTITASK_UNION=0 for one gym per scenario, or step it as a MegaverseEnv of its own")
        self.w, self.h, self.num_envs, self.num_agents_per_env = int(w), int(h), int(num_envs), int(num_agents_per_env)
        self.per_task = num_envs // S
        total = total_envs if total_envs > 0 else num_envs
        self.gyms = [MegaverseGym(name, w, h, self.per_task, num_agents_per_env, num_simulation_threads, False, float_params or {},
                                  device=device, env_offset=env_offset + k, total_envs=total, env_stride=S)
                     for k, name in enumerate(self.scenarios)]
        for g in self.gyms:
            g.set_obs_layout(obs_layout)
        self.union = os.environ.get("MV_MULTITASK_UNION", "1") != "0" and len(self.gyms) <= 8
        if not self.union:
            for g in self.gyms:   # the sub-gyms overlap each other, one stream each: a second (simulation) stream per gym only
                g.set_pipelining(False)   # oversubscribes the hardware queues (measured: 8 gyms, 64 x 64: 3.5 M vs 6.0 M obs/s)
        self._group = None
        self._streams = None
        self._obs = None
        self._handles = None
        self._sample = None
        self.ring_obs = self.ring_rewards = self.ring_dones = None
        self.action_rings = None

    # ---- plumbing: torch owns the slab and the streams
    def attach(self, torch_device):
        import torch
        A = self.num_agents_per_env
        return self.attach_tensor(torch.empty((self.num_envs * A,) + self.frame_shape(), dtype=torch.uint8, device=torch_device))

    def frame_shape(self):
        """one observation frame: (h, w, 4), or (3, h, w) with obs_layout='chw'"""
        return (3, self.h, self.w) if self.obs_layout == "chw" else (self.h, self.w, 4)

    def attach_tensor(self, obs):
        """render into the caller's [num_envs * A, h, w, 4] uint8 slab -- [num_envs * A, 3, h, w] with obs_layout='chw' (one stream per scenario,
        created on first use)"""
        import torch
        A, n = self.num_agents_per_env, self.per_task
        assert tuple(obs.shape) == (self.num_envs * A,) + self.frame_shape() and obs.dtype == torch.uint8 and obs.is_contiguous()
        if self.union:
            if self._group is None:   # one stream for all of them: torch's current one
                cur = torch.cuda.current_stream(obs.device).cuda_stream
                for g in self.gyms:
                    g.set_stream(cur)
                self._group = GymGroup(self.gyms)
        elif self._streams is None:
            self._streams = [torch.cuda.Stream(device=obs.device) for _ in self.gyms]
            for k, g in enumerate(self.gyms):
                g.set_stream(self._streams[k].cuda_stream)
        self._obs = obs
        frame_bytes = int(np.prod(self.frame_shape()))
        for k, g in enumerate(self.gyms):
            g.set_obs_buffer(obs.data_ptr() + k * n * A * frame_bytes)
        return obs

    def set_output_ring(self, count):
        """Rollout rings, one set per scenario (mv_set_output_ring): tick t of sub-gym k leaves its observations in ``ring_obs[k][t % count]``
        ([count, n_k * A, h, w, 4] uint8; obs_layout='chw': [count, n_k * A, 3, h, w]), its rewards in ``ring_rewards[k][t % count]`` and its dones in ``ring_dones[k][t % count]``.  With rings at
        least as deep as a call (of 2 ... 8 ticks; up to 1024 envs in the group), ``step_n`` is TWO launches for all scenarios and all of its ticks (one union
        step launch, one union observation launch); otherwise two launches per tick.  count = 0: back to the shared slab.  -> (ring_obs, ring_rewards, ring_dones), lists of CUDA tensors."""
        import torch
        if count <= 0:
            for g in self.gyms:
                g.set_output_ring(0)
            self.ring_obs = self.ring_rewards = self.ring_dones = None
            return None
        dev = self._obs.device if self._obs is not None else torch.device("cuda", self.gyms[0].device if hasattr(self.gyms[0], "device") else 0)
        A, n = self.num_agents_per_env, self.per_task
        self.ring_obs = [torch.zeros((count, n * A) + self.frame_shape(), dtype=torch.uint8, device=dev) for _ in self.gyms]
        self.ring_rewards = [torch.zeros((count, n * A), dtype=torch.float32, device=dev) for _ in self.gyms]
        self.ring_dones = [torch.zeros((count, n), dtype=torch.uint8, device=dev) for _ in self.gyms]
        torch.cuda.synchronize(dev)
        for k, g in enumerate(self.gyms):
            g.set_output_ring(count, self.ring_obs[k].data_ptr(), self.ring_rewards[k].data_ptr(), self.ring_dones[k].data_ptr())
        return self.ring_obs, self.ring_rewards, self.ring_dones

    def set_action_ring(self, actions):
        """Action rings for step_n(..., policy='sequence') (mv_set_action_ring): `actions` is ONE int32 [count, num_envs * A, 6] array -- numpy, or a CUDA
        tensor -- in the batch's global env numbering; every sub-gym gets its own contiguous [count, n_k * A, 6] part (locate's rule), kept alive in
        ``action_rings``.  None detaches.  Call it again after changing the actions: the parts are copies."""
        if actions is None:
            for g in self.gyms:
                g.set_action_ring(0)
            self.action_rings = None
            return None
        count = check_action_ring(actions, self.num_envs, self.num_agents_per_env)
        import torch
        dev = self._obs.device if self._obs is not None else torch.device("cuda", self.gyms[0].device)
        if not hasattr(actions, "data_ptr"):
            actions = torch.as_tensor(np.ascontiguousarray(actions))
        actions = actions.to(dev)
        self.action_rings = [p.contiguous() for p in split_action_ring(actions, len(self.gyms), self.num_agents_per_env)]
        for g, ring in zip(self.gyms, self.action_rings):   # (the copies run on torch's current stream: the gyms' stream, attach_tensor)
            g.set_action_ring(count, ring.data_ptr())
        return self.action_rings

    def macro_step(self, k, actions, ticks=None, render="last"):
        """macro steps (MegaverseGym.macro_step) are per gym: mv_macro_step refuses a gym in an mv_group, and a multi-task batch has no call that holds one
        decision over k ticks of every sub-gym -- not provided"""
        raise RuntimeError("MultiTaskGym.macro_step: not provided -- mv_macro_step refuses a gym that belongs to an mv_group (the union launches know no "
                           "macro steps); use one MegaverseGym per task and call its macro_step")

    def set_episode_budget(self, budget):
        """episode budgets (MegaverseGym.set_episode_budget) are per gym: a group's union launches read none, and the library refuses"""
        if self._group is not None and budget is not None:
            self.gyms[0].set_episode_budget(budget if isinstance(budget, (int, np.integer)) else 1)   # (raises, with the library's text)
        raise _per_gym("set_episode_budget", "an episode budget", "read")

    def set_draw_mask(self, mask):
        """draw masks (MegaverseGym.set_draw_mask) are per gym: a group's union launches read none, and the library refuses"""
        if self._group is not None and mask is not None:
            self.gyms[0].set_draw_mask(np.ones(self.gyms[0].num_envs, np.bool_))   # (raises, with the library's text)
        raise _per_gym("set_draw_mask", "a draw mask", "read")

    def set_depth_obs(self, buf=True, dtype=None):
        """depth observations (MegaverseGym.set_depth_obs) are per gym: a group's union launches write none, and the library refuses"""
        raise _per_gym("set_depth_obs", "depth observations", "write")

    def set_seg_obs(self, buf=True, fmt="class"):
        """segmentation observations (MegaverseGym.set_seg_obs) are per gym: a group's union launches write none, and the library refuses"""
        raise _per_gym("set_seg_obs", "segmentation observations", "write")

    def set_normal_obs(self, buf=True, dtype=None):
        """normal observations (MegaverseGym.set_normal_obs) are per gym: a group's union launches write none, and the library refuses"""
        raise _per_gym("set_normal_obs", "normal observations", "write")

    def set_state_obs(self, buf=True):
        """state observations (MegaverseGym.set_state_obs) are per gym: a group's union launches write none, and the library refuses"""
        raise _per_gym("set_state_obs", "state observations", "write")

    def set_scene_obs(self, buf=True):
        """scene observations (MegaverseGym.set_scene_obs) are per gym: a group's union launches write none, and the library refuses"""
        raise _per_gym("set_scene_obs", "scene observations", "write")

    def set_entity_obs(self, buf=True):
        """entity observations (MegaverseGym.set_entity_obs) are per gym: a group's union launches write none, and the library refuses"""
        raise _per_gym("set_entity_obs", "entity observations", "write")

    def set_overview(self, w, h, buf=True):
        """overview cameras (MegaverseGym.set_overview) are per gym: a group's union launches draw none, and the library refuses"""
        raise _per_gym("set_overview", "an overview", "draw")

    def recommended_ticks_per_call(self):
        """the k to ask step_n for: what every member recommends (mv_recommended_ticks_per_call), at most 8 -- the two-launch group call's limit"""
        return max(1, min([8] + [g.recommended_ticks_per_call() for g in self.gyms]))

    def recommended_pass_overlap(self):
        return False

    def device_generator(self):
        """per member: are its episodes drawn on the device (MegaverseGym.device_generator)?"""
        return [g.device_generator() for g in self.gyms]

    def set_pixel_mode(self, mode):
        for g in self.gyms:
            g.set_pixel_mode(mode)

    # ---- episode log (include/megaverse_hip.h: mv_set_episode_log): every sub-gym keeps its own
    def set_episode_log(self, capacity):
        """`capacity` records per scenario (0: off)"""
        for g in self.gyms:
            g.set_episode_log(capacity)

    def flush_episode_log(self):
        for g in self.gyms:
            g.flush_episode_log()

    def episode_log_count(self):
        """-> (records waiting, records dropped), summed over the scenarios"""
        counts = [g.episode_log_count() for g in self.gyms]
        return sum(c for c, _ in counts), sum(d for _, d in counts)

    def drain_episode_log(self):
        """every sub-gym's records as ONE array of MULTITASK_EPISODE_DTYPE: `task` is the sub-gym, `agent` is global_env * A + a with the batch's env
        numbering (the inverse of locate: local env j of task k is global env j * S + k), sorted by (end_tick, agent).  end_tick counts each
        sub-gym's own ticks since its reset -- the same for all of them when they are reset and stepped together."""
        S, A = len(self.gyms), self.num_agents_per_env
        parts = []
        for k, g in enumerate(self.gyms):
            r = g.drain_episode_log()
            out = np.zeros(r.size, MULTITASK_EPISODE_DTYPE)
            for n in EPISODE_RECORD_DTYPE.names:
                out[n] = r[n]
            out["task"] = k
            out["agent"] = ((r["agent"] // A) * S + k) * A + r["agent"] % A
            parts.append(out)
        allr = np.concatenate(parts) if parts else np.zeros(0, MULTITASK_EPISODE_DTYPE)
        return allr[np.lexsort((allr["agent"], allr["end_tick"]))]

    def locate(self, env_idx):
        """global env index -> (sub-gym, local env index)"""
        S = len(self.gyms)
        return self.gyms[env_idx % S], env_idx // S

    def frame_row(self, env_idx, agent_idx=0):
        """row of the shared observation slab that holds (global env, agent)"""
        S, A = len(self.gyms), self.num_agents_per_env
        return ((env_idx % S) * self.per_task + env_idx // S) * A + agent_idx

    # ---- MegaverseGym surface, env indices are global
    def num_agents(self):
        return self.num_envs * self.num_agents_per_env

    def seed(self, seed):
        for g in self.gyms:
            g.seed(seed)

    def reset(self):
        for g in self.gyms:
            g.reset()

    def reset_envs(self, mask, render=True):
        """Masked resets (MegaverseGym.reset_envs; mv_reset_envs follows mv_reset's path, so members of a group are served): `mask` holds one bool per env in
        the batch's global numbering -- a numpy array / sequence (host form) or a bool / uint8 CUDA tensor (device form) -- and is dealt to the sub-gyms by
        locate's rule (global env i is local env i // S of sub-gym i % S).  The parts of a tensor are copies made on torch's current stream, the gyms'."""
        S = len(self.gyms)
        if hasattr(mask, "data_ptr"):
            if tuple(mask.shape) != (self.num_envs,):
                raise ValueError(f"reset_envs: the mask must have shape ({self.num_envs},), got {tuple(mask.shape)}")
            parts = [mask.reshape(self.per_task, S)[:, k].contiguous() for k in range(S)]
        else:
            m = np.asarray(mask)
            if m.shape != (self.num_envs,):
                raise ValueError(f"reset_envs: the mask must be {self.num_envs} bools, got {m.dtype} {m.shape}")
            parts = [np.ascontiguousarray(m.reshape(self.per_task, S)[:, k]) for k in range(S)]
        for g, part in zip(self.gyms, parts):
            g.reset_envs(part, render)

    def seed_envs(self, seeds):
        """Level seeds (MegaverseGym.seed_envs; members of a group are served like reset_envs'): `seeds` in the batch's global numbering -- num_envs ints
        (negative or None: leave the env alone), a dict {env: seed}, or an int32 CUDA tensor (TowerBuilding members only) -- dealt to the sub-gyms by
        locate's rule.  The parts of a tensor are copies made on torch's current stream, the gyms'."""
        S = len(self.gyms)
        if hasattr(seeds, "data_ptr"):
            check_env_seeds(seeds, self.num_envs)
            host_fed = [g.scenario for g in self.gyms if not g.episodes_drawn_on_device()]
            if host_fed:   # (refused before the first member is touched)
                raise RuntimeError(f"MultiTaskGym.seed_envs: a tensor takes mv_seed_envs' device form, which {', '.join(host_fed)} refuse (their episode "
                                   "generators live on the host): pass the seeds as a numpy array, a sequence or a dict (mv_seed_envs_host)")
            parts = [seeds.reshape(self.per_task, S)[:, k].contiguous() for k in range(S)]
        else:
            m = check_env_seeds(seeds, self.num_envs)
            parts = [np.ascontiguousarray(m.reshape(self.per_task, S)[:, k]) for k in range(S)]
        for g, part in zip(self.gyms, parts):
            g.seed_envs(part)

    def set_actions(self, env_idx, agent_idx, actions):
        g, j = self.locate(env_idx)
        g.set_actions(j, agent_idx, actions)

    def sample_random_actions(self, seed, step_index):
        self._sample = (int(seed) & 0xFFFFFFFF, int(step_index) & 0xFFFFFFFF)   # drawn inside the next step (one C call for all sub-gyms)

    def _ensure_group(self):
        if self.union and self._group is None:
            self._group = GymGroup(self.gyms)
        return self._group

    def step_n(self, k, policy="multidiscrete", seed=0, first_step_index=0):
        """k open-loop ticks of every scenario with one call (union launches; mv_group_step); without the union (MV_MULTITASK_UNION=0, or more
        scenarios than a group holds): k single steps of every sub-gym.  Every tick is drawn: groups keep their own render=True/False (GymGroup.step,
        mv_group_step); the render modes of MegaverseGym.step_n ('last' / 'none') are a single gym's."""
        if not self.union:
            if policy == "sequence":   # (every sub-gym replays its own ring)
                for g in self.gyms:
                    g.step_n(k, "sequence", 0, first_step_index)
                return
            if policy != "multidiscrete":
                raise ValueError("MultiTaskGym.step_n without union launches supports the 'multidiscrete' and 'sequence' policies only")
            for j in range(int(k)):
                self.sample_random_actions(seed, int(first_step_index) + j)
                self.step()
            return
        self._ensure_group().step(k, True, policy, seed, first_step_index)
        self._release_seeds()

    def _release_seeds(self):
        """a stepping call has been enqueued: the members' device seeds (seed_envs with a tensor: per-member copies) have been read in stream order"""
        for g in self.gyms:
            g._seed_held = []

    def step(self):
        import ctypes as C
        if self.union:
            seed, idx = self._sample if self._sample else (0, 0)
            self._ensure_group().step(1, True, "multidiscrete" if self._sample else "none", seed, idx)
            self._sample = None
            self._release_seeds()
            return
        if self._handles is None:
            self._handles = (C.c_void_p * len(self.gyms))(*[g._g for g in self.gyms])
        lib = self.gyms[0]._lib
        seed, idx = self._sample if self._sample else (0, 0)
        rc = lib.mv_step_many(self._handles, len(self.gyms), 1, 1 if self._sample else 0, seed, idx)
        self._sample = None   # (every sub-gym was stepped, whatever one of them reports: nothing to retry)
        self._release_seeds()
        if rc < 0:
            raise RuntimeError(lib.mv_last_error().decode())
        if rc > 0:
            import warnings
            warnings.warn(lib.mv_last_error().decode(), RuntimeWarning, stacklevel=2)

    def synchronize(self):
        for g in self.gyms:
            g.synchronize()

    def is_done(self, env_idx):
        g, j = self.locate(env_idx)
        return g.is_done(j)

    def get_observation(self, env_idx, agent_idx):
        g, j = self.locate(env_idx)
        return g.get_observation(j, agent_idx)

    def get_last_rewards(self):
        """env-major over GLOBAL env indices, like MegaverseGym::getLastRewards (megaverse.cpp:128-137)"""
        S, A = len(self.gyms), self.num_agents_per_env
        out = np.empty((self.per_task, S, A), np.float32)
        for k, g in enumerate(self.gyms):
            out[:, k, :] = g.get_rewards_array().reshape(self.per_task, A)
        return out.reshape(-1)

    def true_objective(self, env_idx, agent_idx):
        g, j = self.locate(env_idx)
        return g.true_objective(j, agent_idx)

    def profile_begin(self, n):
        for g in self.gyms:
            g.profile_begin(n)

    def profile_end(self):
        return [g.profile_end() for g in self.gyms]

    def close(self):
        if self._group is not None:
            self._group.close()
            self._group = None
        for g in self.gyms:
            g.close()
