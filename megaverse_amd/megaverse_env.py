"""MegaverseEnv: the reference's Python surface on top of the HIP simulator.

Reference: megaverse/megaverse_env.py:42-201 (class MegaverseEnv(gym.Env)).  Same constructor
arguments, attributes (num_envs, num_agents_per_env, num_agents, action_space, observation_space,
is_multiagent) and methods (seed/reset/step/render/close + reward-shaping accessors), same return
conventions: ``reset() -> [obs]*num_agents`` with obs uint8 (3, H, W) *un-flipped* (rows bottom-up),
``step(actions) -> (obs, rewards, dones, infos)`` with ``infos[i] = {'true_reward': ...}`` on done.

Differences, all additive:
  * img_w/img_h are constructor keywords (reference hard-codes 128x72, megaverse_env.py:51-52);
  * ``step_batched`` / ``step_device`` / ``observations_tensor`` return one device tensor instead of O(num_agents)
    numpy views (the Python loops at megaverse_env.py:121-130,138-141 cap the reference well below
    the GPU's rate);
  * gym and cv2 are optional;
  * ``obs_layout="chw"`` (opt-in): the observation pass writes the frames as (3, H, W) planes itself, so the device tensors are contiguous and the
    host copy moves 3 bytes per pixel instead of 4 (include/megaverse_hip.h: mv_set_obs_layout).
"""
import numpy as np

from . import spaces
from .extension import ENTITY_OBS_FIELDS, MEGAVERSE8, MegaverseGym, SCENARIOS, SCENE_OBS_FIELDS, SCENE_OBS_SCENARIO_FIELDS, STATE_OBS_FIELDS, render_mode_of, \
    set_megaverse_log_level

OBSTACLES_MULTITASK = ['ObstaclesWalls', 'ObstaclesSteps', 'ObstaclesLava', 'ObstaclesEasy', 'ObstaclesHard']
# what libmegaverse_hip.so can construct (mv_create): every scenario of the reference's multi-task sets, Empty, BoxAGone and Football
SUPPORTED_SCENARIOS = list(SCENARIOS)
_warned_unsupported = False


def make_env_multitask(multitask_name, task_idx, num_envs, num_agents_per_env, num_simulation_threads, use_vulkan=False, params=None):
    """reference: megaverse_env.py:27-39"""
    assert 'multitask' in multitask_name
    if multitask_name.endswith('megaverse8'):
        tasks = MEGAVERSE8
    elif multitask_name.endswith('obstacles'):
        tasks = OBSTACLES_MULTITASK
    else:
        raise NotImplementedError()
    supported = [t for t in tasks if t in SUPPORTED_SCENARIOS]
    if len(supported) != len(tasks):   # say it once, up front, instead of failing in 2 of every 8 workers at construction
        global _warned_unsupported
        if not _warned_unsupported:
            import warnings
            warnings.warn(f"{multitask_name}: {sorted(set(tasks) - set(supported))} are not available in this build; "
                          f"the multi-task job is dealt over {supported}")
            _warned_unsupported = True
        tasks = supported
    scenario = tasks[task_idx % len(tasks)]
    return MegaverseEnv(scenario, num_envs, num_agents_per_env, num_simulation_threads, use_vulkan, params)


def check_sequence_actions(actions, num_agents):
    """MegaverseEnv.step_sequence's argument check (no device needed): [k >= 1, num_agents, 6] -- an integer numpy array, or a CUDA int32 tensor -> k"""
    is_tensor = hasattr(actions, 'data_ptr')
    if not is_tensor:
        actions = np.asarray(actions)
    shape = tuple(actions.shape)
    if len(shape) != 3 or shape[0] < 1 or shape[1:] != (int(num_agents), 6):
        raise ValueError(f'step_sequence: actions must be [k >= 1, num_agents = {int(num_agents)}, 6], got {shape}')
    if is_tensor:
        if str(actions.dtype) != 'torch.int32' or not actions.is_cuda:
            raise ValueError(f'step_sequence: a tensor of actions must be int32 and on the device, got {actions.dtype} on {actions.device}')
    elif actions.dtype.kind not in 'iu':
        raise ValueError(f'step_sequence: actions must be integers, got {actions.dtype}')
    return int(shape[0])


class MegaverseEnv:
    def __init__(self, scenario_name, num_envs, num_agents_per_env, num_simulation_threads=1, use_vulkan=False, params=None,
                 img_w=128, img_h=72, device=0, env_offset=0, total_envs=0, obs_layout="rgba", episode_log=0, state_obs=False, frame_skip=1,
                 still_frames=False, scene_obs=False, depth_obs=False, seg_obs=False, entity_obs=False, overview=None, normal_obs=False):
        if isinstance(frame_skip, (bool, np.bool_)) or not isinstance(frame_skip, (int, np.integer)) or int(frame_skip) < 1:
            raise ValueError(f"frame_skip must be an int >= 1, got {frame_skip!r}")
        # frame_skip = k > 1: step, step_batched and step_device hold their actions for up to k ticks -- one macro step (MegaverseGym.macro_step) per call: every
        # env stops at its own first done, rewards are the sums, dones the ORs, the observation the frame behind the last tick.  1: every path as it always was.
        self.frame_skip = int(frame_skip)
        if obs_layout not in ("rgba", "chw"):
            raise ValueError("obs_layout must be 'rgba' (frames written as (H, W, 4) RGBA, handed out as a permuted view) or 'chw' (written as (3, H, W))")
        scenario_name = scenario_name.casefold()
        self.obs_layout = obs_layout
        self.scenario_name = scenario_name
        self.is_multiagent = True
        set_megaverse_log_level(2)

        self.img_w, self.img_h, self.channels = int(img_w), int(img_h), 3
        self.use_vulkan = use_vulkan
        self.num_agents = num_envs * num_agents_per_env
        self.num_envs = num_envs
        self.num_agents_per_env = num_agents_per_env
        self.device = device

        float_params = {}
        if params is not None:
            for k, v in params.items():
                if isinstance(v, float):
                    float_params[k] = v
                else:
                    raise Exception('Params of type %r not supported', type(v))

        self.env = MegaverseGym(self.scenario_name, self.img_w, self.img_h, num_envs, num_agents_per_env, num_simulation_threads,
                                use_vulkan, float_params, device=device, env_offset=env_offset, total_envs=total_envs)
        if obs_layout == "chw":
            self.env.set_obs_layout("chw")
        # episode_log = capacity > 0: returns, lengths and true objectives of finished episodes are collected on the device (mv_set_episode_log) and read
        # with self.env.drain_episode_log() -- what the fast paths (step_device, env.step_n) otherwise leave to the caller
        self.episode_log = int(episode_log)
        if self.episode_log > 0:
            self.env.set_episode_log(self.episode_log)
        # The observation streams beside the RGB frames, each a CUDA tensor the gym writes without a host wait, read with self.<name>_obs(); the gym observation
        # space stays the RGB one.  _streams: the wanted ones, name -> the arguments of MegaverseGym.set_<name>_obs behind True, in the order they are attached.
        #   state_obs: every tick leaves one row of 16 float32 per agent (STATE_OBS_FIELDS: pose, velocities, carrying, episode time, total reward;
        #     mv_set_state_obs) -- in every render mode
        #   scene_obs: ... one row of 32 float32 per ENV (SCENE_OBS_FIELDS, SCENE_OBS_SCENARIO_FIELDS: level, goal and ball; mv_set_scene_obs)
        #   entity_obs: ... E rows of 8 float32 per ENV (ENTITY_OBS_FIELDS: segmentation word, centre, half extents, state of every terrain box, movable
        #     object, collectable and agent; megaverse_amd.entity_layout has the rows; mv_set_entity_obs)
        #   depth_obs (True: float32, "float16"): every drawn frame leaves its per-pixel camera depth (mv_set_depth_obs)
        #   seg_obs (True: the class byte, "instance": class << 12 | instance): every drawn frame leaves its per-pixel labels (mv_set_seg_obs)
        if depth_obs is not False and depth_obs is not True and depth_obs not in ("float16", "float32"):
            raise ValueError(f"depth_obs must be False, True or 'float16', got {depth_obs!r}")
        #   normal_obs (True: float16, "int8": signed normalised bytes): every drawn frame leaves its per-pixel camera-space surface normals (mv_set_normal_obs)
        if normal_obs is not False and normal_obs is not True and normal_obs not in ("float16", "int8"):
            raise ValueError(f"normal_obs must be False, True, 'float16' or 'int8', got {normal_obs!r}")
        if seg_obs is not False and seg_obs is not True and seg_obs not in ("class", "instance"):
            raise ValueError(f"seg_obs must be False, True, 'class' or 'instance', got {seg_obs!r}")
        wanted = (("state", state_obs, ()), ("scene", scene_obs, ()), ("entity", entity_obs, ()),
                  ("depth", depth_obs, ("float32" if depth_obs is True else depth_obs,)), ("seg", seg_obs, ("class" if seg_obs is True else seg_obs,)),
                  ("normal", normal_obs, ("float16" if normal_obs is True else normal_obs,)))
        self._streams = {name: args for name, on, args in wanted if on}
        if "state" in self._streams:
            self._attach_stream("state")
        # still_frames: envs that did not change -- frozen, halted by a budget, stopped inside a macro step -- are not drawn again (mv_set_still_frames); every
        # observation byte stays what it is without the option.  Switched on behind the state rows and before every other stream, as it always was: under
        # still frames the plane setters refuse, in their own words
        if still_frames:
            self.env.set_still_frames(True)
        for name in self._streams:
            if name != "state":
                self._attach_stream(name)
        # overview = (w, h): one overview camera per env (mv_set_overview), every env at the reference's pose until set_overview_cameras moves them; drawn on
        # demand by render_overview(), read with self.overview_obs(); no stepping call changes
        if overview is not None:
            if len(tuple(overview)) != 2:
                raise ValueError(f"overview must be None or (w, h), got {overview!r}")
            self.env.set_overview(int(overview[0]), int(overview[1]))
        self.default_shaping_scheme = self.env.get_reward_shaping(0, 0)
        self.action_space = self.generate_action_space(self.env.action_space_sizes())
        self.observation_space = spaces.Box(0, 255, (self.channels, self.img_h, self.img_w), dtype=np.uint8)
        self._obs_tensor = None
        self._host_obs = None
        self._dev_out = None
        self._seq = None   # step_sequence: ((k, render), obs ring or None, rewards ring, dones ring, actions) while its rings are attached
        self._frozen = np.zeros(self.num_envs, np.bool_)   # freeze / thaw: the envs this env keeps frozen through a host step mask

    STATE_OBS_FIELDS = STATE_OBS_FIELDS   # column name -> index of a state_obs() row (the table MegaverseGym shares)

    def state_obs(self):
        """the last tick's state observations: float32 (num_agents, 16) on the device, columns STATE_OBS_FIELDS -- a view of the attached buffer, valid in
        the order of the gym's stream until the next stepping call; no host wait.  After step_sequence: its last tick's rows (self.env.state_obs() has all k
        entries, entry j what tick j left).  Ask again after every call: when step_device or step_sequence swap the env's output rings, the buffer is
        detached and a NEW tensor of the new depth attached (_set_output_ring) -- a view held from before such a call is no longer written.  Needs
        MegaverseEnv(..., state_obs=True)."""
        return self._stream_entry("state", self.env.state_obs())

    SCENE_OBS_FIELDS = SCENE_OBS_FIELDS                     # column name -> index of a scene_obs() row, columns 0..15 (the tables MegaverseGym shares)
    SCENE_OBS_SCENARIO_FIELDS = SCENE_OBS_SCENARIO_FIELDS   # scenario name -> {column name: index}, columns 16..31

    def scene_obs(self):
        """the last tick's scene observations: float32 (num_envs, 32) on the device, columns SCENE_OBS_FIELDS and SCENE_OBS_SCENARIO_FIELDS[scenario] -- a view
        of the attached buffer, under state_obs()'s rules: ask again after every call.  Needs MegaverseEnv(..., scene_obs=True)."""
        return self._stream_entry("scene", self.env.scene_obs_ring())

    ENTITY_OBS_FIELDS = ENTITY_OBS_FIELDS   # column name -> index of an entity_obs() row

    def entity_obs(self):
        """the last tick's entity observations: float32 (num_envs, E, 8) on the device, columns ENTITY_OBS_FIELDS, rows megaverse_amd.entity_layout(scenario,
        num_agents_per_env) -- a view of the attached buffer, under state_obs()'s rules: ask again after every call.  Needs MegaverseEnv(..., entity_obs=True)."""
        return self._stream_entry("entity", self.env.entity_obs_ring())

    def depth_obs(self):
        """the last tick's depth planes: float32 or float16 (num_envs, num_agents_per_env, H, W) on the device -- planar camera depth in world units, 0 where a
        ray hits nothing, row 0 the bottom row -- a view of the attached buffer, under state_obs()'s rules: ask again after every call.  A tick that drew no
        frame wrote nothing.  Needs MegaverseEnv(..., depth_obs=True | "float16")."""
        return self._stream_entry("depth", self.env.depth_obs_ring(), per_agent_planes=True)

    def seg_obs(self):
        """the last tick's label planes: uint8 classes (megaverse_amd.SEG_CLASSES) or int16 words class << 12 | instance (megaverse_amd.seg_split),
        (num_envs, num_agents_per_env, H, W) on the device, 0 where a ray hits nothing, row 0 the bottom row -- a view of the attached buffer, under
        state_obs()'s rules: ask again after every call.  A tick that drew no frame wrote nothing.  Needs MegaverseEnv(..., seg_obs=True | "instance")."""
        return self._stream_entry("seg", self.env.seg_obs_ring(), per_agent_planes=True)

    def normal_obs(self):
        """the last tick's normal planes: float16 (x, y, z, 1) or int8 (b / 127; megaverse_amd.normals_to_float widens either), (num_envs,
        num_agents_per_env, H, W, 4) on the device -- unit surface normals in the viewer's camera frame, four zeros where a ray hits nothing, row 0 the
        bottom row -- a view of the attached buffer, under state_obs()'s rules: ask again after every call.  A tick that drew no frame wrote nothing.
        Needs MegaverseEnv(..., normal_obs=True | "int8")."""
        return self._stream_entry("normal", self.env.normal_obs_ring(), per_agent_planes=True)

    def _attach_stream(self, name, on=True):
        """one wanted stream's tensor attached (a new one, of the output ring's depth) or detached"""
        getattr(self.env, f"set_{name}_obs")(*((True,) + self._streams[name] if on else (None,)))

    def _stream_entry(self, name, buf, per_agent_planes=False):
        """the accessors' shared body: the last tick's entry of stream `name`'s attached tensor `buf` -- step_sequence's last tick, else entry 0;
        per_agent_planes: viewed as (num_envs, num_agents_per_env, H, W[, 4])"""
        if buf is None:
            raise RuntimeError(f"{name}_obs: create the env with {name}_obs=True")
        entry = buf[self._seq[0][0] - 1 if self._seq is not None else 0]
        return entry.view(self.num_envs, self.num_agents_per_env, *entry.shape[1:]) if per_agent_planes else entry

    def _set_output_ring(self, count, *ptrs):
        """the env's own output rings change (step_device, step_sequence): every attached stream's buffer is one more ring of the same depth and the library
        refuses a ring change while one is attached, so they are detached around the change and buffers of the new depth attached -- the planes first"""
        for name in self._streams:
            self._attach_stream(name, on=False)
        self.env.set_output_ring(count, *ptrs)
        for name in sorted(self._streams, key=lambda name: name not in ("depth", "seg", "normal")):
            self._attach_stream(name)

    @staticmethod
    def generate_action_space(action_space_sizes):
        return spaces.Tuple([spaces.Discrete(sz) for sz in action_space_sizes])

    def seed(self, seed=None):
        if seed is None:
            return
        assert isinstance(seed, int), 'Expect seed to be an integer'
        self.env.seed(seed)

    # ---- reference-shaped (list of per-agent numpy arrays) ----
    def observations(self):
        """list of (3, H, W) uint8, one per agent (megaverse_env.py:121-130)"""
        frames = self.observations_numpy()
        return [frames[i] for i in range(self.num_agents)]

    def observations_numpy(self):
        """(num_agents, 3, H, W) uint8 on the host: ONE D2H copy of the slab into a pinned buffer (the reference's getObservation is a view of host
        memory, megaverse.cpp:139-143, here the frames live in HBM).  obs_layout 'rgba': the RGBA slab, 4 bytes per pixel (PCIe: ~64 MB per step at
        1024 x 128 x 128), returned as a transposed view of it like the reference's np.transpose(obs[:, :, :3], (2, 0, 1)) (megaverse_env.py:121-130);
        'chw': the planes, 3 bytes per pixel (~48 MB), returned as they are.  Valid until the next call"""
        torch = self._torch()
        slab = self.observations_tensor(rgba=self.obs_layout == "rgba")   # (obs_layout 'chw': the planes themselves, 3 bytes per pixel)
        if self._host_obs is None:
            self._host_obs = torch.empty(slab.shape, dtype=torch.uint8, pin_memory=True)
        self._host_obs.copy_(slab, non_blocking=True)
        torch.cuda.current_stream(slab.device).synchronize()
        if self.obs_layout == "chw":
            return self._host_obs.numpy()
        return self._host_obs.numpy()[..., :3].transpose(0, 3, 1, 2)

    def reset(self):
        self.env.reset()
        return self.observations()

    def _held_actions(self, actions, who):
        """what a frame_skip > 1 step hands to macro_step: a CUDA tensor as int32 [num_agents, 6] (a converted copy where needed), anything else as numpy"""
        if actions is None:
            raise ValueError(f"{who}: with frame_skip > 1 the call holds its actions for the macro step: actions=None (keep what was set) has nothing to hold")
        if hasattr(actions, 'data_ptr'):
            torch = self._torch()
            return actions.to(dtype=torch.int32).contiguous().reshape(self.num_agents, 6)
        return np.asarray(actions, dtype=np.int32).reshape(self.num_agents, 6)

    def step(self, actions):
        self._leave_sequence()
        if self.frame_skip > 1:
            self.env.macro_step(self.frame_skip, self._held_actions(actions, 'step'), render="last")
        else:
            self.env.set_actions_batched(np.asarray(actions, dtype=np.int32).reshape(self.num_agents, -1))
            self.env.step()
        dones_env = self.env.get_dones().astype(bool)
        A = self.num_agents_per_env
        dones = np.repeat(dones_env, A).tolist()          # (megaverse_env.py:149-150: the env's done, once per agent)
        infos = [{} for _ in range(self.num_agents)]
        if dones_env.any():                                # true_reward of the agents whose episode just ended (megaverse_env.py:152-156)
            true_obj = self.env.get_true_objectives()
            for env_i in np.nonzero(dones_env)[0]:
                for j in range(A):
                    infos[env_i * A + j] = dict(true_reward=float(true_obj[env_i * A + j]))
        rewards = self.env.get_last_rewards()
        return self.observations(), rewards, dones, infos

    # ---- batched device path ----
    def _torch(self):
        import torch
        return torch

    def observations_tensor(self, rgba=False):
        """uint8 CUDA tensor viewing the HBM observation slab written by the raster kernel:
        (num_agents, 3, H, W) (a permuted view, no copy; obs_layout 'chw': the contiguous slab itself) or (num_agents, H, W, 4) if rgba
        (obs_layout 'rgba' only: a 'chw' slab has no alpha to hand out -- ValueError)."""
        torch = self._torch()
        if rgba and self.obs_layout == "chw":
            raise ValueError("observations_tensor(rgba=True): this env writes its frames as (3, H, W) planes (obs_layout='chw')")
        self._leave_sequence()
        if self._obs_tensor is None:
            shape = (self.num_agents, 3, self.img_h, self.img_w) if self.obs_layout == "chw" else (self.num_agents, self.img_h, self.img_w, 4)
            self._obs_tensor = torch.empty(shape, dtype=torch.uint8, device=f'cuda:{self.device}')
            self.env.set_obs_buffer(self._obs_tensor.data_ptr())
            self.env.render()
        self.env.synchronize()
        return self._obs_view() if not rgba else self._obs_tensor

    def _obs_view(self):
        """the slab as (num_agents, 3, H, W)"""
        if self.obs_layout == "chw":
            return self._obs_tensor
        return self._obs_tensor[..., :3].permute(0, 3, 1, 2)

    def step_batched(self, actions=None):
        """actions: int32 [num_agents, 6] (numpy, or a CUDA torch tensor) or None (keep what was set).
        Returns (obs uint8 CUDA view (num_agents,3,H,W), rewards float32 np [num_agents], dones bool np [num_envs])."""
        self._leave_sequence()
        if self._obs_tensor is None:
            self.observations_tensor()   # (allocates: before the action buffer is handed over, not between hand-over and step)
        if self.frame_skip > 1:
            self.env.macro_step(self.frame_skip, self._held_actions(actions, 'step_batched'), render="last")
            return self.observations_tensor(), self.env.get_rewards_array(), self.env.get_dones().astype(bool)
        held = None
        if actions is not None:
            if hasattr(actions, 'data_ptr'):
                # Lifetime rule of mv_set_actions_device: the buffer is READ BY THE NEXT STEP KERNEL, in the order of the gym's stream -- it must stay
                # alive and unchanged until that step has been enqueued (a reset or a host-side action setter in between reads it at once instead).
                # int32, contiguous, [num_agents, 6]; `held` keeps a converted copy alive until step() has returned (the caching allocator does not
                # hand its memory to anyone on another stream before the stream's work is done).
                import torch
                held = actions.to(dtype=torch.int32).contiguous()
                self.env.set_actions_device(held.data_ptr())
            else:
                self.env.set_actions_batched(actions)
        self.env.step()
        del held
        return self.observations_tensor(), self.env.get_rewards_array(), self.env.get_dones().astype(bool)

    def step_device(self, actions=None):
        """step_batched without a host synchronisation: (obs uint8 (num_agents, 3, H, W), rewards float32 [num_agents], dones uint8 [num_envs]), all three
        CUDA tensors the step writes into (mv_set_output_ring with one entry), valid in the order of the gym's stream -- torch's current stream when the
        env's first observation was asked for -- until the next step.  What a learner whose policy runs on the device wants (the reference has no
        counterpart: its outputs are host arrays, megaverse_env.py:121-162); `infos` / true rewards stay available through env.get_true_objectives()."""
        torch = self._torch()
        if self._obs_tensor is None:
            self.observations_tensor()
        self._leave_sequence()
        if self._dev_out is None:
            dev = self._obs_tensor.device
            self._dev_out = (torch.zeros(self.num_agents, dtype=torch.float32, device=dev), torch.zeros(self.num_envs, dtype=torch.uint8, device=dev))
            self._set_output_ring(1, self._obs_tensor.data_ptr(), self._dev_out[0].data_ptr(), self._dev_out[1].data_ptr())
        if self.frame_skip > 1:
            self.env.macro_step(self.frame_skip, self._held_actions(actions, 'step_device'), render="last")   # (the gym holds the tensors it reads)
            return self._obs_view(), self._dev_out[0], self._dev_out[1]
        held = None
        if actions is not None:
            if hasattr(actions, 'data_ptr'):   # (the lifetime rule of step_batched)
                held = actions.to(dtype=torch.int32).contiguous()
                self.env.set_actions_device(held.data_ptr())
            else:
                self.env.set_actions_batched(actions)
        self.env.step()
        del held
        return self._obs_view(), self._dev_out[0], self._dev_out[1]

    def macro_step(self, actions, k=None, ticks=None, render="last"):
        """One decision held for up to k ticks (default: this env's frame_skip) -- MegaverseGym.macro_step with step_device's outputs and no host
        synchronisation: (obs uint8 (num_agents, 3, H, W), rewards float32 [num_agents], dones uint8 [num_envs]), CUDA tensors valid in the order of the gym's
        stream until the next step.  Every env stops at its own first done; rewards are the call's sums (fp32, in tick order), dones the ORs, obs the frame
        behind the call's last tick (render='none': obs is what it was).  ticks: None, or int32 [num_envs] -- env e holds its action for min(ticks[e], k)
        ticks, 0: it does not step (options, dynamic frame skip, "wait d ticks"); a CUDA tensor of actions takes a CUDA tensor of ticks, a host array a host
        array."""
        torch = self._torch()
        if self._obs_tensor is None:
            self.observations_tensor()
        self._leave_sequence()
        if self._dev_out is None:
            dev = self._obs_tensor.device
            self._dev_out = (torch.zeros(self.num_agents, dtype=torch.float32, device=dev), torch.zeros(self.num_envs, dtype=torch.uint8, device=dev))
            self._set_output_ring(1, self._obs_tensor.data_ptr(), self._dev_out[0].data_ptr(), self._dev_out[1].data_ptr())
        if ticks is not None and hasattr(ticks, 'data_ptr'):
            ticks = ticks.to(dtype=torch.int32).contiguous()
        elif ticks is not None:
            ticks = np.asarray(ticks, dtype=np.int32).reshape(self.num_envs)
        self.env.macro_step(self.frame_skip if k is None else int(k), self._held_actions(actions, 'macro_step'), ticks=ticks, render=render)
        return self._obs_view(), self._dev_out[0], self._dev_out[1]

    def fork(self, src_env, dst_envs=None):
        """env src_env's running episode continues in every env of dst_envs as well (default: in all others) -- MegaverseGym.fork_envs with the map built
        here: N candidate plans branch from one situation, then step_sequence plays them.  The destinations keep their own next episodes.  Outputs are
        untouched: they still describe the last stepped tick."""
        src_env = int(src_env)
        if not 0 <= src_env < self.num_envs:
            raise ValueError(f'fork: src_env must be within 0 .. {self.num_envs - 1}, got {src_env}')
        m = np.full(self.num_envs, -1, np.int32)
        if dst_envs is None:
            m[:] = src_env
        else:
            d = np.asarray(list(dst_envs), dtype=np.int64).reshape(-1)
            if d.size and (d.min() < 0 or d.max() >= self.num_envs):
                raise ValueError(f'fork: dst_envs must be within 0 .. {self.num_envs - 1}')
            m[d] = src_env
        m[src_env] = -1
        self.env.fork_envs(m)

    def resample(self, src_of):
        """every env d continues from the state env src_of[d] had before the call (MegaverseGym.resample_envs): any map of num_envs entries -- chains,
        swaps, cycles, sources that are overwritten themselves; -1 or d leaves env d alone.  The resampling step of a population method: a CUDA int32
        tensor (the output of torch.multinomial, cast) is applied without a host synchronisation.  Envs keep their own next episodes; outputs are untouched."""
        self.env.resample_envs(src_of)

    def swap(self, a, b):
        """envs a and b exchange their running episodes (resample with the two-entry map); each keeps its own next episodes"""
        a, b = int(a), int(b)
        if not (0 <= a < self.num_envs and 0 <= b < self.num_envs):
            raise ValueError(f'swap: envs must be within 0 .. {self.num_envs - 1}, got {a}, {b}')
        m = np.full(self.num_envs, -1, np.int32)
        m[a], m[b] = b, a
        self.env.resample_envs(m)

    def _store_map(self, who, env_ids, slots):
        ids = self._env_ids(env_ids, who)
        if len(set(ids.tolist())) != ids.size:
            raise ValueError(f'{who}: env_ids names an env twice')
        sl = ids if slots is None else np.asarray(list(slots), dtype=np.int64).reshape(-1)
        if sl.shape != ids.shape:
            raise ValueError(f'{who}: slots must name one record per env of env_ids')
        m = np.full(self.num_envs, -1, np.int32)
        m[ids] = sl
        return m

    def new_store(self, slots):
        """a zeroed env store of `slots` records (MegaverseGym.new_env_store): a torch.uint8 CUDA tensor the caller owns"""
        return self.env.new_env_store(slots)

    def save(self, env_ids, store, slots=None):
        """the running episodes of the envs of env_ids are saved into the records `slots` of store (default: record e for env e) -- MegaverseGym.save_envs
        with the map built here.  A savepoint that costs no live env: a search keeps as many states as the store has records.  The gym is unchanged."""
        self.env.save_envs(self._store_map('save', env_ids, slots), store)

    def load(self, env_ids, store, slots=None):
        """the envs of env_ids leave their running episodes and continue the records `slots` of store (default: record e for env e) -- MegaverseGym.load_envs
        with the map built here.  The envs keep their own next episodes; outputs are untouched: they still describe the last stepped tick."""
        self.env.load_envs(self._store_map('load', env_ids, slots), store)

    def reset_envs(self, env_ids, render=True):
        """the envs of env_ids abandon their running episode and start the next one of their own sequence (MegaverseGym.reset_envs with the mask built
        here); the others are untouched.  What a learner's own time limit, a curriculum, or a planner handing its fork destinations back needs.  With render
        the observations of those envs are redrawn where step_device / step_batched leave observations; rewards and dones of the reset envs read zero."""
        ids = np.asarray(list(env_ids), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.num_envs):
            raise ValueError(f'reset_envs: env_ids must be within 0 .. {self.num_envs - 1}')
        m = np.zeros(self.num_envs, np.bool_)
        m[ids] = True
        self.env.reset_envs(m, render)

    def _seed_words(self, env_ids, seeds, who):
        ids = np.asarray(list(env_ids), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.num_envs):
            raise ValueError(f'{who}: env_ids must be within 0 .. {self.num_envs - 1}')
        if isinstance(seeds, (int, np.integer)) and not isinstance(seeds, (bool, np.bool_)):
            seeds = [int(seeds)] * ids.size
        vals = np.asarray(list(seeds)).reshape(-1)
        if vals.shape != ids.shape or (vals.size and vals.dtype.kind not in 'iu') or (vals.size and (vals.min() < 0 or vals.max() >= 2 ** 31)):
            raise ValueError(f'{who}: seeds must be one non-negative int32 per env of env_ids (or one int for all of them)')
        return {int(e): int(v) for e, v in zip(ids, vals)}, ids

    def seed_envs(self, env_ids, seeds):
        """the envs of env_ids restart their level stream from seeds (one per env, or one int for all of them) -- MegaverseGym.seed_envs with the words
        built here.  Their running episodes go on; their next reset plays the first level of the new stream.  An env named twice takes its last seed."""
        words, _ = self._seed_words(env_ids, seeds, 'seed_envs')
        self.env.seed_envs(words)

    def start_levels(self, env_ids, seeds, render=True):
        """the envs of env_ids start level seeds[k] NOW: seed_envs, then reset_envs on the same envs.  Two envs given the same seed play the same level
        sequence; calling this again with the same seeds replays the levels.  What level replay, a held-out level set and "every candidate gets the same
        fresh level" need.  With render the observations of those envs are redrawn; their rewards and dones read zero."""
        words, ids = self._seed_words(env_ids, seeds, 'start_levels')
        self.env.seed_envs(words)
        m = np.zeros(self.num_envs, np.bool_)
        m[ids] = True
        self.env.reset_envs(m, render)

    def set_step_mask(self, mask):
        """Step masks (MegaverseGym.set_step_mask): mask[e] true: env e steps; false: env e is frozen -- step, step_batched, step_device and step_sequence
        leave its state alone, report reward 0 and done 0 for it and discard its actions, and its observation stays its current view -- until the mask is
        replaced or detached (None).  A bool / uint8 CUDA tensor is read in place (rewrite it, then call this again); a numpy array or a sequence is copied.
        freeze / thaw keep a mask of their own: a mask set here replaces it."""
        self.env.set_step_mask(mask)
        self._frozen[:] = False

    def _env_ids(self, env_ids, who):
        ids = np.asarray(list(env_ids), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.num_envs):
            raise ValueError(f'{who}: env_ids must be within 0 .. {self.num_envs - 1}')
        return ids

    def freeze(self, env_ids):
        """the envs of env_ids stand still from the next tick on (a host step mask this env keeps): savepoints to fork from, envs whose evaluation episode
        is over, envs whose action is not ready.  Envs frozen earlier stay frozen."""
        self._frozen[self._env_ids(env_ids, 'freeze')] = True
        self.env.set_step_mask(~self._frozen)

    def thaw(self, env_ids=None):
        """the envs of env_ids (default: all) step again; with none left frozen the mask is detached"""
        if env_ids is None:
            self._frozen[:] = False
        else:
            self._frozen[self._env_ids(env_ids, 'thaw')] = False
        self.env.set_step_mask(~self._frozen if self._frozen.any() else None)

    def set_draw_mask(self, mask):
        """Draw masks (MegaverseGym.set_draw_mask): mask[e] true: env e is drawn as always; false: its frames are neither set up nor drawn and its rows in the
        observation slab or ring keep what they held -- everything else about its ticks is unchanged -- until the mask is replaced or detached (None).  A bool
        / uint8 CUDA tensor is read in place (rewrite it, then call this again); a numpy array or a sequence is copied."""
        self.env.set_draw_mask(mask)

    def set_still_frames(self, on=True):
        """Still frames (MegaverseGym.set_still_frames): while on, envs whose state did not change since their frames were drawn last -- frozen (freeze),
        halted by a budget, stopped inside a macro step -- are not drawn again; their observations stay byte for byte what drawing them would leave.  No
        host wait."""
        self.env.set_still_frames(on)

    def draw_only(self, env_ids):
        """only the envs of env_ids are drawn from the next observation pass on (a host draw mask): the leaves a search feeds to its value net, the few envs
        whose video is recorded"""
        m = np.zeros(self.num_envs, np.bool_)
        m[self._env_ids(env_ids, 'draw_only')] = True
        self.env.set_draw_mask(m)

    def draw_all(self):
        """every env is drawn again: the draw mask is detached"""
        self.env.set_draw_mask(None)

    def set_episode_budget(self, budget):
        """Episode budgets (MegaverseGym.set_episode_budget): env e may finish budget[e] more episodes (an int: every env that many; < 0: unlimited) and then
        halts on the device, frozen on the first frame of its next episode -- inside a batched call too; None detaches.  Setting it again replaces every
        value: the halted envs resume."""
        self.env.set_episode_budget(budget)

    def device_generator(self):
        """are this env's episodes drawn on the device (MegaverseGym.device_generator)?"""
        return self.env.device_generator()

    def halted(self):
        """bool CUDA tensor [num_envs]: the envs whose budget is spent (episode_budget() == 0), in the order of the gym's stream"""
        self._torch()
        return self.env.episode_budget() == 0

    def run_episodes(self, episodes=1, policy="random", render="none", max_ticks=None, actions=None, seed=0):
        """Every env runs exactly `episodes` episodes and stops where its last one ends -- the unbiased evaluation protocol, as batched calls: the episode log
        is switched on if it is off, the budget attached, and calls of recommended_ticks_per_call() ticks follow until every env has halted (the halted count
        is read once per call, not per tick) or max_ticks ticks have been stepped.  policy: 'random' (the device-side multi-discrete policy, `seed`) or
        'sequence' (actions: [count, num_agents, 6], replayed modulo count, as step_sequence takes them).  render: 'none' | 'last' | 'every'
        (MegaverseGym.step_n).  -> the drained records (EPISODE_RECORD_DTYPE): episodes x num_envs x agents of them when nobody ran out of ticks -- in
        front of them whatever a log that was already on still held: drain it first where that matters.  The
        budget stays attached and every env halted: set_episode_budget resumes or detaches."""
        if policy not in ("random", "sequence"):
            raise ValueError("run_episodes: policy is 'random' or 'sequence'")
        if int(episodes) < 1:
            raise ValueError("run_episodes: episodes >= 1")
        render_mode_of(render)
        self._leave_sequence()
        if self._obs_tensor is None:
            self.observations_tensor()
        held = None
        if policy == "sequence":
            if actions is None:
                raise ValueError("run_episodes: policy='sequence' replays `actions` [count, num_agents, 6]")
            count = check_sequence_actions(actions, self.num_agents)
            torch = self._torch()
            held = actions.contiguous() if hasattr(actions, 'data_ptr') else \
                torch.as_tensor(np.ascontiguousarray(actions, dtype=np.int32)).to(torch.device(f'cuda:{self.device}'))
            self.env.set_action_ring(count, held.data_ptr())
        if self.env.episode_log_capacity() <= 0:
            self.env.set_episode_log(int(episodes) * self.num_envs * self.num_agents_per_env)
        self.env.set_episode_budget(int(episodes))
        chunk, tick = max(1, self.env.recommended_ticks_per_call()), 0
        while max_ticks is None or tick < int(max_ticks):
            k = chunk if max_ticks is None else min(chunk, int(max_ticks) - tick)
            self.env.step_n(k, 'sequence' if policy == "sequence" else 'multidiscrete', seed, tick, render=render)
            tick += k
            if self.env.halted_count() == self.num_envs:
                break
        records = self.env.drain_episode_log()
        if held is not None:
            self.env.set_action_ring(0)
        del held
        return records

    def _leave_sequence(self):
        """step_sequence's rings are attached: back to the single slab and arrays, the slab brought up to date"""
        if self._seq is None:
            return
        self._seq = None
        self._dev_out = None
        self._set_output_ring(0)
        self.env.set_action_ring(0)
        self.env.render()

    def step_sequence(self, actions, render="every"):
        """k ticks on GIVEN actions as batched calls (mv_set_action_ring + mv_step_n with MV_POLICY_SEQUENCE): replaying a recorded trajectory, a scripted
        test, an open-loop plan, action repeat.  actions: [k, num_agents, 6] -- an integer numpy array, or an int32 CUDA tensor (read in place: unchanged until
        the stream has passed this call).  -> (obs uint8 [k, num_agents, 3, H, W], rewards float32 [k, num_agents], dones uint8 [k, num_envs]): CUDA tensors,
        entry j what tick j left, valid in the order of the gym's stream until the next stepping call (rings this env owns, as step_device's outputs).  k
        may exceed what one call holds: it is stepped in chunks of recommended_ticks_per_call().  No host synchronisation.
        render (mv_step_n_render): 'every' as above; 'last': only the last tick is drawn, obs is [1, num_agents, 3, H, W] (a one-entry ring: nothing is
        allocated for the ticks that are not drawn); 'none': nothing is drawn, obs is None and no observation ring exists.  Rewards and dones are the full
        [k, ...] in every mode."""
        mode = render_mode_of(render)
        k = check_sequence_actions(actions, self.num_agents)
        torch = self._torch()
        dev = torch.device(f'cuda:{self.device}')
        if hasattr(actions, 'data_ptr'):
            held = actions.contiguous()
        else:
            held = torch.as_tensor(np.ascontiguousarray(actions, dtype=np.int32)).to(dev)
        if self._seq is None or self._seq[0] != (k, render):
            if self._obs_tensor is None:
                self.observations_tensor()   # (the env's own slab exists before the rings take its place)
            rings = (torch.zeros((k, self.num_agents), dtype=torch.float32, device=dev), torch.zeros((k, self.num_envs), dtype=torch.uint8, device=dev))
            self._dev_out = None   # (step_device attaches its own one-entry ring again)
            # tick j of a call -> entry j: every call is k ticks
            if render == "every":
                frame = (3, self.img_h, self.img_w) if self.obs_layout == 'chw' else (self.img_h, self.img_w, 4)
                rings = (torch.zeros((k, self.num_agents) + frame, dtype=torch.uint8, device=dev),) + rings
                self._set_output_ring(k, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
            else:   # ('last': the one drawn tick goes to the env's own slab -- a NULL ring keeps that output where it was)
                rings = (None,) + rings
                self._set_output_ring(k, 0, rings[1].data_ptr(), rings[2].data_ptr())
        else:
            rings = self._seq[1:4]
        self._seq = ((k, render),) + tuple(rings) + (held,)   # (the actions stay alive until the next call replaces them)
        self.env.set_action_ring(k, held.data_ptr())
        chunk = max(1, self.env.recommended_ticks_per_call())
        if render == "every":
            for done in range(0, k, chunk):
                self.env.step_n(min(chunk, k - done), 'sequence', 0, done)
        else:   # (one call: which tick is the last is the call's to know; the library splits it)
            self.env.step_n(k, 'sequence', 0, 0, render=render)
        if mode == 2:
            return None, rings[1], rings[2]
        if mode == 1:
            slab = self._obs_tensor.view((1, self.num_agents) + tuple(self._obs_tensor.shape[1:]))
            return (slab if self.obs_layout == 'chw' else slab[..., :3].permute(0, 1, 4, 2, 3)), rings[1], rings[2]
        obs = rings[0] if self.obs_layout == 'chw' else rings[0][..., :3].permute(0, 1, 4, 2, 3)
        return obs, rings[1], rings[2]

    # ---- rendering (megaverse_env.py:164-184): returns the tiled BGR image, shows it if cv2 exists ----
    def convert_obs(self, obs):
        if not self.use_vulkan:
            obs = obs[::-1]
        return np.ascontiguousarray(obs[:, :, [2, 1, 0]])

    def render(self, mode='human'):
        self.env.draw_overview()
        self.env.draw_hires()
        rows = []
        for env_i in range(self.num_envs):
            obs = [self.convert_obs(self.env.get_hires_observation(env_i, i)) for i in range(self.num_agents_per_env)]
            rows.append(np.concatenate(obs, axis=1))
        obs_final = np.concatenate(rows, axis=0)
        if mode == 'human':
            try:
                import cv2  # type: ignore
                cv2.imshow(f'agent_{id(self)}', obs_final)
                cv2.waitKey(1)
            except Exception:  # noqa: BLE001 - headless image
                pass
        return obs_final

    def overview_obs(self):
        """-> torch.uint8 [num_envs, h, w, 4] (RGBA, row 0 the bottom row): the frames the last render_overview() drew, valid in the order of the gym's stream;
        None without overview=(w, h)"""
        return self.env.overview_obs()

    def set_overview_cameras(self, cams):
        """one camera per env: records built with megaverse_amd.look_at / follow / overview_default_camera, a CUDA tensor of them, or None for the default
        pose (MegaverseGym.set_overview_cameras)"""
        self.env.set_overview_cameras(cams)

    def render_overview(self, mode='rgb_array'):
        """draws every env from its overview camera and returns the envs' frames tiled side by side as one BGR image, top row first -- the way render() tiles
        the agents' hires frames; mode 'human' shows it if cv2 exists.  render() itself is unchanged."""
        if self.env.overview_obs() is None:
            raise RuntimeError("render_overview: construct the env with overview=(w, h)")
        self.env.draw_overview()
        obs_final = np.concatenate([self.convert_obs(self.env.get_overview_observation(env_i)) for env_i in range(self.num_envs)], axis=1)
        if mode == 'human':
            try:
                import cv2  # type: ignore
                cv2.imshow(f'overview_{id(self)}', obs_final)
                cv2.waitKey(1)
            except Exception:  # noqa: BLE001 - headless image
                pass
        return obs_final

    def get_default_reward_shaping(self):
        return self.default_shaping_scheme

    def get_current_reward_shaping(self, actor_idx: int):
        return self.env.get_reward_shaping(actor_idx // self.num_agents_per_env, actor_idx % self.num_agents_per_env)

    def set_reward_shaping(self, reward_shaping: dict, actor_idx: int):
        return self.env.set_reward_shaping(actor_idx // self.num_agents_per_env, actor_idx % self.num_agents_per_env, reward_shaping)

    def close(self):
        if self.env:
            self.env.close()
