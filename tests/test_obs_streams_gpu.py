"""GPU: what the five observation streams (state, scene, entity, depth, segmentation) share.  The library's refusal texts in full, as they read before the
streams were folded onto shared descriptors (literals); MegaverseEnv with all five on while step_sequence swaps the output rings twice, against a twin
MegaverseGym driven by hand."""
import numpy as np
import pytest
import torch

from megaverse_amd.extension import MV_DEPTH_F32, MV_SEG_INSTANCE_U16, MegaverseGym
from megaverse_amd.megaverse_env import MegaverseEnv

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

STREAMS = ("state", "scene", "entity", "depth", "seg")
N, A, W, H = 4, 1, 40, 24

RING = {
    "state": "mv_set_output_ring: state observations are attached (mv_set_state_obs), sized by the ring count they were attached under: "
             "detach the state observations first",
    "scene": "mv_set_output_ring: scene observations are attached (mv_set_scene_obs), sized by the ring count they were attached under: "
             "detach the scene observations first",
    "entity": "mv_set_output_ring: entity observations are attached (mv_set_entity_obs), sized by the ring count they were attached under: "
              "detach the entity observations first",
    "depth": "mv_set_output_ring: depth observations are attached (mv_set_depth_obs), sized by the ring count they were attached under: "
             "detach the depth observations first",
    "seg": "mv_set_output_ring: segmentation observations are attached (mv_set_seg_obs), sized by the ring count they were attached under: "
           "detach the segmentation observations first",
}
NOT_ATTACHED = {
    "state": "mv_get_state_observation: no state observations attached (mv_set_state_obs)",
    "scene": "mv_get_scene_observation: no scene observations attached (mv_set_scene_obs)",
    "entity": "mv_get_entity_observation: no entity observations attached (mv_set_entity_obs)",
    "depth": "mv_get_depth_observation: no depth observations attached (mv_set_depth_obs)",
    "seg": "mv_get_seg_observation: no segmentation observations attached (mv_set_seg_obs)",
}
OUT_OF_RANGE = {
    "state": "mv_get_state_observation: index out of range",
    "scene": "mv_get_scene_observation: index out of range",
    "entity": "mv_get_entity_observation: index out of range",
    "depth": "mv_get_depth_observation: index out of range",
    "seg": "mv_get_seg_observation: index out of range",
}
RESOLUTION = {
    "depth": "mv_set_render_resolution: depth observations are attached (mv_set_depth_obs), whose planes are of the observation size: "
             "detach the depth observations first",
    "seg": "mv_set_render_resolution: segmentation observations are attached (mv_set_seg_obs), whose planes are of the observation size: "
           "detach the segmentation observations first",
}
STILL_ON = {
    "depth": "mv_set_still_frames: depth observations are attached (mv_set_depth_obs), and a still frame's depth plane would not be carried: "
             "detach the depth observations first",
    "seg": "mv_set_still_frames: segmentation observations are attached (mv_set_seg_obs), and a still frame's label plane would not be carried: "
           "detach the segmentation observations first",
}
UNDER_STILL = {
    "depth": "mv_set_depth_obs: still frames are switched on (mv_set_still_frames), and a still frame's depth plane would not be carried: "
             "switch them off first",
    "seg": "mv_set_seg_obs: still frames are switched on (mv_set_still_frames), and a still frame's label plane would not be carried: "
           "switch them off first",
}
UNKNOWN_FORMAT = {
    "depth": "mv_set_depth_obs: unknown format (MV_DEPTH_F32, MV_DEPTH_F16)",
    "seg": "mv_set_seg_obs: unknown format (MV_SEG_CLASS_U8, MV_SEG_INSTANCE_U16)",
}
MISALIGNED = {
    "depth": "mv_set_depth_obs: the buffer must be 4-byte aligned",
    "seg": "mv_set_seg_obs: a MV_SEG_INSTANCE_U16 buffer must be 2-byte aligned",
}


def refusal(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    return str(e.value)


def attach(g, name, on=True):
    return getattr(g, f"set_{name}_obs")(True if on else None)


def read(g, name, env):
    return getattr(g, f"get_{name}_observation")(*((env, 0) if name in ("state", "depth", "seg") else (env,)))


def test_refusal_texts(hip):
    """every refusal an attached stream causes, and every reader's, character for character; with all five attached the ring refusal names the state stream"""
    g = MegaverseGym("TowerBuilding", W, H, N, A, 1, False, {})
    g.seed(1); g.reset()
    lib = g._lib
    ring = torch.zeros((2, N * A, H, W, 4), dtype=torch.uint8, device="cuda")
    bytes_ = torch.zeros(N * A * H * W * 4 + 16, dtype=torch.uint8, device="cuda")
    for name in STREAMS:
        assert refusal(read, g, name, 0) == NOT_ATTACHED[name]
        attach(g, name)
        assert refusal(g.set_output_ring, 2, ring.data_ptr()) == RING[name]
        assert refusal(read, g, name, N) == OUT_OF_RANGE[name] and refusal(read, g, name, -1) == OUT_OF_RANGE[name]
        if name in ("depth", "seg"):
            setter = getattr(lib, f"mv_set_{name}_obs")
            assert refusal(g.set_render_resolution, 64, 36) == RESOLUTION[name]
            assert refusal(g.set_still_frames, True) == STILL_ON[name]
            attach(g, name, on=False)
            assert setter(g._g, bytes_.data_ptr(), 5) == -1 and lib.mv_last_error().decode() == UNKNOWN_FORMAT[name]
            # (refused before the pointer is kept or read: one byte off a 256-byte aligned allocation)
            assert setter(g._g, bytes_.data_ptr() + 1, MV_DEPTH_F32 if name == "depth" else MV_SEG_INSTANCE_U16) == -1
            assert lib.mv_last_error().decode() == MISALIGNED[name]
            g.set_still_frames(True)
            assert refusal(attach, g, name) == UNDER_STILL[name]
            assert setter(g._g, bytes_.data_ptr(), 5) == -1 and lib.mv_last_error().decode() == UNKNOWN_FORMAT[name]   # (the format is looked at first)
            g.set_still_frames(False)
            assert getattr(lib, f"mv_get_{name}_obs")(g._g) == 0 and getattr(lib, f"mv_get_{name}_format")(g._g) == -1
        else:
            assert read(g, name, N - 1).dtype == np.float32
            attach(g, name, on=False)
        assert refusal(read, g, name, 0) == NOT_ATTACHED[name]
    g.set_output_ring(2, ring.data_ptr()); g.set_output_ring(0)   # (nothing attached: accepted)
    for name in reversed(STREAMS):
        attach(g, name)
    assert refusal(g.set_output_ring, 2, ring.data_ptr()) == RING["state"]
    assert refusal(g.set_render_resolution, 64, 36) == RESOLUTION["depth"] and refusal(g.set_still_frames, True) == STILL_ON["depth"]
    attach(g, "state", on=False)
    assert refusal(g.set_output_ring, 2, ring.data_ptr()) == RING["depth"]
    attach(g, "depth", on=False)
    assert refusal(g.set_output_ring, 2, ring.data_ptr()) == RING["seg"] and refusal(g.set_render_resolution, 64, 36) == RESOLUTION["seg"]
    attach(g, "seg", on=False)
    assert refusal(g.set_output_ring, 2, ring.data_ptr()) == RING["scene"]
    attach(g, "scene", on=False)
    assert refusal(g.set_output_ring, 2, ring.data_ptr()) == RING["entity"]
    g.close()


def rings_of(g):
    return {"state": g.state_obs(), "scene": g.scene_obs_ring(), "entity": g.entity_obs_ring(), "depth": g.depth_obs_ring(), "seg": g.seg_obs_ring()}


def raw(t):
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().numpy().tobytes()


def sequence_by_hand(g, held, actions):
    """what MegaverseEnv.step_sequence(actions) does to its gym when the ring depth changes, call for call: detach the five streams, swap the rings, attach
    depth, labels, state, scene, entity again, play the actions"""
    k = int(actions.shape[0])
    dev = torch.device("cuda:0")
    rings = (torch.zeros((k, N * 2, H, W, 4), dtype=torch.uint8, device=dev), torch.zeros((k, N * 2), dtype=torch.float32, device=dev),
             torch.zeros((k, N), dtype=torch.uint8, device=dev))
    acts = torch.as_tensor(np.ascontiguousarray(actions, dtype=np.int32)).to(dev)
    held.append((rings, acts))
    g.set_state_obs(None); g.set_scene_obs(None); g.set_entity_obs(None); g.set_depth_obs(None); g.set_seg_obs(None)
    g.set_output_ring(k, rings[0].data_ptr(), rings[1].data_ptr(), rings[2].data_ptr())
    g.set_depth_obs(True, "float32"); g.set_seg_obs(True, "instance"); g.set_state_obs(True); g.set_scene_obs(True); g.set_entity_obs(True)
    g.set_action_ring(k, acts.data_ptr())
    chunk = max(1, g.recommended_ticks_per_call())
    for done in range(0, k, chunk):
        g.step_n(min(chunk, k - done), "sequence", 0, done)
    return rings


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_env_swaps_rings_with_all_streams(hip, mode):
    """MegaverseEnv with all five streams: step_sequence swaps the output rings twice (3 ticks, then 2); after each swap every accessor hands out the last
    entry of a tensor of the new depth, the library reports every stream attached with the new entry count, and every row and plane of every tick equals
    those of a twin gym driven by hand"""
    env = MegaverseEnv("TowerBuilding", N, 2, img_w=W, img_h=H, state_obs=True, scene_obs=True, entity_obs=True, depth_obs=True, seg_obs="instance")
    twin = MegaverseGym("towerbuilding", W, H, N, 2, 1, False, {})
    twin.set_state_obs(True); twin.set_scene_obs(True); twin.set_entity_obs(True); twin.set_depth_obs(True, "float32"); twin.set_seg_obs(True, "instance")
    for g in (env.env, twin):
        g.set_pixel_mode(mode)
    env.seed(7); twin.seed(7)
    env.reset()
    twin.reset()
    slab = torch.empty((N * 2, H, W, 4), dtype=torch.uint8, device="cuda:0")
    twin.set_obs_buffer(slab.data_ptr()); twin.render()
    for name, a, b in ((n, rings_of(env.env)[n], rings_of(twin)[n]) for n in STREAMS):
        assert a.shape[0] == 1 and raw(a) == raw(b), name
    rng = np.random.default_rng(5)
    held = []
    for k in (3, 2):
        actions = rng.integers(0, [3, 3, 3, 2, 2, 3], size=(k, N * 2, 6)).astype(np.int32)
        obs, rewards, dones = env.step_sequence(actions)
        want = sequence_by_hand(twin, held, actions)
        assert raw(rewards) == raw(want[1]) and raw(dones) == raw(want[2])
        got, ref = rings_of(env.env), rings_of(twin)
        views = {"state": env.state_obs(), "scene": env.scene_obs(), "entity": env.entity_obs(), "depth": env.depth_obs(), "seg": env.seg_obs()}
        for name in STREAMS:
            assert getattr(env.env._lib, f"mv_get_{name}_obs")(env.env._g) == k, name
            assert got[name].shape == ref[name].shape and got[name].shape[0] == k and got[name].dtype == ref[name].dtype, name
            assert views[name].data_ptr() == got[name][k - 1].data_ptr() and views[name].numel() == got[name][k - 1].numel(), name
            assert raw(got[name]) == raw(ref[name]), name
        assert tuple(views["depth"].shape) == (N, 2, H, W) and tuple(views["seg"].shape) == (N, 2, H, W)
        assert np.frombuffer(raw(got["depth"]), np.float32).max() > 0 and np.frombuffer(raw(got["seg"]), np.uint16).max() > 0   # (something was drawn)
    env.close(); twin.close()
