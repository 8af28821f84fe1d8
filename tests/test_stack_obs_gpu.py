"""Stack observations on the GPU (include/megaverse_hip.h: mv_set_stack_obs): per agent the last S drawn frames, downsampled, grey or RGB, refilled with the
first frame of every new episode.  Every comparison is byte for byte: the kernel alone against integer numpy (stack_reference), and the gym's stacks against
the same reference folded over the gym's own frames and dones."""
import ctypes as C

import numpy as np
import pytest

import episode_log_util as U
import stack_reference as R
from megaverse_amd import MultiTaskGym
from megaverse_amd import extension as ext
from megaverse_amd.extension import MegaverseGym

pytestmark = pytest.mark.gpu

N, A = 4, 2


def cuda(x):
    import torch
    return torch.as_tensor(x).cuda()


@pytest.mark.parametrize("W,H", R.SIZES + ((128, 128),))
@pytest.mark.parametrize("factor", (1, 2, 4))
@pytest.mark.parametrize("fmt", tuple(R.FORMATS))
@pytest.mark.parametrize("chw", (False, True))
def test_kernel_equals_integer_numpy(chw, fmt, factor, W, H):
    """S 1, 2, 8; a shift and a refill; in place and into a second buffer; random and all-255 frames.  128 x 128: several items per lane; 40 x 24: the dword shift"""
    if R.refused(W, H, factor):
        with pytest.raises(ValueError, match="multiple of 4"):
            ext.debug_stack_device(cuda(R.frame_of(1, W, H, chw)), 4, factor, fmt)
        return
    for S in (1, 2, 8):
        for i, (clear, in_place, full) in enumerate(((0, False, False), (0, True, False), (1, False, False), (1, True, True), (0, True, True))):
            frame = R.frame_of(W + S + i, W, H, chw, full)
            prev = np.random.default_rng(i).integers(0, 256, (S, R.FORMATS[fmt], H // factor, W // factor), dtype=np.uint8)
            p = cuda(prev)
            got = ext.debug_stack_device(cuda(frame), S, factor, fmt, p, clear, out=p if in_place else None)
            assert np.array_equal(got.cpu().numpy(), R.stack(frame, prev, factor, fmt, clear)), (S, clear, in_place, full)
            assert in_place or np.array_equal(p.cpu().numpy(), prev)


@pytest.mark.parametrize("fmt,factor,chw", (("gray", 2, False), ("rgb", 1, True), ("gray", 4, True)))
def test_a_chain_in_place_and_through_two_entries(fmt, factor, chw):
    """five frames, the third the first of a new episode: one entry shifted in place and two entries taken in turn end in the folded reference's bytes"""
    import torch
    S, W, H = 4, 48, 24
    frames, clears = [R.frame_of(10 + i, W, H, chw) for i in range(5)], (0, 0, 1, 0, 0)
    start = np.random.default_rng(0).integers(0, 256, (S, R.FORMATS[fmt], H // factor, W // factor), dtype=np.uint8)
    want = R.fold(frames, clears, S, factor, fmt, start)
    one, two = cuda(start), [cuda(start), torch.zeros_like(cuda(start))]
    for i, (f, c) in enumerate(zip(frames, clears)):
        ext.debug_stack_device(cuda(f), S, factor, fmt, one, c, out=one)
        ext.debug_stack_device(cuda(f), S, factor, fmt, two[i % 2], c, out=two[(i + 1) % 2])
    assert np.array_equal(one.cpu().numpy(), want) and np.array_equal(two[1].cpu().numpy(), want)


def make_gym(scenario, mode, layout="rgba", ring=0, W=64, H=64, stack=(4, 2, "gray"), params=None, ticks=16):
    """a gym whose frames, rewards and dones go to tensors of ours (`ring` entries, or one), stacks attached (stack given), reset, with an action ring"""
    import torch
    U.boxoban_env()
    g = MegaverseGym(scenario, W, H, N, A, 1, False, params or {})
    if layout == "chw":
        g.set_obs_layout("chw")
    g.set_pixel_mode(mode)
    g.seed(42)
    shape = (N * A, 3, H, W) if layout == "chw" else (N * A, H, W, 4)
    g.frames = torch.zeros((max(1, ring),) + shape, dtype=torch.uint8, device="cuda:0")
    g.outs = [torch.zeros((max(1, ring), N * A), dtype=torch.float32, device="cuda:0"), torch.zeros((max(1, ring), N), dtype=torch.uint8, device="cuda:0")]
    sizes = np.asarray(g.action_space_sizes())
    g.actions = torch.as_tensor(np.random.default_rng(3).integers(0, sizes, (ticks, N * A, sizes.size)).astype(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    if ring:
        g.set_output_ring(ring, g.frames.data_ptr(), g.outs[0].data_ptr(), g.outs[1].data_ptr())
    else:
        g.set_obs_buffer(g.frames.data_ptr())
    buf = g.set_stack_obs(True, *stack) if stack else None
    g.reset()
    g.set_action_ring(ticks, g.actions.data_ptr())
    return g, buf


def host(g, *tensors):
    import torch
    g.synchronize()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def tick_of(g, ring, entry):
    """-> the frames [N*A, ...] and dones [N] the gym left in `entry`"""
    frames, dones = host(g, g.frames, g.outs[1])
    return frames[entry], (dones[entry] if ring else g.get_dones()) != 0


def folded(want, frames, clear, factor, fmt):
    return np.stack([R.stack(frames[f], want[f], factor, fmt, bool(clear[f // A])) for f in range(N * A)])


@pytest.mark.parametrize("layout", ("rgba", "chw"))
@pytest.mark.parametrize("ring", (0, 4))
@pytest.mark.parametrize("mode", ("exact", "fast"))
@pytest.mark.parametrize("scenario,params,W,H,stack", (("TowerBuilding", {"episodeLengthSec": -190.0}, 64, 64, (4, 2, "gray")), ("Football", {}, 80, 48, (3, 2, "rgb"))))
def test_gym_stacks_equal_the_reference_folded_over_the_gyms_own_frames(scenario, params, W, H, stack, mode, ring, layout):
    """after reset, after eight single ticks and after one step_n(4) batch, in every entry the batch wrote.  Without a ring the batch's frames are gone: a twin
    stepped tick by tick supplies them (and equals the gym's own frames on the single ticks)"""
    S, factor, fmt = stack
    g, buf = make_gym(scenario, mode, layout, ring, W, H, stack, params)
    assert tuple(buf.shape) == (max(1, ring), N * A) + ext.stack_shape(W, H, *stack) and g._lib.mv_get_stack_obs(g._g) == max(1, ring)
    shape = (C.c_int32 * 4)()
    assert g._lib.mv_stack_obs_shape(g._g, shape) == 0 and tuple(shape) == tuple(buf.shape[2:])
    twin = None if ring else make_gym(scenario, mode, layout, 0, W, H, None, params)[0]
    last = lambda: (max(1, g._ring_ticks) - 1) % max(1, ring)
    frames, _ = tick_of(g, ring, last())
    want = folded(np.zeros(tuple(buf.shape[1:]), np.uint8), frames, np.ones(N), factor, fmt)   # the reset's frame fills every plane-set
    assert np.array_equal(host(g, buf)[0][last()], want) and frames.any()
    dones = np.zeros(N, bool)
    for t in range(8):
        g.step_n(1, "sequence", 0, t)
        frames, done = tick_of(g, ring, last())
        if twin:
            twin.step_n(1, "sequence", 0, t)
            assert np.array_equal(tick_of(twin, 0, 0)[0], frames)
        want, dones = folded(want, frames, done, factor, fmt), dones | done
        assert np.array_equal(host(g, buf)[0][last()], want), t
    first = g._ring_ticks
    g.step_n(4, "sequence", 0, 8)
    for j in range(4):
        if twin:
            twin.step_n(1, "sequence", 0, 8 + j)
        frames, done = tick_of(g, ring, (first + j) % ring) if ring else tick_of(twin, 0, 0)
        want, dones = folded(want, frames, done, factor, fmt), dones | done
        assert ring == 0 or np.array_equal(host(g, buf)[0][(first + j) % ring], want), j
    assert np.array_equal(host(g, buf)[0][last()], want)
    assert dones.any() or scenario != "TowerBuilding"   # (its short episodes end on the way: stacks were refilled)
    assert np.array_equal(g.get_stack_observation(N - 1, A - 1), want[-1]) and np.array_equal(g.stack_obs().cpu().numpy(), want)
    for x in (g, twin):
        if x:
            x.close()


def test_a_done_inside_a_batched_call():
    """Rearrange, 65-tick episodes, no ring, nine step_n(8) calls: the done falls inside a truly batched call and is read from the tick's own slot"""
    params, stack = {"episodeLengthSec": 4.3}, (4, 2, "gray")
    g, buf = make_gym("Rearrange", "fast", stack=stack, params=params, ticks=72)
    twin = make_gym("Rearrange", "fast", stack=None, params=params, ticks=72)[0]
    want, dones = folded(np.zeros(tuple(buf.shape[1:]), np.uint8), tick_of(twin, 0, 0)[0], np.ones(N), 2, "gray"), np.zeros(N, bool)
    for t in range(72):
        twin.step_n(1, "sequence", 0, t)
        frames, done = tick_of(twin, 0, 0)
        want, dones = folded(want, frames, done, 2, "gray"), dones | done
    for c in range(9):
        g.step_n(8, "sequence", 0, 8 * c)
    assert dones.all() and np.array_equal(host(g, buf)[0][0], want)
    g.close(); twin.close()


def test_masked_resets_render_launch_counts_and_reattach():
    import torch
    g, buf = make_gym("TowerBuilding", "fast")
    bare = make_gym("TowerBuilding", "fast", stack=None)[0]
    before, bare_before = g.debug_launch_counts(), bare.debug_launch_counts()
    for x in (g, bare):
        x.step_n(4, "sequence", 0, 0)
        x.step_n(1, "sequence", 0, 4)
    after, bare_after = g.debug_launch_counts(), bare.debug_launch_counts()
    assert after[0] - before[0] == bare_after[0] - bare_before[0] and after[1] - before[1] == bare_after[1] - bare_before[1] + 5   # one launch per drawn tick
    assert np.array_equal(host(g, g.frames)[0], host(bare, bare.frames)[0]) and np.array_equal(g.get_rewards_array(), bare.get_rewards_array())
    was = host(g, buf)[0][0]
    assert (was[:, 0] != was[:, 3]).any()   # five ticks in: the plane-sets differ
    g.render()   # the newest plane-set imaged again from the same state: nothing shifts
    assert np.array_equal(host(g, buf)[0][0], was)
    mask = [0, 1, 0, 1]
    g.reset_envs(torch.tensor(mask, dtype=torch.uint8, device="cuda:0"))   # the flagged envs refill, the others shift
    want = folded(was, tick_of(g, 0, 0)[0], mask, 2, "gray")
    got = host(g, buf)[0][0]
    assert np.array_equal(got, want) and (got[A:2 * A, 0] == got[A:2 * A, 3]).all() and (got[:A, 0] != got[:A, 3]).any()
    g.set_stack_obs(None)
    assert g.stack_obs() is None and g._lib.mv_get_stack_obs(g._g) == 0
    g.step_n(1, "sequence", 0, 5)
    assert np.array_equal(host(g, buf)[0][0], want)   # detached: the tensor is no longer written
    buf = g.set_stack_obs(True, 2, 4, "rgb")   # another shape; reset fills it
    g.reset()
    assert np.array_equal(host(g, buf)[0][0], folded(np.zeros(tuple(buf.shape[1:]), np.uint8), tick_of(g, 0, 0)[0], np.ones(N), 4, "rgb"))
    g.close(); bare.close()


def test_refusals():
    import torch
    g, buf = make_gym("TowerBuilding", "fast", W=40, H=24)
    text = "stack observations are attached .mv_set_stack_obs."
    ring = torch.zeros((2, N * A, 24, 40, 4), dtype=torch.uint8, device="cuda:0")
    for name, call in (("mv_step_no_render", g.step_no_render), ("mv_step_n_render", lambda: g.step_n(2, "sequence", 0, 0, render="last")),
                       ("mv_step_n_render", lambda: g.step_n(2, "sequence", 0, 0, render="none")),
                       ("mv_macro_step", lambda: g.macro_step(2, torch.zeros((N * A, 6), dtype=torch.int32, device="cuda:0"))),
                       ("mv_reset_envs_host", lambda: g.reset_envs(np.ones(N, np.uint8), render=False)),
                       ("mv_set_draw_mask_host", lambda: g.set_draw_mask(np.ones(N, np.uint8))), ("mv_set_still_frames", lambda: g.set_still_frames(True)),
                       ("mv_set_output_ring", lambda: g.set_output_ring(2, ring.data_ptr())), ("mv_set_render_resolution", lambda: g.set_render_resolution(64, 36)),
                       ("mv_set_obs_layout", lambda: g.set_obs_layout("chw"))):
        with pytest.raises(RuntimeError, match=f"{name}.*{text}"):
            call()
    other = make_gym("TowerBuilding", "fast", W=40, H=24, stack=None)[0]
    handles, out, lib = (C.c_void_p * 2)(g._g.value, other._g.value), C.c_void_p(), g._lib
    assert lib.mv_group_create(handles, 2, C.byref(out)) == -1 and b"stack observations attached (mv_set_stack_obs)" in lib.mv_last_error()
    assert lib.mv_step_many(handles, 2, 1, 1, 0, 0) == -1 and b"stack observations attached (mv_set_stack_obs)" in lib.mv_last_error()
    g.draw_hires()   # ignores the option
    g.set_stack_obs(None)
    for bad, why in (((4, 4, "gray"), "multiple of 4"), ((9, 2, "gray"), "frames must lie"), ((4, 3, "gray"), "factor must be")):
        with pytest.raises(ValueError, match=why):
            g.set_stack_obs(True, *bad)
    assert lib.mv_set_stack_obs(g._g, C.c_void_p(buf.data_ptr()), 4, 4, 0) == -1 and b"multiple of 4" in lib.mv_last_error()
    assert lib.mv_set_stack_obs(g._g, C.c_void_p(buf.data_ptr() + 4), 4, 2, 0) == -1 and b"16-byte aligned" in lib.mv_last_error()
    g.set_draw_mask(np.ones(N, np.uint8))
    with pytest.raises(RuntimeError, match="mv_set_stack_obs.*a draw mask attached .mv_set_draw_mask."):
        g.set_stack_obs(True)
    g.close(); other.close()
    mt = MultiTaskGym(["ObstaclesEasy", "ObstaclesHard"], 40, 24, 2, 1)
    with pytest.raises(RuntimeError, match="set_stack_obs"):
        mt.set_stack_obs(True)
    mt.close()
