"""An independent model of Rearrange's rules: one function judges one tick of one env.  TEST INFRASTRUCTURE ONLY.

Written from the reference's rules, not from the kernel (megaverse_amd/csrc/mv_tick_rearrange.h) or the oracle (oracle/mv_oracle.cpp) (reference paths
relative to src/libs):
    ObjectStackingComponent::step / onInteractAction        scenarios/include/scenarios/component_object_stacking.hpp:45-168  (tests/tower_model.py: interact)
    RearrangeScenario::canPlaceObject                       scenarios/src/scenario_rearrange.cpp:131-135
    RearrangeScenario::countMatchingObjects                 :137-151   (a carried item never counts; a match needs shape, colour and the offset from rightCenter)
    placedObject / pickedObject / checkDone                 :153-179   (both callbacks call checkDone)
    leftCenter (5, 2, 5), rightCenter (13, 2, 5)            scenarios/include/scenarios/scenario_rearrange.hpp:130-131
    trueObjective == solved                                 scenario_rearrange.hpp:95
    Scenario::rewardAgent / rewardTeam / doneWithTimer      env/include/env/scenario.hpp:259-298, :114-117
    Env::step: scenario->step(), then currEpisodeSec += dt, then done                                                         env/src/env.cpp:131-138

The solid cells are stated here from the reference, not read from the record:
    the room: RearrangePlatform is 19 long (x), 14 wide (z), H = randRange(4, 7) high, with all four walls   scenario_rearrange.cpp:21-26, :54-56
    its floor {0, 0, 0, L, 1, W} and walls {0, 0, 0, 1, H, W}, {L - 1, 0, 0, L, H, W}, {0, 0, 0, L, H, 1}, {0, 0, W - 1, L, H, W}  platforms.hpp:167-190
    every voxel of those boxes is solid (VoxelGridComponent::addPlatform)                                     component_voxel_grid.hpp:73-92
    the layer y = 1 within +-3 (x and z) of both centres is solid                                             scenario_rearrange.cpp:271-277
    the left arrangement's items are not in the grid (interactive == false)                                   :255-261
A State compares this statement with the record's chunk where the record holds one (the oracle's does).  One documented deviation of this build is part of the model: the grid is a
32 x 16 x 32 chunk, a placement outside it in x / z / +y is refused (tower_model.interact).

The timer is taken from the record in fp32, it is discrete: a solving tick sets episode_sec = max(episode_sec, episode_len - 0.3f) before the tick's
+ dt, dt = 1 / 15 (float); the episode is done when episode_sec >= episode_len.

Rules (E), (R), (U) are tests/tower_model.py's, applied by tests/rule_judge.py: the interact point and the poses are TowerBuilding's, so FRAGILE and its
derivation hold here unchanged; a reward here is a sum of at most 2 A products of shaping weights, the bound `Reward` carries is a few ulp of it."""
import functools

import numpy as np

import tower_model as T

CX, CY, CZ = T.CX, T.CY, T.CZ
L, W = 19, 14
LEFT, RIGHT = (5, 2, 5), (13, 2, 5)
K_SPIRIT, K_ONE_MORE, K_ALL = 0, 1, 2       # the scenario's reward-shaping table in the snapshot's order
DT = np.float32(1.0 / 15.0)
REMAINING = np.float32(0.3)                 # doneWithTimer's default
ACT_INTERACT = T.ACT_INTERACT


class Rules:
    """the reference's rules; every field is one planted mistake of the rejection demo when changed (tests/test_rearrange_model.py)"""
    carried_counts = False         # a carried item counts as matching
    match_colour = True
    match_y = True
    high_water = True              # maxMatchingObjects only grows
    one_more_with_bonus = True     # the solving placement pays the +1 as well
    reach = 2                      # canPlaceObject: |dx| <= 2 and |dz| <= 2
    clamp = True                   # doneWithTimer
    team_divisor = None
    # tower_model.interact's own fields, at the reference's values
    lookup_limit, lookup_shift, covered_can_be_taken, descent = None, 0, False, "full"

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Rules, k), k
            setattr(self, k, v)


REFERENCE = Rules()

MISTAKES = {
    "a carried item counts as matching": dict(carried_counts=True),
    "a match ignores colour": dict(match_colour=False),
    "a match ignores the y offset": dict(match_y=False),
    "maxMatching is not a high-water mark": dict(high_water=False),
    "the solve bonus is paid without the +1": dict(one_more_with_bonus=False),
    "canPlace +-3": dict(reach=3),
    "no timer clamp": dict(clamp=False),
    "the team share is divided by 8": dict(team_divisor=8),
}


def solid(x, y, z, H):
    """the reference's solid voxels (module docstring)"""
    if not (0 <= x < L and 0 <= z < W):
        return False
    if y == 0:
        return True
    if 0 <= y < H and (x in (0, L - 1) or z in (0, W - 1)):
        return True
    return y == 1 and any(abs(x - c[0]) <= 3 and abs(z - c[2]) <= 3 for c in (LEFT, RIGHT))


@functools.lru_cache(maxsize=None)
def solid_chunk(H):
    """`solid` over the chunk, indexed [y, z, x] like the record's"""
    return np.array([[[solid(x, y, z, H) for x in range(CX)] for z in range(CZ)] for y in range(CY)], bool)


def has_chunk(snap):
    """the oracle's record holds the room as a dense chunk; the HIP gym keeps none for this scenario and reports zeros (tests/hip_util.py: diff_snapshots
    compares chunks for TowerBuilding only) -- the two chunk checks apply where there is one"""
    return bool(np.asarray(snap["chunk"]).any())


class State:
    """the record a tick starts from"""

    def __init__(self, snap, A, prev=None):
        self.A = A
        self.H = int(snap["H"])
        n = int(snap["num_items"])
        self.items = [(int(it[0]), int(it[1]), (int(it[2]), int(it[3]), int(it[4]))) for it in snap["items"][:n]]
        self.objects = [[int(v) for v in snap["objects"][i]] for i in range(int(snap["num_objects"]))]
        ag = snap["agents"]
        self.carrying = [int(ag[i]["carrying"]) for i in range(A)]
        self.shaping = [[float(v) for v in ag[i]["shaping"][:3]] for i in range(A)]
        self.max_matching = int(snap["num_platforms"])
        self.solved = int(snap["solved"])
        self.sec, self.len = np.float32(snap["episode_sec"]), np.float32(snap["episode_len"])
        self.complaints = []
        if (int(snap["L"]), int(snap["W"])) != (L, W) or len(self.objects) != n:
            self.complaints.append(f"the room is {int(snap['L'])} x {int(snap['W'])} with {len(self.objects)} objects for {n} items")
        got = (np.asarray(snap["chunk"]).reshape(CY, CZ, CX) & T.VX_SOLID) != 0
        if has_chunk(snap) and not np.array_equal(got, solid_chunk(self.H)):
            self.complaints.append(f"solid cells: {[(int(x), int(y), int(z)) for y, z, x in np.argwhere(got != solid_chunk(self.H))][:6]} differ from the reference's room")

    def is_solid(self, x, y, z):
        return solid(x, y, z, self.H)

    def object_cells(self):
        return sorted((o[0], o[1], o[2]) for o in self.objects if o[3] == 0)


def count_matching(st, rules):
    """countMatchingObjects, :137-151; object i is the movable copy of item i (arrangementDrawables, :223-261)"""
    n = 0
    for i, o in enumerate(st.objects):
        if o[3] != 0 and not rules.carried_counts:
            continue
        shape, colour, _ = st.items[i]
        off = (o[0] - RIGHT[0], o[1] - RIGHT[1], o[2] - RIGHT[2])
        for s, c, f in st.items:   # Arrangement::contains, scenario_rearrange.hpp:66-73
            if s == shape and (c == colour or not rules.match_colour) and (f == off if rules.match_y else (f[0], f[2]) == (off[0], off[2])):
                n += 1
                break
    return n


def ends_without_interaction(st):
    return np.float32(st.sec + DT) >= st.len


class Result:
    pass


def judge_tick(st, masks, poses, rules=None):
    """One tick of one env.  st: the State before the tick (changed in place into the state after it); masks [A]; poses [A]: the implementation's
    post-tick (pos, basis, pitch) -> Result"""
    rules = rules or REFERENCE
    A = st.A
    rewards = [T.Reward() for _ in range(A)]
    margins, events = [], []
    res = Result()
    res.solved_now = res.clamped = 0

    def check_done(agent, idx, voxel):   # :165-179
        matches = count_matching(st, rules)
        solving = matches >= len(st.items) and not st.solved
        if matches > st.max_matching and (rules.one_more_with_bonus or not solving):
            T.reward_team(st, rewards, K_ONE_MORE, agent, 1.0, 0.0, rules)
        st.max_matching = max(st.max_matching, matches) if rules.high_water else matches
        if solving:
            st.solved = 1
            res.solved_now = 1
            T.reward_team(st, rewards, K_ALL, agent, 1.0, 0.0, rules)
            events.append(("solve", agent, idx, voxel))
            if rules.clamp and st.len - REMAINING > st.sec:   # doneWithTimer, scenario.hpp:114-117
                st.sec = np.float32(st.len - REMAINING)
                res.clamped = 1

    def can_place(x, y, z):              # :131-135
        return abs(x - RIGHT[0]) <= rules.reach and abs(z - RIGHT[2]) <= rules.reach

    res.interact = 0
    for i in range(A):   # ObjectStackingComponent::step :45-52: agents act in index order
        if not (int(masks[i]) & ACT_INTERACT):
            continue
        res.interact += 1
        others = [T.agent_point(poses[j][0]) for j in range(A) if j != i]
        T.interact(st, i, poses[i], others, can_place, check_done, check_done, rules, margins, events)
    st.sec = np.float32(st.sec + DT)     # env.cpp:133
    res.done = bool(st.sec >= st.len)    # :137-138
    res.rewards, res.events = rewards, events
    res.margin = min(margins) if margins else float("inf")
    return res


def differences(st, snap, A):
    """the model's state after a tick against the implementation's record: the discrete outputs of rule (E)"""
    out = []
    n = int(snap["num_objects"])
    if n != len(st.objects):
        return [f"num_objects {n} vs the model's {len(st.objects)}"]
    for i in range(n):
        got = [int(v) for v in snap["objects"][i]]
        if got != st.objects[i] and not (got[3] == st.objects[i][3] != 0):   # (a carried item's coordinates mean nothing)
            out.append(f"object {i}: {got} vs the model's {st.objects[i]}")
    ag = snap["agents"]
    for i in range(A):
        if int(ag[i]["carrying"]) != st.carrying[i]:
            out.append(f"agent {i} carrying: {int(ag[i]['carrying'])} vs the model's {st.carrying[i]}")
    for name, want in (("num_platforms", st.max_matching), ("solved", st.solved)):
        if int(snap[name]) != want:
            out.append(f"{name}: {int(snap[name])} vs the model's {want}")
    if np.float32(snap["episode_sec"]).tobytes() != np.float32(st.sec).tobytes():
        out.append(f"episode_sec: {float(snap['episode_sec'])!r} vs the model's {float(st.sec)!r}")
    chunk = np.asarray(snap["chunk"]).reshape(CY, CZ, CX)
    got = sorted((int(x), int(y), int(z)) for y, z, x in np.argwhere((chunk & T.VX_OBJECT) != 0))
    if has_chunk(snap) and got != st.object_cells():
        out.append(f"object cells: {sorted(set(got) ^ set(st.object_cells()))[:6]} differ")
    return out
