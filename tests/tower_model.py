"""An independent float64 model of TowerBuilding's stacking rules: one function judges one tick of one env.  TEST INFRASTRUCTURE ONLY.

Written from the reference's rules, not from the kernel (megaverse_amd/csrc/mv_tick_tower.h) or the oracle (oracle/mv_oracle.cpp), whose arithmetic is
one author's and shared (reference paths relative to src/libs):
    ObjectStackingComponent::step / onInteractAction   scenarios/include/scenarios/component_object_stacking.hpp:45-168
    TowerBuildingScenario::step and its callbacks      scenarios/src/scenario_tower_building.cpp:179-261
    Scenario::rewardAgent / rewardTeam                 env/include/env/scenario.hpp:259-298

What a tick is given: the PRE-tick record (objects, per-agent carrying / picked_up / visited_zone / shaping table, zone, highest_tower, the solid cells,
A), the tick's action masks and the POST-tick agent poses of the implementation under judgement.  The controller is judged elsewhere
(tests/physics_reference.py); interact runs after it and only a fall respawn moves an agent afterwards, so the post-tick pose is what interact saw.

Arithmetic: everything discrete is exact integer work on Python ints, the rest is float64.
    eye            = pos + (0, 0.05 + 0.41, 0)                          agent.cpp:33, :95
    interact point = eye + R(yaw, pitch) (0, -0.44, -1)  when picking   (the interact location, agent.cpp)
                   = eye + R(yaw, pitch) (0, -0.74, -1)  when placing   (the carried object hangs 0.3 below it, component_object_stacking.hpp:151)
    agent voxel    = floor(pos + (0, 0.05, 0))                          :79-80
R = the yaw basis of the record times the pitch rotation about the local X axis (agent.cpp:110-133).

The pick / place core (`interact`) takes the scenario's canPlaceObject as a function, so that the same component inside Obstacles, Collect and Rearrange
can be judged with another one later.

Two deviations of this build from the reference are part of the model because they are documented product behaviour: the voxel grid is a
32 x 16 x 32 chunk, a placement outside it in x / z / +y is refused; and TowerBuilding's zone has min.y == 1.

THE THREE RULES (tests/test_tower_model.py, tests/test_tower_model_gpu.py)

(E) exact.  Where the tick's margin -- the smallest distance of any point the tick floored to a voxel boundary -- is >= FRAGILE (1e-3), every discrete
    output equals the implementation's.  Below it the tick is fragile and unjudged, and the model resynchronises from the implementation's record.
    FRAGILE is a condition, not a measurement; it stays >= 10 x POINT_BOUND, the bound of the fp32 interact point against the float64 one:
        a coordinate of the point is  (b * sp) * vy + (b * cp) * vz + eye  with |b| <= 1, |vy| <= 0.74, vz = -1, |eye| < 32:
        * six roundings (two products with sin / cos, two with the offset, two sums; the eye's own sum stands for the third) of values below 32:
          each at most half an ulp of 32, 2^-24 * 32                                                            -> 6 * 32 * 2^-24 = 1.15e-5
        * sin and cos each off by at most SINCOS_ERR, entering with weights |vy| and |vz|                       -> 1.74 * SINCOS_ERR
        SINCOS_ERR is measured on the CPU through mvo_sincos against numpy over [-1.6, 1.6] by test_fp32_point_bound, which asserts it:
        the largest error seen is 6.39e-8 (that test prints it), SINCOS_ERR = 2.6e-7 is four times that, so POINT_BOUND = 1.15e-5 + 4.5e-7 = 1.19e-5
        and FRAGILE / POINT_BOUND = 84.
(R) rewards.  |fp32 reward - float64 reward| <= the bound the model returns with every reward, derived here and tuned nowhere.  With u = 2^-24:
        * a tower sum over m non-zero terms, in ANY order (the product's index order, the reference's set order):  recursive summation gives
          (m - 1) u S, S = sum |x_i|; every term x_i = h * 0.05f + min(0.05f * 2^h, 20) carries two roundings of its own (the product by a
          power of two is exact): 2 u |x_i|.  Together (m + 1) u S.  The model's 0.05 is the fp32 literal's value.
        * the delta is new - old: both sums' bounds and one rounding, u |delta|.
        * rewardAgent multiplies by the shaping weight, rewardTeam by (1 - teamSpirit) and teamSpirit / teamSize: the incoming bound times the
          exact factor, plus one rounding per operation (u times the magnitude of the product), plus one rounding for every += into the
          tick's reward (u times the running sum).
        * second-order terms: the whole bound is multiplied by 1 + 2^-10.
    The bound has to stay well under the smallest real error, one missing box at y = 0: 0.05 x the weight the delta is multiplied by.  The judge
    asserts bound <= 0.05 x weight / 16 for every reward that holds a tower delta.
(U) unjudged ticks are counted, never silent: fragile ticks (capped at 2 % of a test's interact ticks), the tick an env finished on (there
    true_objective == the model's highest_tower is checked, then the model resynchronises; where an agent interacted on that very tick the objective
    is unjudged too and counted: finish_unjudged, 0 in these tests), an agent whose post pose is a respawn (0 in these tests),
    and the reward of the first placement after a fragile tick in which one agent placed a box and another took one (which of the two came first
    decides what the reward was last summed over; the record does not say).
"""
import numpy as np

CX, CY, CZ = 32, 16, 32
VX_SOLID, VX_OBJECT = 1, 4
ACT_INTERACT = 1 << 8
ZONE_MIN_Y = 1                       # the building zone's terrain box has min.y == max.y == 1
LOWEST_Y = -30                       # component_object_stacking.hpp:96
K_SPIRIT, K_PICKED, K_VISITED, K_BUILDING = 0, 1, 2, 3   # the scenario's reward-shaping table in the snapshot's order
U = 2.0 ** -24
FRAGILE = 1e-3
SINCOS_ERR = 2.6e-7
POINT_BOUND = 6 * 32 * U + 1.74 * SINCOS_ERR
assert FRAGILE >= 10 * POINT_BOUND
C05 = float(np.float32(0.05))        # the reference's literal 0.05f
PICK_OFFSET, PLACE_OFFSET = (0.0, -0.44, -1.0), (0.0, -0.44 - 0.3, -1.0)
EYE_UP = 0.05 + 0.41


class Rules:
    """the reference's rules; every field is one planted mistake of the rejection demo when changed (tests/test_tower_model.py)"""
    lookup_limit = None          # object lookup blind to indices >= this
    lookup_shift = 0             # object lookup returns index + this
    covered_can_be_taken = False
    descent = "full"             # "none": no descent; "short": stops one voxel above the support
    sum_limit = None             # the reward sum skips indices >= this
    cap = True                   # min(0.05 * 2^h, 20)
    team_divisor = None          # the team share divided by this instead of A
    zone_upper_inclusive = False
    first_pick_every_time = False
    tower_offset = 0             # highest_tower off by this

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Rules, k), k
            setattr(self, k, v)


REFERENCE = Rules()

MISTAKES = {
    "lookup blind to indices >= 48": dict(lookup_limit=48),
    "lookup off by 16": dict(lookup_shift=16),
    "a covered box can be taken": dict(covered_can_be_taken=True),
    "no descent": dict(descent="none"),
    "descent one short": dict(descent="short"),
    "the reward sum skips indices >= 48": dict(sum_limit=48),
    "the cap is missing": dict(cap=False),
    "team share divided by MAX_AGENTS": dict(team_divisor=8),
    "the zone's upper bound is inclusive": dict(zone_upper_inclusive=True),
    "first-pick reward paid every time": dict(first_pick_every_time=True),
    "highest_tower off by one": dict(tower_offset=1),
}


def coeff(h, rules=None):
    """buildingRewardCoeffForHeight, scenario_tower_building.cpp:246-251, in float64 (exact for every int h in [-30, 15] but for the two products by C05)"""
    top = C05 * 2.0 ** h
    return h * C05 + (min(top, 20.0) if rules is None or rules.cap else top)


def interact_point(pos, basis, pitch, offset):
    """eye + R(yaw, pitch) offset in float64; basis = (m00, m02, m20, m22) of the record"""
    m00, m02, m20, m22 = (float(b) for b in basis)
    sp, cp = np.sin(float(pitch)), np.cos(float(pitch))
    x, y, z = offset
    # R = Yaw * Pitch: columns right / up / back of the camera
    return (float(pos[0]) + m00 * x + m02 * sp * y + m02 * cp * z,
            float(pos[1]) + EYE_UP + cp * y - sp * z,
            float(pos[2]) + m20 * x + m22 * sp * y + m22 * cp * z)


def floor3(p):
    return tuple(int(np.floor(c)) for c in p)


def margin_of(p, axes=(0, 1, 2)):
    return min(min(p[k] - np.floor(p[k]), np.floor(p[k]) + 1.0 - p[k]) for k in axes)


def agent_point(pos):
    return (float(pos[0]), float(pos[1]) + 0.05, float(pos[2]))


class State:
    """the record a tick starts from"""

    def __init__(self, snap, A):
        n = int(snap["num_objects"])
        self.A = A
        self.objects = [[int(v) for v in snap["objects"][i]] for i in range(n)]
        ag = snap["agents"]
        self.carrying = [int(ag[i]["carrying"]) for i in range(A)]
        self.picked_up = [int(ag[i]["picked_up"]) for i in range(A)]
        self.visited_zone = [int(ag[i]["visited_zone"]) for i in range(A)]
        self.shaping = [[float(v) for v in ag[i]["shaping"][:4]] for i in range(A)]
        self.spawn = [[int(v) for v in ag[i]["spawn"]] for i in range(A)]
        self.pre_pos = [[float(v) for v in ag[i]["pos"]] for i in range(A)]
        self.zone = tuple(int(v) for v in snap["bz"])
        self.highest_tower = int(snap["highest_tower"])
        chunk = np.asarray(snap["chunk"]).reshape(CY, CZ, CX)
        self.solid = (chunk & VX_SOLID) != 0
        # currBuildingZoneReward as the heights it was summed over: the zone's boxes when the reward was last computed
        # (None: not known, Judge.sync)
        self.zone_heights = [(i, o[1]) for i, o in enumerate(self.objects) if o[3] == 0 and self.in_zone(o[0], o[2])]
        self.bz_bits = np.float32(snap["bz_reward"]).tobytes()

    def in_zone(self, x, z, rules=None):
        a, b, c, d = self.zone
        if rules is not None and rules.zone_upper_inclusive:
            return a <= x <= b and c <= z <= d
        return a <= x < b and c <= z < d

    def is_solid(self, x, y, z):
        return 0 <= x < CX and 0 <= y < CY and 0 <= z < CZ and bool(self.solid[y, z, x])

    def object_cells(self):
        return sorted((o[0], o[1], o[2]) for o in self.objects if o[3] == 0 and 0 <= o[0] < CX and 0 <= o[1] < CY and 0 <= o[2] < CZ)


def poses_of(snap, A):
    ag = snap["agents"]
    return [([float(v) for v in ag[i]["pos"]], [float(v) for v in ag[i]["basis"]], float(ag[i]["pitch"])) for i in range(A)]


class Reward:
    """one agent's reward of the tick: float64 value and the bound of rule (R)"""

    def __init__(self):
        self.v, self.err, self.weight = 0.0, 0.0, None

    def add(self, value, err_in, ops, weight=None):
        self.err += err_in + ops * U * abs(value)
        self.v += value
        self.err += U * abs(self.v)
        if weight is not None and weight > 0:
            self.weight = weight + (self.weight or 0.0)   # (what this agent's reward multiplies tower deltas by, all in all)

    @property
    def bound(self):
        return self.err * (1.0 + 2.0 ** -10)


def reward_agent(st, rewards, key, agent, mult, mult_err=0.0, ops=0, weight_of=None):
    """rewardAgent, scenario.hpp:259-262: lastReward += getReward(name) * multiplier"""
    w = st.shaping[agent][key]
    rewards[agent].add(w * mult, abs(w) * mult_err, ops + 1, None if weight_of is None else abs(w) * weight_of)


def reward_team(st, rewards, key, agent, mult, mult_err=0.0, rules=None, tower=False):
    """rewardTeam, scenario.hpp:291-298: the actor gets multiplier * (1 - teamSpirit), then every agent of the team (all of them: teamAffinity is 0)
    getReward * teamSpirit * multiplier / teamSize"""
    s = st.shaping[agent][K_SPIRIT]
    reward_agent(st, rewards, key, agent, mult * (1.0 - s), abs(1.0 - s) * mult_err, 2, abs(1.0 - s) if tower else None)
    size = st.A if rules is None or rules.team_divisor is None else rules.team_divisor
    for i in range(st.A):
        w, si = st.shaping[i][key], st.shaping[i][K_SPIRIT]
        rewards[i].add(w * si * mult / size, abs(w * si / size) * mult_err, 3, abs(w * si / size) if tower else None)


def tower_sum(st, heights, rules):
    """calculateTowerReward, scenario_tower_building.cpp:232-241 -> (float64 sum, the fp32 sum's bound in any order)"""
    terms = [coeff(h, rules) for i, h in heights if rules.sum_limit is None or i < rules.sum_limit]
    nz = [abs(t) for t in terms if t != 0.0]
    return float(np.sum(np.asarray(terms, np.float64))) if terms else 0.0, (len(nz) + 1) * U * sum(nz)


def object_at(st, x, y, z, rules):
    for i, o in enumerate(st.objects):
        if rules.lookup_limit is not None and i >= rules.lookup_limit:
            break
        if o[3] == 0 and (o[0], o[1], o[2]) == (x, y, z):   # a carried box occupies no voxel
            j = i + rules.lookup_shift
            return j if j < len(st.objects) else -1
    return -1


def interact(st, agent, pose, other_points, can_place, on_placed, on_picked, rules, margins, events):
    """onInteractAction, component_object_stacking.hpp:59-168, for one agent"""
    pos, basis, pitch = pose
    if st.carrying[agent] >= 0:
        p = interact_point(pos, basis, pitch, PLACE_OFFSET)
        margins.append(margin_of(p))
        x, y, z = floor3(p)
        collides = False
        for q in other_points:                                         # :75-86
            c = floor3(q)
            if max(abs(c[0] - x), abs(c[1] - y), abs(c[2] - z)) <= 1:   # (farther away no boundary can matter)
                margins.append(margin_of(q))
            collides = collides or c == (x, y, z)
        placeable = 0 <= x < CX and 0 <= z < CZ and y < CY             # this build's chunk
        empty = not st.is_solid(x, y, z) and object_at(st, x, y, z, REFERENCE) < 0   # :88
        if placeable and empty and not collides and can_place(x, y, z):
            while rules.descent != "none":                             # :94-106
                if y - 1 < LOWEST_Y:
                    break
                if st.is_solid(x, y - 1, z) or object_at(st, x, y - 1, z, REFERENCE) >= 0:
                    break
                y -= 1
            if rules.descent == "short" and not (y - 1 < LOWEST_Y) and y < floor3(p)[1]:
                y += 1
            idx = st.carrying[agent]
            st.objects[idx] = [x, y, z, 0]
            st.carrying[agent] = -1
            events.append(("place", agent, idx, (x, y, z)))
            on_placed(agent, idx, (x, y, z))
    else:
        p = interact_point(pos, basis, pitch, PICK_OFFSET)
        margins.append(margin_of(p))
        x, y, z = floor3(p)
        for _ in range(2):                                             # maxPickupHeight == 1: the voxel, then the one above (:137-166)
            idx = object_at(st, x, y, z, rules)
            above = object_at(st, x, y + 1, z, REFERENCE) >= 0
            if idx >= 0 and (not above or rules.covered_can_be_taken):
                st.objects[idx][3] = 1 + agent
                st.carrying[agent] = idx
                events.append(("pick", agent, idx, (x, y, z)))
                on_picked(agent, idx, (x, y, z))
                break
            y += 1


class Result:
    pass


def judge_tick(st, masks, poses, rules=None):
    """One tick of one env.  st: the State before the tick (changed in place into the state after it); masks [A]: the tick's action bit masks;
    poses [A]: the implementation's post-tick (pos, basis, pitch).  -> Result: rewards [A] (Reward), margin (inf: the tick floored nothing),
    events, interact (how many agents interacted), respawns (agents whose post pose is a fall respawn: unjudged)."""
    rules = rules or REFERENCE
    A = st.A
    rewards = [Reward() for _ in range(A)]
    margins, events = [], []
    res = Result()
    res.respawns, res.reward_unjudged = 0, False
    for i in range(A):   # FallDetectionComponent moves an agent to its spawn column's centre: the pose is then not what interact saw
        pos, basis, _ = poses[i]
        sx, sy, sz = st.spawn[i]
        if pos[0] == sx + 0.5 and pos[2] == sz + 0.5 and pos[1] - np.floor(pos[1]) == 0.5 and tuple(basis) == (1.0, 0.0, 0.0, 1.0) and st.pre_pos[i][1] < -10.0:
            res.respawns += 1

    def placed(agent, idx, voxel):   # TowerBuildingScenario::placedObject, :206-214, addCollectiveReward :253-261
        heights = [(i, o[1]) for i, o in enumerate(st.objects) if o[3] == 0 and st.in_zone(o[0], o[2], rules)]
        if st.zone_heights is None:   # (Judge.sync: what the last reward was summed over is not known; this placement's delta is unjudged)
            st.zone_heights, res.reward_unjudged = heights, True
            st.highest_tower = max(st.highest_tower, voxel[1] - ZONE_MIN_Y + 1 + rules.tower_offset)
            return
        new, new_err = tower_sum(st, heights, rules)
        old, old_err = tower_sum(st, st.zone_heights, rules)
        st.zone_heights = heights
        delta = new - old
        reward_team(st, rewards, K_BUILDING, agent, delta, new_err + old_err + U * abs(delta), rules, tower=True)
        st.highest_tower = max(st.highest_tower, voxel[1] - ZONE_MIN_Y + 1 + rules.tower_offset)

    def picked(agent, idx, voxel):   # pickedObject :216-225 (the zone set loses the voxel; the reward is not recomputed before the next placement)
        if not st.picked_up[agent] or rules.first_pick_every_time:
            reward_agent(st, rewards, K_PICKED, agent, 1.0)
            st.picked_up[agent] = 1

    res.interact = 0
    for i in range(A):   # ObjectStackingComponent::step :45-52: agents act in index order
        if not (int(masks[i]) & ACT_INTERACT):
            continue
        res.interact += 1
        others = [agent_point(poses[j][0]) for j in range(A) if j != i]
        interact(st, i, poses[i], others, lambda x, y, z: st.in_zone(x, z, rules), placed, picked, rules, margins, events)
    for i in range(A):   # TowerBuildingScenario::step :184-198, after interact and fall detection
        if st.carrying[i] < 0:
            continue
        q = agent_point(poses[i][0])
        if not st.visited_zone[i]:
            margins.append(margin_of(q, (0, 2)))
        c = floor3(q)
        if st.in_zone(c[0], c[2], rules) and not st.visited_zone[i]:
            reward_team(st, rewards, K_VISITED, i, 1.0, 0.0, rules)
            st.visited_zone[i] = 1
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
        if got != st.objects[i] and not (got[3] == st.objects[i][3] != 0):   # (a carried box's coordinates mean nothing)
            out.append(f"object {i}: {got} vs the model's {st.objects[i]}")
    ag = snap["agents"]
    for i in range(A):
        for name, want in (("carrying", st.carrying[i]), ("picked_up", st.picked_up[i]), ("visited_zone", st.visited_zone[i])):
            if int(ag[i][name]) != want:
                out.append(f"agent {i} {name}: {int(ag[i][name])} vs the model's {want}")
    if int(snap["highest_tower"]) != st.highest_tower:
        out.append(f"highest_tower: {int(snap['highest_tower'])} vs the model's {st.highest_tower}")
    chunk = np.asarray(snap["chunk"]).reshape(CY, CZ, CX)
    got = sorted((int(x), int(y), int(z)) for y, z, x in np.argwhere((chunk & VX_OBJECT) != 0))
    if got != st.object_cells():
        out.append(f"object cells: {sorted(set(got) ^ set(st.object_cells()))[:6]} differ")
    return out


class Judge:
    """Follows one gym-like object (OracleGym, MegaverseGym) env by env and applies rules (E), (R), (U) tick by tick; collects the figures the tests print."""

    def __init__(self, snapshot_of, N, A, rules=None):
        self.snapshot_of, self.N, self.A, self.rules = snapshot_of, N, A, rules
        self.states = [None] * N
        self.interact_ticks = self.fragile = self.judged = self.finished = self.respawns = self.reward_unjudged = self.finish_unjudged = 0
        self.worst_ratio, self.min_margin = 0.0, float("inf")
        self.events = []       # (env, kind, agent, index, voxel) of every judged or unjudged tick
        self.objectives = []   # (env, true_objective, the model's highest_tower, whether the last tick interacted) of every finished episode
        self.failures = []

    def sync(self, envs=None, keep=False, carried_before=None):
        """the model takes the implementation's record.  keep: the record's objects were not restated since the model last saw it -- the heights behind
        currBuildingZoneReward stay the model's own unless the implementation computed the reward anew meanwhile (a placement in an unjudged tick): then
        they are the record's zone boxes, unless an agent also took a box in that tick (carried_before: who carried what before it) -- whether before or
        after the placement is not known, the next placement's delta is unjudged (counted: reward_unjudged) and states the heights anew"""
        for e in (range(self.N) if envs is None else envs):
            old, self.states[e] = self.states[e], State(self.snapshot_of(e), self.A)
            new = self.states[e]
            if keep and old is not None and old.bz_bits == new.bz_bits:
                new.zone_heights = old.zone_heights
            elif keep and carried_before is not None and any(c >= 0 and c != b for c, b in zip(new.carrying, carried_before)):
                new.zone_heights = None

    def tick(self, masks, rewards, dones, true_objective=None, min_margin=None):
        """after the implementation stepped: masks [N, A], rewards [N * A] fp32, dones [N]; min_margin: the scripted cases' own condition"""
        masks = np.asarray(masks).reshape(self.N, self.A)
        rewards = np.asarray(rewards, np.float32).reshape(self.N, self.A)
        for e in range(self.N):
            st = self.states[e]
            snap = self.snapshot_of(e)
            if dones[e]:   # (U): the record is the next episode's
                self.finished += 1
                # the finished episode's post poses are gone with it: where an agent interacted on this very tick a placement may have raised the tower,
                # the objective is unjudged and counted; otherwise it equals the model's highest_tower
                acted = any(int(m) & ACT_INTERACT for m in masks[e])
                if true_objective is not None:
                    got = [true_objective(e, a) for a in range(self.A)]
                    if acted:
                        self.finish_unjudged += 1
                    elif not all(g == st.highest_tower for g in got):
                        self.failures.append(f"env {e}: true_objective {got} vs the model's highest_tower {st.highest_tower}")
                    self.objectives.append((e, got[0], st.highest_tower, acted))
                self.sync([e])
                continue
            carried, bits = list(st.carrying), st.bz_bits
            res = judge_tick(st, masks[e], poses_of(snap, self.A), self.rules)
            st.bz_bits = bits
            self.interact_ticks += res.interact > 0
            self.respawns += res.respawns
            self.events += [(e,) + ev for ev in res.events]
            if res.respawns:
                self.sync([e], keep=True, carried_before=carried)
                continue
            if res.interact:
                self.min_margin = min(self.min_margin, res.margin)
            if min_margin is not None and res.margin < min_margin:
                self.failures.append(f"env {e}: a scripted tick with margin {res.margin:.4f} < {min_margin}")
            if res.margin < FRAGILE:
                self.fragile += 1
                self.sync([e], keep=True, carried_before=carried)
                continue
            self.judged += 1
            self.reward_unjudged += res.reward_unjudged
            for d in differences(st, snap, self.A):
                self.failures.append(f"env {e}: {d}")
            for a in range(self.A if not res.reward_unjudged else 0):
                r = res.rewards[a]
                err = abs(float(rewards[e, a]) - r.v)
                if r.bound > 0:
                    self.worst_ratio = max(self.worst_ratio, err / r.bound)
                if err > r.bound:
                    self.failures.append(f"env {e} agent {a}: reward {float(rewards[e, a])!r} vs the model's {r.v!r}, bound {r.bound:.3g}")
                if r.weight is not None and not r.bound <= 0.05 * r.weight / 16:
                    self.failures.append(f"env {e} agent {a}: bound {r.bound:.3g} not well under one missing box, 0.05 x {r.weight:.3g}")
            if self.failures:
                self.sync([e], keep=True, carried_before=carried)   # (one difference is reported once)
            else:
                st.pre_pos = [p[0] for p in poses_of(snap, self.A)]
                st.bz_bits = np.float32(snap["bz_reward"]).tobytes()

    def counts(self):
        picks = [ev for ev in self.events if ev[1] == "pick"]
        places = [ev for ev in self.events if ev[1] == "place"]
        return {"picks": len(picks), "placements": len(places), "picks_48": sum(ev[3] >= 48 for ev in picks),
                "placements_48": sum(ev[3] >= 48 for ev in places), "placements_y3": sum(ev[4][1] >= 3 for ev in places)}
