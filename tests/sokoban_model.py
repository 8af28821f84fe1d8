"""An independent model of Sokoban's rules: one function judges one tick of one env.  TEST INFRASTRUCTURE ONLY.

Written from the reference's rules, not from the kernel (megaverse_amd/csrc/mv_tick_sokoban.h) or the oracle (oracle/mv_oracle.cpp) (reference paths
relative to src/libs):
    SokobanScenario::createLayout      scenarios/src/scenario_sokoban.cpp:120-166   rows[x][z]; '#' a wall (:142-147); '.' and '+' a goal (:157-158);
                                                                                    '$' and '*' a box (:160-163) -- a '*' cell holds a box and NO goal
    SokobanScenario::reset             :103-118                                     solved = false, numBoxesOnGoal = 0
    SokobanScenario::step              :168-233
    VoxelGrid::getCoords               util/include/util/voxel_grid.hpp:144-149     floor(p / voxelSize), voxelSize = 2 (scenario_sokoban.cpp:40)
    trueObjective == solved            scenarios/include/scenarios/scenario_sokoban.hpp
    Scenario::rewardTeam / doneWithTimer, Env::step                                 as in tests/rearrange_model.py

The rule, in agent order (:173-232): Interact was pressed; the interact point's cell holds a box; the Manhattan distance between the agent's cell and
the box's cell -- all three coordinates -- is exactly 1; no agent stands in the cell behind the box (the loop :192-196 does not skip the pusher; it
cannot matter, see UNOBSERVABLE); the destination is no wall and holds no box; the box moves by the cell delta; +sokobanBoxOnTarget when it enters a
goal from a cell that is none, and then sokobanAllBoxesOnTarget when onGoal == numBoxes && !solved, with doneWithTimer; -sokobanBoxLeavesTarget (the
weight is negative) when it leaves a goal for a cell that is none.

The model states the terrain from the LEVEL TEXT (the fixture the gym was made with), not from the record: a State recognises its level by walls and
start boxes when an episode begins and complains where the record's cells differ.  Cells are floor(p / 2); the fragile margin of rule (E) is taken on
p / 2 (the division by two is exact), of the interact point, of the pusher's position and of every agent's position next to the destination.

Rules (E), (R), (U) are tests/tower_model.py's, applied by tests/rule_judge.py."""
import numpy as np

import tower_model as T
from rearrange_model import DT, REMAINING, Result

K_SPIRIT, K_ON, K_LEAVES, K_ALL = 0, 1, 2, 3   # the scenario's reward-shaping table in the snapshot's order
ACT_INTERACT = T.ACT_INTERACT
BOX_Y = 1
DIM = 32


class Rules:
    """the reference's rules; every field is one planted mistake of the rejection demo when changed (tests/test_sokoban_model.py)"""
    skip_pusher = False          # the occupied test skips the pusher
    max_distance = 1             # with min_distance: the push needs min <= distance <= max
    min_distance = 1
    star_goal = False            # '*' makes a goal
    bonus_every_time = False     # the solve bonus is paid whenever onGoal reaches numBoxes
    leave_on_goal_to_goal = False
    box_blocks = True
    team_divisor = None

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Rules, k), k
            setattr(self, k, v)


REFERENCE = Rules()

MISTAKES = {
    "`*` makes a goal": dict(star_goal=True),
    "the solve bonus is paid every time onGoal reaches numBoxes": dict(bonus_every_time=True),
    "the leave penalty is paid on goal -> goal moves": dict(leave_on_goal_to_goal=True),
    "a box can be pushed into a box": dict(box_blocks=False),
    "the team share is divided by 8": dict(team_divisor=8),
    "distance <= 2 instead of == 1": dict(max_distance=2),
}

# Two mistakes one might plant change nothing that can be observed, by the reference's own lines: with distance == 1 the destination is the pusher's
# cell plus twice a non-zero delta, never the pusher's own cell, so skipping the pusher in the occupied test changes nothing; and at distance 0 the
# delta is zero, the destination is the box's own cell, which holds a box (and the pusher): refused either way.  test_sokoban_model.py shows that no
# scripted case tells them from the reference; "distance <= 2" above is the observable form of the second.
UNOBSERVABLE = {
    "the pusher is skipped in the occupied test": dict(skip_pusher=True),
    "distance <= 1 instead of == 1": dict(min_distance=0),
}


def parse_levels(text):
    """the levels a SokobanScenario can pick from one file: all but the last (reloadLevels stores a level when it meets the next ';' line, :92-99)"""
    levels, cur = [], None
    for line in text.split("\n"):
        if line.startswith(";"):
            if cur is not None:
                levels.append(cur)
            cur = []
        elif cur is not None:
            cur.append(line)
    return [[r for r in lv if r] for lv in levels]


def cells_of(rows, chars):
    return {(x, z) for x, r in enumerate(rows) for z, c in enumerate(r) if c in chars}


class State:
    """the record a tick starts from"""

    def __init__(self, snap, A, prev=None, levels=()):
        self.A = A
        self.objects = [[int(v) for v in snap["objects"][i]] for i in range(int(snap["num_objects"]))]
        ag = snap["agents"]
        self.shaping = [[float(v) for v in ag[i]["shaping"][:4]] for i in range(A)]
        self.on_goal = int(snap["highest_tower"])
        self.solved = int(snap["solved"])
        self.sec, self.len = np.float32(snap["episode_sec"]), np.float32(snap["episode_len"])
        self.complaints = []
        grid = np.asarray(snap["soko"]).reshape(DIM, DIM)
        walls = {(int(x), int(z)) for x, z in zip(*np.nonzero(grid == 1))}
        goals = {(int(x), int(z)) for x, z in zip(*np.nonzero(grid == 2))}
        if prev is not None:
            self.rows = prev.rows
        else:
            boxes = sorted((o[0], o[2]) for o in self.objects)
            found = [rows for rows in levels if cells_of(rows, "#") == walls and sorted(cells_of(rows, "$*")) == boxes]
            self.rows = found[0] if len(found) == 1 else None
            if self.rows is None:
                self.complaints.append(f"{len(found)} levels of the fixture have these walls and boxes")
                self.rows = [""]
            elif self.on_goal != 0 or self.solved != 0:
                self.complaints.append(f"an episode begins with onGoal {self.on_goal}, solved {self.solved}")
        if cells_of(self.rows, "#") != walls or cells_of(self.rows, ".+") != goals:
            self.complaints.append(f"the record's cells differ from the level's: walls {sorted(cells_of(self.rows, '#') ^ walls)[:4]}, goals {sorted(cells_of(self.rows, '.+') ^ goals)[:4]}")
        if any(o[1] != BOX_Y or o[3] != 0 for o in self.objects):
            self.complaints.append("a box outside the layer y = 1")

    def char(self, cell):
        x, y, z = cell
        if y != BOX_Y or not (0 <= x < len(self.rows) and 0 <= z < len(self.rows[x])):
            return " "
        return self.rows[x][z]

    def is_goal(self, cell, rules):
        return self.char(cell) in (".+*" if rules.star_goal else ".+")

    def is_wall(self, cell):
        return self.char(cell) == "#"

    def box_at(self, cell):
        for i, o in enumerate(self.objects):
            if (o[0], o[1], o[2]) == tuple(cell):
                return i
        return -1

    def num_goals(self, rules=None):
        return len(cells_of(self.rows, ".+*" if rules is not None and rules.star_goal else ".+"))


def ends_without_interaction(st):
    return np.float32(st.sec + DT) >= st.len


def half(p):
    return tuple(float(c) / 2.0 for c in p)


def judge_tick(st, masks, poses, rules=None):
    """One tick of one env.  st: the State before the tick (changed in place into the state after it); masks [A]; poses [A]: the implementation's
    post-tick (pos, basis, pitch) -> Result"""
    rules = rules or REFERENCE
    A = st.A
    rewards = [T.Reward() for _ in range(A)]
    margins, events = [], []
    res = Result()
    res.solved_now = res.clamped = res.interact = 0
    for i in range(A):
        if not (int(masks[i]) & ACT_INTERACT):
            continue
        res.interact += 1
        pos, basis, pitch = poses[i]
        p = half(T.interact_point(pos, basis, pitch, T.PICK_OFFSET))   # agent->interactLocation(), :178
        margins.append(T.margin_of(p))
        box = T.floor3(p)
        idx = st.box_at(box)
        if idx < 0:                                                    # :181
            continue
        margins.append(T.margin_of(half(pos)))
        me = T.floor3(half(pos))
        delta = tuple(b - a for a, b in zip(me, box))
        dist = sum(abs(d) for d in delta)                              # :184
        if not (rules.min_distance <= dist <= rules.max_distance):     # :186
            events.append(("refuse_distance", i, idx, box))
            continue
        dst = tuple(b + d for b, d in zip(box, delta))
        occupied = False
        for j in range(A):                                             # :192-196
            q = half(poses[j][0])
            c = T.floor3(q)
            if max(abs(c[k] - dst[k]) for k in range(3)) <= 1:         # (farther away no boundary can matter)
                margins.append(T.margin_of(q))
            if c == dst and not (rules.skip_pusher and j == i):
                occupied = True
        if occupied:
            events.append(("refuse_agent", i, idx, box))
            continue
        if st.is_wall(dst):                                            # :203
            events.append(("refuse_wall", i, idx, box))
            continue
        if st.box_at(dst) >= 0 and rules.box_blocks:
            events.append(("refuse_box", i, idx, box))
            continue
        st.objects[idx][:3] = list(dst)                                # :204-207
        events.append(("push", i, idx, dst))
        src_goal, dst_goal = st.is_goal(box, rules), st.is_goal(dst, rules)
        if not src_goal and dst_goal:                                  # :210-220
            st.on_goal += 1
            events.append(("enter", i, idx, dst))
            T.reward_team(st, rewards, K_ON, i, 1.0, 0.0, rules)
            if st.on_goal == len(st.objects) and (not st.solved or rules.bonus_every_time):
                st.solved = 1
                res.solved_now = 1
                events.append(("solve", i, idx, dst))
                T.reward_team(st, rewards, K_ALL, i, 1.0, 0.0, rules)
                if st.len - REMAINING > st.sec:
                    st.sec = np.float32(st.len - REMAINING)
                    res.clamped = 1
        elif src_goal and (not dst_goal or rules.leave_on_goal_to_goal):   # :222-226
            if not dst_goal:
                st.on_goal -= 1
            events.append(("leave", i, idx, dst))
            T.reward_team(st, rewards, K_LEAVES, i, 1.0, 0.0, rules)
    st.sec = np.float32(st.sec + DT)
    res.done = bool(st.sec >= st.len)
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
        if got != st.objects[i]:
            out.append(f"box {i}: {got} vs the model's {st.objects[i]}")
    for name, want in (("highest_tower", st.on_goal), ("solved", st.solved)):
        if int(snap[name]) != want:
            out.append(f"{name}: {int(snap[name])} vs the model's {want}")
    if np.float32(snap["episode_sec"]).tobytes() != np.float32(st.sec).tobytes():
        out.append(f"episode_sec: {float(snap['episode_sec'])!r} vs the model's {float(st.sec)!r}")
    return out
