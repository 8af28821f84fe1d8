"""Scripted Sokoban cases and the `pusher` stress policy (tests/sokoban_model.py judges them), shared by the CPU test of the oracle
(test_sokoban_model.py) and the GPU tests (test_sokoban_model_gpu.py).  TEST INFRASTRUCTURE ONLY.

Structured like tests/tower_cases.py.  The levels are tests/golden/boxoban_solvable (hand-written, public Boxoban text format; BOXOBAN_LEVELS must name
that directory while a case's gym lives).  Levels are shuffled per env: a case recognises the level of every env from the snapshot's cells and plays its
script in the envs that hold the level it is about.

Geometry: a cell is 2 x 2, its floor's top is at 2.0; an agent standing half a unit from its cell's centre towards a box in the next cell has its
interact point, 1 ahead, half a unit inside the box's cell."""
import functools
import os

import numpy as np

import sokoban_model as M
import tower_cases as TC

MARGIN = TC.MARGIN
LEVEL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxoban_solvable")
LEVEL_FILE = os.path.join(LEVEL_DIR, "unfiltered", "train", "000.txt")
CORRIDOR, TWO_BOX, STAR, BLOCKED = 0, 1, 2, 3   # the fixture's levels the scripted cases are about
DIRS = {"+x": (1, 0), "-x": (-1, 0), "+z": (0, 1), "-z": (0, -1)}
FLOOR = 2.0


@functools.lru_cache(maxsize=None)
def levels():
    with open(LEVEL_FILE) as f:
        return M.parse_levels(f.read())


class Case(TC.Case):
    scenario = "Sokoban"

    def make(self, cls, **kw):
        assert os.environ.get("BOXOBAN_LEVELS") == LEVEL_DIR, "BOXOBAN_LEVELS must name tests/golden/boxoban_solvable"
        return super().make(cls, **kw)


def yaw_of(d, turn=0.0):
    """(cos, sin) of the yaw that looks along d = (dx, dz): forward = (-sin yaw, 0, -cos yaw)"""
    if not turn and d in DIRS.values():
        return (float(-d[1]), float(-d[0]))
    yaw = np.arctan2(-d[0], -d[1]) + turn
    return (float(np.float32(np.cos(yaw))), float(np.float32(np.sin(yaw))))


def push_pose(e, a, box, d, pitch=0.0, turn=0.0):
    """agent a in the cell before `box` (against d), half a unit towards it, looking along d"""
    cell = (box[0] - d[0], box[1] - d[1])
    return ("pose", e, a, (cell[0] * 2 + 1 + 0.5 * d[0], TC.stand(FLOOR), cell[1] * 2 + 1 + 0.5 * d[1]), yaw_of(d, turn), float(pitch))


def stand_pose(e, a, cell):
    return ("pose", e, a, (cell[0] * 2 + 1.0, TC.stand(FLOOR), cell[1] * 2 + 1.0), (1.0, 0.0), 0.0)


class World:
    """one env as the script's author sees it"""

    def __init__(self, snap, e, A, prev=None):
        """prev: the World of the same episode a tick ago (a level is recognised by its START boxes)"""
        st = self.state = M.State(snap, A, prev=prev and prev.state, levels=levels())
        self.e, self.A, self.rows = e, A, st.rows
        self.level = levels().index(st.rows) if st.rows in levels() else -1
        self.boxes = [(o[0], o[2]) for o in st.objects]
        self.script = []

    def char(self, c):
        return self.rows[c[0]][c[1]] if 0 <= c[0] < len(self.rows) and 0 <= c[1] < len(self.rows[c[0]]) else "#"

    def free(self, c):
        return self.char(c) != "#" and c not in self.boxes

    def parks(self):
        """cells to stand aside in: free, no goal, at least two cells from every box, from the bottom row up"""
        out = [(x, z) for x in range(len(self.rows) - 2, 0, -1) for z in range(1, 9) if self.char((x, z)) == " " and (x, z) not in self.boxes
               and all(max(abs(x - b[0]), abs(z - b[1])) >= 2 for b in self.boxes)]
        return out[::2]

    def tick(self, acts=None, idle=None):
        """acts: {agent: pose command} -- those agents interact; idle: the same for agents that only stand there; everybody else stands aside"""
        acts, idle = acts or {}, idle or {}
        parks = self.parks()
        cmds = [acts[a] if a in acts else idle[a] if a in idle else stand_pose(self.e, a, parks[a]) for a in range(self.A)]
        self.script.append((cmds, [int(a in acts) for a in range(self.A)]))
        return len(self.script) - 1

    def push(self, a, i, face, moves=True):
        """the pose command for agent a pushing box i along `face`; the author's world follows when the box is to move"""
        d = DIRS[face]
        b = self.boxes[i]
        assert self.free((b[0] - d[0], b[1] - d[1]))
        cmd = push_pose(self.e, a, b, d)
        if moves:
            dst = (b[0] + d[0], b[1] + d[1])
            assert self.free(dst)
            self.boxes[i] = dst
        return cmd


def build_with(level, script):
    """a builder: every env that holds `level` plays script(world) -> notes; the envs' scripts begin on one tick"""
    def build(case, snaps):
        ws = [World(s, e, case.A) for e, s in enumerate(snaps)]
        notes = {}
        for w in ws:
            if w.level == level:
                notes[w.e] = script(w)
        assert notes, f"no env of this seed holds level {level}"
        case.notes = notes
        n = max(len(w.script) for w in ws)
        segs = []
        for t in range(n):
            cmds, act = [], np.zeros((1, case.N * case.A, 6), np.int32)
            for w in ws:
                if t < len(w.script):
                    cmds += w.script[t][0]
                    act[0, w.e * case.A:(w.e + 1) * case.A, 4] = w.script[t][1]
            segs.append((cmds, act))
        segs[-1] = (segs[-1][0], np.concatenate([segs[-1][1], np.zeros((case.tail, case.N * case.A, 6), np.int32)]))
        return segs
    return build


def box_index(w, cell):
    return w.boxes.index(cell)


def script_corridor(w):
    """one push solves: +1 and +10; four idle ticks follow: solved, the timer clamped, and on the last one done and the next level"""
    return dict(t_solve=w.tick({0: w.push(0, box_index(w, (2, 3)), "+z")}))


def script_goals(w):
    """the two-box level: onto a goal (+1), goal to goal (nothing), off it (-1), back on (+1); the other box in two pushes, the second one solves
    (+1 and +10); then, solved, that box off its goal (-1) and back on (+1 only: solved stays)"""
    b, a = box_index(w, (4, 4)), box_index(w, (2, 2))
    n = dict(t_on=w.tick({0: w.push(0, b, "+z")}), t_goal_to_goal=w.tick({0: w.push(0, b, "+z")}), t_off=w.tick({0: w.push(0, b, "+z")}),
             t_back=w.tick({0: w.push(0, b, "-z")}), t_plain=w.tick({0: w.push(0, a, "+z")}), t_solve=w.tick({0: w.push(0, a, "+z")}),
             t_off_solved=w.tick({0: w.push(0, a, "+z")}), t_on_solved=w.tick({0: w.push(0, a, "-z")}))
    return n


def script_star(w):
    """the level with a '*': its box stands on no goal, pushing it away pays nothing; one box more than goals: never solved"""
    s = box_index(w, (2, 3))
    return dict(t_star=w.tick({0: w.push(0, s, "+z")}), t_goal=w.tick({0: w.push(0, s, "+z")}))


def script_refusals(w):
    """A = 2: a wall behind the box; a box behind the box; agent 1 behind the box; the interact point in a box's cell from the diagonal cell; and from
    the cell over the neighbour cell, two cells away.  Nothing moves."""
    corner, left, right = box_index(w, (1, 1)), box_index(w, (2, 3)), box_index(w, (2, 4))
    n = dict(t_wall=w.tick({0: w.push(0, corner, "-x", moves=False)}), t_box=w.tick({0: w.push(0, left, "+z", moves=False)}),
             t_agent=w.tick({0: w.push(0, right, "-x", moves=False)}, idle={1: stand_pose(w.e, 1, (1, 4))}))
    diag = ("pose", w.e, 0, (4.3, TC.stand(FLOOR), 4.3), yaw_of((-1.0, -1.0)), 0.0)   # in cell (2, 2)'s low corner, looking at (1, 1)
    n["t_diagonal"] = w.tick({0: diag})
    above = ("pose", w.e, 0, (5.0, 4.3, 5.8), yaw_of((0, 1)), -0.8)   # over cell (2, 2), looking down into (2, 3)
    n["t_above"] = w.tick({0: above})
    return n


def script_two_agents(w):
    """A = 2: both push different boxes on one tick; both push one box from opposite sides -- each stands in the cell behind the box as the other
    sees it, both are refused; both push it from two sides at a right angle: agent 0 moves it, agent 1's point no longer holds a box"""
    a, b = box_index(w, (2, 2)), box_index(w, (4, 4))
    n = dict(t_both=w.tick({0: w.push(0, a, "+z"), 1: w.push(1, b, "+z")}))
    n["t_opposite"] = w.tick({0: w.push(0, a, "+z", moves=False), 1: w.push(1, a, "-z", moves=False)})
    side = w.push(1, a, "+x", moves=False)
    n["t_angle"] = w.tick({0: w.push(0, a, "+z"), 1: side})
    return n


def script_spirit(w):
    """A = 3, teamSpirit 0.5: agent 1 earns the +1, rewardTeam shares it"""
    w.script.append(([("shaping", w.e, a, {"teamSpirit": 0.5}) for a in range(w.A)], [0] * w.A))
    return dict(t_on=w.tick({1: w.push(1, box_index(w, (4, 4)), "+z")}))


# ---- the pusher ----------------------------------------------------------------------------------------------------------------------------------

STRESS_TICKS = 300
STRESS_PARAMS = {"episodeLengthSec": 8.0}
STRESS_SEEDS = {1: 21, 4: 22}   # chosen on the CPU with the oracle (test_sokoban_model.py asserts the counts they give)


@functools.lru_cache(maxsize=None)
def pusher_script(name):
    """The stress policy, computed ONCE from the CPU oracle's snapshots and recorded as setter calls and masks, so that every gym replays the identical
    script.  On most ticks every agent is teleported next to a random box, turned to the box (or, sometimes, to another of the four axis directions)
    plus an offset within +-0.3 rad, given a pitch and presses Interact -- often at a box that one push puts on a goal; now and then it stands in the diagonal cell instead, or in the cell behind the
    box another agent pushes; on the other ticks, and on the tick an episode's timer runs out, it walks."""
    import oracle_lib
    case = CASES[name]
    rng = np.random.default_rng(STRESS_SEEDS[case.A])
    g = case.make(oracle_lib.OracleGym)
    faces = list(DIRS.values())
    segs, worlds = [], [None] * case.N
    for t in range(STRESS_TICKS):
        cmds, act = [], np.zeros((1, case.N * case.A, 6), np.int32)
        for e in range(case.N):
            w = worlds[e] = World(TC.snapshot(g, e), e, case.A, worlds[e])
            taken, behind = [], None
            last = M.ends_without_interaction(w.state)   # the timer runs out on this tick: everybody walks, the finishing tick stays judged
            for a in range(case.A):
                if rng.random() < 0.1 or not w.boxes or last:
                    act[0, e * case.A + a, 1] = 1
                    continue
                if behind is not None and behind not in taken:   # in the way of the agent before
                    taken.append(behind)
                    cmds.append(stand_pose(e, a, behind))
                    behind = None
                    continue
                onto = [(b, d) for b in w.boxes for d in faces if w.char(b) not in ".+" and w.char((b[0] + d[0], b[1] + d[1])) in ".+"
                        and w.free((b[0] + d[0], b[1] + d[1])) and w.free((b[0] - d[0], b[1] - d[1])) and (b[0] - d[0], b[1] - d[1]) not in taken]
                errand = onto[int(rng.integers(len(onto)))] if onto and rng.random() < 0.4 else None   # a box that one push puts on a goal
                for _ in range(8):
                    b = w.boxes[int(rng.integers(len(w.boxes)))]
                    d = faces[int(rng.integers(4))]
                    kind = rng.random()
                    if errand:
                        b, d, kind = errand[0], errand[1], 1.0
                    cell = (b[0] - d[0], b[1] - d[1]) if kind >= 0.12 else (b[0] - d[0] - d[1], b[1] - d[1] - d[0])
                    if w.free(cell) and cell not in taken:
                        break
                else:
                    act[0, e * case.A + a, 1] = 1
                    continue
                taken.append(cell)
                pitch = float(np.float32(rng.uniform(-0.3, 0.5)))
                turn = float(rng.uniform(-0.3, 0.3))
                if kind < 0.12:      # from the diagonal cell, towards the box
                    dd = (b[0] - cell[0], b[1] - cell[1])
                    cmds.append(("pose", e, a, (cell[0] * 2 + 1 + 0.7 * dd[0], TC.stand(FLOOR), cell[1] * 2 + 1 + 0.7 * dd[1]),
                                 yaw_of((float(dd[0]), float(dd[1])), turn), pitch))
                else:
                    look = d if kind >= 0.2 else faces[int(rng.integers(4))]
                    cmds.append(push_pose(e, a, b, d, pitch, turn)[:4] + (yaw_of(look, turn), pitch))
                    dst = (b[0] + d[0], b[1] + d[1])
                    if look == d and rng.random() < 0.3 and w.free(dst):
                        behind = dst
                act[0, e * case.A + a, 4] = 1
        TC.apply(g, cmds)
        for i in range(case.N * case.A):
            g.set_actions(i // case.A, i % case.A, act[0, i].tolist())
        TC.tick(g)
        segs.append((cmds, act))
        for e in np.nonzero(TC.dones_of(g, case.N))[0]:
            worlds[e] = None
    g.close()
    return segs


def make_stress(name):
    return lambda case, snaps: pusher_script(name)


def scripted(name, N, A, level, script, tail=0, **kw):
    c = Case(name, N, A, None, **kw)
    c.tail = tail
    c.build = build_with(level, script)
    return c


CASES = {c.name: c for c in (
    scripted("corridor", 12, 1, CORRIDOR, script_corridor, tail=4, replay=1),
    scripted("goals", 12, 1, TWO_BOX, script_goals, tail=2, replay=1),
    scripted("star", 12, 1, STAR, script_star),
    scripted("refusals", 12, 2, BLOCKED, script_refusals),
    scripted("two_agents", 12, 2, TWO_BOX, script_two_agents, replay=1),
    scripted("spirit", 12, 3, TWO_BOX, script_spirit, replay=1),
    Case("pusher_a1", 8, 1, make_stress("pusher_a1"), params=STRESS_PARAMS, scripted=False, replay=1),
    Case("pusher_a4", 8, 4, make_stress("pusher_a4"), params=STRESS_PARAMS, scripted=False, replay=1),
)}
