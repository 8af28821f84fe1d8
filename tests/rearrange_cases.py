"""Scripted Rearrange cases and the `courier` stress policy (tests/rearrange_model.py judges them), shared by the CPU test of the oracle
(test_rearrange_model.py) and the GPU tests (test_rearrange_model_gpu.py).  TEST INFRASTRUCTURE ONLY.

Structured like tests/tower_cases.py: a case drives ONE gym-like object; it is a list of segments -- setter commands (poses, reward shaping), then k
ticks of multi-discrete actions.  Nothing is assumed about what a seed draws: every item and every cell is read from the snapshots the case is built
from; an item reaches a cell by being picked up and carried there.  Every scripted tick keeps its floored points MARGIN away from a voxel boundary.

Geometry (reference: scenario_rearrange.cpp:285-299): the working pedestal's top is at 2.0 over x in [10.5, 16.5], z in [2.5, 8.5], and at 2.05 over the
cells within +-1 of rightCenter (13, 2, 5); the raised floor's top is at 1.5.  An agent standing on the pedestal at pitch 0 picks at y = 2.835 and
places at y = 2.535, one voxel ahead (items lie at voxel y = 2); at pitch 0.5 it picks, at 0.6 it places in y = 3, still one voxel ahead."""
import functools

import numpy as np

import rearrange_model as M
import tower_cases as TC

MARGIN = TC.MARGIN
CENTRE = (M.RIGHT[0], M.RIGHT[2])
WORK = [(x, z) for x in range(CENTRE[0] - 2, CENTRE[0] + 3) for z in range(CENTRE[1] - 2, CENTRE[1] + 3)]
NEIGHBOURS = (("+x", (1, 0)), ("-x", (-1, 0)), ("+z", (0, 1)), ("-z", (0, -1)))
PITCH_PICK_UP, PITCH_PLACE_UP = 0.5, 0.6


def surface(cell):
    return 2.05 if abs(cell[0] - CENTRE[0]) <= 1 and abs(cell[1] - CENTRE[1]) <= 1 else 2.0


def pose(e, a, cell, face="+x", pitch=0.0, turn=0.0):
    """agent a of env e standing over the centre of pedestal cell (x, z), facing `face` turned by `turn` rad"""
    dx, dz = TC.DIRS[face]
    cs = (float(-dz), float(-dx))
    if turn:
        yaw = np.arctan2(-dx, -dz) + turn
        cs = (float(np.float32(np.cos(yaw))), float(np.float32(np.sin(yaw))))
    return ("pose", e, a, (cell[0] + 0.5, TC.stand(surface(cell)), cell[1] + 0.5), cs, float(pitch))


def park(e, a):
    """aside on the raised floor, beyond both pedestals' steps"""
    return ("pose", e, a, (3.5 + 2 * a, TC.stand(1.5), 11.5), (1.0, 0.0), 0.0)


class Case(TC.Case):
    scenario = "Rearrange"


class World:
    """one env as the script's author sees it: what lies where, who carries what; its methods append one tick each to the env's script"""

    def __init__(self, snap, e, A):
        st = M.State(snap, A)
        self.e, self.A, self.items = e, A, st.items
        self.objects = [list(o) for o in st.objects]
        self.carry = [-1] * A
        self.script = []   # (commands, [A] interact flags) per tick

    def target(self, i):
        off = self.items[i][2]
        return (M.RIGHT[0] + off[0], M.RIGHT[1] + off[1], M.RIGHT[2] + off[2])

    def at(self, voxel):
        for i, o in enumerate(self.objects):
            if o[3] == 0 and tuple(o[:3]) == tuple(voxel):
                return i
        return -1

    def column(self, cell):
        return [i for i, o in enumerate(self.objects) if o[3] == 0 and (o[0], o[2]) == tuple(cell)]

    def displaced(self):
        return [i for i, o in enumerate(self.objects) if o[3] == 0 and tuple(o[:3]) != self.target(i)]

    def free_cells(self, avoid=()):
        return [c for c in WORK if not self.column(c) and c not in avoid]

    def stand_for(self, cell, avoid=()):
        """(a free pedestal cell beside `cell`, the direction from it to `cell`) or None"""
        for face, (dx, dz) in NEIGHBOURS:
            s = (cell[0] - dx, cell[1] - dz)
            if s in WORK and not self.column(s) and s not in avoid:
                return s, face
        return None

    def tick(self, acts=None, idle=None, extra=()):
        """acts: {agent: (stand cell, face, pitch)} -- those agents interact; idle: the same for agents that only stand there; everybody else stands
        aside; extra: further commands"""
        acts, idle = acts or {}, idle or {}
        mk = lambda a, v: v if v[0] == "pose" else pose(self.e, a, *v)   # (a ready-made pose command passes through)
        cmds = [mk(a, acts[a]) if a in acts else mk(a, idle[a]) if a in idle else park(self.e, a) for a in range(self.A)]
        self.script.append((cmds + list(extra), [int(a in acts) for a in range(self.A)]))
        return len(self.script) - 1

    def pick_act(self, a, i, avoid=()):
        x, y, z = self.objects[i][:3]
        s = self.stand_for((x, z), avoid)
        assert s is not None and self.carry[a] < 0
        self.objects[i][3], self.carry[a] = 1 + a, i
        return (s[0], s[1], 0.0 if y == 2 else PITCH_PICK_UP)

    def place_act(self, a, voxel, avoid=(), settle=None):
        """settle: the voxel the item comes to rest in when that is not the one aimed at (the descent)"""
        s = self.stand_for((voxel[0], voxel[2]), avoid)
        assert s is not None and self.carry[a] >= 0
        self.objects[self.carry[a]] = list(settle or voxel) + [0]
        self.carry[a] = -1
        return (s[0], s[1], 0.0 if voxel[1] == 2 else PITCH_PLACE_UP)

    def move(self, a, i, voxel):
        self.tick({a: self.pick_act(a, i)})
        return self.tick({a: self.place_act(a, voxel)})

    def reachable(self, i):
        o = self.objects[i]
        return self.stand_for((o[0], o[2])) is not None and self.stand_for((self.target(i)[0], self.target(i)[2])) is not None


def combine(case, scripts, tail=0):
    """the envs' scripts side by side, aligned at their LAST tick -> segments of one tick each; the last one goes on for `tail` idle ticks"""
    n = max(len(s) for s in scripts)
    segs = []
    for t in range(n):
        cmds, act = [], np.zeros((1, case.N * case.A, 6), np.int32)
        for e, s in enumerate(scripts):
            k = t - (n - len(s))
            if k >= 0:
                cmds += s[k][0]
                act[0, e * case.A:(e + 1) * case.A, 4] = s[k][1]
        segs.append((cmds, act))
    if tail:
        segs[-1] = (segs[-1][0], np.concatenate([segs[-1][1], np.zeros((tail, case.N * case.A, 6), np.int32)]))
    return segs


def worlds(case, snaps):
    return [World(s, e, case.A) for e, s in enumerate(snaps)]


def floor_item(w, more=2):
    """a displaced item whose place is on the pedestal itself, in an env with at least `more` displaced items (so that placing it does not solve)"""
    d = w.displaced()
    for i in d:
        if len(d) >= more and w.target(i)[1] == 2 and w.reachable(i):
            return i
    return None


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
# every builder leaves case.notes: {env: what the tests assert on, by tick index of the whole case}

def finish(case, ws, notes, tail=0):
    n = max(len(w.script) for w in ws)
    case.notes = {e: {k: (v + n - len(ws[e].script) if k.startswith("t_") else v) for k, v in d.items()} for e, d in notes.items()}
    assert case.notes, "no env of this seed allows the case"
    return combine(case, [w.script for w in ws], tail)


def build_match(case, snaps):
    """place a displaced item on its matching cell (+1, maxMatching grows), take it again and put it back (nothing: a high-water mark)"""
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        i = floor_item(w)
        if i is None:
            continue
        t = w.move(0, i, w.target(i))
        t2 = w.move(0, i, w.target(i))
        notes[w.e] = dict(t_first=t, t_second=t2, item=i)
    return finish(case, ws, notes)


def solve_all(w, a=0, leave=0):
    """every displaced item to its place in item order (a support comes before what stands on it); the last `leave` stay where they are"""
    d = w.displaced()
    for i in d[:len(d) - leave]:
        if not w.reachable(i):
            return None
        t = w.move(a, i, w.target(i))
    return d[len(d) - leave:] if leave else t


def build_solve(case, snaps):
    """every env puts all its items in place; the scripts end on one tick, the solving one, and four idle ticks follow: on the last one the envs finish and restart"""
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        saved = ([list(o) for o in w.objects], list(w.script))
        t = solve_all(w)
        if t is None:
            w.objects, w.script = saved
            continue
        notes[w.e] = dict(t_solve=t, items=len(w.items))
    return finish(case, ws, notes, tail=4)


def build_timeout(case, snaps):
    """nobody does anything: the episode times out unsolved"""
    case.notes = {e: {} for e in range(case.N)}
    return [([], np.zeros((int(np.ceil(float(snaps[0]["episode_len"]) * 15.0)) + 2, case.N * case.A, 6), np.int32))]


def build_stacked(case, snaps):
    """an arrangement with an item on another one: the lower first, the upper onto it (pitch raised: the point falls in y = 3); then a pick aimed at the
    covered lower item takes the upper one instead, which goes back"""
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        below = lambda u: [k for k in range(len(w.items)) if w.target(k) == (w.target(u)[0], 2, w.target(u)[2])][0]
        pairs = [(u, below(u)) for u in w.displaced() if w.target(u)[1] == 3]
        if not pairs:
            continue
        u, lo = pairs[0]
        if tuple(w.objects[lo][:3]) != w.target(lo):
            if not w.reachable(lo):
                continue
            w.move(0, lo, w.target(lo))
        if not w.reachable(u):
            continue
        t_up = w.move(0, u, w.target(u))
        x, _, z = w.target(lo)
        s = w.stand_for((x, z))
        w.objects[u][3], w.carry[0] = 1, u          # aimed at the lower item's voxel: the upper one comes
        t_cov = w.tick({0: (s[0], s[1], 0.0)})
        t_back = w.tick({0: w.place_act(0, w.target(u))})
        notes[w.e] = dict(t_up=t_up, t_covered=t_cov, t_back=t_back, upper=u, lower=lo)
    return finish(case, ws, notes)


REFUSALS = ("outside reach", "holds an item", "solid", "another agent's cell")


def build_refusals(case, snaps):
    """A = 2.  Agent 0 takes an item and tries to put it down where it must not: one cell outside +-2 of the centre; into a voxel that holds an item;
    into a solid voxel; into the voxel agent 1 stands in.  Nothing changes.  The only solid voxels within +-2 are the layer y = 1 under the pedestal, and
    a place point stays above y = 2.03 for an agent standing on it: the agent stands on the raised floor beside the pedestal's edge (x = 16.5) and looks
    slightly down, its point falls into (15, 1, z)."""
    assert case.A == 2
    ws, notes, todo = worlds(case, snaps), {}, list(REFUSALS)
    for w in ws:
        if not todo:
            break
        d = [i for i in w.displaced() if w.stand_for((w.objects[i][0], w.objects[i][2]))]
        if not d:
            continue
        rule = todo[0]
        if rule == "outside reach":
            zs = [z for z in range(3, 8) if not w.column((15, z))]
            if not zs:
                continue
            w.tick({0: w.pick_act(0, d[0])})
            zs = [z for z in range(3, 8) if not w.column((15, z))]
            t = w.tick({0: ((15, zs[0]), "+x", 0.0)})
        elif rule == "holds an item":
            w.tick({0: w.pick_act(0, d[0])})
            others = [k for k, o in enumerate(w.objects) if o[3] == 0 and w.stand_for((o[0], o[2]))]
            if not others:
                w.script.pop(); continue
            o = w.objects[others[0]]
            s = w.stand_for((o[0], o[2]))
            t = w.tick({0: (s[0], s[1], 0.0 if o[1] == 2 else PITCH_PLACE_UP)})
        elif rule == "solid":
            w.tick({0: w.pick_act(0, d[0])})
            t = w.tick({0: ("pose", w.e, 0, (16.87, TC.stand(1.5), 5.5), (0.0, 1.0), -0.1)})
        else:
            w.tick({0: w.pick_act(0, d[0])})
            pairs = [(c, w.stand_for(c)) for c in w.free_cells()]
            c, s = [(c, s) for c, s in pairs if s is not None][0]
            t = w.tick({0: (s[0], s[1], 0.0)}, idle={1: (c, "+x", 0.0)})
        notes[w.e] = dict(t_refused=t, rule=rule, item=d[0])
        todo.pop(0)
    assert not todo, todo
    return finish(case, ws, notes)


def build_descent(case, snaps):
    """a placement aimed at y = 3 over an empty column lands on y = 2"""
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        d = [i for i in w.displaced() if w.stand_for((w.objects[i][0], w.objects[i][2]))]
        if not d:
            continue
        w.tick({0: w.pick_act(0, d[0])})
        cells = [c for c in w.free_cells() if w.stand_for(c) and (c[0], 2, c[1]) != w.target(d[0])]
        if not cells:
            w.script.pop(); continue
        c = cells[0]
        t = w.tick({0: w.place_act(0, (c[0], 3, c[1]), settle=(c[0], 2, c[1]))})
        notes[w.e] = dict(t_place=t, item=d[0], cell=c)
    return finish(case, ws, notes)


def build_spirit(case, snaps):
    """A = 2, teamSpirit 0.5 for both: agent 1 earns the +1, rewardTeam shares it"""
    assert case.A == 2
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        i = floor_item(w)
        if i is None:
            continue
        w.tick(extra=[("shaping", w.e, a, {"teamSpirit": 0.5}) for a in range(2)])
        t = w.move(1, i, w.target(i))
        notes[w.e] = dict(t_place=t, item=i)
    return finish(case, ws, notes)


def build_wrong_colour(case, snaps):
    """an item is put on the free place of another item of its shape but of another colour: no match, nothing is paid"""
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        d = w.displaced()
        pairs = [(i, j) for i in d for j in d if i != j and w.items[i][0] == w.items[j][0] and w.items[i][1] != w.items[j][1] and w.target(j)[1] == 2
                 and w.stand_for((w.objects[i][0], w.objects[i][2])) and w.stand_for((w.target(j)[0], w.target(j)[2]))]
        if not pairs:
            continue
        i, j = pairs[0]
        t = w.move(0, i, w.target(j))
        notes[w.e] = dict(t_place=t, item=i, place_of=j)
    return finish(case, ws, notes)


def build_carried(case, snaps):
    """A = 2: agent 1 lifts an item off its matching cell and holds it; agent 0 puts another item in place -- as many match as did before, which pays
    nothing (a carried item does not count); then agent 1 puts its item back: one more than ever, +1"""
    assert case.A == 2
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        placed = [i for i, o in enumerate(w.objects) if tuple(o[:3]) == w.target(i) and w.at((o[0], o[1] + 1, o[2])) < 0 and w.reachable(i)]
        b = floor_item(w, more=1)
        if not placed or b is None:
            continue
        a = placed[0]
        w.tick({1: w.pick_act(1, a)})
        if not w.reachable(b) or w.stand_for((w.target(a)[0], w.target(a)[2])) is None:
            continue
        t = w.move(0, b, w.target(b))
        t_back = w.tick({1: w.place_act(1, w.target(a))})
        notes[w.e] = dict(t_place=t, t_back=t_back)
    return finish(case, ws, notes, tail=4)


def build_both(case, snaps):
    """A = 2: agent 0 puts everything in place but the last two items; then each agent takes one and both put theirs down on ONE tick -- agent 0 acts
    first and earns +1, agent 1's placement is the solving one: +1 and +10"""
    assert case.A == 2
    ws, notes = worlds(case, snaps), {}
    for w in ws:
        if len(w.displaced()) < 2:
            continue
        saved = ([list(o) for o in w.objects], list(w.script))
        last = solve_all(w, 0, leave=2)
        try:
            assert last is not None and all(w.reachable(i) for i in last)
            a0 = w.pick_act(0, last[0])
            w.tick({0: a0})
            a1 = w.pick_act(1, last[1])
            w.tick({1: a1})
            p0 = w.place_act(0, w.target(last[0]))
            p1 = w.place_act(1, w.target(last[1]), avoid=(p0[0], (w.target(last[0])[0], w.target(last[0])[2])))
            assert p0[0] != (w.target(last[1])[0], w.target(last[1])[2])
        except AssertionError:
            w.objects, w.script, w.carry = saved[0], saved[1], [-1] * w.A
            continue
        t = w.tick({0: p0, 1: p1})
        notes[w.e] = dict(t_both=t)
    return finish(case, ws, notes, tail=4)


# ---- the courier ---------------------------------------------------------------------------------------------------------------------------------

STRESS_TICKS = 300
STRESS_PARAMS = {"episodeLengthSec": 10.0}
STRESS_SEEDS = {1: 11, 4: 12}   # chosen on the CPU with the oracle (test_rearrange_model.py asserts the counts they give)


@functools.lru_cache(maxsize=None)
def courier_script(name):
    """The stress policy, computed ONCE from the CPU oracle's snapshots and recorded as setter calls and masks, so that every gym replays the identical
    script.  On most ticks every agent is teleported to a free pedestal cell, turned to one of the four axis directions plus an offset within +-0.3 rad,
    given a pitch and presses Interact; on the others it walks.  In the even envs most moves are errands (to the carried item's place, or to an item that
    lies wrong), so that episodes get solved; in the odd ones all are random, so that episodes time out.  On the tick an episode's timer runs out everybody
    walks."""
    import oracle_lib
    case = CASES[name]
    rng = np.random.default_rng(STRESS_SEEDS[case.A])
    g = case.make(oracle_lib.OracleGym)
    segs = []
    for t in range(STRESS_TICKS):
        cmds, act = [], np.zeros((1, case.N * case.A, 6), np.int32)
        for e in range(case.N):
            w = World(TC.snapshot(g, e), e, case.A)
            w.carry = [int(TC.snapshot(g, e)["agents"][a]["carrying"]) for a in range(case.A)]
            taken = []
            last = M.ends_without_interaction(M.State(TC.snapshot(g, e), case.A))   # the timer runs out on this tick: everybody walks, the finishing tick stays judged
            for a in range(case.A):
                if rng.random() < 0.1 or last:
                    act[0, e * case.A + a, 1] = 1
                    continue
                errand = None
                if e % 2 == 0 and rng.random() < 0.8:
                    if w.carry[a] >= 0:
                        v = w.target(w.carry[a])
                        if w.at(v) < 0 and (v[1] == 2 or w.at((v[0], 2, v[2])) >= 0):
                            s = w.stand_for((v[0], v[2]), taken)
                            errand = s and (s[0], s[1], (0.0 if v[1] == 2 else PITCH_PLACE_UP) + rng.uniform(-0.04, 0.04))
                    else:
                        wrong = [i for i in w.displaced() if w.at((w.objects[i][0], w.objects[i][1] + 1, w.objects[i][2])) < 0]
                        if wrong:
                            o = w.objects[wrong[int(rng.integers(len(wrong)))]]
                            s = w.stand_for((o[0], o[2]), taken)
                            errand = s and (s[0], s[1], (0.0 if o[1] == 2 else PITCH_PICK_UP) + rng.uniform(-0.04, 0.04))
                if not errand:
                    free = w.free_cells(taken)
                    errand = (free[int(rng.integers(len(free)))], NEIGHBOURS[int(rng.integers(4))][0], rng.uniform(-0.4, 0.7))
                taken.append(errand[0])
                cmds.append(pose(e, a, errand[0], errand[1], float(np.float32(errand[2])), float(rng.uniform(-0.3, 0.3))))
                act[0, e * case.A + a, 4] = 1
        TC.apply(g, cmds)
        for i in range(case.N * case.A):
            g.set_actions(i // case.A, i % case.A, act[0, i].tolist())
        TC.tick(g)
        segs.append((cmds, act))
    g.close()
    return segs


def make_stress(name):
    return lambda case, snaps: courier_script(name)


CASES = {c.name: c for c in (
    Case("match", 4, 1, build_match, replay=1),
    Case("solve", 8, 1, build_solve, replay=1),
    Case("timeout", 2, 1, build_timeout, params={"episodeLengthSec": 0.5}),
    Case("stacked", 8, 1, build_stacked, replay=1),
    Case("refusals", 8, 2, build_refusals),
    Case("descent", 2, 1, build_descent),
    Case("spirit", 4, 2, build_spirit, replay=1),
    Case("wrong_colour", 8, 1, build_wrong_colour),
    Case("carried", 8, 2, build_carried),
    Case("both", 8, 2, build_both, replay=1),
    Case("courier_a1", 8, 1, make_stress("courier_a1"), params=STRESS_PARAMS, scripted=False, replay=1),
    Case("courier_a4", 8, 4, make_stress("courier_a4"), params=STRESS_PARAMS, scripted=False, replay=1),
)}
