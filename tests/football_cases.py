"""What the Football tests share (CPU: test_oracle_football.py, GPU: test_football_parity_gpu.py): the chase-and-kick policy, the events a rollout has
to contain -- read from the ORACLE's records only --, and the scripted contact cases at the geometric edges of the sphere collider.  A case places
the agents and the ball through the debug hooks both gyms have, says what every agent does on every tick, and states what must have happened (checked
on the oracle alone, so a case cannot quietly stop exercising the edge it is named after)."""
import numpy as np

import football_model as M
from megaverse_amd.rollout import action_masks, sample_actions

F32 = np.float32
CAP_R, CAP_HH, BALL_R = 0.33, 0.525, 1.0
SUM_R = BALL_R + CAP_R
MAX_PEN_DEPTH = 0.041
WALK_PER_TICK = 4.5 / 15.0            # MAX_H_SPEED x dt
REST_Y = 1.0 + CAP_HH + CAP_R - 0.04   # capsule centre of an agent standing on the floor (canonical_frames.REST_Y)
ACT_FORWARD, ACT_INTERACT = 1 << 3, 1 << 8


def record(d):
    """MegaverseGym.debug_football_state's dict -> a football_model.STATE record (the oracle's football_state() already is one)"""
    s = np.zeros((), M.STATE)
    for k in ("pos", "radius", "vel", "kicks", "ang", "contacts", "force"):
        s[k] = d[k]
    return s


def chaser(snap, ball, A):
    """turn towards the ball, walk, kick: multi-discrete actions of one env's agents"""
    acts = np.zeros((A, 6), np.int32)
    for k in range(A):
        p, b = snap["agents"][k]["pos"], snap["agents"][k]["basis"]
        d = np.array([ball[0] - p[0], ball[2] - p[2]], np.float64)
        left = np.array([-b[0], b[1]], np.float64)
        side = float(d @ left) / (np.linalg.norm(d) + 1e-9)
        acts[k, 1] = 1
        acts[k, 2] = 1 if side > 0.15 else 2 if side < -0.15 else 0
        acts[k, 4] = 1
    return acts


def policy_actions(kind, og, N, A, seed, t):
    """[N * A, 6] actions of tick t.  "random": the counter-based random policy for everybody.  "chaser": even envs chase the ball and kick (from the
    ORACLE's state), odd envs act at random -- the mix of test_football_gpu.py's replay."""
    acts = sample_actions(seed, t, N * A).reshape(N, A, 6)
    if kind == "chaser":
        for e in range(0, N, 2):
            acts[e] = chaser(og.snapshot(e), og.football_state(e)["pos"], A)
    return acts.reshape(N * A, 6)


def capsule_ball_distance(p, c):
    """the capsule's centre p to the vertical segment of half-length CAP_HH through the ball's centre c (float64): the ball collider's distance
    before the summed radii are taken off"""
    qy = min(max(float(p[1]), float(c[1]) - CAP_HH), float(c[1]) + CAP_HH)
    return float(np.sqrt((float(p[0]) - float(c[0])) ** 2 + (float(p[1]) - qy) ** 2 + (float(p[2]) - float(c[2])) ** 2))


class Events:
    """what happened in a rollout, from the oracle's records: kicks, wall contacts (boxes 1..4), capsule contacts, resets, and ticks on which the ball
    stopped a walking agent -- Forward held, moved less than HALF a walking tick (stricter than "below the walk's"), and its capsule within 0.05 of
    touching the ball (distance to the ball's segment within 0.05 of the summed radii)"""

    def __init__(self):
        self.kicks = self.walls = self.capsules = self.resets = self.stopped = 0

    def tick(self, A, masks, before, after, ball, done):
        if done:
            self.resets += 1
            return
        self.kicks += int(ball["kicks"]) > 0
        self.walls += bool(int(ball["contacts"]) & (0xF << 9))
        self.capsules += bool(int(ball["contacts"]) & 0xFF)
        for i in range(A):
            p0, p1 = before["agents"][i]["pos"], after["agents"][i]["pos"]
            moved = float(np.hypot(float(p1[0]) - float(p0[0]), float(p1[2]) - float(p0[2])))
            if (int(masks[i]) & ACT_FORWARD) and moved < 0.5 * WALK_PER_TICK and abs(capsule_ball_distance(p1, ball["pos"]) - SUM_R) <= 0.05:
                self.stopped += 1

    def all_seen(self):
        return all(v > 0 for v in (self.kicks, self.walls, self.capsules, self.resets, self.stopped))

    def __repr__(self):
        return f"Events(kicks={self.kicks}, walls={self.walls}, capsules={self.capsules}, resets={self.resets}, stopped={self.stopped})"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scripted contacts.  Every room is at least 14 x 3 x 12 (interior 1..13 x 1..11): the cases stay inside x, z <= 10.

def facing(frm, to):
    """(cos, sin) of the yaw that looks from `frm` towards `to` in the xz plane: forward = (-sin, 0, -cos) (agent.cpp:135-150)"""
    dx, dz = float(to[0]) - float(frm[0]), float(to[2]) - float(frm[2])
    n = float(np.hypot(dx, dz))
    return float(F32(-dz / n)), float(F32(-dx / n))


def act(forward=False, interact=False):
    a = np.zeros(6, np.int32)
    a[1], a[4] = int(forward), int(interact)
    return a


class Case:
    def __init__(self, name, agents, ball, actions, expect, ball_kw=None):
        """agents: [(pos, facing target or None, (hvx, hvz, vvel))]; ball: its centre; ball_kw: vel / ang / force; actions: one per agent, held on
        every tick; expect(trace): asserts on the oracle's trace [(ball record, [agent pos], [agent snap records])] of every tick"""
        self.name, self.agents, self.ball, self.ball_kw, self.actions, self.expect = name, agents, ball, ball_kw or {}, actions, expect

    def place(self, g, env):
        """the same calls on the oracle's gym and on the device's"""
        set_ball = getattr(g, "set_football_state", None) or g.debug_set_football_state
        for k, (pos, look, vel) in enumerate(self.agents):
            g.debug_set_agent_pos(env, k, float(pos[0]), float(pos[1]), float(pos[2]))
            if look is not None:
                g.debug_set_agent_yaw(env, k, *facing(pos, look))
            g.debug_set_agent_velocity(env, k, *[float(v) for v in vel])
        set_ball(env, tuple(float(v) for v in self.ball), **self.ball_kw)


def _bits(x):
    return bin(int(x) & 0xFFFFFFFF).count("1")


def _finite(trace):
    for ball, pos, _ in trace:
        assert all(np.isfinite(ball[k]).all() for k in ("pos", "vel", "ang", "force")) and np.isfinite(np.array(pos)).all()


def _walk_in(trace):
    _finite(trace)
    assert any(int(b["contacts"]) & 1 for b, _, _ in trace)       # the ball felt the capsule
    gaps = [capsule_ball_distance(p[0], b["pos"]) - SUM_R for b, p, _ in trace]
    assert min(gaps) >= -(MAX_PEN_DEPTH + 0.045), min(gaps)         # the walk-in test's margin
    assert min(abs(g) for g in gaps) <= 0.05, gaps                  # and it did get to the ball (head-on it stays; at 45 degrees it slides round)


def _drop(kind):
    def check(trace):
        _finite(trace)
        touched = any(int(b["contacts"]) & 1 for b, _, _ in trace)
        ys = [float(p[0][1]) for _, p, _ in trace]
        stood = any(a[0]["vvel"] == 0.0 and a[0]["voffset"] == 0.0 and float(p[0][1]) > 3.0 for _, p, a in trace)   # at rest well above the floor
        if kind == "stands":
            assert touched and stood, (touched, stood)
        elif kind == "slides":
            assert touched and ys[-1] < 2.0, (touched, ys[-1])      # met the ball, ended on the floor
        else:
            assert not stood and ys[-1] < 2.0, ys[-1]                # past the ball, down to the floor
    return check


def _on_axis_ball(trace):
    _finite(trace)
    b, p, _ = trace[0]
    assert int(b["contacts"]) & 1                                    # the ball's contact search took the (1, 0, 0) fallback: pushed along +x only,
    assert float(b["pos"][0]) > 6.5 and float(b["pos"][2]) == 6.0   # 1.33 deep at ERP 0.8; the controller then meets it off its axis
    assert float(p[0][0]) < 6.0 and float(p[0][2]) == 6.0


def _on_axis_controller(trace):
    _finite(trace)
    b, p, _ = trace[0]
    assert int(b["contacts"]) == 0                                   # two units away at the start pose: no contact
    assert float(b["pos"][0]) == 6.0 and float(b["pos"][2]) == 6.0  # the ball flew exactly onto the capsule's axis (30 dt == 2 in float32) ...
    assert abs(float(p[0][0]) - (6.0 + SUM_R)) < 1e-5 and float(p[0][2]) == 6.0   # ... and the recovery's fallback normal pushed the capsule out along +x


def _ball_into_agent(trace):
    _finite(trace)
    assert any(int(b["contacts"]) & 1 for b, _, _ in trace)
    assert max(float(p[0][0]) for _, p, _ in trace) > 8.0 + 1e-3    # the standing agent was pushed out of the ball's new pose


def _corner(trace):
    _finite(trace)
    assert max(_bits(b["contacts"]) for b, _, _ in trace) >= 3       # two walls (or more) and the floor and / or the capsule at once
    assert any(int(b["kicks"]) == 1 and np.any(b["force"] != 0) for b, _, _ in trace)
    assert any(int(b["contacts"]) & 1 for b, _, _ in trace)


def _two_kick(trace):
    _finite(trace)
    both = [b for b, _, _ in trace if int(b["kicks"]) == 2]
    assert both and float(both[0]["force"][1]) == 70.0               # 2 x 70 x 0.5: the kicks add
    assert any((int(b["contacts"]) & 3) == 3 for b, _, _ in trace)  # both capsules, in index order, on one tick


def _between(trace):
    _finite(trace)
    # placed 0.33 deep in the ball and 0.077 deep in agent 1's capsule.  The ball's own push (ERP 0.8) takes it most of the way out, and the controller
    # still meets it deeper than MAX_PEN_DEPTH in the ball's new pose AND in the capsule: which one the recovery takes first is the colliders' order
    # (the ball, then the capsules), and the five alternating pushes end somewhere else if it is the other way round.  It ends clear of both.
    b, p, _ = trace[0]
    assert int(b["contacts"]) & 1 and not int(b["contacts"]) & 2
    assert capsule_ball_distance((7.0, REST_Y, 6.0), b["pos"]) - SUM_R < -MAX_PEN_DEPTH and float(np.hypot(0.5, 0.3)) - 2 * CAP_R < -MAX_PEN_DEPTH
    b, p, _ = trace[-1]
    assert capsule_ball_distance(p[0], b["pos"]) - SUM_R >= -(MAX_PEN_DEPTH + 0.045)
    assert float(np.hypot(float(p[0][0]) - float(p[1][0]), float(p[0][2]) - float(p[1][2]))) - 2 * CAP_R >= -(MAX_PEN_DEPTH + 0.045)


def _over_wall(trace):
    _finite(trace)
    assert all(int(b["contacts"]) == 0 and int(b["kicks"]) == 0 for b, _, _ in trace)
    assert float(trace[-1][0]["pos"][0]) < -1.0                      # outside the room


def scripted_cases():
    rest, still = (6.0, 2.0, 6.0), (0.0, 0.0, 0.0)
    cases = []
    for k in range(8):   # walking into the resting ball from eight headings
        ang = np.pi / 4 * k
        pos = (6.0 + 3.0 * float(np.cos(ang)), REST_Y, 6.0 + 3.0 * float(np.sin(ang)))
        cases.append(Case(f"walk_in_{45 * k}", [(pos, rest, still)], rest, [act(forward=True)], _walk_in))
    for off, kind in ((0.0, "stands"), (0.3, "stands"), (0.9, "slides"), (1.3, "misses")):   # dropped onto the ball: the down-sweep against the sphere
        cases.append(Case(f"drop_{off}", [((6.0 + off, 4.6, 6.0), None, still)], rest, [act()], _drop(kind)))
    cases.append(Case("on_axis_ball", [((6.0, 2.0, 6.0), None, still)], rest, [act()], _on_axis_ball))
    cases.append(Case("on_axis_controller", [((6.0, REST_Y, 6.0), None, still)], (4.0, 2.1, 6.0), [act()], _on_axis_controller, {"vel": (30.0, 0.0, 0.0)}))
    cases.append(Case("ball_into_agent", [((8.0, REST_Y, 6.0), None, still)], (5.5, 2.0, 6.0), [act()], _ball_into_agent, {"vel": (6.0, 0.0, 0.0)}))
    cases.append(Case("corner", [((3.2, REST_Y, 3.2), (2.0, 2.0, 2.0), still)], (2.0, 2.0, 2.0), [act(forward=True, interact=True)], _corner))
    cases.append(Case("two_kick", [((4.25, REST_Y, 6.0), rest, (4.5, 0.0, 0.0)), ((7.75, REST_Y, 6.0), rest, (-4.5, 0.0, 0.0))], rest,
                      [act(forward=True, interact=True)] * 2, _two_kick))
    cases.append(Case("between_ball_and_capsule", [((7.0, REST_Y, 6.0), None, still), ((7.5, REST_Y, 6.3), None, still)], rest, [act()] * 2, _between))
    cases.append(Case("over_wall", [((10.0, REST_Y, 9.0), None, still)], (4.0, 2.5, 6.0), [act()], _over_wall, {"force": (-300.0, 1500.0, 0.0)}))
    return cases


def run_on_oracle(og, cases, ticks, after_tick=None):
    """place every case in its env (env k = case k), step `ticks` times; -> one trace per case.  after_tick(t): the caller's own checks"""
    A = og.num_agents_per_env
    for e, c in enumerate(cases):
        c.place(og, e)
    masks = action_masks(np.stack([a for c in cases for a in c.actions]))
    traces = [[] for _ in cases]
    for t in range(ticks):
        og.set_action_masks(masks)
        og.step_norender()
        for e in range(len(cases)):
            s = og.snapshot(e)
            traces[e].append((og.football_state(e), [s["agents"][i]["pos"].copy() for i in range(A)], [s["agents"][i].copy() for i in range(A)]))
        if after_tick:
            after_tick(t)
    return traces
