#!/usr/bin/env python
"""What still frames cost and buy (include/megaverse_hip.h: mv_set_still_frames).  Needs a GPU; reads nothing outside the tree.

  bench      nothing switched on: bench.py --gpus 1 of the tree given with --parent against this tree's, --reps alternating runs each (child processes).  The
             commit's median must lie inside or above the parent's own min .. max.
  sequence   16-tick rendered step_n calls with 100 / 50 / 0 % of the envs stepping (a step mask), with an output ring of 16 and without one, option off
             against on, TowerBuilding and HexMemory, --envs x 1 agent at --size x --size -> us per tick.
  episodes   MegaverseEnv.run_episodes(1, render='every'), off against on -> ms per run (short episodes: --episode-sec).
  planner    the savepoint planner: env 0 frozen, per iteration fork(0) into every other env + step_n(16, render='last'), off against on -> us per iteration.
  closed     the closed loop: mv_step into a ring of 2 with every env stepping, off against on -> us per step (on: the extra carry launch).

One gym is alive at a time: every repetition creates a gym, measures it (a host clock around --calls calls that end in a device synchronise, after --warmup
calls) and closes it, off and on in turn, --reps repetitions each: median [min .. max].  No threshold is set but bench's.  Not measured here: several
agents per env, several GPUs.

JSON lines on stdout; the report is appended to --out (default profiles/still_frames_measured.txt) under --label.
    python scripts/still_frames_bench.py [--what bench|sequence|episodes|planner|closed|all] [--parent DIR] [--label text]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 16


def make_gym(MegaverseGym, scenario, N, S, still):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    if still:
        g.set_still_frames(True)
    return g


def timed(g, call, calls, warmup):
    """seconds of `calls` back-to-back calls, the last one waited for"""
    import torch
    for _ in range(warmup):
        call()
    g.synchronize(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    g.synchronize(); torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def alternate(args, make_form, per_call):
    """make_form(still) -> (gym, call, what the call's buffers are held by): one gym alive at a time, created, measured and closed once per repetition, off and
    on in turn -- two gyms of one process that live side by side land 10 - 30 % apart whichever option they have, by the order they were created in
    (profiles/macro_step_measured.txt saw the same) -> {name: stats of us per `per_call`-th of a call}"""
    us = {"off": [], "on": []}
    for _ in range(args.reps):
        for f in us:
            g, call, held = make_form(f == "on")
            us[f].append(timed(g, call, args.calls, args.warmup) / (args.calls * per_call) * 1e6)
            g.close()
            del held
    return {f: stats(v) for f, v in us.items()}


def run_bench(args, emit):
    if not args.parent:
        emit({"what": "bench", "unmeasured": "no --parent tree given"})
        return
    rates = {"parent": [], "this": []}
    for _ in range(args.reps):
        for name, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                               cwd=tree, capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                emit({"what": "bench", "failed": name, "stderr": r.stderr[-400:]})
                return
            rates[name].append(json.loads(line[-1])["value"])
    p, t = stats(rates["parent"]), stats(rates["this"])
    emit({"what": "bench", "steps": args.bench_steps, "obs_per_sec": {"parent": p, "this": t}, "runs": rates,
          "median_inside_or_above_parents_range": t["median"] >= p["min"]})


def run_sequence(args, torch, MegaverseGym, emit):
    N, S = args.envs, args.size
    for scenario in args.scenarios:
        for ring in (K, 0):
            for percent in (100, 50, 0):
                def make_form(still, scenario=scenario, ring=ring, percent=percent):
                    held = []
                    g = make_gym(MegaverseGym, scenario, N, S, still)
                    if ring:
                        bufs = (torch.zeros((ring, N, S, S, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((ring, N), dtype=torch.float32, device="cuda:0"),
                                torch.zeros((ring, N), dtype=torch.uint8, device="cuda:0"))
                        g.set_output_ring(ring, *(b.data_ptr() for b in bufs))
                        held.append(bufs)
                    if percent < 100:
                        mask = (torch.arange(N, device="cuda:0") % 100) < percent
                        g.set_step_mask(mask)
                        held.append(mask)
                    step = [0]

                    def call(g=g, step=step):
                        g.step_n(K, "multidiscrete", 7, step[0])
                        step[0] += K
                    return g, call, held
                emit({"what": "sequence", "scenario": scenario, "envs": N, "size": S, "ring": ring, "percent_stepping": percent,
                      "us_per_tick": alternate(args, make_form, K)})


def run_episodes(args, torch, emit):
    from megaverse_amd.megaverse_env import MegaverseEnv
    ms = {"off": [], "on": []}
    for _ in range(args.reps):
        for name in ms:
            env = MegaverseEnv("TowerBuilding", args.envs, 1, params={"episodeLengthSec": args.episode_sec}, img_w=args.size, img_h=args.size,
                               still_frames=name == "on")
            env.env.seed(42)
            env.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = env.run_episodes(1, render="every", seed=3)
            env.env.synchronize(); torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            n = len(rec)
            env.close() if hasattr(env, "close") else env.env.close()
    emit({"what": "episodes", "envs": args.envs, "size": args.size, "episode_sec": args.episode_sec, "records": n, "ms_per_run": {f: stats(v) for f, v in ms.items()}})


def run_planner(args, torch, MegaverseGym, emit):
    N, S = args.envs, args.size
    def make_form(still):
        g = make_gym(MegaverseGym, "TowerBuilding", N, S, still)
        mask = torch.ones(N, dtype=torch.bool, device="cuda:0")
        mask[0] = False
        src = torch.zeros(N, dtype=torch.int32, device="cuda:0")
        src[0] = -1
        g.set_step_mask(mask)
        step = [0]

        def call(g=g, step=step, src=src):
            g.fork_envs(src)
            g.step_n(K, "multidiscrete", 7, step[0], render="last")
            step[0] += K
        return g, call, [mask, src]
    emit({"what": "planner", "envs": N, "size": S, "ticks_per_iteration": K, "us_per_iteration": alternate(args, make_form, 1)})


def run_closed(args, torch, MegaverseGym, emit):
    N, S = args.envs, args.size
    def make_form(still):
        g = make_gym(MegaverseGym, "TowerBuilding", N, S, still)
        bufs = (torch.zeros((2, N, S, S, 4), dtype=torch.uint8, device="cuda:0"), torch.zeros((2, N), dtype=torch.float32, device="cuda:0"),
                torch.zeros((2, N), dtype=torch.uint8, device="cuda:0"))
        g.set_output_ring(2, *(b.data_ptr() for b in bufs))
        step = [0]

        def call(g=g, step=step):
            g.sample_random_actions(7, step[0])
            g.step()
            step[0] += 1
        return g, call, bufs
    emit({"what": "closed", "envs": N, "size": S, "us_per_step": alternate(args, make_form, 1)})


def fmt(v, digits=2):
    return f"{v['median']:.{digits}f} [{v['min']:.{digits}f} .. {v['max']:.{digits}f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["all"], choices=("bench", "sequence", "episodes", "planner", "closed", "all"))
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit (bench)")
    ap.add_argument("--scenarios", nargs="+", default=["TowerBuilding", "HexMemory"])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--episode-sec", type=float, default=10.0)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "still_frames_measured.txt"))
    args = ap.parse_args()
    what = set(args.what)
    if "all" in what:
        what = {"bench", "sequence", "episodes", "planner", "closed"}
    lines = []

    def emit(rec):
        rec["label"] = args.label
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    if "bench" in what:   # (child processes: before this process opens the device)
        run_bench(args, emit)
    if what - {"bench"}:
        import torch
        from megaverse_amd.extension import MegaverseGym
        if "sequence" in what:
            run_sequence(args, torch, MegaverseGym, emit)
        if "episodes" in what:
            run_episodes(args, torch, emit)
        if "planner" in what:
            run_planner(args, torch, MegaverseGym, emit)
        if "closed" in what:
            run_closed(args, torch, MegaverseGym, emit)
    with open(args.out, "a") as f:
        f.write(f"\n== {args.label}: scripts/still_frames_bench.py --what {' '.join(sorted(what))} --envs {args.envs} --size {args.size} --reps {args.reps} "
                f"--calls {args.calls} (median [min .. max] over the repetitions)\n")
        for rec in lines:
            w = rec["what"]
            if "unmeasured" in rec or "failed" in rec:
                f.write(f"{w:<9} UNMEASURED: {rec.get('unmeasured') or 'bench.py failed in the ' + rec['failed'] + ' tree'}\n")
            elif w == "bench":
                o = rec["obs_per_sec"]
                f.write(f"bench     bench.py --gpus 1 --steps {rec['steps']}, M obs/s: parent {fmt({k: v / 1e6 for k, v in o['parent'].items()}, 3)}   this commit "
                        f"{fmt({k: v / 1e6 for k, v in o['this'].items()}, 3)}   median inside or above the parent's range: {rec['median_inside_or_above_parents_range']}\n")
            elif w == "sequence":
                u = rec["us_per_tick"]
                f.write(f"sequence  {rec['scenario']:<14} {'ring 16' if rec['ring'] else 'no ring'}  {rec['percent_stepping']:>3} % stepping  us per tick: off {fmt(u['off'])}   "
                        f"on {fmt(u['on'])}   off / on {u['off']['median'] / u['on']['median']:.2f}\n")
            elif w == "episodes":
                u = rec["ms_per_run"]
                f.write(f"episodes  run_episodes(1, render='every'), episodes of {rec['episode_sec']} s, {rec['records']} records, ms per run: off {fmt(u['off'])}   on {fmt(u['on'])}   "
                        f"off / on {u['off']['median'] / u['on']['median']:.2f}\n")
            elif w == "planner":
                u = rec["us_per_iteration"]
                f.write(f"planner   fork(0) + step_n(16, render='last') from a frozen root, us per iteration: off {fmt(u['off'], 1)}   on {fmt(u['on'], 1)}   "
                        f"off / on {u['off']['median'] / u['on']['median']:.2f}\n")
            elif w == "closed":
                u = rec["us_per_step"]
                f.write(f"closed    mv_step into a ring of 2, every env stepping, us per step: off {fmt(u['off'])}   on {fmt(u['on'])}   "
                        f"on - off {u['on']['median'] - u['off']['median']:.2f}\n")


if __name__ == "__main__":
    main()
