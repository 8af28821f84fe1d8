#!/usr/bin/env python3
"""Measurements of the overview cameras (mv_set_overview) on one MI355X -> profiles/overview_measured.txt (or --out).

1. bench.py with nothing attached, the parent commit against this one, --runs alternating runs each (--parent DIR: a checkout of the parent with its library
   built; without it this part is skipped and said so).  Acceptance: this commit's median inside the parent's own range.
2. 1024 envs at 128 x 128, TowerBuilding / ObstaclesHard / HexMemory, one agent per env: the time of one mv_draw_overview with every camera at
   follow(0, first_person=True) -- the agents' own frames -- beside one exact-mode mv_render of the same gym (the pass an existing caller launches: its kernels
   are the parent's, profiles/overview_resources.txt); then the default pose and the chase pose follow(0, back=2, up=1), where lists are longer.
3. The same draws in env order (MV_OVERVIEW_ORDER=0: no frame-order launch) against the cost-bin order, each in a child process of its own.
Times are device events around --reps calls after --warmup, per call, the median of --rounds rounds.  Every child runs under its own time limit; the first one
that fails ends the script."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ("TowerBuilding", "ObstaclesHard", "HexMemory")


def child(args):
    """one scenario in this process -> one JSON line"""
    sys.path.insert(0, ROOT)
    import torch
    from megaverse_amd import follow, overview_default_camera
    from megaverse_amd.extension import MegaverseGym
    N, W, H = args.envs, args.obs[0], args.obs[1]
    g = MegaverseGym(args.child, W, H, N, 1, 1, False, {})
    g.set_pixel_mode("exact"); g.seed(42); g.reset()
    for t in range(40):
        g.sample_random_actions(7, t); g.step_no_render()
    g.set_overview(W, H)

    def timed(fn):
        rounds = []
        for _ in range(args.rounds):
            for _ in range(args.warmup):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record(); torch.cuda.synchronize()
            rounds.append(a.elapsed_time(b) * 1000.0 / args.reps)
        return {"median_us": statistics.median(rounds), "min_us": min(rounds), "max_us": max(rounds)}
    out = {"scenario": args.child, "envs": N, "obs": [W, H], "capacity": g.overview_capacity(), "cost_order": os.environ.get("MV_OVERVIEW_ORDER", "1") != "0"}
    out["mv_render exact"] = timed(g.render)
    for name, cam in (("follow(0, first_person)", follow(0, first_person=True)), ("default pose", overview_default_camera()), ("chase follow(0, 2, 1)", follow(0, back=2.0, up=1.0))):
        g.set_overview_cameras(cam)
        out[name] = timed(g.draw_overview)
    out["dropped"] = list(g.overview_dropped())
    g.close()
    print("OVERVIEW_BENCH " + json.dumps(out), flush=True)


def run(cmd, limit, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {p.returncode}; nothing more is started")
    return p.stdout


def bench_value(tree, steps, warmup, limit):
    env = dict(os.environ)
    env.pop("MV_LIB_PATH", None)
    out = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extra-legs"], limit, env)
    rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return float(rec["value"]), rec.get("unit", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--obs", type=int, nargs=2, default=[128, 128])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overview_measured.txt"))
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = ["Overview cameras, measured by scripts/overview_bench.py on one MI355X.", ""]
    if args.parent:
        vals = {"parent": [], "this": []}
        unit = ""
        for _ in range(args.runs):
            for tag, tree in (("parent", args.parent), ("this", ROOT)):
                v, unit = bench_value(tree, args.steps, args.bench_warmup, args.limit)
                vals[tag].append(v)
                print(f"bench.py {tag}: {v:.4g} {unit}", flush=True)
        lo, hi, med = min(vals["parent"]), max(vals["parent"]), statistics.median(vals["this"])
        lines += [f"1. bench.py --gpus 1 --steps {args.steps} --warmup {args.bench_warmup}, nothing attached, {args.runs} alternating runs ({unit}):",
                  "   parent: " + " ".join(f"{v:.4g}" for v in vals["parent"]) + f"   median {statistics.median(vals['parent']):.4g}, range {lo:.4g} .. {hi:.4g}",
                  "   this:   " + " ".join(f"{v:.4g}" for v in vals["this"]) + f"   median {med:.4g}",
                  f"   this commit's median is {'INSIDE' if lo <= med <= hi else 'OUTSIDE'} the parent's own range"
                  + ("" if lo <= med <= hi else f" ({(med / statistics.median(vals['parent']) - 1) * 100:+.2f} % against the parent's median)"), ""]
    else:
        lines += ["1. bench.py, parent against this commit: NOT RUN (no --parent checkout given).", ""]
    lines.append(f"2./3. {args.envs} envs at {args.obs[0]} x {args.obs[1]}, one agent per env, exact pixel mode; us per call, median (min .. max) of {args.rounds} rounds of {args.reps} calls:")
    for scen in SCENARIOS:
        for order in ("1", "0"):
            env = dict(os.environ, MV_OVERVIEW_ORDER=order)
            out = run([sys.executable, os.path.abspath(__file__), "--child", scen, "--envs", str(args.envs), "--obs", str(args.obs[0]), str(args.obs[1]),
                       "--reps", str(args.reps), "--warmup", str(args.warmup), "--rounds", str(args.rounds)], args.limit, env)
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("OVERVIEW_BENCH ")][-1][len("OVERVIEW_BENCH "):])
            print(f"measured {scen}, MV_OVERVIEW_ORDER={order}", flush=True)
            lines.append(f"   {scen} (list capacity {rec['capacity']}), {'cost-bin order' if rec['cost_order'] else 'env order, no frame-order launch'}; dropped {rec['dropped']}:")
            for k in ("mv_render exact", "follow(0, first_person)", "default pose", "chase follow(0, 2, 1)"):
                r = rec[k]
                lines.append(f"      {k:26s} {r['median_us']:9.1f}  ({r['min_us']:.1f} .. {r['max_us']:.1f})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
