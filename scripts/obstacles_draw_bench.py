#!/usr/bin/env python
"""What drawing the Obstacles family's episodes on the device costs and buys (megaverse_amd/csrc/mv_obstacles_draw.h, MV_OBSTACLES_DEVICE_GEN=1).  Needs a GPU;
reads nothing outside the tree but --parent.

  draws    obstacles_draw_kernel alone (mv_debug_obstacles_draw_device): ms per launch of --envs episodes and episodes per second, ObstaclesEasy and
           ObstaclesHard, --runs runs of 3 launches each (HIP events around the launches); min, median and max over the runs.
  seed     mv_seed_envs_host of ALL --envs ObstaclesEasy envs, host-fed against device-fed (this tree, the switch set before the gym is made): every call timed
           on its own with the host's clock, the device idle before it, from the call to the end of a synchronise behind it (scripts/seed_envs_bench.py's
           method); mean and minimum over --calls calls.
  hard     bench.py --scenario ObstaclesHard (--envs envs, 128 x 128, bench.py's launch shape): host-fed in a checkout of the PARENT commit (--parent DIR,
           built) against device-fed in this tree, alternated, --hard-runs runs each -- once with every CPU the process may use and once pinned to two cores
           (taskset -c 0-1, the share of a rank at eight ranks).
  bench    python bench.py with nothing switched on, parent against this tree, --runs alternating runs each: the headline must not move -- this tree's
           median inside the parent's own min .. max.

The figures go to --out (default profiles/obstacles_draw_measured.txt) as they are measured, one JSON line each under a header that states the method.
    python scripts/obstacles_draw_bench.py [--what draws|seed|hard|bench|all] [--parent DIR] [--out FILE]
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

SIZE = 128
HEADER = """# Obstacles-family episodes drawn on the device (obstacles_draw_kernel, MV_OBSTACLES_DEVICE_GEN=1) on one MI355X, written by scripts/obstacles_draw_bench.py:
# one JSON line per figure.
# what = draws: mv_debug_obstacles_draw_device, {envs} env seeds, 1 agent; one run = 3 launches of {envs} episodes between two HIP events, ms = the mean launch
#   of the run; min / median / max over the runs of the line.  A launch of {envs} episodes has 256 waves draw 4 episodes each (one grid region per wave).
# what = seed: ONE mv_seed_envs_host call naming all {envs} ObstaclesEasy envs, {size} x {size}, timed on its own with the host's clock from the call to the end
#   of a synchronise behind it, the device idle before it; every call gets fresh seeds and is followed by one untimed step.  mean / min over the calls.
# what = hard: the value of bench.py --scenario ObstaclesHard (M agent observations/s), host-fed in the parent commit's tree against device-fed in this one,
#   alternated in one session; cpus = all: no pinning; cpus = 0-1: taskset -c 0-1 around the whole run.
# what = bench: bench.py's headline with nothing switched on, parent commit and this tree alternated, the same box, the same session.
# Not measured: several agents per env, several GPUs, members of an mv_group, the other four Obstacles names and Empty in bench.py's shape.
"""


def stats3(xs):
    return {"min": round(min(xs), 3), "median": round(statistics.median(xs), 3), "max": round(max(xs), 3), "runs": len(xs)}


def bench_draws(args, emit):
    import numpy as np
    from megaverse_amd import extension as ext
    lib = ext.load_library()
    record = lib.mv_debug_obstacles_draw_host(b"ObstaclesHard", 1, 0, 1, 60.0, None, 0)
    seeds = (np.arange(args.envs, dtype=np.int64) * 7919 + 13).astype(np.int32)
    out = np.zeros(args.envs * record, np.uint8)
    ms = np.zeros(1, np.float32)
    for name in ("ObstaclesEasy", "ObstaclesHard"):
        runs = []
        for r in range(args.runs + 1):
            rc = lib.mv_debug_obstacles_draw_device(0, name.encode(), 1, seeds.ctypes.data, args.envs, 3, 60.0, out.ctypes.data, out.nbytes, ms.ctypes.data)
            if rc != 0:
                emit({"what": "draws", "scenario": name, "failed": rc})
                return False   # (a failed HIP call can be a device fault: nothing more is started on this GPU)
            if r > 0:   # (the first run warms the device up)
                runs.append(float(ms[0]))
        s = stats3(runs)
        emit({"what": "draws", "scenario": name, "episodes_per_launch": args.envs, "ms_per_launch": s,
              "k_episodes_per_s": {"min": round(args.envs / s["max"], 1), "median": round(args.envs / s["median"], 1), "max": round(args.envs / s["min"], 1)}})
    return True


def bench_seed(args, emit):
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    N = args.envs
    for device in (False, True, False, True):
        os.environ["MV_OBSTACLES_DEVICE_GEN"] = "1" if device else "0"
        g = MegaverseGym("ObstaclesEasy", SIZE, SIZE, N, 1, 0, False, {})
        g.set_pixel_mode("fast")
        g.seed(42); g.reset()
        for t in range(8):
            g.sample_random_actions(7, t); g.step()
        g.synchronize()
        host = []
        for i in range(args.warmup + args.calls):
            words = ((1000 * (i + 1) + np.arange(N)) % (1 << 30)).astype(np.int32)
            g.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.seed_envs(words)
            g.synchronize(); torch.cuda.synchronize()
            if i >= args.warmup:
                host.append((time.perf_counter() - t0) * 1e6)
            g.sample_random_actions(7, 100 + i); g.step()
        emit({"what": "seed", "scenario": "ObstaclesEasy", "fed": "device" if device else "host", "envs": N, "flagged": N, "calls": len(host),
              "host_us_mean": round(sum(host) / len(host), 1), "host_us_min": round(min(host), 1), "host_us_max": round(max(host), 1),
              "host_generator_threads": g.host_generator_threads(), "device_generator": g.device_generator()})
        g.close()
    os.environ.pop("MV_OBSTACLES_DEVICE_GEN", None)


def run_bench(args, tree, extra, env, pin):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.bench_warmup)] + args.bench_args.split() + extra
    if pin:
        cmd = ["taskset", "-c", pin] + cmd
    out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=args.bench_timeout, env=env)
    if out.returncode != 0:
        return None, {"failed": out.returncode, "stderr": out.stderr[-400:]}
    line = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    return line, None


def alternate(args, emit, what, extra, this_env, pin, runs):
    values = {"parent": [], "this": []}
    base = {k: v for k, v in os.environ.items() if k != "MV_OBSTACLES_DEVICE_GEN"}
    for r in range(runs):
        for name, tree, env in (("parent", os.path.abspath(args.parent), base), ("this", ROOT, dict(base, **this_env))):
            line, err = run_bench(args, tree, extra, env, pin)
            if err:
                emit(dict({"what": what, "tree": name, "run": r, "cpus": pin or "all"}, **err))
                return False   # (whatever made a run fail is not run again)
            values[name].append(round(float(line["value"]), 3))
            emit({"what": what, "tree": name, "run": r, "cpus": pin or "all", "value": values[name][-1], "unit": line.get("unit"),
                  "host_generator_threads": line.get("host_generator_threads")})
    p, t = values["parent"], values["this"]
    emit({"what": what, "summary": True, "cpus": pin or "all", "parent": stats3(p), "this": stats3(t),
          "this_median_inside_parent_range": min(p) <= statistics.median(t) <= max(p),
          "this_median_vs_parent_median_pct": round((statistics.median(t) / statistics.median(p) - 1) * 100, 2)})
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", help="comma-separated: draws, seed, hard, bench, all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default="", help="hard, bench: a built checkout of the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--hard-runs", type=int, default=3, help="hard: runs per tree and pinning")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--bench-args", default="--no-cpu-baseline --no-extra-legs", help="further arguments of both trees' bench.py runs")
    ap.add_argument("--bench-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacles_draw_measured.txt"))
    args = ap.parse_args()
    what = set(args.what.split(","))
    everything = "all" in what
    fresh = not os.path.exists(args.out)
    f = open(args.out, "a")
    if fresh:
        f.write(HEADER.format(envs=args.envs, size=SIZE))

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    if (everything or "draws" in what) and not bench_draws(args, emit):
        f.close()
        sys.exit("obstacles_draw_bench: a draw launch failed; stopping")
    if everything or "seed" in what:
        bench_seed(args, emit)
    if everything or what & {"hard", "bench"}:
        if not args.parent or not os.path.exists(os.path.join(args.parent, "bench.py")):
            emit({"what": "hard / bench", "skipped": "no --parent checkout"})
        else:
            ok = True
            if everything or "bench" in what:
                ok = alternate(args, emit, "bench", [], {}, "", args.runs)
            if ok and (everything or "hard" in what):
                hard = ["--scenario", "ObstaclesHard", "--envs-per-gpu", str(args.envs)]
                ok = alternate(args, emit, "hard", hard, {"MV_OBSTACLES_DEVICE_GEN": "1"}, "", args.hard_runs)
                ok = ok and alternate(args, emit, "hard", hard, {"MV_OBSTACLES_DEVICE_GEN": "1"}, "0-1", args.hard_runs)
    f.close()


if __name__ == "__main__":
    main()
