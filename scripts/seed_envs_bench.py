#!/usr/bin/env python
"""What a level seed costs (include/megaverse_hip.h: mv_seed_envs / mv_seed_envs_host).  Needs a GPU; reads nothing outside the tree but --parent.

  calls    time per call at --envs envs x 128 x 128 with 1 env flagged and with all envs flagged: TowerBuilding in the host and the device form,
           ObstaclesEasy and HexMemory in the host form.  Every call is timed on its own with the host's clock, the device idle before it, from the call to
           the end of a synchronise behind it -- the host-fed host form waits on the host by contract, so a stream interval would miss most of it; for
           TowerBuilding the stream interval between two HIP events is reported too.  Each call gets fresh seeds and is followed by one untimed step and a
           synchronise; the device form's tensor is filled before the timed interval.  Mean and minimum over --calls calls.
  start    start_levels of all envs (seed_envs + reset_envs, render on) beside mv_seed + mv_reset on the same gym, alternated, timed the same way.
  bench    python bench.py in a checkout of the PARENT commit (--parent DIR, built) and in this tree, --runs alternating runs each: the headline must not
           move; the parent's own spread is the margin.

The figures go to --out (default profiles/seed_envs_measured.txt) as they are measured, one JSON line each under a header that states the method.
    python scripts/seed_envs_bench.py [--what calls|start|bench|all] [--parent DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 128
HEADER = """# Level seeds (mv_seed_envs / mv_seed_envs_host) on one MI355X, written by scripts/seed_envs_bench.py: one JSON line per figure.
# {envs} envs, 1 agent per env, {size} x {size} frames, fast pixels, pipelined, 8 random-action ticks before the first call.
# what = call: ONE call timed on its own, the device idle before it.  host_us: the host's clock from the call to the end of a synchronise behind it (the
#   host-fed host form waits on the host by contract: this is its cost).  stream_us (TowerBuilding): two HIP events on the gym's stream around the call.
#   Every call gets fresh seeds (the device form's tensor is filled before the interval) and is followed by one untimed step and a synchronise.  mean / min
#   over {calls} calls after {warmup}.
# what = start: start_levels of ALL envs (mv_seed_envs_host + mv_reset_envs_host, render on) beside mv_seed + mv_reset on the same gym, alternated, host clock
#   as above.
# what = bench: the value of bench.py's result line (M agent observations/s), parent commit and this tree alternated, the same box, the same session.
# Not measured: several agents per env, several GPUs, members of an mv_group, batch sizes other than {envs}, Collect and Sokoban (the feeder's Sokoban
#   undo and Collect's device generator are exercised by the tests only).
"""


def make_gym(MegaverseGym, scenario, N):
    g = MegaverseGym(scenario, SIZE, SIZE, N, 1, 0, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    for t in range(8):
        g.sample_random_actions(7, t)
        g.step()
    g.synchronize()
    return g


def stats(xs):
    return round(sum(xs) / len(xs), 2), round(min(xs), 2)


def timed(torch, g, fn, calls, warmup, stream_too=False, prepare=None):
    host, stream = [], []
    for i in range(warmup + calls):
        if prepare is not None:
            prepare(i)   # (untimed: this call's arguments, a device tensor filled)
        g.synchronize()
        torch.cuda.synchronize()
        if stream_too:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        t0 = time.perf_counter()
        fn(i)
        if stream_too:
            b.record()
        g.synchronize()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e6
        if i >= warmup:
            host.append(dt)
            if stream_too:
                stream.append(a.elapsed_time(b) * 1e3)
        g.sample_random_actions(7, 100 + i)
        g.step()
    return host, stream


def bench_calls(args, emit, torch, MegaverseGym, np):
    N = args.envs
    for scenario, forms in (("TowerBuilding", ("host", "device")), ("ObstaclesEasy", ("host",)), ("HexMemory", ("host",))):
        g = make_gym(MegaverseGym, scenario, N)
        for form in forms:
            for flagged in (1, N):
                envs = np.linspace(0, N - 1, flagged).astype(np.int64)
                dev = torch.full((N,), -1, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()

                words = np.full(N, -1, np.int32)

                def prepare(i):
                    words[envs] = (1000 * (i + 1) + envs) % (1 << 30)
                    if form == "device":
                        dev.copy_(torch.as_tensor(words), non_blocking=False)

                def call(i):
                    g.seed_envs(dev if form == "device" else words)

                host, stream = timed(torch, g, call, args.calls, args.warmup, stream_too=scenario == "TowerBuilding", prepare=prepare)
                line = {"what": "call", "scenario": scenario, "form": form, "envs": N, "flagged": int(flagged), "calls": args.calls,
                        "host_us_mean": stats(host)[0], "host_us_min": stats(host)[1], "host_generator_threads": g.host_generator_threads()}
                if stream:
                    line["stream_us_mean"], line["stream_us_min"] = stats(stream)
                emit(line)
        g.close()


def bench_start(args, emit, torch, MegaverseGym, np):
    N = args.envs
    for scenario in ("TowerBuilding", "ObstaclesEasy", "HexMemory"):
        g = make_gym(MegaverseGym, scenario, N)
        ones = np.ones(N, np.bool_)

        def start(i):
            g.seed_envs(((1000 * (i + 1) + np.arange(N)) % (1 << 30)).astype(np.int32))
            g.reset_envs(ones, render=True)

        def whole(i):
            g.seed(1000 + i)
            g.reset()

        res = {"start_levels": [], "seed_reset": []}
        for _ in range(2):
            for name, fn in (("start_levels", start), ("seed_reset", whole)):
                res[name] += timed(torch, g, fn, args.calls // 2, args.warmup)[0]
        emit({"what": "start", "scenario": scenario, "envs": N, "calls": len(res["start_levels"]),
              "start_levels_us_mean": stats(res["start_levels"])[0], "start_levels_us_min": stats(res["start_levels"])[1],
              "seed_reset_us_mean": stats(res["seed_reset"])[0], "seed_reset_us_min": stats(res["seed_reset"])[1]})
        g.close()


def bench_headline(args, emit):
    if not args.parent or not os.path.exists(os.path.join(args.parent, "bench.py")):
        emit({"what": "bench", "skipped": "no --parent checkout"})
        return
    values = {"parent": [], "this": []}
    for r in range(args.runs):
        for name, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.bench_warmup)] + args.bench_args.split(),
                                 cwd=tree, capture_output=True, text=True, timeout=args.bench_timeout)
            if out.returncode != 0:
                emit({"what": "bench", "tree": name, "run": r, "failed": out.returncode, "stderr": out.stderr[-400:]})
                return   # (whatever made a run fail is not run again)
            line = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
            values[name].append(round(float(line["value"]), 3))
            emit({"what": "bench", "tree": name, "run": r, "value": values[name][-1], "unit": line.get("unit")})
    p, t = values["parent"], values["this"]
    emit({"what": "bench", "summary": True, "parent": p, "this": t, "parent_spread_pct": round((max(p) - min(p)) / min(p) * 100, 2),
          "this_min_vs_parent_min_pct": round((min(t) - min(p)) / min(p) * 100, 2), "this_mean_vs_parent_mean_pct": round((sum(t) / len(t) - sum(p) / len(p)) / (sum(p) / len(p)) * 100, 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["calls", "start", "bench", "all"], default="all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--parent", default="", help="bench: a built checkout of the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--bench-args", default="--no-cpu-baseline --no-extra-legs", help="further arguments of both trees' bench.py runs")
    ap.add_argument("--bench-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_envs_measured.txt"))
    args = ap.parse_args()
    fresh = not os.path.exists(args.out)
    f = open(args.out, "a")
    if fresh:
        f.write(HEADER.format(envs=args.envs, size=SIZE, calls=args.calls, warmup=args.warmup))

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        f.write(text + "\n")
        f.flush()

    if args.what in ("calls", "start", "all"):
        import numpy as np
        import torch
        from megaverse_amd.extension import MegaverseGym
        if not torch.cuda.is_available():
            sys.exit("seed_envs_bench: no GPU")
        if args.what in ("calls", "all"):
            bench_calls(args, emit, torch, MegaverseGym, np)
        if args.what in ("start", "all"):
            bench_start(args, emit, torch, MegaverseGym, np)
    if args.what in ("bench", "all"):
        bench_headline(args, emit)
    f.close()


if __name__ == "__main__":
    main()
