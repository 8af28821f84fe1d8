#!/usr/bin/env python
"""What map observations cost (include/megaverse_hip.h: mv_set_map_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each: bench.py's headline (agent observations/s).
           --parent DIR: the parent's checkout, built.  Every kernel such a gym launches is the parent's, so the expectation is "inside the parent's own
           min - max spread"; both lists are recorded and the report says plainly when it is outside.
  calls    --envs x 1 agents at --size x --size, fast pixels, 16-tick MV_POLICY_SEQUENCE calls into rings with float16 depth and class labels attached,
           without the map and with it at M = 32 and M = 64 (cells of 0.5), on TowerBuilding and HexMemory: us per tick, and the differences -- what the
           one launch per drawn tick behind the planes' follower adds.  Reported, not gated.
  torch    the same rule as torch ops on the planes of one ring entry (index arithmetic, scatter_add_ for the counts, scatter_reduce_ amax for the keys):
           device events around --calls repetitions after a warm-up, us per tick; the ratio to the HIP launch's added time is reported, promised nowhere.
           The share of cells on which the torch grids differ from the library's (its fp32 operations come in another order) is printed beside it.

Every measurement is a process of its own under a time limit (--step-timeout seconds), one at a time; the first one that fails, is killed by a signal or
runs out of time ends the whole run, and nothing more is started on the device.  Not measured here: several agents per env, exact pixels, several GPUs.

JSON lines on stdout; the report goes to --out.
    python scripts/map_obs_bench.py [--what off|calls|torch|all] [--parent DIR] [--out profiles/map_obs_measured.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16
FORMS = (("depth + labels", 0), ("depth + labels + map, M = 32", 32), ("depth + labels + map, M = 64", 64))
CELL_SIZE = 0.5
SCENARIOS = ("TowerBuilding", "HexMemory")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v, fmt="{:.2f}"):
    return f"{fmt.format(median(v)):>10}  ({fmt.format(min(v))} - {fmt.format(max(v))})"


def run_json(cmd, cwd, key, limit):
    """one measurement: a child under a time limit; -> the JSON lines of its stdout that have `key`.  Anything but a clean exit ends the run."""
    try:
        out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"map_obs_bench: {' '.join(cmd)} ran past its {limit} s: stopping, nothing more is started")
    found = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{") and f'"{key}"' in line]
    if out.returncode != 0 or not found:
        sys.exit(f"map_obs_bench: {' '.join(cmd)} ended with status {out.returncode}: stopping, nothing more is started\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return found


def verdict(parent, this, unit):
    """the acceptance rule (higher is better): this commit's median not worse than the parent's median by more than the parent's own max - min spread"""
    mp, mt, sp = median(parent), median(this), max(parent) - min(parent)
    inside = min(parent) <= mt <= max(parent)
    return (f"this commit's median {mt:.3f} {unit} against the parent's {mp:.3f} {unit}: " + ("worse" if mp > mt else "not worse") + f" by {abs(mp - mt):.3f}, the parent's "
            f"own max - min spread is {sp:.3f}; the median is " + ("INSIDE" if inside else "OUTSIDE") + f" the parent's range {min(parent):.3f} - {max(parent):.3f}"
            + ("" if inside else " (" + ("better" if mt >= mp else "WORSE") + ")"))


def make_gym(args, ring, script, cells):
    """a reset gym stepping into `ring` from `script` with float16 depth and class labels attached, and the map where cells > 0"""
    from megaverse_amd.extension import MegaverseGym
    g = MegaverseGym(args.scenario, args.size, args.size, args.envs, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    g.set_action_ring(K, script.data_ptr())
    g.set_depth_obs(True, "float16")
    g.set_seg_obs(True, "class")
    if cells:
        g.set_map_obs(True, cells, CELL_SIZE)
    return g


def torch_map(depth, seg, cams, M, inv):
    """the rule as torch ops: depth [F, H, W] float16, seg [F, H, W] uint8, cams [F, 12] float32 -> int16 [F, 3, M, M]"""
    import torch
    F, H, W = depth.shape
    t = depth.float()
    x = (((torch.arange(W, device=t.device, dtype=torch.float32) + 0.5) / W) * 2 - 1) * 1.19175359
    y = (((torch.arange(H, device=t.device, dtype=torch.float32) + 0.5) / H) * 2 - 1) * (1.19175359 / (128.0 / 72.0))
    c = cams[:, 3:].reshape(F, 3, 3)
    d = torch.einsum("fkj,fjhw->fkhw", c, torch.stack([x[None, None, :] * t, y[None, :, None] * t, -t], 1))
    rx, rz = c[:, 0, 0, None, None], c[:, 2, 0, None, None]
    col = torch.floor((d[:, 0] * rx + d[:, 2] * rz) * inv).long() + M // 2
    row = torch.floor((d[:, 0] * rz - d[:, 2] * rx) * inv).long()
    hq = torch.clamp(torch.floor(d[:, 1] * 32), -32767, 32767).int()
    cls = seg.int() & 15
    ok = (t != 0) & (cls != 14) & (col >= 0) & (col < M) & (row >= 0) & (row < M)
    idx = (torch.arange(F, device=t.device)[:, None, None] * (M * M) + row * M + col)[ok]
    key = (((hq + 32768) << 4) | cls)[ok]
    count = torch.zeros(F * M * M, dtype=torch.int32, device=t.device).scatter_add_(0, idx, torch.ones_like(key))
    best = torch.zeros(F * M * M, dtype=torch.int32, device=t.device).scatter_reduce_(0, idx, key, "amax")
    seen = count > 0
    out = torch.stack([count.clamp(max=32767), torch.where(seen, (best >> 4) - 32768, 0), torch.where(seen, best & 15, 0)], 0)
    return out.reshape(3, F, M, M).permute(1, 0, 2, 3).to(torch.int16).contiguous()


def child_torch(args):
    """one scenario: a 16-tick call with the map attached, then the torch rule on the last entry's planes, timed with device events"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("map_obs_bench: no GPU")
    N, S = args.envs, args.size
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    for cells in (32, 64):
        g = make_gym(args, ring, script, cells)
        g.step_n(K, "sequence", 0, 0)
        g.synchronize()
        cams = torch.as_tensor(np.stack([g.debug_map_camera(e, 0) for e in range(N)])).to("cuda")
        depth, seg, want = g.depth_obs_ring()[K - 1], g.seg_obs_ring()[K - 1], g.map_obs_ring()[K - 1]
        inv = float(np.float32(1.0) / np.float32(CELL_SIZE))
        for _ in range(max(2, args.warmup)):
            got = torch_map(depth, seg, cams, cells, inv)
        differ = float((got != want).any(1).float().mean())
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            torch_map(depth, seg, cams, cells, inv)
        stop.record()
        torch.cuda.synchronize()
        g.close()
        print(json.dumps({"what": "torch", "scenario": args.scenario, "cells": cells, "us_per_tick": round(start.elapsed_time(stop) / args.calls * 1e3, 3),
                          "cells_that_differ": differ}), flush=True)


def child_calls(args):
    """one scenario: the three forms, --share-reps repetitions, the forms alternating within each, one gym alive at a time"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("map_obs_bench: no GPU")
    N, S = args.envs, args.size
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    for rep in range(args.share_reps):
        for name, cells in FORMS:
            g = make_gym(args, ring, script, cells)
            for _ in range(args.warmup):
                g.step_n(K, "sequence", 0, 0)
            g.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                g.step_n(K, "sequence", 0, 0)
            g.synchronize()
            dt = time.perf_counter() - t0
            g.close()
            print(json.dumps({"what": "calls", "scenario": args.scenario, "form": name, "rep": rep, "us_per_tick": round(dt / (args.calls * K) * 1e6, 3)}), flush=True)


def bench_off(args, lines):
    trees = (("parent", os.path.abspath(args.parent)), ("this commit", ROOT))
    obs = {name: [] for name, _ in trees}
    for rep in range(args.reps):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):   # (alternating, and which build goes first alternates too)
            line = run_json([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                             "--no-cpu-baseline", "--no-extra-legs"], tree, "value", args.step_timeout)[-1]
            obs[name].append(line["value"] / 1e6)
            print(json.dumps({"what": "off", "label": name, "rep": rep, "bench_py_value": line["value"], "unit": line.get("unit")}), flush=True)
    lines.append(f"(a) Nothing attached: the parent commit against this one, {args.reps} alternating runs each (parent first in the even repetitions, this commit "
                 "first in the odd ones), every run a process of its own.")
    lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-extra-legs, M agent observations/s (higher is better):")
    for name, _ in trees:
        lines.append(f"  {name:<12} " + " ".join(f"{v:.3f}" for v in obs[name]) + f"   median {median(obs[name]):.3f}   range {min(obs[name]):.3f} - {max(obs[name]):.3f}")
    lines.append("  " + verdict(obs["parent"], obs["this commit"], "M obs/s"))
    lines.append("")


def bench_calls(args, lines):
    lines.append(f"(b) {args.envs} x 1 at {args.size}x{args.size}, fast pixels, {K}-tick MV_POLICY_SEQUENCE calls into rings, {args.calls} calls timed after {args.warmup}, "
                 f"{args.share_reps} repetitions, the forms alternating within each, one gym alive at a time; us per tick, median (min - max).  The map: ONE "
                 "launch per drawn tick behind the planes' follower.  torch: the same rule as torch ops on one entry's planes, device events.  Reported, not gated.")
    for scenario in SCENARIOS:
        found = run_json([sys.executable, os.path.abspath(__file__), "--what", "child_calls", "--scenario", scenario, "--envs", str(args.envs), "--size", str(args.size),
                          "--calls", str(args.calls), "--warmup", str(args.warmup), "--share-reps", str(args.share_reps)], ROOT, "us_per_tick", args.step_timeout)
        for line in found:
            print(json.dumps(line), flush=True)
        lines.append(scenario)
        med = {}
        for name, _ in FORMS:
            us = [x["us_per_tick"] for x in found if x["form"] == name]
            med[name] = median(us)
            lines.append(f"  {name:<24}{spread(us)}")
        torch_us = {x["cells"]: x for x in run_json([sys.executable, os.path.abspath(__file__), "--what", "child_torch", "--scenario", scenario, "--envs", str(args.envs),
                                                     "--size", str(args.size), "--calls", str(args.calls), "--warmup", str(args.warmup)], ROOT, "us_per_tick",
                                                    args.step_timeout)} if args.what in ("torch", "all") else {}
        for name, cells in FORMS[1:]:
            added = med[name] - med[FORMS[0][0]]
            lines.append(f"  M = {cells}: added per tick (difference of the medians): {added:.2f} us")
            if cells in torch_us:
                lines.append(f"          the rule in torch on the same planes: {torch_us[cells]['us_per_tick']:.2f} us per tick, {torch_us[cells]['us_per_tick'] / max(added, 1e-9):.1f} x the "
                             f"added time ({100 * torch_us[cells]['cells_that_differ']:.3f} % of its cells differ from the library's: another order of fp32 operations)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["off", "calls", "torch", "all", "child_calls", "child_torch"], default="all")
    ap.add_argument("--parent", default="", help="the parent commit's checkout, built (off)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=64, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5, help="off: alternating runs of each build")
    ap.add_argument("--share-reps", type=int, default=3, help="calls: repetitions")
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds every measurement's process may take")
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    ap.add_argument("--scenario", default="TowerBuilding")
    args = ap.parse_args()
    if args.what == "child_calls":
        return child_calls(args)
    if args.what == "child_torch":
        return child_torch(args)
    if args.what in ("off", "all") and not args.parent:
        sys.exit("map_obs_bench: off needs --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["Map observations (mv_set_map_obs): measured by scripts/map_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every measurement a process of its own, one gym alive at a time.  Several agents per env, "
             "exact pixels, several GPUs: unmeasured.", ""]
    if args.what in ("off", "all"):
        bench_off(args, lines)
    if args.what in ("calls", "torch", "all"):
        bench_calls(args, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
