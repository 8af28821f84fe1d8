#!/usr/bin/env python
"""What world map observations cost (include/megaverse_hip.h: mv_set_world_map_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.
The measurement rules, the child processes' time limits and the report's helpers are scripts/map_obs_bench.py's, imported from it.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each (map_obs_bench.bench_off)
  calls    --envs x 1 agents at --size x --size, fast pixels, 16-tick MV_POLICY_SEQUENCE calls into rings with float16 depth and class labels attached:
           without a map, with the egocentric map and with the world map, each at M = 32 and M = 64 (cells of 0.5), on TowerBuilding and HexMemory: us per
           tick and the differences -- the world map's launch beside the egocentric one's, which zeroes its LDS where this one loads the grid back
  torch    the same rule as torch ops on the planes of one ring entry, merged into a persistent tensor: device events, us per tick

JSON lines on stdout; the report goes to --out.
    python scripts/world_map_obs_bench.py [--what off|calls|torch|all] [--parent DIR] [--out profiles/world_map_obs_measured.txt]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_obs_bench as B  # noqa: E402

ROOT, K, CELL_SIZE, ORIGIN = B.ROOT, B.K, B.CELL_SIZE, (-4.0, -4.0)
FORMS = (("depth + labels", "", 0), ("+ map, M = 32", "map", 32), ("+ map, M = 64", "map", 64), ("+ world map, M = 32", "world", 32),
         ("+ world map, M = 64", "world", 64))


def make_gym(args, ring, script, kind, cells):
    g = B.make_gym(args, ring, script, cells if kind == "map" else 0)
    if kind == "world":
        g.set_world_map_obs(True, cells, CELL_SIZE, ORIGIN)
    return g


def buffers(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("world_map_obs_bench: no GPU")
    N, S = args.envs, args.size
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def torch_world_map(depth, seg, cams, grid, M, inv):
    """the rule as torch ops: depth [F, H, W] float16, seg [F, H, W] uint8, cams [F, 12] float32 merged into grid int16 [F, 3, M, M] -> the new grid"""
    import torch
    F, H, W = depth.shape
    t = depth.float()
    x = (((torch.arange(W, device=t.device, dtype=torch.float32) + 0.5) / W) * 2 - 1) * 1.19175359
    y = (((torch.arange(H, device=t.device, dtype=torch.float32) + 0.5) / H) * 2 - 1) * (1.19175359 / (128.0 / 72.0))
    P = cams[:, :3, None, None] + torch.einsum("fkj,fjhw->fkhw", cams[:, 3:].reshape(F, 3, 3), torch.stack([x[None, None, :] * t, y[None, :, None] * t, -t], 1))
    col, row = torch.floor((P[:, 0] - ORIGIN[0]) * inv).long(), torch.floor((P[:, 2] - ORIGIN[1]) * inv).long()
    hq = torch.clamp(torch.floor(P[:, 1] * 32), -32767, 32767).int()
    cls = seg.int() & 15
    ok = (t != 0) & (cls != 14) & (col >= 0) & (col < M) & (row >= 0) & (row < M)
    idx = (torch.arange(F, device=t.device)[:, None, None] * (M * M) + row * M + col)[ok]
    key = (((hq + 32768) << 4) | cls)[ok]
    old = grid.int().permute(1, 0, 2, 3).reshape(3, F * M * M)
    count = old[0].clone().scatter_add_(0, idx, torch.ones_like(key))
    best = torch.where(old[0] > 0, ((old[1] + 32768) << 4) | old[2], 0).scatter_reduce_(0, idx, key, "amax")
    seen = count > 0
    out = torch.stack([count.clamp(max=32767), torch.where(seen, (best >> 4) - 32768, 0), torch.where(seen, best & 15, 0)], 0)
    return out.reshape(3, F, M, M).permute(1, 0, 2, 3).to(torch.int16).contiguous()


def child_torch(args):
    """one scenario: a 16-tick call with the world map attached, then the torch rule on the last entry's planes, timed with device events; its first merge
    into the grids as they stood before the call's last tick is not reproduced -- the figure is the cost of one merge, which does not depend on the grid"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    ring, script = buffers(args)
    for cells in (32, 64):
        g = make_gym(args, ring, script, "world", cells)
        g.step_n(K, "sequence", 0, 0)
        g.synchronize()
        cams = torch.as_tensor(np.stack([g.debug_map_camera(e, 0) for e in range(args.envs)])).to("cuda")
        depth, seg, grid = g.depth_obs_ring()[K - 1], g.seg_obs_ring()[K - 1], g.world_map_obs().clone()
        inv = float(np.float32(1.0) / np.float32(CELL_SIZE))
        for _ in range(max(2, args.warmup)):
            torch_world_map(depth, seg, cams, grid, cells, inv)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            grid = torch_world_map(depth, seg, cams, grid, cells, inv)
        stop.record()
        torch.cuda.synchronize()
        g.close()
        print(json.dumps({"what": "torch", "scenario": args.scenario, "cells": cells, "us_per_tick": round(start.elapsed_time(stop) / args.calls * 1e3, 3)}), flush=True)


def child_calls(args):
    """one scenario: the five forms, --share-reps repetitions, the forms alternating within each, one gym alive at a time"""
    sys.path.insert(0, ROOT)
    ring, script = buffers(args)
    for rep in range(args.share_reps):
        for name, kind, cells in FORMS:
            g = make_gym(args, ring, script, kind, cells)
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


def bench_calls(args, lines):
    lines.append(f"(b) {args.envs} x 1 at {args.size}x{args.size}, fast pixels, {K}-tick MV_POLICY_SEQUENCE calls into rings, {args.calls} calls timed after {args.warmup}, "
                 f"{args.share_reps} repetitions, the forms alternating within each, one gym alive at a time; us per tick, median (min - max).  Either map: ONE "
                 "launch per drawn tick behind the planes' follower; the world map's loads each agent's grid back where the egocentric one zeroes its LDS.  torch: "
                 "the same rule as torch ops on one entry's planes, merged into a persistent tensor, device events.  Reported, not gated.")
    me = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--size", str(args.size), "--calls", str(args.calls), "--warmup", str(args.warmup)]
    for scenario in B.SCENARIOS:
        found = B.run_json(me + ["--what", "child_calls", "--scenario", scenario, "--share-reps", str(args.share_reps)], ROOT, "us_per_tick", args.step_timeout)
        for line in found:
            print(json.dumps(line), flush=True)
        lines.append(scenario)
        med = {}
        for name, _, _ in FORMS:
            us = [x["us_per_tick"] for x in found if x["form"] == name]
            med[name] = B.median(us)
            lines.append(f"  {name:<24}{B.spread(us)}")
        torch_us = {x["cells"]: x["us_per_tick"] for x in B.run_json(me + ["--what", "child_torch", "--scenario", scenario], ROOT, "us_per_tick", args.step_timeout)} \
            if args.what in ("torch", "all") else {}
        for name, kind, cells in FORMS[1:]:
            added = med[name] - med[FORMS[0][0]]
            lines.append(f"  {name[2:]}: added per tick (difference of the medians): {added:.2f} us"
                         + (f"; the rule in torch on the same planes: {torch_us[cells]:.2f} us per tick, {torch_us[cells] / max(added, 1e-9):.1f} x the added time"
                            if kind == "world" and cells in torch_us else ""))
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
        sys.exit("world_map_obs_bench: off needs --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["World map observations (mv_set_world_map_obs): measured by scripts/world_map_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every measurement a process of its own, one gym alive at a time.  Several agents per env, "
             "exact pixels, several GPUs: unmeasured.", ""]
    if args.what in ("off", "all"):
        B.bench_off(args, lines)
    if args.what in ("calls", "torch", "all"):
        bench_calls(args, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
