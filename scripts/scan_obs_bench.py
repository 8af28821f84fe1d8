#!/usr/bin/env python
"""What scan observations cost (include/megaverse_hip.h: mv_set_scan_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each: bench.py's headline (scripts/map_obs_bench.py's
           measurement and acceptance rule, as they stand).
  calls    --envs x 1 agents at --size x --size, fast pixels, 16-tick MV_POLICY_SEQUENCE calls into rings with float16 depth and class labels attached:
           alone, with the scan at K = 64 and K = 128 (the default band), and with the egocentric map at M = 32 (cells of 0.5) on the same gym, on
           TowerBuilding and HexMemory: us per tick, and the differences -- what each one launch per drawn tick adds.  Reported, not gated.
  torch    the same rule as torch ops on the planes of one ring entry, every fp32 operation in the rule's order (elementwise kernels, one division, one
           square root, scatter_add_ for the counts, scatter_reduce_ amin for the keys): device events around --calls repetitions after a warm-up, us per
           tick.  Its fans must EQUAL the library's on that entry: a difference ends the run.

Every measurement is a process of its own under a time limit (--step-timeout seconds), one at a time; the first one that fails, is killed by a signal or
runs out of time ends the whole run, and nothing more is started on the device.  Not measured here: several agents per env, exact pixels, a kernel trace of
the launch alone.

JSON lines on stdout; the report goes to --out.
    python scripts/scan_obs_bench.py [--what off|calls|torch|all] [--parent DIR] [--out profiles/scan_obs_measured.txt]
"""
import argparse
import json
import os
import sys
import time

from map_obs_bench import CELL_SIZE, K, ROOT, SCENARIOS, bench_off, median, run_json, spread

FORMS = (("depth + labels", None, 0), ("depth + labels + scan, K = 64", "scan", 64), ("depth + labels + scan, K = 128", "scan", 128),
         ("depth + labels + map, M = 32", "map", 32))
BEAMS = (64, 128)


def make_gym(args, ring, script, kind, size):
    """a reset gym stepping into `ring` from `script` with float16 depth and class labels attached, and the scan of `size` beams or the map of `size` cells"""
    from megaverse_amd.extension import MegaverseGym
    g = MegaverseGym(args.scenario, args.size, args.size, args.envs, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    g.set_action_ring(K, script.data_ptr())
    g.set_depth_obs(True, "float16")
    g.set_seg_obs(True, "class")
    if kind == "scan":
        g.set_scan_obs(True, size)
    if kind == "map":
        g.set_map_obs(True, size, CELL_SIZE)
    return g


def buffers(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("scan_obs_bench: no GPU")
    N, S = args.envs, args.size
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def torch_scan(depth, seg, cams, beams, bscale, h_lo, h_hi):
    """the rule as torch ops, mv_scan_obs.h's operations in its order: depth [F, H, W] float16, seg [F, H, W] uint8, cams [F, 12] float32 -> int16 [F, 3, K]"""
    import torch
    F, H, W = depth.shape
    t = depth.float()
    x = ((((torch.arange(W, device=t.device, dtype=torch.float32) + 0.5) / W) * 2 - 1) * 1.19175359)[None, None, :]
    y = ((((torch.arange(H, device=t.device, dtype=torch.float32) + 0.5) / H) * 2 - 1) * (1.19175359 / (128.0 / 72.0)))[None, :, None]
    c = [cams[:, 3 + q, None, None] for q in range(9)]
    pcx, pcy, pcz = x * t, y * t, -t
    dx, dy, dz = (c[0] * pcx + c[1] * pcy) + c[2] * pcz, (c[3] * pcx + c[4] * pcy) + c[5] * pcz, (c[6] * pcx + c[7] * pcy) + c[8] * pcz
    u, f = dx * c[0] + dz * c[6], dx * c[6] - dz * c[0]
    cls = seg.int() & 15
    fb = torch.floor((u / f) * bscale)
    ok = (t != 0) & (cls != 14) & (f > 0) & (dy >= h_lo) & (dy <= h_hi) & (fb >= -(beams // 2)) & (fb < beams // 2)
    rq = torch.clamp(torch.floor(torch.sqrt(u * u + f * f) * 64), 0, 32767).int()
    idx = (torch.arange(F, device=t.device)[:, None, None] * beams + (torch.where(ok, fb, 0.0).long() + beams // 2))[ok]
    key = ((rq << 4) | (15 - cls))[ok]
    count = torch.zeros(F * beams, dtype=torch.int32, device=t.device).scatter_add_(0, idx, torch.ones_like(key))
    best = torch.full((F * beams,), 0x7FFFFFFF, dtype=torch.int32, device=t.device).scatter_reduce_(0, idx, key, "amin")
    seen = count > 0
    out = torch.stack([torch.where(seen, best >> 4, -1), torch.where(seen, 15 - (best & 15), 0), count.clamp(max=32767)], 0)
    return out.reshape(3, F, beams).permute(1, 0, 2).to(torch.int16).contiguous()


def child_torch(args):
    """one scenario: a 16-tick call with the scan attached, then the torch rule on the last entry's planes, compared and timed with device events"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from megaverse_amd.extension import SCAN_DEFAULT_BAND
    ring, script = buffers(args)
    for beams in BEAMS:
        g = make_gym(args, ring, script, "scan", beams)
        g.step_n(K, "sequence", 0, 0)
        g.synchronize()
        cams = torch.as_tensor(np.stack([g.debug_map_camera(e, 0) for e in range(args.envs)])).to("cuda")
        depth, seg, want = g.depth_obs_ring()[K - 1], g.seg_obs_ring()[K - 1], g.scan_obs_ring()[K - 1]
        bscale = float(np.float32(beams // 2) / np.float32(1.19175359))
        for _ in range(max(2, args.warmup)):
            got = torch_scan(depth, seg, cams, beams, bscale, *SCAN_DEFAULT_BAND)
        differ = float((got != want).any(1).float().mean())
        hit = float((want[:, 0] >= 0).float().mean())
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            torch_scan(depth, seg, cams, beams, bscale, *SCAN_DEFAULT_BAND)
        stop.record()
        torch.cuda.synchronize()
        g.close()
        print(json.dumps({"what": "torch", "scenario": args.scenario, "beams": beams, "us_per_tick": round(start.elapsed_time(stop) / args.calls * 1e3, 3),
                          "beams_that_differ": differ, "beams_hit": hit}), flush=True)
        if differ:
            sys.exit(f"scan_obs_bench: the torch rule differs from the library's fans on {100 * differ:.4f} % of the beams")


def child_calls(args):
    """one scenario: the forms, --share-reps repetitions, the forms alternating within each, one gym alive at a time"""
    sys.path.insert(0, ROOT)
    ring, script = buffers(args)
    for rep in range(args.share_reps):
        for name, kind, size in FORMS:
            g = make_gym(args, ring, script, kind, size)
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
                 f"{args.share_reps} repetitions, the forms alternating within each, one gym alive at a time; us per tick, median (min - max).  The scan, the map: "
                 "ONE launch per drawn tick behind the planes' follower.  torch: the same rule as torch ops on one entry's planes, device events; its fans equal "
                 "the library's on that entry, or the run ends.  Reported, not gated.")
    child = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--size", str(args.size), "--calls", str(args.calls), "--warmup", str(args.warmup),
             "--share-reps", str(args.share_reps)]
    for scenario in SCENARIOS:
        found = run_json(child + ["--what", "child_calls", "--scenario", scenario], ROOT, "us_per_tick", args.step_timeout)
        for line in found:
            print(json.dumps(line), flush=True)
        lines.append(scenario)
        med = {}
        for name, _, _ in FORMS:
            us = [x["us_per_tick"] for x in found if x["form"] == name]
            med[name] = median(us)
            lines.append(f"  {name:<32}{spread(us)}")
        torch_us = {x["beams"]: x for x in run_json(child + ["--what", "child_torch", "--scenario", scenario], ROOT, "us_per_tick", args.step_timeout)} \
            if args.what in ("torch", "all") else {}
        for name, kind, size in FORMS[1:]:
            added = med[name] - med[FORMS[0][0]]
            lines.append(f"  {kind}, {size}: added per tick (difference of the medians): {added:.2f} us")
            if kind == "scan" and size in torch_us:
                lines.append(f"          the rule in torch on the same planes: {torch_us[size]['us_per_tick']:.2f} us per tick, {torch_us[size]['us_per_tick'] / max(added, 1e-9):.1f} x "
                             f"the added time; its fans equal the library's on every beam ({100 * torch_us[size]['beams_hit']:.1f} % of the beams are hit)")
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
        sys.exit("scan_obs_bench: off needs --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["Scan observations (mv_set_scan_obs): measured by scripts/scan_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every measurement a process of its own, one gym alive at a time.  Several agents per env, "
             "exact pixels, a kernel trace of the launch alone: unmeasured.", ""]
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
