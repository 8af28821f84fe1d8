#!/usr/bin/env python
"""What stack observations cost (include/megaverse_hip.h: mv_set_stack_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each: bench.py's headline (scripts/map_obs_bench.py's
           measurement and acceptance rule, as they stand).
  calls    --envs x 1 agents at --size x --size, fast pixels, 16-tick MV_POLICY_SEQUENCE calls into a ring of 16 with NOTHING else attached: alone, and with
           the stack at (S, factor, fmt) = (4, 2, gray), (4, 1, gray), (4, 2, rgb), on TowerBuilding and Football: us per tick, and the differences -- what
           the one launch per drawn tick adds.  Reported, not gated.
  torch    the same rule as torch ops on the frames of the same ring entries (a channel-weighted integer sum over the pooled blocks, a roll of the stack, a
           where on done), device events around --calls repetitions of a 16-entry sweep after a warm-up, us per tick.  Its stacks must EQUAL the library's in
           every entry of the ring: a difference ends the run before anything is timed.

Every measurement is a process of its own under a time limit (--step-timeout seconds), one at a time; the first one that fails, is killed by a signal or
runs out of time ends the whole run, and nothing more is started on the device.  Not measured here: several agents per env, exact pixels, several GPUs.

JSON lines on stdout; the report goes to --out.
    python scripts/stack_obs_bench.py [--what off|calls|torch|all] [--parent DIR] [--out profiles/stack_obs_measured.txt]
"""
import argparse
import json
import os
import sys
import time

from map_obs_bench import K, ROOT, bench_off, median, run_json, spread

SCENARIOS = ("TowerBuilding", "Football")
STACKS = ((4, 2, "gray"), (4, 1, "gray"), (4, 2, "rgb"))
FORMS = (("frames alone", None),) + tuple((f"frames + stack, S = {s}, factor {f}, {fmt}", (s, f, fmt)) for s, f, fmt in STACKS)


def buffers(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("stack_obs_bench: no GPU")
    N, S = args.envs, args.size
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def make_gym(args, ring, script, stack):
    """a gym stepping into `ring` from `script`, the stack attached where given, reset"""
    from megaverse_amd.extension import MegaverseGym
    g = MegaverseGym(args.scenario, args.size, args.size, args.envs, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    if stack:
        g.set_stack_obs(True, *stack)
    g.reset()
    g.set_action_ring(K, script.data_ptr())
    return g


def torch_stack(frames, done, prev, factor, fmt):
    """the rule as torch ops for one tick: frames [F, H, W, 4] uint8, done [F] uint8, prev [F, S, C, h, w] uint8 -> the tick's stacks"""
    import torch
    import torch.nn.functional as nnf
    rgb = frames[..., :3].permute(0, 3, 1, 2).float()   # (sums of at most 16 bytes: exact in float32)
    sums = (nnf.avg_pool2d(rgb, factor, divisor_override=1) if factor > 1 else rgb).to(torch.int32)
    n = factor * factor
    if fmt == "gray":
        img = ((77 * sums[:, 0] + 150 * sums[:, 1] + 29 * sums[:, 2] + 128 * n) // (256 * n)).to(torch.uint8)[:, None]
    else:
        img = ((sums + n // 2) // n).to(torch.uint8)
    shifted = torch.roll(prev, -1, 1)
    shifted[:, -1] = img
    return torch.where(done[:, None, None, None, None] != 0, img[:, None].expand_as(prev), shifted)


def child_torch(args):
    """one scenario: per stack form a 16-tick call, then the torch rule over the same 16 entries, compared in every entry and timed with device events"""
    sys.path.insert(0, ROOT)
    import torch
    ring, script = buffers(args)
    for stack in STACKS:
        g = make_gym(args, ring, script, stack)
        want = g.stack_obs_ring()
        g.synchronize()
        torch.cuda.synchronize()
        start_stack = want[0].clone()   # the reset's stacks: entry 0, before the call overwrites it
        g.step_n(K, "sequence", 0, 0)
        g.synchronize()
        torch.cuda.synchronize()

        def sweep(check):
            prev, differ = start_stack, 0.0
            for j in range(K):
                prev = torch_stack(ring[0][j], ring[2][j], prev, stack[1], stack[2])
                if check:
                    differ = max(differ, float((prev != want[j]).float().mean()))
            return differ
        differ = sweep(True)
        if differ:
            sys.exit(f"stack_obs_bench: the torch rule differs from the library's stacks on {100 * differ:.4f} % of the bytes of an entry")
        for _ in range(max(1, args.warmup // 4)):
            sweep(False)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            sweep(False)
        stop.record()
        torch.cuda.synchronize()
        g.close()
        print(json.dumps({"what": "torch", "scenario": args.scenario, "stack": list(stack), "us_per_tick": round(start.elapsed_time(stop) / (args.calls * K) * 1e3, 3),
                          "bytes_that_differ": differ}), flush=True)


def child_calls(args):
    """one scenario: the forms, --share-reps repetitions, the forms alternating within each, one gym alive at a time"""
    sys.path.insert(0, ROOT)
    ring, script = buffers(args)
    for rep in range(args.share_reps):
        for name, stack in FORMS:
            g = make_gym(args, ring, script, stack)
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
    lines.append(f"(b) {args.envs} x 1 at {args.size}x{args.size}, fast pixels, {K}-tick MV_POLICY_SEQUENCE calls into a ring of {K}, nothing else attached, {args.calls} "
                 f"calls timed after {args.warmup}, {args.share_reps} repetitions, the forms alternating within each, one gym alive at a time; us per tick, median "
                 "(min - max).  The stack: ONE launch per drawn tick behind the call's passes.  torch: the same rule as torch ops over the same ring entries, "
                 "device events; its stacks equal the library's in every entry, or the run ends.  Reported, not gated.")
    child = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--size", str(args.size), "--calls", str(args.calls), "--warmup", str(args.warmup),
             "--share-reps", str(args.share_reps)]
    for scenario in SCENARIOS:
        found = run_json(child + ["--what", "child_calls", "--scenario", scenario], ROOT, "us_per_tick", args.step_timeout)
        for line in found:
            print(json.dumps(line), flush=True)
        lines.append(scenario)
        med = {}
        for name, _ in FORMS:
            us = [x["us_per_tick"] for x in found if x["form"] == name]
            med[name] = median(us)
            lines.append(f"  {name:<44}{spread(us)}")
        torch_us = {tuple(x["stack"]): x for x in run_json(child + ["--what", "child_torch", "--scenario", scenario], ROOT, "us_per_tick", args.step_timeout)} \
            if args.what in ("torch", "all") else {}
        for name, stack in FORMS[1:]:
            added = med[name] - med[FORMS[0][0]]
            lines.append(f"  {stack}: added per tick (difference of the medians): {added:.2f} us")
            if stack in torch_us:
                lines.append(f"          the rule in torch over the same entries: {torch_us[stack]['us_per_tick']:.2f} us per tick; its stacks equal the library's byte for byte")
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
        sys.exit("stack_obs_bench: off needs --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["Stack observations (mv_set_stack_obs): measured by scripts/stack_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
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
