#!/usr/bin/env python
"""What a masked env reset costs (include/megaverse_hip.h: mv_reset_envs).  Needs a GPU; reads nothing outside the tree.

  masked   mv_reset_envs (device mask, render = 0) for TowerBuilding and HexMemory with --envs envs and --flagged envs flagged (default: 1, 32 and all):
           every call is timed on its own with two HIP events on the gym's stream -- the call as the stream sees it: its launches and what lies between
           them -- and followed by one untimed step and a synchronise, so that a host-fed gym (HexMemory) has its rings topped up again before the next
           call.  Mean and minimum over --calls calls.
  reset    mv_reset timed the same way (it always draws: its figure includes the observation pass) -- no masked call in this mode, so the same script
           measures a tree that does not have them yet; the kernels' own durations come from a kernel trace of either mode.
  plan     a planner's iteration on TowerBuilding --envs x 128 x 128: fork every env from env 0, mv_step_n(16, sequence), reset_envs of the destinations
           (render = 0: the next iteration's ticks draw) -- with map and mask in device memory and in host memory, beside the same iteration without the reset.

One JSON line per figure.   python scripts/reset_envs_bench.py [--what masked|reset|plan|all] [--scenario NAME] [--flagged K]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENARIOS = ("TowerBuilding", "HexMemory")


def make_gym(MegaverseGym, scenario, N, size=(64, 36)):
    g = MegaverseGym(scenario, size[0], size[1], N, 1, 0, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    for t in range(8):   # states that differ from what a reset leaves
        g.sample_random_actions(7, t)
        g.step()
    g.synchronize()
    return g


def per_call(torch, g, fn, calls, warmup):
    """fn() timed call by call between two HIP events on the current (the gym's) stream; one step and a synchronise between calls -> (mean, min) in us"""
    times = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b) * 1e3)
        g.sample_random_actions(7, 100 + i)
        g.step()
        g.synchronize()
    return sum(times) / len(times), min(times)


def bench_masked(args, torch, MegaverseGym, np):
    N = args.envs
    for scenario in ([args.scenario] if args.scenario else SCENARIOS):
        g = make_gym(MegaverseGym, scenario, N)
        for flagged in ([args.flagged] if args.flagged else (1, 32, N)):
            m = np.zeros(N, np.bool_)
            m[np.linspace(0, N - 1, flagged).astype(np.int64)] = True   # spread over the batch
            dev = torch.as_tensor(m).to("cuda")
            torch.cuda.synchronize()
            mean, best = per_call(torch, g, lambda: g.reset_envs(dev, render=False), args.calls, args.warmup)
            print(json.dumps({"what": "masked", "scenario": scenario, "envs": N, "flagged": int(m.sum()), "calls": args.calls, "render": 0,
                              "call_us_mean": round(mean, 2), "call_us_min": round(best, 2), "host_generator_threads": g.host_generator_threads()}), flush=True)
        g.close()


def bench_reset(args, torch, MegaverseGym, np):
    N = args.envs
    for scenario in ([args.scenario] if args.scenario else SCENARIOS):
        g = make_gym(MegaverseGym, scenario, N)
        mean, best = per_call(torch, g, g.reset, args.calls, args.warmup)
        print(json.dumps({"what": "reset", "scenario": scenario, "envs": N, "calls": args.calls, "render": 1,
                          "call_us_mean": round(mean, 2), "call_us_min": round(best, 2)}), flush=True)
        g.close()


def bench_plan(args, torch, MegaverseGym, np):
    N, S, K = args.envs, 128, 16
    host_map = np.array([-1] + [0] * (N - 1), np.int32)
    host_mask = host_map >= 0
    for form in ("fork_only_host", "host", "device") * 2:
        g = MegaverseGym("TowerBuilding", S, S, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        g.reset()
        ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
                torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
        script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
        dev_map, dev_mask = torch.as_tensor(host_map).to("cuda"), torch.as_tensor(host_mask).to("cuda")
        torch.cuda.synchronize()
        g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
        g.set_action_ring(K, script.data_ptr())

        def iteration():
            g.fork_envs(dev_map if form == "device" else host_map)
            g.step_n(K, "sequence", 0, 0)
            if form != "fork_only_host":
                g.reset_envs(dev_mask if form == "device" else host_mask, render=False)

        for _ in range(args.plan_warmup):
            iteration()
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.plan_iterations):
            iteration()
        g.synchronize()
        dt = time.perf_counter() - t0
        ticks = args.plan_iterations * K
        print(json.dumps({"what": "plan", "form": form, "envs": N, "size": S, "ticks_per_iteration": K, "iterations": args.plan_iterations,
                          "seconds": round(dt, 4), "obs_per_s": round(ticks * N / dt), "us_per_iteration": round(dt / args.plan_iterations * 1e6, 1)}),
              flush=True)
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["masked", "reset", "plan", "all"], default="all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--scenario", default="", help="masked / reset: this scenario only")
    ap.add_argument("--flagged", type=int, default=0, help="masked: this many flagged envs only")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plan-iterations", type=int, default=256)
    ap.add_argument("--plan-warmup", type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("reset_envs_bench: no GPU")
    if args.what in ("masked", "all"):
        bench_masked(args, torch, MegaverseGym, np)
    if args.what in ("reset", "all"):
        bench_reset(args, torch, MegaverseGym, np)
    if args.what in ("plan", "all"):
        bench_plan(args, torch, MegaverseGym, np)


if __name__ == "__main__":
    main()
