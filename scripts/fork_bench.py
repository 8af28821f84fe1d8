#!/usr/bin/env python
"""What an env fork costs (include/megaverse_hip.h: mv_fork_envs).  Needs a GPU; reads nothing outside the tree.

  fork     mv_fork_envs (device map) timed with HIP events on the gym's stream over --calls back-to-back calls after a warm-up, for TowerBuilding and
           HexMemory (the largest per-env state) with --envs envs and two maps each: every env from env 0 (one source, cached), odd envs from their even
           neighbour (envs / 2 distinct sources).  Next to each: ONE hipMemcpyAsync device to device of the same number of bytes, timed the same way --
           the yardstick; the gather kernel can at best match it.
  plan     one planning iteration on TowerBuilding --envs x 128 x 128: fork every env from env 0, then mv_step_n(16, sequence) -- obs/s beside the same
           mv_step_n without the fork (a host clock around work that ends in a device synchronise), with the map in device memory (mv_fork_envs) and in
           host memory (mv_fork_envs_host).

One JSON line per figure.   python scripts/fork_bench.py [--what fork|plan|all]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hip_runtime():
    """the HIP runtime this process has already loaded (torch's or the system's): hipMemcpyAsync itself, not a framework's copy kernel"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            return C.CDLL(path)
    return None


def timed(torch, fn, calls, warmup):
    """mean microseconds of fn() over `calls` back-to-back calls, between two HIP events on the current (the gym's) stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def bench_fork(args, torch, MegaverseGym, np):
    hip = hip_runtime()
    if hip is not None:
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    N = args.envs
    maps = {"all_from_env_0": np.array([-1] + [0] * (N - 1), np.int32),
            "odd_from_even_neighbour": np.array([-1 if d % 2 == 0 else d - 1 for d in range(N)], np.int32)}
    for scenario in ("TowerBuilding", "HexMemory"):
        g = MegaverseGym(scenario, 64, 36, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        g.reset()
        for t in range(8):   # states that differ from what a reset leaves
            g.sample_random_actions(7, t)
            g.step()
        g.synchronize()
        per_env = g.fork_bytes_per_env()
        for name, m in maps.items():
            dev = torch.as_tensor(m).to("cuda")
            dests = int((m >= 0).sum())
            nbytes = dests * per_env
            us = timed(torch, lambda: g.fork_envs(dev), args.calls, args.warmup)
            src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            if hip is not None:
                copy, how = (lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None)), "hipMemcpyAsync"   # 3: device to device
            else:
                copy, how = (lambda: dst.copy_(src)), "torch copy_ (the HIP runtime was not found among the loaded libraries)"
            us_copy = timed(torch, copy, args.calls, args.warmup)
            print(json.dumps({"what": "fork", "scenario": scenario, "envs": N, "map": name, "destinations": dests, "bytes_per_env": per_env,
                              "bytes_per_call": nbytes, "calls": args.calls, "fork_us": round(us, 2), "fork_GBps": round(2 * nbytes / us / 1e3, 1),
                              "copy": how, "copy_us": round(us_copy, 2), "copy_GBps": round(2 * nbytes / us_copy / 1e3, 1),
                              "fork_over_copy": round(us / us_copy, 2)}), flush=True)
            g.step()   # (takes the status read-backs the device-form calls left pending)
            g.synchronize()
        g.close()


def bench_plan(args, torch, MegaverseGym, np):
    N, S, K = args.envs, 128, 16
    host_map = np.array([-1] + [0] * (N - 1), np.int32)
    for fork in ("none", "device_map", "host_map") * 2:
        g = MegaverseGym("TowerBuilding", S, S, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        g.reset()
        ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
                torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
        script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
        dev_map = torch.as_tensor(np.array([-1] + [0] * (N - 1), np.int32)).to("cuda")
        torch.cuda.synchronize()
        g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
        g.set_action_ring(K, script.data_ptr())

        def iteration():
            if fork != "none":
                g.fork_envs(dev_map if fork == "device_map" else host_map)
            g.step_n(K, "sequence", 0, 0)

        for _ in range(args.plan_warmup):
            iteration()
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.plan_iterations):
            iteration()
        g.synchronize()
        dt = time.perf_counter() - t0
        ticks = args.plan_iterations * K
        print(json.dumps({"what": "plan", "fork": fork, "envs": N, "size": S, "ticks_per_iteration": K, "iterations": args.plan_iterations,
                          "seconds": round(dt, 4), "obs_per_s": round(ticks * N / dt), "us_per_iteration": round(dt / args.plan_iterations * 1e6, 1)}),
              flush=True)
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["fork", "plan", "all"], default="all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200, help="timed fork calls (at least 100)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--plan-iterations", type=int, default=256)
    ap.add_argument("--plan-warmup", type=int, default=16)
    args = ap.parse_args()
    args.calls = max(100, args.calls)
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("fork_bench: no GPU")
    if args.what in ("fork", "all"):
        bench_fork(args, torch, MegaverseGym, np)
    if args.what in ("plan", "all"):
        bench_plan(args, torch, MegaverseGym, np)


if __name__ == "__main__":
    main()
