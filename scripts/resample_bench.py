#!/usr/bin/env python
"""What env resampling costs (include/megaverse_hip.h: mv_resample_envs).  Needs a GPU; reads nothing outside the tree.

  fork        (a) a pure fork map -- every env from env 0 -- through mv_resample_envs and through mv_fork_envs, device maps, timed with HIP events on the
              gym's stream over --calls back-to-back calls after a warm-up, the two alternated twice in one process, for TowerBuilding and HexMemory (the
              largest per-env state) with --envs envs: what the generality costs on the old use case is the second launch, in which every workgroup exits.
  staged      (b) a full random map (every env draws its source uniformly) and a full rotation (src_of[d] = d + 1 mod N: every env staged), timed the same
              way.  Next to each: TWO back-to-back hipMemcpyAsync device to device of the staged envs' bytes -- into a staging buffer and out of it -- the
              floor a staged copy cannot beat; and one such copy of all moved bytes.
  population  (c) one population iteration on TowerBuilding --envs x 128 x 128: resample with a random map (one of eight, in turn), then
              mv_step_n(16, sequence) -- obs/s beside the same loop without the call, and beside the chain-free alternative: half the envs live, half
              savepoints, two mv_fork_envs calls per iteration (live -> savepoints, then savepoints -> live by the draw), counting the live envs'
              observations only.  Device maps and host maps; a host clock around work that ends in a device synchronise.

One JSON line per figure.   python scripts/resample_bench.py [--what fork|staged|population|all]
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
            lib = C.CDLL(path)
            lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return lib
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


def stepped_gym(MegaverseGym, scenario, N):
    g = MegaverseGym(scenario, 64, 36, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    for t in range(8):   # states that differ from what a reset leaves
        g.sample_random_actions(7, t)
        g.step()
    g.synchronize()
    return g


def settle(g):
    g.step()   # (takes the status read-backs the device-form calls left pending)
    g.synchronize()


def bench_fork_map(args, torch, MegaverseGym, np):
    N = args.envs
    m = np.array([-1] + [0] * (N - 1), np.int32)
    for scenario in ("TowerBuilding", "HexMemory"):
        g = stepped_gym(MegaverseGym, scenario, N)
        dev = torch.as_tensor(m).to("cuda")
        per_env = g.fork_bytes_per_env()
        g.resample_envs(dev)   # (the first call allocates the staging arena)
        settle(g)
        us = {"resample": [], "fork": []}
        for _ in range(2):
            us["resample"].append(round(timed(torch, lambda: g.resample_envs(dev), args.calls, args.warmup), 2)); settle(g)
            us["fork"].append(round(timed(torch, lambda: g.fork_envs(dev), args.calls, args.warmup), 2)); settle(g)
        print(json.dumps({"what": "fork_map", "scenario": scenario, "envs": N, "map": "all_from_env_0", "destinations": N - 1, "bytes_per_env": per_env,
                          "calls": args.calls, "resample_us": us["resample"], "fork_us": us["fork"],
                          "resample_minus_fork_us": round(sum(us["resample"]) / 2 - sum(us["fork"]) / 2, 2), "staging_bytes": g.resample_staging_bytes()}),
              flush=True)
        g.close()


def bench_staged(args, torch, MegaverseGym, np):
    from megaverse_amd.extension import debug_resample_plan_host
    hip = hip_runtime()
    N = args.envs
    maps = {"random_draw": np.random.default_rng(7).integers(0, N, N).astype(np.int32), "rotation": ((np.arange(N) + 1) % N).astype(np.int32)}
    for scenario in ("TowerBuilding", "HexMemory"):
        g = stepped_gym(MegaverseGym, scenario, N)
        per_env = g.fork_bytes_per_env()
        for name, m in maps.items():
            resolved, staged, _ = debug_resample_plan_host(m)
            moved, n_staged = int((resolved >= 0).sum()), int(staged.sum())
            dev = torch.as_tensor(m).to("cuda")
            g.resample_envs(dev)
            settle(g)
            us = timed(torch, lambda: g.resample_envs(dev), args.calls, args.warmup)
            settle(g)
            all_bytes, staged_bytes = moved * per_env, max(n_staged * per_env, 16)
            bufs = [torch.zeros(all_bytes, dtype=torch.uint8, device="cuda") for _ in range(3)]
            if hip is not None:
                how = "hipMemcpyAsync"

                def copy(dst, src, n):
                    hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n, 3, None)   # 3: device to device
            else:
                how = "torch copy_ (the HIP runtime was not found among the loaded libraries)"

                def copy(dst, src, n):
                    dst[:n].copy_(src[:n])
            us_two = timed(torch, lambda: (copy(bufs[1], bufs[0], staged_bytes), copy(bufs[2], bufs[1], staged_bytes)), args.calls, args.warmup)
            us_one = timed(torch, lambda: copy(bufs[1], bufs[0], all_bytes), args.calls, args.warmup)
            print(json.dumps({"what": "staged", "scenario": scenario, "envs": N, "map": name, "moved_envs": moved, "staged_envs": n_staged,
                              "bytes_per_env": per_env, "calls": args.calls, "resample_us": round(us, 2), "copy": how,
                              "two_copies_of_staged_bytes_us": round(us_two, 2), "one_copy_of_moved_bytes_us": round(us_one, 2),
                              "resample_over_two_copies": round(us / us_two, 2)}), flush=True)
            del bufs
        g.close()


def bench_population(args, torch, MegaverseGym, np):
    N, S, K = args.envs, 128, 16
    half = N // 2
    rng = np.random.default_rng(7)
    draws = [rng.integers(0, N, N).astype(np.int32) for _ in range(8)]
    # the chain-free alternative: envs 0 .. half - 1 live, the rest their savepoints
    save = np.concatenate([np.full(half, -1), np.arange(half)]).astype(np.int32)
    restores = [np.concatenate([half + rng.integers(0, half, half), np.full(N - half, -1)]).astype(np.int32) for _ in range(8)]
    for how in ("none", "resample_device", "resample_host", "savepoints_device", "savepoints_host") * 2:
        g = MegaverseGym("TowerBuilding", S, S, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        g.reset()
        ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
                torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
        script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
        dev_draws = [torch.as_tensor(m).to("cuda") for m in draws]
        dev_save, dev_restores = torch.as_tensor(save).to("cuda"), [torch.as_tensor(m).to("cuda") for m in restores]
        torch.cuda.synchronize()
        g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
        g.set_action_ring(K, script.data_ptr())
        count = [0]

        def iteration():
            i = count[0] % 8
            count[0] += 1
            if how == "resample_device":
                g.resample_envs(dev_draws[i])
            elif how == "resample_host":
                g.resample_envs(draws[i])
            elif how == "savepoints_device":
                g.fork_envs(dev_save)
                g.fork_envs(dev_restores[i])
            elif how == "savepoints_host":
                g.fork_envs(save)
                g.fork_envs(restores[i])
            g.step_n(K, "sequence", 0, 0)

        for _ in range(args.iterations_warmup):
            iteration()
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iterations):
            iteration()
        g.synchronize()
        dt = time.perf_counter() - t0
        live = half if how.startswith("savepoints") else N
        print(json.dumps({"what": "population", "how": how, "envs": N, "live_envs": live, "size": S, "ticks_per_iteration": K, "iterations": args.iterations,
                          "seconds": round(dt, 4), "live_obs_per_s": round(args.iterations * K * live / dt),
                          "us_per_iteration": round(dt / args.iterations * 1e6, 1)}), flush=True)
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["fork", "staged", "population", "all"], default="all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200, help="timed calls (at least 100)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=256)
    ap.add_argument("--iterations-warmup", type=int, default=16)
    args = ap.parse_args()
    args.calls = max(100, args.calls)
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("resample_bench: no GPU")
    if args.what in ("fork", "all"):
        bench_fork_map(args, torch, MegaverseGym, np)
    if args.what in ("staged", "all"):
        bench_staged(args, torch, MegaverseGym, np)
    if args.what in ("population", "all"):
        bench_population(args, torch, MegaverseGym, np)


if __name__ == "__main__":
    main()
