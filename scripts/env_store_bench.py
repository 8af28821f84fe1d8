#!/usr/bin/env python
"""What env stores cost (include/megaverse_hip.h: mv_save_envs / mv_load_envs).  Needs a GPU; reads nothing outside the tree.

  store    mv_save_envs and mv_load_envs (device maps) timed with HIP events on the gym's stream over --calls back-to-back calls after a warm-up, for
           TowerBuilding and HexMemory (the largest per-env state) with --envs envs: every env to / from its own record, and the odd envs only.  Next to
           them, on the same build and in the same run: mv_fork_envs of the same destinations (the odd envs from their even neighbours -- a fork cannot
           write every env) and ONE hipMemcpyAsync device to device of the same number of bytes.  A save or a load moves the bytes a fork moves: the
           fork's time is the bar, the plain copy the floor.
  plan     one "deep savepoint" planning iteration on TowerBuilding --envs x 128 x 128: load every env from --envs records picked out of a store of
           --store-slots, mv_step_n(16, sequence, render=none), save every env back -- beside the fork-based iteration of scripts/fork_bench.py (fork every
           env from env 0, the same call) and the call alone (a host clock around work that ends in a device synchronise).

One JSON line per figure, on stdout and appended to --out.   python scripts/env_store_bench.py [--what store|plan|all] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fork_bench import hip_runtime, timed  # noqa: E402

OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def bench_store(args, torch, MegaverseGym, np):
    hip = hip_runtime()
    if hip is not None:
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    N = args.envs
    own = np.arange(N, dtype=np.int32)
    maps = {"every_env": own, "odd_envs": np.where(own % 2 == 1, own, -1).astype(np.int32)}
    fork_map = np.array([-1 if d % 2 == 0 else d - 1 for d in range(N)], np.int32)
    for scenario in ("TowerBuilding", "HexMemory"):
        g = MegaverseGym(scenario, 64, 36, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        g.reset()
        for t in range(8):   # states that differ from what a reset leaves
            g.sample_random_actions(7, t)
            g.step()
        g.synchronize()
        record, per_env = g.env_record_bytes(), g.fork_bytes_per_env()
        store = g.new_env_store(N)
        g.save_envs(own, store)
        dev_fork = torch.as_tensor(fork_map).to("cuda")
        us_fork = timed(torch, lambda: g.fork_envs(dev_fork), args.calls, args.warmup)
        g.step(); g.synchronize()   # (takes the status read-backs the device-form calls left pending)
        for name, m in maps.items():
            dev = torch.as_tensor(m).to("cuda")
            count = int((m >= 0).sum())
            nbytes = count * record
            us_save = timed(torch, lambda: g.save_envs(dev, store), args.calls, args.warmup)
            g.step(); g.synchronize()
            us_load = timed(torch, lambda: g.load_envs(dev, store), args.calls, args.warmup)
            g.step(); g.synchronize()
            src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            if hip is not None:
                copy, how = (lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None)), "hipMemcpyAsync"   # 3: device to device
            else:
                copy, how = (lambda: dst.copy_(src)), "torch copy_ (the HIP runtime was not found among the loaded libraries)"
            us_copy = timed(torch, copy, args.calls, args.warmup)
            rec = {"what": "store", "scenario": scenario, "envs": N, "map": name, "records": count, "record_bytes": record, "fork_bytes_per_env": per_env,
                   "bytes_per_call": nbytes, "calls": args.calls, "save_us": round(us_save, 2), "load_us": round(us_load, 2), "copy": how,
                   "copy_us": round(us_copy, 2), "save_over_copy": round(us_save / us_copy, 2), "load_over_copy": round(us_load / us_copy, 2)}
            if name == "odd_envs":   # the fork of the same destinations
                rec.update({"fork_us": round(us_fork, 2), "save_over_fork": round(us_save / us_fork, 2), "load_over_fork": round(us_load / us_fork, 2)})
            emit(rec)
        g.close()


def bench_plan(args, torch, MegaverseGym, np):
    N, S, K = args.envs, 128, 16
    rng = np.random.default_rng(7)
    for mode in ("none", "fork_from_env_0", "load_and_save") * 2:
        g = MegaverseGym("TowerBuilding", S, S, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        g.reset()
        ring = (torch.zeros((K, N), dtype=torch.float32, device="cuda"), torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
        script = torch.as_tensor((rng.integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
        fork_map = torch.as_tensor(np.array([-1] + [0] * (N - 1), np.int32)).to("cuda")
        torch.cuda.synchronize()
        g.set_output_ring(K, 0, ring[0].data_ptr(), ring[1].data_ptr())
        g.set_action_ring(K, script.data_ptr())
        store = slot_maps = None
        if mode == "load_and_save":
            slots = max(args.store_slots, N)
            store = g.new_env_store(slots)
            for first in range(0, slots - N + 1, N):   # every record of the store holds an episode
                g.save_envs(torch.arange(first, first + N, dtype=torch.int32, device="cuda"), store)
                g.step_n(K, "sequence", 0, 0, render="none")
            g.synchronize()
            filled = (slots // N) * N
            slot_maps = [torch.as_tensor(rng.permutation(filled)[:N].astype(np.int32)).to("cuda") for _ in range(8)]
            torch.cuda.synchronize()
        count = [0]

        def iteration():
            if mode == "fork_from_env_0":
                g.fork_envs(fork_map)
            elif mode == "load_and_save":
                m = slot_maps[count[0] % len(slot_maps)]
                g.load_envs(m, store)
            g.step_n(K, "sequence", 0, 0, render="none")
            if mode == "load_and_save":
                g.save_envs(m, store)
            count[0] += 1

        for _ in range(args.plan_warmup):
            iteration()
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.plan_iterations):
            iteration()
        g.synchronize()
        dt = time.perf_counter() - t0
        emit({"what": "plan", "mode": mode, "envs": N, "size": S, "ticks_per_iteration": K, "render": "none", "iterations": args.plan_iterations,
              "store_slots": 0 if store is None else int(store.shape[0]), "seconds": round(dt, 4), "env_ticks_per_s": round(args.plan_iterations * K * N / dt),
              "us_per_iteration": round(dt / args.plan_iterations * 1e6, 1)})
        g.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["store", "plan", "all"], default="all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200, help="timed calls (at least 100)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--store-slots", type=int, default=8192)
    ap.add_argument("--plan-iterations", type=int, default=256)
    ap.add_argument("--plan-warmup", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "env_store_measured.txt"))
    args = ap.parse_args()
    args.calls = max(100, args.calls)
    OUT = args.out
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("env_store_bench: no GPU")
    if args.what in ("store", "all"):
        bench_store(args, torch, MegaverseGym, np)
    if args.what in ("plan", "all"):
        bench_plan(args, torch, MegaverseGym, np)


if __name__ == "__main__":
    main()
