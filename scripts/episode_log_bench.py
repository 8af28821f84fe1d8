#!/usr/bin/env python
"""What the episode log costs (include/megaverse_hip.h: mv_set_episode_log), on the flagship shape: TowerBuilding, 1024 envs x 128 x 128.

  open loop    mv_step_n(16) with output rings 16 deep -- log off, and log on (capacity 65536, drained every 64 calls)
  closed loop  MegaverseEnv.step_device per tick with device actions (a policy in the loop) -- log off and on

One JSON line per measurement: obs/s over a host clock around work that ends in a device synchronise.  --root DIR runs the same measurement on another
checkout of this repository (the parent commit: its library has no log, so --log on is refused there); bench.py is not involved.

  python scripts/episode_log_bench.py --mode open --log off [--root /path/to/parent/checkout]
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["open", "closed"], default="open")
    ap.add_argument("--log", choices=["off", "on"], default="off")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=2048, help="open loop: timed calls of 16 ticks; closed loop: timed ticks = 16 x calls (recorded: 256)")
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    from megaverse_amd.megaverse_env import MegaverseEnv
    N, S, K, CAP = a.envs, a.size, 16, 65536
    drained = 0
    if a.mode == "open":
        g = MegaverseGym("TowerBuilding", S, S, N, 1, 1, False, {})
        g.set_pixel_mode("fast")
        g.seed(42)
        if a.log == "on":
            g.set_episode_log(CAP)
        g.reset()
        ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
                torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
        tick = 0
        for _ in range(a.warmup):
            g.step_n(K, "multidiscrete", 7, tick)
            tick += K
        g.synchronize()
        t0 = time.perf_counter()
        for c in range(a.calls):
            g.step_n(K, "multidiscrete", 7, tick)
            tick += K
            if a.log == "on" and (c + 1) % 64 == 0:
                drained += len(g.drain_episode_log())
        g.synchronize()
        dt = time.perf_counter() - t0
        ticks = a.calls * K
    else:
        # (no episode_log argument with the log off: the same call works on a checkout from before the log existed)
        env = MegaverseEnv("TowerBuilding", N, 1, img_w=S, img_h=S, **({"episode_log": CAP} if a.log == "on" else {}))
        env.seed(42)
        env.reset()
        g = env.env
        g.set_pixel_mode("fast")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        sizes = torch.tensor([3, 3, 3, 2, 2, 3], device="cuda")

        def policy(obs):   # stands for a policy that reads the frames: the actions depend on the step's observations
            r = torch.randint(0, 1 << 16, (N, 6), generator=gen, device="cuda") + obs[:, 0, 0, :6].to(torch.int64)
            return (r % sizes).to(torch.int32)

        obs = env.observations_tensor()
        ticks = a.calls * K
        for _ in range(a.warmup * 4):
            obs, _, _ = env.step_device(policy(obs))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(ticks):
            obs, _, _ = env.step_device(policy(obs))
            if a.log == "on" and (t + 1) % (64 * K) == 0:
                drained += len(g.drain_episode_log())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(json.dumps({"tag": a.tag, "mode": a.mode, "log": a.log, "envs": N, "size": S, "ticks": ticks, "seconds": round(dt, 4),
                      "obs_per_s": round(ticks * N / dt), "us_per_tick": round(dt / ticks * 1e6, 2), "records_drained": drained}), flush=True)
    g.close()


if __name__ == "__main__":
    main()
