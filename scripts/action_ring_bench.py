#!/usr/bin/env python
"""What replaying given actions costs (include/megaverse_hip.h: mv_set_action_ring), on the flagship shape: TowerBuilding, 1024 envs x 128 x 128, calls of 16
ticks into output rings 16 deep.

  random     mv_step_n(16, multidiscrete): the batched call with actions drawn inside the step kernel -- the yardstick
  sequence   mv_step_n(16, sequence) out of an action ring of 256 entries (a static script: one mv_set_action_ring before the run)
  single     mv_set_actions_device + mv_step per tick for the same script: what a caller with known actions had before

One JSON line per measurement: obs/s over a host clock around work that ends in a device synchronise.  --root DIR runs the same measurement on another
checkout of this repository (the parent commit: its library has no action ring, so only --mode random and --mode single run there); bench.py is not involved.

  python scripts/action_ring_bench.py --mode random [--root /path/to/parent/checkout]
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["random", "sequence", "single"], default="random")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=1024, help="timed calls of 16 ticks (single: 16 x calls ticks)")
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--entries", type=int, default=256, help="entries of the action ring")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    N, S, K = a.envs, a.size, 16
    g = MegaverseGym("TowerBuilding", S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    # the script: the uniform policy's own distribution, so that the three modes simulate alike
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (a.entries, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    if a.mode == "sequence":
        g.set_action_ring(a.entries, script.data_ptr())
    ptrs = [script[e].data_ptr() for e in range(a.entries)]
    tick = 0

    def call():
        nonlocal tick
        if a.mode == "single":
            for j in range(K):
                g.set_actions_device(ptrs[(tick + j) % a.entries])
                g.step()
        else:
            g.step_n(K, "multidiscrete" if a.mode == "random" else "sequence", 7, tick)
        tick += K

    for _ in range(a.warmup):
        call()
    g.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        call()
    g.synchronize()
    dt = time.perf_counter() - t0
    ticks = a.calls * K
    print(json.dumps({"tag": a.tag, "mode": a.mode, "envs": N, "size": S, "ticks": ticks, "seconds": round(dt, 4), "obs_per_s": round(ticks * N / dt),
                      "us_per_tick": round(dt / ticks * 1e6, 2)}), flush=True)
    g.close()


if __name__ == "__main__":
    main()
