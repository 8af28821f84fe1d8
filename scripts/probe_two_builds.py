#!/usr/bin/env python
"""The host time of one stepping call, two builds of the library compared inside ONE process.  Needs a GPU.

A process that steps a gym runs in a mode of its own: between processes of the same build the host time of one call differs by a factor of two (15 to 31 us
for a call of 8 ticks on an MI355X host -- the CPU the process runs on, its clock, its neighbours), so runs of two builds in processes of their own
(scripts/probe_host_calls.py) cannot resolve a few microseconds.  Here both libmegaverse_hip.so are loaded side by side, each steps a gym of its own
(probe_host_calls.py's: TowerBuilding 1024 x 1 at 128x128, a ring of 8 slabs) in alternating blocks of calls, and the percentiles of one call's host time are
printed per build: in a device-bound loop a call either returns at once or waits for the device, so the LOW percentiles are the host cost.
    python scripts/probe_two_builds.py --a DIR --b DIR [--first a|b]     (DIR: a checkout, built; default --b: this one)
"""
import argparse
import importlib
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(tree, alias):
    """tree's megaverse_amd.extension under a package name of its own, bound to tree's library"""
    pkg = types.ModuleType(alias)
    pkg.__path__ = [os.path.join(tree, "megaverse_amd")]
    sys.modules[alias] = pkg
    os.environ["MV_LIB_PATH"] = os.path.join(tree, "megaverse_amd", "libmegaverse_hip.so")
    ext = importlib.import_module(alias + ".extension")
    ext.load_library()
    return ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="the other build's checkout")
    ap.add_argument("--b", default=ROOT)
    ap.add_argument("--first", choices=["a", "b"], default="a", help="which library is loaded and stepped first")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=12)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("probe_two_builds: no GPU")
    trees = [("a", os.path.abspath(args.a)), ("b", os.path.abspath(args.b))]
    if args.first == "b":
        trees.reverse()
    N, W = args.envs, args.size
    gyms, keep = {}, []
    for label, tree in trees:
        ext = load(tree, "mv_build_" + label)
        g = ext.MegaverseGym("TowerBuilding", W, W, N, 1, 8, False, {})
        g.set_pixel_mode("fast")
        keep.append(torch.zeros((8, N, W, W, 4), dtype=torch.uint8, device="cuda:0"))
        g.set_output_ring(8, keep[-1].data_ptr())
        g.seed(42); g.reset()
        gyms[label] = g
    times = {label: {"step_n(8)": [], "sample+step": []} for label in gyms}
    st = {label: 0 for label in gyms}
    for block in range(args.blocks):
        for label, _ in (trees if block % 2 == 0 else trees[::-1]):
            g = gyms[label]
            for what, count in (("step_n(8)", 60), ("sample+step", 120)):
                for i in range(count + 10):
                    t0 = time.perf_counter()
                    if what == "step_n(8)":
                        g.step_n(8, "multidiscrete", 1234, st[label]); st[label] += 8
                    else:
                        g.sample_random_actions(1234, st[label]); g.step(); st[label] += 1
                    if i >= 10 and block >= 2:   # (the first calls of a block fill the pipeline; the first two blocks warm up)
                        times[label][what].append(time.perf_counter() - t0)
                g.synchronize(); torch.cuda.synchronize()
    for what in ("step_n(8)", "sample+step"):
        for label, tree in sorted(trees):
            ts = np.array(times[label][what]) * 1e6
            print(f"{what:<12} {label}  p2 p5 p10 p25 p50 p75 (us): " + " ".join("%.1f" % x for x in np.percentile(ts, [2, 5, 10, 25, 50, 75])) + f"  ({len(ts)} calls)  {tree}", flush=True)
    for g in gyms.values():
        g.close()


if __name__ == "__main__":
    main()
