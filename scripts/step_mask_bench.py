#!/usr/bin/env python
"""What step masks cost and buy (include/megaverse_hip.h: mv_set_step_mask).  Needs a GPU; reads nothing outside the tree.

  nomask   the 16-tick render='none' MV_POLICY_SEQUENCE call of scripts/step_n_render_bench.py on TowerBuilding, no mask attached: us per tick.  Run it on
           the parent commit and on this one alternately (the section uses nothing the parent lacks; --label names the build in the JSON line): a mask
           that is not attached must cost nothing.  --tree DIR imports the package from another checkout (the parent's, built).
  frozen   TowerBuilding and HexMemory, --envs x 1 agents at --size x --size, 16-tick sequence calls with 100 % of the envs stepping (no mask), 50 %
           (every odd env frozen, host form) and 0 % (an all-zero mask), for render='none' and 'every': us per tick.
  plan     the savepoint planner -- env 0 frozen as the root; per iteration: fork every other env from env 0 (device map), a 16-tick render='none' call,
           the episode log's running returns copied to the host -- against the scheme a root needed before (scripts/resample_bench.py's): half the envs
           live, half savepoints, two fork calls per iteration (live -> savepoints, savepoints -> live), the same call and read-back.

Not measured here: several agents per env, the episode log on in the `frozen` section, several GPUs.

JSON lines on stdout; the report of `frozen` and `plan` goes to --out (default profiles/step_mask_measured.txt is assembled by hand from these runs and the
parent-against-this-commit runs: the script writes a file only where --out says so).
    python scripts/step_mask_bench.py [--what nomask|frozen|plan|all] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16


def buffers(torch, np, N, S, obs=True):
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda") if obs else None, torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def make_gym(MegaverseGym, scenario, N, S, ring, script, log=0):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    if log:
        g.set_episode_log(log)
    g.set_output_ring(K, ring[0].data_ptr() if ring[0] is not None else 0, ring[1].data_ptr(), ring[2].data_ptr())
    g.set_action_ring(K, script.data_ptr())
    return g


def timed(g, call, calls, warmup):
    for _ in range(warmup):
        call()
    g.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    g.synchronize()
    return time.perf_counter() - t0


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def bench_nomask(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    us = []
    for rep in range(args.reps):
        g = make_gym(MegaverseGym, "TowerBuilding", N, S, ring, script)
        dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render="none"), args.calls, args.warmup)
        g.close()
        us.append(dt / (args.calls * K) * 1e6)
        print(json.dumps({"what": "nomask", "label": args.label, "scenario": "TowerBuilding", "envs": N, "size": S, "render": "none", "rep": rep,
                          "ticks": args.calls * K, "seconds": round(dt, 4), "us_per_tick": round(us[-1], 3)}), flush=True)
    lines.append(f"nomask [{args.label}]: TowerBuilding {N} x 1 at {S}x{S}, {K}-tick render='none' calls, no mask: us/tick per repetition "
                 + " ".join(f"{u:.3f}" for u in us) + f", median {median(us):.3f}")
    lines.append("")


def bench_frozen(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    shares = (("100 % step (no mask)", None), ("50 % step", np.arange(N) % 2 == 0), ("0 % step", np.zeros(N, bool)))
    for scenario in ("TowerBuilding", "HexMemory"):
        lines.append(f"{scenario} {N} x 1 at {S}x{S}, {K}-tick MV_POLICY_SEQUENCE calls, {args.calls} calls timed after {args.warmup}, {args.reps} repetitions; "
                     "us per tick, median (min - max)")
        for render in ("none", "every"):
            us = {name: [] for name, _ in shares}
            for rep in range(args.reps):
                for name, mask in shares:   # (alternating: every repetition visits every share once)
                    g = make_gym(MegaverseGym, scenario, N, S, ring, script)
                    g.set_step_mask(mask)
                    dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=render), args.calls, args.warmup)
                    g.close()
                    us[name].append(dt / (args.calls * K) * 1e6)
                    print(json.dumps({"what": "frozen", "scenario": scenario, "envs": N, "size": S, "render": render, "share": name, "rep": rep,
                                      "ticks": args.calls * K, "seconds": round(dt, 4), "us_per_tick": round(us[name][-1], 2)}), flush=True)
            for name, _ in shares:
                v = us[name]
                lines.append(f"  render={render:<6} {name:<22}{median(v):>9.2f}  ({min(v):.2f} - {max(v):.2f})")
        lines.append("")


def bench_plan(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    half = N // 2
    ring, script = buffers(torch, np, N, S, obs=False)
    dev = lambda m: torch.as_tensor(np.asarray(m, np.int32)).to("cuda")   # noqa: E731
    root_map = dev([-1] + [0] * (N - 1))
    save = dev(np.concatenate([np.full(half, -1), np.arange(half)]))
    rng = np.random.default_rng(7)
    restores = [dev(np.concatenate([half + rng.integers(0, half, half), np.full(N - half, -1)])) for _ in range(8)]
    torch.cuda.synchronize()
    us = {"frozen_root": [], "refork_savepoints": []}
    for rep in range(args.reps):
        for how in us:
            g = make_gym(MegaverseGym, "TowerBuilding", N, S, ring, script, log=4096)
            returns = g.episode_returns_tensor()
            count = [0]
            if how == "frozen_root":
                g.set_step_mask(np.arange(N) != 0)

            def iteration():
                if how == "frozen_root":
                    g.fork_envs(root_map)
                else:
                    g.fork_envs(save)
                    g.fork_envs(restores[count[0] % 8])
                count[0] += 1
                g.step_n(K, "sequence", 0, 0, render="none")
                return returns.cpu()   # (the gym's stream is torch's current one: the copy waits for the call)

            dt = timed(g, iteration, args.plan_iterations, args.warmup)
            g.close()
            live = N - 1 if how == "frozen_root" else half
            us[how].append(dt / args.plan_iterations * 1e6)
            print(json.dumps({"what": "plan", "how": how, "envs": N, "live_envs": live, "size": S, "rep": rep, "iterations": args.plan_iterations,
                              "seconds": round(dt, 4), "us_per_iteration": round(us[how][-1], 1),
                              "live_env_ticks_per_s": round(args.plan_iterations * K * live / dt)}), flush=True)
    lines.append(f"Planning iteration, TowerBuilding {N} x 1 at {S}x{S}, a {K}-tick render='none' sequence call + the episode log's running returns copied to the")
    lines.append(f"host; {args.plan_iterations} iterations timed after {args.warmup}, {args.reps} repetitions; us per iteration, median (min - max); live env ticks/s")
    for how, live in (("frozen_root", N - 1), ("refork_savepoints", half)):
        v = us[how]
        what = "env 0 frozen as the root, one fork per iteration" if how == "frozen_root" else "half live, half savepoints, two forks per iteration"
        lines.append(f"  {how:<18}{median(v):>9.1f}  ({min(v):.1f} - {max(v):.1f}){K * live * 1e6 / median(v):>14.0f}   {what}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["nomask", "frozen", "plan", "all"], default="all")
    ap.add_argument("--label", default="this commit", help="nomask: the build's name in the JSON line")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=512, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plan-iterations", type=int, default=512)
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose megaverse_amd is measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("step_mask_bench: no GPU")
    lines = ["Step masks (mv_set_step_mask): measured by scripts/step_mask_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every form on a gym of its own, the forms alternating within each repetition.", ""]
    if args.what in ("nomask", "all"):
        bench_nomask(args, torch, MegaverseGym, np, lines)
    if args.what in ("frozen", "all"):
        bench_frozen(args, torch, MegaverseGym, np, lines)
    if args.what in ("plan", "all"):
        bench_plan(args, torch, MegaverseGym, np, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
