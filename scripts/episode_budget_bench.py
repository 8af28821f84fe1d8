#!/usr/bin/env python
"""What episode budgets cost and buy (include/megaverse_hip.h: mv_set_episode_budget).  Needs a GPU; reads nothing outside the tree.

  nobudget  the 16-tick render='none' MV_POLICY_SEQUENCE call of scripts/step_mask_bench.py on TowerBuilding, nothing attached: us per tick.  Run it on the
            parent commit and on this one alternately (the section uses nothing the parent lacks; --label names the build in the JSON line; --tree DIR
            imports the package from another checkout, built): a budget that is not attached must cost nothing.
  budget    TowerBuilding and HexMemory, --envs x 1 agents at --size x --size, episodeLengthSec 4.3 (the shortest episodes the library still steps in
            resident multi-tick launches), 16-tick sequence render='none' calls: no budget; -1 everywhere; budget 1 over the first calls from the reset
            (hardly anybody has halted yet); budget 1 once everybody has halted: us per tick.
  usecase   "one episode per env": MegaverseEnv.run_episodes(1) (calls of recommended_ticks_per_call() ticks, render='none', the halted count read once
            per call) against the emulation it replaces -- one-tick calls, mask &= ~done in torch and a device-form set_step_mask after every tick (the
            parent's API, unchanged), "anybody left?" asked every 16 ticks: wall time per evaluation, env ticks per second.

Not measured here: several agents per env, several GPUs.

JSON lines on stdout, the report to --out where given (profiles/episode_budget_measured.txt is assembled by hand from these runs and bench.py's).
    python scripts/episode_budget_bench.py [--what nobudget|budget|usecase|all] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16
SHORT = {"episodeLengthSec": 4.3}


def buffers(torch, np, N):
    ring = (torch.zeros((K, N), dtype=torch.float32, device="cuda"), torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def make_gym(MegaverseGym, scenario, N, S, ring, script, params=None):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, params or {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    g.set_output_ring(K, 0, ring[0].data_ptr(), ring[1].data_ptr())
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


def bench_nobudget(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N)
    us = []
    for rep in range(args.reps):
        g = make_gym(MegaverseGym, "TowerBuilding", N, S, ring, script)
        dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render="none"), args.calls, args.warmup)
        g.close()
        us.append(dt / (args.calls * K) * 1e6)
        print(json.dumps({"what": "nobudget", "label": args.label, "scenario": "TowerBuilding", "envs": N, "size": S, "render": "none", "rep": rep,
                          "ticks": args.calls * K, "seconds": round(dt, 4), "us_per_tick": round(us[-1], 3)}), flush=True)
    lines.append(f"nobudget [{args.label}]: TowerBuilding {N} x 1 at {S}x{S}, {K}-tick render='none' calls, nothing attached: us/tick per repetition "
                 + " ".join(f"{u:.3f}" for u in us) + f", median {median(us):.3f}")
    lines.append("")


def bench_budget(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N)
    call_of = lambda g: (lambda: g.step_n(K, "sequence", 0, 0, render="none"))   # noqa: E731
    for scenario in ("TowerBuilding", "HexMemory"):
        us = {"no budget": [], "-1 everywhere": [], "budget 1, from the reset": [], "budget 1, everybody halted": []}
        ticks_to_halt, early = [], []
        for rep in range(args.reps):
            for name in list(us)[:3]:   # (alternating: every repetition visits every form once)
                g = make_gym(MegaverseGym, scenario, N, S, ring, script, SHORT)
                if name != "no budget":
                    g.set_episode_budget(-1 if name.startswith("-1") else 1)
                dt = timed(g, call_of(g), args.short_calls, args.warmup)
                us[name].append(dt / (args.short_calls * K) * 1e6)
                if name.startswith("budget 1"):
                    early.append(g.halted_count())
                    ticks = (args.short_calls + args.warmup) * K
                    while g.halted_count() < N:   # (one read per 16 calls)
                        for _ in range(16):
                            g.step_n(K, "sequence", 0, 0, render="none")
                        ticks += 16 * K
                        assert ticks < 200000, "the envs do not halt"
                    ticks_to_halt.append(ticks)
                    dt = timed(g, call_of(g), args.calls, args.warmup)
                    us["budget 1, everybody halted"].append(dt / (args.calls * K) * 1e6)
                g.close()
            print(json.dumps({"what": "budget", "scenario": scenario, "envs": N, "size": S, "rep": rep, "ticks_until_everybody_halted": ticks_to_halt[-1],
                              "us_per_tick": {k: round(v[-1], 2) for k, v in us.items()}}), flush=True)
        lines.append(f"{scenario} {N} x 1 at {S}x{S}, episodeLengthSec 4.3, {K}-tick MV_POLICY_SEQUENCE render='none' calls, {args.reps} repetitions; "
                     "us per tick, median (min - max)")
        for name, v in us.items():
            lines.append(f"  {name:<30}{median(v):>9.2f}  ({min(v):.2f} - {max(v):.2f})")
        lines.append(f"  (the first three over {args.short_calls} calls from the reset -- {max(early)} of {N} envs had halted by their end -- the last over "
                     f"{args.calls} calls; everybody had halted within {max(ticks_to_halt)} ticks, looked at every 256)")
        lines.append("")


def bench_usecase(args, torch, MegaverseEnv, np, lines):
    N, S = args.envs, args.size
    res = {"run_episodes": [], "emulation": []}
    for rep in range(args.reps):
        for how in res:
            env = MegaverseEnv("TowerBuilding", N, 1, params=dict(SHORT), img_w=S, img_h=S)
            env.seed(42)
            env.reset()
            env.observations_tensor()
            g = env.env
            g.set_pixel_mode("fast")
            g.set_episode_log(N)
            if how == "run_episodes":
                g.synchronize()
                t0 = time.perf_counter()
                records = env.run_episodes(1, seed=7)
                dt = time.perf_counter() - t0
                ticks = int(records["length"].sum())
                assert len(records) == N
            else:
                dones = torch.zeros((1, N), dtype=torch.uint8, device="cuda")
                rewards = torch.zeros((1, N), dtype=torch.float32, device="cuda")
                mask = torch.ones(N, dtype=torch.bool, device="cuda")
                torch.cuda.synchronize()
                g.set_output_ring(1, 0, rewards.data_ptr(), dones.data_ptr())
                g.synchronize()
                t0 = time.perf_counter()
                t = 0
                while True:
                    g.set_step_mask(mask)
                    g.step_n(1, "multidiscrete", 7, t, render="none")
                    mask &= dones[0] == 0
                    t += 1
                    if t % K == 0 and not bool(mask.any()):   # (one read per 16 ticks, as run_episodes' one per call)
                        break
                dt = time.perf_counter() - t0
                records = g.drain_episode_log()
                ticks = int(records["length"].sum())
                assert len(records) == N, len(records)
            env.close()
            res[how].append((dt, ticks))
            print(json.dumps({"what": "usecase", "how": how, "envs": N, "size": S, "rep": rep, "seconds": round(dt, 4), "env_ticks": ticks,
                              "env_ticks_per_s": round(ticks / dt)}), flush=True)
    lines.append(f"One episode per env, TowerBuilding {N} x 1 at {S}x{S}, episodeLengthSec 4.3, random policy, nothing drawn, the episode log on; {args.reps} "
                 "repetitions; wall time per evaluation in ms, median (min - max); env ticks/s")
    for how, what in (("run_episodes", "MegaverseEnv.run_episodes(1): budget 1, calls of 16 ticks, one halted-count read per call"),
                      ("emulation", "one-tick calls, mask &= ~done in torch, set_step_mask per tick (the parent's API)")):
        v = sorted(res[how])
        dt, ticks = v[len(v) // 2]
        lines.append(f"  {how:<14}{dt * 1e3:>9.1f}  ({v[0][0] * 1e3:.1f} - {v[-1][0] * 1e3:.1f}){ticks / dt:>14.0f}   {what}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["nobudget", "budget", "usecase", "all"], default="all")
    ap.add_argument("--label", default="this commit", help="nobudget: the build's name in the JSON line")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=512, help="timed 16-tick calls per repetition")
    ap.add_argument("--short-calls", type=int, default=24, help="budget: timed calls while nobody has halted yet")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose megaverse_amd is measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    from megaverse_amd.megaverse_env import MegaverseEnv
    if not torch.cuda.is_available():
        sys.exit("episode_budget_bench: no GPU")
    lines = ["Episode budgets (mv_set_episode_budget): measured by scripts/episode_budget_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every form on a gym of its own, the forms alternating within each repetition.", ""]
    if args.what in ("nobudget", "all"):
        bench_nobudget(args, torch, MegaverseGym, np, lines)
    if args.what in ("budget", "all"):
        bench_budget(args, torch, MegaverseGym, np, lines)
    if args.what in ("usecase", "all"):
        bench_usecase(args, torch, MegaverseEnv, np, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
