#!/usr/bin/env python
"""What the render modes of a batched call buy (include/megaverse_hip.h: mv_step_n_render).  Needs a GPU; reads nothing outside the tree.

  calls    16-tick MV_POLICY_SEQUENCE calls on TowerBuilding and HexMemory (the long-list scenario), --envs x 1 agents at --size x --size, output rings 16
           deep, in four forms:
             every          step_n(16, 'sequence')                     = mv_step_n(16) rendered: the first form a caller had before the render modes
             no_render_x16  16 x (set_actions_device + step_no_render)   the second: one tick-only launch and one publish launch per tick
             last / none    step_n(16, 'sequence', render=...)
           Every form runs on a gym of its own; the forms alternate, --reps repetitions each (a host clock around --calls calls that end in a device
           synchronise, after --warmup calls).  -> ticks/s and us per tick, the spread of the repetitions, and the two requirements: `none` no slower per
           tick than either earlier form, `last` no slower than `every`, both beyond the spread.
  plan     one planning iteration on TowerBuilding: fork every env from env 0 (device map), a 16-tick sequence call, the running returns of the episode log
           read back to the host -- with render='none' against render='every'.

Not measured here: several agents per env, several GPUs, groups of gyms (mv_group_step keeps its own render flag).

JSON lines on stdout; the report goes to --out (default profiles/step_n_render_measured.txt; a `== kernel resources` section already in that file is kept).
    python scripts/step_n_render_bench.py [--what calls|plan|all]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 16
FORMS = ("every", "no_render_x16", "last", "none")
RESOURCES_MARK = "== kernel resources"


def make_gym(MegaverseGym, scenario, N, S, ring, script, log=0):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    if log:
        g.set_episode_log(log)
    g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
    g.set_action_ring(K, script.data_ptr())
    return g


def call_of(g, form, script):
    if form == "no_render_x16":
        def call():
            for j in range(K):
                g.set_actions_device(script[j].data_ptr())
                g.step_no_render()
        return call
    return lambda: g.step_n(K, "sequence", 0, 0, render=form)


def timed(g, call, calls, warmup):
    """seconds of `calls` back-to-back calls, the last one waited for"""
    for _ in range(warmup):
        call()
    g.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    g.synchronize()
    return time.perf_counter() - t0


def buffers(torch, np, N, S):
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def bench_calls(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    ok = True
    for scenario in ("TowerBuilding", "HexMemory"):
        us = {f: [] for f in FORMS}
        for rep in range(args.reps):
            for form in FORMS:   # (alternating: every repetition visits every form once)
                g = make_gym(MegaverseGym, scenario, N, S, ring, script)
                dt = timed(g, call_of(g, form, script), args.calls, args.warmup)
                g.close()
                us[form].append(dt / (args.calls * K) * 1e6)
                print(json.dumps({"what": "calls", "scenario": scenario, "envs": N, "size": S, "form": form, "rep": rep, "ticks": args.calls * K,
                                  "seconds": round(dt, 4), "us_per_tick": round(us[form][-1], 2), "ticks_per_s": round(args.calls * K / dt)}), flush=True)
        lines.append(f"{scenario} {N} x 1 at {S}x{S}, {K}-tick MV_POLICY_SEQUENCE calls, {args.calls} calls timed after {args.warmup}, {args.reps} repetitions")
        lines.append(f"  {'form':<15}{'us/tick (median)':>18}{'min':>9}{'max':>9}{'spread %':>10}{'ticks/s (median)':>18}")
        for form in FORMS:
            v = sorted(us[form])
            med = v[len(v) // 2]
            lines.append(f"  {form:<15}{med:>18.2f}{v[0]:>9.2f}{v[-1]:>9.2f}{(v[-1] - v[0]) / med * 100:>10.1f}{1e6 / med:>18.0f}")
        # the requirements, beyond the spread: the slowest repetition of the new form against the fastest of the old one
        for new, olds in (("none", ("every", "no_render_x16")), ("last", ("every",))):
            for old in olds:
                holds = max(us[new]) <= min(us[old])
                ok = ok and holds
                lines.append(f"  {new} no slower than {old}: {'HOLDS' if holds else 'FAILS'} beyond the spread "
                             f"(slowest {new} {max(us[new]):.2f} us/tick, fastest {old} {min(us[old]):.2f} us/tick)")
        lines.append("")
    return ok


def bench_plan(args, torch, MegaverseGym, np, lines):
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    dev_map = torch.as_tensor(np.array([-1] + [0] * (N - 1), np.int32)).to("cuda")
    us = {"every": [], "none": []}
    for rep in range(args.reps):
        for mode in ("every", "none"):
            g = make_gym(MegaverseGym, "TowerBuilding", N, S, ring, script, log=4096)
            returns = g.episode_returns_tensor()

            def iteration():
                g.fork_envs(dev_map)
                g.step_n(K, "sequence", 0, 0, render=mode)
                return returns.cpu()   # (the gym's stream is torch's current one: the copy waits for the call)

            dt = timed(g, iteration, args.plan_iterations, args.warmup)
            g.close()
            us[mode].append(dt / args.plan_iterations * 1e6)
            print(json.dumps({"what": "plan", "render": mode, "envs": N, "size": S, "rep": rep, "iterations": args.plan_iterations, "seconds": round(dt, 4),
                              "us_per_iteration": round(us[mode][-1], 1), "env_ticks_per_s": round(args.plan_iterations * K * N / dt)}), flush=True)
    lines.append(f"One planning iteration, TowerBuilding {N} x 1 at {S}x{S}: fork every env from env 0 (device map), a {K}-tick sequence call, the episode")
    lines.append(f"log's running returns copied to the host; {args.plan_iterations} iterations timed after {args.warmup}, {args.reps} repetitions")
    lines.append(f"  {'render':<15}{'us/iteration (median)':>23}{'min':>10}{'max':>10}{'env ticks/s (median)':>22}")
    for mode in ("every", "none"):
        v = sorted(us[mode])
        med = v[len(v) // 2]
        lines.append(f"  {mode:<15}{med:>23.1f}{v[0]:>10.1f}{v[-1]:>10.1f}{K * N * 1e6 / med:>22.0f}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["calls", "plan", "all"], default="all")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=1536, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plan-iterations", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_n_render_measured.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("step_n_render_bench: no GPU")
    lines = ["Render modes of batched calls (mv_step_n_render): measured by scripts/step_n_render_bench.py on " + torch.cuda.get_device_name(0) + " (" + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every form on a gym of its own, the forms alternating within each repetition.",
             "spread % = (max - min) / median of the repetitions.  Not measured: several agents per env, several GPUs, groups of gyms.", ""]
    ok = True
    if args.what in ("calls", "all"):
        ok = bench_calls(args, torch, MegaverseGym, np, lines)
    if args.what in ("plan", "all"):
        bench_plan(args, torch, MegaverseGym, np, lines)
    kept = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if RESOURCES_MARK in old:
            kept = old[old.index(RESOURCES_MARK):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)
    if not ok:
        print("step_n_render_bench: a requirement FAILS (see the report)", file=sys.stderr)


if __name__ == "__main__":
    main()
