#!/usr/bin/env python
"""What state observations cost (include/megaverse_hip.h: mv_set_state_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each (every run a process of its own): bench.py's
           headline (agent observations/s).  --parent DIR: the parent's checkout, built.  The report gives both ranges and says whether this commit's median
           lies inside the parent's own run-to-run spread.
  calls    TowerBuilding and HexMemory, --envs x 1 agents at --size x --size, 16-tick MV_POLICY_SEQUENCE calls into rings, rendered and render='none', with
           the buffer off and on: us per tick -- what the MASKED instantiation of the step kernels plus the publish launch cost.
  masked   what the change costs a gym that already runs the MASKED step kernels and attaches no buffer: an all-ones step mask, the parent commit against
           this one, --reps alternating runs each (a process of its own per run), the 16-tick call rendered and render='none' on TowerBuilding: us per tick.
  plan     the planner iteration -- a fork of every env from env 0 and 16 render='none' ticks -- reading the returns from the episode log's running sums,
           and reading the returns plus the last tick's state rows: us per iteration.

Not measured here: several agents per env, several GPUs.

JSON lines on stdout; the report goes to --out.
    python scripts/state_obs_bench.py [--what off|masked|calls|plan|all] [--parent DIR] [--out profiles/state_obs_measured.txt]
"""
import argparse
import json
import os
import subprocess
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


def make_gym(MegaverseGym, scenario, N, S, ring, script, log=0, state=False):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    if log:
        g.set_episode_log(log)
    g.set_output_ring(K, ring[0].data_ptr() if ring[0] is not None else 0, ring[1].data_ptr(), ring[2].data_ptr())
    g.set_action_ring(K, script.data_ptr())
    if state:   # (behind the ring: one entry per ring entry)
        g.set_state_obs(True)
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


def spread(v, fmt="{:.2f}"):
    return f"{fmt.format(median(v)):>10}  ({fmt.format(min(v))} - {fmt.format(max(v))})"


def imports(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("state_obs_bench: no GPU")
    return np, torch, MegaverseGym


def run_json(cmd, cwd, key):
    """the last JSON line of a child's stdout that has `key`"""
    out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and f'"{key}"' in line:
            return json.loads(line)
    sys.exit(f"state_obs_bench: {' '.join(cmd)} printed no result\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")


def bench_off(args, lines):
    trees = (("parent", os.path.abspath(args.parent)), ("this commit", ROOT))
    obs = {name: [] for name, _ in trees}
    for rep in range(args.reps):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):   # (alternating, and which build goes first alternates too)
            line = run_json([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                             "--no-cpu-baseline", "--no-extra-legs"], tree, "value")
            obs[name].append(line["value"])
            print(json.dumps({"what": "off", "label": name, "rep": rep, "bench_py_value": line["value"], "unit": line.get("unit")}), flush=True)
    lines.append(f"(a) Nothing attached: the parent commit against this one, {args.reps} alternating runs each (parent first in the even repetitions, this commit "
                 "first in the odd ones), every run a process of its own.")
    lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-extra-legs, agent observations/s (higher is better):")
    for name, _ in trees:
        lines.append(f"  {name:<12} " + " ".join(f"{v / 1e6:.3f}M" for v in obs[name]) + f"   median {median(obs[name]) / 1e6:.3f}M"
                     f"   range {min(obs[name]) / 1e6:.3f}M - {max(obs[name]) / 1e6:.3f}M")
    m = median(obs["this commit"])
    inside = min(obs["parent"]) <= m <= max(obs["parent"])
    lines.append(f"  this commit's median {m / 1e6:.3f}M lies " + ("INSIDE" if inside else "above" if m > max(obs["parent"]) else "BELOW")
                 + f" the parent's own spread {min(obs['parent']) / 1e6:.3f}M - {max(obs['parent']) / 1e6:.3f}M.")
    lines.append("")


def child_call16(args):
    """(a process of its own, --what call16 --tree DIR) one gym of the tree's library with an all-ones step mask and no state buffer: us per tick of the
    16-tick call with --render"""
    np, torch, MegaverseGym = imports(args.tree)
    ring, script = buffers(torch, np, args.envs, args.size, obs=args.render != "none")
    g = make_gym(MegaverseGym, "TowerBuilding", args.envs, args.size, ring, script)
    g.set_step_mask(np.ones(args.envs, bool))
    dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=args.render), args.calls, args.warmup)
    g.close()
    print(json.dumps({"what": "call16", "label": args.label, "render": args.render, "us_per_tick": round(dt / (args.calls * K) * 1e6, 3)}), flush=True)


def bench_masked(args, lines):
    trees = (("parent", os.path.abspath(args.parent)), ("this commit", ROOT))
    us = {(name, render): [] for name, _ in trees for render in ("every", "none")}
    for rep in range(args.reps):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):   # (alternating, and which build goes first alternates too)
            for render in ("every", "none"):
                cmd = [sys.executable, os.path.abspath(__file__), "--what", "call16", "--tree", tree, "--label", name, "--render", render, "--envs",
                       str(args.envs), "--size", str(args.size), "--calls", str(args.calls), "--warmup", str(args.warmup)]
                line = run_json(cmd, ROOT, "us_per_tick")
                print(json.dumps(dict(line, what="masked", rep=rep)), flush=True)
                us[(name, render)].append(line["us_per_tick"])
    lines.append(f"(d) The MASKED step kernels with NO buffer attached -- what a step-mask, budget or draw-mask user pays for this change: TowerBuilding {args.envs} x 1 at")
    lines.append(f"{args.size}x{args.size}, an all-ones step mask, {K}-tick MV_POLICY_SEQUENCE calls, the parent commit against this one, {args.reps} alternating runs each (a process of")
    lines.append("its own per run, the builds taking turns going first); us per tick, median (min - max).")
    for render, title in (("every", "rendered"), ("none", "render='none'")):
        for name, _ in trees:
            lines.append(f"  {title + ', ' + name:<28}{spread(us[(name, render)])}")
    lines.append("")


def bench_calls(args, lines):
    np, torch, MegaverseGym = imports(ROOT)
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    forms = (("rendered, buffer off", "every", False), ("rendered, buffer on", "every", True), ("render='none', buffer off", "none", False),
             ("render='none', buffer on", "none", True))
    lines.append(f"(b) {N} x 1 at {S}x{S}, {K}-tick MV_POLICY_SEQUENCE calls into rings, {args.calls} calls timed after {args.warmup}, {args.share_reps} "
                 "repetitions, the forms alternating within each; us per tick, median (min - max).  Buffer on: the MASKED step kernels + one publish launch per call.")
    for scenario in ("TowerBuilding", "HexMemory"):
        us = {name: [] for name, _, _ in forms}
        for rep in range(args.share_reps):
            for name, render, state in forms:
                g = make_gym(MegaverseGym, scenario, N, S, ring, script, state=state)
                dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=render), args.calls, args.warmup)
                g.close()
                us[name].append(dt / (args.calls * K) * 1e6)
                print(json.dumps({"what": "calls", "scenario": scenario, "envs": N, "size": S, "form": name, "rep": rep, "ticks": args.calls * K,
                                  "seconds": round(dt, 4), "us_per_tick": round(us[name][-1], 2)}), flush=True)
        lines.append(f"{scenario}")
        for name, _, _ in forms:
            lines.append(f"  {name:<28}{spread(us[name])}")
    lines.append("")


def bench_plan(args, lines):
    np, torch, MegaverseGym = imports(ROOT)
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S, obs=False)
    root_map = torch.as_tensor(np.asarray([-1] + [0] * (N - 1), np.int32)).to("cuda")
    torch.cuda.synchronize()
    us = {"returns from the log": [], "returns + state rows": []}
    for rep in range(args.share_reps):
        for how in us:
            state = how != "returns from the log"
            g = make_gym(MegaverseGym, "TowerBuilding", N, S, ring, script, log=4 * N, state=state)
            returns = g.episode_returns_tensor()
            rows = g.state_obs()
            sink = [None, None]

            def iteration():
                g.fork_envs(root_map)
                g.step_n(K, "sequence", 0, 0, render="none")
                sink[0] = returns.to(torch.float32).argmax()           # (what a planner does with them: a device-side reduction, no host wait)
                if state:
                    sink[1] = rows[K - 1, :, 1].argmax()               # (height reached: column pos_y of the call's last tick)

            dt = timed(g, iteration, args.plan_iterations, args.warmup)
            torch.cuda.synchronize()
            g.close()
            us[how].append(dt / args.plan_iterations * 1e6)
            print(json.dumps({"what": "plan", "how": how, "envs": N, "size": S, "rep": rep, "iterations": args.plan_iterations, "seconds": round(dt, 4),
                              "us_per_iteration": round(us[how][-1], 1)}), flush=True)
    lines.append(f"(c) The planner iteration, TowerBuilding {N} x 1 at {S}x{S}: a fork of every other env from env 0 (device map), a {K}-tick render='none' sequence")
    lines.append(f"call, then a device-side argmax over the episode log's running returns -- and, second form, over column pos_y of the last tick's state rows as well;")
    lines.append(f"{args.plan_iterations} iterations timed after {args.warmup}, {args.share_reps} repetitions; us per iteration, median (min - max).")
    for how, v in us.items():
        lines.append(f"  {how:<22}{spread(v, '{:.1f}')}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["off", "masked", "calls", "plan", "all", "call16"], default="all")
    ap.add_argument("--parent", default="", help="the parent commit's checkout, built (off, masked)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=256, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5, help="off: alternating runs of each build")
    ap.add_argument("--share-reps", type=int, default=3, help="calls, plan: repetitions")
    ap.add_argument("--plan-iterations", type=int, default=256)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    ap.add_argument("--tree", default=ROOT, help="call16: the checkout whose megaverse_amd is measured")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--render", default="none")
    args = ap.parse_args()
    if args.what == "call16":
        return child_call16(args)
    if args.what in ("off", "masked", "all") and not args.parent:
        sys.exit("state_obs_bench: off and masked need --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["State observations (mv_set_state_obs): measured by scripts/state_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every form on a gym of its own.  Several agents per env, several GPUs: unmeasured.", ""]
    if args.what in ("off", "all"):
        bench_off(args, lines)
    if args.what in ("calls", "all"):
        bench_calls(args, lines)
    if args.what in ("plan", "all"):
        bench_plan(args, lines)
    if args.what in ("masked", "all"):
        bench_masked(args, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
