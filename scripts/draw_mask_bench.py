#!/usr/bin/env python
"""What draw masks cost and buy (include/megaverse_hip.h: mv_set_draw_mask).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  nomask   a gym without a mask, the parent commit against this one, --reps alternating runs each (every run a process of its own): bench.py's headline
           (agent observations/s) and the 16-tick render='none' MV_POLICY_SEQUENCE call on TowerBuilding (us per tick).  --parent DIR: the parent's checkout,
           built.  Condition: this commit's median must not fall below the parent's lowest run (bench.py), nor rise above its highest (us per tick).
  shares   TowerBuilding and HexMemory, --envs x 1 agents at --size x --size, 16-tick sequence calls into rings, us per tick: unmasked, 100 % (an all-ones
           mask), 50 % (every even env), 6.25 % (the first envs / 16) and 0 % of the envs drawn, and render='none'; with --parent, the parent's rendered and
           'none' figures from the same session.
  plan     the savepoint planner of scripts/step_mask_bench.py -- env 0 frozen as the root; per iteration a fork of every other env from env 0 and 16
           RENDERED ticks into the ring -- with every env drawn and with only 64 leaves drawn: us per iteration.

Not measured here: several agents per env, several GPUs.

JSON lines on stdout; the report goes to --out.
    python scripts/draw_mask_bench.py [--what nomask|shares|plan|all] [--parent DIR] [--out profiles/draw_mask_measured.txt]
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


def spread(v, fmt="{:.2f}"):
    return f"{fmt.format(median(v)):>10}  ({fmt.format(min(v))} - {fmt.format(max(v))})"


def imports(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("draw_mask_bench: no GPU")
    return np, torch, MegaverseGym


def child_call16(args):
    """(a process of its own, --what call16 --tree DIR) one gym of the tree's library: us per tick of the 16-tick call with --render, no mask attached"""
    np, torch, MegaverseGym = imports(args.tree)
    ring, script = buffers(torch, np, args.envs, args.size, obs=args.render != "none")
    g = make_gym(MegaverseGym, args.scenario, args.envs, args.size, ring, script)
    dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=args.render), args.calls, args.warmup)
    g.close()
    print(json.dumps({"what": "call16", "label": args.label, "scenario": args.scenario, "envs": args.envs, "size": args.size, "render": args.render,
                      "ticks": args.calls * K, "seconds": round(dt, 4), "us_per_tick": round(dt / (args.calls * K) * 1e6, 3)}), flush=True)


def run_json(cmd, cwd, key):
    """the last JSON line of a child's stdout that has `key`"""
    out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and f'"{key}"' in line:
            return json.loads(line)
    sys.exit(f"draw_mask_bench: {' '.join(cmd)} printed no result\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")


def call16_of(args, tree, label, scenario, render):
    me = os.path.abspath(__file__)
    cmd = [sys.executable, me, "--what", "call16", "--tree", tree, "--label", label, "--scenario", scenario, "--render", render, "--envs", str(args.envs),
           "--size", str(args.size), "--calls", str(args.calls), "--warmup", str(args.warmup)]
    line = run_json(cmd, ROOT, "us_per_tick")
    print(json.dumps(line), flush=True)
    return line["us_per_tick"]


def bench_nomask(args, lines):
    trees = (("parent", os.path.abspath(args.parent)), ("this commit", ROOT))
    obs = {name: [] for name, _ in trees}
    none = {name: [] for name, _ in trees}
    for rep in range(args.reps):
        for name, tree in trees:   # (alternating)
            line = run_json([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                             "--no-cpu-baseline", "--no-extra-legs"], tree, "value")
            obs[name].append(line["value"])
            print(json.dumps({"what": "nomask", "label": name, "rep": rep, "bench_py_value": line["value"], "unit": line.get("unit")}), flush=True)
            none[name].append(call16_of(args, tree, name, "TowerBuilding", "none"))
    lines.append(f"1. No mask attached: the parent commit against this one, {args.reps} alternating runs each, every run a process of its own.")
    lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-extra-legs, agent observations/s (higher is better):")
    for name, _ in trees:
        lines.append(f"  {name:<12} " + " ".join(f"{v / 1e6:.3f}M" for v in obs[name]) + f"   median {median(obs[name]) / 1e6:.3f}M")
    ok = median(obs["this commit"]) >= min(obs["parent"])
    lines.append(f"  condition (this commit's median {median(obs['this commit']) / 1e6:.3f}M >= the parent's lowest run {min(obs['parent']) / 1e6:.3f}M): "
                 + ("MET" if ok else "NOT MET"))
    lines.append(f"TowerBuilding {args.envs} x 1 at {args.size}x{args.size}, {K}-tick render='none' sequence calls, us per tick (lower is better):")
    for name, _ in trees:
        lines.append(f"  {name:<12} " + " ".join(f"{v:.3f}" for v in none[name]) + f"   median {median(none[name]):.3f}")
    ok = median(none["this commit"]) <= max(none["parent"])
    lines.append(f"  condition (this commit's median {median(none['this commit']):.3f} <= the parent's highest run {max(none['parent']):.3f}): " + ("MET" if ok else "NOT MET"))
    lines.append("")


def bench_shares(args, lines):
    np, torch, MegaverseGym = imports(ROOT)
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    few = np.arange(N) < max(1, N // 16)
    shares = (("unmasked", "every", None), ("100 % drawn (all ones)", "every", np.ones(N, bool)), ("50 % drawn", "every", np.arange(N) % 2 == 0),
              (f"6.25 % drawn ({int(few.sum())} envs)", "every", few), ("0 % drawn", "every", np.zeros(N, bool)), ("render='none'", "none", None))
    lines.append(f"2. What the mask buys: {N} x 1 at {S}x{S}, {K}-tick MV_POLICY_SEQUENCE calls into rings, {args.calls} calls timed after {args.warmup}, "
                 f"{args.share_reps} repetitions, the forms alternating within each; us per tick, median (min - max).")
    for scenario in ("TowerBuilding", "HexMemory"):
        us = {name: [] for name, _, _ in shares}
        base = {"parent, rendered": [], "parent, render='none'": []}
        for rep in range(args.share_reps):
            for name, render, mask in shares:
                g = make_gym(MegaverseGym, scenario, N, S, ring, script)
                if mask is not None:
                    g.set_draw_mask(mask)
                dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=render), args.calls, args.warmup)
                g.close()
                us[name].append(dt / (args.calls * K) * 1e6)
                print(json.dumps({"what": "shares", "scenario": scenario, "envs": N, "size": S, "share": name, "rep": rep, "ticks": args.calls * K,
                                  "seconds": round(dt, 4), "us_per_tick": round(us[name][-1], 2)}), flush=True)
            if args.parent:
                base["parent, rendered"].append(call16_of(args, os.path.abspath(args.parent), "parent", scenario, "every"))
                base["parent, render='none'"].append(call16_of(args, os.path.abspath(args.parent), "parent", scenario, "none"))
        lines.append(f"{scenario}")
        for name, _, _ in shares:
            lines.append(f"  {name:<28}{spread(us[name])}")
        for name, v in base.items():
            if v:
                lines.append(f"  {name:<28}{spread(v)}   (a process of its own per run)")
    lines.append("")


def bench_plan(args, lines):
    np, torch, MegaverseGym = imports(ROOT)
    N, S = args.envs, args.size
    ring, script = buffers(torch, np, N, S)
    root_map = torch.as_tensor(np.asarray([-1] + [0] * (N - 1), np.int32)).to("cuda")
    leaves = np.zeros(N, bool)
    leaves[1:65] = True
    torch.cuda.synchronize()
    us = {"every env drawn": [], "64 leaves drawn": []}
    for rep in range(args.share_reps):
        for how in us:
            g = make_gym(MegaverseGym, "TowerBuilding", N, S, ring, script)
            g.set_step_mask(np.arange(N) != 0)
            if how == "64 leaves drawn":
                g.set_draw_mask(leaves)

            def iteration():
                g.fork_envs(root_map)
                g.step_n(K, "sequence", 0, 0, render="every")

            dt = timed(g, iteration, args.plan_iterations, args.warmup)
            g.close()
            us[how].append(dt / args.plan_iterations * 1e6)
            print(json.dumps({"what": "plan", "how": how, "envs": N, "size": S, "rep": rep, "iterations": args.plan_iterations, "seconds": round(dt, 4),
                              "us_per_iteration": round(us[how][-1], 1)}), flush=True)
    lines.append(f"3. The savepoint planner, TowerBuilding {N} x 1 at {S}x{S}: env 0 frozen as the root; per iteration a fork of every other env from env 0 (device")
    lines.append(f"map) and a {K}-tick RENDERED sequence call into the ring; {args.plan_iterations} iterations timed after {args.warmup}, {args.share_reps} repetitions; us per "
                 "iteration, median (min - max).")
    for how, v in us.items():
        lines.append(f"  {how:<18}{spread(v, '{:.1f}')}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["nomask", "shares", "plan", "all", "call16"], default="all")
    ap.add_argument("--parent", default="", help="the parent commit's checkout, built (nomask; the parent's figures of shares)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=256, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5, help="nomask: alternating runs of each build")
    ap.add_argument("--share-reps", type=int, default=3, help="shares, plan: repetitions")
    ap.add_argument("--plan-iterations", type=int, default=256)
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    ap.add_argument("--tree", default=ROOT, help="call16: the checkout whose megaverse_amd is measured")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--scenario", default="TowerBuilding")
    ap.add_argument("--render", default="none")
    args = ap.parse_args()
    if args.what == "call16":
        return child_call16(args)
    if args.what in ("nomask", "all") and not args.parent:
        sys.exit("draw_mask_bench: nomask needs --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["Draw masks (mv_set_draw_mask): measured by scripts/draw_mask_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every form on a gym of its own.  Several agents per env, several GPUs: unmeasured.", ""]
    if args.what in ("nomask", "all"):
        bench_nomask(args, lines)
    if args.what in ("shares", "all"):
        bench_shares(args, lines)
    if args.what in ("plan", "all"):
        bench_plan(args, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
