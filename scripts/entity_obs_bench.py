#!/usr/bin/env python
"""What entity observations cost (include/megaverse_hip.h: mv_set_entity_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each: bench.py's headline (agent observations/s).
           --parent DIR: the parent's checkout, built.  Every kernel such a gym launches is the parent's, so the expectation is "inside the parent's own
           min - max spread"; both lists are recorded and the report says plainly when it is outside.
  masked   what the change costs a gym that already runs the MASKED step kernels and attaches no buffer: an all-ones step mask, the parent commit against
           this one, --reps alternating runs each, the 16-tick call rendered and render='none' on TowerBuilding: us per tick, the same rule.
  calls    --envs x 1 agents at --size x --size, 16-tick MV_POLICY_SEQUENCE calls into rings with no buffer, entity rows, and scene rows: TowerBuilding rendered
           and render='none', ObstaclesHard rendered, HexMemory render='none' (the largest E), Sokoban render='none' (the goal compaction): us per tick, with
           the bytes a tick stages beside each figure.  Reported, not gated.

Every measurement is a process of its own under a time limit (--step-timeout seconds), one at a time; the first one that fails, is killed by a signal or
runs out of time ends the whole run, and nothing more is started on the device.  Not measured here: several agents per env, several GPUs.

JSON lines on stdout; the report goes to --out.
    python scripts/entity_obs_bench.py [--what off|masked|calls|all] [--parent DIR] [--out profiles/entity_obs_measured.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16
FORMS = (("buffer off", False, False), ("entity on", False, True), ("scene on", True, False))   # (name, scene rows, entity rows)
CASES = (("TowerBuilding", "every"), ("TowerBuilding", "none"), ("ObstaclesHard", "every"), ("HexMemory", "none"), ("Sokoban", "none"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v, fmt="{:.2f}"):
    return f"{fmt.format(median(v)):>10}  ({fmt.format(min(v))} - {fmt.format(max(v))})"


def run_json(cmd, cwd, key, limit):
    """one measurement: a child under a time limit; -> the JSON lines of its stdout that have `key`.  Anything but a clean exit ends the run."""
    try:
        out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"entity_obs_bench: {' '.join(cmd)} ran past its {limit} s: stopping, nothing more is started")
    found = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{") and f'"{key}"' in line]
    if out.returncode != 0 or not found:
        sys.exit(f"entity_obs_bench: {' '.join(cmd)} ended with status {out.returncode}: stopping, nothing more is started\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return found


def child(args, what, *extra):
    return [sys.executable, os.path.abspath(__file__), "--what", what, "--envs", str(args.envs), "--size", str(args.size), "--calls", str(args.calls),
            "--warmup", str(args.warmup), "--share-reps", str(args.share_reps)] + list(extra)


def verdict(parent, this, higher_is_better, unit):
    """the acceptance rule: this commit's median not worse than the parent's median by more than the parent's own max - min spread"""
    mp, mt, sp = median(parent), median(this), max(parent) - min(parent)
    worse = (mp - mt) if higher_is_better else (mt - mp)
    inside = min(parent) <= mt <= max(parent)
    return (f"this commit's median {mt:.3f} {unit} against the parent's {mp:.3f} {unit}: " + ("worse" if worse > 0 else "not worse") + f" by {abs(worse):.3f}, the parent's own "
            f"max - min spread is {sp:.3f}; the median is " + ("INSIDE" if inside else "OUTSIDE") + f" the parent's range {min(parent):.3f} - {max(parent):.3f}"
            + ("" if inside else " (" + ("better" if worse <= 0 else "WORSE") + ")"))


# ---- children: one process per measurement -------------------------------------------------------------------------------------------------------------------
def imports(tree):
    sys.path.insert(0, os.path.abspath(tree))
    os.environ.setdefault("BOXOBAN_LEVELS", os.path.join(ROOT, "tests", "golden", "boxoban"))   # (Sokoban: the tree's own Boxoban-format levels)
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    if not torch.cuda.is_available():
        sys.exit("entity_obs_bench: no GPU")
    return np, torch, MegaverseGym


def buffers(torch, np, N, S, obs=True):
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda") if obs else None, torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    return ring, script


def make_gym(MegaverseGym, scenario, N, S, ring, script, scene=False, entity=False):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    g.set_output_ring(K, ring[0].data_ptr() if ring[0] is not None else 0, ring[1].data_ptr(), ring[2].data_ptr())
    g.set_action_ring(K, script.data_ptr())
    if scene:   # (behind the ring: one entry per ring entry)
        g.set_scene_obs(True)
    if entity:
        g.set_entity_obs(True)
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


def child_call16(args):
    """one gym of --tree's library with an all-ones step mask and no buffer: us per tick of the 16-tick call with --render"""
    np, torch, MegaverseGym = imports(args.tree)
    ring, script = buffers(torch, np, args.envs, args.size, obs=args.render != "none")
    g = make_gym(MegaverseGym, "TowerBuilding", args.envs, args.size, ring, script)
    g.set_step_mask(np.ones(args.envs, bool))
    dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=args.render), args.calls, args.warmup)
    g.close()
    print(json.dumps({"what": "call16", "label": args.label, "render": args.render, "us_per_tick": round(dt / (args.calls * K) * 1e6, 3)}), flush=True)


def child_calls(args):
    """one scenario, one render mode: the three forms, --share-reps repetitions, the forms alternating within each, one gym alive at a time"""
    np, torch, MegaverseGym = imports(ROOT)
    from megaverse_amd import entity_rows
    ring, script = buffers(torch, np, args.envs, args.size, obs=args.render != "none")
    for rep in range(args.share_reps):
        for name, scene, entity in FORMS:
            g = make_gym(MegaverseGym, args.scenario, args.envs, args.size, ring, script, scene=scene, entity=entity)
            dt = timed(g, lambda: g.step_n(K, "sequence", 0, 0, render=args.render), args.calls, args.warmup)
            g.close()
            staged = args.envs * (entity_rows(args.scenario, 1) * 32 if entity else 128 if scene else 0)
            print(json.dumps({"what": "calls", "scenario": args.scenario, "render": args.render, "form": name, "rep": rep, "staged_bytes_per_tick": staged,
                              "us_per_tick": round(dt / (args.calls * K) * 1e6, 3)}), flush=True)


# ---- the report ------------------------------------------------------------------------------------------------------------------------------------------------
def bench_off(args, lines):
    trees = (("parent", os.path.abspath(args.parent)), ("this commit", ROOT))
    obs = {name: [] for name, _ in trees}
    for rep in range(args.reps):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):   # (alternating, and which build goes first alternates too)
            line = run_json([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                             "--no-cpu-baseline", "--no-extra-legs"], tree, "value", args.step_timeout)[-1]
            obs[name].append(line["value"] / 1e6)
            print(json.dumps({"what": "off", "label": name, "rep": rep, "bench_py_value": line["value"], "unit": line.get("unit")}), flush=True)
    lines.append(f"(a) Nothing attached: the parent commit against this one, {args.reps} alternating runs each (parent first in the even repetitions, this commit "
                 "first in the odd ones), every run a process of its own.")
    lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --no-cpu-baseline --no-extra-legs, M agent observations/s (higher is better):")
    for name, _ in trees:
        lines.append(f"  {name:<12} " + " ".join(f"{v:.3f}" for v in obs[name]) + f"   median {median(obs[name]):.3f}   range {min(obs[name]):.3f} - {max(obs[name]):.3f}")
    lines.append("  " + verdict(obs["parent"], obs["this commit"], True, "M obs/s"))
    lines.append("")


def bench_masked(args, lines):
    trees = (("parent", os.path.abspath(args.parent)), ("this commit", ROOT))
    us = {(name, render): [] for name, _ in trees for render in ("every", "none")}
    for rep in range(args.reps):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):
            for render in ("every", "none"):
                line = run_json(child(args, "call16", "--tree", tree, "--label", name, "--render", render), ROOT, "us_per_tick", args.step_timeout)[-1]
                print(json.dumps(dict(line, what="masked", rep=rep)), flush=True)
                us[(name, render)].append(line["us_per_tick"])
    lines.append(f"(b) The MASKED step kernels with NO buffer attached -- what the extra uniform branch costs users of masks and budgets: TowerBuilding {args.envs} x 1 at")
    lines.append(f"{args.size}x{args.size}, an all-ones step mask, {K}-tick MV_POLICY_SEQUENCE calls, the parent commit against this one, {args.reps} alternating runs each (a process of")
    lines.append("its own per run, the builds taking turns going first); us per tick (lower is better), every run, then median (min - max).")
    for render, title in (("every", "rendered"), ("none", "render='none'")):
        for name, _ in trees:
            lines.append(f"  {title + ', ' + name:<28}" + " ".join(f"{v:.2f}" for v in us[(name, render)]) + "  " + spread(us[(name, render)]))
        lines.append("  " + title + ": " + verdict(us[("parent", render)], us[("this commit", render)], False, "us"))
    lines.append("")


def bench_calls(args, lines):
    lines.append(f"(c) {args.envs} x 1 at {args.size}x{args.size}, {K}-tick MV_POLICY_SEQUENCE calls into rings, {args.calls} calls timed after {args.warmup}, {args.share_reps} "
                 "repetitions, the forms alternating within each, one gym alive at a time; us per tick, median (min - max), and the bytes one tick stages.  A buffer "
                 "on: the MASKED step kernels + ONE publication launch per call.  Reported, not gated.")
    for scenario, render in CASES:
        title = "rendered" if render == "every" else "render='none'"
        lines.append(f"{scenario}, {title}")
        found = run_json(child(args, "child_calls", "--scenario", scenario, "--render", render), ROOT, "us_per_tick", args.step_timeout)
        for line in found:
            print(json.dumps(line), flush=True)
        for name, _, _ in FORMS:
            mine = [x for x in found if x["form"] == name]
            lines.append(f"  {name:<14}{spread([x['us_per_tick'] for x in mine])}   staged {mine[0]['staged_bytes_per_tick']} B per tick")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["off", "masked", "calls", "all", "call16", "child_calls"], default="all")
    ap.add_argument("--parent", default="", help="the parent commit's checkout, built (off, masked)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=256, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5, help="off, masked: alternating runs of each build")
    ap.add_argument("--share-reps", type=int, default=3, help="calls: repetitions")
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds every measurement's process may take")
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    ap.add_argument("--tree", default=ROOT, help="call16: the checkout whose megaverse_amd is measured")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--render", default="none")
    ap.add_argument("--scenario", default="TowerBuilding")
    args = ap.parse_args()
    if args.what in ("call16", "child_calls"):
        return {"call16": child_call16, "child_calls": child_calls}[args.what](args)
    if args.what in ("off", "masked", "all") and not args.parent:
        sys.exit("entity_obs_bench: off and masked need --parent DIR (the parent commit's checkout, built)")
    import torch
    lines = ["Entity observations (mv_set_entity_obs): measured by scripts/entity_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Host clock around calls that end in a device synchronise; every measurement a process of its own, one gym alive at a time.  Several agents per env, "
             "several GPUs: unmeasured.", ""]
    if args.what in ("off", "all"):
        bench_off(args, lines)
    if args.what in ("masked", "all"):
        bench_masked(args, lines)
    if args.what in ("calls", "all"):
        bench_calls(args, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
