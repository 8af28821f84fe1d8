#!/usr/bin/env python
"""What normal observations cost (include/megaverse_hip.h: mv_set_normal_obs).  Needs a GPU; reads nothing outside the tree and the --parent checkout.

  off      a gym that attaches nothing, the parent commit against this one, --reps alternating runs each (every run a process of its own): bench.py's
           headline (agent observations/s).  --parent DIR: the parent's checkout, built.  The report gives both ranges and says whether this commit's median
           lies inside the parent's own run-to-run spread.
  calls    TowerBuilding and HexMemory, --envs x 1 agents at --size x --size, 16-tick MV_POLICY_SEQUENCE calls into rings of 16: us per tick for
           fast; fast + normals (F16, SNORM8); fast + depth + labels (float32, U16); fast + depth + labels + normals (F16); exact; exact + normals;
           exact + all three.  The structural claim: the three-plane follower costs ONE trace -- its time beyond the fast call's must be less than the
           depth + labels follower's plus the normals-only follower's of the same run.

Not measured here: several agents per env, several GPUs.

JSON lines on stdout; the report goes to --out.
    python scripts/normal_obs_bench.py [--what off|calls|all] [--parent DIR] [--out profiles/normal_obs_measured.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(v, fmt="{:.2f}"):
    return f"{fmt.format(median(v)):>10}  ({fmt.format(min(v))} - {fmt.format(max(v))})"


def run_json(cmd, cwd, key):
    """the last JSON line of a child's stdout that has `key`"""
    out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and f'"{key}"' in line:
            return json.loads(line)
    sys.exit(f"normal_obs_bench: {' '.join(cmd)} printed no result\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")


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


# (name, pixel mode, depth + labels attached, the normals' dtype or None)
FORMS = (("fast", "fast", False, None), ("fast + normals F16", "fast", False, "float16"), ("fast + normals SNORM8", "fast", False, "int8"),
         ("fast + depth + labels", "fast", True, None), ("fast + depth + labels + normals", "fast", True, "float16"),
         ("exact", "exact", False, None), ("exact + normals", "exact", False, "float16"), ("exact + all three", "exact", True, "float16"))


def bench_calls(args, lines):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from megaverse_amd.extension import MegaverseGym
    N, S = args.envs, args.size
    ring = (torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda"), torch.zeros((K, N), dtype=torch.float32, device="cuda"),
            torch.zeros((K, N), dtype=torch.uint8, device="cuda"))
    script = torch.as_tensor((np.random.default_rng(7).integers(0, 1 << 30, (K, N, 6)) % np.array([3, 3, 3, 2, 2, 3])).astype(np.int32)).to("cuda")
    depth = torch.zeros((K, N, S, S), dtype=torch.float32, device="cuda")
    labels = torch.zeros((K, N, S, S), dtype=torch.int16, device="cuda")
    normals = {"float16": torch.zeros((K, N, S, S, 4), dtype=torch.float16, device="cuda"), "int8": torch.zeros((K, N, S, S, 4), dtype=torch.int8, device="cuda")}
    torch.cuda.synchronize()
    lines.append(f"(b) {N} x 1 at {S}x{S}, {K}-tick MV_POLICY_SEQUENCE calls into rings of {K}, {args.calls} calls timed after {args.warmup} (exact mode: a quarter of "
                 f"both), {args.share_reps} repetitions, the forms alternating within each; us per tick, median (min - max).  Host clock around calls that end in a "
                 "device synchronise.  depth: float32; labels: U16; normals: F16 unless named.")
    lines.append("fast + anything: the fast passes as they are, then ONE launch per tick on the same stream for whatever is attached; exact + anything: the pass "
                 "stores every output itself.")
    for scenario in ("TowerBuilding", "HexMemory"):
        us = {f[0]: [] for f in FORMS}
        launches = {}
        for rep in range(args.share_reps):
            for name, mode, both, ndtype in FORMS:
                g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
                g.set_pixel_mode(mode); g.seed(42); g.reset()
                g.set_output_ring(K, ring[0].data_ptr(), ring[1].data_ptr(), ring[2].data_ptr())
                g.set_action_ring(K, script.data_ptr())
                if both:
                    g.set_depth_obs(depth)
                    g.set_seg_obs(labels, "instance")
                if ndtype:
                    g.set_normal_obs(normals[ndtype])
                calls, warm = (args.calls, args.warmup) if mode == "fast" else (max(1, args.calls // 4), max(1, args.warmup // 4))
                for _ in range(warm):
                    g.step_n(K, "sequence", 0, 0)
                g.synchronize()
                c0 = g.debug_launch_counts()
                t0 = time.perf_counter()
                for _ in range(calls):
                    g.step_n(K, "sequence", 0, 0)
                g.synchronize()
                dt = time.perf_counter() - t0
                c1 = g.debug_launch_counts()
                g.close()
                us[name].append(dt / (calls * K) * 1e6)
                launches[name] = (c1[1] - c0[1]) / (calls * K)
                print(json.dumps({"what": "calls", "scenario": scenario, "envs": N, "size": S, "form": name, "rep": rep, "ticks": calls * K,
                                  "seconds": round(dt, 4), "us_per_tick": round(us[name][-1], 2), "pass_side_launches_per_tick": round(launches[name], 4)}), flush=True)
        lines.append(f"{scenario}")
        for name, _, _, _ in FORMS:
            lines.append(f"  {name:<34}{spread(us[name])}    pass-side launches per tick {launches[name]:.3f}")
        off, n16, dl, all3 = (median(us[n]) for n in ("fast", "fast + normals F16", "fast + depth + labels", "fast + depth + labels + normals"))
        holds = all3 - off < (dl - off) + (n16 - off)
        lines.append(f"  one trace: the three-plane follower takes {all3 - off:.2f} us per tick beyond the fast call, the depth + labels follower {dl - off:.2f} and the "
                     f"normals-only follower {n16 - off:.2f} (together {(dl - off) + (n16 - off):.2f}): the relation three planes < depth + labels + normals-only "
                     + ("HOLDS" if holds else "FAILS") + f".  Launches per tick beyond the fast call's: normals {launches['fast + normals F16'] - launches['fast']:.3f}, "
                     f"all three {launches['fast + depth + labels + normals'] - launches['fast']:.3f}.")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["off", "calls", "all"], default="all")
    ap.add_argument("--parent", default="", help="the parent commit's checkout, built (off)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=128, help="timed 16-tick calls per repetition")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5, help="off: alternating runs of each build")
    ap.add_argument("--share-reps", type=int, default=3, help="calls: repetitions")
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    ap.add_argument("--out", default="", help="write the report here (default: stdout only)")
    args = ap.parse_args()
    if args.what in ("off", "all") and not args.parent:
        sys.exit("normal_obs_bench: off needs --parent DIR (the parent commit's checkout, built)")
    import torch
    if not torch.cuda.is_available():
        sys.exit("normal_obs_bench: no GPU")
    lines = ["Normal observations (mv_set_normal_obs): measured by scripts/normal_obs_bench.py on " + torch.cuda.get_device_name(0) + " ("
             + torch.cuda.get_device_properties(0).gcnArchName + ").",
             "Every form on a gym of its own.  A normal is one 8-byte (F16) or 4-byte (SNORM8) store per lane and pixel.",
             "Unmeasured: several agents per env, several GPUs.", ""]
    if args.what in ("off", "all"):
        bench_off(args, lines)
    if args.what in ("calls", "all"):
        bench_calls(args, lines)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
