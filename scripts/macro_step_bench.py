#!/usr/bin/env python
"""What a macro step costs and buys (include/megaverse_hip.h: mv_macro_step).  Needs a GPU; reads nothing outside the tree.

  decision   per decision at k = 4 and k = 8, TowerBuilding and HexMemory, --envs x 1 agents at --size x --size, the actions in device memory, in three forms:
               macro        macro_step(k, actions, render='last')
               composition  what a caller composed before: set_episode_budget(1) re-attached, set_action_ring(1, actions), step_n(k, 'sequence',
                            render='last') into reward / done rings of k, a torch sum over the ring
               rendered     k x (set_actions_device + step): k rendered ticks, the wrapper loop without its break
             Every form runs on a gym of its own; the forms alternate, --reps repetitions each (a host clock around --calls decisions that end in a device
             synchronise, after --warmup decisions) -> us per decision, the spread of the repetitions, the ratios.  No threshold is set.
  masked     an all-ones step mask without macro steps, step_n(16) rendered, us per tick: what the MASKED kernels cost a gym that never makes a macro step.
             Run on the parent commit and on this one (the library of the tree the script is started in) and compare.

On a tree without macro steps the `macro` form is left out, so that the same script measures the parent.  Not measured here: several agents per env, several
GPUs.

JSON lines on stdout; the report is appended to --out (default profiles/macro_step_measured.txt) under --label.
    python scripts/macro_step_bench.py [--what decision|masked|all] [--label text]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


DECISION_FORMS, MASKED_FORMS = ("macro", "composition", "rendered"), ("plain", "all_ones_mask")


def make_gym(MegaverseGym, scenario, N, S):
    g = MegaverseGym(scenario, S, S, N, 1, 1, False, {})
    g.set_pixel_mode("fast")
    g.seed(42)
    g.reset()
    return g


def timed(g, call, calls, warmup):
    """seconds of `calls` back-to-back calls, the last one waited for"""
    import torch
    for _ in range(warmup):
        call()
    g.synchronize(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    g.synchronize(); torch.cuda.synchronize()
    return time.perf_counter() - t0


def decision_forms(torch, MegaverseGym, scenario, N, S, k, wanted):
    """the forms of `wanted`, in its order (the gyms are created in that order too: --forms lets a run show what the order does)"""
    from megaverse_amd.rollout import sample_actions
    acts = torch.as_tensor(sample_actions(3, 0, N).astype("int32").reshape(N, 6)).to("cuda:0")
    made = {}
    if "macro" in wanted and hasattr(MegaverseGym, "macro_step"):
        gm = make_gym(MegaverseGym, scenario, N, S)
        made["macro"] = (gm, lambda: gm.macro_step(k, acts, render="last"))
    rew = done = ones = None
    keep = []
    if "composition" in wanted:
        made["composition"], (rew, done, ones) = composition_form(torch, MegaverseGym, scenario, N, S, k, acts, keep)
    if "rendered" in wanted:
        gr = make_gym(MegaverseGym, scenario, N, S)

        def rendered():
            for _ in range(k):
                gr.set_actions_device(acts.data_ptr())
                gr.step()
        made["rendered"] = (gr, rendered)
    return {f: made[f] for f in wanted if f in made}, (acts, rew, done, ones, keep)


def composition_form(torch, MegaverseGym, scenario, N, S, k, acts, keep):
    gc = make_gym(MegaverseGym, scenario, N, S)
    rew = torch.zeros((k, N), dtype=torch.float32, device="cuda:0")
    done = torch.zeros((k, N), dtype=torch.uint8, device="cuda:0")
    gc.set_output_ring(k, 0, rew.data_ptr(), done.data_ptr())
    gc.set_action_ring(1, acts.data_ptr())
    ones = torch.ones(N, dtype=torch.int32, device="cuda:0")

    def composition():
        gc.set_episode_budget(ones)
        gc.step_n(k, "sequence", 0, 0, render="last")
        keep[:] = [rew.sum(dim=0), done.amax(dim=0)]
    return (gc, composition), (rew, done, ones)


def run_decision(args, torch, MegaverseGym, emit):
    for scenario in args.scenarios:
        for k in (4, 8):
            forms, held = decision_forms(torch, MegaverseGym, scenario, args.envs, args.size, k, [f for f in args.forms if f in DECISION_FORMS])
            us = {f: [] for f in forms}
            for _ in range(args.reps):
                for f, (g, call) in forms.items():
                    us[f].append(timed(g, call, args.calls, args.warmup) / args.calls * 1e6)
            rec = {"what": "decision", "scenario": scenario, "k": k, "envs": args.envs, "size": args.size,
                   "us_per_decision": {f: {"median": statistics.median(v), "min": min(v), "max": max(v)} for f, v in us.items()}}
            med = {f: statistics.median(v) for f, v in us.items()}
            if "macro" in med and "composition" in med and "rendered" in med:
                rec["composition_over_macro"] = med["composition"] / med["macro"]
                rec["rendered_over_macro"] = med["rendered"] / med["macro"]
            emit(rec)
            for g, _ in forms.values():
                g.close()
            del held


def run_masked(args, torch, MegaverseGym, emit):
    K = 16
    for scenario in args.scenarios:
        N, S = args.envs, args.size
        gyms = {}
        for form in [f for f in args.forms if f in MASKED_FORMS]:
            g = make_gym(MegaverseGym, scenario, N, S)
            obs = torch.zeros((K, N, S, S, 4), dtype=torch.uint8, device="cuda:0")
            rew = torch.zeros((K, N), dtype=torch.float32, device="cuda:0")
            done = torch.zeros((K, N), dtype=torch.uint8, device="cuda:0")
            g.set_output_ring(K, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
            mask = torch.ones(N, dtype=torch.bool, device="cuda:0")
            if form == "all_ones_mask":
                g.set_step_mask(mask)
            gyms[form] = (g, (obs, rew, done, mask))
        us = {f: [] for f in gyms}
        step = [0]

        def call_of(g):
            def call():
                g.step_n(K, "multidiscrete", 7, step[0])
                step[0] += K
            return call
        for _ in range(args.reps):
            for f, (g, _) in gyms.items():
                us[f].append(timed(g, call_of(g), args.calls, args.warmup) / (args.calls * K) * 1e6)
        emit({"what": "masked", "scenario": scenario, "envs": N, "size": S, "ticks_per_call": K,
              "us_per_tick": {f: {"median": statistics.median(v), "min": min(v), "max": max(v)} for f, v in us.items()}})
        for g, _ in gyms.values():
            g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("decision", "masked", "all"))
    ap.add_argument("--scenarios", nargs="+", default=["TowerBuilding", "HexMemory"])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forms", nargs="+", default=list(DECISION_FORMS + MASKED_FORMS), choices=DECISION_FORMS + MASKED_FORMS,
                    help="the forms to measure, in the order their gyms are created")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "macro_step_measured.txt"))
    args = ap.parse_args()
    import torch
    from megaverse_amd.extension import MegaverseGym
    lines = []

    def emit(rec):
        rec["label"] = args.label
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    if args.what in ("decision", "all"):
        run_decision(args, torch, MegaverseGym, emit)
    if args.what in ("masked", "all"):
        run_masked(args, torch, MegaverseGym, emit)
    with open(args.out, "a") as f:
        f.write(f"\n== {args.label}: scripts/macro_step_bench.py --what {args.what} --forms {' '.join(args.forms)} --envs {args.envs} --size {args.size} --reps {args.reps} "
                f"--calls {args.calls} (median [min .. max] over the repetitions)\n")
        for rec in lines:
            if rec["what"] == "decision":
                cells = "   ".join(f"{n} {v['median']:.1f} [{v['min']:.1f} .. {v['max']:.1f}]" for n, v in rec["us_per_decision"].items())
                ratios = "" if "composition_over_macro" not in rec else \
                    f"   composition / macro {rec['composition_over_macro']:.2f}   rendered / macro {rec['rendered_over_macro']:.2f}"
                f.write(f"decision  {rec['scenario']:<14} k = {rec['k']}  us per decision: {cells}{ratios}\n")
            else:
                cells = "   ".join(f"{n} {v['median']:.2f} [{v['min']:.2f} .. {v['max']:.2f}]" for n, v in rec["us_per_tick"].items())
                f.write(f"masked    {rec['scenario']:<14} step_n(16) rendered, us per tick: {cells}\n")


if __name__ == "__main__":
    main()
