"""What the deterministic training mode costs: ms per TrainStep.step on one MI355X at 640x360, batch 16, f16x3.

    python profiles/train_deterministic.py [--parent-tree DIR] [--reps 3] [--steps 5] [--out profiles/train_deterministic.jsonl]

Legs, run alternately `reps` times, each in a child process of its own (a fresh model, two warm-up steps, then the host
clock around `steps` steps, ending in a device synchronise):
  parent         the parent commit's library and package: DIR is a checkout of that commit with its library built
                 (git worktree add DIR HEAD~1 && python DIR/__graft_entry__.py); skipped without --parent-tree
  parent_deterministic  the same tree, TrainStep(deterministic=True): the parent beside the deterministic leg as well
  default        this commit, TrainStep(deterministic=False)
  two_pass       this commit, default mode with Options(train_one_pass=False): the plain legs the deterministic mode takes,
                 still on atomics - the part of the cost that is the lost fusions
  deterministic  this commit, TrainStep(deterministic=True); det_workspace_bytes is recorded
One JSON line per (repetition, leg) is written to --out (replacing an earlier record); the last line is the summary (medians, ratios).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("parent", "parent_deterministic", "default", "two_pass", "deterministic")
B, H, W = 16, 360, 640


def child(leg, tree, steps):
    sys.path.insert(0, tree)
    import dataclasses

    import torch
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    from sfh_amd.training import TrainStep
    dev = torch.device("cuda", 0)
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B).to(dev)
    poi = synth.load_court_poi("pitch", B).to(dev)
    net = Reconstructor(court, poi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.to(dev).train()
    if leg == "two_pass":
        net.options = dataclasses.replace(net.options, train_one_pass=False)
    ts = TrainStep(net, **({"deterministic": True} if leg.endswith("deterministic") else {}))
    g = torch.Generator().manual_seed(7)
    npoi = poi.shape[1]
    batch = {"mask": torch.randint(0, 4, (B, H, W), generator=g).to(dev), "weight": torch.ones(B, device=dev),
             "poi": torch.rand((B, npoi, 2), generator=g).to(dev), "nonzeros": torch.ones((B, npoi), device=dev),
             "num_nonzero": torch.full((B,), float(npoi), device=dev)}
    x = synth.smooth_frames(B, H, W, seed=3).to(dev)
    for _ in range(2):
        ts.step(x, batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(x, batch)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print("RESULT " + json.dumps({"leg": leg, "ms_per_step": round(ms, 3), "steps": steps, "batch": B, "frame": [W, H],
                                  "precision": os.environ["SFH_TRAIN_PRECISION"], "range_fallbacks": ts.range_fallbacks,
                                  "det_workspace_bytes": getattr(ts, "det_workspace_bytes", 0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_deterministic.jsonl"))
    ap.add_argument("--child")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tree, a.steps)
    env = dict(os.environ, SFH_TRAIN_PRECISION="f16x3")
    env.pop("SFH_AMD_LIB", None)
    legs = [leg for leg in LEGS if not leg.startswith("parent") or a.parent_tree]
    rows = []
    with open(a.out, "w") as out:    # one run, one record: an earlier file is replaced
        for rep in range(a.reps):
            for leg in legs:
                tree = os.path.abspath(a.parent_tree) if leg.startswith("parent") else ROOT
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--tree", tree, "--steps", str(a.steps)],
                                   env=env, cwd=tree, capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.exit(f"leg {leg} failed ({r.returncode}): nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                row = dict(json.loads(line[0][7:]), rep=rep)
                rows.append(row)
                out.write(json.dumps(row) + "\n")
                out.flush()
                print(row, flush=True)
        med = {leg: statistics.median(r["ms_per_step"] for r in rows if r["leg"] == leg) for leg in legs}
        summary = {"summary": True, "median_ms_per_step": med,
                   "det_workspace_bytes": max(r["det_workspace_bytes"] for r in rows),
                   "deterministic_over_default": round(med["deterministic"] / med["default"], 3),
                   "two_pass_over_default": round(med["two_pass"] / med["default"], 3)}
        # "no slower": per mode, this commit's median minus the parent's, beside the spread of the parent's own repetitions
        for ours, theirs in (("default", "parent"), ("deterministic", "parent_deterministic")):
            if theirs in med:
                par = [r["ms_per_step"] for r in rows if r["leg"] == theirs]
                summary[f"{theirs}_spread_ms"] = round(max(par) - min(par), 3)
                summary[f"{ours}_minus_{theirs}_median_ms"] = round(med[ours] - med[theirs], 3)
                summary[f"{ours}_minus_{theirs}_ms_per_rep"] = [
                    round(d["ms_per_step"] - p, 3) for d, p in zip((r for r in rows if r["leg"] == ours), par)]
        out.write(json.dumps(summary) + "\n")
        print(summary)


if __name__ == "__main__":
    main()
