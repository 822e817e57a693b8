"""Throughput of the homography refinement (sfh_amd.refine, csrc/refine.hip), batch 16, logits 640x360, on one GPU.

    python profiles/refine_throughput.py             # alternating timings -> profiles/refine_throughput.jsonl
    python profiles/refine_throughput.py --trace     # steady-state calls only, for a kernel trace

(a) the refiner alone, default schedule (levels 4, 2, 1, five steps each), templates 640x360 and 1280x720: ms per call on the
    host clock, each figure ending in a synchronise; the two templates alternate inside every repetition, every repetition is
    reported.  Launches per call are counted by wrapping the library's entries; bytes per full-resolution pass are the
    algorithmic ones: evidence planes once, theta, the template planes once (they stay cache-resident), the partial sums.
(b) predict() of a full-size model (random weights, batch 16, 640x360) with and without the refiner, alternating.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, H = 16, 640, 360
TEMPLATES = ("ncaa_nc4_640x360", "ncaa_nc4_1280x720")


def _host_ms(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _count_launches(lib, fn):
    """calls of the sfh_refine_* entries that launch, during fn()"""
    names = ("sfh_refine_template_planes", "sfh_refine_evidence_planes", "sfh_refine_accumulate", "sfh_refine_step")
    counts, saved = {n: 0 for n in names}, {n: getattr(lib, n) for n in names}

    def wrap(n):
        def call(*a):
            counts[n] += 1
            return saved[n](*a)
        return call
    try:
        for n in names:
            setattr(lib, n, wrap(n))
        fn()
    finally:
        for n in names:
            setattr(lib, n, saved[n])
    return counts


def measure(args):
    import numpy as np
    import torch
    from sfh_amd import _lib, synth
    from sfh_amd.reconstructor import Reconstructor
    from sfh_amd.refine import ThetaRefiner
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    lib = _lib.load()
    g = np.random.default_rng(7)
    theta = torch.from_numpy(np.stack([synth.REALISTIC_THETAS[k % 2] for k in range(B)]).astype(np.float32)).cuda().view(B, 1, 3, 3)
    logits = torch.from_numpy(g.normal(0, 3, (B, 4, H, W)).astype(np.float32)).cuda()
    refiners = {name: ThetaRefiner(synth.load_court_template(name, 4, 1).cuda(), 4, (W, H)) for name in TEMPLATES}
    rows = []
    for name, r in refiners.items():
        r(theta, logits)                                        # planes, workspaces
        c = _count_launches(lib, lambda: r(theta, logits))
        ht, wt = r.court_img.shape[2:]
        full = B * H * W * 16 + ht * wt * 16 + 36 * B + lib.sfh_refine_workspace_bytes(B, H, W)
        rows.append({"what": "launches", "template": name, "per_call": c, "total": sum(c.values()),
                     "bytes_per_full_resolution_pass": int(full)})
    if args.trace:
        for _ in range(args.iters):
            for r in refiners.values():
                r(theta, logits)
        torch.cuda.synchronize()
        return
    for rep in range(args.reps):                                # alternating, so drift hits both alike
        row = {"what": "refiner", "batch": B, "logits": f"{W}x{H}", "rep": rep, "iters": args.iters}
        for name, r in refiners.items():
            row[f"ms_per_call_{name}"] = round(_host_ms(torch, lambda: r(theta, logits), 3, args.iters), 4)
        rows.append(row)
    court = synth.load_court_template(TEMPLATES[0], 4, B).cuda()
    net = Reconstructor(court, synth.load_court_poi("pitch", B).cuda(), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.cuda().eval()
    x = synth.smooth_frames(B, H, W, seed=19).cuda()
    refiner = ThetaRefiner(court, 4, net.warp_size)
    with torch.no_grad():
        for rep in range(args.reps):
            row = {"what": "predict", "batch": B, "frame": f"{W}x{H}", "rep": rep, "iters": args.predict_iters}
            for key, rf in (("ms_plain", None), ("ms_refined", refiner)):
                net.refiner = rf
                row[key] = round(_host_ms(torch, lambda: net.predict(x, consistency=True), 2, args.predict_iters), 3)
            row["refined_minus_plain_ms"] = round(row["ms_refined"] - row["ms_plain"], 3)
            rows.append(row)
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--predict-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_throughput.jsonl"))
    measure(ap.parse_args())
