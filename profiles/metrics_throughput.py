"""Throughput of the registration-metric kernels (sfh_amd.metrics, csrc/metrics.hip) on one GPU.

    python profiles/metrics_throughput.py             # alternating timings -> profiles/metrics_throughput.jsonl
    python profiles/metrics_throughput.py --trace     # steady-state calls only, for a kernel trace in a run of its own

(a) sfh_metrics_confusion, kind 2 (logits), batch 16, 640x360, nc = 4 against sfh_mask_format_fwd (kind 2, gray) on the SAME
    logits: the existing kernel with the same dominant read.  Algorithmic bytes: 59.0 MB of logits + 29.5 MB of int64 mask
    against 59.0 MB + 3.7 MB of uint8 output, a ratio of 1.41.  The two alternate inside every repetition, every repetition is
    reported; each figure is on the host clock and ends in a synchronise.  The logits carry a court-like class layout (large
    uniform regions), which is what the per-wave key aggregation meets in practice; a second pair of rows uses i.i.d. noise
    logits and an i.i.d. mask, the worst case for the distinct-key loop (up to nc^2 keys in every wave).
(b) sfh_metrics_region on a 1280x720 raster, both modes (mode 1 with the default margin: a 2560x1440 canvas), batch 16, and
    sfh_metrics_points (33 court points, a 16x9 lattice), batch 16.  No target.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, H, NC = 16, 640, 360, 4


def _host_ms(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def measure(args):
    import numpy as np
    import torch
    from sfh_amd import _lib, metrics, synth
    from sfh_amd.ops import _ptr, _stream
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    lib = _lib.load()
    g = np.random.default_rng(11)
    ids = (synth.load_court_template("ncaa_nc4_640x360", NC, 1)[0, 0].numpy() * NC).round().astype(np.int64)
    court_logits = g.normal(0, 1, (B, NC, H, W)).astype(np.float32)
    np.put_along_axis(court_logits, np.broadcast_to(ids, (B, H, W))[:, None], 6.0, axis=1)
    inputs = {"court": (torch.from_numpy(court_logits).cuda(), torch.from_numpy(np.broadcast_to(ids, (B, H, W)).copy()).cuda()),
              "noise": (torch.from_numpy(g.normal(0, 3, (B, NC, H, W)).astype(np.float32)).cuda(),
                        torch.from_numpy(g.integers(0, NC, (B, H, W))).cuda())}
    out = torch.empty((B, NC, NC), dtype=torch.int64, device="cuda")
    gray = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    flag = metrics.new_flag("cuda")
    st = _stream()

    def confusion(lg, gt):
        _lib.check(lib.sfh_metrics_confusion(_ptr(lg), 2, _ptr(gt), NC, B, H, W, _ptr(out), _ptr(flag), st), "confusion")

    def mask_format(lg):
        _lib.check(lib.sfh_mask_format_fwd(_ptr(lg), 2, NC, B, H, W, H, W, 0, None, _ptr(gray), st), "mask_format")

    theta_p = torch.from_numpy(np.stack([synth.REALISTIC_THETAS[k % 2] for k in range(B)]).astype(np.float32)).cuda().view(B, 3, 3)
    theta_g = (theta_p * (1 + 0.01 * torch.randn(B, 3, 3, device="cuda"))).contiguous()
    pts = synth.load_court_poi("pitch", 1)[0].double().cuda().contiguous()
    calls = {"region_part_1280x720": lambda: metrics.region_counts(theta_p, theta_g, "part", (1280, 720)),
             "region_whole_1280x720_margin_half": lambda: metrics.region_counts(theta_p, theta_g, "whole", (1280, 720)),
             "points_33_lattice_16x9": lambda: metrics.point_errors(theta_p, theta_g, pts, (W, H))}
    if args.trace:
        for _ in range(args.iters):
            for lg, gt in inputs.values():
                confusion(lg, gt)
                mask_format(lg)
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        return
    rows = []
    for rep in range(args.reps):                                # alternating, so drift hits both alike
        for name, (lg, gt) in inputs.items():
            row = {"what": "confusion_vs_mask_format", "input": name, "batch": B, "frame": f"{W}x{H}", "nc": NC, "rep": rep,
                   "iters": args.iters}
            row["ms_confusion"] = round(_host_ms(torch, lambda: confusion(lg, gt), 5, args.iters), 4)
            row["ms_mask_format"] = round(_host_ms(torch, lambda: mask_format(lg), 5, args.iters), 4)
            row["time_ratio"] = round(row["ms_confusion"] / row["ms_mask_format"], 3)
            row["byte_ratio"] = round((B * H * W * (4 * NC + 8)) / (B * H * W * (4 * NC + 1)), 3)
            row["confusion_gb_per_s"] = round(B * H * W * (4 * NC + 8) / row["ms_confusion"] / 1e6, 1)
            rows.append(row)
        row = {"what": "region_and_points", "batch": B, "rep": rep, "iters": args.iters}
        for name, fn in calls.items():
            row["ms_" + name] = round(_host_ms(torch, fn, 3, args.iters), 4)
        rows.append(row)
    assert flag.item() == 0
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_throughput.jsonl"))
    measure(ap.parse_args())
