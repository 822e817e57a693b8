"""Court overlay throughput at 1280x720 and 640x360, batch 16: sfh_amd.visualize.OverlayRenderer (csrc/overlay.hip) against the
composed path on the same GPU in the same run - what the package offered before the fused kernel:
sfh_homography_warp_fwd (nearest, int32 ids) -> format_masks("rgb") -> the blend in stock torch uint8 / where ops.

    python profiles/overlay_throughput.py                 # alternating timings -> profiles/overlay_throughput.jsonl
    python profiles/overlay_throughput.py --trace         # render + annotate calls at 1280x720 only, for a kernel trace

The condition the record is read against: the fused render is not slower than the composed path at either size (it moves
6 B per pixel against at least 20).  How close it comes to the bandwidth roofline is a result, not a gate: the warp leg is
bound by vector issue (two IEEE divisions and a reciprocal per pixel), as warp.hip's kernel is.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1280, 720), (640, 360))
B = 16
NPTS = 52
HBM_PEAK = 8.0e12


def algorithmic_bytes(W, H, wt, ht):
    """per batch: 3 B read + 3 B written per pixel, one template, 36 B of theta per frame"""
    return B * H * W * 6 + ht * wt * 4 + 36 * B


def _time(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _inputs(torch, np, W, H):
    from sfh_amd import synth
    g = np.random.default_rng(5)
    fr = torch.from_numpy(g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    ident = np.eye(3, dtype=np.float32)
    th = [ident, synth.REALISTIC_THETAS[0], synth.REALISTIC_THETAS[1]]
    th += [(ident + g.normal(0, 0.05, (3, 3))).astype(np.float32) for _ in range(B - 3)]
    theta = torch.from_numpy(np.stack(th)).reshape(B, 1, 3, 3).cuda()
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1).cuda()
    poi = torch.from_numpy(g.random((B, NPTS, 2)).astype(np.float32)).cuda()
    score = torch.from_numpy(np.linspace(0.0, 0.09, B).astype(np.float32)).cuda()
    return fr, theta, court, poi, score


def measure(args):
    import numpy as np
    import torch
    from bench import device_calibration
    from sfh_amd import engine as E
    from sfh_amd import outputs as O
    from sfh_amd import visualize as V
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    rows = []
    if not args.trace:
        cal = device_calibration(dev)
        rows.append({"what": "device_calibration", "mfma_f16_tflops": cal["mfma_f16_tflops"],
                     "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"], "device": cal["device"]})
    for W, H in SIZES:
        fr, theta, court, poi, score = _inputs(torch, np, W, H)
        ht, wt = int(court.shape[2]), int(court.shape[3])
        labels = ['{:4f}'.format(float(s)) for s in score.cpu()]
        plain = V.OverlayRenderer(court, source="warp")
        full = V.OverlayRenderer(court, source="warp", marker_radius=3)
        out = torch.empty_like(fr)

        def render():
            return plain(fr, theta, out=out)

        def render_annotate():
            return full(fr, theta, score=score, poi=poi, labels=labels, out=out)

        def composed():
            _, ids = E.homography_warp(theta, court, H, W, True, scale=4.0, want_f32=False, want_i32=True, shared_template=True)
            rgb = O.format_masks(ids, "rgb", 4)
            keep = (rgb == 0).all(dim=-1, keepdim=True)
            mix = (rgb & fr) + ((rgb ^ fr) >> 1)        # floor((a + b) / 2) without leaving uint8: the cheapest stock form
            return torch.where(keep, fr, mix)

        if args.trace:
            if (W, H) == SIZES[0]:
                for _ in range(args.iters):
                    render_annotate()
                torch.cuda.synchronize()
            continue
        assert torch.equal(render(), composed()), "the fused render and the composed path disagree"
        nbytes = algorithmic_bytes(W, H, wt, ht)
        for rep in range(args.reps):          # alternating, so drift hits all three alike
            t_r = _time(torch, render, 5, args.iters)
            t_a = _time(torch, render_annotate, 5, args.iters)
            t_c = _time(torch, composed, 5, args.iters)
            rows.append({"size": f"{W}x{H}", "batch": B, "rep": rep, "iters": args.iters,
                         "render_us": round(t_r * 1e3, 2), "render_annotate_us": round(t_a * 1e3, 2),
                         "composed_us": round(t_c * 1e3, 2), "composed_over_render": round(t_c / t_r, 2),
                         "render_frames_per_s": round(B / t_r * 1e3, 0), "algorithmic_bytes": nbytes,
                         "render_TBps": round(nbytes / (t_r * 1e-3) / 1e12, 3),
                         "fraction_of_8TBps": round(nbytes / (t_r * 1e-3) / HBM_PEAK, 3),
                         "render_not_slower_than_composed": bool(t_r <= t_c)})
    if not args.trace:
        with open(args.out, "w") as f:
            for r in rows:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_throughput.jsonl"))
    measure(ap.parse_args())
