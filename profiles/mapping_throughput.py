"""Frame -> court mapping throughput, batch 16: sfh_amd.mapping (csrc/mapping.hip) against what the package offered before
it, on the same GPU in the same run.

    python profiles/mapping_throughput.py             # alternating timings -> profiles/mapping_throughput.jsonl
    python profiles/mapping_throughput.py --trace     # steady-state calls only, for a kernel trace

(a) top view: TopViewRenderer (invert + one render launch) against the composed path of the parent commit - split the uint8
    frames to three fp32 planes, three sfh_homography_warp_fwd (nearest) sampling them with theta_c2f, cast to uint8, stack.
    The condition the record is read against: the fused path is not slower in any repetition.  Algorithmic traffic of the
    fused path: 3 B read + 3 B + 1 B written per court pixel.
(b) mosaic: CourtMosaic.add against render-then-torch-sum (TopViewRenderer, masked int32 sum over the batch, count).
(c) points: sfh_map_points at N = 10^6 against the numpy restatement tests/mapping_ref.py on the host.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1280, 720), (640, 360))
B = 16
HBM_PEAK = 8.0e12


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


def _thetas(np, n):
    from sfh_amd import synth
    g = np.random.default_rng(7)
    t = [synth.REALISTIC_THETAS[k % 2] if k % 4 < 2 else (np.eye(3) + g.normal(0, 0.15, (3, 3))).astype(np.float32)
         for k in range(n)]
    return np.stack(t).astype(np.float32)


def measure(args):
    import numpy as np
    import torch
    import mapping_ref as R
    from sfh_amd import engine as E
    from sfh_amd import mapping as M
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    theta = torch.from_numpy(_thetas(np, B)).cuda()
    N = 1000000
    g = np.random.default_rng(1)
    pts = (g.uniform(0, 1, (N, 2)) * [1280, 720]).astype(np.float32)
    idx = g.integers(0, 4096, N).astype(np.int32)
    cm = M.CourtMapping(_thetas(np, 4096))
    mapper = M.FrameCourtMapper(cm)
    pd, idd = torch.from_numpy(pts).cuda(), torch.from_numpy(idx).cuda()
    if args.trace:
        W, H = SIZES[0]
        fr = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()   # a copy, no kernel
        rn, rb, mos = M.TopViewRenderer((W, H)), M.TopViewRenderer((W, H), "bilinear"), M.CourtMosaic((W, H))
        for warm in (True, False):              # first round: allocations and uploads
            for _ in range(1 if warm else args.iters):
                rn(fr, theta)
                rb(fr, theta)
                mos.add(fr, theta)
                mos.result()
                mapper.frame_to_court(pd, idd, (1280, 720), units="meters")
            torch.cuda.synchronize()
        return
    from bench import device_calibration
    rows = []
    cal = device_calibration(dev)
    calrow = {"mfma_f16_tflops": cal["mfma_f16_tflops"], "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"]}
    rows.append({"what": "device_calibration", "device": cal["device"], **calrow})
    for W, H in SIZES:
        fr = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
        rn, rb = M.TopViewRenderer((W, H), "nearest"), M.TopViewRenderer((W, H), "bilinear")

        def fused():
            return rn(fr, theta)["top_view"]

        def fused_bilinear():
            return rb(fr, theta)["top_view"]

        def composed():
            c2f, _ = M.invert_theta(theta)
            planes = fr.permute(0, 3, 1, 2).to(torch.float32).contiguous()
            out = [E.homography_warp(c2f.reshape(B, 1, 3, 3), planes[:, c:c + 1].contiguous(), H, W, True)[0] for c in range(3)]
            return torch.stack(out, dim=-1).to(torch.uint8)

        assert torch.equal(fused(), composed()), "the fused top view and the composed path disagree"
        mos = M.CourtMosaic((W, H))

        def mosaic():
            mos.add(fr, theta)

        def render_then_sum():
            o = rn(fr, theta)
            ok = o["valid"] != 0
            return (o["top_view"].to(torch.int32) * ok[..., None]).sum(dim=0), ok.sum(dim=0)

        mos.add(fr, theta)
        s, n = render_then_sum()
        assert torch.equal(mos.sum, s.to(torch.int32)) and torch.equal(mos.count, n.to(torch.int32)), "mosaic and render-then-sum disagree"
        by = B * H * W * 7 + 36 * B
        for rep in range(args.reps):            # alternating, so drift hits all alike
            t_f, t_c = _time(torch, fused, 5, args.iters), _time(torch, composed, 5, args.iters)
            t_b = _time(torch, fused_bilinear, 5, args.iters)
            t_m, t_r = _time(torch, mosaic, 5, args.iters), _time(torch, render_then_sum, 5, args.iters)
            rows.append({"what": "top_view", "size": f"{W}x{H}", "batch": B, "rep": rep, "iters": args.iters,
                         "fused_us": round(t_f * 1e3, 2), "composed_us": round(t_c * 1e3, 2),
                         "composed_over_fused": round(t_c / t_f, 2), "fused_TBps": round(by / (t_f * 1e-3) / 1e12, 3),
                         "fused_fraction_of_8TBps": round(by / (t_f * 1e-3) / HBM_PEAK, 3),
                         "bilinear_us": round(t_b * 1e3, 2), "fused_not_slower": bool(t_f <= t_c), **calrow})
            rows.append({"what": "mosaic", "size": f"{W}x{H}", "batch": B, "rep": rep, "iters": args.iters,
                         "add_us": round(t_m * 1e3, 2), "render_then_sum_us": round(t_r * 1e3, 2),
                         "render_then_sum_over_add": round(t_r / t_m, 2), "add_not_slower": bool(t_m <= t_r), **calrow})
    want, wflag = None, None
    t0 = time.perf_counter()
    want, wflag = R.map_points(pts, idx, cm.theta, (1280, 720), M.UNITS["meters"])
    t_ref = time.perf_counter() - t0
    out, flag = mapper.frame_to_court(pd, idd, (1280, 720), units="meters")
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(flag.cpu().numpy(), wflag)
    for rep in range(args.reps):
        t = _time(torch, lambda: mapper.frame_to_court(pd, idd, (1280, 720), units="meters"), 5, args.iters)
        rows.append({"what": "map_points", "points": N, "frames": len(cm), "rep": rep, "iters": args.iters,
                     "map_us": round(t * 1e3, 2), "points_per_s": round(N / t * 1e3, 0), "numpy_host_ms": round(t_ref * 1e3, 1),
                     "numpy_over_gpu": round(t_ref * 1e3 / t, 0), **calrow})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapping_throughput.jsonl"))
    measure(ap.parse_args())
