"""Label preparation throughput, batch 16: sfh_amd.preparation.LabelMaker (csrc/prepare.hip) against what the package
offered before it, on the same GPU in the same run.

    python profiles/prep_throughput.py             # alternating timings -> profiles/prep_throughput.jsonl
    python profiles/prep_throughput.py --trace     # steady-state make() calls only, for a kernel trace

Render: the fused label render against the composed path sfh_homography_warp_fwd (nearest, int32 ids) -> uint8 cast, plus
torch gathers of the two tables and a stack for the UV label.  The condition the record is read against: the fused render
is not slower than the composed path in any repetition (it writes 1 B / 7 B per pixel in one launch against 4 B + casts).
Fit: frames per second at B = 16 and B = 4096 against the numpy restatement tests/prep_ref.py on 16 host processes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((640, 360), (1280, 720))
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


def _ref_chunk(args):
    import prep_ref as R
    court, manual = args
    return R.fit_batch(court, manual, refine=10)["status"].sum()


def _inputs(np, nframes):
    import prep_fixtures as F
    court = F.court_poi("ncaa")
    th = F.fixture_thetas()
    th = np.stack([th[k % th.shape[0]] for k in range(nframes)])
    manual, _ = F.exact_annotations(court, th, seed=9, n_short=0, noise_px=2.0)
    return court, th, manual


def measure(args):
    import numpy as np
    import torch
    import prep_fixtures as F
    from sfh_amd import engine as E
    from sfh_amd import preparation as P
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    ids = F.court_ids("ncaa_nc4_640x360")
    court, th, manual = _inputs(np, B)
    if args.trace:
        lm = P.LabelMaker(ids, court, (1280, 720), 4, uv=True)
        m = torch.from_numpy(manual).cuda()
        lm.make(m)                              # first call: uploads
        torch.cuda.synchronize()
        for _ in range(args.iters):
            lm.make(m)
        torch.cuda.synchronize()
        return
    from bench import device_calibration
    rows = []
    cal = device_calibration(dev)
    rows.append({"what": "device_calibration", "mfma_f16_tflops": cal["mfma_f16_tflops"],
                 "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"], "device": cal["device"]})
    tmpl = torch.from_numpy(ids.astype(np.float32) / 4.0)[None, None].cuda()
    for W, H in SIZES:
        lm = P.LabelMaker(ids, court, (W, H), 4)
        theta = lm.fit(manual)["theta_f32"]
        u_t, v_t = (torch.from_numpy(t.astype(np.int32)).cuda() for t in (lm.u_tab, lm.v_tab))
        ws, hs = ids.shape[1], ids.shape[0]
        nearest = torch.from_numpy(np.ascontiguousarray(ids)).cuda().to(torch.int64)

        def fused():
            return lm.render(theta, uv=False)["mask"]

        def fused_uv():
            return lm.render(theta, uv=True)["uv"]

        def composed():
            _, wi = E.homography_warp(theta.reshape(B, 1, 3, 3), tmpl, H, W, True, scale=4.0, want_f32=False, want_i32=True,
                                      shared_template=True)
            return wi.to(torch.uint8)

        # the parent commit has no tap indices outside the kernel: the cheapest stock form warps the two coordinate ramps too
        ramp_u = (u_t.to(torch.float32)[None, :].expand(hs, ws) / 65536.0).contiguous()[None, None]
        ramp_v = (v_t.to(torch.float32)[:, None].expand(hs, ws) / 65536.0).contiguous()[None, None]

        def composed_uv():
            th4 = theta.reshape(B, 1, 3, 3)
            _, wi = E.homography_warp(th4, tmpl, H, W, True, scale=4.0, want_f32=False, want_i32=True, shared_template=True)
            _, ui = E.homography_warp(th4, ramp_u, H, W, True, scale=65536.0, want_f32=False, want_i32=True, shared_template=True)
            _, vi = E.homography_warp(th4, ramp_v, H, W, True, scale=65536.0, want_f32=False, want_i32=True, shared_template=True)
            return torch.stack([wi, ui, vi], dim=-1).to(torch.int16)

        assert torch.equal(fused(), composed()), "the fused render and the composed path disagree"
        assert torch.equal(fused_uv().view(torch.int16), composed_uv()), "the fused uv render and the composed path disagree"
        by_m = B * H * W * 1 + hs * ws + 36 * B
        by_uv = B * H * W * 7 + hs * ws + 2 * (hs + ws) + 36 * B
        for rep in range(args.reps):            # alternating, so drift hits all alike
            t_f, t_c = _time(torch, fused, 5, args.iters), _time(torch, composed, 5, args.iters)
            t_fu, t_cu = _time(torch, lambda: lm.render(theta, uv=True), 5, args.iters), _time(torch, composed_uv, 5, args.iters)
            rows.append({"what": "render", "size": f"{W}x{H}", "batch": B, "rep": rep, "iters": args.iters,
                         "mask_us": round(t_f * 1e3, 2), "composed_mask_us": round(t_c * 1e3, 2),
                         "composed_over_fused_mask": round(t_c / t_f, 2), "mask_TBps": round(by_m / (t_f * 1e-3) / 1e12, 3),
                         "uv_us": round(t_fu * 1e3, 2), "composed_uv_us": round(t_cu * 1e3, 2),
                         "composed_over_fused_uv": round(t_cu / t_fu, 2), "uv_TBps": round((by_uv) / (t_fu * 1e-3) / 1e12, 3),
                         "uv_fraction_of_8TBps": round(by_uv / (t_fu * 1e-3) / HBM_PEAK, 3),
                         "fused_not_slower": bool(t_f <= t_c and t_fu <= t_cu)})
    from multiprocessing import Pool
    for nb in (16, 4096):
        court, th, manual = _inputs(np, nb)
        lm = P.LabelMaker(ids, court, (640, 360), 4)
        m = torch.from_numpy(manual).cuda()
        t = _time(torch, lambda: lm.fit(m), 3, 20)
        nref = min(nb, 256)
        chunks = [(court, manual[k:nref:16]) for k in range(16)]
        with Pool(16) as pool:
            pool.map(_ref_chunk, chunks[:1])
            t0 = time.perf_counter()
            pool.map(_ref_chunk, chunks)
            t_ref = time.perf_counter() - t0
        rows.append({"what": "fit", "batch": nb, "refine": 10, "points": int(court.shape[0]), "fit_us": round(t * 1e3, 2),
                     "frames_per_s": round(nb / t * 1e3, 0), "numpy_16proc_frames": nref,
                     "numpy_16proc_frames_per_s": round(nref / t_ref, 1)})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_throughput.jsonl"))
    measure(ap.parse_args())
