"""Time of the temporal smoothing of theta (sfh_track_smooth, csrc/track.hip) on a clip of 4096 frames, on one GPU.

    python profiles/smooth_throughput.py            # alternating timings -> profiles/smooth_throughput.jsonl

Every figure is ms per call on the host clock, ending in a synchronise; what is compared alternates inside every repetition
and every repetition is reported.  Per radius (12 and 31):
  ms_smooth      sfh_track_smooth, back = ahead = radius, three re-weightings, on a noisy pan / zoom clip (every frame good)
  ms_propagate   sfh_track_propagate with max_gap = radius on the same clip with every second theta zeroed: the existing
                 one-thread-per-frame walk
  ms_aligner     FrameAligner's recorded 0.72 ms per 16 pairs of 640x360 (profiles/track_throughput.jsonl, per_call), scaled to
                 the clip: what measuring M for these frames costs.  Not run here.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 4096
ALIGNER_MS_PER_16 = 0.72


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
    from sfh_amd import _lib
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = np.random.default_rng(7)
    t = np.arange(F)
    M = np.tile(np.eye(3).reshape(9), (F, 1))
    M[:, 0] = M[:, 4] = 1.0 + 0.004 * np.sin(t / 7.0)
    M[:, 2], M[:, 5] = 0.012 * np.cos(t / 11.0), 0.006 * np.sin(t / 5.0)
    true = [np.array([[0.62, 0.05, 0.04], [-0.04, 0.58, -0.03], [0.05, -0.03, 1.0]])]
    for k in range(1, F):
        nxt = true[-1] @ M[k].reshape(3, 3)
        true.append(nxt / nxt[2, 2])
    theta = np.stack([m.reshape(9) for m in true]) + 0.004 * g.standard_normal((F, 9))
    theta[:, 8] = 1.0
    holes = theta.copy()
    holes[1::2] = 0.0
    d = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    theta, holes, M, link = d(theta), d(holes), d(M), torch.ones(F, dtype=torch.int32, device="cuda")
    out, src = torch.empty((F, 9), device="cuda"), torch.empty(F, dtype=torch.int32, device="cuda")
    mem, stats = torch.empty(F, dtype=torch.int32, device="cuda"), torch.empty((F, 3), dtype=torch.float64, device="cuda")
    smooth = lambda r: lib.sfh_track_smooth(p(theta), None, 0.0, p(M), p(link), F, r, r, 3, 0.05, 1, None, p(out), p(mem), p(stats), st())
    carry = lambda r: lib.sfh_track_propagate(p(holes), None, 0.0, p(M), p(link), F, r, p(out), p(src), st())
    rows = []
    for r in (12, 31):
        assert smooth(r) == 0 and carry(r) == 0
    for rep in range(args.reps):
        for r in (12, 31):
            row = {"what": "clip", "frames": F, "radius": r, "rep": rep, "iters": args.iters}
            row["ms_smooth"] = round(_host_ms(torch, lambda: smooth(r), 5, args.iters), 5)
            row["ms_propagate"] = round(_host_ms(torch, lambda: carry(r), 5, args.iters), 5)
            row["ms_aligner_recorded"] = round(ALIGNER_MS_PER_16 * F / 16, 2)
            row["aligner_over_smooth"] = round(row["ms_aligner_recorded"] / row["ms_smooth"], 1)
            rows.append(row)
    smooth(12)
    torch.cuda.synchronize()
    rows.append({"what": "sanity", "members_min_max": [int(mem.min()), int(mem.max())], "finite": bool(torch.isfinite(out).all()),
                 "median_deviation": round(float(stats[:, 2].median()), 5)})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_throughput.jsonl"))
    measure(ap.parse_args())
