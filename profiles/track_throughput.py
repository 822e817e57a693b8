"""Throughput of the inter-frame tracking (sfh_amd.track, csrc/track.hip), batch 16, frames 640x360, on one GPU.

    python profiles/track_throughput.py             # alternating timings -> profiles/track_throughput.jsonl
    python profiles/track_throughput.py --trace     # steady-state calls only, for a kernel trace

Every figure is ms per call on the host clock, ending in a synchronise; what is compared alternates inside every repetition
and every repetition is reported.
(a) sfh_track_accumulate against its yardstick sfh_refine_accumulate (nc = 4, the 640x360 template) on the same grid and
    batch: 16 pairs / frames, grids 640x360 (level 1), 320x180 (level 2) and 80x45 (level 8).
(b) sfh_track_planes, level 2 and level 8, with the bytes it moves (the frames read once, the planes written once).
(c) FrameAligner per call (16 frames with prev: 16 pairs, default levels 8, 4, 2, six steps each) beside ThetaRefiner per call
    (default levels 4, 2, 1, five steps each) on the same batch.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, W, H = 16, 640, 360


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
    from sfh_amd import _lib, synth
    from sfh_amd.refine import ThetaRefiner
    from sfh_amd.track import FrameAligner
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = np.random.default_rng(7)
    # a smooth scene panning by two pixels a frame, as uint8 frames; frame 0 serves as prev
    yy, xx = np.mgrid[0:H, 0:W + 2 * (B + 1)]
    scene = 127 + 60 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + 40 * np.sin((xx + yy) / 41.0) + g.normal(0, 2, xx.shape)
    frames = np.stack([scene[:, 2 * k:2 * k + W] for k in range(B + 1)]).clip(0, 255).astype(np.uint8)
    frames = torch.from_numpy(np.ascontiguousarray(np.repeat(frames[..., None], 3, axis=3))).cuda()
    prev, cur = frames[:1].contiguous(), frames[1:].contiguous()
    theta = torch.from_numpy(np.stack([synth.REALISTIC_THETAS[k % 2] for k in range(B)]).astype(np.float32)).cuda().view(B, 1, 3, 3)
    logits = torch.from_numpy(g.normal(0, 3, (B, 4, H, W)).astype(np.float32)).cuda()
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1).cuda()
    al, rf = FrameAligner((W, H)), ThetaRefiner(court, 4, (W, H))
    al(cur, prev=prev), rf(theta, logits)
    torch.cuda.synchronize()
    rows = []

    # (a) the two accumulate kernels on the same grid and batch
    ident = torch.eye(3, device="cuda").reshape(1, 9).repeat(B, 1).contiguous()
    ia, ib = torch.arange(0, B, dtype=torch.int32, device="cuda"), torch.arange(1, B + 1, dtype=torch.int32, device="cuda")
    calls = {}
    for f in (1, 2, 8):
        pl = torch.empty((B + 1, H // f, W // f), dtype=torch.float32, device="cuda")
        _lib.check(lib.sfh_track_planes(p(frames), B + 1, H, W, f, 0, p(pl), st()), "planes")
        tp = torch.empty((1, H // f, W // f, 4), dtype=torch.float32, device="cuda")
        ev = torch.empty((B, H // f, W // f, 4), dtype=torch.float32, device="cuda")
        _lib.check(lib.sfh_refine_template_planes(p(court), 1, H, W, 4, f, p(tp), st()), "tplanes")
        _lib.check(lib.sfh_refine_evidence_planes(p(logits), B, 4, H, W, f, p(ev), st()), "eplanes")
        nb_t, nb_r = lib.sfh_track_workspace_bytes(B, H // f, W // f), lib.sfh_refine_workspace_bytes(B, H // f, W // f)
        ws = torch.empty(max(nb_t, nb_r) // 8, dtype=torch.float64, device="cuda")
        calls[f] = {
            "track": (lambda pl=pl, f=f, nb=nb_t, ws=ws: lib.sfh_track_accumulate(p(ident), p(pl), B + 1, p(ia), p(ib), B, H, W, f, 0.06, p(ws), nb, st())),
            "refine": (lambda tp=tp, ev=ev, f=f, nb=nb_r, ws=ws: lib.sfh_refine_accumulate(p(theta), p(tp), 0, H, W, p(ev), B, 4, H, W, H, W, f, p(ws), nb, st())),
            "keep": (pl, tp, ev, ws)}
        assert calls[f]["track"]() == 0 and calls[f]["refine"]() == 0
    planes_out = {f: torch.empty((B, H // f, W // f), dtype=torch.float32, device="cuda") for f in (2, 8)}
    plane_call = lambda f: lib.sfh_track_planes(p(cur), B, H, W, f, 0, p(planes_out[f]), st())
    if args.trace:
        for _ in range(args.iters):
            for f in calls:
                calls[f]["track"](), calls[f]["refine"]()
            plane_call(2), plane_call(8)
            al(cur, prev=prev), rf(theta, logits)
        torch.cuda.synchronize()
        return
    for rep in range(args.reps):
        for f in calls:
            row = {"what": "accumulate", "batch": B, "grid": f"{W // f}x{H // f}", "rep": rep, "iters": args.iters}
            for name in ("track", "refine"):
                row[f"ms_{name}"] = round(_host_ms(torch, calls[f][name], 5, args.iters), 5)
            row["track_over_refine"] = round(row["ms_track"] / row["ms_refine"], 3)
            rows.append(row)
    # (b) planes
    for rep in range(args.reps):
        for f in (2, 8):
            ms = _host_ms(torch, lambda: plane_call(f), 5, args.iters)
            nbytes = B * H * W * 3 + B * (H // f) * (W // f) * 4
            rows.append({"what": "planes", "batch": B, "level": f, "rep": rep, "ms": round(ms, 5), "bytes": nbytes,
                         "GB_per_s": round(nbytes / ms / 1e6, 1)})
    # (c) the two schedules per call
    for rep in range(args.reps):
        row = {"what": "per_call", "batch": B, "frame": f"{W}x{H}", "rep": rep, "iters": args.call_iters}
        row["ms_FrameAligner"] = round(_host_ms(torch, lambda: al(cur, prev=prev), 3, args.call_iters), 4)
        row["ms_ThetaRefiner"] = round(_host_ms(torch, lambda: rf(theta, logits), 3, args.call_iters), 4)
        rows.append(row)
    M, stats, accepted, ok = al(cur, prev=prev)
    rows.append({"what": "sanity", "ok": ok.cpu().tolist(), "pan_px": [round(float(v) * (W - 1) / 2, 3) for v in M[:, 0, 0, 2].cpu()],
                 "accepted": accepted.cpu().tolist()[:2]})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--call-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_throughput.jsonl"))
    measure(ap.parse_args())
