"""Throughput of the coarse shift search of the tracker (sfh_track_search, FrameAligner(search=)), batch 16 with prev (16
pairs), frames 640x360, factors (8, 4, 2), on one GPU.

    python profiles/search_throughput.py             # alternating timings -> profiles/search_throughput.jsonl

Every figure is ms per call on the host clock, ending in a synchronise; the three things compared alternate inside every
repetition and every repetition is reported:
(a) sfh_track_search alone at radius (16, 8) on the 80x45 planes: 561 shifts of 3600 pixels per pair, two launches;
(b) FrameAligner per call, plain: the yardstick, measured in the same visit;
(c) FrameAligner(search=(16, 8)) per call.
The scene pans by 40 pixels a frame (five plane pixels of level 8), so the searched aligner has a shift to find and the
plain one runs its full schedule on a pair it cannot align; a second pair of rows takes the 2-pixel pan of
profiles/track_throughput.py, which both align.  A last row records what the two found.
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
RADIUS = (16, 8)


def _host_ms(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _clip(np, torch, step):
    g = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W + step * (B + 1)]
    scene = 127 + 60 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + 40 * np.sin((xx + yy) / 41.0) + 25 * np.sin(xx / 97.0 + yy / 61.0) + g.normal(0, 2, xx.shape)
    frames = np.stack([scene[:, step * k:step * k + W] for k in range(B + 1)]).clip(0, 255).astype(np.uint8)
    frames = torch.from_numpy(np.ascontiguousarray(np.repeat(frames[..., None], 3, axis=3))).cuda()
    return frames[:1].contiguous(), frames[1:].contiguous()


def measure(args):
    import math
    import numpy as np
    import torch
    from sfh_amd import _lib
    from sfh_amd.track import FrameAligner
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    f = 8
    hl, wl = H // f, W // f
    ia, ib = torch.arange(0, B, dtype=torch.int32, device="cuda"), torch.arange(1, B + 1, dtype=torch.int32, device="cuda")
    nbytes = lib.sfh_track_search_workspace_bytes(B, *RADIUS)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    shift, found = torch.empty((B, 2), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
    m0, sstats = torch.empty((B, 9), dtype=torch.float32, device="cuda"), torch.empty((B, 3), dtype=torch.float64, device="cuda")
    nmin = float(math.ceil(0.25 * hl * wl))
    for step in (40, 2):
        prev, cur = _clip(np, torch, step)
        pl = torch.empty((B + 1, hl, wl), dtype=torch.float32, device="cuda")
        _lib.check(lib.sfh_track_planes(p(prev), 1, H, W, f, 0, p(pl), st()), "planes")
        _lib.check(lib.sfh_track_planes(p(cur), B, H, W, f, 0, p(pl[1:]), st()), "planes")
        search = lambda: lib.sfh_track_search(p(pl), B + 1, p(ia), p(ib), B, H, W, f, RADIUS[0], RADIUS[1], 0.06, nmin, p(ws), nbytes,
                                              p(shift), p(found), p(m0), p(sstats), st())
        assert search() == 0
        plain, searched = FrameAligner((W, H)), FrameAligner((W, H), search=RADIUS)
        plain(cur, prev=prev), searched(cur, prev=prev)
        torch.cuda.synchronize()
        for rep in range(args.reps):
            row = {"what": "per_call", "pan_px_per_frame": step, "batch": B, "frame": f"{W}x{H}", "radius": list(RADIUS), "rep": rep,
                   "iters": args.call_iters}
            row["ms_search_alone"] = round(_host_ms(torch, search, 5, args.iters), 5)
            row["ms_FrameAligner"] = round(_host_ms(torch, lambda: plain(cur, prev=prev), 3, args.call_iters), 4)
            row["ms_FrameAligner_search"] = round(_host_ms(torch, lambda: searched(cur, prev=prev), 3, args.call_iters), 4)
            row["searched_over_plain"] = round(row["ms_FrameAligner_search"] / row["ms_FrameAligner"], 3)
            rows.append(row)
        px = lambda M: [round(float(v) * (W - 1) / 2, 2) for v in M[:, 0, 0, 2].cpu()]
        Mp, _, _, okp = plain(cur, prev=prev)
        Ms, _, _, oks = searched(cur, prev=prev)
        rows.append({"what": "sanity", "pan_px_per_frame": step, "shift": shift.cpu().tolist()[:3], "found": found.cpu().tolist(),
                     "plain_pan_px": px(Mp)[:4], "searched_pan_px": px(Ms)[:4], "ok_plain": okp.cpu().tolist(), "ok_searched": oks.cpu().tolist()})
    with open(args.out, "w") as fo:
        for r in rows:
            print(json.dumps(r), flush=True)
            fo.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--call-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_throughput.jsonl"))
    measure(ap.parse_args())
