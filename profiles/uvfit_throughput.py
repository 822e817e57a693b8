"""Time of the UV homography fit (sfh_amd.uvfit.UVFit) beside the segmentation refinement (sfh_amd.refine.ThetaRefiner) on the
same logits, and of predict() for a UV-input model beside an img+mask model of the same depth.  640x360, batch 16, nc = 4,
gated, iters = 4; synthetic inputs (a zoomed view's exact uv, logits with a background band).

    python profiles/uvfit_throughput.py              # five alternating repetitions of 50 calls, host clock ending in a
                                                     # synchronise; single launches; predict(); rows -> uvfit_throughput.jsonl
    python profiles/uvfit_throughput.py --rounds 20  # warm-up, then 20 steady-state calls of each and nothing else: the body of
                                                     # a kernel trace (rocprofv3 --kernel-trace --stats -- python ... --rounds 20)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B, NC = 640, 360, 16, 4
WT, HT = 640, 360
OUT = os.path.join(ROOT, "profiles", "uvfit_throughput.jsonl")


def _inputs():
    import torch
    from sfh_amd import synth
    dev = "cuda"
    theta = torch.tensor([0.55, 0.02, 0.1, -0.015, 0.6, -0.05, 0.0, 0.0, 1.0], dtype=torch.float64)
    x = (torch.arange(W, dtype=torch.float64) / (W - 1) - 0.5) * 2
    y = (torch.arange(H, dtype=torch.float64) / (H - 1) - 0.5) * 2
    yy, xx = torch.meshgrid(y, x, indexing="ij")
    wd = theta[6] * xx + theta[7] * yy + theta[8]
    u = ((theta[0] * xx + theta[1] * yy + theta[2]) / wd + (1 + 1.0 / WT)) / 2
    v = ((theta[3] * xx + theta[4] * yy + theta[5]) / wd + (1 + 1.0 / HT)) / 2
    uv = torch.stack([u, v]).float().unsqueeze(0).repeat(B, 1, 1, 1).to(dev).contiguous()
    g = torch.Generator().manual_seed(7)
    lg = torch.randn(B, NC, H, W, generator=g)
    cls = 1 + (torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % (NC - 1)
    cls[:, ::7] = 0
    lg.scatter_add_(1, cls.view(1, 1, H, W).expand(B, 1, H, W), torch.full((B, 1, H, W), 4.0))
    t0 = theta.clone()
    t0[2] += 0.8 * 9 * 2 / WT
    t0[5] += 0.6 * 9 * 2 / HT
    theta0 = t0.float().view(1, 1, 3, 3).repeat(B, 1, 1, 1).to(dev).contiguous()
    court = synth.load_court_template("ncaa_nc4_640x360", NC, 1).to(dev)
    return uv, lg.to(dev).contiguous(), theta0, court


def _timed(fn, calls):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def _alternate(fns, reps, calls):
    """{name: [ms per call] * reps}, the candidates alternating within every repetition"""
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(_timed(fn, calls))
    return out


def _row(name, ms, **kw):
    r = {"what": name, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "reps": len(ms), **kw}
    print(json.dumps(r), flush=True)
    return r


def _models():
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    court = synth.load_court_template("ncaa_nc4_640x360", NC, B)
    poi = synth.load_court_poi("pitch", B)
    nets = {}
    for name, kw in (("img+mask", {}), ("img+mask+uv", dict(unet_uv=True, resnet_input="img+mask+uv"))):
        net = Reconstructor(court.cuda(), poi.cuda(), target_size=(W, H), unet_size=(W, H), warp_size=(W, H), **kw)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
        nets[name] = net.cuda().eval()
    return nets, synth.smooth_frames(B, H, W, seed=19).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--no-predict", action="store_true")
    a = ap.parse_args()
    import torch
    from sfh_amd import _lib
    from sfh_amd.ops import _ptr, _stream
    from sfh_amd.refine import ThetaRefiner
    from sfh_amd.uvfit import UVFit
    uv, lg, theta0, court = _inputs()
    fit = UVFit((WT, HT), (W, H), mask_classes=NC, iters=4)
    ref = ThetaRefiner(court, mask_classes=NC, grid_size=(W, H))
    fns = {"uvfit": lambda: fit(uv, lg, theta0), "refiner": lambda: ref(theta0, lg)}
    for fn in fns.values():
        for _ in range(5):
            fn()
    if a.rounds:
        for _ in range(a.rounds):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        return
    theta, stats, status = fit(uv, lg, theta0)
    rows = [_row(k, ms, shape=f"{B}x{W}x{H}", calls=50) for k, ms in _alternate(fns, 5, 50).items()]
    rows[0].update(status=status.tolist()[:2], stats=stats[0].tolist())

    # single launches: one uvfit accumulate (27 sums, no taps) beside one full-resolution refine accumulate (45 sums, 4 taps)
    lib = _lib.load()
    wk = fit._buffers(B, H, W, uv.device)
    u_min, v_min, kx, ky = fit.constants()
    th9 = theta0.view(B, 9)
    rw = ref._buffers(B, H, W, lg.device)
    _, tplanes = ref._template_planes()

    def uv_acc(theta=th9, logits=lg):
        _lib.check(lib.sfh_uvfit_accumulate(_ptr(uv), _ptr(logits), NC, _ptr(theta), B, H, W, H, W, WT, HT, u_min, v_min, kx, ky, 2.0,
                                            _ptr(wk["ws"]), wk["ws_bytes"], _stream()), "uvfit_accumulate")

    def rf_acc():
        _lib.check(lib.sfh_refine_accumulate(_ptr(th9), _ptr(tplanes[-1]), 0, court.shape[2], court.shape[3], _ptr(rw["ev"][-1]), B, NC,
                                             H, W, H, W, 1, _ptr(rw["ws"]), rw["ws_bytes"], _stream()), "refine_accumulate")

    def uv_step():
        _lib.check(lib.sfh_uvfit_step(_ptr(wk["ws"]), wk["slabs"], B, 0, 0, _ptr(th9), _ptr(wk["cand"]), _ptr(status), _ptr(stats),
                                      _stream()), "uvfit_step")

    singles = {"uvfit_accumulate(theta, logits)": uv_acc, "uvfit_accumulate(theta)": lambda: uv_acc(logits=None),
               "uvfit_accumulate(no theta, logits)": lambda: uv_acc(theta=None), "refine_accumulate(f=1)": rf_acc, "uvfit_step": uv_step}
    pix = B * H * W
    for k, ms in _alternate(singles, 5, 200).items():
        nbytes = pix * (8 + (4 * NC if "logits" in k else 0)) if k.startswith("uvfit_acc") else None
        rows.append(_row(k, ms, calls=200, launches_back_to_back=True,
                         **({"GB_per_s": nbytes / (statistics.median(ms) * 1e-3) / 1e9} if nbytes else {})))
    if not a.no_predict:
        nets, x = _models()
        with torch.no_grad():
            pf = {k: (lambda n=n: n.predict(x, consistency=True)) for k, n in nets.items()}
            for fn in pf.values():
                for _ in range(3):
                    fn()
            rows += [_row(f"predict() {k}", ms, shape=f"{B}x{W}x{H}", calls=5) for k, ms in _alternate(pf, 5, 5).items()]
    try:
        with open(OUT, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    except OSError:
        pass


if __name__ == "__main__":
    main()
