"""Augmentation throughput at 640x360, batch 16: sfh_amd.augment.BatchAugment (csrc/augment.hip) against the same rule run as
stock torch ops on the same GPU (augment.reference_apply on device tensors: what a user would write without the kernels; the
reference's CPU torchvision path cannot be run here), and as a share of the TrainStep step time measured in the same run.

    python profiles/augment_throughput.py                 # alternating timings -> profiles/augment_throughput.jsonl
    python profiles/augment_throughput.py --trace         # HIP path only, for a kernel trace of its launches
    python profiles/augment_throughput.py --summarize DIR # kernel time and achieved bytes/s from the trace's kernel stats
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B = 640, 360, 16
HBM_PEAK = 8.0e12
JIT = {'brightness': 0.35, 'contrast': 0.35, 'saturation': 0.25, 'hue': 0.25}
CONFIGS = {"default": {'apperance': {'jitter': JIT, 'blur': 5}, 'geometric': {'hflip': 0.5}},
           "everything": {'apperance': {'jitter': JIT, 'blur': 5}, 'geometric': {'scale': [0.5, 1.0], 'hflip': 0.5}}}


def algorithmic_bytes(contrast=True):
    """per batch: 3 B read + 12 B written per pixel, 1 B + 8 B for the mask, the pre-pass's 3 B when contrast is on"""
    px = B * H * W
    return {"aug_apply_kernel": px * (3 + 12 + 1 + 8), "aug_gray_mean_kernel": px * 3 if contrast else 0}


def _inputs(torch):
    g = torch.Generator().manual_seed(5)
    fr = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    mk = torch.randint(0, 4, (B, H, W), generator=g, dtype=torch.uint8).cuda()
    return fr, mk


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


def _train_step(torch):
    from sfh_amd import synth, training
    from sfh_amd.reconstructor import Reconstructor
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B).cuda()
    poi = synth.load_court_poi("pitch", B).cuda()
    net = Reconstructor(court, poi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 0))
    net.cuda().train()
    ts = training.TrainStep(net, lr=1e-5, weight_decay=1e-8)
    g = torch.Generator().manual_seed(0)
    x = synth.frames_to_float(synth.synth_frames_u8(B, H, W, seed=0)).cuda()
    nz = torch.ones(B, poi.shape[1]).cuda()
    batch = {"mask": torch.randint(0, 4, (B, H, W), generator=g).cuda(), "weight": torch.ones(B).cuda(),
             "poi": torch.rand(B, poi.shape[1], 2, generator=g).cuda(), "nonzeros": nz, "num_nonzero": nz.sum(1)}
    return lambda: ts.step(x, batch)


def measure(args):
    import torch
    from sfh_amd import augment as A
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    fr, mk = _inputs(torch)
    out_path = os.path.join(ROOT, "profiles", "augment_throughput.jsonl")
    rows = []
    step_ms = None
    if not args.trace:
        step = _train_step(torch)
        step_ms = _time(torch, step, 3, 20)
        rows.append({"what": "TrainStep.step", "ms_per_batch": round(step_ms, 3), "frames_per_s": round(B / step_ms * 1e3, 1)})
    for name, cfg in CONFIGS.items():
        aug = A.BatchAugment(cfg, target_size=(W, H))
        g = torch.Generator().manual_seed(7)
        plist = [aug.sample(B, generator=g) for _ in range(8)]
        state = {"i": 0}

        def hip():
            state["i"] += 1
            return aug(fr, mk, params=plist[state["i"] % 8])

        def torch_ops():
            state["i"] += 1
            return A.reference_apply(fr, mk, plist[state["i"] % 8], blur_k=5, dtype=torch.float32)

        if args.trace:
            _time(torch, hip, 5, args.iters)
            continue
        for rep in range(args.reps):          # alternating, so drift hits both alike
            t_hip = _time(torch, hip, 5, args.iters)
            t_ops = _time(torch, torch_ops, 2, max(20, args.iters // 4))
            rows.append({"config": name, "rep": rep, "hip_ms_per_batch": round(t_hip, 4),
                         "hip_frames_per_s": round(B / t_hip * 1e3, 1), "torch_ops_ms_per_batch": round(t_ops, 3),
                         "torch_ops_frames_per_s": round(B / t_ops * 1e3, 1), "speedup": round(t_ops / t_hip, 1),
                         "share_of_train_step": round(t_hip / step_ms, 5)})
    if not args.trace:
        with open(out_path, "w") as f:
            for r in rows:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")


def summarize(d):
    """kernel_stats.csv of a kernel trace of `--trace` (5 warm-up + iters calls per config, contrast on in both configs)"""
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel_stats.csv under {d}"
    need = algorithmic_bytes()
    for row in csv.DictReader(open(files[0])):
        for k, nbytes in need.items():
            if k in row["Name"]:
                avg_ns = float(row["AverageNs"])
                bps = nbytes / (avg_ns * 1e-9)
                print(json.dumps({"kernel": k, "calls": int(row["Calls"]), "avg_us": round(avg_ns / 1e3, 2),
                                  "algorithmic_bytes": nbytes, "achieved_TBps": round(bps / 1e12, 3),
                                  "fraction_of_8TBps": round(bps / HBM_PEAK, 3)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        measure(a)
