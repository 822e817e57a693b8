"""JPEG encoding throughput, batch 16, quality 90: sfh_amd.jpegenc (csrc/jpegenc.hip) against what a user does without it,
in the same run.

    python profiles/jpegenc_throughput.py             # alternating timings -> profiles/jpegenc_throughput.jsonl
    python profiles/jpegenc_throughput.py --trace     # steady-state calls only, for a kernel trace

Per image set (16 overlay-like frames at 640x360 and 1280x720: the packaged court templates blended over noise frames, the
16 different): us per encode call (two launches), bytes in and out and the file size against raw, against
(a) PIL's libjpeg (outputs.encode_jpeg) of the same 16 frames spread over 16 host processes (the frames live in the workers:
    the time is the encoding and the return of the files), and
(b) the raw device-to-host copy into pinned memory of the same frames, next to the copy of the encoded bytes.
The condition the record is read against: device encode + download of the files is not slower than download of the raw
frames + host encode, in any repetition.
(c) end to end: FramePipeline frames/s with jpeg=("overlay",) against the same pipeline with the raw "overlay" output.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 16
QUALITY = 90
SETS = (("overlay_640x360", "ncaa_nc4_640x360"), ("overlay_1280x720", "ncaa_nc4_1280x720"))
_IMGS = None


def _images(np):
    import jpegenc_cases as cases
    return {key: np.stack([cases.template_over_noise(name, seed=k) for k in range(B)]) for key, name in SETS}


def _worker_init():
    global _IMGS
    import numpy as np
    _IMGS = _images(np)


def _worker_encode(job):
    from sfh_amd.outputs import encode_jpeg
    key, k = job
    return encode_jpeg(_IMGS[key][k], QUALITY).size


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


def _pipeline_fps(torch, net, renderer, frames, n, jpeg):
    from sfh_amd.pipeline import FramePipeline
    pipe = FramePipeline(net, B, tuple(frames[0].shape[1:3]), req_outputs=("theta", "warp_mask", "overlay"), overlay=renderer,
                         jpeg=("overlay",) if jpeg else None, jpeg_quality=QUALITY)
    best = 0.0
    for _ in range(2):                                # the first pass warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for res in pipe.run(frames[k % 2] for k in range(n)):
            got += len(res["overlay_jpeg"]) if jpeg else res["overlay"].shape[0]
        best = got / (time.perf_counter() - t0)
    return best


def measure(args):
    # the host workers first: forked before this process opens the GPU, and they never touch it
    pool = None if args.trace else mp.get_context("fork").Pool(16, initializer=_worker_init)
    import numpy as np
    import torch
    from sfh_amd.jpegenc import JpegEncoder
    from sfh_amd.outputs import encode_jpeg
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    imgs = _images(np)
    encs, devs = {}, {}
    for key, a in imgs.items():
        encs[key] = JpegEncoder(a.shape[1], a.shape[2], 3, B, quality=QUALITY)
        devs[key] = torch.from_numpy(a).cuda()
    if args.trace:
        for warm in (True, False):
            for _ in range(1 if warm else args.iters):
                for key in imgs:
                    encs[key].encode(devs[key])
            torch.cuda.synchronize()
        return
    from bench import device_calibration
    rows = []
    cal = device_calibration(dev)
    calrow = {"mfma_f16_tflops": cal["mfma_f16_tflops"], "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"]}
    rows.append({"what": "device_calibration", "device": cal["device"], **calrow})
    for key, a in imgs.items():
        enc, d = encs[key], devs[key]
        files = enc.encode(d).to_host()
        for k in (0, B - 1):
            assert np.array_equal(files[k], encode_jpeg(a[k], QUALITY)), "device bytes differ from libjpeg's"
        out_bytes = int(sum(f.size for f in files))
        pin_raw = torch.empty(d.shape, dtype=torch.uint8).pin_memory()
        pin_jpg = torch.empty(out_bytes, dtype=torch.uint8).pin_memory()
        jobs = [(key, k) for k in range(B)]
        pool.map(_worker_encode, jobs)                                     # warm
        for rep in range(args.reps):                                       # alternating, so drift hits all alike
            t_enc = _time(torch, lambda: enc.encode(d), 5, args.iters)
            t0 = time.perf_counter()
            for _ in range(args.host_iters):
                zsizes = pool.map(_worker_encode, jobs, chunksize=1)
            t_host = (time.perf_counter() - t0) / args.host_iters * 1e3
            t_raw = _time(torch, lambda: pin_raw.copy_(d, non_blocking=True), 5, args.iters)
            t_jpg = _time(torch, lambda: pin_jpg.copy_(enc.out.data[:out_bytes], non_blocking=True), 5, args.iters)
            rows.append({"what": "encode", "images": key, "batch": B, "quality": QUALITY, "rep": rep, "iters": args.iters,
                         "device_encode_us": round(t_enc * 1e3, 2), "host_16proc_libjpeg_us": round(t_host * 1e3, 1),
                         "raw_d2h_us": round(t_raw * 1e3, 2), "encoded_d2h_us": round(t_jpg * 1e3, 2),
                         "device_path_us": round((t_enc + t_jpg) * 1e3, 2), "host_path_us": round((t_raw + t_host) * 1e3, 1),
                         "device_not_slower": bool(t_enc + t_jpg <= t_raw + t_host),
                         "bytes_in": int(a.size), "bytes_out": out_bytes, "libjpeg_bytes_out": int(sum(zsizes)),
                         "raw_over_file": round(a.size / out_bytes, 2), "passes_max": int(enc.passes().max()), **calrow})
    pool.close()
    pool.join()
    if not args.no_pipeline:
        from sfh_amd import synth
        from sfh_amd.reconstructor import Reconstructor
        from sfh_amd.visualize import OverlayRenderer
        W, H = 640, 360
        court = synth.load_court_template("ncaa_nc4_640x360", 4, B).to(dev)
        poi = synth.load_court_poi("pitch", B).to(dev)
        net = Reconstructor(court, poi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H), warp_with_nearest=True)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 0))
        net.to(dev).eval()
        renderer = OverlayRenderer(court[:1], mask_classes=4, source="warp")
        frames = [torch.from_numpy(synth.synth_frames_u8(B, H, W, seed=500 + k)).pin_memory() for k in range(2)]
        with torch.no_grad():
            for rep in range(args.reps):
                f_raw = _pipeline_fps(torch, net, renderer, frames, args.batches, False)
                f_jpg = _pipeline_fps(torch, net, renderer, frames, args.batches, True)
                rows.append({"what": "pipeline_overlay", "size": f"{W}x{H}", "batch": B, "rep": rep, "batches": args.batches,
                             "raw_overlay_frames_per_s": round(f_raw, 1), "jpeg_overlay_frames_per_s": round(f_jpg, 1),
                             "jpeg_over_raw": round(f_jpg / f_raw, 2), **calrow})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegenc_throughput.jsonl"))
    measure(ap.parse_args())
