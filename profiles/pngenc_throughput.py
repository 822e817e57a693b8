"""PNG encoding throughput, batch 16: sfh_amd.pngenc (csrc/pngenc.hip) against what the package offered before it, in the
same run.

    python profiles/pngenc_throughput.py             # alternating timings -> profiles/pngenc_throughput.jsonl
    python profiles/pngenc_throughput.py --trace     # steady-state calls only, for a kernel trace

Per image set (16 gray class-id masks at 640x360 and 1280x720, 16 palette RGB masks at 1280x720: the packaged court
templates, rolled so that the 16 differ): us per encode call (two launches), bytes in and out, against
(a) outputs.encode_png(level=1) of the same 16 images spread over 16 host processes (the images live in the workers: the
    time is the encoding and the return of the files), and
(b) the raw device-to-host copy into pinned memory that the encoded path replaces, next to the copy of the encoded bytes.
The condition the record is read against: the device encode is not slower than (a) in any repetition.
(c) end to end: FramePipeline frames/s with png=("segm_mask", "warp_mask") against the pipeline without it plus
    MaskPickleWriter.write of both masks on the host, the same frames, the bench's headline geometry.
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
SETS = (("gray_640x360", "ncaa_nc4_640x360", False), ("gray_1280x720", "ncaa_nc4_1280x720", False),
        ("rgb_1280x720", "ncaa_nc4_1280x720", True))
_IMGS = None


def _images(np):
    import pngenc_cases as cases
    return {key: np.stack([cases.variant(cases.template(name, rgb), 3 * k) for k in range(B)]) for key, name, rgb in SETS}


def _worker_init():
    global _IMGS
    import numpy as np
    _IMGS = _images(np)


def _worker_encode(job):
    from sfh_amd.outputs import encode_png
    key, k = job
    return encode_png(_IMGS[key][k], level=1).size


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


def _pipeline_fps(torch, np, net, frames, n, tmp, png):
    from sfh_amd.outputs import MaskPickleWriter
    from sfh_amd.pipeline import FramePipeline
    pipe = FramePipeline(net, B, tuple(frames[0].shape[1:3]), req_outputs=("theta", "warp_mask", "segm_mask"), consistency=True,
                         png=("segm_mask", "warp_mask") if png else None)
    best = 0.0
    for _ in range(2):                                # the first pass warms up
        with MaskPickleWriter(tmp, "segm") as ws, MaskPickleWriter(tmp, "warp") as ww:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, res in enumerate(pipe.run(frames[k % 2] for k in range(n))):
                for b in range(B):
                    if png:
                        ws.write_encoded(f"{i}_{b}", res["segm_mask_png"][b])
                        ww.write_encoded(f"{i}_{b}", res["warp_mask_png"][b])
                    else:
                        ws.write(f"{i}_{b}", res["segm_mask"][b])
                        ww.write(f"{i}_{b}", res["warp_mask"][b])
            best = n * B / (time.perf_counter() - t0)
    return best


def measure(args):
    # the host workers first: forked before this process opens the GPU, and they never touch it
    pool = None if args.trace else mp.get_context("fork").Pool(16, initializer=_worker_init)
    import numpy as np
    import torch
    import pngenc_ref as R
    from sfh_amd.pngenc import PngEncoder
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    imgs = _images(np)
    encs, devs = {}, {}
    for key, a in imgs.items():
        encs[key] = PngEncoder(a.shape[1], a.shape[2], 1 if a.ndim == 3 else 3, B)
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
            assert np.array_equal(files[k], np.frombuffer(R.ref_encode(a[k]), np.uint8)), "device bytes differ from the restatement"
        out_bytes = int(sum(f.size for f in files))
        pin_raw = torch.empty(d.shape, dtype=torch.uint8).pin_memory()
        pin_png = torch.empty(out_bytes, dtype=torch.uint8).pin_memory()
        jobs = [(key, k) for k in range(B)]
        pool.map(_worker_encode, jobs)                                     # warm
        for rep in range(args.reps):                                       # alternating, so drift hits all alike
            t_enc = _time(torch, lambda: enc.encode(d), 5, args.iters)
            t0 = time.perf_counter()
            for _ in range(args.host_iters):
                zsizes = pool.map(_worker_encode, jobs, chunksize=1)
            t_host = (time.perf_counter() - t0) / args.host_iters * 1e3
            t_raw = _time(torch, lambda: pin_raw.copy_(d, non_blocking=True), 5, args.iters)
            t_png = _time(torch, lambda: pin_png.copy_(enc.out.data[:out_bytes], non_blocking=True), 5, args.iters)
            rows.append({"what": "encode", "images": key, "batch": B, "rep": rep, "iters": args.iters,
                         "device_encode_us": round(t_enc * 1e3, 2), "host_16proc_zlib1_us": round(t_host * 1e3, 1),
                         "host_over_device": round(t_host / t_enc, 1), "device_not_slower": bool(t_enc <= t_host),
                         "bytes_in": int(a.size), "bytes_out": out_bytes, "zlib1_bytes_out": int(sum(zsizes)),
                         "raw_d2h_us": round(t_raw * 1e3, 2), "encoded_d2h_us": round(t_png * 1e3, 2), **calrow})
    pool.close()
    pool.join()
    if not args.no_pipeline:
        import tempfile
        from sfh_amd import synth
        from sfh_amd.reconstructor import Reconstructor
        W, H = 640, 360
        court = synth.load_court_template("ncaa_nc4_640x360", 4, B).to(dev)
        poi = synth.load_court_poi("pitch", B).to(dev)
        net = Reconstructor(court, poi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H), warp_with_nearest=True)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 0))
        net.to(dev).eval()
        frames = [torch.from_numpy(synth.synth_frames_u8(B, H, W, seed=500 + k)).pin_memory() for k in range(2)]
        with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
            for rep in range(args.reps):
                f_host = _pipeline_fps(torch, np, net, frames, args.batches, tmp, False)
                f_dev = _pipeline_fps(torch, np, net, frames, args.batches, tmp, True)
                rows.append({"what": "pipeline_mask_stream", "size": f"{W}x{H}", "batch": B, "rep": rep, "batches": args.batches,
                             "host_write_frames_per_s": round(f_host, 1), "device_png_frames_per_s": round(f_dev, 1),
                             "device_over_host": round(f_dev / f_host, 2), **calrow})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pngenc_throughput.jsonl"))
    measure(ap.parse_args())
