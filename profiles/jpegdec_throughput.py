"""JPEG decoding throughput, batch 16, quality 90: sfh_amd.jpegdec (csrc/jpegdec.hip) against what a user does without it, in
the same run.

    python profiles/jpegdec_throughput.py             # alternating timings -> profiles/jpegdec_throughput.jsonl
    python profiles/jpegdec_throughput.py --trace     # steady-state calls only, for `rocprofv3 --kernel-trace --stats -- python ...`

Per case (16 frames at 640x360, 1280x720 and 1920x1080: a packaged court template blended over noise, tiled to the size, the 16
different; each written by libjpeg without DRI and with a DRI of one MCU row): ms per call of
(a) the device leg: host parse + staging, the upload of the files and tables, the device decode (JpegDecoder.decode), and
(b) the host leg: PIL's decode of the same 16 files spread over 16 host processes (the files live in the workers, the frames
    come back) + the upload of the raw frames from pinned memory,
with the largest round count of the entropy kernel per case.  The condition the record is read against: the device leg was not
slower than the host leg in any repetition.  Known and accepted: a file without restart markers occupies ONE workgroup per
image in the entropy kernel - measured here, not tuned.
(c) end to end: FramePipeline frames/s through submit_jpeg (files in) against submit (the decoded frames in), 1280x720.
"""
import argparse
import io
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
SIZES = ((360, 640), (720, 1280), (1080, 1920))
_FILES = None


def _files(np):
    """{(H, W, dri): [B files]}"""
    from PIL import Image
    import jpegenc_cases as cases
    out = {}
    for H, W in SIZES:
        name = "ncaa_nc4_640x360" if H == 360 else "ncaa_nc4_1280x720"
        for dri in (False, True):
            fs = []
            for k in range(B):
                t = cases.template_over_noise(name, seed=k)
                img = np.ascontiguousarray(np.tile(t, (-(-H // t.shape[0]), -(-W // t.shape[1]), 1))[:H, :W, ::-1])
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, "JPEG", quality=QUALITY, subsampling=2, **({"restart_marker_rows": 1} if dri else {}))
                fs.append(buf.getvalue())
            out[H, W, dri] = fs
    return out


def _worker_init():
    global _FILES
    import numpy as np
    _FILES = _files(np)


def _worker_decode(job):
    import numpy as np
    from PIL import Image
    key, k = job
    return np.asarray(Image.open(io.BytesIO(_FILES[key][k])))


def _pipeline_fps(torch, pipe, batches, n, jpeg):
    best = 0.0
    for _ in range(2):                                # the first pass warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for res in pipe.run((batches[k % 2] for k in range(n)), jpeg=jpeg):
            got += res["theta"].shape[0]
        best = got / (time.perf_counter() - t0)
    return best


def measure(args):
    # the host workers first: forked before this process opens the GPU, and they never touch it
    pool = None if args.trace else mp.get_context("fork").Pool(16, initializer=_worker_init)
    import numpy as np
    import torch
    from sfh_amd.jpegdec import JpegDecoder
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    files = _files(np)
    decs = {key: JpegDecoder(key[0], key[1], 3, B, max_file_bytes=max(len(f) for f in fs)) for key, fs in files.items()}
    if args.trace:
        for warm in (True, False):
            for _ in range(1 if warm else args.iters):
                for key, fs in files.items():
                    decs[key].decode(fs)
            torch.cuda.synchronize()
        return
    from bench import device_calibration
    rows = []
    cal = device_calibration(dev)
    calrow = {"mfma_f16_tflops": cal["mfma_f16_tflops"], "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"]}
    rows.append({"what": "device_calibration", "device": cal["device"], **calrow})
    for key, fs in files.items():
        H, W, dri = key
        dec = decs[key]
        got = dec.decode(fs).cpu().numpy()
        assert not dec.status.any()
        for k in (0, B - 1):
            assert np.array_equal(got[k][:, :, ::-1], _decode_here(np, fs[k])), "device pixels differ from libjpeg's"
        rounds = dec.rounds()
        pin_raw = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()
        d_raw = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        jobs = [(key, k) for k in range(B)]
        pool.map(_worker_decode, jobs)                                     # warm
        for rep in range(args.reps):                                       # alternating, so drift hits all alike
            for _ in range(3):
                dec.decode(fs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                dec.decode(fs)
            torch.cuda.synchronize()
            t_dev = (time.perf_counter() - t0) / args.iters * 1e3
            t0 = time.perf_counter()
            for _ in range(args.host_iters):
                frames = pool.map(_worker_decode, jobs, chunksize=1)
                for k, f in enumerate(frames):
                    pin_raw[k].copy_(torch.from_numpy(f))
                d_raw.copy_(pin_raw, non_blocking=True)
                torch.cuda.synchronize()
            t_host = (time.perf_counter() - t0) / args.host_iters * 1e3
            rows.append({"what": "decode", "size": f"{W}x{H}", "dri": "mcu_row" if dri else "none", "batch": B, "quality": QUALITY,
                         "rep": rep, "iters": args.iters, "device_leg_ms": round(t_dev, 3), "host_leg_ms": round(t_host, 3),
                         "device_slower": bool(t_dev > t_host), "file_bytes": int(sum(len(f) for f in fs)),
                         "raw_bytes": B * H * W * 3, "rounds_max": rounds, **calrow})
    pool.close()
    pool.join()
    if not args.no_pipeline:
        from sfh_amd import synth
        from sfh_amd.pipeline import FramePipeline
        from sfh_amd.reconstructor import Reconstructor
        court = synth.load_court_template("ncaa_nc4_640x360", 4, B).to(dev)
        poi = synth.load_court_poi("pitch", B).to(dev)
        net = Reconstructor(court, poi, target_size=(640, 360), unet_size=(640, 360), warp_size=(640, 360), warp_with_nearest=True)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 0))
        net.to(dev).eval()
        for dri in (False, True):
            fs = files[720, 1280, dri]
            rolled = fs[1:] + fs[:1]
            decoded = [torch.from_numpy(np.stack([_decode_here(np, f)[:, :, ::-1] for f in b])).pin_memory() for b in (fs, rolled)]
            pipe = FramePipeline(net, B, (720, 1280), req_outputs=("theta", "warp_mask"), jpeg_in_max_bytes=max(len(f) for f in fs))
            with torch.no_grad():
                for rep in range(args.reps):
                    f_raw = _pipeline_fps(torch, pipe, decoded, args.batches, False)
                    f_jpg = _pipeline_fps(torch, pipe, [fs, rolled], args.batches, True)
                    rows.append({"what": "pipeline", "size": "1280x720", "dri": "mcu_row" if dri else "none", "batch": B, "rep": rep,
                                 "batches": args.batches, "submit_frames_per_s": round(f_raw, 1),
                                 "submit_jpeg_frames_per_s": round(f_jpg, 1), "jpeg_over_raw": round(f_jpg / f_raw, 2), **calrow})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


def _decode_here(np, data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegdec_throughput.jsonl"))
    measure(ap.parse_args())
