"""PNG decoding throughput, 16 files per call: sfh_amd.pngdec (csrc/pngdec.hip) against what a user does without it, in the same
run.

    python profiles/pngdec_throughput.py             # alternating timings -> profiles/pngdec_throughput.jsonl
    python profiles/pngdec_throughput.py --trace     # steady-state calls only, for `rocprofv3 --kernel-trace --stats -- python ...`

Cases (16 files each): the packaged court id masks at 640x360 and 1280x720, the 16 rolled against each other, as sfh_amd.pngenc
writes them (one IDAT chunk per strip: the segmented leg) and as outputs.encode_png writes them (zlib, one stream: the serial
leg); the 3421x1819 one-hot mask of tests/golden/png (libpng, 7-9 chunks cut anywhere: the serial leg); a 1280x720 RGB
photograph-like frame (a court template over noise) from PIL (almost all literals in one stream: the case this decoder is
expected to lose).  Per case, ms per call of
(a) the device leg: host parse with every chunk's CRC-32 + staging, the upload of the files and tables, the device decode
    (PngDecoder.decode), and
(b) the host leg: PIL's decode of the same 16 files spread over 16 host processes (the files live in the workers, the pixels
    come back) + the upload of the pixels from pinned memory,
with the share of the images that took the segmented leg.  The condition each case is read against: was the device leg slower
than the host leg in any repetition.  Nothing here gates the change.
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
_FILES = None


def _files(np):
    """{case name: (H, W, C, [B files])}"""
    from PIL import Image
    import jpegenc_cases
    import pngenc_cases
    import pngenc_ref
    from sfh_amd.outputs import encode_png
    out = {}
    for name in ("ncaa_nc4_640x360", "ncaa_nc4_1280x720"):
        ids = pngenc_cases.template(name)
        masks = [pngenc_cases.variant(ids, 3 * k) for k in range(B)]
        H, W = ids.shape
        out[f"mask_{W}x{H}_pngenc"] = (H, W, 1, [bytes(pngenc_ref.ref_encode(m)) for m in masks])      # sfh_amd.pngenc's bytes
        out[f"mask_{W}x{H}_encode_png"] = (H, W, 1, [bytes(encode_png(m)) for m in masks])
    with open(os.path.join(ROOT, "tests", "golden", "png", "mask_ncaa_v4_nc4_m_onehot.png"), "rb") as f:
        out["mask_3421x1819_fixture"] = (1819, 3421, 1, [f.read()] * B)
    fs = []
    for k in range(B):
        t = jpegenc_cases.template_over_noise("ncaa_nc4_1280x720", seed=k)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(t[:720, :1280, ::-1])).save(buf, "PNG")
        fs.append(buf.getvalue())
    out["photo_1280x720_rgb_pil"] = (720, 1280, 3, fs)
    return out


def _worker_init():
    global _FILES
    import numpy as np
    _FILES = _files(np)


def _worker_decode(job):
    import numpy as np
    from PIL import Image
    key, k = job
    return np.asarray(Image.open(io.BytesIO(_FILES[key][3][k])))


def measure(args):
    # the host workers first: forked before this process opens the GPU, and they never touch it
    pool = None if args.trace else mp.get_context("fork").Pool(16, initializer=_worker_init)
    import numpy as np
    import torch
    from sfh_amd.pngdec import PngDecoder
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    files = _files(np)
    decs = {key: PngDecoder(H, W, C, B, bgr=False, max_file_bytes=max(len(f) for f in fs)) for key, (H, W, C, fs) in files.items()}
    if args.trace:
        for warm in (True, False):
            for _ in range(1 if warm else args.iters):
                for key, v in files.items():
                    decs[key].decode(v[3])
            torch.cuda.synchronize()
        return
    from bench import device_calibration
    rows = []
    cal = device_calibration(dev)
    calrow = {"mfma_f16_tflops": cal["mfma_f16_tflops"], "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"]}
    rows.append({"what": "device_calibration", "device": cal["device"], **calrow})
    for key, (H, W, C, fs) in files.items():
        dec = decs[key]
        got = dec.decode(fs).cpu().numpy()
        assert not dec.status.any()
        for k in (0, B - 1):
            assert np.array_equal(got[k], _decode_here(np, fs[k])), "device pixels differ from PIL's"
        share = float(dec.segmented().mean())
        shape = (B, H, W) + ((C,) if C > 1 else ())
        pin_raw = torch.empty(shape, dtype=torch.uint8).pin_memory()
        d_raw = torch.empty(shape, dtype=torch.uint8, device=dev)
        jobs = [(key, k) for k in range(B)]
        pool.map(_worker_decode, jobs)                                     # warm
        for rep in range(args.reps):                                       # alternating, so drift hits all alike
            for _ in range(2):
                dec.decode(fs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                dec.decode(fs)
            torch.cuda.synchronize()
            t_dev = (time.perf_counter() - t0) / args.iters * 1e3
            t0 = time.perf_counter()
            for _ in range(args.host_iters):
                images = pool.map(_worker_decode, jobs, chunksize=1)
                for k, f in enumerate(images):
                    pin_raw[k].copy_(torch.from_numpy(f))
                d_raw.copy_(pin_raw, non_blocking=True)
                torch.cuda.synchronize()
            t_host = (time.perf_counter() - t0) / args.host_iters * 1e3
            rows.append({"what": "decode", "case": key, "size": f"{W}x{H}x{C}", "batch": B, "rep": rep, "iters": args.iters,
                         "device_leg_ms": round(t_dev, 3), "host_leg_ms": round(t_host, 3), "device_slower": bool(t_dev > t_host),
                         "segmented_share": share, "file_bytes": int(sum(len(f) for f in fs)), "raw_bytes": B * H * W * C, **calrow})
    pool.close()
    pool.join()
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


def _decode_here(np, data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pngdec_throughput.jsonl"))
    measure(ap.parse_args())
