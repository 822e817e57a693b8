"""UV labels as 16-bit TIFF files, 16 per call: sfh_amd.tiffdec / sfh_amd.tiffenc (csrc/tiffdec.hip, csrc/tiffenc.hip) beside the
``.npy`` route the labels took before, in the same run.

    python profiles/tiff_throughput.py             # alternating timings -> profiles/tiff_throughput.jsonl

Labels: ``LabelMaker.render`` of the fixture homographies (tests/prep_fixtures.py) at 640x360 and 1280x720, uint16 (id, u, v), 16
per batch.  Both routes go through files in a temporary directory (the page cache serves them).  Per size and repetition, ms per
batch and files/s of
(a) read, TIFF: ``np.fromfile`` of the 16 files + ``TiffDecoder.decode`` (host parse, staging, the upload of the files, 3 launches);
(b) read, npy: ``np.load`` of the 16 files + ``.to(device)``;
(c) write, TIFF: ``TiffEncoder.encode`` + ``to_host()`` (only the files come down) + writing the 16 files;
(d) write, npy: ``.cpu()`` + ``np.save`` of the 16 labels;
and the device calls alone (decode of staged files, encode without the download).  File sizes: the TIFF files against the ``.npy``
files and against libtiff's strips of the same differenced rows (through Pillow, labels 0 and 15 only: Pillow writes no 3 x 16-bit
file, so the strips are compared and the container is this project's).  The feature is the file format: no ratio is a pass
condition; ``tif_slower`` records whether the TIFF route was slower than the ``.npy`` route in that repetition.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 16


def labels(torch, np, W, H):
    import prep_fixtures as F
    from sfh_amd.preparation import LabelMaker
    court, ids = F.court_poi("pitch"), F.court_ids("pitch_v3_nc4_640x360")
    th = np.asarray(F.fixture_thetas(), dtype=np.float32).reshape(-1, 3, 3)
    th = np.stack([th[k % len(th)] for k in range(B)])
    lm = LabelMaker(ids, court, (W, H), 4, uv=True)
    return lm.render(torch.from_numpy(np.ascontiguousarray(th)).cuda())["uv"]


def timed(fn, iters, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters * 1e3


def measure(args):
    import numpy as np
    import torch
    import tiff_cases as tc
    from bench import device_calibration
    from sfh_amd import outputs as O
    from sfh_amd.tiffdec import TiffDecoder
    from sfh_amd.tiffenc import TiffEncoder
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    cal = device_calibration(dev)
    calrow = {"mfma_f16_tflops": cal["mfma_f16_tflops"], "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"]}
    rows = [{"what": "device_calibration", "device": cal["device"], **calrow}]
    for W, H in ((640, 360), (1280, 720)):
        uv = labels(torch, np, W, H)
        host = uv.view(torch.int16).cpu().numpy().view(np.uint16)
        enc = TiffEncoder(H, W, 3, 16, B)
        dec = TiffDecoder(H, W, 3, 16, B, max_file_bytes=enc.capacity)
        files = enc.encode(uv).to_host()
        assert np.array_equal(files[0], O.encode_tiff(host[0])) and np.array_equal(files[B - 1], O.encode_tiff(host[B - 1]))
        back = dec.decode(files)
        assert not dec.status.any() and np.array_equal(back.view(torch.int16).cpu().numpy().view(np.uint16), host)
        R = O.tiff_strip_rows(H, W, 3, 16)
        ours = libtiff = 0
        for k in (0, B - 1):
            head = O.tiff_parse(bytes(files[k]))
            ours += sum(s[1] for s in head["strips"])
            rowsk = tc.stored_rows(host[k][:, :, ::-1], 2, False)
            libtiff += sum(len(tc.libtiff_strip(rowsk[y:y + R])) for y in range(0, H, R))
        rows.append({"what": "size", "size": f"{W}x{H}", "batch": B, "tif_bytes": int(sum(len(f) for f in files)),
                     "npy_bytes": B * (host[0].nbytes + 128), "raw_bytes": int(host.nbytes), "strips_per_file": -(-H // R),
                     "strip_bytes_2_files": int(ours), "libtiff_strip_bytes_2_files": int(libtiff)})
        with tempfile.TemporaryDirectory() as tmp:
            tif = [os.path.join(tmp, f"{k}.tif") for k in range(B)]
            npy = [os.path.join(tmp, f"{k}.npy") for k in range(B)]

            def write_tif():
                for p, f in zip(tif, enc.encode(uv).to_host()):
                    f.tofile(p)

            def write_npy():
                h = uv.view(torch.int16).cpu().numpy().view(np.uint16)
                for p, a in zip(npy, h):
                    np.save(p, a)

            def read_tif():
                dec.decode([np.fromfile(p, dtype=np.uint8) for p in tif])

            def read_npy():
                torch.from_numpy(np.stack([np.load(p) for p in npy]).view(np.int16)).to(dev)

            write_tif()
            write_npy()
            dec.stage(files)
            dec.upload()
            for rep in range(args.reps):                                   # alternating, so drift hits all alike
                t = {"read_tif_ms": timed(read_tif, args.iters, sync), "read_npy_ms": timed(read_npy, args.iters, sync),
                     "write_tif_ms": timed(write_tif, args.iters, sync), "write_npy_ms": timed(write_npy, args.iters, sync),
                     "decode_staged_ms": timed(dec.decode_staged, args.iters, sync),
                     "encode_device_ms": timed(lambda: enc.encode(uv), args.iters, sync)}
                rows.append({"what": "throughput", "size": f"{W}x{H}", "batch": B, "rep": rep, "iters": args.iters,
                             **{k: round(v, 3) for k, v in t.items()},
                             "read_tif_files_per_s": round(B / t["read_tif_ms"] * 1e3, 1),
                             "read_npy_files_per_s": round(B / t["read_npy_ms"] * 1e3, 1),
                             "write_tif_files_per_s": round(B / t["write_tif_ms"] * 1e3, 1),
                             "write_npy_files_per_s": round(B / t["write_npy_ms"] * 1e3, 1),
                             "tif_slower": {"read": bool(t["read_tif_ms"] > t["read_npy_ms"]),
                                            "write": bool(t["write_tif_ms"] > t["write_npy_ms"])}, **calrow})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiff_throughput.jsonl"))
    measure(ap.parse_args())
