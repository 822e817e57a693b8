"""Frame resize throughput, batch 16, Pillow's bicubic: sfh_amd.resample (csrc/resample.hip) against what a user does without
it, in the same run.

    python profiles/resample_throughput.py             # alternating timings -> profiles/resample_throughput.jsonl
    rocprofv3 --kernel-trace --stats -- python profiles/resample_throughput.py --trace     # steady-state calls only

Per source size (16 different RGB frames at 1280x720 and 1920x1080, resized to 640x360):
(a) device leg: upload of the source frames from pinned memory + Resampler.to_input;
    host leg: Image.resize of the same 16 frames spread over 16 host processes (the frames live in the workers: the time is the
    resize and the return of the resized frames) + upload of the resized frames + frames_u8_to_input.
    The condition the record is read against: the device leg is not slower than the host leg, in any repetition.
(b) the kernel alone against sfh_u8hwc_areak_to_f32nchw (the INTER_AREA path of the same size pair).
(c) end to end: FramePipeline(resize="pil") frames/s against resize="area" on the same frames.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 16
DST = (360, 640)
SETS = (("1280x720", (720, 1280)), ("1920x1080", (1080, 1920)))
_IMGS = None


def _images():
    from sfh_amd import synth
    return {key: synth.synth_frames_u8(B, hw[0], hw[1], seed=900 + k) for k, (key, hw) in enumerate(SETS)}


def _worker_init():
    global _IMGS
    _IMGS = _images()


def _worker_resize(job):
    import numpy as np
    from PIL import Image
    key, k = job
    return np.asarray(Image.fromarray(_IMGS[key][k]).resize((DST[1], DST[0])))


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


def _pipeline_fps(torch, net, frames, n, resize):
    from sfh_amd.pipeline import FramePipeline
    pipe = FramePipeline(net, B, tuple(frames[0].shape[1:3]), req_outputs=("theta", "warp_mask"), resize=resize)
    best = 0.0
    for _ in range(2):                                # the first pass warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for res in pipe.run(frames[k % 2] for k in range(n)):
            got += res["theta"].shape[0]
        best = got / (time.perf_counter() - t0)
    return best


def measure(args):
    # the host workers first: forked before this process opens the GPU, and they never touch it
    pool = None if args.trace else mp.get_context("fork").Pool(16, initializer=_worker_init)
    import numpy as np
    import torch
    from sfh_amd import ops
    from sfh_amd.resample import Resampler
    assert torch.cuda.is_available(), "needs the MI355X: a timing without it says nothing"
    dev = torch.device("cuda", 0)
    imgs = _images()
    rs = {key: Resampler(hw, DST) for key, hw in SETS}
    pins = {key: torch.from_numpy(a).pin_memory() for key, a in imgs.items()}
    devs = {key: p.cuda() for key, p in pins.items()}
    if args.trace:
        for warm in (True, False):
            for _ in range(1 if warm else args.iters):
                for key in imgs:
                    rs[key].to_input(devs[key])
            torch.cuda.synchronize()
        return
    from bench import device_calibration
    rows = []
    cal = device_calibration(dev)
    calrow = {"mfma_f16_tflops": cal["mfma_f16_tflops"], "in_kernel_clock_ghz": cal["in_kernel_clock_ghz"]}
    rows.append({"what": "device_calibration", "device": cal["device"], **calrow})
    for key, hw in SETS:
        r, d, pin = rs[key], devs[key], pins[key]
        jobs = [(key, k) for k in range(B)]
        small = np.stack(pool.map(_worker_resize, jobs))                   # warm, and the bytes to compare
        assert np.array_equal(r.resize(d).cpu().numpy(), small), "device bytes differ from Pillow's"
        pin_small = torch.from_numpy(small).pin_memory()
        dsmall = torch.empty_like(pin_small, device=dev)
        k = hw[1] // DST[1]
        for rep in range(args.reps):                                       # alternating, so drift hits all alike
            t_dev = _time(torch, lambda: (d.copy_(pin, non_blocking=True), r.to_input(d)), 5, args.iters)
            t0 = time.perf_counter()
            for _ in range(args.host_iters):
                pool.map(_worker_resize, jobs, chunksize=1)
            t_host = (time.perf_counter() - t0) / args.host_iters * 1e3
            t_up = _time(torch, lambda: (dsmall.copy_(pin_small, non_blocking=True), ops.frames_u8_to_input(dsmall)), 5, args.iters)
            t_kernel = _time(torch, lambda: r.to_input(d), 5, args.iters)
            t_area = _time(torch, lambda: ops.frames_u8_to_input(d, (DST[1], DST[0])), 5, args.iters)
            rows.append({"what": "resize", "frames": key, "to": f"{DST[1]}x{DST[0]}", "batch": B, "rep": rep, "iters": args.iters,
                         "device_leg_us": round(t_dev * 1e3, 2), "host_16proc_pillow_us": round(t_host * 1e3, 1),
                         "resized_upload_to_input_us": round(t_up * 1e3, 2), "host_leg_us": round((t_host + t_up) * 1e3, 1),
                         "device_slower": bool(t_dev > t_host + t_up), "resample_kernel_us": round(t_kernel * 1e3, 2),
                         f"area{k}_kernel_us": round(t_area * 1e3, 2), "bytes_in": int(imgs[key].size), **calrow})
    pool.close()
    pool.join()
    if not args.no_pipeline:
        from sfh_amd import synth
        from sfh_amd.reconstructor import Reconstructor
        W, H = DST[1], DST[0]
        court = synth.load_court_template("ncaa_nc4_640x360", 4, B).to(dev)
        poi = synth.load_court_poi("pitch", B).to(dev)
        net = Reconstructor(court, poi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H), warp_with_nearest=True)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 0))
        net.to(dev).eval()
        frames = [torch.from_numpy(synth.synth_frames_u8(B, 720, 1280, seed=500 + k)).pin_memory() for k in range(2)]
        with torch.no_grad():
            for rep in range(args.reps):
                f_area = _pipeline_fps(torch, net, frames, args.batches, "area")
                f_pil = _pipeline_fps(torch, net, frames, args.batches, "pil")
                rows.append({"what": "pipeline", "frames": "1280x720", "batch": B, "rep": rep, "batches": args.batches,
                             "area_frames_per_s": round(f_area, 1), "pil_frames_per_s": round(f_pil, 1),
                             "pil_over_area": round(f_pil / f_area, 3), **calrow})
    with open(args.out, "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_throughput.jsonl"))
    measure(ap.parse_args())
