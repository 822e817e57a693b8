"""Validation throughput: the native eval_reconstructor (sfh_amd.evaluation) against the reference's eval.py:142-234 loop body
restated here with the same torch ops and .item() syncs, on the same net (640x360, batch 16, f16x3, synthetic checkpoint).

    python profiles/eval_throughput.py                      # alternating timings, one JSON line per run + a summary line
    python profiles/eval_throughput.py --trace              # one native call over the timed batches, bracketed by two marker
                                                            # launches (sfh_probe_mfma_f16, 1 workgroup) for a kernel trace
    python profiles/eval_throughput.py --summarize DIR      # metric-kernel time / bytes/s and foreign launches between markers
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B, NC = 640, 360, 16, 4
HBM_PEAK = 8.0e12
FOREIGN = ("at::native", "at::cuda", "__amd_rocclr", "rccl", "nccl", "c10::", "hipcub", "rocprim", "Cijk_", "thrust")


def _setup(batches, distinct=2):
    import torch
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    court = synth.load_court_template("ncaa_nc4_640x360", NC, B)
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.cuda().train()
    data = []
    for i in range(distinct):
        g = torch.Generator().manual_seed(900 + i)
        b = {"image": synth.frames_to_float(synth.synth_frames_u8(B, H, W, seed=900 + i)),
             "mask": torch.randint(0, NC, (B, H, W), generator=g), "weight": torch.rand(B, generator=g) + 0.5,
             "poi": torch.rand(B, poi.shape[1], 2, generator=g) * 2 - 1,
             "nonzeros": (torch.rand(B, poi.shape[1], generator=g) > 0.3).float()}
        b["num_nonzero"] = b["nonzeros"].sum(1).clamp(min=1.0)
        data.append(b)
    return net, [data[i % distinct] for i in range(batches)]


def reference_eval(net, loader, device, target_size, use_per_sample_weights=True):
    """eval.py:142-234 as written (torch ops, one .item() per score and batch)."""
    import torch
    import torch.nn.functional as F

    def pswc(criterion, inputs, targets, w):           # models/losses.py:33-41
        loss = criterion(inputs, targets, reduction='none')
        return torch.mean(torch.mean(loss, dim=(1, 2)) * w)

    def reproj(inputs, targets, nonzeros, num_nonzero):  # models/losses.py:6-19, 'sum'
        dist = torch.sqrt(torch.sum(torch.pow(targets - inputs, 2), dim=2))
        return torch.sum(torch.sum(dist * nonzeros, dim=1) / num_nonzero)

    ce_score, rec_score, reproj_score, reproj_px, consist_score, uv_score = 0, 0, 0, 0, 0, 0
    n_val = len(loader)
    target_w, target_h = target_size[0], target_size[1]
    net.eval()
    counter = 0
    with torch.no_grad():
        for batch in loader:
            imgs = batch['image'].to(device=device, dtype=torch.float32)
            gt_masks_i = batch['mask'].to(device=device, dtype=torch.long)
            gt_masks_f = gt_masks_i.to(dtype=torch.float32) / float(net.mask_classes)
            gt_poi = batch['poi'].to(device=device, dtype=torch.float32)
            nonzeros = batch['nonzeros'].to(device=device, dtype=torch.float32)
            num_nonzero = batch['num_nonzero'].to(device=device, dtype=torch.float32)
            counter += imgs.shape[0]
            preds = net(imgs)
            logits, poi, warp_masks = preds['logits'], preds['poi'], preds['warp_mask']
            if use_per_sample_weights:
                gt_weights = batch['weight'].to(device=device)
                ce_score += pswc(F.cross_entropy, logits, gt_masks_i, gt_weights).item()
                rec_score += pswc(F.mse_loss, warp_masks, gt_masks_f, gt_weights).item()
            else:
                ce_score += F.cross_entropy(logits, gt_masks_i).item()
                rec_score += F.mse_loss(warp_masks, gt_masks_f).item()
            warp_masks_i = (warp_masks * net.mask_classes).to(dtype=torch.long)
            consist_score += F.cross_entropy(logits, warp_masks_i).item()
            reproj_score += reproj(poi, gt_poi, nonzeros, num_nonzero).item()
            gt_poi[:, :, 0] = gt_poi[:, :, 0] * target_w
            gt_poi[:, :, 1] = gt_poi[:, :, 1] * target_h
            poi[:, :, 0] = poi[:, :, 0] * target_w
            poi[:, :, 1] = poi[:, :, 1] * target_h
            reproj_px += reproj(poi, gt_poi, nonzeros, num_nonzero).item()
    net.train()
    return {'val_seg_score': ce_score / n_val, 'val_rec_score': rec_score / n_val, 'val_uv_score': uv_score / n_val,
            'val_reproj_score': reproj_score / counter, 'val_reproj_px': reproj_px / counter,
            'val_consist_score': consist_score / n_val, 'imgs': imgs.cpu(), 'logits': logits.cpu(),
            'warp_masks': warp_masks.cpu()}


def _marker(lib):
    import ctypes
    import torch
    from sfh_amd import _lib
    from sfh_amd.engine import _stream
    out = torch.empty(256, dtype=torch.float32, device="cuda")
    clk = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.sfh_probe_mfma_f16(1, 1, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(clk.data_ptr()), _stream()),
               "marker")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.batches)
    import torch
    from sfh_amd import _lib
    from sfh_amd.evaluation import eval_reconstructor
    torch.cuda.set_device(0)
    lib = _lib.load()
    net, loader = _setup(a.batches)
    warm = loader[:2]
    eval_reconstructor(net, warm, "cuda", (W, H))
    reference_eval(net, warm, "cuda", (W, H))
    torch.cuda.synchronize()
    if a.trace:
        _marker(lib)
        eval_reconstructor(net, loader, "cuda", (W, H))
        _marker(lib)
        print(json.dumps({"trace": "native eval_reconstructor", "batches": a.batches, "frames": a.batches * B}))
        return
    frames = a.batches * B
    runs = {"native": [], "reference": []}
    scores = {}
    for rep in range(a.reps):
        for name, fn in (("native", eval_reconstructor), ("reference", reference_eval)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(net, loader, "cuda", (W, H))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            runs[name].append(frames / dt)
            scores[name] = {k: v for k, v in res.items() if k.startswith("val_")}
            print(json.dumps({"rep": rep, "variant": name, "frames": frames, "seconds": round(dt, 4),
                              "frames_per_s": round(frames / dt, 1)}), flush=True)
    rel = max(abs(scores["native"][k] - scores["reference"][k]) / max(abs(scores["reference"][k]), 1e-30)
              for k in scores["native"] if scores["reference"][k] != 0)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    print(json.dumps({"summary": "eval throughput 640x360 batch 16 f16x3", "timed_batches": a.batches,
                      "median_frames_per_s": {k: round(v, 1) for k, v in med.items()},
                      "speedup": round(med["native"] / med["reference"], 3), "range_rescales": net.range_rescales,
                      "max_rel_score_diff_native_vs_torch": rel, "scores_native": scores["native"]}))


def summarize(root, batches):
    rows = []
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "probe_mfma_f16_kernel" in r["Kernel_Name"]]
    if len(marks) < 2:
        raise SystemExit(f"expected two marker launches, found {len(marks)}")
    win = rows[marks[-2] + 1:marks[-1]]
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])  # noqa: E731
    pix = [dur(r) for r in win if "eval_pixels_kernel" in r["Kernel_Name"]]
    comb = [dur(r) for r in win if "eval_combine_kernel" in r["Kernel_Name"]]
    foreign = [r["Kernel_Name"] for r in win if any(o in r["Kernel_Name"] for o in FOREIGN)]
    nbytes = (4 * NC + 8 + 4) * B * H * W
    mean_pix = sum(pix) / max(len(pix), 1) * 1e-9
    out = {"window_launches": len(win), "eval_pixels_kernel": {"launches": len(pix), "mean_us": round(mean_pix * 1e6, 2),
                                                               "min_us": round(min(pix) * 1e-3, 2) if pix else None,
                                                               "bytes_per_launch": nbytes,
                                                               "achieved_TBps": round(nbytes / mean_pix / 1e12, 3) if pix else None,
                                                               "share_of_8TBps_peak": round(nbytes / mean_pix / HBM_PEAK, 3) if pix else None},
           "eval_combine_kernel": {"launches": len(comb), "mean_us": round(sum(comb) / max(len(comb), 1) * 1e-3, 2)},
           "window_kernel_time_us": round(sum(dur(r) for r in win) * 1e-3, 1),
           "foreign_launches": len(foreign), "foreign_kernels": sorted(set(n[:120] for n in foreign))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
