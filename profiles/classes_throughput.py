"""predict() with the 4-, 7- and 8-class court models, and the 16-channel stem kernel against the leg it replaces: 640x360,
batch 16, f16x3, synthetic checkpoints, one device.

    python profiles/classes_throughput.py [--calls 10] [--reps 3] > profiles/classes_throughput.jsonl

Three alternating repetitions per class count, one JSON line each:
  frames_per_s       predict(consistency=True) calls on one batch, a host clock around them, ending in a device synchronise
  stem_new_ms        7 and 8 classes, in a ConvTimer pass of its own (device events, not inside the throughput window): the
                     tap-packed stem launch (sfh_stem7x7_fwd, 12 stored channels) on the STN input the UNet pass left
  stem_old_ms        the same input through the leg that launch replaces: sfh_space_to_depth2 (+ the fp32 -> S3 conversion
                     where the 4x4 stem layer is a split one) + the 4x4 stem conv L["stem"]
and a summary line: was the new stem slower than the leg it replaces in any repetition?
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B = 640, 360, 16
CLASSES = (4, 7, 8)


def _template(nc):
    import numpy as np
    import torch
    from sfh_amd import synth
    if nc == 4:
        return synth.load_court_template("ncaa_nc4_640x360", 4, B)
    with np.load(os.path.join(ROOT, "tests", "golden", f"court_ids_ncaa_nc{nc}_640x360.npz")) as z:
        t = torch.from_numpy(z["ids"].astype(np.float32) / float(nc))
    return t[None, None].repeat(B, 1, 1, 1).contiguous()


def _net(nc):
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    net = Reconstructor(_template(nc).cuda(), synth.load_court_poi("pitch", B).cuda(), mask_classes=nc, target_size=(W, H),
                        unet_size=(W, H), warp_size=(W, H), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.precision = "f16x3"
    return net.cuda().eval()


def _stem_ms(net, x, repeats=10):
    """device-event times of the two stem legs on the STN input of one UNet pass -> (new ms, old ms) per launch / leg"""
    import torch
    from sfh_amd import _lib, engine as E
    lib = _lib.load()
    un, rn = net._get_engines()
    y = un.run(x, want_stn_in=True)["stn_in"].clone()
    cs = y.shape[3]
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    c_new = torch.empty((B, H2, W2, 64), device="cuda")
    c_old = torch.empty((B, H2, W2, 64), device="cuda")
    s2d = torch.empty((B, H2, W2, 4 * cs), device="cuda")
    old = rn.L["stem"]
    s2d3 = E.split_empty("s3", B, H2, W2, 4 * cs, "cuda") if old.s3 else None
    st = rn.stem7
    tag = st.tag

    def old_leg():
        _lib.check(lib.sfh_space_to_depth2(y.data_ptr(), s2d.data_ptr(), B, H, W, cs, None), "space_to_depth2")
        src = s2d
        if s2d3 is not None:
            _lib.check(lib.sfh_f32_to_s3(s2d.data_ptr(), s2d3.data_ptr(), B * H2, W2, 4 * cs, None), "f32_to_s3")
            src = s2d3
        old.run(src, B, H2, W2, c_old)

    st.run(y, B, H, W, c_new)       # warm-up of both legs
    old_leg()
    torch.cuda.synchronize()
    st.tag = "stem.new"
    E.PackedConv.timer = tm = E.ConvTimer(only={"stem.new", "stem.old"})
    try:
        for _ in range(repeats):
            st.run(y, B, H, W, c_new)
            t = E._timed("stem.old")
            old_leg()
            t.stop()
            t.add(0.0)
        torch.cuda.synchronize()
        s = tm.summary()
    finally:
        E.PackedConv.timer = None
        st.tag = tag
    diff = float((c_new - c_old).abs().max())
    return s["stem.new"][2] / repeats, s["stem.old"][2] / repeats, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from sfh_amd import synth
    torch.cuda.set_device(0)
    x = synth.frames_to_float(synth.synth_frames_u8(B, H, W, seed=19)).cuda()
    nets = {nc: _net(nc) for nc in CLASSES}
    fps = {nc: [] for nc in CLASSES}
    stem = {nc: [] for nc in CLASSES if nc > 5}
    with torch.no_grad():
        for net in nets.values():       # warm-up: engines, exponents, every shape
            for _ in range(3):
                net.predict(x, consistency=True)
        torch.cuda.synchronize()
        for rep in range(a.reps):
            for nc, net in nets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    net.predict(x, consistency=True)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                line = {"rep": rep, "mask_classes": nc, "frames": a.calls * B, "seconds": round(dt, 4),
                        "frames_per_s": round(a.calls * B / dt, 1), "range_rescales": net.range_rescales}
                if nc in stem:
                    new, old, diff = _stem_ms(net, x)
                    line.update(stem_new_ms=round(new, 4), stem_old_ms=round(old, 4), stem_legs_max_abs_diff=diff)
                    stem[nc].append((new, old))
                fps[nc].append(line["frames_per_s"])
                print(json.dumps(line), flush=True)
    print(json.dumps({"summary": "predict(consistency=True) 640x360 batch 16 f16x3 by mask_classes; 16-channel stem against "
                                 "space_to_depth2 + 4x4 stem conv on the same 12-channel input",
                      "frames_per_s": {str(k): v for k, v in fps.items()},
                      "stem_new_ms": {str(k): [round(n, 4) for n, _ in v] for k, v in stem.items()},
                      "stem_old_ms": {str(k): [round(o, 4) for _, o in v] for k, v in stem.items()},
                      "new_stem_slower_in_any_repetition": any(n > o for v in stem.values() for n, o in v)}))


if __name__ == "__main__":
    main()
