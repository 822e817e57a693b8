"""ResNeXt-50 regressor against the ResNet-50 regressor: predict() at 640x360, batch 16, f16x3, synthetic checkpoints.

    python profiles/resnext_throughput.py [--calls 10] [--reps 3] > profiles/resnext_throughput.jsonl

Three alternating repetitions per model, one JSON line each:
  frames_per_s       predict() calls on one batch, a host clock around them, ending in a device synchronise
  conv2_ms           ConvTimer total of the sixteen Bottleneck.conv2 launches of one predict() (device events; taken in a
                     pass of its own, not inside the throughput window)
  convert_ms         resnext50_32x4d only: the sixteen fp32 -> H2 conversions behind the grouped launches
                     (ops._f32_to_split_into on tensors of the layers' shapes, device events) - the boundary cost that
                     fusing the conversion into the neighbours' epilogues would remove
and a summary line: was the ResNeXt-50 regressor slower in any repetition, and the conversions' share of the grouped
layers' time (conv2 + conversions).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, B, NC = 640, 360, 16, 4
NAMES = ("resnext50_32x4d", "resnet50")


def _net(name):
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    court = synth.load_court_template("ncaa_nc4_640x360", NC, B)
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(W, H), unet_size=(W, H), warp_size=(W, H),
                        warp_with_nearest=True, resnet_name=name)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    return net.cuda().eval()


def _conv2_ms(net, x):
    """device-event total of the conv2 launches of one predict(): the layers get a tag of their own for the pass"""
    import torch
    from sfh_amd import engine as E
    eng = net._get_engines()[1]
    layers = [v for k, v in eng.L.items() if k.endswith(".conv2")]
    for v in layers:
        v.tag = "conv2"
    E.PackedConv.timer = tm = E.ConvTimer(only={"conv2"})
    try:
        net.predict(x, consistency=False)
        torch.cuda.synchronize()
        n, work, ms = tm.summary()["conv2"]
    finally:
        E.PackedConv.timer = None
        for v in layers:
            v.tag = "resnet"
    return n, work, ms


def _convert_ms(net, repeats=20):
    """device-event time of one set of the fp32 -> H2 conversions behind the grouped launches"""
    import torch
    from sfh_amd import engine as E
    eng = net._get_engines()[1]
    h, w = ((H + 1) // 2 - 1) // 2 + 1, ((W + 1) // 2 - 1) // 2 + 1
    pairs = []
    for name, width, cout, stride, has_down, bottleneck in eng.blocks:
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
        if isinstance(eng.L[name + ".conv2"], E.GroupedConv):
            src = torch.rand((B, h, w, width), device="cuda")
            pairs.append((src, E.split_empty("h2", B, h, w, width, "cuda")))
    run = lambda: [E._f32_to_split_into(s, d) for s, d in pairs]
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        run()
    e1.record()
    torch.cuda.synchronize()
    return len(pairs), e0.elapsed_time(e1) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from sfh_amd import synth
    torch.cuda.set_device(0)
    x = synth.frames_to_float(synth.synth_frames_u8(B, H, W, seed=19)).cuda()
    nets = {n: _net(n) for n in NAMES}
    with torch.no_grad():
        for net in nets.values():       # warm-up: engines, exponents, every shape
            for _ in range(3):
                net.predict(x, consistency=False)
        torch.cuda.synchronize()
        fps = {n: [] for n in NAMES}
        rec = {}
        for rep in range(a.reps):
            for name, net in nets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    net.predict(x, consistency=False)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                n2, work, ms2 = _conv2_ms(net, x)
                line = {"rep": rep, "model": name, "frames": a.calls * B, "seconds": round(dt, 4),
                        "frames_per_s": round(a.calls * B / dt, 1), "conv2_launches": n2, "conv2_ms": round(ms2, 4),
                        "conv2_gflop": round(work / 1e9, 2), "range_rescales": net.range_rescales}
                if name == "resnext50_32x4d":
                    nconv, msc = _convert_ms(net)
                    line.update(convert_launches=nconv, convert_ms=round(msc, 4))
                fps[name].append(line["frames_per_s"])
                rec.setdefault(name, []).append(line)
                print(json.dumps(line), flush=True)
    gx = rec["resnext50_32x4d"]
    share = [r["convert_ms"] / (r["convert_ms"] + r["conv2_ms"]) for r in gx]
    print(json.dumps({"summary": "predict 640x360 batch 16 f16x3, resnext50_32x4d against resnet50",
                      "frames_per_s": fps,
                      "resnext_slower_in_any_repetition": any(g < d for g, d in zip(fps["resnext50_32x4d"], fps["resnet50"])),
                      "conversion_share_of_grouped_layer_time": [round(s, 3) for s in share]}))


if __name__ == "__main__":
    main()
