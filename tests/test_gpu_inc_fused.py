"""The UNet's first DoubleConv as ONE launch (csrc/conv_inc_fused.hip, engine.run_inc_fused; Options.fuse_inc) against the two
launches it replaces (sfh_conv3x3_c4h2_fwd writing the 64-channel H2 intermediate, sfh_conv_s3_fwd reading it back): the fused
kernel performs the same products in the same order per output element, so everything it leaves must have the same BITS - the
full-resolution output planes, the pooled output planes, and the range / overflow words of the intermediate (which no longer
exists as a tensor) and of the output."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from sfh_amd import synth  # noqa: E402


def _layers(cin, seed):
    """(first conv over the FH2 frame, second conv) with deterministic weights and BatchNorm statistics"""
    from sfh_amd import engine as E
    g = torch.Generator().manual_seed(seed)
    cv1, cv2 = torch.nn.Conv2d(cin, 64, 3, padding=1), torch.nn.Conv2d(64, 64, 3, padding=1)
    bn1, bn2 = torch.nn.BatchNorm2d(64), torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        for cv, fan in ((cv1, 9 * cin), (cv2, 9 * 64)):
            cv.weight.copy_(torch.randn(cv.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
            cv.bias.copy_(torch.randn(64, generator=g) * 0.1)
        for bn in (bn1, bn2):
            bn.weight.copy_(0.5 + torch.rand(64, generator=g))
            bn.bias.copy_(torch.randn(64, generator=g) * 0.2)      # some channels' ReLU(shift) is positive, some zero
            bn.running_mean.copy_(torch.randn(64, generator=g) * 0.1)
            bn.running_var.copy_(0.5 + torch.rand(64, generator=g))
    for m in (cv1, cv2, bn1, bn2):
        m.cuda().eval()
    l0 = E.PackedConv(cv1.weight, cv1.bias, bn1, 3, cin, fmt=None, frame_h2=True)
    l3 = E.PackedConv(cv2.weight, cv2.bias, bn2, 3, 64, fmt="h2")
    return l0, l3


def _frame_h2(x, exp):
    """(B,C,H,W) float32 -> the FH2 frame tensor, held as float32 (B,H,W,4)"""
    from sfh_amd import _lib
    from sfh_amd import engine as E
    B, C, H, W = x.shape
    fh2 = torch.zeros((B, H, W, 4), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sfh_frame_to_h2(E._ptr(x), None, E._ptr(fh2), B, C, H, W, exp, None, None, E._stream()), "frame_to_h2")
    return fh2


def _both_ways(l0, l3, fh2, exps=(2, 2, 2)):
    """-> {"two": ..., "one": ...}, each (output planes, pooled planes, words [range mid, range out, overflow])"""
    from sfh_amd import engine as E
    B, H, W, _ = fh2.shape
    e_frame, e_mid, e_out = exps
    got = {}
    for how in ("two", "one"):
        words = torch.zeros(3, dtype=torch.int32, device=fh2.device)
        l0.overflow = l3.overflow = words[2:3]
        w_mid, w_out = words.data_ptr(), words.data_ptr() + 4
        out = torch.zeros(E.split_shape("h2", B, H, W, 64), dtype=torch.float16, device=fh2.device)
        pool = torch.zeros(E.split_shape("h2", B, H // 2, W // 2, 64), dtype=torch.float16, device=fh2.device)
        if how == "two":
            mid = torch.zeros_like(out)
            l0.run(fh2, B, H, W, mid, exp_src=e_frame, exp_dst=e_mid, range_word=w_mid)
            l3.run(mid, B, H, W, out, dst_pool=pool, exp_src=e_mid, exp_dst=e_out, range_word=w_out)
        else:
            E.run_inc_fused(l0, l3, fh2, out, B, H, W, dst_pool=pool, exp_frame=e_frame, exp_mid=e_mid, exp_dst=e_out,
                            range_mid=w_mid, range_dst=w_out)
        torch.cuda.synchronize()
        got[how] = (out, pool, words)
    return got


def _assert_same_bits(got):
    (o2, p2, w2), (o1, p1, w1) = got["two"], got["one"]
    # (bit patterns: NaN planes would compare unequal as floats)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)), "full-resolution output planes differ"
    assert torch.equal(p1.view(torch.int16), p2.view(torch.int16)), "pooled output planes differ"
    assert torch.equal(w1, w2), f"range / overflow words differ: {w1.tolist()} / {w2.tolist()}"
    assert int(w2[0]) != 0 and int(w2[1]) != 0       # both tensors reported a range
    assert o2.float().abs().sum().item() > 0.0


@pytest.mark.parametrize("B,C,H,W,exps", [
    (2, 3, 34, 70, (2, 2, 2)),     # odd tile remainders both ways, tiles across the zero rows between frames, a partial last tile
    (1, 3, 16, 32, (2, 2, 2)),     # one tile per tile row: every halo pixel is frame border or the shared zero rows
    (3, 4, 45, 80, (1, 0, 3)),     # img+mask-style 4-channel input, odd height (even-rows-per-frame padding), other exponents
])
def test_one_launch_gives_the_two_launch_bits(B, C, H, W, exps):
    l0, l3 = _layers(C, 7 + C)
    x = synth.smooth_frames(B, H, W, seed=3)
    if C == 4:
        x = torch.cat([x, x[:, :1] * 0.5 + 0.25], 1).contiguous()
    got = _both_ways(l0, l3, _frame_h2(x.cuda(), exps[0]), exps)
    _assert_same_bits(got)
    assert int(got["two"][2][2]) == 0               # nothing saturated


def test_nan_pixel_and_saturation_behave_identically():
    """frame 0 holds a NaN pixel (written into the FH2 tensor itself: sfh_frame_to_h2 would saturate it away), frame 1
    drives the intermediate beyond the fp16 range: same output bits - the NaN reaches exactly the same outputs -, the
    intermediate's range word holds the NaN pattern and the overflow word is raised in both forms."""
    from sfh_amd.h2ranges import H2Ranges
    B, H, W = 2, 24, 40
    l0, l3 = _layers(3, 11)
    x = synth.smooth_frames(B, H, W, seed=5)
    x[1] *= 8000.0
    fh2 = _frame_h2(x.cuda(), 2)
    fh2.view(torch.float16).view(B, H, W, 8)[0, 9, 17, 1] = float("nan")
    got = _both_ways(l0, l3, fh2)
    _assert_same_bits(got)
    words = got["one"][2].cpu().numpy().view("uint32")
    assert words[0] >= H2Ranges.NONFINITE and words[2] == 1


def _model(B, H, W):
    from sfh_amd.reconstructor import Reconstructor
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :H, :W].contiguous()
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(W, H), unet_size=(W, H), warp_size=(W, H),
                        warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    return net.cuda().eval()


def _count_fused_calls(monkeypatch):
    from sfh_amd import engine as E
    calls = []
    real = E.run_inc_fused
    monkeypatch.setattr(E, "run_inc_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_predict_is_unchanged_by_the_switch(monkeypatch):
    """predict() on 2 frames of 64x96 with Options.fuse_inc on (the default) and off: logits, theta and warp_mask equal; the
    fused launch really ran in the first and not in the second."""
    B, H, W = 2, 64, 96
    net = _model(B, H, W)
    x = synth.smooth_frames(B, H, W, seed=19).cuda()
    calls = _count_fused_calls(monkeypatch)
    outs, ncalls = {}, {}
    for sw in ("1", "0"):
        net.options = dataclasses.replace(net.options, fuse_inc=sw == "1")
        del calls[:]
        with torch.no_grad():
            outs[sw] = net.predict(x, consistency=True)
        torch.cuda.synchronize()
        ncalls[sw] = len(calls)
        assert net._get_engines()[0].options.fuse_inc == (sw == "1")
        assert net._get_engines()[0].fuse_inc == (sw == "1")
    assert ncalls["1"] >= 1 and ncalls["0"] == 0
    for k in ("logits", "theta", "warp_mask"):
        assert torch.equal(outs["1"][k], outs["0"][k]), k


def test_options_are_per_model_and_part_of_the_engine_stamp(monkeypatch):
    """Two models of one process with the same weights, one with fuse_inc = False: equal bits, the fused launch runs for one and
    not for the other.  Assigning another record to a model that has run - no invalidate_engines() - rebuilds its engines (the
    next predict() makes no fused call) and voids its captured graphs (predict_replay() captures anew, on the fused launch
    again once the option is back): always the same bits."""
    B, H, W = 2, 64, 96
    a, b = _model(B, H, W), _model(B, H, W)
    b.options = dataclasses.replace(b.options, fuse_inc=False)
    x = synth.smooth_frames(B, H, W, seed=19).cuda()
    calls = _count_fused_calls(monkeypatch)

    def run(net, how="predict"):
        del calls[:]
        with torch.no_grad():
            out = getattr(net, how)(x, consistency=True)
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in ("logits", "theta", "warp_mask")}, len(calls)

    def same(o, ref):
        return all(torch.equal(o[k], ref[k]) for k in ref)

    ref, na = run(a)
    ob, nb = run(b)
    assert na >= 1 and nb == 0 and same(ob, ref)
    assert a.options.fuse_inc and not b.options.fuse_inc          # neither model changed the other's record
    a.options = dataclasses.replace(a.options, fuse_inc=False)
    oa, na = run(a)
    assert na == 0 and same(oa, ref)
    # graph replay: the capture of one setting is never replayed under another
    a.options = dataclasses.replace(a.options, fuse_inc=True)
    a.graph_replay = True
    o1, n1 = run(a, "predict_replay")          # eager pass + capture: the fused launch is recorded
    o2, _ = run(a, "predict_replay")
    assert n1 >= 1 and same(o1, ref) and same(o2, ref)
    a.options = dataclasses.replace(a.options, fuse_inc=False)
    o3, n3 = run(a, "predict_replay")          # captures anew, without the fused launch
    assert n3 == 0 and same(o3, ref) and not a._get_engines()[0].fuse_inc
    a.options = dataclasses.replace(a.options, fuse_inc=True)
    o4, n4 = run(a, "predict_replay")          # and anew with it: run_inc_fused is counted again
    assert n4 >= 1 and same(o4, ref)
