"""The 7- and 8-class court models on the fused inference path: the 16-channel tap-packed stem instance, the OutConv head
fused behind the last conv for 6..8 classes, the fused nearest-warp + consistency kernel at 7 and 8 classes, and
predict() / forward() end to end in the default geometry (resnet_input='img+mask', no resize around the UNet).  Templates:
tests/golden/court_ids_ncaa_nc{7,8}_640x360.npz."""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402
from oracle import torch_ref, train_ref, warp_ref  # noqa: E402
from sfh_amd import synth  # noqa: E402

torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


@pytest.fixture(scope="module")
def E():
    from sfh_amd import engine, _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


def _maxerr(a, b):
    return (torch.as_tensor(a).float() - torch.as_tensor(b).float()).abs().max().item()


@functools.lru_cache(maxsize=None)
def _ids(nc):
    src = 7 if nc <= 7 else 8
    with np.load(os.path.join(GOLDEN, f"court_ids_ncaa_nc{src}_640x360.npz")) as z:
        return np.minimum(z["ids"], nc - 1)     # (6 classes: the 7-class template with its last id folded into the sixth)


def _template(nc, B, h=360, w=640):
    t = torch.from_numpy(_ids(nc)[:h, :w].astype(np.float32) / float(nc))
    return t[None, None].repeat(B, 1, 1, 1).contiguous()


# ------------------------------------------------------------------------------------------------ stem
def _stem_case(shape, cin):
    B, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + H + cin)
    conv = torch.nn.Conv2d(cin, 64, 7, stride=2, padding=3, bias=False)
    bn = torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        conv.weight.normal_(0, 0.1, generator=g)
        bn.weight.uniform_(0.5, 1.5, generator=g); bn.bias.uniform_(-0.3, 0.3, generator=g)
        bn.running_mean.uniform_(-0.2, 0.2, generator=g); bn.running_var.uniform_(0.5, 1.5, generator=g)
    bn.eval()
    x = torch.randn(B, cin, H, W, generator=g)
    with torch.no_grad():
        want = torch.relu(bn(conv(x.double().float()))).double()
        ref64 = torch.relu(torch.nn.functional.batch_norm(
            torch.nn.functional.conv2d(x.double(), conv.weight.double(), None, 2, 3), bn.running_mean.double(),
            bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps))
    return conv, bn, x, want, ref64


def _guarded_out(B, ho, wo):
    """(B,ho,wo,64) view filled with NaN, followed by a 64-float guard"""
    n = B * ho * wo * 64
    buf = torch.full((n + 64,), float("nan"), device="cuda")
    buf[n:] = 12345.0
    return buf, buf[:n].view(B, ho, wo, 64)


@pytest.mark.parametrize("fmt", ["s3", "h2"])
@pytest.mark.parametrize("shape", [(3, 45, 83), (1, 16, 16), (2, 23, 70), (1, 1, 1)])
@pytest.mark.parametrize("cin", [9, 10, 11, 12, 13, 16])
def test_wide_stem_kernel_vs_torch(E, shape, cin, fmt):
    """test_stem_kernel_vs_torch (tests/test_gpu_parity.py) for the 16-channel instance, its two bounds unchanged: 9..16 input
    channels at 12 / 16 stored, odd sizes, partial tiles, one pixel; every output written, nothing behind the last one, and
    the same bits from a second launch."""
    B, H, W = shape
    cs = -(-cin // 4) * 4
    conv, bn, x, want, ref64 = _stem_case(shape, cin)
    conv.cuda(); bn.cuda()
    st = E.StemConv(conv, bn, cin, fmt=fmt, cs=cs)
    assert st.cs == cs and E.StemConv(conv, bn, cin, fmt=fmt).cs == cs      # the default stored width is the engine's rule
    xin = E.nchw_to_nhwc(x.cuda(), cs)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    buf, out = _guarded_out(B, ho, wo)
    st.run(xin, B, H, W, out)
    buf2, out2 = _guarded_out(B, ho, wo)
    st.run(xin, B, H, W, out2)
    torch.cuda.synchronize()
    assert bool((buf[-64:] == 12345.0).all()) and not bool(torch.isnan(out).any())
    assert torch.equal(out, out2)
    got = out.permute(0, 3, 1, 2).cpu().double()
    e64, e32 = (got - ref64).abs().max().item(), (want - ref64).abs().max().item()
    print(f"stem cin={cin} {shape} {fmt}: |got - fp64| {e64:.3e}, torch fp32 {e32:.3e}")
    assert e64 < 3e-5 * max(1.0, ref64.abs().max().item())
    assert e64 < 4 * e32 + 1e-6   # fp32-grade accuracy


@pytest.mark.parametrize("fmt", ["s3", "h2"])
@pytest.mark.parametrize("cin", [10, 16])
def test_wide_stem_impulse_weights_copy_one_channel_exactly(E, cin, fmt):
    """A single 1 in the weight makes the raw conv output (StemConv without BatchNorm) the shifted, stride-2, zero-padded copy of
    one input channel - exactly: the inputs are integers of at most 8 bits, exact in bf16 and fp16.  Taps at the corners and
    the centre, channels on both sides of the channel-half boundary (7 | 8), first and last output channel: a weight packed
    into the wrong lane group, or a lane group reading the wrong channel half or tap, moves or zeroes the copy."""
    B, H, W = 2, 23, 38            # 12 x 19 outputs: two tile rows, two tile columns, both partial
    cs = -(-cin // 4) * 4
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pix = (torch.arange(H * W) % 8).reshape(1, 1, H, W)
    x = (torch.arange(cin).reshape(1, cin, 1, 1) + 16 * pix).float().repeat(B, 1, 1, 1)
    x[1] = x[1].flip(2)
    assert float(x.max()) <= 255
    xin = E.nchw_to_nhwc(x.cuda(), cs)
    xpad = torch.nn.functional.pad(x, (3, 3, 3, 3))
    conv = torch.nn.Conv2d(cin, 64, 7, stride=2, padding=3, bias=False).cuda()
    for ky, kx in ((0, 0), (3, 3), (6, 6), (0, 6), (6, 0)):
        for c in (0, 7, 8, cin - 1):
            for co in (0, 63):
                with torch.no_grad():
                    conv.weight.zero_()
                    conv.weight[co, c, ky, kx] = 1.0
                st = E.StemConv(conv, None, cin, fmt=fmt, cs=cs)
                out = torch.full((B, ho, wo, 64), float("nan"), device="cuda")
                st.run(xin, B, H, W, out)
                want = torch.zeros(B, ho, wo, 64)
                want[..., co] = xpad[:, c, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2]
                assert torch.equal(out.cpu(), want), (ky, kx, c, co)


def test_stem_refuses_other_stored_widths(E):
    """sfh_stem7x7_fwd: cs0 outside {8, 12, 16} and c0 > cs0 return -1 before anything is launched (the destination keeps
    its bytes); the pack entries refuse more channels than their instance holds"""
    from sfh_amd import _lib
    lib = _lib.load()
    conv = torch.nn.Conv2d(10, 64, 7, stride=2, padding=3, bias=False).cuda()
    st = E.StemConv(conv, None, 10, fmt="s3")
    x = torch.zeros(1, 16, 16, 16, device="cuda")
    out = torch.full((1, 8, 8, 64), float("nan"), device="cuda")
    for c0, cs0 in ((10, 10), (4, 4), (10, 20), (13, 12), (9, 8), (17, 16)):
        d = _lib.ConvDesc()
        d.src0, d.c0, d.cs0, d.h0, d.w0 = x.data_ptr(), c0, cs0, 16, 16
        d.batch, d.H, d.W, d.ksize, d.stride = 1, 16, 16, 7, 2
        d.wpacked, d.scale, d.shift = st.wpacked.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr()
        d.cout, d.relu = 64, 0
        d.dst, d.dst_cs, d.out_mode = out.data_ptr(), 64, _lib.OUT_NHWC
        d.src_fmt = d.dst_fmt = _lib.FMT_F32
        d.split_arith = _lib.FMT_S3
        assert lib.sfh_stem7x7_fwd(ctypes.byref(d), None) == -1, (c0, cs0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    w = conv.weight.detach()
    big = torch.empty(lib.sfh_packed_stem16_weight_bytes(), dtype=torch.uint8, device="cuda")
    assert lib.sfh_packed_stem16_weight_bytes() == 25 * 3 * 4 * 64 * 16
    assert lib.sfh_pack_stem_weights(w.data_ptr(), big.data_ptr(), 10, _lib.FMT_S3, 0, None) == -1
    assert lib.sfh_pack_stem16_weights(w.data_ptr(), big.data_ptr(), 17, _lib.FMT_S3, 0, None) == -1
    with pytest.raises(ValueError):
        E.StemConv(conv, None, 10, fmt="s3", cs=8)


# ------------------------------------------------------------------------------------------------ fused head
def _net(nc, wh, B, precision=None, seed=19, **kw):
    from sfh_amd.reconstructor import Reconstructor
    w, h = wh
    court = _template(nc, B, h, w)
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), mask_classes=nc, target_size=(w, h), unet_size=(w, h), warp_size=(w, h), **kw)
    sd = synth.synth_state_dict(net.state_dict(), seed)
    net.load_state_dict(sd)
    net.cuda().eval()
    if precision is not None:
        net.precision = precision
    return net, sd, court, poi


@functools.lru_cache(maxsize=None)
def _unet_reference(nc, wh, seed):
    w, h = wh
    from sfh_amd.reconstructor import Reconstructor
    net = Reconstructor(_template(nc, 2, h, w), synth.load_court_poi("pitch", 2), mask_classes=nc, target_size=wh,
                        unet_size=wh, warp_size=wh)
    sd = synth.synth_state_dict(net.state_dict(), seed)
    x = synth.smooth_frames(2, h, w, seed=seed)
    with torch.no_grad():
        return torch_ref.forward_unet(x, sd, wh, wh)[0]


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("nc", [6, 7, 8])
def test_fused_outconv_head_writes_twelve_channel_stn_rows(E, nc, precision):
    """test_fused_outconv_head_vs_outconv_kernel (tests/test_gpu_parity.py) for 6..8 classes, its bounds unchanged: the head
    fused behind the last conv against the separate OutConv kernel; STN rows of ceil4(nc + 3) = 12 floats, the frame
    channels bit-equal, the padding channels exactly zero - after a second run into the same workspace as well."""
    B, (W, H) = 2, (112, 90)
    x = synth.smooth_frames(B, H, W, seed=41)
    res = {}
    for flag in (True, False):
        net, sd, _, _ = _net(nc, (W, H), B, precision, seed=41)
        net.options = dataclasses.replace(net.options, fuse_head=flag)
        un, rn = net._get_engines()
        assert rn.cs_in == 12 and rn.stem7 is not None and rn.stem7.cs == 12
        with torch.no_grad():
            un.run(x.cuda().flip(0), want_stn_in=True)          # other frames first: the workspace is reused, not re-zeroed
            r = un.run(x.cuda(), want_stn_in=True)
            torch.cuda.synchronize()
        assert ("y4" in r) == (not flag)          # the 64-channel tensor is not stored when the head is fused
        assert tuple(r["stn_in"].shape) == (B, H, W, 12)
        res[flag] = (r["logits"].clone(), r["stn_in"].clone())
    lg, stn = res[True]
    assert _maxerr(lg.cpu(), res[False][0].cpu()) < 2e-5
    assert _maxerr(stn.cpu(), res[False][1].cpu()) < 2e-5
    assert torch.equal(stn[..., nc:nc + 3], res[False][1][..., nc:nc + 3])
    assert torch.equal(stn[..., nc:nc + 3], x.cuda().permute(0, 2, 3, 1))
    assert torch.equal(stn[..., :nc], lg.permute(0, 2, 3, 1))
    for flag in (True, False):
        assert float(res[flag][1][..., nc + 3:].abs().max()) == 0.0 and res[flag][1][..., nc + 3:].shape[-1] == 9 - nc
    assert _maxerr(lg.cpu(), _unet_reference(nc, (W, H), 41)) < 3e-4


# ------------------------------------------------------------------------------------------------ warp + consistency
def _thetas():
    """the fifteen homographies of the 4-class warp tests (identity, two realistic ones, perturbed, Z = 0, out of range)"""
    import test_gpu_parity
    return test_gpu_parity._thetas()


def _wide_template(nc, B, shared):
    tmpl = _template(nc, B)
    if not shared:
        tmpl[1::2] = torch.flip(tmpl[1::2], dims=[3])
    return tmpl


@functools.lru_cache(maxsize=None)
def _want_mask(nc, size, shared):
    """the oracle's nearest warp of the fixture template, once per (classes, size, template kind)"""
    w, h = size
    theta = _thetas()
    return (warp_ref.homography_warp(theta, _wide_template(nc, theta.shape[0], shared), h, w, "nearest") * nc).to(torch.int32)


@pytest.mark.parametrize("size", [(97, 61), (320, 45), (640, 360)])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("nc", [7, 8])
def test_warp_consistency_fused_kernel_wide(E, nc, size, shared):
    """test_warp_consistency_fused_kernel (tests/test_gpu_parity.py) at 7 and 8 classes with the wide court templates: mask
    bit-identical to the oracle's warp and to sfh_homography_warp_fwd's, score equal to torch's cross_entropy on that mask
    and to the separate CE kernel's, the same bits from a second launch."""
    w, h = size
    theta = _thetas()
    B = theta.shape[0]
    tmpl = _wide_template(nc, B, shared)
    g = synth._rng(11, f"wce{nc}_{w}x{h}")
    logits = torch.from_numpy(g.normal(0, 3, (B, nc, h, w)).astype(np.float32))
    want_mask = _want_mask(nc, size, shared)
    assert int(want_mask.max()) == nc - 1
    want = torch.nn.functional.cross_entropy(logits, want_mask.long(), reduction="none").mean(dim=(1, 2))
    lg, th, tm = logits.cuda(), theta.cuda(), tmpl.cuda()
    wm, score = E.warp_consistency(th, tm, lg, float(nc), shared_template=shared)
    _, wm2 = E.homography_warp(th, tm, h, w, True, scale=float(nc), want_f32=False, want_i32=True, shared_template=shared)
    sep = E.consistency_ce(lg, wm2)
    wm_b, score_b = E.warp_consistency(th, tm, lg, float(nc), shared_template=shared)
    torch.cuda.synchronize()
    assert torch.equal(wm.cpu(), want_mask) and torch.equal(wm, wm2)
    assert torch.equal(wm_b, wm) and torch.equal(score_b, score)
    assert _maxerr(score.cpu(), want) < 1e-5, _maxerr(score.cpu(), want)
    assert _maxerr(score, sep) < 1e-5


@pytest.mark.parametrize("size", [(194, 122), (640, 90)])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("nc", [7, 8])
def test_warp_consistency_fused_kernel_wide_with_a_warp_twice_the_logits_size(E, nc, size, shared):
    """test_warp_consistency_fused_kernel_with_a_warp_twice_the_logits_size at 7 and 8 classes: logit pixel (y, x) scores
    against mask pixel (2y, 2x)"""
    w, h = size
    theta = _thetas()
    B = theta.shape[0]
    tmpl = _wide_template(nc, B, shared)
    g = synth._rng(12, f"wce2_{nc}_{w}x{h}")
    logits = torch.from_numpy(g.normal(0, 3, (B, nc, h // 2, w // 2)).astype(np.float32))
    want_mask = _want_mask(nc, size, shared)
    m = torch.nn.functional.interpolate(want_mask.float().unsqueeze(1), size=(h // 2, w // 2), mode="nearest").squeeze(1).long()
    assert torch.equal(m, want_mask[:, ::2, ::2].long())
    want = torch.nn.functional.cross_entropy(logits, m, reduction="none").mean(dim=(1, 2))
    lg, th, tm = logits.cuda(), theta.cuda(), tmpl.cuda()
    wm, score = E.warp_consistency(th, tm, lg, float(nc), shared_template=shared, warp_hw=(h, w))
    _, wm2 = E.homography_warp(th, tm, h, w, True, scale=float(nc), want_f32=False, want_i32=True, shared_template=shared)
    sep = E.consistency_ce(lg, wm2)
    wm_b, score_b = E.warp_consistency(th, tm, lg, float(nc), shared_template=shared, warp_hw=(h, w))
    torch.cuda.synchronize()
    assert torch.equal(wm.cpu(), want_mask) and torch.equal(wm, wm2)
    assert torch.equal(wm_b, wm) and torch.equal(score_b, score)
    assert _maxerr(score.cpu(), want) < 1e-5 and _maxerr(score, sep) < 1e-5


def test_warp_consistency_still_refuses_five_classes(E):
    theta = _thetas()[:2].cuda()
    tmpl = _template(7, 2).cuda()
    with pytest.raises(ValueError, match="built for 4 classes"):
        E.warp_consistency(theta, tmpl, torch.zeros(2, 5, 45, 64, device="cuda"), 5.0, shared_template=True)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _predict_reference(nc, wh, seed=19):
    w, h = wh
    from sfh_amd.reconstructor import Reconstructor
    court, poi = _template(nc, 2, h, w), synth.load_court_poi("pitch", 2)
    net = Reconstructor(court, poi, mask_classes=nc, target_size=wh, unet_size=wh, warp_size=wh, warp_with_nearest=True)
    sd = synth.synth_state_dict(net.state_dict(), seed)
    x = synth.smooth_frames(2, h, w, seed=seed)
    with torch.no_grad():
        return torch_ref.predict(x, sd, court, poi, mask_classes=nc, warp_size=wh, unet_size=wh, target_size=wh,
                                 project_poi=True)


def _check_predict(E, nc, wh, precision, replay_and_forward=True):
    from sfh_amd import outputs
    w, h = wh
    net, sd, court, poi = _net(nc, wh, 2, precision, warp_with_nearest=True)
    x = synth.smooth_frames(2, h, w, seed=19).cuda()
    calls = []
    real = E.warp_consistency
    E.warp_consistency = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad():
            out = net.predict(x, consistency=True, project_poi=True)        # the parent: NotImplementedError here
            assert len(calls) == 1
            net.fuse_warp_ce = False
            sep = net.predict(x, consistency=True, project_poi=True)
            net.fuse_warp_ce = True
            assert len(calls) == 1
    finally:
        E.warp_consistency = real
    torch.cuda.synchronize()
    want = _predict_reference(nc, wh)
    dth, dlg = _maxerr(out["theta"].cpu(), want["theta"]), _maxerr(out["logits"].cpu(), want["logits"])
    dpo, dcs = _maxerr(out["poi"].cpu(), want["poi"]), _maxerr(out["consist_score"].cpu(), want["consist_score"])
    print(f"predict nc={nc} {wh} {precision}: dtheta {dth:.2e} dlogits {dlg:.2e} dpoi {dpo:.2e} dscore {dcs:.2e}")
    assert dth < 1e-4 and dlg < 5e-4 and dpo < 1e-4 and dcs < 2e-4
    assert sorted(out) == sorted(sep)
    assert torch.equal(out["warp_mask"], sep["warp_mask"]) and torch.equal(out["theta"], sep["theta"])
    assert _maxerr(out["consist_score"], sep["consist_score"]) < 1e-5
    assert out["warp_mask"].dtype == torch.int32 and tuple(out["logits"].shape) == (2, nc, h, w)
    wm = (warp_ref.homography_warp(out["theta"].cpu(), court, h, w, "nearest") * nc).to(torch.int32)
    assert torch.equal(out["warp_mask"].cpu(), wm)
    # the argmax mask: the reference's rule (argmax of softmax) on the same logits wherever the two rules cannot differ, and
    # the reference's own mask wherever its top-2 margin exceeds twice the logit bound
    mask = torch.as_tensor(outputs.preds_to_masks(out["logits"], n_classes=nc)).cpu().long()
    lg = out["logits"].cpu()
    sure = ~torch_ref.softmax_argmax_may_differ(lg)
    assert torch.equal(mask[sure], torch.softmax(lg, 1).argmax(1)[sure])
    top2 = want["logits"].topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(mask[safe], want["logits"].argmax(1)[safe]) and int(mask.max()) <= nc - 1
    if not replay_and_forward:
        return
    with torch.no_grad():
        rep = [net.predict_replay(x, consistency=True, project_poi=True) for _ in range(3)]     # eager, capture, replay
        fwd = net(x)
    torch.cuda.synchronize()
    for r in rep:
        assert sorted(r) == sorted(out) and all(torch.equal(r[k], out[k]) for k in out)
    assert torch.equal(fwd["theta"], out["theta"]) and torch.equal(fwd["logits"], out["logits"])


@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("nc", [7, 8])
def test_predict_with_seven_and_eight_classes(E, nc, precision):
    """predict(consistency=True, project_poi=True) in the default geometry against the oracle with mask_classes = nc; one
    fused warp + consistency launch per call; HIP-graph replay returns the same bytes; eval-mode forward() the same theta."""
    _check_predict(E, nc, (112, 90), precision)


def test_predict_with_eight_classes_full_size(E):
    _check_predict(E, 8, (640, 360), "f16x3", replay_and_forward=False)


# ------------------------------------------------------------------------------------------------ training
def _stage(k):
    p = k.split(".")
    if p[0] != "resnet_reg":
        return p[0]
    return "resnet_reg." + (p[1] if p[1].startswith("layer") or p[1] == "reg" else "stem")


def test_training_forward_backward_with_seven_classes_vs_fp64():
    """One training-mode forward + backward at 7 classes (72x128, two frames) against autograd over the oracle in fp64, with
    the oracle's own fp32 run as the yardstick - the bounds of test_c3_training_step_640x360_vs_fp64_reference
    (tests/test_gpu_configs.py): theta 1e-4; logits 3x the fp32 run's error + 2e-5; losses 3x the fp32 run's + 2e-5 (1e-3
    for the consistency term); every parameter gradient within 4x the larger of its own fp32 error and the upper quartile
    of its stage's, + 1e-5."""
    from sfh_amd.reconstructor import Reconstructor
    nc, B, H, W = 7, 2, 72, 128
    court, poi = _template(nc, B, H, W), synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), mask_classes=nc, target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    sd = synth.synth_state_dict(net.state_dict(), 47)
    net.load_state_dict(sd)
    x = synth.frames_to_float(synth.synth_frames_u8(B, H, W, seed=47))
    g = torch.Generator().manual_seed(47)
    batch = {"mask": torch.randint(0, nc, (B, H, W), generator=g), "weight": torch.rand(B, generator=g) + 0.5,
             "poi": torch.rand(B, poi.shape[1], 2, generator=g),
             "nonzeros": (torch.rand(B, poi.shape[1], generator=g) > 0.3).float()}
    batch["num_nonzero"] = batch["nonzeros"].sum(1).clamp(min=1.0)
    runs = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        ref = train_ref.leaf_state({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()})
        pr = train_ref.forward_train(x.to(dt), ref, court.to(dt), poi.to(dt), warp_size=(W, H), unet_size=(W, H),
                                     target_size=(W, H))
        ls = train_ref.losses(pr, {k: (v.to(dt) if v.is_floating_point() else v) for k, v in batch.items()}, mask_classes=nc)
        ls["total"].backward()
        runs[tag] = (pr, {k: float(v.detach()) for k, v in ls.items()},
                     {k: v.grad.detach().double() for k, v in ref.items() if v.requires_grad})
    net.cuda().train()
    preds = net(x.cuda())
    loss = train_ref.losses(preds, {k: v.cuda() for k, v in batch.items()}, mask_classes=nc)
    loss["total"].backward()
    torch.cuda.synchronize()
    p32, l32, g32 = runs["f32"]
    p64, l64, g64 = runs["f64"]
    assert _maxerr(preds["theta"].detach().cpu().double(), p64["theta"].detach()) < 1e-4
    dl = float((preds["logits"].detach().cpu().double() - p64["logits"].detach()).abs().max())
    dl32 = float((p32["logits"].detach().double() - p64["logits"].detach()).abs().max())
    print(f"train nc=7: dlogits {dl:.3e} (fp32 oracle {dl32:.3e})")
    assert dl < 3.0 * dl32 + 2e-5, (dl, dl32)
    for k in ("seg", "rec", "reproj", "consist", "total"):
        got = float(loss[k].detach())
        tol = 3.0 * abs(l32[k] - l64[k]) + (1e-3 if k in ("consist", "total") else 2e-5) * max(1.0, abs(l64[k]))
        print(f"train nc=7: loss {k} {got:.6f} fp32 {l32[k]:.6f} fp64 {l64[k]:.6f}")
        assert abs(got - l64[k]) < tol, (k, got, l32[k], l64[k])
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(g64)
    e32, rows = {}, []
    for k, w64 in g64.items():
        n64 = float(w64.norm())
        if n64 < 1e-9:          # conv bias in front of BatchNorm: the exact gradient is zero
            assert float(params[k].grad.abs().max()) < 1e-6, k
            continue
        e32[k] = float((g32[k] - w64).norm()) / n64
        rows.append((k, float((params[k].grad.detach().cpu().double() - w64).norm()) / n64))
    by_stage = {}
    for k, e in e32.items():
        by_stage.setdefault(_stage(k), []).append(e)
    q75 = {s: float(np.quantile(v, 0.75)) for s, v in by_stage.items()}
    worst = [(k, e, e32[k], q75[_stage(k)]) for k, e in rows if e > 4.0 * max(e32[k], q75[_stage(k)]) + 1e-5]
    print(f"train nc=7: {len(rows)} gradients, median error {np.median([e for _, e in rows]):.3e}, "
          f"fp32 oracle median {np.median(list(e32.values())):.3e}, over the bound: {worst}")
    assert len(rows) > 150 and not worst, worst
