"""The grouped 3x3 convolution (csrc/conv_grouped.hip) on the GPU: the three kernels through the raw C entry points on every
case of tests/grouped_conv_cases.py against the fp64 references and bounds of tests/grouped_conv_ref.py; the ResNeXt depths
through ResNetEngine, Reconstructor.predict (eager and graph replay), conv_bn_act and train_forward.

The training-mode checks have no fixed tolerance (BatchNorm over a handful of pixels amplifies by invstd): their yardstick is
the dense sibling - the identical test code on groups = 1 (a plain Bottleneck block; resnet50) in the same process.  Per
tensor e = max |got - ref| / max |ref|, and e_grouped <= 2 * e_dense + 2^-20 is demanded.  Measured on an MI355X: the block
(y, dx, 9 - 11 gradients, both strides, three precisions) 3e-8 .. 9.2e-7 grouped against 3e-8 .. 9.1e-7 dense; the whole
regressor: _train_forward_errors' docstring."""
import ctypes
import os

import numpy as np
import pytest
import torch

import grouped_conv_cases as K
import grouped_conv_ref as R
from conftest import GOLDEN
from oracle import torch_ref, warp_ref
from sfh_amd import modules, synth
from train_kernel_ref import ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from sfh_amd import _lib, engine
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine


@pytest.fixture(scope="module")
def lib():
    from sfh_amd import _lib
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() if a is not None else None


class _Out:
    """an output buffer of n floats that starts as NaN (or as `init`) and ends in a 64-float guard of NaN"""

    def __init__(self, shape, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + K.GUARD,), float("nan"), device="cuda")
        if init is not None:
            self.buf[:self.n] = _dev(init).reshape(-1)

    def numpy(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[self.n:]).all()), "the guard behind the output was written"
        return self.buf[:self.n].cpu().numpy().reshape(self.shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())


def _pack(lib, w, G, cg, mode):
    n = lib.sfh_packed_grouped_weight_floats(G, cg)
    assert n > 0
    packed = torch.full((n,), float("nan"), device="cuda")
    assert lib.sfh_pack_grouped_weights(_p(w), _p(packed), G, cg, mode, _st()) == 0
    return packed


def _forward(lib, case, x, w, scale=None, shift=None, relu=False):
    B, H, W, G, cg, s = case
    out = _Out((B,) + K.out_hw(case) + (G * cg,))
    assert lib.sfh_conv_grouped_fwd(_p(x), _p(_pack(lib, w, G, cg, 0)), _p(scale), _p(shift), int(relu), _p(out.buf), B, H, W,
                                    G, cg, s, _st()) == 0, lib.sfh_last_error()
    return out


def _backward_data(lib, case, dz, w):
    """as the library does it: stride 2 through sfh_zero_stuff2, then the stride-1 kernel over the mode-1 weights"""
    B, H, W, G, cg, s = case
    C, (ho, wo) = G * cg, K.out_hw(case)
    if s == 2:
        up = torch.full((B, H, W, C), float("nan"), device="cuda")
        assert lib.sfh_zero_stuff2(_p(dz), _p(up), B, ho, wo, H, W, C, _st()) == 0
        dz = up
    out = _Out((B, H, W, C))
    assert lib.sfh_conv_grouped_fwd(_p(dz), _p(_pack(lib, w, G, cg, 1)), None, None, 0, _p(out.buf), B, H, W, G, cg, 1,
                                    _st()) == 0, lib.sfh_last_error()
    return out


def _wgrad(lib, case, dz, x, raw0):
    B, H, W, G, cg, s = case
    out = _Out((G * cg, 9, cg), init=raw0)
    assert lib.sfh_conv_grouped_wgrad(_p(dz), _p(x), _p(out.buf), B, H, W, G, cg, s, _st()) == 0, lib.sfh_last_error()
    return out


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_kernels_on_every_case(lib, case):
    """integers: the fp64 value bit for bit; randn: inside the bound, with and without the epilogue; two forward calls give
    the same bits; guards intact"""
    B, H, W, G, cg, s = case
    x, w, dz, raw0 = K.int_inputs(case)
    xd, wd, dzd = _dev(x), _dev(w), _dev(dz)
    assert np.array_equal(_forward(lib, case, xd, wd).numpy().astype(np.float64), R.conv(x, w, s)[0])
    assert np.array_equal(_backward_data(lib, case, dzd, wd).numpy().astype(np.float64), R.bwd_data(dz, w, s, H, W)[0])
    raw = _wgrad(lib, case, dzd, xd, raw0).numpy()
    assert np.array_equal(R.raw_to_oihw(raw, cg).astype(np.float64), R.wgrad(dz, x, cg, s)[0] + R.raw_to_oihw(raw0, cg))

    x, w, dz, raw0 = K.randn_inputs(case)
    xd, wd, dzd = _dev(x), _dev(w), _dev(dz)
    acc, A = R.conv(x, w, s)
    y = _forward(lib, case, xd, wd).numpy()
    worst = {"forward": ratio(y, acc, R.conv_bound(A, cg))}
    assert np.array_equal(y.view(np.uint32), _forward(lib, case, xd, wd).numpy().view(np.uint32))
    ref, Ad = R.bwd_data(dz, w, s, H, W)
    worst["backward-data"] = ratio(_backward_data(lib, case, dzd, wd).numpy(), ref, R.conv_bound(Ad, cg))
    dw, Aw = R.wgrad(dz, x, cg, s)
    r0 = R.raw_to_oihw(raw0, cg).astype(np.float64)
    worst["backward-filter"] = ratio(R.raw_to_oihw(_wgrad(lib, case, dzd, xd, raw0).numpy(), cg), dw + r0,
                                     R.wgrad_bound(Aw, r0, *K.wgrad_plan(case)))
    scale, shift = K.epilogue_inputs(case, acc)
    want, bound = R.epilogue(acc, A, cg, scale, shift, True)
    y = _forward(lib, case, xd, wd, _dev(scale), _dev(shift), relu=True).numpy()
    worst["epilogue"] = ratio(y, want, bound)
    assert np.array_equal(y[..., 1], np.full_like(y[..., 1], 0.25))       # the scale = 0 channel: the shift alone
    want, bound = R.epilogue(acc, A, cg, scale, shift, False)
    worst["epilogue, no ReLU"] = ratio(_forward(lib, case, xd, wd, _dev(scale), _dev(shift)).numpy(), want, bound)
    print(K.case_id(case), "largest error / bound:", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", K.IMPULSE, ids=K.case_id)
def test_impulses(lib, case):
    """a single 1 in the weight: exactly one shifted, zero-padded source channel in one destination channel - a wrong group,
    tap flip or padding side is a wrong integer"""
    B, H, W, G, cg, s = case
    C, (ho, wo) = G * cg, K.out_hw(case)
    src, dz = K.impulse_source((B, H, W, C)), K.impulse_source((B, ho, wo, C))
    sd, dzd = _dev(src), _dev(dz)
    for w, g, o, c, ky, kx in K.impulse_weights(case):
        wd = _dev(w)
        assert np.array_equal(_forward(lib, case, sd, wd).numpy(), R.shifted_copy(src, g * cg + c, g * cg + o, ky, kx, s)), \
            (g, o, c, ky, kx)
        assert np.array_equal(_backward_data(lib, case, dzd, wd).numpy(),
                              R.scattered_copy(dz, g * cg + o, g * cg + c, ky, kx, s, H, W)), (g, o, c, ky, kx)


def test_refused_geometry_launches_nothing(lib):
    x = torch.zeros(2 * 7 * 5 * 256, device="cuda")
    wp = torch.zeros(1 << 20, device="cuda")
    for (G, cg, s, B, H, W) in ((4, 3, 1, 2, 7, 5), (4, 12, 1, 2, 7, 5), (1, 128, 1, 1, 7, 5), (4, 0, 1, 2, 7, 5),
                                (4, 8, 3, 2, 7, 5), (4, 8, 0, 2, 7, 5), (0, 8, 1, 2, 7, 5), (4, 8, 1, 0, 7, 5),
                                (4, 8, 1, 2, 0, 5), (4, 8, 2, 2, 7, 0)):
        out = _Out((2, 7, 5, 64))
        assert lib.sfh_conv_grouped_fwd(_p(x), _p(wp), None, None, 0, _p(out.buf), B, H, W, G, cg, s, _st()) == -1
        assert out.untouched()
        assert lib.sfh_conv_grouped_wgrad(_p(x), _p(x), _p(out.buf), B, H, W, G, cg, s, _st()) == -1
        assert out.untouched()
    out = _Out((64,))
    assert lib.sfh_conv_grouped_fwd(_p(x), _p(wp), _p(x), None, 0, _p(out.buf), 2, 7, 5, 4, 8, 1, _st()) == -1   # scale alone
    assert lib.sfh_pack_grouped_weights(_p(x), _p(out.buf), 4, 5, 0, _st()) == -1
    assert lib.sfh_pack_grouped_weights(_p(x), _p(out.buf), 4, 8, 2, _st()) == -1
    assert out.untouched()
    assert lib.sfh_packed_grouped_weight_floats(4, 5) == -1 and lib.sfh_packed_grouped_weight_floats(0, 8) == -1
    assert lib.sfh_packed_grouped_weight_floats(3, 4) == 9 * 4 * 32
    assert lib.sfh_packed_grouped_weight_floats(32, 64) == 32 * 9 * 64 * 64


@pytest.mark.parametrize("case", K.DENSE, ids=K.case_id)
def test_one_group_is_the_dense_conv(E, lib, case):
    """G = 1, cg = 64 is a dense 64 -> 64 conv: the grouped kernel and PackedConv in fp32 mode each lie inside their own
    bound of the fp64 value (both are K-term fp32 sums: the same bound)"""
    B, H, W, G, cg, s = case
    x, w, _, _ = K.randn_inputs(case)
    acc, A = R.conv(x, w, s)
    xd, wd = _dev(x), _dev(w)
    grouped = _forward(lib, case, xd, wd).numpy()
    dense = torch.empty((B,) + K.out_hw(case) + (64,), device="cuda")
    E.PackedConv(wd, None, None, 3, 64, relu=False, stride=s, shared_unit_scale=True).run(xd, B, H, W, dense)
    torch.cuda.synchronize()
    r = (ratio(grouped, acc, R.conv_bound(A, cg)), ratio(dense.cpu().numpy(), acc, R.conv_bound(A, cg)))
    print(K.case_id(case), "grouped / PackedConv error over bound:", r)
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------------------------------------ the engine
_SEEDS = {"resnext50_32x4d": 21, "resnext101_32x8d": 22}
_STATE = {}


def _stn(name):
    """(ResNetSTN on the GPU in eval mode, its synthetic state dict), built once per name"""
    if name not in _STATE:
        rn = modules.ResNetSTN(name, 7)
        sd = synth.synth_state_dict(rn.state_dict(), _SEEDS[name])
        rn.load_state_dict(sd)
        _STATE[name] = (rn.cuda().eval(), sd)
    return _STATE[name]


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "fp32"])
@pytest.mark.parametrize("name", sorted(_SEEDS))
def test_resnext_stn_golden(E, golden_blocks, name, precision):
    """ResNetEngine on the fixture made with the reference's own class, with the rescale loop of test_resnet_stn_golden"""
    rn, _ = _stn(name)
    want = np.load(os.path.join(GOLDEN, "resnext_stn.npz"))[name + "_7.theta"]
    x = torch.from_numpy(golden_blocks["resnet34_7.x"])
    rg = E.H2Ranges(torch.device("cuda")) if precision == "f16x3" else None
    eng = E.ResNetEngine(rn, 7, torch.device("cuda"), precision, ranges=rg)
    assert sum(isinstance(v, E.GroupedConv) for v in eng.L.values()) == len(eng.blocks)
    theta = eng.run(E.nchw_to_nhwc(x.cuda(), 8), 2, 72, 128)
    torch.cuda.synchronize()
    rescales = 0
    while rg is not None:
        bits = rg.read()
        bad, nonfinite = rg.saturated(bits)
        assert not nonfinite
        if not bad:
            break
        rg.reset_words()
        theta = eng.rerun(eng.first_step(rg.lower(bad, bits)))
        rescales += 1
        assert rescales < 40
    assert float(np.abs(theta.cpu().numpy() - want).max()) < 1e-4
    if rg is not None:
        assert min(rg.headroom().values()) >= 1.0 and len(rg.peak) > 10
        assert any(n.endswith(".t2") for n in rg.peak)          # the grouped layers' outputs keep their range words


def test_predict_resnext50(E):
    """Reconstructor(resnet_name='resnext50_32x4d') end to end at the size of test_predict_resnet50_variant, eager and
    through graph replay"""
    from sfh_amd.reconstructor import Reconstructor
    B = 2
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :90, :112].contiguous()
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(112, 90), unet_size=(112, 90), warp_size=(112, 90),
                        warp_with_nearest=True, resnet_name="resnext50_32x4d")
    sd = synth.synth_state_dict(net.state_dict(), 31)
    net.load_state_dict(sd)
    net.cuda().eval()
    x = synth.smooth_frames(B, 90, 112, seed=31)
    with torch.no_grad():
        out = {k: v.clone() for k, v in net.predict(x.cuda(), consistency=False).items()}
        logits, _, _ = torch_ref.forward_unet(x, sd, (112, 90), (112, 90))
        theta = R.resnet_stn(torch.cat((logits, x), 1), sd)
    assert float((out["theta"].cpu() - theta).abs().max()) < 1e-4
    wm = (warp_ref.homography_warp(out["theta"].cpu(), court, 90, 112, "nearest") * 4)
    assert torch.equal(out["warp_mask"].cpu(), wm.to(torch.int32))
    net.graph_replay = True
    with torch.no_grad():
        for _ in range(2):      # the capture, then a replay
            via = net.predict(x.cuda(), consistency=False)
            assert sorted(via) == sorted(out) and all(torch.equal(via[k], out[k]) for k in out)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ training
class _Holder(torch.nn.Module):
    def __init__(self, b):
        super().__init__()
        self.b = b


def _e(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max())


def _block_errors(T, groups, base_width, stride):
    """one Bottleneck block (planes 64, B = 2, 9 x 11) in training mode through conv_bn_act, as ResNetTrainer chains it,
    against fp64 autograd of the restatement -> {tensor: e}"""
    B, H, W, cin = 2, 9, 11, 256
    g = torch.Generator().manual_seed(77 + stride)
    down = None
    if stride == 2:
        down = torch.nn.Sequential(torch.nn.Conv2d(cin, 256, 1, stride=2, bias=False), torch.nn.BatchNorm2d(256))
    holder = _Holder(modules.Bottleneck(cin, 64, stride, down, groups=groups, base_width=base_width))
    with torch.no_grad():
        for m in holder.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, (2.0 / (m.weight.shape[1] * m.weight[0, 0].numel())) ** 0.5, generator=g)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.uniform_(-0.3, 0.3, generator=g)
    x = torch.randn(B, cin, H, W, generator=g)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(B, 256, ho, wo, generator=g)
    ref = {k: v.double().requires_grad_(v.dim() > 0 and v.dtype.is_floating_point and "running" not in k)
           for k, v in holder.state_dict().items()}
    xr = x.double().requires_grad_(True)
    yr = R.bottleneck(xr, ref, "b", stride, training=True)
    yr.backward(dy.double())

    holder.cuda().train()
    blk, names, tape = holder.b, T._Names(holder), T.Tape()
    xs = x.permute(0, 2, 3, 1).contiguous().cuda()

    def cba(conv, bn, src, hh, ww, relu=True, residual=None):
        return T.conv_bn_act(tape, names, conv, bn, [(src, src.shape[3], 0, 0)], B, hh, ww, relu=relu, residual=residual)
    idn = cba(blk.downsample[0], blk.downsample[1], xs, H, W, relu=False) if down is not None else xs
    t = cba(blk.conv1, blk.bn1, xs, H, W)
    t = cba(blk.conv2, blk.bn2, t, H, W)
    y = cba(blk.conv3, blk.bn3, t, ho, wo, residual=idn)
    tape.add_grad(y, dy.permute(0, 2, 3, 1).contiguous().cuda())
    tape.backward()
    torch.cuda.synchronize()
    errs = {"y": _e(y.f32.permute(0, 3, 1, 2), yr), "dx": _e(tape.pop_grad(xs).permute(0, 3, 1, 2), xr.grad)}
    for k, p in ref.items():
        if p.requires_grad:
            errs[k] = _e(tape.param_grads[k], p.grad)
    return errs


def _demand(grouped, dense):
    """e_grouped <= 2 * e_dense + 2^-20 per tensor; prints both columns"""
    assert sorted(grouped) == sorted(dense)
    for k in grouped:
        print(f"  {k:32s} grouped {grouped[k]:.3e}   dense {dense[k]:.3e}")
    bad = {k: (grouped[k], dense[k]) for k in grouped if not grouped[k] <= 2 * dense[k] + 2.0 ** -20}
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6", "fp32"])
@pytest.mark.parametrize("stride", [1, 2])
def test_grouped_bottleneck_block_in_training_mode(stride, prec, monkeypatch):
    """y, dx, the three conv gradients and the BatchNorm gradients of a grouped block (32 groups of 4) against the dense
    block (planes 64) under the identical code"""
    from sfh_amd import training as T
    monkeypatch.setenv("SFH_TRAIN_PRECISION", prec)
    print(f"block, stride {stride}, {prec}:")
    _demand(_block_errors(T, 32, 4, stride), _block_errors(T, 1, 64, stride))


def _train_forward_errors(name):
    """train_forward on the STN alone (2 x 3 x 72 x 128), loss = a fixed random projection of theta and poi: theta, poi and
    every parameter gradient against fp64 autograd of the restatement -> ({tensor: e}, the same against the reference under
    its own ReLU decisions).

    The reference takes the ReLU decisions of the pass under test (training.CAPTURE: the stem's and every block's three
    activations), as test_gpu_configs.py does for the last stage.  Why: of the 3 million ReLU inputs of such a pass a handful
    lie within 2e-6 of zero in the fp64 reference itself; with these weights resnext50_32x4d has one at 1.5e-8
    (layer3.0.bn1), which torch's own CPU fp32 pass decides the other way too.  A flipped decision moves the output by
    1e-8 and toggles that element's whole gradient - 4.3e-3 of layer3.0.conv1.weight's largest element, 1e-4 .. 5e-4 of
    everything upstream, against 3e-6 .. 9e-6 where no decision differs.  That is a property of ReLU
    (test_conv_bn_act_backward), not of a kernel: under equal decisions the two gradients differ by rounding alone, and the
    dense sibling is held to the same reference."""
    from sfh_amd import training
    from sfh_amd.reconstructor import Reconstructor
    B, H, W = 2, 72, 128
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(None, poi.cuda(), use_unet=False, use_warper=False, resnet_input="img", resnet_name=name,
                        target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    sd = synth.synth_state_dict(net.state_dict(), 33)
    net.load_state_dict(sd)
    x = synth.smooth_frames(B, H, W, seed=33)
    g = torch.Generator().manual_seed(5)
    p_theta, p_poi = torch.randn(B, 1, 3, 3, generator=g), torch.randn(poi.shape, generator=g)

    net.cuda().train()
    cap = training.CAPTURE = {}
    try:
        preds = net(x.cuda())
        ((preds["theta"] * p_theta.cuda()).sum() + (preds["poi"] * p_poi.cuda()).sum()).backward()
    finally:
        training.CAPTURE = None
    torch.cuda.synchronize()
    open_ = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()
    masks = {"resnet_reg.stem": open_(cap["stem"])}
    for k, v in cap.items():
        if k.startswith("layer"):
            masks.update({f"resnet_reg.{k}.{a}": open_(v[a]) for a in ("t1", "t", "out")})

    def against(masks):
        ref = {k: v.double().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
        theta = R.resnet_stn(x.double(), ref, training=True, masks=masks)
        proj = R.transform_poi(theta, poi.double())
        ((theta * p_theta.double()).sum() + (proj * p_poi.double()).sum()).backward()
        errs = {"theta": _e(preds["theta"], theta), "poi": _e(preds["poi"], proj)}
        errs.update({k: _e(p.grad, ref[k].grad) for k, p in net.named_parameters()})
        return errs
    return against(masks), against(None)


def test_train_forward_resnext50_against_resnet50():
    (grouped, g_own), (dense, d_own) = _train_forward_errors("resnext50_32x4d"), _train_forward_errors("resnet50")
    print("largest e against the reference under its OWN ReLU decisions (not demanded): grouped %.3e (%s), dense %.3e (%s)"
          % (max(g_own.values()), max(g_own, key=g_own.get), max(d_own.values()), max(d_own, key=d_own.get)))
    _demand(grouped, dense)
