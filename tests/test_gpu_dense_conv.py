"""The dense convolution launches on the GPU, one launch per check, through the raw C entry points with a hand-filled
sfh_conv_desc: sfh_conv_fwd, sfh_conv_s3_fwd (S3 and H2 sources), sfh_conv_small_fwd, the same kernels as backward-data
(pack modes 1, 3, 4), sfh_conv_wgrad and sfh_conv_wgrad_s3 - on every case of tests/dense_conv_cases.py against the fp64
values and bounds of tests/dense_conv_ref.py.  Weights are packed by the library's pack entry points, split tensors come
from sfh_f32_to_s3 / sfh_f32_to_h2; the expected values come from the reference only.  Every comparison is per element:
bit equality, or a bound built from the reference's absolute sums.  Outputs start as NaN (accumulated ones non-zero) and
end in a guard that must keep its bytes."""
import ctypes

import numpy as np
import pytest
import torch

import dense_conv_cases as K
import dense_conv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1       # a NaN in bf16 and in fp16: what split outputs start as
NP = {"s3": 3, "h2": 2}
FMT = {"f32": 0, "s3": 1, "h2": 2}
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from sfh_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield lib
    for k in sorted(WORST):       # the largest error / bound per kernel over whatever part of the file ran
        print(f"WORST {k}: {WORST[k]:.3f}")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _a(t):
    return t.data_ptr() if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() if a is not None else None


def _sync():
    """a HIP error ends the run: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"GPU error, stopping: {err}", 3)


def _report(name, **ratios):
    for k, v in ratios.items():
        WORST[k.split(":")[0]] = max(WORST.get(k.split(":")[0], 0.0), v)
    print(f"RATIO {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (name, ratios)


class _F32Out:
    """(shape) floats that start as NaN (or as `init`) and end in a guard of NaN"""

    def __init__(self, shape, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + K.GUARD,), float("nan"), device="cuda")
        if init is not None:
            self.buf[:self.n] = _dev(init).reshape(-1)

    def ptr(self):
        return self.buf.data_ptr()

    def numpy(self):
        _sync()
        assert bool(torch.isnan(self.buf[self.n:]).all()), "the guard behind the output was written"
        return self.buf[:self.n].cpu().numpy().reshape(self.shape)

    def untouched(self):
        _sync()
        return bool((self.buf.view(torch.int32) == 0x7FC00000).all())


class _SplitOut:
    """a split tensor (B,H,cs/32,planes,4,W,8) of 16-bit words that start as SENTINEL and end in a guard of it"""

    def __init__(self, lib, fmt, B, H, W, cs, exp):
        self.lib, self.fmt, self.dims, self.exp = lib, fmt, (B, H, W, cs), exp
        self.n = B * H * W * cs * NP[fmt]
        self.buf = torch.full((self.n + K.GUARD,), SENTINEL, dtype=torch.int16, device="cuda")

    def ptr(self):
        return self.buf.data_ptr()

    def numpy(self, cout):
        """-> (B,H,W,cout) float32 through the library's inverse conversion; blocks beyond cout must keep their words"""
        B, H, W, cs = self.dims
        _sync()
        assert bool((self.buf[self.n:] == SENTINEL).all()), "the guard behind the output was written"
        planes = self.buf[:self.n].view(B, H, cs // 32, NP[self.fmt], 4, W, 8)
        assert bool((planes[:, :, cout // 32:] == SENTINEL).all()), "stored channels behind cout were written"
        out = torch.empty((B, H, W, cs), device="cuda")
        if self.fmt == "s3":
            assert self.lib.sfh_s3_to_f32(_p(self.buf), _p(out), B * H, W, cs, _st()) == 0
        else:
            assert self.lib.sfh_h2_to_f32(_p(self.buf), _p(out), B * H, W, cs, self.exp, _st()) == 0
        _sync()
        return out[..., :cout].cpu().numpy()

    def untouched(self):
        _sync()
        return bool((self.buf == SENTINEL).all())


def _split(lib, x, fmt, exp):
    """fp32 NHWC device tensor -> the split tensor of the library's own conversion"""
    B, H, W, cs = x.shape
    out = torch.full((B * H * W * cs * NP[fmt],), SENTINEL, dtype=torch.int16, device="cuda")
    if fmt == "s3":
        assert lib.sfh_f32_to_s3(_p(x), _p(out), B * H, W, cs, _st()) == 0, lib.sfh_last_error()
    else:
        assert lib.sfh_f32_to_h2(_p(x), _p(out), B * H, W, cs, exp, None, None, _st()) == 0, lib.sfh_last_error()
    return out


def _pack(lib, case, w):
    """-> (packed weights, the power of two the accumulator has to be multiplied with)"""
    ar, wd = K.arith(case), _dev(w)
    args = (case.ks, case.c0, case.c1, case.cout)
    if ar == "f32":
        n = lib.sfh_packed_weight_floats(*args)
        assert n > 0
        packed = torch.full((n,), float("nan"), device="cuda")
        assert lib.sfh_pack_conv_weights(_p(wd), _p(packed), *args, case.mode, case.aux, _st()) == 0, lib.sfh_last_error()
        return packed, 1.0
    n = (lib.sfh_packed_s3_weight_bytes if ar == "s3" else lib.sfh_packed_h2_weight_bytes)(*args)
    assert n > 0
    packed = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    if ar == "s3":
        assert lib.sfh_pack_s3_weights(_p(wd), _p(packed), *args, case.mode, case.aux, _st()) == 0, lib.sfh_last_error()
        return packed, 1.0
    wexp = K.wexp_for(w)
    assert lib.sfh_pack_h2_weights(_p(wd), _p(packed), *args, case.mode, case.aux, wexp, _st()) == 0, lib.sfh_last_error()
    return packed, 2.0 ** -wexp


def _entry(lib, case):
    return {"f32": lib.sfh_conv_fwd, "s3": lib.sfh_conv_s3_fwd, "h2": lib.sfh_conv_s3_fwd,
            "small": lib.sfh_conv_small_fwd}[case.kern]


def _launch(lib, case, inp, scale=None, shift=None, relu=False, exps=(2, 2, 2), reverse=False, wg_couts=None,
            expect=0, mutate=None):
    """one launch of `case` on the inputs `inp` -> dict y (destination layout, real channels), pool, word, ovf"""
    from sfh_amd._lib import ConvDesc
    ar = K.arith(case)
    e_src, e_dst, e_res = exps
    keep = []
    x0 = _dev(inp["x0"])
    if case.mode in (2, 4):       # the launch reads the space-to-depth tensor
        B, Hs, Ws, cs = x0.shape
        s2d = torch.full((B, (Hs + 1) // 2, (Ws + 1) // 2, 4 * cs), float("nan"), device="cuda")
        assert lib.sfh_space_to_depth2(_p(x0), _p(s2d), B, Hs, Ws, cs, _st()) == 0
        x0 = s2d
    x1 = _dev(inp["x1"])
    h0, w0, cs0 = x0.shape[1], x0.shape[2], x0.shape[3]
    s0 = x0 if ar == "f32" else _split(lib, x0, ar, e_src)
    s1 = x1 if (ar == "f32" or x1 is None) else _split(lib, x1, ar, e_src)
    packed, wscale = _pack(lib, case, inp["w"])
    scale = np.ones(case.cout, np.float32) if scale is None else scale
    shift = np.zeros(case.cout, np.float32) if shift is None else shift
    eff = scale.astype(np.float64) * wscale * (2.0 ** -e_src if ar == "h2" else 1.0)
    assert np.array_equal(eff.astype(np.float32).astype(np.float64), eff)       # a power of two: exact
    scd, shd = _dev(eff), _dev(shift)
    creal = case.cout // 4 if K.is_up(case) else case.cout
    dh, dw = K.dst_hw(case)
    split = "split" in case.flags
    dst = _SplitOut(lib, ar, case.B, dh, dw, case.dst_cs, e_dst) if split else _F32Out((case.B, dh, dw, case.dst_cs))
    pool = None
    if "dst_pool" in case.flags:
        pool = (_SplitOut(lib, ar, case.B, dh // 2, dw // 2, creal, e_dst) if split
                else _F32Out((case.B, dh // 2, dw // 2, creal)))
    res = None
    if "res" in case.flags or "res_f32" in case.flags:
        full = np.zeros((case.B, dh, dw, case.dst_cs), np.float32)
        full[..., :creal] = inp["res"]
        res = _dev(full)
        if split and "res" in case.flags:
            res = _split(lib, res, ar, e_res)
    word = torch.zeros(2, dtype=torch.int32, device="cuda")
    d = ConvDesc()
    d.src0, d.c0, d.cs0, d.h0, d.w0 = s0.data_ptr(), case.c0, cs0, h0, w0
    d.pool0 = 1 if "pool0" in case.flags else 0
    if s1 is not None:
        d.src1, d.c1, d.cs1, d.h1, d.w1 = s1.data_ptr(), case.c1, x1.shape[3], x1.shape[1], x1.shape[2]
        d.pad_top1, d.pad_left1 = case.pad1
    d.batch, d.H, d.W, d.ksize, d.stride, d.tile = case.B, case.H, case.W, case.ks, case.stride, case.tile
    d.wpacked, d.scale, d.shift, d.cout, d.relu = packed.data_ptr(), scd.data_ptr(), shd.data_ptr(), case.cout, int(relu)
    d.residual, d.residual_f32 = _a(res), 1 if "res_f32" in case.flags else 0
    d.dst, d.dst_cs, d.out_mode = dst.ptr(), case.dst_cs, 1 if K.is_up(case) else 0
    d.src_fmt, d.dst_fmt = FMT[ar], FMT[ar] if split else 0
    if pool is not None:
        d.dst_pool, d.pool_cs = pool.ptr(), creal
    if "short" in case.flags:
        d.up_dst_h, d.up_dst_w = dh, dw
    d.reverse_tiles = int(reverse)
    d.h2_exp_src, d.h2_exp_dst, d.h2_exp_res = exps
    if ar == "h2" and split:
        d.h2_range, d.h2_overflow = word.data_ptr(), word.data_ptr() + 4
    d.wg_couts = wg_couts if wg_couts is not None else (128 if "wg128" in case.flags else 0)
    if mutate is not None:
        mutate(d)
    keep += [s0, s1, packed, scd, shd, res, word]
    rc = _entry(lib, case)(ctypes.byref(d), _st())
    _sync()
    assert rc == expect, (rc, lib.sfh_last_error())
    if expect != 0:
        assert dst.untouched() and (pool is None or pool.untouched())
        return None
    get = (lambda o: o.numpy(creal)) if split else (lambda o: o.numpy()[..., :creal])
    if not split and case.dst_cs > creal:
        tail = dst.buf[:dst.n].view(torch.int32).view(case.B, dh, dw, case.dst_cs)[..., creal:]
        assert bool((tail == 0x7FC00000).all()), "stored channels behind cout were written"
    w2 = word.cpu().numpy()
    return dict(y=get(dst), pool=get(pool) if pool is not None else None,
                word=float(w2[:1].view(np.float32)[0]), ovf=int(w2[1]))


def _check_range_word(out, ref, e_dst):
    """H2 destination: the range word holds a value within the element bound of max |y * 2^e| over the tensor's elements, the
    overflow word stays 0, nothing saturates"""
    lo = float((np.abs(ref["y"]) - ref["bound"]).max()) * 2.0 ** e_dst
    hi = float((np.abs(ref["y"]) + ref["bound"]).max()) * 2.0 ** e_dst
    assert out["ovf"] == 0 and hi < 65504.0
    assert lo <= out["word"] <= hi, (lo, out["word"], hi)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ forward and backward-data
PARTS = ("int", "int_epilogue", "randn", "randn_epilogue")


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("case", K.FWD, ids=lambda c: c.name)
def test_forward_cases(lib, case, part):
    """int: the fp64 value bit for bit from the raw launch; int_epilogue: bit for bit through scale (one channel 0), a shift
    that puts half the outputs below zero, residual, ReLU and the pooled output; randn: inside the bound, a second call (and
    reverse_tiles, and the other wg_couts) gives the same bits; randn_epilogue: inside the bound through the epilogue, H2
    destinations also at other exponents.  H2 destinations leave a correct range word."""
    ar, h2dst = K.arith(case), K.arith(case) == "h2" and "split" in case.flags
    up = K.is_up(case)
    inp = K.fwd_inputs(case, "int" if part.startswith("int") else "randn")
    ref = K.reference(case, inp)
    if part == "int":
        assert float(ref["A"].max()) < 2 ** 24
        out = _launch(lib, case, inp)
        assert np.array_equal(out["y"].astype(np.float64), ref["y"])
        return
    if part == "randn":
        out = _launch(lib, case, inp)
        worst = {f"{ar} forward": R.ratio(out["y"], ref["y"], ref["bound"])}
        again = _launch(lib, case, inp, reverse="rev" in case.flags, wg_couts=64 if "wg128" in case.flags else None)
        assert np.array_equal(_bits(out["y"]), _bits(again["y"]))
        _report(case.name, **worst)
        return
    scale, shift = K.epilogue_inputs(case, ref["acc"])
    refe = K.reference(case, inp, scale, shift, relu=True)
    oute = _launch(lib, case, inp, scale, shift, relu=True)
    if part == "int_epilogue":
        assert np.array_equal(oute["y"].astype(np.float64), refe["y"])
        assert 0.1 < float((refe["y"] > 0).mean()) < 0.9
        if not ("res" in case.flags or "res_f32" in case.flags) and not up:
            assert (oute["y"][..., 1] == np.float32(0.25)).all()                       # scale = 0: the shift alone
        if oute["pool"] is not None:
            assert np.array_equal(oute["pool"].astype(np.float64), refe["pool"])
        if h2dst:
            _check_range_word(oute, refe, 2)
        return
    worst = {f"{ar} epilogue": R.ratio(oute["y"], refe["y"], refe["bound"])}
    if oute["pool"] is not None:
        worst[f"{ar} epilogue:pool"] = R.ratio(oute["pool"], refe["pool"], refe["pool_bound"])
    if h2dst:
        _check_range_word(oute, refe, 2)
        e3 = (2, 0, 1)       # other exponents for the destination and the residual: the same values
        ref3 = K.reference(case, inp, scale, shift, relu=True, exps=e3)
        out3 = _launch(lib, case, inp, scale, shift, relu=True, exps=e3)
        worst[f"{ar} epilogue:exps"] = R.ratio(out3["y"], ref3["y"], ref3["bound"])
        _check_range_word(out3, ref3, 0)
    _report(case.name, **worst)


def _impulse_sources(case):
    s0, s1 = K.source_shapes(case)
    for code in (K.pixel_coded, K.channel_coded):
        yield dict(x0=code(s0), x1=code(s1) + 7.0 if s1 else None, res=None)


@pytest.mark.parametrize("case", K.IMPULSE, ids=lambda c: c.name)
def test_forward_impulses(lib, case):
    """a single 1 in the weight: exactly one shifted, zero-padded source channel in one destination channel, from a pixel-coded
    and a channel-coded source; H2 at source exponents 0 and 2"""
    for src in _impulse_sources(case):
        frame = R.assemble(src["x0"], case.c0, src["x1"], case.c1, case.pad1)
        for w, o, c, ky, kx in K.impulse_weights(case):
            want = R.shifted_copy(frame, c, case.cout, o, ky, kx, case.ks, case.stride)
            for e in ((0, 2) if K.arith(case) == "h2" else (2,)):
                got = _launch(lib, case, dict(src, w=w), exps=(e, 2, 2))["y"]
                assert np.array_equal(got.astype(np.float64), want), (o, c, ky, kx, e)


@pytest.mark.parametrize("case", K.IMPULSE_BWD, ids=lambda c: c.name)
def test_backward_data_impulses(lib, case):
    """pack mode 3 on a weight with a single 1 at (o, c, ky, kx): dx channel c is dz channel o moved the other way (the tap
    flip), zero elsewhere and in the padded output channels"""
    s0, _ = K.source_shapes(case)
    for code in (K.pixel_coded, K.channel_coded):
        dz = code(s0)
        for w, o, c, ky, kx in K.impulse_weights(case):
            want = R.scattered_copy(dz, o, case.cout, c, ky, kx, case.ks)
            got = _launch(lib, case, dict(x0=dz, x1=None, w=w, res=None))["y"]
            assert np.array_equal(got.astype(np.float64), want), (o, c, ky, kx)


@pytest.mark.parametrize("case", K.IMPULSE_UP2 + K.IMPULSE_BWD_REF, ids=lambda c: c.name)
def test_impulses_against_the_reference(lib, case):
    """the 2x2 up-scatter conv (source and destination one short), pack mode 3 at 1x1, modes 1 and 4: a single 1 in the weight
    at the first and last (o, c) and every tap, pixel- and channel-coded sources - the fp64 reference's value (integers:
    exact; tests/test_dense_conv_host.py holds these references to torch and to a loop restatement) bit for bit"""
    s0, _ = K.source_shapes(case)
    ws = K.weight_shape(case)
    for code in (K.pixel_coded, K.channel_coded):
        x = code(s0)
        for (o, c) in ((0, 0), (ws[0] - 1, ws[1] - 1), (ws[0] // 4 + 5, 3), (ws[0] // 2 - 1, ws[1] // 2)):
            for ky in range(ws[2]):
                for kx in range(ws[3]):
                    w = np.zeros(ws, np.float32)
                    w[o, c, ky, kx] = 1.0
                    inp = dict(x0=x, x1=None, w=w, res=None)
                    want = K.reference(case, inp)["y"]
                    assert want.any() or (case.mode == 2)
                    got = _launch(lib, case, inp)["y"]
                    assert np.array_equal(got.astype(np.float64), want), (o, c, ky, kx)


@pytest.mark.parametrize("case", K.PLANE_WALK, ids=lambda c: c.name)
def test_forward_plane_walk(lib, case):
    """operands with one bit in every plane and a one-tap weight of the same structure: the sum of the RETAINED products is an
    fp32 number and the fp64 product rounds to exactly it (tests/test_dense_conv_host.py proves both for these constants)
    - the output must equal it bit for bit; a lost product moves it by 32 (S3) or 1024 (H2) ulps"""
    ar = K.arith(case)
    s0, _ = K.source_shapes(case)
    for e in ((0, 2) if ar == "h2" else (2,)):
        x = K.walk_values(s0, ar, 11, e)
        for (o, c, ky, kx) in ((0, 0, 0, 0), (case.cout - 1, case.c0 - 1, 2, 2), (64, 31, 1, 2), (63, 32, 2, 0)):
            w = np.zeros(K.weight_shape(case), np.float32)
            w[o % case.cout, c % case.c0, ky, kx] = K.walk_weight(ar)
            inp = dict(x0=x, x1=None, w=w, res=None)
            want = K.reference(case, inp)["y"]          # rounds to the retained sum (_bits takes it to fp32)
            got = _launch(lib, case, inp, exps=(e, 2, 2))["y"]
            assert np.array_equal(_bits(got), _bits(want)), (o, c, ky, kx, e)


@pytest.mark.parametrize("kern", ["h2", "small"])
def test_h2_range_word_sees_the_tensor_only(lib, kern):
    """The range and overflow words cover the tensor's elements, not the lanes of the workgroup tiles that store nothing
    (tile round-up past the last row and column, the shared zero rows between frames).  A source whose last column and
    last row are 1000 times the rest, under a weight whose single tap reads one pixel up and to the left: the 1000s land only
    on output pixels past the frame.  The stored maximum is 1: the word must be 4.0 at exponent 2 (before the fix to
    sfh_conv_epilogue: 4000.0, on both kernels)."""
    case = K.fwd(f"{kern}_range", kern, 2, 7, 9, flags=("split",))
    x = np.ones((2, 7, 9, 32), np.float32)
    x[:, -1, :, :] = 1000.0
    x[:, :, -1, :] = 1000.0
    w = np.zeros(K.weight_shape(case), np.float32)
    w[3, 5, 0, 0] = 1.0
    inp = dict(x0=x, x1=None, w=w, res=None)
    ref = K.reference(case, inp)
    assert float(np.abs(ref["y"]).max()) == 1.0
    out = _launch(lib, case, inp)
    assert np.array_equal(out["y"].astype(np.float64), ref["y"])
    assert out["ovf"] == 0 and out["word"] == 4.0, out["word"]


def test_refused_launches_write_nothing(lib):
    """the refusals next to the admitted cases: -1, and the NaN-filled outputs keep every byte"""
    f32, s3, h2 = K.fwd("r_f32", "f32", 2, 7, 9, c0=16, c1=16), K.fwd("r_s3", "s3", 2, 7, 9), K.fwd("r_h2", "h2", 2, 7, 9)
    inp = lambda c: K.fwd_inputs(c, "int")

    def set_(**kw):
        def m(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return m
    for case in (f32, s3, h2):
        _launch(lib, case, inp(case), expect=-1, mutate=set_(cout=96))             # no multiple of 64
    for case in (s3, h2):
        _launch(lib, case, inp(case), expect=-1, mutate=set_(c0=16))               # c0 % 32
        _launch(lib, case, inp(case), expect=-1, mutate=set_(pool0=1))             # pool0 on a split source
    _launch(lib, f32, inp(f32), expect=-1, mutate=set_(pad_top1=2))                 # source 1 does not fit the frame
    _launch(lib, f32, inp(f32), expect=-1, mutate=set_(w1=9, pad_left1=1))
    two = K.fwd("r_s3_two", "s3", 2, 7, 9, c0=32, c1=32)
    _launch(lib, two, inp(two), expect=-1, mutate=set_(pad_left1=2))
    big = K.fwd("r_s3_ksplit", "s3", 2, 7, 9, c0=64)
    _launch(lib, big, inp(big), relu=True, expect=-1, mutate=set_(ksplit=2, ksplit_stride=2 * 7 * 9 * 64 * 4))   # split-K with ReLU
    small = K.fwd("r_small", "small", 2, 7, 9)
    _launch(lib, small, inp(small), expect=-1, mutate=set_(stride=2))


@pytest.mark.parametrize("fmt", ["s3", "h2"])
def test_split_conversions(lib, fmt):
    """sfh_f32_to_s3 / sfh_f32_to_h2 and their inverses on an odd shape (B 3, 5 x 7, 64 channels): S3 round trip bit for bit
    over 40 binades, H2 within the header's stated error at exponents 2 and -3 (the bound is the header's figure, reached
    exactly - ratio 1.000 - by a value half-way between two plane-1 subnormals: the conversion has no other rounding to
    count, so the bound carries no 1.01, and error and bound are both exact binary fractions: the comparison is not a matter
    of rounding), integers below 2^11 exact"""
    r = np.random.default_rng(9)
    shape = (3, 5, 7, 64)
    x = (r.standard_normal(shape) * np.exp(r.uniform(-14, 14, shape))).astype(np.float32)
    x[0, 0, 0, :4] = (0.0, -0.0, 2.0 ** -30, 1.0)

    def back(t, e):
        out = _SplitOut(lib, fmt, 3, 5, 7, 64, e)
        out.buf[:out.n] = t
        return out.numpy(64)
    if fmt == "s3":
        got = back(_split(lib, _dev(x), "s3", 0), 0)
        diff = _bits(got) != _bits(x)
        print("S3 round trip: elements whose bits differ:", int(diff.sum()), x[diff][:8], got[diff][:8])
        assert np.array_equal(got, x)          # every value; -0 comes back as +0 (plane 1 of -0 is +0, and -0 + 0 = +0)
        assert np.array_equal(_bits(got)[x != 0], _bits(x)[x != 0])
        return
    for e in (2, -3):
        v = np.clip(x, -1000.0, 1000.0)
        got = back(_split(lib, _dev(v), "h2", e), e)
        _report(f"h2 round trip e={e}", **{"h2 conversion": R.ratio(got, v.astype(np.float64), R.h2_rep(v, e)[0])})
    q = r.integers(-2047, 2048, shape).astype(np.float32)
    assert np.array_equal(back(_split(lib, _dev(q), "h2", 2), 2), q)


# ------------------------------------------------------------------------------------------------ backward-filter
def _wgrad(lib, case, dz, x0, x1, raw0):
    """the launches of one case: source 0 at n_off 0 and, with a second source, source 1 at n_off N -> raw (M, ks^2, raw_n)"""
    raw = _F32Out(raw0.shape, init=raw0)
    raw_n = raw0.shape[2]
    dzd = _dev(dz)
    B, H, W, M = dz.shape
    dzs = dzd if case.kern == "f32" else _split(lib, dzd, case.kern, 2)
    for x, n_off, pad in ((x0, 0, (0, 0)), (x1, case.N, case.pad)):
        if x is None:
            continue
        xd = _dev(x)
        _, xh, xw, N = x.shape
        if case.kern == "f32":
            rc = lib.sfh_conv_wgrad(_p(dzd), M, M, _p(xd), N, xh, xw, N, pad[0], pad[1], B, H, W, case.ks, raw.ptr(), raw_n,
                                    n_off, _st())
        else:
            xs = _split(lib, xd, case.kern, 2)
            rc = lib.sfh_conv_wgrad_s3(_p(dzs), M, _p(xs), N, xh, xw, N, pad[0], pad[1], B, H, W, case.ks, raw.ptr(), raw_n,
                                       n_off, FMT[case.kern], _st())
        _sync()
        assert rc == 0, lib.sfh_last_error()
    return raw.numpy()


def _wgrad_ref(case, dz, x0, x1, raw0):
    """-> (raw, bound) over the whole (M, ks^2, raw_n) buffer: columns no launch adds to keep raw0 exactly"""
    want, bound = raw0.astype(np.float64), np.zeros(raw0.shape)
    for x, n_off, pad in ((x0, 0, (0, 0)), (x1, case.N, case.pad)):
        if x is not None:
            sl = slice(n_off, n_off + x.shape[3])
            want[..., sl], bound[..., sl] = R.wgrad(dz, x, raw0[..., sl], case.ks, case.kern, pad)
    return want, bound


@pytest.mark.parametrize("case", K.WGRAD, ids=lambda c: c.name)
def test_wgrad_cases(lib, case):
    """onto a non-zero raw: integers bit for bit; randn inside the bound; the columns behind the sources keep raw0"""
    dz, x0, x1, raw0 = K.wg_inputs(case, "int")
    want, _ = _wgrad_ref(case, dz, x0, x1, raw0)
    assert np.array_equal(_wgrad(lib, case, dz, x0, x1, raw0).astype(np.float64), want)
    dz, x0, x1, raw0 = K.wg_inputs(case, "randn")
    want, bound = _wgrad_ref(case, dz, x0, x1, raw0)
    _report(case.name, **{f"{case.kern} backward-filter": R.ratio(_wgrad(lib, case, dz, x0, x1, raw0), want, bound)})


@pytest.mark.parametrize("case", [c for c in K.WGRAD if c.name.endswith(("_M64", "two_pad11"))], ids=lambda c: c.name)
def test_wgrad_impulses(lib, case):
    """a single non-zero dz element against a pixel-coded and a channel-coded x: raw is a window of x, exactly"""
    B, H, W = case.B, case.H, case.W
    raw0 = np.ones((case.M, case.ks ** 2, case.N + case.N1 + 32), np.float32)
    for code in (K.pixel_coded, K.channel_coded):
        x0 = code((B, H, W, case.N))
        x1 = code((B, H - 1, W - 1, case.N1)) + 5.0 if case.N1 else None
        for (b, y, x, m) in ((0, 0, 0, 0), (B - 1, H - 1, W - 1, case.M - 1), (0, H // 2, min(31, W - 1), 63),
                             (B - 1, min(1, H - 1), min(32, W - 1), 17)):
            dz = np.zeros((B, H, W, case.M), np.float32)
            dz[b, y, x, m] = 2.0
            want, _ = _wgrad_ref(case, dz, x0, x1, raw0)
            assert np.array_equal(_wgrad(lib, case, dz, x0, x1, raw0).astype(np.float64), want), (b, y, x, m)


@pytest.mark.parametrize("case", [c for c in K.WGRAD if c.kern != "f32" and c.name.endswith("_M64")], ids=lambda c: c.name)
def test_wgrad_plane_walk(lib, case):
    """a single non-zero dz element and an x whose values have one bit in every plane, onto raw0 = 8: bit for bit the fp64 value"""
    B, H, W = case.B, case.H, case.W
    x0 = K.walk_values((B, H, W, case.N), case.kern, 13)
    raw0 = np.full((case.M, case.ks ** 2, case.N + 32), 8.0, np.float32)
    for (b, y, x, m) in ((0, 0, 0, 0), (B - 1, H - 1, W - 1, case.M - 1), (0, H // 2, 31, 33)):
        dz = np.zeros((B, H, W, case.M), np.float32)
        dz[b, y, x, m] = K.walk_weight(case.kern) * 2.0
        want, _ = _wgrad_ref(case, dz, x0, None, raw0)      # rounds to 8 + the retained sum
        assert np.array_equal(_bits(_wgrad(lib, case, dz, x0, None, raw0)), _bits(want)), (b, y, x, m)


def test_wgrad_refusals(lib):
    raw = _F32Out((64, 9, 64))
    x = torch.zeros(2 * 7 * 9 * 64, device="cuda")
    s = torch.zeros(2 * 7 * 9 * 64 * 3, dtype=torch.int16, device="cuda")
    assert lib.sfh_conv_wgrad(_p(x), 64, 64, _p(x), 64, 7, 9, 64, 0, 0, 2, 7, 9, 3, raw.ptr(), 64, 32, _st()) == -1   # n_off + N > raw_n
    assert lib.sfh_conv_wgrad(_p(x), 64, 64, _p(x), 64, 7, 9, 64, 0, 0, 2, 7, 9, 4, raw.ptr(), 64, 0, _st()) == -1    # ksize 4: N <= 32
    assert lib.sfh_conv_wgrad(_p(x), 64, 64, _p(x), 64, 7, 9, 64, 1, 0, 2, 7, 9, 3, raw.ptr(), 64, 0, _st()) == -1    # does not fit
    assert lib.sfh_conv_wgrad_s3(_p(s), 32, _p(s), 64, 7, 9, 64, 0, 0, 2, 7, 9, 3, raw.ptr(), 64, 0, 1, _st()) == -1   # M % 64
    assert lib.sfh_conv_wgrad_s3(_p(s), 64, _p(s), 64, 7, 9, 64, 0, 0, 2, 7, 9, 4, raw.ptr(), 64, 0, 1, _st()) == -1   # ksize 4
    assert lib.sfh_conv_wgrad_s3(_p(s), 64, _p(s), 64, 7, 9, 64, 0, 1, 2, 7, 9, 3, raw.ptr(), 64, 0, 2, _st()) == -1   # does not fit
    assert raw.untouched()
