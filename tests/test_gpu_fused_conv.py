"""The specialised convolution launches on the GPU, one launch per check, through the raw C entry points with a hand-filled
sfh_conv_desc: sfh_conv_upfused_fwd and the two launches it replaces (sfh_conv_s3_fwd with ksize 2 / shift_border writing the
fp32 partial, sfh_conv_s3_fwd with acc_init), sfh_conv3x3_c4h2_fwd, sfh_conv3x3_c4_fwd, sfh_frame_to_h2,
sfh_conv_inc_fused_fwd and sfh_stem7x7_fwd (both instances, three arithmetics) - on every case of tests/fused_conv_cases.py
against the fp64 values and bounds of tests/fused_conv_ref.py.  Weights are packed by the library's own pack entries, split
tensors come from sfh_f32_to_h2 / sfh_frame_to_h2; the expected values come from the reference only.  Every comparison is per
element: bit equality, or a bound built from the reference's absolute sums (tests/test_fused_conv_host.py holds every bound to
a numpy restatement of the kernel's arithmetic and proves that the reference meets the equalities asked here).  Outputs start
as NaN and end in a guard that must keep its bytes; stored channels beyond cout must keep theirs."""
import ctypes

import numpy as np
import pytest
import torch

import dense_conv_cases as K
import fused_conv_cases as C
import fused_conv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1       # a NaN in bf16 and in fp16: what split outputs start as
NP = {"s3": 3, "h2": 2}
FMT = {"f32": 0, "s3": 1, "h2": 2, "fh2": 3}
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

    def numpy(self, cout=None):
        """-> the tensor (channels [0, cout) of it: the stored channels behind cout must keep their NaN)"""
        _sync()
        assert bool(torch.isnan(self.buf[self.n:]).all()), "the guard behind the output was written"
        out = self.buf[:self.n].view(self.shape)
        if cout is not None and cout < self.shape[-1]:
            tail = self.buf[:self.n].view(torch.int32).view(self.shape)[..., cout:]
            assert bool((tail == 0x7FC00000).all()), "stored channels behind cout were written"
            out = out[..., :cout]
        return out.cpu().numpy()

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


def _out(lib, fmt, B, H, W, cs, exp):
    return _F32Out((B, H, W, cs)) if fmt == "f32" else _SplitOut(lib, fmt, B, H, W, cs, exp)


def _split_h2(lib, x, exp):
    """fp32 NHWC numpy tensor -> the H2 tensor of the library's own conversion"""
    x = _dev(x)
    B, H, W, cs = x.shape
    out = torch.full((B * H * W * cs * 2,), SENTINEL, dtype=torch.int16, device="cuda")
    assert lib.sfh_f32_to_h2(_p(x), _p(out), B * H, W, cs, exp, None, None, _st()) == 0, lib.sfh_last_error()
    return out


def _frame_h2(lib, x, exp, words=None, nhwc4=None):
    """NHWC numpy (B,H,W,C) -> the FH2 frame tensor of sfh_frame_to_h2 (8 fp16 words per pixel, + a guard)"""
    B, H, W, Cn = x.shape
    src = _dev(np.transpose(x, (0, 3, 1, 2)))
    out = torch.full((B * H * W * 8 + K.GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    ovf = _p(words[1:]) if words is not None else None
    rng = _p(words[:1]) if words is not None else None
    rc = lib.sfh_frame_to_h2(_p(src), ctypes.c_void_p(nhwc4.ptr()) if nhwc4 is not None else None, _p(out), B, Cn, H, W, exp,
                             ovf, rng, _st())
    _sync()
    assert rc == 0, lib.sfh_last_error()
    assert bool((out[B * H * W * 8:] == SENTINEL).all()), "the guard behind the frame tensor was written"
    return out


def _pack_h2(lib, w, ks, c0, cout):
    """-> (packed weights of sfh_pack_h2_weights, wexp)"""
    n = lib.sfh_packed_h2_weight_bytes(ks, c0, 0, cout)
    assert n > 0
    packed = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    wexp = K.wexp_for(w)
    assert lib.sfh_pack_h2_weights(_p(_dev(w)), _p(packed), ks, c0, 0, cout, 0, 0, wexp, _st()) == 0, lib.sfh_last_error()
    return packed, wexp


def _pow2(v, e):
    """v * 2^e as float32, which must be exact (a power of two folded into a scale)"""
    out = np.asarray(v, np.float64) * 2.0 ** e
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return _dev(out)


def _words():
    return torch.zeros(2, dtype=torch.int32, device="cuda")


def _read_words(word):
    w2 = word.cpu().numpy()
    return float(w2[:1].view(np.float32)[0]), int(w2[1])


def _check_range_word(word, ovf, y, bound, e):
    """H2 destination: the range word holds a value within the element bound of max |y * 2^e| over the tensor's elements, the
    overflow word stays 0, nothing saturates"""
    lo, hi = R.range_word_limits(y, bound, e)
    assert ovf == 0 and hi < 65504.0
    assert lo <= word <= hi, (lo, word, hi)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _set(**kw):
    def m(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return m


# ------------------------------------------------------------------------------------------------ the fused Up block
def _up_sources(lib, case, inp):
    return dict(skip=_split_h2(lib, inp["skip"], case.e_src), low=_split_h2(lib, inp["low"], case.e_src))


def _up_launch(lib, case, src, inp, scale, shift, relu, form, mutate=None, expect=0):
    """the fused Up block's first conv as ONE launch (form 'fused') or as the two launches it replaces ('two')
    -> dict y (B,H,W,cout), buf (the destination's words), word, ovf"""
    from sfh_amd._lib import ConvDesc
    B, H, W, cout = case.B, case.H, case.W, case.cout
    wsk, wexp_sk = _pack_h2(lib, inp["w"], 3, case.c0, cout)
    wup, wexp_up = _pack_h2(lib, inp["wq"], 2, case.c1, 4 * cout)
    # everything in the skip-half conv's accumulator units: real = acc * 2^-(e_src + wexp_sk)
    usk = _pow2(inp["us"], wexp_sk - wexp_up)
    sbk = _pow2(inp["sb"], case.e_src + wexp_sk)
    sck, shd = _pow2(scale, -(case.e_src + wexp_sk)), _dev(shift)
    dst = _SplitOut(lib, "h2", B, H, W, cout + 32, case.e_dst)
    word = _words()
    d = ConvDesc()
    d.src0, d.c0, d.cs0, d.h0, d.w0 = src["skip"].data_ptr(), case.c0, case.c0 + 32, H, W
    d.batch, d.H, d.W, d.ksize, d.stride = B, H, W, 3, 1
    d.wpacked, d.scale, d.shift, d.cout, d.relu = wsk.data_ptr(), sck.data_ptr(), shd.data_ptr(), cout, int(relu)
    d.dst, d.dst_cs, d.src_fmt, d.dst_fmt = dst.ptr(), cout + 32, FMT["h2"], FMT["h2"]
    d.h2_exp_src, d.h2_exp_dst, d.h2_range, d.h2_overflow = case.e_src, case.e_dst, word.data_ptr(), word.data_ptr() + 4
    part = zero4 = None
    if form == "fused":
        d.src1, d.c1, d.cs1, d.h1, d.w1 = src["low"].data_ptr(), case.c1, case.c1 + 32, case.h1, case.w1
        d.up_wpacked, d.up_scale, d.shift_border = wup.data_ptr(), usk.data_ptr(), sbk.data_ptr()
        if mutate is not None:
            mutate(d)
        rc = lib.sfh_conv_upfused_fwd(ctypes.byref(d), _st())
    else:
        Hc, Wc = C.up_frame(case)
        part, zero4 = _F32Out((B, H, W, cout)), torch.zeros(4 * cout, device="cuda")
        u = ConvDesc()
        u.src0, u.c0, u.cs0, u.h0, u.w0 = src["low"].data_ptr(), case.c1, case.c1 + 32, case.h1, case.w1
        u.batch, u.H, u.W, u.ksize, u.stride = B, Hc, Wc, 2, 1
        u.wpacked, u.scale, u.shift, u.cout, u.relu = wup.data_ptr(), usk.data_ptr(), zero4.data_ptr(), 4 * cout, 0
        u.shift_border, u.up_dst_h, u.up_dst_w = sbk.data_ptr(), H, W
        u.dst, u.dst_cs, u.out_mode, u.src_fmt, u.dst_fmt = part.ptr(), cout, 1, FMT["h2"], FMT["f32"]
        u.h2_exp_src = case.e_src
        rc = lib.sfh_conv_s3_fwd(ctypes.byref(u), _st())
        _sync()
        assert rc == 0, lib.sfh_last_error()
        part.numpy()       # the guard behind the partial
        d.acc_init = part.ptr()
        if mutate is not None:
            mutate(d)
        rc = lib.sfh_conv_s3_fwd(ctypes.byref(d), _st())
    _sync()
    assert rc == expect, (rc, lib.sfh_last_error())
    if expect != 0:
        assert dst.untouched()
        return None
    word_, ovf = _read_words(word)
    return dict(y=dst.numpy(cout), buf=dst.buf, word=word_, ovf=ovf, wexp=(wexp_up, wexp_sk))


def _up_both(lib, case, src, inp, scale, shift, relu):
    """both forms; the fused launch must leave the two-launch form's words bit for bit (planes, range, overflow)"""
    one = _up_launch(lib, case, src, inp, scale, shift, relu, "fused")
    two = _up_launch(lib, case, src, inp, scale, shift, relu, "two")
    assert torch.equal(one["buf"], two["buf"]), "the fused launch and the two launches differ"
    assert (one["word"], one["ovf"]) == (two["word"], two["ovf"])
    return one, two


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("case", C.UP, ids=lambda c: c.name)
def test_up_block_cases(lib, case, kind):
    """int: the fp64 value bit for bit from the fused launch and from the two-launch form; randn: both inside the bound.  The
    two forms agree in every stored word, the range word lies within the element bound, the overflow word stays 0."""
    inp = C.up_inputs(case, kind)
    wexp = (K.wexp_for(inp["wq"]), K.wexp_for(inp["w"]))
    ones, zeros = np.ones(case.cout, np.float32), np.zeros(case.cout, np.float32)
    scale, shift = C.up_epilogue(case, R.upfused(case, inp, ones, zeros, False, *wexp)["acc"], kind)
    ref = R.upfused(case, inp, scale, shift, bool(case.relu), *wexp)
    src = _up_sources(lib, case, inp)
    one, two = _up_both(lib, case, src, inp, scale, shift, bool(case.relu))
    assert one["wexp"] == wexp
    for out in (one, two):
        _check_range_word(out["word"], out["ovf"], ref["y"], ref["bound"], case.e_dst)
    if kind == "int":
        assert np.array_equal(one["y"].astype(np.float64), ref["y"])
        assert np.array_equal(two["y"].astype(np.float64), ref["y"])
        return
    _report(case.name, **{"upfused": R.ratio(one["y"], ref["y"], ref["bound"]),
                          "two-launch up block": R.ratio(two["y"], ref["y"], ref["bound"])})


@pytest.mark.parametrize("case", C.UP_IMPULSE, ids=lambda c: c.name)
def test_up_block_impulses(lib, case):
    """a single 1 in the composed conv's weights (all 4 taps of all 4 quadrants) or in the skip half's (all 9 taps), the other
    half zero, up_scale 1 and a zero border table: exactly one shifted, zero-padded source channel in one destination channel,
    from pixel-coded and channel-coded sources, in both forms"""
    ones, zeros = np.ones(case.cout, np.float32), np.zeros(case.cout, np.float32)
    tab = dict(us=np.ones(4 * case.cout, np.float32), sb=np.zeros((16, 4 * case.cout), np.float32))
    sk, lo = (case.B, case.H, case.W, case.c0 + 32), (case.B, case.h1, case.w1, case.c1 + 32)
    for code in (K.pixel_coded, K.channel_coded):
        data = dict(skip=code(sk), low=code(lo) + 7.0)
        src = _up_sources(lib, case, data)
        for half, w, wq, o, c, ky, kx in C.up_impulses(case):
            if half == "up":
                want = R.up_shifted_copy(case, data["low"], c, o, ky, kx)
            else:
                want = R.shifted_copy(data["skip"][..., :case.c0], c, case.cout, o, ky, kx, 3, 1)
            one, _ = _up_both(lib, case, src, dict(data, w=w, wq=wq, **tab), ones, zeros, False)
            assert np.array_equal(one["y"].astype(np.float64), want), (half, o, c, ky, kx)


@pytest.mark.parametrize("case", C.UP_WALK, ids=lambda c: c.name)
def test_up_block_plane_walk(lib, case):
    """both phases: one walk-structured weight over a walk-valued source (the other half zero): the retained products sum to an
    fp32 number that the H2 destination holds exactly - the output equals the fp64 product bit for bit, in both forms; a
    missing or doubled cross product moves it by 1024 ulps"""
    ones, zeros = np.ones(case.cout, np.float32), np.zeros(case.cout, np.float32)
    tab = dict(us=np.ones(4 * case.cout, np.float32), sb=np.zeros((16, 4 * case.cout), np.float32))
    data = dict(skip=K.walk_values((case.B, case.H, case.W, case.c0 + 32), "h2", 21, case.e_src),
                low=K.walk_values((case.B, case.h1, case.w1, case.c1 + 32), "h2", 22, case.e_src))
    src = _up_sources(lib, case, data)
    ws, wqs = (case.cout, case.c0, 3, 3), (4 * case.cout, case.c1, 2, 2)
    picks = [("up", (q * case.cout + o, c, t >> 1, t & 1)) for q, o, c, t in ((0, 0, 0, 0), (1, 63, 31, 3), (2, 64, 32, 1),
                                                                           (3, case.cout - 1, case.c1 - 1, 2))]
    picks += [("skip", p) for p in ((0, 0, 0, 0), (case.cout - 1, case.c0 - 1, 2, 2), (64, 31, 1, 2), (63, 32, 2, 0), (5, 7, 1, 1))]
    for half, (o, c, ky, kx) in picks:
        w, wq = np.zeros(ws, np.float32), np.zeros(wqs, np.float32)
        (wq if half == "up" else w)[o, c, ky, kx] = K.walk_weight("h2")
        inp = dict(data, w=w, wq=wq, **tab)
        want = R.upfused(case, inp, ones, zeros, False, K.wexp_for(wq), K.wexp_for(w))["y"]
        assert want.any()
        one, _ = _up_both(lib, case, src, inp, ones, zeros, False)
        assert np.array_equal(_bits(one["y"]), _bits(want)), (half, o, c, ky, kx)


def test_up_block_refusals(lib):
    """every SFH_REQUIRE of sfh_conv_upfused_fwd's launcher: -1, and the destination keeps every byte"""
    case = C.Up("up_refuse", 1, 5, 7, 2, 3, 32, 32, 64, 0, 2, 2)
    inp = C.up_inputs(case, "int")
    src = _up_sources(lib, case, inp)
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    keep = torch.zeros(64, device="cuda")
    for m in (_set(H=6, h0=6), _set(W=8, w0=8), _set(h0=4), _set(h1=3), _set(cout=96), _set(cout=32), _set(c0=16), _set(c1=48),
              _set(cs0=32 + 16), _set(dst_cs=64 + 16), _set(dst_cs=32), _set(residual=keep.data_ptr()),
              _set(dst_pool=keep.data_ptr()), _set(acc_init=keep.data_ptr()), _set(head_w=keep.data_ptr()), _set(pool0=1),
              _set(ksplit=2), _set(src_fmt=FMT["s3"]), _set(dst_fmt=FMT["f32"]), _set(dst_fmt=FMT["s3"]), _set(src_fmt=FMT["f32"]),
              _set(h2_exp_dst=65), _set(src1=None), _set(up_wpacked=None), _set(up_scale=None), _set(shift_border=None),
              _set(batch=0)):
        _up_launch(lib, case, src, inp, ones, zeros, False, "fused", mutate=m, expect=-1)
    out = _up_launch(lib, case, src, inp, ones, zeros, False, "fused")       # and the unmutated descriptor is admitted
    assert np.array_equal(out["y"].astype(np.float64), R.upfused(case, inp, ones, zeros, False, *out["wexp"])["y"])


# ------------------------------------------------------------------------------------------------ sfh_frame_to_h2
def _f2h(lib, x, e):
    """-> (planes (B,H,W,2,4) float32, nhwc4 (B,H,W,4), range word bits, overflow word)"""
    B, Cn, H, W = x.shape
    nhwc4, words = _F32Out((B, H, W, 4)), _words()
    fh2 = _frame_h2(lib, np.transpose(x, (0, 2, 3, 1)), e, words, nhwc4)
    planes = fh2[:B * H * W * 8].view(torch.float16).view(B, H, W, 2, 4).float().cpu().numpy()
    w2 = words.cpu().numpy().view(np.uint32)
    return planes, nhwc4.numpy(), int(w2[0]), int(w2[1])


@pytest.mark.parametrize("case", C.F2HS, ids=lambda c: c.name)
def test_frame_to_h2(lib, case):
    """both planes are the numpy split bit for bit (channels beyond C: +0), the NHWC4 copy is exact, the range word is the bit
    pattern of max |x * 2^e|, the overflow word stays 0 below 65504 / 2^e and is raised by one value beyond it"""
    x = C.f2h_input(case)
    planes, nhwc4, word, ovf = _f2h(lib, x, case.e)
    want_p, want_n, want_w, want_o = R.frame_to_h2(x, case.e)
    assert np.array_equal(_bits(planes), _bits(want_p))
    assert np.array_equal(_bits(nhwc4), _bits(want_n)) and not _bits(nhwc4[..., case.C:]).any()
    assert (word, ovf) == (want_w, want_o) and ovf == 0
    assert word == int(_bits(np.float32(np.abs(x).max()) * np.float32(2.0 ** case.e))[0])
    big = x.copy()
    big.reshape(-1)[big.size // 2] = -np.nextafter(np.float32(65504.0), np.float32(np.inf)) * np.float32(2.0 ** -case.e)   # the first fp32 beyond
    planes, _, word, ovf = _f2h(lib, big, case.e)
    want_p, _, want_w, want_o = R.frame_to_h2(big, case.e)
    assert np.array_equal(_bits(planes), _bits(want_p)) and (word, ovf) == (want_w, 1) and want_o == 1
    assert np.isfinite(planes).all() and planes.min() == -65504.0


def test_frame_to_h2_non_finite(lib):
    """what a NaN or an Inf becomes (include/sfh_amd.h): +-Inf saturate to +-65504, a NaN becomes -65504 with plane 1 at +0;
    the range word reads the non-finite bit pattern (>= 0x7F800000), the overflow word is raised, the NHWC4 copy keeps the
    input's bits"""
    for e in (-3, 0, 2):
        x = np.linspace(-3.0, 3.0, 2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
        x[0, 0, 1, 2], x[0, 1, 2, 3], x[1, 2, 4, 6] = np.inf, -np.inf, np.nan
        planes, nhwc4, word, ovf = _f2h(lib, x, e)
        want_p, want_n, want_w, _ = R.frame_to_h2(x, e)
        assert np.array_equal(_bits(planes), _bits(want_p)) and np.array_equal(_bits(nhwc4), _bits(want_n))
        assert planes[0, 1, 2, 0, 0] == 65504.0 and planes[0, 2, 3, 0, 1] == -65504.0
        assert planes[1, 4, 6, 0, 2] == -65504.0 and int(_bits(planes[1, 4, 6, 1, 2])[0]) == 0
        assert word == want_w and word > 0x7F800000 and ovf == 1
        x[1, 2, 4, 6] = 0.0                                   # without the NaN: the Inf pattern itself
        assert _f2h(lib, x, e)[2:] == (0x7F800000, 1)


# ------------------------------------------------------------------------------------------------ the first layer
def _c4_pack(lib, case, w):
    """-> (packed weights, wexp or None)"""
    wd = _dev(w)
    if case.kern == "c4":
        packed = torch.full(((case.cout // 64) * 9 * 256,), float("nan"), device="cuda")
        assert lib.sfh_pack_c4_weights(_p(wd), _p(packed), case.c0, case.cout, _st()) == 0, lib.sfh_last_error()
        return packed, None
    n = lib.sfh_packed_c4h2_weight_bytes(case.cout)
    assert n > 0
    packed = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    wexp = K.wexp_for(w)
    assert lib.sfh_pack_c4h2_weights(_p(wd), _p(packed), case.c0, case.cout, wexp, _st()) == 0, lib.sfh_last_error()
    return packed, wexp


def _c4_source(lib, case, x):
    if case.kern == "c4h2":
        return _frame_h2(lib, x, case.e_src)
    full = np.zeros(x.shape[:3] + (4,), np.float32)
    full[..., :case.c0] = x
    return _dev(full)


def _c4_launch(lib, case, src, w, scale, shift, relu, mutate=None, expect=0):
    from sfh_amd._lib import ConvDesc
    packed, wexp = _c4_pack(lib, case, w)
    fold = -(wexp + case.e_src) if case.kern == "c4h2" else 0
    sck, shd = _pow2(scale, fold), _dev(shift)
    dst = _out(lib, case.dst, case.B, case.H, case.W, case.cout + 32, case.e_dst)
    word = _words()
    d = ConvDesc()
    d.src0, d.c0, d.cs0, d.h0, d.w0 = src.data_ptr(), case.c0, 4, case.H, case.W
    d.batch, d.H, d.W, d.ksize, d.stride = case.B, case.H, case.W, 3, 1
    d.wpacked, d.scale, d.shift, d.cout, d.relu = packed.data_ptr(), sck.data_ptr(), shd.data_ptr(), case.cout, int(relu)
    d.dst, d.dst_cs, d.src_fmt, d.dst_fmt = dst.ptr(), case.cout + 32, FMT["fh2" if case.kern == "c4h2" else "f32"], FMT[case.dst]
    d.h2_exp_src, d.h2_exp_dst = case.e_src, case.e_dst
    if case.dst == "h2":
        d.h2_range, d.h2_overflow = word.data_ptr(), word.data_ptr() + 4
    if mutate is not None:
        mutate(d)
    rc = (lib.sfh_conv3x3_c4h2_fwd if case.kern == "c4h2" else lib.sfh_conv3x3_c4_fwd)(ctypes.byref(d), _st())
    _sync()
    assert rc == expect, (rc, lib.sfh_last_error())
    if expect != 0:
        assert dst.untouched()
        return None
    word_, ovf = _read_words(word)
    return dict(y=dst.numpy(case.cout), word=word_, ovf=ovf)


@pytest.mark.parametrize("case", C.C4S, ids=lambda c: c.name)
def test_first_layer_cases(lib, case):
    """int: the fp64 value bit for bit, raw and through scale (one channel 0), shift and ReLU; randn: inside the bound, raw and
    through the epilogue, a second call gives the same bits; H2 destinations leave a correct range word"""
    ones, zeros = np.ones(case.cout, np.float32), np.zeros(case.cout, np.float32)
    worst = {}
    for kind in ("int", "randn"):
        inp = C.c4_inputs(case, kind)
        wexp = K.wexp_for(inp["w"])
        src = _c4_source(lib, case, inp["x"])
        raw = R.first_layer(case, inp, ones, zeros, False, wexp)
        scale, shift = C.plain_epilogue(case.name, raw["acc"], kind)
        for tag, sc, sh, relu in (("raw", ones, zeros, False), ("epilogue", scale, shift, True)):
            ref = raw if tag == "raw" else R.first_layer(case, inp, sc, sh, relu, wexp)
            out = _c4_launch(lib, case, src, inp["w"], sc, sh, relu)
            if case.dst == "h2":
                _check_range_word(out["word"], out["ovf"], ref["y"], ref["bound"], case.e_dst)
            if kind == "int":
                assert np.array_equal(out["y"].astype(np.float64), ref["y"]), tag
            else:
                worst[f"{case.kern} {tag}"] = R.ratio(out["y"], ref["y"], ref["bound"])
                again = _c4_launch(lib, case, src, inp["w"], sc, sh, relu)
                assert np.array_equal(_bits(out["y"]), _bits(again["y"]))
    _report(case.name, **worst)


@pytest.mark.parametrize("case", C.C4_IMPULSE, ids=lambda c: c.name)
def test_first_layer_impulses(lib, case):
    ones, zeros = np.ones(case.cout, np.float32), np.zeros(case.cout, np.float32)
    for code in (K.pixel_coded, K.channel_coded):
        x = code((case.B, case.H, case.W, case.c0))
        src = _c4_source(lib, case, x)
        for o, c in C.impulse_oc(case.cout, case.c0):
            for t in range(9):
                w = np.zeros((case.cout, case.c0, 3, 3), np.float32)
                w[o, c, t // 3, t % 3] = 1.0
                want = R.shifted_copy(x, c, case.cout, o, t // 3, t % 3, 3, 1)
                got = _c4_launch(lib, case, src, w, ones, zeros, False)["y"]
                assert np.array_equal(got.astype(np.float64), want), (o, c, t)


@pytest.mark.parametrize("case", C.C4_WALK, ids=lambda c: c.name)
def test_first_layer_plane_walk(lib, case):
    """sfh_conv3x3_c4h2_fwd over a walk-valued frame (split by sfh_frame_to_h2 at the frame's exponent): bit for bit the fp64
    product"""
    ones, zeros = np.ones(case.cout, np.float32), np.zeros(case.cout, np.float32)
    x = K.walk_values((case.B, case.H, case.W, case.c0), "h2", 23, case.e_src)
    src = _c4_source(lib, case, x)
    for o, c, t in ((0, 0, 0), (case.cout - 1, case.c0 - 1, 8), (63, 1, 5), (case.cout - 64, 2 % case.c0, 7), (17, 0, 4)):
        w = np.zeros((case.cout, case.c0, 3, 3), np.float32)
        w[o, c, t // 3, t % 3] = K.walk_weight("h2")
        want = R.first_layer(case, dict(x=x, w=w), ones, zeros, False, K.wexp_for(w))["y"]
        got = _c4_launch(lib, case, src, w, ones, zeros, False)["y"]
        assert want.any() and np.array_equal(_bits(got), _bits(want)), (o, c, t)


def test_first_layer_refusals(lib):
    h2 = C.C4("c4h2_refuse", "c4h2", 1, 5, 6, 3, 64, "h2", 2, 2)
    f32 = C.C4("c4_refuse", "c4", 1, 5, 6, 3, 64, "f32", 0, 2)
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    keep = torch.zeros(64, device="cuda")
    for case, muts in ((h2, (_set(src_fmt=FMT["f32"]), _set(src_fmt=FMT["h2"]), _set(dst_fmt=FMT["s3"]), _set(cs0=8), _set(c0=5),
                             _set(c0=0), _set(cout=96), _set(stride=2), _set(ksize=1), _set(h0=4), _set(residual=keep.data_ptr()),
                             _set(dst_pool=keep.data_ptr()), _set(acc_init=keep.data_ptr()), _set(h2_exp_src=65), _set(h2_exp_dst=-65))),
                       (f32, (_set(src_fmt=FMT["fh2"]), _set(dst_fmt=FMT["fh2"]), _set(dst_fmt=-1), _set(cs0=8), _set(c0=5), _set(c0=0),
                              _set(cout=96), _set(stride=2), _set(w0=5),
                              _set(dst_pool=keep.data_ptr()), _set(pool0=1), _set(h2_exp_dst=65)))):
        inp = C.c4_inputs(case, "int")
        src = _c4_source(lib, case, inp["x"])
        for m in muts:
            _c4_launch(lib, case, src, inp["w"], ones, zeros, False, mutate=m, expect=-1)


# ------------------------------------------------------------------------------------------------ the fused first DoubleConv
def _inc_launch(lib, case, src, inp, scale, shift, relu, mutate=None, expect=0):
    """sfh_conv_inc_fused_fwd -> dict y, pool, words (mid, out), ovf (mid, out)"""
    from sfh_amd._lib import ConvDesc
    B, H, W = case.B, case.H, case.W
    c4 = C.C4("", "c4h2", B, H, W, case.c0, 64, "h2", case.e_frame, case.e_mid)
    w1p, wexp1 = _c4_pack(lib, c4, inp["w1"])
    w2p, wexp2 = _pack_h2(lib, inp["w2"], 3, 64, 64)
    s1k, h1d = _pow2(inp["s1"], -(wexp1 + case.e_frame)), _dev(inp["h1"])
    sck, shd = _pow2(scale, -(wexp2 + case.e_mid)), _dev(shift)
    dst = _SplitOut(lib, "h2", B, H, W, 96, case.e_dst)
    pool = _SplitOut(lib, "h2", B, H // 2, W // 2, 96, case.e_dst) if case.pool else None
    wmid, wout = _words(), _words()
    a, d = ConvDesc(), ConvDesc()
    a.src0, a.c0, a.cs0, a.h0, a.w0 = src.data_ptr(), case.c0, 4, H, W
    a.batch, a.H, a.W, a.ksize, a.stride = B, H, W, 3, 1
    a.wpacked, a.scale, a.shift, a.cout, a.relu = w1p.data_ptr(), s1k.data_ptr(), h1d.data_ptr(), 64, case.relu
    a.src_fmt, a.dst_fmt, a.h2_exp_src, a.h2_exp_dst = FMT["fh2"], FMT["h2"], case.e_frame, case.e_mid
    a.h2_range, a.h2_overflow = wmid.data_ptr(), wmid.data_ptr() + 4
    d.c0, d.cs0, d.h0, d.w0 = 64, 64, H, W
    d.batch, d.H, d.W, d.ksize, d.stride, d.tile = B, H, W, 3, 1, 0
    d.wpacked, d.scale, d.shift, d.cout, d.relu = w2p.data_ptr(), sck.data_ptr(), shd.data_ptr(), 64, int(relu)
    d.dst, d.dst_cs, d.src_fmt, d.dst_fmt = dst.ptr(), 96, FMT["h2"], FMT["h2"]
    d.h2_exp_src, d.h2_exp_dst, d.reverse_tiles = case.e_mid, case.e_dst, int(case.rev)
    d.h2_range, d.h2_overflow = wout.data_ptr(), wout.data_ptr() + 4
    if pool is not None:
        d.dst_pool, d.pool_cs = pool.ptr(), 96
    if mutate is not None:
        mutate(a, d)
    rc = lib.sfh_conv_inc_fused_fwd(ctypes.byref(a), ctypes.byref(d), _st())
    _sync()
    assert rc == expect, (rc, lib.sfh_last_error())
    if expect != 0:
        assert dst.untouched() and (pool is None or pool.untouched())
        return None
    (m, mo), (o, oo) = _read_words(wmid), _read_words(wout)
    return dict(y=dst.numpy(64), pool=pool.numpy(64) if pool is not None else None, words=(m, o), ovf=(mo, oo), wexp=(wexp1, wexp2))


def _inc_check_words(case, out, ref):
    _check_range_word(out["words"][0], out["ovf"][0], ref["mid"], ref["bound_mid"], case.e_mid)
    _check_range_word(out["words"][1], out["ovf"][1], ref["y"], ref["bound"], case.e_dst)


@pytest.mark.parametrize("case", C.INC, ids=lambda c: c.name)
def test_inc_fused_cases(lib, case):
    """the fp64 DoubleConv with the intermediate's H2 rounding carried through: integers bit for bit (output and pooled
    output), randn inside the bound; both range words within their bounds, both overflow words 0"""
    worst = {}
    for kind in ("int", "randn"):
        inp = C.inc_inputs(case, kind)
        wexp = (K.wexp_for(inp["w1"]), K.wexp_for(inp["w2"]))
        ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
        raw = R.inc_fused(case, inp, ones, zeros, False, *wexp)
        scale, shift = C.plain_epilogue(case.name, raw["acc"], kind, 0.5)
        ref = R.inc_fused(case, inp, scale, shift, True, *wexp)
        out = _inc_launch(lib, case, _frame_h2(lib, inp["x"], case.e_frame), inp, scale, shift, True)
        assert out["wexp"] == wexp
        _inc_check_words(case, out, ref)
        if kind == "int":
            assert np.array_equal(out["y"].astype(np.float64), ref["y"])
            assert out["pool"] is None or np.array_equal(out["pool"].astype(np.float64), ref["pool"])
        else:
            worst["inc_fused"] = R.ratio(out["y"], ref["y"], ref["bound"])
            if out["pool"] is not None:
                worst["inc_fused:pool"] = R.ratio(out["pool"], ref["pool"], ref["pool_bound"])
    _report(case.name, **worst)


def _centre(o, c, shape):
    w = np.zeros(shape, np.float32)
    w[o, c, 1, 1] = 1.0
    return w


@pytest.mark.parametrize("case", C.INC_IMPULSE, ids=lambda c: c.name)
def test_inc_fused_impulses(lib, case):
    """a single 1 at every tap of the first conv under a centre tap of the second, and at every tap of the second over a centre
    tap of the first (scales 1, shifts 0, no ReLU): the exact shifted copy of the frame's channel, zeros where the tap lies
    in the padding - of the frame, or of the INTERMEDIATE: a halo pixel outside the frame holds zero, not conv-of-padding"""
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    s1 = dict(s1=ones, h1=zeros)
    for code in (K.pixel_coded, K.channel_coded):
        x = code((case.B, case.H, case.W, case.c0))
        src = _frame_h2(lib, x, case.e_frame)
        for o, c in C.impulse_oc(64, case.c0):
            for t in range(9):
                w1 = np.zeros((64, case.c0, 3, 3), np.float32)
                w1[o, c, t // 3, t % 3] = 1.0
                o2 = (o + 13) % 64
                want = R.shifted_copy(x, c, 64, o2, t // 3, t % 3, 3, 1)
                out = _inc_launch(lib, case, src, dict(s1, w1=w1, w2=_centre(o2, o, (64, 64, 3, 3))), ones, zeros, False)
                assert np.array_equal(out["y"].astype(np.float64), want), ("first", o, c, t)
                if out["pool"] is not None:
                    assert np.array_equal(out["pool"].astype(np.float64), R.pooled(want, want)[0]), ("first pool", o, c, t)
        for o, c in C.impulse_oc(64, 64):
            for t in range(9):
                w2 = np.zeros((64, 64, 3, 3), np.float32)
                w2[o, c, t // 3, t % 3] = 1.0
                cf = c % case.c0
                want = R.shifted_copy(x, cf, 64, o, t // 3, t % 3, 3, 1)
                out = _inc_launch(lib, case, src, dict(s1, w1=_centre(c, cf, (64, case.c0, 3, 3)), w2=w2), ones, zeros, False)
                assert np.array_equal(out["y"].astype(np.float64), want), ("second", o, c, t)


@pytest.mark.parametrize("case", C.INC_WALK, ids=lambda c: c.name)
def test_inc_fused_plane_walk(lib, case):
    """both convs: a walk-structured weight in one of them, a centre-tap 1 in the other, over a walk-valued frame; the
    intermediate (exponent = the frame's) holds the walk value or the 13-bit product exactly: bit for bit the fp64 value"""
    assert case.e_frame == case.e_mid
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    x = K.walk_values((case.B, case.H, case.W, case.c0), "h2", 24, case.e_frame)
    src = _frame_h2(lib, x, case.e_frame)
    for which in ("first", "second"):
        for o, c, t in ((0, 0, 0), (63, case.c0 - 1, 8), (31, 1, 5), (32, 2 % case.c0, 7), (17, 0, 4)):
            if which == "first":
                w1 = np.zeros((64, case.c0, 3, 3), np.float32)
                w1[o, c, t // 3, t % 3] = K.walk_weight("h2")
                w2 = _centre((o + 13) % 64, o, (64, 64, 3, 3))
            else:
                w1 = _centre(o, c, (64, case.c0, 3, 3))
                w2 = np.zeros((64, 64, 3, 3), np.float32)
                w2[(o + 13) % 64, o, t // 3, t % 3] = K.walk_weight("h2")
            inp = dict(x=x, w1=w1, w2=w2, s1=ones, h1=zeros)
            want = R.inc_fused(case, inp, ones, zeros, False, K.wexp_for(w1), K.wexp_for(w2))["y"]
            got = _inc_launch(lib, case, src, inp, ones, zeros, False)["y"]
            assert want.any() and np.array_equal(_bits(got), _bits(want)), (which, o, c, t)


# ------------------------------------------------------------------------------------------------ the stem
def _stem_launch(lib, case, x, w, scale, shift, relu, mutate=None, expect=0):
    from sfh_amd._lib import ConvDesc
    wide = case.cs0 != 8
    nbytes = (lib.sfh_packed_stem16_weight_bytes if wide else lib.sfh_packed_stem_weight_bytes)()
    packed = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    h2 = case.arith == 2
    wexp = K.wexp_for(w) if h2 else 0
    pack = lib.sfh_pack_stem16_weights if wide else lib.sfh_pack_stem_weights
    assert pack(_p(_dev(w)), _p(packed), case.c0, FMT["h2" if h2 else "s3"], wexp, _st()) == 0, lib.sfh_last_error()
    sck, shd, xd = _pow2(scale, -(wexp + case.e_src) if h2 else 0), _dev(shift), _dev(x)
    ho, wo = C.stem_out_hw(case)
    dst = _F32Out((case.B, ho, wo, case.dst_cs))
    d = ConvDesc()
    d.src0, d.c0, d.cs0, d.h0, d.w0 = xd.data_ptr(), case.c0, case.cs0, case.H, case.W
    d.batch, d.H, d.W, d.ksize, d.stride = case.B, case.H, case.W, 7, 2
    d.wpacked, d.scale, d.shift, d.cout, d.relu = packed.data_ptr(), sck.data_ptr(), shd.data_ptr(), 64, int(relu)
    d.dst, d.dst_cs, d.src_fmt, d.dst_fmt = dst.ptr(), case.dst_cs, FMT["f32"], FMT["f32"]
    d.split_arith, d.h2_exp_src = case.arith, case.e_src
    if mutate is not None:
        mutate(d)
    rc = lib.sfh_stem7x7_fwd(ctypes.byref(d), _st())
    _sync()
    assert rc == expect, (rc, lib.sfh_last_error())
    if expect != 0:
        assert dst.untouched()
        return None
    return dst.numpy(64)


@pytest.mark.parametrize("case", C.STEM, ids=lambda c: c.name)
def test_stem_cases(lib, case):
    """both instances, split_arith 0 / S3 / H2: integers bit for bit, randn inside the bound, raw and through the epilogue"""
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    worst = {}
    for kind in ("int", "randn"):
        inp = C.stem_inputs(case, kind)
        wexp = K.wexp_for(inp["w"])
        raw = R.stem(case, inp, ones, zeros, False, wexp)
        scale, shift = C.plain_epilogue(case.name, raw["acc"], kind)
        for tag, sc, sh, relu in (("raw", ones, zeros, False), ("epilogue", scale, shift, bool(case.relu))):
            ref = raw if tag == "raw" else R.stem(case, inp, sc, sh, relu, wexp)
            got = _stem_launch(lib, case, inp["x"], inp["w"], sc, sh, relu)
            if kind == "int":
                assert np.array_equal(got.astype(np.float64), ref["y"]), tag
            else:
                worst[f"stem{8 if case.cs0 == 8 else 16} {C.stem_fmt(case)} {tag}"] = R.ratio(got, ref["y"], ref["bound"])
    _report(case.name, **worst)


@pytest.mark.parametrize("case", C.STEM_IMPULSE, ids=lambda c: c.name)
def test_stem_impulses(lib, case):
    """all 49 taps, the first and last real channel: the exact stride-2 shifted copy; the stored channels >= c0 hold non-zero
    values here and must contribute nothing"""
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    for code in (K.pixel_coded, K.channel_coded):
        x = code((case.B, case.H, case.W, case.cs0))
        for o, c in ((0, 0), (63, case.c0 - 1), (31, case.c0 // 2), (32, min(8, case.c0 - 1))):
            for t in range(49):
                w = np.zeros((64, case.c0, 7, 7), np.float32)
                w[o, c, t // 7, t % 7] = 1.0
                want = R.shifted_copy(x, c, 64, o, t // 7, t % 7, 7, 2)
                got = _stem_launch(lib, case, x, w, ones, zeros, False)
                assert np.array_equal(got.astype(np.float64), want), (o, c, t)


@pytest.mark.parametrize("case", C.STEM_WALK, ids=lambda c: c.name)
def test_stem_plane_walk(lib, case):
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    fmt = C.stem_fmt(case)
    x = K.walk_values((case.B, case.H, case.W, case.cs0), fmt, 25, case.e_src)
    x[..., case.c0:] = 0.0
    for o, c, t in ((0, 0, 0), (63, case.c0 - 1, 48), (31, case.c0 // 2, 24), (32, min(8, case.c0 - 1), 45), (17, 0, 3)):
        w = np.zeros((64, case.c0, 7, 7), np.float32)
        w[o, c, t // 7, t % 7] = K.walk_weight(fmt)
        want = R.stem(case, dict(x=x, w=w), ones, zeros, False, K.wexp_for(w))["y"]
        got = _stem_launch(lib, case, x, w, ones, zeros, False)
        assert want.any() and np.array_equal(_bits(got), _bits(want)), (o, c, t)


def test_stem_and_inc_fused_refusals(lib):
    ones, zeros = np.ones(64, np.float32), np.zeros(64, np.float32)
    keep = torch.zeros(64, device="cuda")
    st = C.Stem("stem_refuse", 1, 9, 11, 5, 8, 2, 2, 64, 0)
    inp = C.stem_inputs(st, "int")
    for m in (_set(cs0=4), _set(cs0=10), _set(c0=9), _set(c0=0), _set(cout=128), _set(dst_cs=32), _set(dst_fmt=FMT["h2"]),
              _set(src_fmt=FMT["h2"]), _set(split_arith=3), _set(h2_exp_src=65), _set(residual=keep.data_ptr()),
              _set(dst_pool=keep.data_ptr()), _set(h0=8), _set(out_mode=1)):
        _stem_launch(lib, st, inp["x"], inp["w"], ones, zeros, False, mutate=m, expect=-1)
    ic = C.Inc("inc_refuse", 1, 5, 6, 3, 1, 0, 2, 2, 2, 1)
    inp = C.inc_inputs(ic, "int")
    src = _frame_h2(lib, inp["x"], 2)
    first = lambda **kw: (lambda a, d: _set(**kw)(a))
    second = lambda **kw: (lambda a, d: _set(**kw)(d))
    for m in (first(src_fmt=FMT["f32"]), first(dst_fmt=FMT["f32"]), first(cout=128), first(c0=5), first(cs0=8), first(stride=2),
              first(h2_exp_dst=1), first(H=6), first(residual=keep.data_ptr()), second(c0=32), second(cout=128), second(tile=1),
              second(stride=2), second(ksize=1), second(dst_fmt=FMT["f32"]), second(dst_cs=80), second(pool_cs=32),
              second(residual=keep.data_ptr()), second(acc_init=keep.data_ptr()), second(h2_exp_dst=65), second(batch=2)):
        _inc_launch(lib, ic, src, inp, ones, zeros, True, mutate=m, expect=-1)
