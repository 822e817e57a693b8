"""Host side of the specialised-conv pin (no GPU): tests/fused_conv_ref.py against torch at fp64 and against the headers'
sums written out as loops; every bound against the kernels' arithmetic restated in numpy (operands split per
include/sfh_amd.h, the retained product set, fp32 accumulation in two different orders, the seed of the fused Up block, the
H2 intermediate of the fused DoubleConv, every epilogue step rounded to fp32); the proof that the reference alone satisfies
every exact-equality demand of tests/test_gpu_fused_conv.py (integer cases: partial sums below 2^24, stored values below
65504, |pre-ReLU| >= 0.25; impulse copies; plane-walk values that the H2 destination holds exactly); and the sensitivity list:
the restatement takes a defect switch, and for every defect at least one demand of the GPU file, evaluated on the restated
output, fails.

Largest restated error / bound (printed as RATIO lines by this file): upfused / two-launch up block H2 0.017; c4h2 H2 0.504,
c4 fp32 0.618 (K = 9 c0 is as small as 9: the count leaves little room); inc_fused H2 0.004 (pooled 0.003); stem S3 0.035,
stem H2 0.062."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_conv_cases as K
import fused_conv_cases as C
import fused_conv_ref as R
from dense_conv_ref import split_h2, split_s3

f32 = np.float32
KEPT = {"f32": ((0, 0),), "s3": ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)), "h2": ((0, 1), (1, 0), (0, 0))}
ONES, ZEROS = np.ones(64, f32), np.zeros(64, f32)


# ------------------------------------------------------------------------------------------------ the restated arithmetic
def planes(v, fmt, e):
    v = np.asarray(v, dtype=f32)
    return {"f32": lambda: (v,), "s3": lambda: split_s3(v), "h2": lambda: split_h2(v, e)}[fmt]()


def mac(acc, xs, ws, fmt, order, skip=()):
    """acc (P,N) float32 += the retained products of x (P,K) and w (K,N), every partial sum rounded to fp32 (a product of two
    16-bit planes is exact in fp32, an fp32 product rounds once).  order 0: 32 k at a time, inside a block product by product in
    the kernels' order (smallest first), k ascending; order 1: k descending, the products of one k together, largest first.
    skip: (k, (weight plane, source plane)) pairs left out"""
    kept, Kn = KEPT[fmt], xs[0].shape[1]

    def add(k, ij):
        if (k, ij) not in skip:
            acc[...] = (acc + (ws[ij[0]][k][None, :] * xs[ij[1]][:, k][:, None]).astype(f32)).astype(f32)
    if order == 0:
        for k0 in range(0, Kn, 32):
            for ij in kept:
                for k in range(k0, min(k0 + 32, Kn)):
                    add(k, ij)
    else:
        for k in range(Kn - 1, -1, -1):
            for ij in kept[::-1]:
                add(k, ij)
    return acc


def cols(x, ks, stride=1, pad=None):
    """NHWC float32 -> (patches (P, C * ks * ks) in (c, ky, kx) order, (B, Ho, Wo)); pad = (before, after), default the kernels'"""
    pb, pa = (ks // 2, (ks - 1) // 2) if pad is None else pad
    t = F.pad(torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).permute(0, 3, 1, 2), (pb, pa, pb, pa))
    Ho, Wo = (t.shape[2] - ks) // stride + 1, (t.shape[3] - ks) // stride + 1
    u = F.unfold(t, ks, stride=stride)
    return u.permute(0, 2, 1).reshape(-1, u.shape[1]).numpy().copy(), (x.shape[0], Ho, Wo)


def conv_acc(x, w, ks, stride, fmt, ex, wexp, order, pad=None, skip=(), acc0=None):
    """the accumulator of one conv in KERNEL units (H2: real * 2^(ex + wexp)) -> (B,Ho,Wo,cout) float32"""
    p, (B, Ho, Wo) = cols(x, ks, stride, pad)
    wm = np.asarray(w, f32).reshape(w.shape[0], -1).T
    acc = np.zeros((p.shape[0], w.shape[0]), f32) if acc0 is None else acc0.reshape(-1, w.shape[0]).astype(f32)
    mac(acc, planes(p, fmt, ex), planes(wm, fmt, wexp), fmt, order, skip)
    return acc.reshape(B, Ho, Wo, w.shape[0])


def finish(acc, sck, shift, relu, dst, e_dst):
    """the epilogue: product and sum rounded separately, ReLU, the destination's format -> float32 values as read back"""
    y = ((acc * np.asarray(sck, f32)).astype(f32) + np.asarray(shift, f32)).astype(f32)
    if relu:
        y = np.maximum(y, f32(0))
    if dst == "h2":
        p0, p1 = split_h2(y, e_dst)
        y = ((p0 + p1).astype(f32) * f32(2.0 ** -e_dst)).astype(f32)
    elif dst == "s3":
        p = split_s3(y)
        y = ((p[0] + p[1]).astype(f32) + p[2]).astype(f32)
    return y


def fold(scale, e):
    out = np.asarray(scale, np.float64) * 2.0 ** e
    assert np.array_equal(out.astype(f32).astype(np.float64), out)
    return out.astype(f32)


def restate_up(case, inp, scale, shift, relu, order=0, defect=None):
    """conv_upfused_kernel (= the two launches): phase A per output parity, the seed v = acc * up_scale + shift_border[class],
    phase B onto v, the skip half's epilogue, the H2 destination.  defect: 'drop' (w0 x1 of tap (1,1) of the skip phase),
    'swap_parity' (the weights of quadrants 1 and 2), 'nbr_class' (the border class of the pixel one to the right), 'halo_off'
    (the wave of parity (1,1) reads the skip halo one column off), 'last_stage' (the last 32 channels of the skip phase)"""
    B, H, W, cout, c0, c1 = case.B, case.H, case.W, case.cout, case.c0, case.c1
    wexp_up, wexp_sk = K.wexp_for(inp["wq"]), K.wexp_for(inp["w"])
    Hc, Wc = C.up_frame(case)
    P = np.zeros((B, Hc + 2, Wc + 2, c1), f32)
    P[:, 1:1 + case.h1, 1:1 + case.w1] = inp["low"][..., :c1]
    accA = np.zeros((B, H, W, cout), f32)
    for q in range(4):
        dy, dx = q >> 1, q & 1
        qq = {1: 2, 2: 1}.get(q, q) if defect == "swap_parity" else q
        a = conv_acc(P[:, dy:dy + Hc + 1, dx:dx + Wc + 1], inp["wq"][qq * cout:(qq + 1) * cout], 2, 1, "h2", case.e_src, wexp_up,
                     order, pad=(0, 0))
        ny, nx = len(range(dy, H, 2)), len(range(dx, W, 2))
        accA[:, dy::2, dx::2] = a[:, :ny, :nx]
    usk, sbk = fold(inp["us"], wexp_sk - wexp_up), fold(inp["sb"], case.e_src + wexp_sk)
    cls1 = lambda i, up: 0 if i == 0 else (2 if i == up - 1 else (3 if i >= up else 1))
    v = np.empty_like(accA)
    for y in range(H):
        for x in range(W):
            cov = ((y & 1) * 2 + (x & 1)) * cout + np.arange(cout)
            cl = 4 * cls1(y, 2 * case.h1) + cls1(x + (defect == "nbr_class"), 2 * case.w1)
            v[:, y, x] = ((accA[:, y, x] * usk[cov]).astype(f32) + sbk[cl, cov]).astype(f32)
    skip = inp["skip"][..., :c0 - 32 if defect == "last_stage" else c0]
    w = inp["w"][:, :skip.shape[3]]
    drop = {(k, (0, 1)) for k in range(skip.shape[3] * 9) if k % 9 == 4} if defect == "drop" else ()
    acc = conv_acc(skip, w, 3, 1, "h2", case.e_src, wexp_sk, order, skip=drop, acc0=v)
    if defect == "halo_off":
        off = np.zeros_like(skip)
        off[:, :, :-1] = skip[:, :, 1:]
        acc[:, 1::2, 1::2] = conv_acc(off, w, 3, 1, "h2", case.e_src, wexp_sk, order, acc0=v)[:, 1::2, 1::2]
    return finish(acc, fold(scale, -(case.e_src + wexp_sk)), shift, relu, "h2", case.e_dst)


def restate_first(case, inp, scale, shift, relu, order=0, defect=None):
    """conv3x3_c4h2_kernel / conv3x3_c4_kernel.  defect 'drop': w0 x1 of tap (1,1)"""
    fmt = "h2" if case.kern == "c4h2" else "f32"
    wexp = K.wexp_for(inp["w"]) if fmt == "h2" else 0
    drop = {(k, (0, 1)) for k in range(case.c0 * 9) if k % 9 == 4} if defect == "drop" else ()
    acc = conv_acc(inp["x"], inp["w"], 3, 1, fmt, case.e_src, wexp, order, skip=drop)
    return finish(acc, fold(scale, -(wexp + case.e_src) if fmt == "h2" else 0), shift, relu, case.dst, case.e_dst)


def restate_inc(case, inp, scale, shift, relu, order=0, defect=None):
    """conv_inc_fused_kernel: the first conv and its epilogue for the frame AND the ring around it, the ring stored as zeros
    (defect 'ring': kept as computed - conv-of-padding instead of the second conv's zero padding; 'drop': w0 x1 of tap (1,1) of
    the second conv), the second conv over the stored intermediate -> (y, pooled y or None)"""
    wexp1, wexp2 = K.wexp_for(inp["w1"]), K.wexp_for(inp["w2"])
    a1 = conv_acc(inp["x"], inp["w1"], 3, 1, "h2", case.e_frame, wexp1, order, pad=(2, 2))
    mid = finish(a1, fold(inp["s1"], -(wexp1 + case.e_frame)), inp["h1"], bool(case.relu), "h2", case.e_mid)
    if defect != "ring":
        mid[:, 0], mid[:, -1], mid[:, :, 0], mid[:, :, -1] = 0, 0, 0, 0
    drop = {(k, (0, 1)) for k in range(64 * 9) if k % 9 == 4} if defect == "drop" else ()
    a2 = conv_acc(mid, inp["w2"], 3, 1, "h2", case.e_mid, wexp2, order, pad=(0, 0), skip=drop)
    y = finish(a2, fold(scale, -(wexp2 + case.e_mid)), shift, relu, "h2", case.e_dst)
    pool = None
    if case.pool:
        pool = F.max_pool2d(torch.from_numpy(y).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
    return y, pool


def restate_stem(case, inp, scale, shift, relu, order=0, defect=None):
    """stem7x7_kernel / stem7x7_wide_kernel: every stored channel enters (the weights of channels >= c0 are packed as zeros).
    defect 'tap48': a padding tap slot (taps >= 49 read tap 48's pixel) carries tap 48's weight instead of zero; 'drop': w0 x1
    (S3: w2 x0) of tap 24"""
    fmt = C.stem_fmt(case)
    wexp = K.wexp_for(inp["w"]) if fmt == "h2" else 0
    w = np.zeros((64, case.cs0, 7, 7), f32)
    w[:, :case.c0] = inp["w"]
    drop = {(k, KEPT[fmt][0] if fmt == "h2" else (2, 0)) for k in range(case.cs0 * 49) if k % 49 == 24} if defect == "drop" else ()
    acc = conv_acc(inp["x"], w, 7, 2, fmt, case.e_src, wexp, order, pad=(3, 3), skip=drop)
    if defect == "tap48":
        w48 = np.zeros_like(w)
        w48[:, :, 6, 6] = w[:, :, 6, 6]
        acc = conv_acc(inp["x"], w48, 7, 2, fmt, case.e_src, wexp, order, pad=(3, 3), acc0=acc)
    return finish(acc, fold(scale, -(wexp + case.e_src) if fmt == "h2" else 0), shift, relu, "f32", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the references
def test_up_block_reference_against_the_headers_sum():
    """border_class / up_tables / upfused against include/sfh_amd.h and the header of csrc/conv_upfused.hip written out as
    loops, torch's conv2d for the skip half; every border class occurs"""
    case = C.Up("t", 2, 5, 7, 2, 3, 3, 2, 2, 0, 2, 2)
    r = np.random.default_rng(1)
    inp = dict(skip=r.standard_normal((2, 5, 7, 5)), low=r.standard_normal((2, 2, 3, 4)), w=r.standard_normal((2, 3, 3, 3)),
               wq=r.standard_normal((8, 2, 2, 2)), us=r.standard_normal(8), sb=r.standard_normal((16, 8)))
    scale, shift = r.standard_normal(2), r.standard_normal(2)
    got = R.upfused(case, inp, scale, shift, True, 0, 0)
    sk = F.conv2d(torch.from_numpy(inp["skip"][..., :3]).permute(0, 3, 1, 2), torch.from_numpy(inp["w"]), None, 1, 1)
    sk = sk.permute(0, 2, 3, 1).numpy()
    seen = set()
    for y in range(5):
        for x in range(7):
            py, px = y & 1, x & 1
            cy = 0 if y == 0 else (2 if y == 3 else (3 if y >= 4 else 1))
            cx = 0 if x == 0 else (2 if x == 5 else (3 if x >= 6 else 1))
            seen.add(4 * cy + cx)
            for co in range(2):
                cov = (py * 2 + px) * 2 + co
                s = np.zeros(2)
                for a in range(2):
                    for b in range(2):
                        yy, xx = (y >> 1) + py - 1 + a, (x >> 1) + px - 1 + b
                        if 0 <= yy < 2 and 0 <= xx < 3:
                            s += inp["low"][:, yy, xx, :2] @ inp["wq"][cov, :, a, b]
                v = s * inp["us"][cov] + inp["sb"][4 * cy + cx, cov]
                assert np.allclose(got["v"][:, y, x, co], v, rtol=0, atol=1e-13)
                want = np.maximum((v + sk[:, y, x, co]) * scale[co] + shift[co], 0.0)
                assert np.allclose(got["y"][:, y, x, co], want, rtol=0, atol=1e-12)
    assert seen == {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}
    assert list(R.border_class(5, 4)) == [0, 1, 1, 2, 3] and list(R.border_class(2, 2)) == [0, 2] and list(R.border_class(3, 2)) == [0, 2, 3]


def test_fused_double_conv_reference_against_torch():
    case = C.Inc("t", 2, 5, 6, 3, 1, 0, 2, 2, 2, 1)
    r = np.random.default_rng(2)
    inp = dict(x=r.standard_normal((2, 5, 6, 3)), w1=r.standard_normal((64, 3, 3, 3)), w2=r.standard_normal((64, 64, 3, 3)) / 24,
               s1=r.standard_normal(64), h1=r.standard_normal(64))
    scale, shift = r.standard_normal(64), r.standard_normal(64)
    got = R.inc_fused(case, inp, scale, shift, True, 0, 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ch = lambda v: t(v).view(1, -1, 1, 1)
    mid = torch.relu(F.conv2d(t(inp["x"]).permute(0, 3, 1, 2), t(inp["w1"]), None, 1, 1) * ch(inp["s1"]) + ch(inp["h1"]))
    y = torch.relu(F.conv2d(mid, t(inp["w2"]), None, 1, 1) * ch(scale) + ch(shift))
    assert np.allclose(got["mid"], mid.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    assert np.allclose(got["y"], y.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-11)
    assert np.allclose(got["pool"], F.max_pool2d(y, 2).permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-11)
    assert got["pool"].shape == (2, 2, 3, 64) and (got["bound"] > got["bound_mid"].min() * 0).all()
    # the intermediate's error enters the second conv: a larger bound_mid gives a larger bound, everywhere
    case0 = case._replace(e_mid=-6)
    assert (R.inc_fused(case0, inp, scale, shift, True, 0, 0)["bound"] > got["bound"]).all()


def test_frame_to_h2_reference():
    x = C.f2h_input(C.F2HS[7])
    e = C.F2HS[7].e
    p, n, word, ovf = R.frame_to_h2(x, e)
    assert p.shape == (1, 15, 17, 2, 4) and not p[..., 3].any() and not n[..., 3].any()
    p0, p1 = split_h2(x[0, 1], e)
    assert np.array_equal(p[0, :, :, 0, 1], p0) and np.array_equal(p[0, :, :, 1, 1], p1)
    assert ovf == 0 and word == int(_bits(f32(np.abs(x).max()) * f32(2.0 ** e))[0])
    assert np.array_equal(_bits(n[..., :3]), _bits(np.transpose(x, (0, 2, 3, 1))))
    x[0, 0, 0, 0], x[0, 1, 0, 0], x[0, 2, 0, 0] = np.nan, np.inf, -65520.0 * 2.0 ** -e
    p, n, word, ovf = R.frame_to_h2(x, e)
    assert (p[0, 0, 0, 0, :3] == (-65504.0, 65504.0, -65504.0)).all() and not p[0, 0, 0, 1, :3].any()
    assert ovf == 1 and word == 0x7FC00000 and np.isnan(n[0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ the exact-equality demands
def _h2_exact(y, e):
    """every value survives the H2 destination: below 65504 / 2^e and held by the two planes"""
    y = np.asarray(y, np.float64)
    y32 = y.astype(f32)
    p0, p1 = split_h2(y32, e)
    return (np.array_equal(y32.astype(np.float64), y) and float(np.abs(y).max()) * 2.0 ** e < 65504.0
            and np.array_equal((p0.astype(np.float64) + p1) * 2.0 ** -e, y))


def _integer_ok(ref, pre_unit=0.25):
    """every partial sum an exact fp32 number in any order: values on a grid of `pre_unit`, A / pre_unit below 2^24"""
    return float(ref["A"].max()) / pre_unit < 2 ** 24 and np.array_equal(ref["acc"] / pre_unit, np.round(ref["acc"] / pre_unit))


def _pre_relu(acc, scale, shift):
    return acc * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)


@pytest.mark.parametrize("case", C.UP, ids=lambda c: c.name)
def test_up_block_integer_cases_are_exact(case):
    inp = C.up_inputs(case, "int")
    wexp = (K.wexp_for(inp["wq"]), K.wexp_for(inp["w"]))
    raw = R.upfused(case, inp, np.ones(case.cout, f32), np.zeros(case.cout, f32), False, *wexp)
    assert _integer_ok(raw, 1.0) and np.array_equal(raw["v"], np.round(raw["v"]))
    scale, shift = C.up_epilogue(case, raw["acc"], "int")
    ref = R.upfused(case, inp, scale, shift, bool(case.relu), *wexp)
    pre = _pre_relu(raw["acc"], scale, shift)
    assert float(np.abs(pre).min()) >= 0.25 and _h2_exact(ref["y"], case.e_dst)
    if case.relu:
        assert 0.1 < float((ref["y"] > 0).mean()) < 0.9
    # the folded tables are exact powers of two times the inputs, and the H2 sources hold the integers and the junk stage
    for t, e in ((inp["skip"], case.e_src), (inp["low"], case.e_src), (inp["w"], wexp[1]), (inp["wq"], wexp[0])):
        p0, p1 = split_h2(t, e)
        assert not p1.any() and np.array_equal(p0 * f32(2.0 ** -e), t)


def test_up_block_weight_exponents_differ_where_the_case_says_so():
    case = {c.name: c for c in C.UP}["up_17x33_b3"]
    inp = C.up_inputs(case, "randn")
    assert len({case.e_src, case.e_dst, K.wexp_for(inp["wq"]), K.wexp_for(inp["w"])}) == 4


@pytest.mark.parametrize("case", C.C4S, ids=lambda c: c.name)
def test_first_layer_integer_cases_are_exact(case):
    inp = C.c4_inputs(case, "int")
    ones, zeros = np.ones(case.cout, f32), np.zeros(case.cout, f32)
    raw = R.first_layer(case, inp, ones, zeros, False, K.wexp_for(inp["w"]))
    assert _integer_ok(raw, 1.0)
    scale, shift = C.plain_epilogue(case.name, raw["acc"], "int")
    y = R.first_layer(case, inp, scale, shift, True, K.wexp_for(inp["w"]))["y"]
    assert float(np.abs(_pre_relu(raw["acc"], scale, shift)).min()) >= 0.25
    assert case.dst != "h2" or (_h2_exact(raw["y"], case.e_dst) and _h2_exact(y, case.e_dst))
    if case.dst == "s3":
        p = split_s3(y.astype(f32))
        assert np.array_equal(p[0].astype(np.float64) + p[1] + p[2], y)
    if case.kern == "c4h2":
        assert not split_h2(inp["x"], case.e_src)[1].any() and float(np.abs(inp["x"]).max()) * 2.0 ** case.e_src < 2048


@pytest.mark.parametrize("case", C.INC, ids=lambda c: c.name)
def test_fused_double_conv_integer_cases_are_exact(case):
    inp = C.inc_inputs(case, "int")
    wexp = (K.wexp_for(inp["w1"]), K.wexp_for(inp["w2"]))
    raw = R.inc_fused(case, inp, ONES, ZEROS, False, *wexp)
    assert float(raw["A1"].max()) < 2 ** 24 and np.array_equal(raw["a1"], np.round(raw["a1"]))
    assert float(np.abs(_pre_relu(raw["a1"], inp["s1"], inp["h1"])).min()) >= 0.5
    p0, p1 = split_h2(raw["mid"].astype(f32), case.e_mid)
    assert not p1.any() and np.array_equal(p0.astype(np.float64) * 2.0 ** -case.e_mid, raw["mid"])     # the first plane holds it
    assert _integer_ok(raw, 0.5)
    scale, shift = C.plain_epilogue(case.name, raw["acc"], "int", 0.5)
    ref = R.inc_fused(case, inp, scale, shift, True, *wexp)
    assert float(np.abs(_pre_relu(raw["acc"], scale, shift)).min()) >= 0.25 and _h2_exact(ref["y"], case.e_dst)
    assert 0.1 < float((ref["y"] > 0).mean()) < 0.9


@pytest.mark.parametrize("case", C.STEM, ids=lambda c: c.name)
def test_stem_integer_cases_are_exact(case):
    inp = C.stem_inputs(case, "int")
    raw = R.stem(case, inp, ONES, ZEROS, False, K.wexp_for(inp["w"]))
    assert _integer_ok(raw, 1.0) and not inp["x"][..., case.c0:].any()
    scale, shift = C.plain_epilogue(case.name, raw["acc"], "int")
    assert float(np.abs(_pre_relu(raw["acc"], scale, shift)).min()) >= 0.25
    y = R.stem(case, inp, scale, shift, bool(case.relu), K.wexp_for(inp["w"]))["y"]
    assert np.array_equal(y.astype(f32).astype(np.float64), y)


def test_impulse_copies_are_what_the_references_compute():
    """shifted_copy / up_shifted_copy, which the GPU tests compare with, are the references on the impulse weights (integers
    below 2^11: exact in every format and through every H2 destination)"""
    for case in C.UP_IMPULSE:
        ones, zeros = np.ones(case.cout, f32), np.zeros(case.cout, f32)
        tab = dict(us=np.ones(4 * case.cout, f32), sb=np.zeros((16, 4 * case.cout), f32))
        data = dict(skip=K.pixel_coded((case.B, case.H, case.W, case.c0 + 32)) + K.channel_coded((case.B, case.H, case.W, case.c0 + 32)),
                    low=K.pixel_coded((case.B, case.h1, case.w1, case.c1 + 32)) + 7.0)
        halves = set()
        for n, (half, w, wq, o, c, ky, kx) in enumerate(C.up_impulses(case)):
            halves.add((half, o // case.cout if half == "up" else 0))
            if n % 7:
                continue
            got = R.upfused(case, dict(data, w=w, wq=wq, **tab), ones, zeros, False, 0, 0)["y"]
            want = (R.up_shifted_copy(case, data["low"], c, o, ky, kx) if half == "up"
                    else R.shifted_copy(data["skip"][..., :case.c0], c, case.cout, o, ky, kx, 3, 1))
            assert np.array_equal(got, want) and want.any() and _h2_exact(want, case.e_dst)
        assert halves == {("up", 0), ("up", 1), ("up", 2), ("up", 3), ("skip", 0)}
    for case in C.C4_IMPULSE:
        x = K.pixel_coded((case.B, case.H, case.W, case.c0))
        assert float(x.max()) < 2048
        for o, c in C.impulse_oc(case.cout, case.c0):
            w = np.zeros((case.cout, case.c0, 3, 3), f32)
            w[o, c, 0, 2] = 1.0
            got = R.first_layer(case, dict(x=x, w=w), np.ones(case.cout, f32), np.zeros(case.cout, f32), False, 13)["y"]
            assert np.array_equal(got, R.shifted_copy(x, c, case.cout, o, 0, 2, 3, 1)) and got.any()
    for case in C.INC_IMPULSE:
        x = K.pixel_coded((case.B, case.H, case.W, case.c0))
        w1, w2 = np.zeros((64, case.c0, 3, 3), f32), np.zeros((64, 64, 3, 3), f32)
        w1[5, 1, 2, 0], w2[9, 5, 1, 1] = 1.0, 1.0
        got = R.inc_fused(case, dict(x=x, w1=w1, w2=w2, s1=ONES, h1=ZEROS), ONES, ZEROS, False, 13, 13)
        want = R.shifted_copy(x, 1, 64, 9, 2, 0, 3, 1)
        assert np.array_equal(got["y"], want) and want.any() and _h2_exact(want, case.e_mid) and _h2_exact(want, case.e_dst)
        w1, w2 = np.zeros_like(w1), np.zeros_like(w2)
        w1[5, 1, 1, 1], w2[9, 5, 0, 2] = 1.0, 1.0
        got = R.inc_fused(case, dict(x=x, w1=w1, w2=w2, s1=ONES, h1=ZEROS), ONES, ZEROS, False, 13, 13)
        assert np.array_equal(got["y"], R.shifted_copy(x, 1, 64, 9, 0, 2, 3, 1))
    for case in C.STEM_IMPULSE:
        x = K.pixel_coded((case.B, case.H, case.W, case.cs0))
        for t in (0, 24, 48):
            w = np.zeros((64, case.c0, 7, 7), f32)
            w[63, case.c0 - 1, t // 7, t % 7] = 1.0
            got = R.stem(case, dict(x=x, w=w), ONES, ZEROS, False, 13)["y"]
            assert np.array_equal(got, R.shifted_copy(x, case.c0 - 1, 64, 63, t // 7, t % 7, 7, 2)) and got.any()
            assert got.shape[1:3] == C.stem_out_hw(case)


# ------------------------------------------------------------------------------------------------ demands, as the GPU file asks them
SENS_UP = C.Up("up_sens", 1, 5, 7, 2, 3, 64, 32, 64, 1, 2, 2)
SENS_C4 = C.C4("c4h2_sens", "c4h2", 1, 4, 5, 3, 64, "h2", 2, 2)
SENS_INC = C.Inc("inc_sens", 1, 4, 5, 3, 1, 0, 2, 2, 2, 1)
SENS_STEM = [C.Stem("stem8_sens", 1, 7, 9, 5, 8, 2, 2, 64, 1), C.Stem("stem16_sens", 1, 7, 9, 9, 12, 1, 0, 64, 1)]


def up_demands(case, run):
    """the demands of tests/test_gpu_fused_conv.py on the fused Up block, evaluated on run(inp, scale, shift, relu) -> {name: met}"""
    ones, zeros = np.ones(case.cout, f32), np.zeros(case.cout, f32)
    met = {}
    for kind in ("int", "randn"):
        inp = C.up_inputs(case, kind)
        wexp = (K.wexp_for(inp["wq"]), K.wexp_for(inp["w"]))
        scale, shift = C.up_epilogue(case, R.upfused(case, inp, ones, zeros, False, *wexp)["acc"], kind)
        ref = R.upfused(case, inp, scale, shift, bool(case.relu), *wexp)
        got = run(inp, scale, shift, bool(case.relu))
        if kind == "int":
            met["int"] = np.array_equal(got.astype(np.float64), ref["y"])
        else:
            met["randn"] = bool((np.abs(got.astype(np.float64) - ref["y"]) <= ref["bound"]).all())
    tab = dict(us=np.ones(4 * case.cout, f32), sb=np.zeros((16, 4 * case.cout), f32))
    sk, lo = (case.B, case.H, case.W, case.c0 + 32), (case.B, case.h1, case.w1, case.c1 + 32)
    data = dict(skip=K.pixel_coded(sk), low=K.pixel_coded(lo) + 7.0)
    ok = True
    for n, (half, w, wq, o, c, ky, kx) in enumerate(C.up_impulses(case)):
        if n % 3 == 0:
            want = (R.up_shifted_copy(case, data["low"], c, o, ky, kx) if half == "up"
                    else R.shifted_copy(data["skip"][..., :case.c0], c, case.cout, o, ky, kx, 3, 1))
            ok = ok and np.array_equal(run(dict(data, w=w, wq=wq, **tab), ones, zeros, False).astype(np.float64), want)
    met["impulse"] = ok
    wdata = dict(skip=K.walk_values(sk, "h2", 21, case.e_src), low=K.walk_values(lo, "h2", 22, case.e_src))
    ok = True
    for half, (o, c, ky, kx) in (("up", (case.cout + 63, 31, 1, 1)), ("skip", (5, 7, 1, 1)), ("skip", (case.cout - 1, case.c0 - 1, 2, 2))):
        w, wq = np.zeros((case.cout, case.c0, 3, 3), f32), np.zeros((4 * case.cout, case.c1, 2, 2), f32)
        (wq if half == "up" else w)[o, c, ky, kx] = K.walk_weight("h2")
        inp = dict(wdata, w=w, wq=wq, **tab)
        want = R.upfused(case, inp, ones, zeros, False, K.wexp_for(wq), K.wexp_for(w))["y"]
        assert want.any() and _h2_exact(want.astype(f32), case.e_dst)
        ok = ok and np.array_equal(_bits(run(inp, ones, zeros, False)), _bits(want))
    met["walk"] = ok
    return met


def plain_demands(case, inputs, reference, run, cin, ks, stride, xkey, e_src, fmt, unit=1.0, wkey="w", fixed=None):
    """the same four families for a launch with one weight tensor under test (fixed: the other inputs of an impulse / walk
    launch): int, randn, impulses at a few taps, the plane walk"""
    met = {}
    cout = 64 if not hasattr(case, "cout") else case.cout
    ones, zeros = np.ones(cout, f32), np.zeros(cout, f32)
    for kind in ("int", "randn"):
        inp = inputs(case, kind)
        raw = reference(inp, ones, zeros, False)
        scale, shift = C.plain_epilogue(case.name, raw["acc"], kind, unit)
        ref = reference(inp, scale, shift, True)
        got = run(inp, scale, shift, True)
        met[kind] = (np.array_equal(got.astype(np.float64), ref["y"]) if kind == "int"
                     else bool((np.abs(got.astype(np.float64) - ref["y"]) <= ref["bound"]).all()))
    shape = inputs(case, "int")[xkey].shape
    x = K.pixel_coded(shape)
    ok = True
    for o, c, t in ((0, 0, 0), (cout - 1, cin - 1, ks * ks - 1), (31, cin // 2, (ks * ks) // 2)):
        w = np.zeros((cout, cin, ks, ks), f32)
        w[o, c, t // ks, t % ks] = 1.0
        inp = dict(fixed(o) if fixed else {}, **{xkey: x, wkey: w})
        want = reference(inp, ones, zeros, False)["y"]
        assert want.any()
        ok = ok and np.array_equal(run(inp, ones, zeros, False).astype(np.float64), want)
    met["impulse"] = ok
    xw = K.walk_values(shape, fmt, 23, e_src)
    if xkey == "x" and shape[3] > cin:
        xw[..., cin:] = 0.0
    ok = True
    for o, c, t in ((0, 0, 0), (cout - 1, cin - 1, ks * ks - 1), (31, cin // 2, (ks * ks) // 2)):
        w = np.zeros((cout, cin, ks, ks), f32)
        w[o, c, t // ks, t % ks] = K.walk_weight(fmt)
        inp = dict(fixed(o) if fixed else {}, **{xkey: xw, wkey: w})
        want = reference(inp, ones, zeros, False)["y"]
        assert want.any()
        ok = ok and np.array_equal(_bits(run(inp, ones, zeros, False)), _bits(want))
    met["walk"] = ok
    return met


def _first_demands(case, defect):
    ref = lambda inp, sc, sh, relu: R.first_layer(case, inp, sc, sh, relu, K.wexp_for(inp["w"]))
    run = lambda inp, sc, sh, relu: restate_first(case, inp, sc, sh, relu, 0, defect)
    return plain_demands(case, C.c4_inputs, ref, run, case.c0, 3, 1, "x", case.e_src, "h2")


def _stem_demands(case, defect):
    ref = lambda inp, sc, sh, relu: R.stem(case, inp, sc, sh, relu, K.wexp_for(inp["w"]))
    run = lambda inp, sc, sh, relu: restate_stem(case, inp, sc, sh, relu, 0, defect)
    return plain_demands(case, C.stem_inputs, ref, run, case.c0, 7, 2, "x", case.e_src, C.stem_fmt(case))


def _inc_demands(case, defect):
    """the second conv's weights under test over a centre-tap first conv (impulse, walk); int and randn on both"""
    centre = np.zeros((64, case.c0, 3, 3), f32)
    for o in range(64):
        centre[o, o % case.c0, 1, 1] = 1.0
    fixed = lambda o: dict(w1=centre, s1=ONES, h1=ZEROS)
    nore = case._replace(relu=0)          # the impulse and walk launches keep the intermediate's sign, as on the GPU
    which = lambda inp: nore if inp["s1"] is ONES else case
    ref = lambda inp, sc, sh, relu: R.inc_fused(which(inp), inp, sc, sh, relu, K.wexp_for(inp["w1"]), K.wexp_for(inp["w2"]))
    run = lambda inp, sc, sh, relu: restate_inc(which(inp), inp, sc, sh, relu, 0, defect)[0]
    return plain_demands(case, C.inc_inputs, ref, run, 64, 3, 1, "x", case.e_frame, "h2", 0.5, "w2", fixed)


def test_the_restatements_meet_every_demand():
    assert all(up_demands(SENS_UP, lambda *a: restate_up(SENS_UP, *a)).values())
    assert all(_first_demands(SENS_C4, None).values())
    assert all(_inc_demands(SENS_INC, None).values())
    for case in SENS_STEM:
        assert all(_stem_demands(case, None).values()), case.name


@pytest.mark.parametrize("defect", ["drop", "swap_parity", "nbr_class", "halo_off", "last_stage"])
def test_up_block_defects_are_caught(defect):
    """drop the smallest retained product at one tap -> the plane walk; exchange the weights of two parity classes, read the
    halo one column off in one wave, skip the last K stage of the skip phase -> integers and impulses; take the border class of
    the neighbouring pixel -> integers and the randn bound"""
    met = up_demands(SENS_UP, lambda *a: restate_up(SENS_UP, *a, 0, defect))
    print(defect, met)
    assert not all(met.values())
    if defect == "drop":
        assert met["int"] and met["impulse"] and not met["walk"]          # the only family that sees it
    if defect == "nbr_class":
        assert not met["int"] and not met["randn"]


@pytest.mark.parametrize("launch,defect", [("c4h2", "drop"), ("inc", "drop"), ("inc", "ring"), ("stem8", "drop"), ("stem16", "drop"),
                                           ("stem8", "tap48"), ("stem16", "tap48")])
def test_first_layer_double_conv_and_stem_defects_are_caught(launch, defect):
    """a dropped cross product -> the plane walk (integers and impulses never see it; at K = 27 the randn bound does too); tap 48's weight in a padding tap slot (stem) -> integers and the tap-48
    impulse; conv-of-padding in the intermediate's ring (inc_fused) -> integers (ReLU(shift) is not zero)"""
    met = {"c4h2": lambda: _first_demands(SENS_C4, defect), "inc": lambda: _inc_demands(SENS_INC, defect),
           "stem8": lambda: _stem_demands(SENS_STEM[0], defect), "stem16": lambda: _stem_demands(SENS_STEM[1], defect)}[launch]()
    print(launch, defect, met)
    assert not all(met.values())
    if defect == "drop":
        assert met["int"] and met["impulse"] and not met["walk"]
    else:
        assert not met["int"]


# ------------------------------------------------------------------------------------------------ the bounds
UP_BY_NAME = {c.name: c for c in C.UP}
C4_BY_NAME = {c.name: c for c in C.C4S}
INC_BY_NAME = {c.name: c for c in C.INC}
STEM_BY_NAME = {c.name: c for c in C.STEM}


@pytest.mark.parametrize("name", ["up_17x33", "up_3x3", "up_19x2", "up_2x35"])
def test_up_block_bound_holds_for_the_restated_arithmetic(name):
    case = UP_BY_NAME[name]
    inp = C.up_inputs(case, "randn")
    wexp = (K.wexp_for(inp["wq"]), K.wexp_for(inp["w"]))
    ones, zeros = np.ones(case.cout, f32), np.zeros(case.cout, f32)
    scale, shift = C.up_epilogue(case, R.upfused(case, inp, ones, zeros, False, *wexp)["acc"], "randn")
    ref = R.upfused(case, inp, scale, shift, bool(case.relu), *wexp)
    worst = max(R.ratio(restate_up(case, inp, scale, shift, bool(case.relu), order), ref["y"], ref["bound"]) for order in (0, 1))
    print(f"RATIO {name}: restated upfused h2 {worst:.3f}")
    assert worst <= 1.0
    inp = C.up_inputs(case, "int")
    wexp = (K.wexp_for(inp["wq"]), K.wexp_for(inp["w"]))
    scale, shift = C.up_epilogue(case, R.upfused(case, inp, ones, zeros, False, *wexp)["acc"], "int")
    got = restate_up(case, inp, scale, shift, bool(case.relu), 1)
    assert np.array_equal(got.astype(np.float64), R.upfused(case, inp, scale, shift, bool(case.relu), *wexp)["y"])


@pytest.mark.parametrize("name", ["c4h2_1x9x33_h2", "c4h2_3x5x6_f32", "c4h2_2x45x80_h2", "c4_1x9x33_s3", "c4_3x5x6_h2", "c4_2x45x80_f32"])
def test_first_layer_bound_holds_for_the_restated_arithmetic(name):
    case = C4_BY_NAME[name]
    inp = C.c4_inputs(case, "randn")
    wexp = K.wexp_for(inp["w"])
    raw = R.first_layer(case, inp, np.ones(case.cout, f32), np.zeros(case.cout, f32), False, wexp)
    scale, shift = C.plain_epilogue(case.name, raw["acc"], "randn")
    ref = R.first_layer(case, inp, scale, shift, True, wexp)
    worst = max(R.ratio(restate_first(case, inp, scale, shift, True, order), ref["y"], ref["bound"]) for order in (0, 1))
    print(f"RATIO {name}: restated {case.kern} {'h2' if case.kern == 'c4h2' else 'f32'} {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["inc_1x9x33_pool_rev", "inc_3x5x6", "inc_1x7x31", "inc_2x9x1"])
def test_fused_double_conv_bound_holds_for_the_restated_arithmetic(name):
    case = INC_BY_NAME[name]
    inp = C.inc_inputs(case, "randn")
    wexp = (K.wexp_for(inp["w1"]), K.wexp_for(inp["w2"]))
    scale, shift = C.plain_epilogue(case.name, R.inc_fused(case, inp, ONES, ZEROS, False, *wexp)["acc"], "randn", 0.5)
    ref = R.inc_fused(case, inp, scale, shift, True, *wexp)
    worst, wpool = 0.0, 0.0
    for order in (0, 1):
        y, pool = restate_inc(case, inp, scale, shift, True, order)
        worst = max(worst, R.ratio(y, ref["y"], ref["bound"]))
        if pool is not None:
            wpool = max(wpool, R.ratio(pool, ref["pool"], ref["pool_bound"]))
    print(f"RATIO {name}: restated inc_fused h2 {worst:.3f} pool {wpool:.3f}")
    assert worst <= 1.0 and wpool <= 1.0


@pytest.mark.parametrize("name", ["stem8_17x65_a1e0", "stem8_18x66_a2e2", "stem8_1x37_a2e0", "stem16_17x33_a0e0", "stem16_18x34_a2e0",
                                  "stem16_9x1_a2e2"])
def test_stem_bound_holds_for_the_restated_arithmetic(name):
    case = STEM_BY_NAME[name]
    inp = C.stem_inputs(case, "randn")
    wexp = K.wexp_for(inp["w"])
    scale, shift = C.plain_epilogue(case.name, R.stem(case, inp, ONES, ZEROS, False, wexp)["acc"], "randn")
    ref = R.stem(case, inp, scale, shift, bool(case.relu), wexp)
    worst = max(R.ratio(restate_stem(case, inp, scale, shift, bool(case.relu), order), ref["y"], ref["bound"]) for order in (0, 1))
    print(f"RATIO {name}: restated stem {C.stem_fmt(case)} {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the case lists
def test_case_lists_cover_the_kernels_constants():
    th, tw = C.UP_TILE
    frames = {(c.H, c.W) for c in C.UP}
    assert {(th, tw), (th - 1, tw - 1), (th + 1, tw + 1), (th + 2, tw + 2), (th, tw + 1), (th + 1, tw), (2, 2), (3, 3)} <= frames
    for c in C.UP + C.UP_IMPULSE + C.UP_WALK:
        assert c.H - 2 * c.h1 in (0, 1) and c.W - 2 * c.w1 in (0, 1) and c.c0 % 32 == 0 and c.c1 % 32 == 0 and c.cout % 64 == 0
    for field, vals in (("c0", {32, 96}), ("c1", {32, 64}), ("cout", {64, 128}), ("relu", {0, 1})):
        assert {getattr(c, field) for c in C.UP} == vals
    b3 = UP_BY_NAME["up_17x33_b3"]
    tiles = b3.B * -(-b3.H // th) * -(-b3.W // tw)
    assert tiles == 12 and -(-tiles // 8) * 8 - tiles == 4
    th, tw = C.C4_TILE
    for kern, dsts in C.C4_DST.items():
        for f in C.C4_FRAMES:
            assert {c.dst for c in C.C4S if c.kern == kern and (c.B, c.H, c.W) == f} == set(dsts)
        assert {c.c0 for c in C.C4S if c.kern == kern} == {1, 3, 4} and {c.cout for c in C.C4S if c.kern == kern} == {64, 128}
    assert {(1, th - 1, tw - 1), (1, th + 1, tw + 1)} <= set(C.C4_FRAMES) and {(c.B, c.H, c.W) for c in C.INC} == set(C.C4_FRAMES)
    assert {(c.H, c.W) for c in C.INC if c.pool} == {(45, 80), (9, 33)} and any(c.rev for c in C.INC) and {c.c0 for c in C.INC} == {3, 4}
    assert {c.B * c.H * c.W for c in C.F2HS} == {1, 255, 257, 7200} and {c.e for c in C.F2HS} == {-3, 0, 2}
    for cs, chans in ((8, {(1, 8), (5, 8), (8, 8)}), (16, {(9, 12), (12, 12), (13, 16), (16, 16)})):
        mine = [c for c in C.STEM if (c.cs0 == 8) == (cs == 8)]
        th, tw = C.STEM_TILE[cs]
        outs = {C.stem_out_hw(c) for c in mine}
        assert {(th - 1, tw - 1), (th + 1, tw + 1)} <= outs and {(c.H, c.W) for c in mine} >= {(1, 1), (1, 37), (9, 1)}
        assert {(c.c0, c.cs0) for c in mine} == chans and {(c.arith, c.e_src) for c in mine} == {(0, 0), (1, 0), (2, 0), (2, 2)}
        assert {c.H % 2 for c in mine} == {0, 1} and {c.dst_cs for c in mine} == {64, 96} and {c.relu for c in mine} == {0, 1}
        assert all(c.B == 3 for c in mine)
