"""Host side of the dense-conv pin (no GPU): tests/dense_conv_ref.py against torch at fp64; the plane-walk constants of
tests/dense_conv_cases.py, properties (a) to (c); every bound against the kernel's arithmetic restated in numpy (the split
into planes per include/sfh_amd.h, the retained product set, fp32 accumulation in two different orders); and the proof
that the reference alone satisfies every exact-equality demand of tests/test_gpu_dense_conv.py.

Largest restated error / bound (printed as RATIO lines by this file): forward fp32 0.079, S3 0.018, H2 0.037;
backward-filter fp32 0.009, S3 0.006, H2 0.013."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_conv_cases as K
import dense_conv_ref as R
from dense_conv_ref import split_h2, split_s3

f32 = np.float32
S3_KEPT = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))      # (weight plane, source plane), in the stage loop's order
H2_KEPT = ((0, 1), (1, 0), (0, 0))
BY_NAME = {c.name: c for c in K.FWD}
WG_BY_NAME = {c.name: c for c in K.WGRAD}


def _planes(v, fmt, e):
    return {"f32": lambda: (np.asarray(v, dtype=f32),), "s3": lambda: split_s3(v), "h2": lambda: split_h2(v, e)}[fmt]()


def restate_matmul(a, b, fmt, order, ea=2, eb=2, kept=None):
    """out[p][n] = sum_k a[p][k] * b[k][n] in the arithmetic `fmt`: operands split per the header, the retained products
    only, every partial sum rounded to fp32.  order 0: 32 k at a time, inside a block product by product in the kernel's order
    (smallest first), k ascending; order 1: k descending, the products of one k together, largest first."""
    pa, pb = _planes(a, fmt, ea), _planes(b, fmt, eb)
    kept = kept or {"f32": ((0, 0),), "s3": S3_KEPT, "h2": H2_KEPT}[fmt]
    Kn = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=f32)
    term = lambda i, j, k: (pb[i][k][None, :] * pa[j][:, k][:, None]).astype(f32)    # b carries the "weight" planes
    if order == 0:
        for k0 in range(0, Kn, 32):
            for (i, j) in kept:
                for k in range(k0, min(k0 + 32, Kn)):
                    acc = (acc + term(i, j, k)).astype(f32)
    else:
        for k in range(Kn - 1, -1, -1):
            for (i, j) in kept[::-1]:
                acc = (acc + term(i, j, k)).astype(f32)
    if fmt == "h2":
        acc = (acc * f32(2.0 ** -(ea + eb))).astype(f32)
    return acc


def _im2col(case, inp):
    """-> (patches (P, K) float32 in (c, ky, kx) order, weights (K, cout) float32)"""
    frame = R.assemble(inp["x0"], case.c0, inp["x1"], case.c1, case.pad1, "pool0" in case.flags)
    pb, pa = case.ks // 2, (case.ks - 1) // 2
    t = F.pad(torch.from_numpy(frame).permute(0, 3, 1, 2), (pb, pa, pb, pa))
    cols = F.unfold(t, case.ks, stride=case.stride)                       # (B, C*ks*ks, L)
    patches = cols.permute(0, 2, 1).reshape(-1, cols.shape[1]).numpy().astype(f32)
    return patches, inp["w"].reshape(case.cout, -1).T.astype(f32)


# ------------------------------------------------------------------------------------------------ the references
def test_forward_references_against_torch():
    r = np.random.default_rng(1)
    x = r.standard_normal((2, 6, 7, 5))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    w3, w1 = r.standard_normal((4, 5, 3, 3)), r.standard_normal((4, 5, 1, 1))
    for s in (1, 2):
        assert np.array_equal(R.conv_op(3, s)(x, w3), F.conv2d(xt, torch.from_numpy(w3), None, s, 1).permute(0, 2, 3, 1).numpy())
        assert np.array_equal(R.conv_op(1, s)(x, w1), F.conv2d(xt, torch.from_numpy(w1), None, s, 0).permute(0, 2, 3, 1).numpy())
        assert R.conv_op(3, s)(x, w3).shape[1:3] == (R.out_size(6, 3, s), R.out_size(7, 3, s))
    # ksize 4: padding 2 before, 1 after
    w4 = r.standard_normal((4, 5, 4, 4))
    want = F.conv2d(F.pad(xt, (2, 1, 2, 1)), torch.from_numpy(w4)).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.conv_op(4)(x, w4), want) and want.shape[1:3] == (6, 7)
    # the transposed conv: virtual channels + quadrant scatter = conv_transpose2d
    wt = r.standard_normal((5, 3, 2, 2))
    want = F.conv_transpose2d(xt, torch.from_numpy(wt), None, 2).permute(0, 2, 3, 1).numpy()
    assert np.allclose(R.upscatter(R.up_op(x, wt)), want, rtol=0, atol=1e-14)
    # the 7x7 stride-2 stem = the ksize-4 conv over the space-to-depth tensor with the weights of pack mode 2
    xs = r.standard_normal((2, 11, 13, 3))
    w7 = r.standard_normal((4, 3, 7, 7))
    s2d = np.zeros((2, 6, 7, 12))
    w4 = np.zeros((4, 12, 4, 4))
    for par in range(4):
        py, px = par >> 1, par & 1
        sub = xs[:, py::2, px::2]
        s2d[:, :sub.shape[1], :sub.shape[2], par * 3:(par + 1) * 3] = sub
        for ky in range(4):
            for kx in range(4):
                ky7, kx7 = 2 * ky + py - 1, 2 * kx + px - 1
                if 0 <= ky7 <= 6 and 0 <= kx7 <= 6:
                    w4[:, par * 3:(par + 1) * 3, ky, kx] = w7[:, :, ky7, kx7]
    assert np.allclose(R.stem_op(xs, w7), R.conv_op(4)(s2d, w4), rtol=0, atol=1e-13)
    # assemble: pool on load (odd sizes: floor), the second source at its offset
    x0, x1 = r.standard_normal((2, 13, 15, 6)), r.standard_normal((2, 5, 6, 3))
    a = R.assemble(x0, 4, x1, 2, (1, 0), pool0=True)
    assert a.shape == (2, 6, 7, 6) and a[0, 2, 3, 1] == x0[0, 4:6, 6:8, 1].max()
    assert a[1, 1, 0, 4] == x1[1, 0, 0, 0] and not a[:, 0, :, 4:].any() and not a[:, :, 6, 4:].any()
    y, b = r.standard_normal((1, 5, 7, 2)), np.abs(r.standard_normal((1, 5, 7, 2)))
    py_, pb_ = R.pooled(y, b)
    assert py_.shape == (1, 2, 3, 2) and py_[0, 1, 2, 0] == y[0, 2:4, 4:6, 0].max() and pb_[0, 0, 0, 1] == b[0, :2, :2, 1].max()


def test_backward_references_against_autograd():
    r = np.random.default_rng(2)
    x, dz = r.standard_normal((2, 5, 6, 4)), r.standard_normal((2, 5, 6, 3))
    for ks in (1, 3, 4):
        w = torch.from_numpy(r.standard_normal((3, 4, ks, ks))).requires_grad_(True)
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
        y = F.conv2d(F.pad(xt, (ks // 2, (ks - 1) // 2) * 2), w)
        y.backward(torch.from_numpy(dz).permute(0, 3, 1, 2))
        raw = R.wgrad_op(ks)(dz, x)                                    # (M, ks^2, N) -> OIHW
        assert np.allclose(raw.reshape(3, ks, ks, 4).transpose(0, 3, 1, 2), w.grad.numpy(), rtol=0, atol=1e-12)
        if ks != 4:
            dx = R.bwd_data_op(ks, 5, 6)(dz, w.detach().numpy())
            assert np.allclose(dx, xt.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
            want = F.conv_transpose2d(torch.from_numpy(dz).permute(0, 3, 1, 2), w.detach(), None, 1, ks // 2)
            assert np.allclose(dx, want.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    # a second source one row and one column short, at (1, 1): the gradient of the zero-padded concat's weight slice
    x1 = r.standard_normal((2, 4, 5, 2))
    w = torch.zeros((3, 2, 3, 3), dtype=torch.float64, requires_grad=True)
    full = F.pad(torch.from_numpy(x1).permute(0, 3, 1, 2), (1, 0, 1, 0))
    F.conv2d(full, w, None, 1, 1).backward(torch.from_numpy(dz).permute(0, 3, 1, 2))
    assert np.allclose(R.wgrad_op(3, (1, 1))(dz, x1).reshape(3, 3, 3, 2).transpose(0, 3, 1, 2), w.grad.numpy(), rtol=0, atol=1e-12)
    # backward-data of the transposed conv
    wt = torch.from_numpy(r.standard_normal((4, 3, 2, 2)))
    dy = r.standard_normal((2, 10, 12, 3))
    want = F.conv2d(torch.from_numpy(dy).permute(0, 3, 1, 2), wt, None, 2).permute(0, 2, 3, 1).numpy()
    assert np.allclose(R.up_bwd_data_op(dy, wt.numpy()), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", K.IMPULSE + K.IMPULSE_BWD, ids=lambda c: c.name)
def test_impulse_copies_are_what_the_references_compute(case):
    """shifted_copy / scattered_copy, which the GPU tests compare with, are the conv references on the impulse weights -
    integers below 2^24 throughout: the exact-equality demand is met by the reference itself"""
    s0, s1 = K.source_shapes(case)
    x0, x1 = K.pixel_coded(s0) + K.channel_coded(s0), (K.channel_coded(s1) + 7.0 if s1 else None)
    assert float(x0.max()) * 2 < 2 ** 24
    for n, (w, o, c, ky, kx) in enumerate(K.impulse_weights(case)):
        if n % 5:
            continue
        got = K.reference(case, dict(x0=x0, x1=x1, w=w, res=None))["y"]
        if case.mode == 3:
            want = R.scattered_copy(x0, o, case.cout, c, ky, kx, case.ks)
        else:
            frame = R.assemble(x0, case.c0, x1, case.c1, case.pad1)
            want = R.shifted_copy(frame, c, case.cout, o, ky, kx, case.ks, case.stride)
        assert np.array_equal(got, want) and want.any()


def test_integer_cases_are_exact_in_every_order():
    """every partial sum of the integer cases is bounded by A = sum |term| < 2^24: exact in fp32 in any order and any of the
    three arithmetics (small integers sit in the first plane: no product is dropped)"""
    for case in K.FWD:
        inp = K.fwd_inputs(case, "int")
        ref = K.reference(case, inp)
        assert float(ref["A"].max()) < 2 ** 24 and np.array_equal(ref["y"], np.round(ref["y"])), case.name
        scale, shift = K.epilogue_inputs(case, ref["acc"])
        y = K.reference(case, inp, scale, shift, relu=True)["y"]
        assert np.array_equal(y * 4, np.round(y * 4)) and float(np.abs(y).max()) * 4 < 2 ** 22, case.name     # two fp16 planes hold it
    for v in (3.0, -2.0, 2047.0):
        assert split_s3(f32(v))[0] + split_s3(f32(v))[1] == v and split_s3(f32(v))[2] == 0
        assert split_h2(f32(v), 2) == (4 * v, 0.0) and split_h2(f32(v), 0) == (v, 0.0)
    for case in K.WGRAD:
        dz, x0, x1, raw0 = K.wg_inputs(case, "int")
        _, A, _ = R.bilinear(R.wgrad_op(case.ks), dz, x0, 1, "f32")
        assert float(A.max()) + 5 < 2 ** 24 and (raw0 != 0).all()


def test_up_scatter_conv_reference_against_a_loop():
    """up2_op (the ksize-2 up-scatter conv) against the sum of include/sfh_amd.h written out as loops, the source one row
    and column short of the frame; and the scatter + clip of the destination"""
    r = np.random.default_rng(3)
    x, w, H, W = r.standard_normal((2, 3, 4, 2)), r.standard_normal((8, 2, 2, 2)), 4, 5
    got = R.up2_op(H, W)(x, w)
    X = np.zeros((2, H + 3, W + 3, 2))
    X[:, 1:4, 1:5] = x
    for q in range(4):
        dy, dx = q >> 1, q & 1
        for y in range(H):
            for xx in range(W):
                want = np.einsum("bklc,ockl->bo", X[:, y + dy:y + dy + 2, xx + dx:xx + dx + 2], w[q * 2:q * 2 + 2])
                assert np.allclose(got[:, y, xx, q * 2:q * 2 + 2], want, rtol=0, atol=1e-13)
    up = R.upscatter(got)
    assert up.shape == (2, 8, 10, 2) and up[1, 5, 2, 1] == got[1, 2, 1, 2 * 2 + 1] and up[0, 0, 3, 0] == got[0, 0, 1, 1 * 2]
    # composed from the identity: a 2x2 weight that is ConvTranspose2d's own tap reproduces conv_transpose2d
    wt = r.standard_normal((2, 3, 2, 2))                                   # IOHW
    w2 = np.zeros((12, 2, 2, 2))
    for q in range(4):
        dy, dx = q >> 1, q & 1
        w2[q * 3:(q + 1) * 3, :, 1 - dy, 1 - dx] = wt[:, :, dy, dx].T      # the window of quadrant (dy, dx) starts at (y+dy-1, x+dx-1)
    want = F.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), None, 2).permute(0, 2, 3, 1).numpy()
    assert np.allclose(R.upscatter(R.up2_op(3, 4)(x, w2)), want, rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ the plane walk
@pytest.mark.parametrize("fmt", ["s3", "h2"])
def test_plane_walk_constants(fmt):
    """(a) the split puts one bit in each plane, (b) the retained products sum to an fp32 number in every order, (c) the fp64
    product rounds to exactly it; and losing any one retained product moves the result by at least 32 ulps"""
    kept = S3_KEPT if fmt == "s3" else H2_KEPT
    w = K.walk_weight(fmt)
    wexp = K.wexp_for(np.array([w]))
    for e in ((0, 2) if fmt == "h2" else (2,)):
        xs = np.unique(K.walk_values((4, 5, 6, 7), fmt, 11, e))
        assert len(xs) == 10
        scalars = lambda v, ex: tuple(np.float64(np.ravel(p)[0]) for p in _planes(f32(v), fmt, ex))
        pw = scalars(w, wexp)
        assert fmt == "s3" or 2.0 ** 13 <= abs(pw[0]) < 2.0 ** 14
        for x in xs:
            px = scalars(x, e)
            for p in px + pw:                                                                   # (a)
                m, _ = np.frexp(np.float64(p))
                assert abs(m) == 0.5, (x, p)
            assert np.float64(sum(px)) == np.float64(x) * 2.0 ** (e if fmt == "h2" else 0)
            terms = [np.float64(pw[i]) * np.float64(px[j]) for i, j in kept]
            total = sum(terms)
            unscale = 2.0 ** -(wexp + e) if fmt == "h2" else 1.0
            for order in (terms, terms[::-1]):                                                  # (b)
                acc = f32(0)
                for t in order:
                    assert np.float64(f32(t)) == t
                    acc = f32(acc + f32(t))
                assert np.float64(acc) == total
            full = np.float64(x) * np.float64(w)
            assert np.float64(f32(full)) == total * unscale and full != total * unscale         # (c)
            ulp = np.spacing(f32(abs(total)))
            assert min(abs(t) for t in terms) >= 32 * ulp
            # backward-filter (H2: always at SFH_H2_ACT_EXP): the dz element is twice the weight, onto a starting value of 8 -
            # |2 x w| <= 4.01, no cancellation, still exact
            if e == K.H2_ACT_EXP:
                assert np.float64(f32(8.0 + 2 * full)) == 8.0 + 2 * total * unscale


# ------------------------------------------------------------------------------------------------ the bounds
# The restatement walks one product at a time in numpy, so it runs on a SUBSET: every arithmetic, both strides, 3x3 and 1x1, a
# stage-width remainder, two sources, pool0 - all pack mode 0, accumulator only (the epilogue's bound is two more roundings
# on top and is exercised on the GPU); pack modes 1 - 4 differ from mode 0 only in how the weights are laid out, which the
# integer and impulse cases check.  The README's host ratios are the largest over this subset.
RESTATED = ["f32_c24", "f32_k1_c48", "f32_two_pad11", "f32_pool0", "s3_c96", "s3_two_pad11", "s3_k1_c96", "h2_c96",
            "h2_two_pad11", "h2_k1_c96", "small_c96", "f32_s2_23x41_tile0", "h2_s2_23x41_tile4"]


@pytest.mark.parametrize("name", RESTATED)
def test_forward_bound_holds_for_the_restated_arithmetic(name):
    case = BY_NAME[name]
    ar = K.arith(case)
    inp = K.fwd_inputs(case, "randn")
    ref = K.reference(case, inp)
    patches, wmat = _im2col(case, inp)
    wexp = K.wexp_for(inp["w"])
    want = ref["acc"].reshape(-1, case.cout)
    worst = 0.0
    for order in (0, 1):
        got = restate_matmul(patches, wmat, ar, order, 2, wexp)
        worst = max(worst, R.ratio(got, want, ref["bound"].reshape(-1, case.cout)))
    print(f"RATIO {name}: restated {ar} forward {worst:.3f}")
    assert worst <= 1.0
    # integers: the restatement gives the fp64 value bit for bit
    inp = K.fwd_inputs(case, "int")
    patches, wmat = _im2col(case, inp)
    got = restate_matmul(patches, wmat, ar, 0, 2, K.wexp_for(inp["w"]))
    assert np.array_equal(got.astype(np.float64), K.reference(case, inp)["acc"].reshape(-1, case.cout))


def test_dropping_a_retained_product_breaks_the_walk_not_the_integers():
    """what the GPU mutation check relies on, shown on the restatement: without w2x0 the plane-walk output is 32 ulps off,
    the integer outputs are unchanged"""
    case = BY_NAME["s3_c96"]
    inp = K.fwd_inputs(case, "int")
    patches, wmat = _im2col(case, inp)
    x = K.walk_values((1, 3, 4, 32), "s3", 11).reshape(-1, 32)
    w = np.zeros((32, 2), f32)
    w[5, 1] = K.walk_weight("s3")
    whole = restate_matmul(x, w, "s3", 0)
    fewer = tuple(p for p in S3_KEPT if p != (2, 0))
    assert np.array_equal(restate_matmul(patches, wmat, "s3", 0, kept=fewer), K.reference(case, inp)["acc"].reshape(-1, 64).astype(f32))
    less = restate_matmul(x, w, "s3", 0, kept=fewer)
    assert np.array_equal(whole.astype(np.float64), (x.astype(np.float64) @ w.astype(np.float64)).astype(f32))
    assert (np.abs(whole[:, 1] - less[:, 1]) >= 32 * np.spacing(np.abs(whole[:, 1]))).all()


@pytest.mark.parametrize("name", ["f32_k3_M64", "f32_k4_M64", "s3_k3_M64", "h2_k3_M64", "s3_k1_two_pad11", "h2_k3_two_pad11"])
def test_wgrad_bound_holds_for_the_restated_arithmetic(name):
    case = WG_BY_NAME[name]
    dz, x0, x1, raw0 = K.wg_inputs(case, "randn")
    x, pad, n_off = (x1, case.pad, case.N) if x1 is not None else (x0, (0, 0), 0)
    N = x.shape[3]
    r0 = raw0[..., n_off:n_off + N]
    want, bound = R.wgrad(dz, x, r0, case.ks, case.kern, pad)
    B, H, W, M = dz.shape
    p = case.ks // 2
    xin = np.zeros((B, H + case.ks - 1, W + case.ks - 1, N), f32)
    xin[:, p + pad[0]:p + pad[0] + x.shape[1], p + pad[1]:p + pad[1] + x.shape[2]] = x
    worst = 0.0
    for tap in (0, case.ks * case.ks - 1):
        ky, kx = divmod(tap, case.ks)
        win = xin[:, ky:ky + H, kx:kx + W].reshape(-1, N)
        for order in (0, 1):
            part = restate_matmul(dz.reshape(-1, M).T.copy(), win, case.kern, order)       # (M, N): k = the pixels
            got = (r0[:, tap] + part).astype(f32)
            worst = max(worst, R.ratio(got, want[:, tap], bound[:, tap]))
    print(f"RATIO {name}: restated {case.kern} backward-filter {worst:.3f}")
    assert worst <= 1.0


def test_h2_representation_error_is_the_header_s():
    """the split restated per the header stays inside h2_rep's d(v) and below its l(v), over 40 binades and at three exponents"""
    r = np.random.default_rng(5)
    v = (r.standard_normal(20000) * np.exp(r.uniform(-14, 7, 20000))).astype(f32)
    for e in (-3, 0, 2):
        p0, p1 = split_h2(v, e)
        d, l = R.h2_rep(v, e)
        err = np.abs((p0.astype(np.float64) + p1) * 2.0 ** -e - v)
        assert (err <= d).all() and (np.abs(p1) * 2.0 ** -e <= l).all() and float(np.abs(v).max()) * 2.0 ** e < 65504
    p = split_s3(v)
    assert np.array_equal(p[0].astype(np.float64) + p[1] + p[2], v.astype(np.float64))
    assert (np.abs(p[1]) <= 2.0 ** -8 * (1 + 2.0 ** -8) * np.abs(v)).all() and (np.abs(p[2]) <= 2.0 ** -16 * np.abs(v)).all()


def test_case_lists_cover_the_kernels_constants():
    names = set(BY_NAME)
    for kern, tiles in (("f32", (0, 1, 2)), ("s3", range(5)), ("h2", range(5))):
        for t in tiles:
            th, tw = K.tile_hw(kern, t, 1)
            assert {f"{kern}_tile{t}_s1_{th - 1}x{tw - 1}", f"{kern}_tile{t}_s1_{th + 1}x{tw + 1}"} <= names
    assert {"small_11x19", "small_13x21", "h2_wg128", "f32_pool0"} <= names
    for case in K.FWD:
        assert case.cout % 64 == 0 and K.cs0(case) >= case.c0 and (case.kern == "f32" or case.c0 % 32 == 0)
        ho, wo = K.out_hw(case)
        th, tw = K.tile_hw(case.kern, case.tile, case.stride)
        assert case.B * -(-(ho + 2) // th) * -(-wo // tw) * (case.cout // 32) <= 400, case.name     # a few hundred workgroups
