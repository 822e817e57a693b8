"""The forward entries of csrc/pointwise.hip one by one against the fp64 CPU references of tests/pointwise_ref.py (which
tests/test_pointwise_host.py holds against torch), through the raw C entry points:

  sfh_nchw_to_nhwc, sfh_nhwc_to_nchw, sfh_space_to_depth2, sfh_maxpool3x3s2_fwd, sfh_resize_nchw (both modes), sfh_upsample2x_bilinear_nhwc,
  sfh_fold_bn, sfh_outconv_fwd, sfh_consistency_ce_fwd, sfh_avgpool_linear_fwd, sfh_compose_up_weights

Conventions of tests/test_gpu_step_tail.py, whose helpers are imported: every output ends in a guard of 64 sentinel elements
that must come back untouched; an output the kernel overwrites starts as NaN (255 for the uint8 argmax); every comparison is
bit equality or a per-element bound built from the reference's own absolute quantities (pointwise_ref.py derives each); an
element whose bound is zero must be exact.  Each test prints its largest error / bound (``pytest -s``) and asserts it <= 1.

The argmax on non-finite logits is pinned as the kernel computes it, not as the reference project does: see
test_outconv_argmax_nonfinite.

Out of scope here:
  sfh_u8hwc_* and sfh_mask_format_fwd       bit-exact tests against OpenCV and the oracle at several sizes exist
  the two backward entries of pointwise.hip   pinned in tests/test_gpu_step_tail.py
  csrc/warp.hip                               its nearest warp is bit-exact against the oracle already
  csrc/hostprep.hip                           host code, held by the preparation tests
"""
import numpy as np
import pytest
import torch

import pointwise_cases as cases
import pointwise_ref as R
from oracle import torch_ref
from test_gpu_step_tail import F32, GUARD, NAN, Guarded, K, _dev, _report, _same_bits  # noqa: F401  (K is the fixture)

pytestmark = pytest.mark.gpu


def _nan(shape, dtype=torch.float32):
    return Guarded(shape, dtype, NAN)


class GuardedBytes(Guarded):
    """the uint8 argmax: starts as 255 (no class), the guard holds 0xA5"""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.guard = self.buf[self.n:].clone()
        self.t = self.buf[:self.n].view(*shape)
        self.t.fill_(255)


def _ok(K, rc):
    assert rc == 0, K[0].sfh_last_error()


# ------------------------------------------------------------------------------------------------ layout conversion
@pytest.mark.parametrize("C", cases.LAYOUT_CHANNELS)
def test_layout_conversion(K, C):
    """NCHW -> NHWC (lanes C .. cs-1 are +0.0 bits) and back (garbage in those lanes is not read into the result), cs = C
    rounded up to 4 and 4 more; 1, 255, 256, 257 pixels and three frames of 91; the round trip is the identity, bit for bit"""
    lib, _ptr, _stream = K
    for cs in cases.layout_strides(C):
        for B, H, W in cases.LAYOUT_SHAPES:
            x = cases.randn(f"layout-{C}-{cs}-{B}x{H}x{W}", (B, C, H, W))
            x.reshape(-1)[0] = -0.0
            xd = _dev(x)
            y = _nan((B, H, W, cs))
            _ok(K, lib.sfh_nchw_to_nhwc(_ptr(xd), _ptr(y.t), B, C, H, W, cs, _stream()))
            got = y.result()
            assert _same_bits(got, R.nchw_to_nhwc_ref(x, cs)), (C, cs, B, H, W)
            back = _nan((B, C, H, W))
            _ok(K, lib.sfh_nhwc_to_nchw(_ptr(y.t), _ptr(back.t), B, C, H, W, cs, _stream()))
            assert _same_bits(back.result(), x)
            dirty = got.copy()
            dirty[..., C:] = 12345.0
            z = _nan((B, C, H, W))
            dd = _dev(dirty)
            _ok(K, lib.sfh_nhwc_to_nchw(_ptr(dd), _ptr(z.t), B, C, H, W, cs, _stream()))
            assert _same_bits(z.result(), R.nhwc_to_nchw_ref(dirty, C)) and _same_bits(z.result(), x)


def test_layout_conversion_refusals(K):
    """cs < C and a cs off the quad are refused, in both directions, and nothing is written"""
    lib, _ptr, _stream = K
    src = torch.ones(1, 5, 3, 3, device="cuda")
    wide = torch.ones(1, 3, 3, 8, device="cuda")
    out = _nan((1, 3, 3, 8))
    for cs in (4, 6):
        assert lib.sfh_nchw_to_nhwc(_ptr(src), _ptr(out.t), 1, 5, 3, 3, cs, _stream()) != 0
        assert lib.sfh_nhwc_to_nchw(_ptr(wide), _ptr(out.t), 1, 5, 3, 3, cs, _stream()) != 0
    assert np.isnan(out.result()).all()


@pytest.mark.parametrize("size", cases.S2D_SIZES, ids=str)
def test_space_to_depth2(K, size):
    """out[Y][X][(py 2 + px) cs + c] = in[2Y + py][2X + px][c], the odd row and column read as +0.0; cs 4, 8, 12; one and two frames"""
    lib, _ptr, _stream = K
    H, W = size
    for cs in cases.S2D_STRIDES:
        for B in cases.S2D_BATCHES:
            x = cases.randn(f"s2d-{size}-{cs}-{B}", (B, H, W, cs))
            y = _nan((B, (H + 1) // 2, (W + 1) // 2, 4 * cs))
            xd = _dev(x)
            _ok(K, lib.sfh_space_to_depth2(_ptr(xd), _ptr(y.t), B, H, W, cs, _stream()))
            assert _same_bits(y.result(), R.space_to_depth2_ref(x)), (size, cs, B)


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("size", cases.MAXPOOL_SIZES, ids=str)
def test_maxpool3x3s2(K, size):
    """MaxPool2d(3, 2, 1) selects: bit for bit against torch in fp64, C 4, 12, 64; planes of -inf; NaNs as the first, middle and
    last tap of a window (torch propagates them); a 1-wide map"""
    lib, _ptr, _stream = K
    H, W = size
    for C in cases.MAXPOOL_CHANNELS:
        for kind in cases.MAXPOOL_KINDS:
            x = cases.maxpool_input(H, W, C, kind)
            y = _nan((2, R.pool_out(H), R.pool_out(W), C))
            xd = _dev(x)
            _ok(K, lib.sfh_maxpool3x3s2_fwd(_ptr(xd), _ptr(y.t), 2, H, W, C, _stream()))
            assert _same_bits(y.result(), R.maxpool_ref(x)), (size, C, kind)


# ------------------------------------------------------------------------------------------------ sfh_resize_nchw
NEAREST_GEOMS = cases.resize_geometries()
BILINEAR_GEOMS = cases.resize_geometries(extra=True)


def _resize(K, x, geom, mode, align):
    lib, _ptr, _stream = K
    hs, ws, hd, wd = geom
    y = _nan((x.shape[0], hd, wd))
    xd = _dev(x)
    _ok(K, lib.sfh_resize_nchw(_ptr(xd), _ptr(y.t), x.shape[0], hs, ws, hd, wd, mode, align, _stream()))
    return y.result()


@pytest.mark.parametrize("geom", NEAREST_GEOMS, ids=str)
def test_resize_nearest(K, geom):
    """a gather through the fp32 index tables, bit for bit, one plane and six; up, down, odd ratios, 1 -> n, n -> 1 and the two
    pairs whose fp32 index differs from the exact quotient's; align_corners does not matter"""
    for P in cases.RESIZE_PLANES:
        x = cases.resize_input(geom, P)
        want = R.resize_nearest_ref(x, geom[2], geom[3])
        for align in (0, 1):
            assert _same_bits(_resize(K, x, geom, 0, align), want), (geom, P, align)


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("geom", BILINEAR_GEOMS, ids=str)
def test_resize_bilinear(K, geom, align):
    """F.interpolate(mode='bilinear') per element: the weights from the exact source coordinate, the bound from the error of the
    kernel's fp32 coordinate and six roundings; out = 1 with align_corners (scale 0), in = 1, 23 x 41 -> 24 x 42"""
    x = cases.resize_input(geom, 2)
    ref, bound = R.bilinear_ref(x, geom[2], geom[3], align)
    _report(f"resize_bilinear {geom} align{align}", y=R.ratio(_resize(K, x, geom, 1, align), ref, bound))


def test_resize_refuses_unknown_mode(K):
    lib, _ptr, _stream = K
    y = _nan((1, 4, 4))
    x = torch.ones(1, 2, 2, device="cuda")
    assert lib.sfh_resize_nchw(_ptr(x), _ptr(y.t), 1, 2, 2, 4, 4, 2, 0, _stream()) != 0
    assert np.isnan(y.result()).all()


# ------------------------------------------------------------------------------------------------ sfh_upsample2x_bilinear_nhwc
def _up2(K, x):
    lib, _ptr, _stream = K
    B, H, W, C = x.shape
    y = _nan((B, 2 * H, 2 * W, C))
    xd = _dev(x)
    _ok(K, lib.sfh_upsample2x_bilinear_nhwc(_ptr(xd), _ptr(y.t), B, H, W, C, _stream()))
    return y.result()


@pytest.mark.parametrize("C", cases.UP2_CHANNELS)
@pytest.mark.parametrize("size", cases.UP2_SIZES, ids=str)
def test_upsample2x_bilinear(K, size, C):
    """(B,H,W,C) -> (B,2H,2W,C) = Wy x Wx of step_tail_ref.up2_weights per channel; one pixel (a copy: the bound allows
    6 u, the weights are exact), a single row, a single column, C = 12"""
    for B in cases.UP2_BATCHES:
        x = cases.randn(f"up2-{size}-{C}-{B}", (B,) + size + (C,))
        ref, bound = R.up2_ref(x)
        got = _up2(K, x)
        if size == (1, 1):
            assert _same_bits(got, np.broadcast_to(x, got.shape))
        _report(f"upsample2x {size} C{C} B{B}", y=R.ratio(got, ref, bound))


def test_upsample2x_bilinear_refuses_channels_off_the_quad(K):
    lib, _ptr, _stream = K
    y = _nan((1, 4, 4, 6))
    x = torch.ones(1, 2, 2, 6, device="cuda")
    assert lib.sfh_upsample2x_bilinear_nhwc(_ptr(x), _ptr(y.t), 1, 2, 2, 6, _stream()) != 0
    assert np.isnan(y.result()).all()


def test_upsample2x_adjoint(K):
    """<up(x), g> = <x, up_bwd(g)> for the two kernels, both dot products in fp64 on the host, within the two references'
    bounds carried through the dot products: the forward tied to the backward that test_gpu_step_tail.py pins"""
    lib, _ptr, _stream = K
    B, H, W, C = 2, 5, 7, 12
    x = cases.randn("up2-adjoint-x", (B, H, W, C))
    g = cases.randn("up2-adjoint-g", (B, 2 * H, 2 * W, C))
    y = _up2(K, x)
    dx = _nan((B, H, W, C))
    gd = _dev(g)
    _ok(K, lib.sfh_upsample2x_bilinear_nhwc_bwd(_ptr(gd), _ptr(dx.t), B, H, W, C, _stream()))
    yref, by = R.up2_ref(x)
    dref, bd = R.S.up2_bwd_ref(g)
    lhs = float((y.astype(np.float64) * g).sum())
    rhs = float((dx.result().astype(np.float64) * x).sum())
    exact = float((yref * g).sum())
    room = R.dot_bound(yref, by, g) + R.dot_bound(dref, bd, x) + 2 * y.size * R.S.E53 * float(np.abs(yref * g).sum())
    _report("upsample2x adjoint", fwd=abs(lhs - exact) / R.dot_bound(yref, by, g), both=abs(lhs - rhs) / room)


# ------------------------------------------------------------------------------------------------ sfh_fold_bn
@pytest.mark.parametrize("repeat", cases.FOLD_REPEAT)
@pytest.mark.parametrize("n", cases.FOLD_N)
def test_fold_bn(K, n, repeat):
    """scale = gamma / sqrt(var + eps) and shift = (conv_bias - mean) scale + beta, tiled i % n over n * repeat elements; with
    and without conv_bias; without gamma: scale exactly 1, shift exactly the bias (or +0.0); var 0, 1e-12, 1, 1e6 on every
    channel in turn; mean == conv_bias (shift = beta exactly) and one ulp beside it"""
    lib, _ptr, _stream = K
    worst = dict(scale=0.0, shift=0.0)
    for off in range(4):
        x = cases.fold_inputs(n, off)
        d = {k: _dev(v) for k, v in x.items()}
        for with_cb in (True, False):
            for with_gamma in (True, False):
                sc, sh = _nan((n * repeat,)), _nan((n * repeat,))
                p = lambda k, on=True: _ptr(d[k]) if on else None
                _ok(K, lib.sfh_fold_bn(p("cb", with_cb), p("gamma", with_gamma), p("beta", with_gamma), p("mean", with_gamma),
                                       p("var", with_gamma), cases.FOLD_EPS, n, repeat, _ptr(sc.t), _ptr(sh.t), _stream()))
                a, s, ba, bs = R.fold_bn_ref(x["cb"] if with_cb else None, x["gamma"] if with_gamma else None, x["beta"], x["mean"],
                                             x["var"], cases.FOLD_EPS, n, repeat)
                gsc, gsh = sc.result(), sh.result()
                if not with_gamma:
                    assert _same_bits(gsc, np.ones(n * repeat, dtype=F32)) and _same_bits(gsh, s.astype(F32))
                elif with_cb:
                    assert gsh[0] == x["beta"][0]
                worst["scale"] = max(worst["scale"], R.ratio(gsc, a, ba))
                worst["shift"] = max(worst["shift"], R.ratio(gsh, s, bs))
    _report(f"fold_bn n{n} x{repeat}", **worst)


def test_fold_bn_refuses_gamma_without_statistics(K):
    lib, _ptr, _stream = K
    sc, sh = _nan((4,)), _nan((4,))
    g = torch.ones(4, device="cuda")
    assert lib.sfh_fold_bn(None, _ptr(g), _ptr(g), None, _ptr(g), 1e-5, 4, 1, _ptr(sc.t), _ptr(sh.t), _stream()) != 0
    assert np.isnan(sc.result()).all() and np.isnan(sh.result()).all()


# ------------------------------------------------------------------------------------------------ sfh_outconv_fwd
def _run_outconv(K, c, x):
    """-> dict(logits, amax, stn) of what the case asks for (None otherwise)"""
    lib, _ptr, _stream = K
    B, H, W = c["shape"]
    nc, cin = c["nc"], c["cin"]
    lg = _nan((B, nc, H, W)) if c["out"] in ("both", "logits") else None
    am = GuardedBytes((B, H, W)) if c["out"] in ("both", "argmax") else None
    st = fr = None
    scs = fcs = 0
    if c["stn"]:
        scs, fcs = c["stn"]
        st, fr = _nan((B, H, W, scs)), _dev(x["frame"])
    xd, wd, bd = _dev(x["x"]), _dev(x["w"]), _dev(x["bias"])
    _ok(K, lib.sfh_outconv_fwd(_ptr(xd), cin, _ptr(wd), _ptr(bd), nc, B, H, W,
                               _ptr(lg.t) if lg else None, _ptr(am.t) if am else None, _ptr(st.t) if st else None, scs,
                               _ptr(fr) if st else None, fcs, _stream()))
    return dict(logits=lg.result() if lg else None, amax=am.result() if am else None, stn=st.result() if st else None)


OUTCONV_CASES = cases.outconv_cases()


@pytest.mark.parametrize("c", OUTCONV_CASES, ids=[c["id"] for c in OUTCONV_CASES])
def test_outconv(K, c):
    """logits per element inside (cin / 8 + 6) u (sum |x w| + |bias|); the argmax = np.argmax of the kernel's own logits and
    = preds_to_masks of them (no pixel of these cases lies inside the tie margin: the host test asserts it); stn_in = the
    logits' bits, the frame's three channels' bits, +0.0 up to stn_cs.  nc 1 .. 8, cin 8 .. 1024, 1 / 127 / 128 / 129 / 133
    pixels, three frames of 91; logits only, argmax only, both, seven stn_in geometries."""
    x = cases.outconv_inputs(c)
    ref, bound = R.outconv_ref(x["x"], x["w"], x["bias"])
    got = _run_outconv(K, c, x)
    lg = got["logits"]
    if lg is not None:
        _report(f"outconv {c['id']}", logits=R.ratio(lg, ref, bound))
    if got["stn"] is not None:
        stn_logits = np.ascontiguousarray(got["stn"][..., :c["nc"]].transpose(0, 3, 1, 2))
        assert _same_bits(stn_logits, lg)
        assert _same_bits(got["stn"], R.stn_in_ref(lg, x["frame"], c["stn"][0]))
    if got["amax"] is not None:
        if lg is None:                       # argmax only: every margin exceeds twice the bound, so the reference decides
            assert np.array_equal(got["amax"], np.argmax(ref, axis=1))
        else:
            assert np.array_equal(got["amax"], np.argmax(lg, axis=1)) and np.array_equal(got["amax"], R.argmax_scan(lg))
            if c["nc"] > 1:
                assert (R.top2_margin(lg) >= torch_ref.SOFTMAX_TIE_MARGIN).all()
            assert np.array_equal(got["amax"], torch_ref.preds_to_masks(torch.from_numpy(lg)).numpy())


def test_outconv_exact_ties(K):
    """integer-valued x, w and bias: the logits are bit-equal to the reference; classes 1 and 2 tie everywhere (the answer is
    never 2) and all four tie on the zero pixels (the answer is 0): the first index wins"""
    x = cases.outconv_tie_inputs()
    c = dict(shape=x["x"].shape[:3], nc=4, cin=8, out="both", stn=None)
    ref, _ = R.outconv_ref(x["x"], x["w"], x["bias"])
    got = _run_outconv(K, c, x)
    assert _same_bits(got["logits"], ref.astype(F32)) and np.array_equal(ref.astype(F32).astype(np.float64), ref)
    assert np.array_equal(got["amax"], np.argmax(ref, axis=1)) and not (got["amax"] == 2).any()
    assert (got["amax"][0, 0, :5] == 0).all() and (got["amax"] == 1).any()


@pytest.mark.parametrize("row,want", cases.OUTCONV_NONFINITE, ids=[str(i) for i in range(len(cases.OUTCONV_NONFINITE))])
def test_outconv_argmax_nonfinite(K, row, want):
    """PINNED DIVERGENCE.  The kernel's strict `>` scan from class 0 skips a NaN (unless it sits at class 0) and lets +inf win;
    the reference project's argmax(softmax(.)) answers 0 for every row that holds a NaN or a +inf.  [1, nan, 3, .5] and
    [1, 2, inf, 0] give 2 here and 0 there.  The fused head epilogue and the mask formatter share the kernel's rule; a frame
    with such logits answers with a NaN theta anyway.  The rows arrive through the bias (x = 0)."""
    c = dict(shape=(1, 1, 3), nc=4, cin=8, out="both", stn=None)
    x = dict(x=np.zeros((1, 1, 3, 8), dtype=F32), w=np.ones((4, 8), dtype=F32), bias=np.array(row, dtype=F32), frame=None)
    got = _run_outconv(K, c, x)
    assert _same_bits(got["logits"], np.broadcast_to(x["bias"][None, :, None, None], (1, 4, 1, 3)))
    assert (got["amax"] == want).all() and (R.argmax_scan(got["logits"]) == want).all()
    theirs = torch_ref.preds_to_masks(torch.from_numpy(got["logits"])).numpy()
    if np.isnan(row).any() or np.inf in row:
        assert (theirs == 0).all()
    else:
        assert (theirs == want).all()


def test_outconv_refusals(K):
    """cin off the 8-channel step, nc 0 and 9, an stn_in too narrow for logits + frame or wider than 16: refused, nothing written"""
    lib, _ptr, _stream = K
    x = torch.ones(1, 2, 2, 64, device="cuda")
    w = torch.ones(9, 64, device="cuda")
    lg, st = _nan((1, 9, 2, 2)), _nan((1, 2, 2, 20))

    def call(cin=64, nc=4, scs=0):
        return lib.sfh_outconv_fwd(_ptr(x), cin, _ptr(w), _ptr(w), nc, 1, 2, 2, _ptr(lg.t), None, _ptr(st.t) if scs else None, scs,
                                   _ptr(x) if scs else None, 4, _stream())
    assert call(cin=12) != 0 and call(nc=0) != 0 and call(nc=9) != 0
    assert call(nc=6, scs=8) != 0 and call(scs=20) != 0 and call(scs=10) != 0
    assert np.isnan(lg.result()).all() and np.isnan(st.result()).all()


# ------------------------------------------------------------------------------------------------ sfh_consistency_ce_fwd
CE_CASES = cases.ce_cases()


@pytest.mark.parametrize("c", CE_CASES, ids=[c["id"] for c in CE_CASES])
def test_consistency_ce(K, c):
    """the frame mean of logsumexp - l[target] inside the per-pixel roundings plus the fp32 sum's longest path; nc 2 .. 8; 1,
    255, 2047, 2048, 2049, 10241 pixels and 257 x 512 (65 partials per frame: the final kernel's second trip); logits with a
    spread of 200, all equal, one at 1e4; the mask at another size through the fp32 nearest tables.  The workspace is exactly
    sfh_ce_workspace_floats long (guarded); a second launch gives the same bits."""
    lib, _ptr, _stream = K
    logits, mask = cases.ce_inputs(c)
    B, H, W = c["shape"]
    hm, wm = c["mask"]
    nws = lib.sfh_ce_workspace_floats(B, H, W)
    assert nws == R.ce_workspace_floats(B, H, W)
    ld, md = _dev(logits), _dev(mask)
    runs = []
    for _ in range(2):
        ws, score = _nan((nws,)), _nan((B,))
        _ok(K, lib.sfh_consistency_ce_fwd(_ptr(ld), _ptr(md), B, c["nc"], H, W, hm, wm, _ptr(ws.t), _ptr(score.t), _stream()))
        runs.append((score.result(), ws.result()))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
    assert np.isfinite(runs[0][1]).all()
    ref, bound = R.ce_ref(logits, mask)
    _report(f"consistency_ce {c['id']}", score=R.ratio(runs[0][0], ref, bound))


# ------------------------------------------------------------------------------------------------ sfh_avgpool_linear_fwd
AVG_CASES = cases.avgpool_cases()


@pytest.mark.parametrize("c", AVG_CASES, ids=[c["id"] for c in AVG_CASES])
def test_avgpool_linear(K, c):
    """feat = the channel means and out = w feat + b on x = 1000 + noise: H W at every edge of the 16-pixel loop and its tail,
    C 4 .. 2048 (65 and 100: a partial block of 64 channels), nout 1 .. 9, one and three frames"""
    lib, _ptr, _stream = K
    x = cases.avgpool_inputs(c)
    B, H, W, C = c["shape"]
    feat, out = _nan((B, C)), _nan((B, c["nout"]))
    xd, wd, bd = _dev(x["x"]), _dev(x["w"]), _dev(x["b"])
    _ok(K, lib.sfh_avgpool_linear_fwd(_ptr(xd), _ptr(wd), _ptr(bd), B, H, W, C, c["nout"],
                                      _ptr(feat.t), _ptr(out.t), _stream()))
    rf, bf, ro, bo = R.avgpool_linear_ref(x["x"], x["w"], x["b"])
    _report(f"avgpool_linear {c['id']} {c['shape']}", feat=R.ratio(feat.result(), rf, bf), out=R.ratio(out.result(), ro, bo))


# ------------------------------------------------------------------------------------------------ sfh_compose_up_weights
def _compose(K, x, c1, c0, cout, cx):
    lib, _ptr, _stream = K
    w2, sb = _nan((4 * cout, cx, 2, 2)), _nan((16, 4 * cout))
    d = {k: _dev(v) for k, v in x.items()}
    rc = lib.sfh_compose_up_weights(_ptr(d["wconv"]), cout, c0, c1, _ptr(d["wt"]), cx, _ptr(d["bt"]), _ptr(d["scale4"]),
                                    _ptr(d["shift4"]), _ptr(w2.t), _ptr(sb.t), _stream())
    return rc, w2, sb


@pytest.mark.parametrize("geom", cases.COMPOSE_CASES, ids=str)
def test_compose_up_weights(K, geom):
    """w2 and shift_border against the explicit einsum over taps, window slots and intermediate channels (which the host test
    holds against conv_transpose2d + conv2d for every parity and border class); c1 16 .. 80 (the 32-channel slab's tail and
    a third slab), c0 0 / 16 / 80, cout and cx 16 / 48"""
    x = cases.compose_inputs(*geom)
    rc, w2, sb = _compose(K, x, *geom)
    _ok(K, rc)
    rw, bw, rs, bs = R.compose_up_ref(x["wconv"], geom[1], x["wt"], x["bt"], x["scale4"], x["shift4"])
    _report(f"compose_up_weights {geom}", w2=R.ratio(w2.result(), rw, bw), shift_border=R.ratio(sb.result(), rs, bs))


def test_compose_up_weights_refusals(K):
    """cout and cx move in tiles of 16: cout = 24 and cx = 8 are refused and nothing is written"""
    for geom in ((16, 0, 24, 16), (16, 0, 16, 8)):
        rc, w2, sb = _compose(K, cases.compose_inputs(*geom), *geom)
        assert rc != 0 and np.isnan(w2.result()).all() and np.isnan(sb.result()).all()
