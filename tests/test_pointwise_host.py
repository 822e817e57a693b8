"""CPU tests of tests/pointwise_ref.py and tests/pointwise_cases.py: every reference against torch (fp64 where torch has the
operator) or a brute-force restatement, every bound against a numpy float32 restatement of the kernel's own order of
operations, and the case tables against the list of edges the kernels have.  No absolute or norm tolerance: a comparison
of two fp64 computations uses the reference's own bound with fp64's unit in place of fp32's (U64)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_cases as cases
import pointwise_ref as R
from oracle import torch_ref

F32 = np.float32
U64 = (2.0 ** -53) / R.U           # a bound counted in fp32 roundings, restated for an fp64 computation of the same shape
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()


def _report(name, **ratios):
    print(f"RATIO {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (name, ratios)


# ------------------------------------------------------------------------------------------------ movers
@pytest.mark.parametrize("C", cases.LAYOUT_CHANNELS)
def test_layout_refs_vs_torch(C):
    for cs in cases.layout_strides(C):
        assert cs % 4 == 0 and cs >= C
        x = cases.randn(f"host-layout-{C}", (3, C, 7, 13))
        want = F.pad(torch.from_numpy(x).permute(0, 2, 3, 1), (0, cs - C)).contiguous().numpy()
        got = R.nchw_to_nhwc_ref(x, cs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(R.nhwc_to_nchw_ref(got, C), x)


def test_layout_table():
    assert sorted(b * h * w for b, h, w in cases.LAYOUT_SHAPES) == [1, 255, 256, 257, 273]
    assert any(b == 3 and 256 % (h * w) != 0 for b, h, w in cases.LAYOUT_SHAPES)      # a frame boundary inside a block
    assert all(cases.layout_strides(C) == (cases.r4(C), cases.r4(C) + 4) for C in cases.LAYOUT_CHANNELS)


def test_space_to_depth_ref_brute():
    for H, W in cases.S2D_SIZES:
        x = cases.randn(f"host-s2d-{H}-{W}", (2, H, W, 8))
        got = R.space_to_depth2_ref(x)
        for Y in range((H + 1) // 2):
            for X in range((W + 1) // 2):
                for py in range(2):
                    for px in range(2):
                        y, xx = 2 * Y + py, 2 * X + px
                        want = x[:, y, xx] if y < H and xx < W else np.zeros((2, 8), dtype=F32)
                        assert np.array_equal(got[:, Y, X, (py * 2 + px) * 8:(py * 2 + px + 1) * 8], want)
    assert any(h & 1 for h, _ in cases.S2D_SIZES) and any(w & 1 for _, w in cases.S2D_SIZES) and (1, 1) in cases.S2D_SIZES


@pytest.mark.parametrize("size", cases.MAXPOOL_SIZES, ids=str)
def test_maxpool_ref_vs_brute(size):
    for kind in cases.MAXPOOL_KINDS:
        x = cases.maxpool_input(*size, 4, kind)
        a, b = R.maxpool_ref(x), R.maxpool_brute(x)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (size, kind)
        assert a.shape[1:3] == (R.pool_out(size[0]), R.pool_out(size[1]))
        if kind == "nan":
            assert np.isnan(a).any()
        if kind == "neginf":
            assert np.isneginf(a[..., 1]).all()


def test_maxpool_table_has_nan_at_every_tap_role():
    roles = set()
    for H, W in cases.MAXPOOL_SIZES:
        for _, y, x in cases.maxpool_nan_positions(H, W):
            for yo in range(R.pool_out(H)):
                for xo in range(R.pool_out(W)):
                    taps = [(yy, xx) for yy in range(2 * yo - 1, 2 * yo + 2) if 0 <= yy < H for xx in range(2 * xo - 1, 2 * xo + 2) if 0 <= xx < W]
                    if (y, x) in taps and len(taps) == 9:
                        roles.add({0: "first", 4: "middle", 8: "last"}.get(taps.index((y, x)), "other"))
    assert {"first", "middle", "last"} <= roles
    assert (1, 1) in cases.MAXPOOL_SIZES and any(h == 1 and w > 1 for h, w in cases.MAXPOOL_SIZES)


# ------------------------------------------------------------------------------------------------ nearest
@pytest.mark.parametrize("pair", cases.SIZE_PAIRS, ids=str)
def test_nearest_table_vs_torch(pair):
    i, o = pair
    idx = torch.arange(i, dtype=torch.float32).view(1, 1, 1, i)
    want = F.interpolate(idx, size=(1, o), mode="nearest").view(-1).long().numpy()
    assert np.array_equal(R.nearest_table(i, o), want)
    x = cases.randn(f"host-nearest-{pair}", (2, i, 3))
    want2 = F.interpolate(torch.from_numpy(x)[None], size=(o, 5), mode="nearest")[0].numpy()
    assert np.array_equal(R.resize_nearest_ref(x, o, 5), want2)


def test_nearest_fp32_pairs_differ_from_the_exact_quotient():
    """the search the cases file speaks of, restated for the two pairs kept: the fp32 rule and floor(o in / out) differ"""
    for i, o in R.NEAREST_FP32_PAIRS:
        assert (i, o) in cases.SIZE_PAIRS
        assert (R.nearest_table(i, o) != R.nearest_exact_table(i, o)).any()
    assert (R.nearest_table(26, 22)[11], R.nearest_exact_table(26, 22)[11]) == (12, 13)
    for i, o in ((45, 90), (90, 45), (7, 3), (61, 97)):
        assert np.array_equal(R.nearest_table(i, o), R.nearest_exact_table(i, o))


def test_resize_geometries_use_every_pair_on_both_axes():
    g = cases.resize_geometries(extra=True)
    assert {(a[0], a[2]) for a in g} >= set(cases.SIZE_PAIRS) and {(a[1], a[3]) for a in g} >= set(cases.SIZE_PAIRS)
    assert (23, 41, 24, 42) in g and (5, 1) in cases.SIZE_PAIRS and (1, 5) in cases.SIZE_PAIRS


# ------------------------------------------------------------------------------------------------ bilinear
def _bilinear_fp32(x, hd, wd, align):
    """the kernel's expression in numpy float32"""
    P, hs, ws = x.shape
    y0, y1, ly = R.bilinear_taps_fp32(hs, hd, align)
    x0, x1, lx = R.bilinear_taps_fp32(ws, wd, align)
    one = F32(1)
    lx, ly = lx[None, None, :], ly[None, :, None]
    g = lambda yy, xx: x[:, yy][:, :, xx]
    top = ((one - lx) * g(y0, x0) + lx * g(y0, x1)).astype(F32)
    bot = ((one - lx) * g(y1, x0) + lx * g(y1, x1)).astype(F32)
    return ((one - ly) * top + ly * bot).astype(F32)


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("geom", cases.resize_geometries(extra=True), ids=str)
def test_bilinear_ref(geom, align):
    """against torch in fp64 (the bound with fp64's unit), torch in fp32 and the float32 restatement (the bound itself)"""
    x = cases.resize_input(geom, 2)
    ref, bound = R.bilinear_ref(x, geom[2], geom[3], align)
    t = lambda v: F.interpolate(v[None], size=geom[2:], mode="bilinear", align_corners=bool(align))[0].numpy()
    _report(f"bilinear {geom} align{align}", torch64=R.ratio(t(T64(x)), ref, bound * U64),
            torch32=R.ratio(t(torch.from_numpy(x)), ref, bound), restated=R.ratio(_bilinear_fp32(x, geom[2], geom[3], align), ref, bound))


def test_bilinear_ref_at_the_workload_size():
    """360 x 640 -> 361 x 641, align_corners=False: the weight error of a few u * src is what a pure 6 u sum |w v| misses by
    two orders of magnitude; the derived dW covers torch's own fp32 result and the restatement"""
    x = cases.randn("host-bilinear-360x640", (1, 360, 640))
    ref, bound = R.bilinear_ref(x, 361, 641, 0)
    got = F.interpolate(torch.from_numpy(x)[None], size=(361, 641), mode="bilinear", align_corners=False)[0].numpy()
    Wy, _ = R.bilinear_weights(360, 361, 0)
    Wx, _ = R.bilinear_weights(640, 641, 0)
    pure = R.K2 * 6 * R.U * np.matmul(np.matmul(Wy, np.abs(x).astype(np.float64)), Wx.T)
    err = np.abs(got - ref)
    print(f"RATIO bilinear 360x640: against the pure rounding bound {float((err / pure).max()):.1f}")
    assert (err / pure).max() > 10          # the weight error is real, not slack
    _report("bilinear 360x640->361x641", torch32=R.ratio(got, ref, bound), restated=R.ratio(_bilinear_fp32(x, 361, 641, 0), ref, bound))


@pytest.mark.parametrize("pair", cases.SIZE_PAIRS + cases.BILINEAR_EXTRA + ((360, 361), (640, 641)), ids=str)
def test_bilinear_fp32_weights_inside_dW(pair):
    """the fp32 taps of the kernel's rule against the exact matrix, element by element, inside dW + u"""
    for align in (0, 1):
        W, dW = R.bilinear_weights(*pair, align)
        i0, i1, l = R.bilinear_taps_fp32(*pair, align)
        Wk = np.zeros_like(W)
        o = np.arange(pair[1])
        np.add.at(Wk, (o, i0), (F32(1) - l).astype(np.float64))
        np.add.at(Wk, (o, i1), l.astype(np.float64))
        assert R.ratio(W.sum(axis=1), np.ones(pair[1]), 4 * 2.0 ** -53) <= 1          # the rows of W sum to 1
        assert R.ratio(Wk, W, dW) <= 1.0


@pytest.mark.parametrize("size", cases.UP2_SIZES, ids=str)
def test_up2_ref_vs_torch(size):
    x = cases.randn(f"host-up2-{size}", (2,) + size + (4,))
    ref, bound = R.up2_ref(x)
    up = torch.nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
    t = lambda v: up(v.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    restated = np.stack([_bilinear_fp32(np.ascontiguousarray(x[b].transpose(2, 0, 1)), 2 * size[0], 2 * size[1], 1).transpose(1, 2, 0)
                         for b in range(2)])
    floor = 4 * 2.0 ** -53 * np.abs(ref)            # up2_weights' dW is 0 at n = 1; torch's fp64 still rounds
    _report(f"up2 {size}", torch64=R.ratio(t(T64(x)), ref, bound * U64 + floor), torch32=R.ratio(t(torch.from_numpy(x)), ref, bound),
            restated=R.ratio(restated, ref, bound))
    Wy, _ = R.up2_weights(size[0])
    Wg, _ = R.bilinear_weights(size[0], 2 * size[0], 1)
    assert np.array_equal(Wy, Wg)                  # the general rule restates the 2x matrix


# ------------------------------------------------------------------------------------------------ fold_bn
@pytest.mark.parametrize("n", cases.FOLD_N)
def test_fold_bn_ref(n):
    eps = float(F32(cases.FOLD_EPS))
    for off in range(4):
        x = cases.fold_inputs(n, off)
        for with_cb in (True, False):
            a, s, ba, bs = R.fold_bn_ref(x["cb"] if with_cb else None, x["gamma"], x["beta"], x["mean"], x["var"], cases.FOLD_EPS, n, 4)
            cb = T64(x["cb"] if with_cb else np.zeros(n, dtype=F32)).view(1, n, 1, 1)
            bn = lambda v, mean, beta: F.batch_norm(v, mean, T64(x["var"]), T64(x["gamma"]), beta, False, 0.0, eps).view(-1).numpy()
            want_s = bn(cb, T64(x["mean"]), T64(x["beta"]))
            want_a = bn(torch.ones(1, n, 1, 1, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
            assert np.array_equal(a[:n], a[n:2 * n]) and np.array_equal(s[:n], s[3 * n:]) and len(a) == 4 * n
            # the float32 restatement, in the kernel's order
            inv = (F32(1) / np.sqrt((x["var"] + F32(cases.FOLD_EPS)).astype(F32)).astype(F32)).astype(F32)
            ak = (x["gamma"] * inv).astype(F32)
            cbk = x["cb"] if with_cb else np.zeros(n, dtype=F32)
            sk = (((cbk - x["mean"]).astype(F32) * ak).astype(F32) + x["beta"]).astype(F32)
            # torch folds as x alpha + (beta - mean alpha): its own fp64 error stands on |x alpha| + |mean alpha|, not on |d a|
            slack = 8 * 2.0 ** -53 * ((np.abs(cb.view(-1).numpy()) + np.abs(x["mean"])) * np.abs(want_a) + np.abs(x["beta"]))
            _report(f"fold_bn n{n} off{off} cb{int(with_cb)}", torch_scale=R.ratio(want_a, a[:n], ba[:n] * U64 + 4 * 2.0 ** -53 * np.abs(a[:n])),
                    torch_shift=R.ratio(want_s, s[:n], slack), scale=R.ratio(ak, a[:n], ba[:n]), shift=R.ratio(sk, s[:n], bs[:n]))
    a, s, ba, bs = R.fold_bn_ref(x["cb"], None, None, None, None, cases.FOLD_EPS, n, 1)
    assert (a == 1).all() and np.array_equal(s, x["cb"].astype(np.float64)) and not ba.any() and not bs.any()
    assert set(cases.FOLD_VARS) == {0.0, 1e-12, 1.0, 1e6} and max(cases.FOLD_N) * max(cases.FOLD_REPEAT) > 256 > min(cases.FOLD_N)


# ------------------------------------------------------------------------------------------------ outconv
def _outconv_fp32(x, w, bias):
    """the kernel's tree in numpy float32: groups of four, two halves, one shuffle add, the bias"""
    B, H, W, cin = x.shape
    nc, ch = w.shape[0], cin // 2
    acc = np.zeros((2, B, H, W, nc), dtype=F32)
    for half in range(2):
        for c in range(half * ch, (half + 1) * ch, 4):
            p = (x[..., None, c:c + 4] * w[None, None, None, :, c:c + 4]).astype(F32)
            g = (((p[..., 0] + p[..., 1]).astype(F32) + p[..., 2]).astype(F32) + p[..., 3]).astype(F32)
            acc[half] = (acc[half] + g).astype(F32)
    return (((acc[0] + acc[1]).astype(F32) + bias).astype(F32)).transpose(0, 3, 1, 2)


OUTCONV_CASES = cases.outconv_cases()


@pytest.mark.parametrize("c", OUTCONV_CASES, ids=[c["id"] for c in OUTCONV_CASES])
def test_outconv_ref_and_tie_margin(c):
    """the reference against conv2d in fp64, the bound against the float32 tree, and the CONDITION the GPU test rests on: every
    top-2 margin of the fp64 logits exceeds SOFTMAX_TIE_MARGIN plus twice the logit bound, so no pixel's argmax can depend on
    rounding and the share of pixels inside the tie margin is zero"""
    x = cases.outconv_inputs(c)
    ref, bound = R.outconv_ref(x["x"], x["w"], x["bias"])
    want = F.conv2d(T64(x["x"]).permute(0, 3, 1, 2), T64(x["w"])[:, :, None, None], T64(x["bias"])).numpy()
    got = _outconv_fp32(x["x"], x["w"], x["bias"])
    _report(f"outconv {c['id']}", torch64=R.ratio(want, ref, bound * U64), restated=R.ratio(got, ref, bound))
    if c["nc"] > 1:
        room = R.top2_margin(ref) - 2 * np.partition(bound, -2, axis=1)[:, -2:].max(axis=1)
        assert (room > torch_ref.SOFTMAX_TIE_MARGIN).all(), (c["id"], float(room.min()))
        assert not torch_ref.softmax_argmax_may_differ(torch.from_numpy(got)).any()
        assert np.array_equal(R.argmax_scan(got), torch_ref.preds_to_masks(torch.from_numpy(got)).numpy())
    assert np.array_equal(R.argmax_scan(got), np.argmax(got, axis=1))


def test_outconv_table():
    cs = cases.outconv_cases()
    at = lambda **kw: [c for c in cs if all(c[k] == v for k, v in kw.items())]
    assert all(at(nc=nc, cin=64) for nc in range(1, 9))
    assert all(at(nc=nc, cin=cin) for nc in (4, 8) for cin in (8, 24, 64, 72, 1024))
    assert at(nc=8, cin=1024)[0]["shape"] == (1, 10, 13)
    assert {math.prod(c["shape"]) for c in cs} >= {1, 127, 128, 129, 133, 273, 130}
    assert at(out="logits") and at(out="argmax") and {(c["nc"],) + c["stn"] for c in cs if c["stn"]} == set(cases.OUTCONV_STN)
    assert len({c["id"] for c in cs}) == len(cs)


def test_outconv_tie_case_is_exact_and_holds_both_kinds_of_tie():
    x = cases.outconv_tie_inputs()
    ref, _ = R.outconv_ref(x["x"], x["w"], x["bias"])
    got = _outconv_fp32(x["x"], x["w"], x["bias"])
    assert np.array_equal(got.astype(np.float64), ref) and np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 2 ** 20
    assert np.array_equal(ref[:, 1], ref[:, 2])
    top = ref.max(axis=1)
    two_way = (ref[:, 1] == top) & (ref[:, 0] < top) & (ref[:, 3] < top)
    all_way = (ref == top[:, None]).all(axis=1)
    assert two_way.sum() >= 10 and all_way[0, 0, :5].all()
    am = R.argmax_scan(got)
    assert (am[two_way] == 1).all() and (am[all_way] == 0).all() and np.array_equal(am, np.argmax(ref, axis=1))


@pytest.mark.parametrize("row,want", cases.OUTCONV_NONFINITE, ids=[str(i) for i in range(len(cases.OUTCONV_NONFINITE))])
def test_argmax_rule_on_nonfinite_rows(row, want):
    """the kernel's rule restated as a scalar loop, and where it leaves the reference project's argmax(softmax(.)): that one
    answers 0 whenever the row holds a NaN or a +inf"""
    best, bv = 0, F32(row[0])
    for k in range(1, 4):
        if F32(row[k]) > bv:
            best, bv = k, F32(row[k])
    assert best == want
    lg = np.array(row, dtype=F32).reshape(1, 4, 1, 1)
    assert R.argmax_scan(lg).item() == want
    theirs = torch_ref.preds_to_masks(torch.from_numpy(lg)).item()
    assert theirs == (0 if (np.isnan(row).any() or np.inf in row) else want)


def test_nonfinite_table_names_the_divergence():
    rows = dict(cases.OUTCONV_NONFINITE)
    assert rows[(1.0, np.nan, 3.0, 0.5)] == 2 and rows[(1.0, 2.0, np.inf, 0.0)] == 2


def test_stn_in_ref():
    lg, fr = cases.randn("host-stn-l", (2, 5, 3, 4)), cases.randn("host-stn-f", (2, 3, 4, 8))
    want = torch.cat((torch.from_numpy(lg), torch.from_numpy(fr[..., :3]).permute(0, 3, 1, 2)), 1).permute(0, 2, 3, 1)
    got = R.stn_in_ref(lg, fr, 12)
    assert np.array_equal(got[..., :8], want.numpy()) and not got[..., 8:].any() and not np.signbit(got[..., 8:]).any()


# ------------------------------------------------------------------------------------------------ consistency CE
CE_CASES = [c for c in cases.ce_cases() if math.prod(c["shape"]) <= 40000]


@pytest.mark.parametrize("c", CE_CASES, ids=[c["id"] for c in CE_CASES])
def test_ce_ref_vs_torch(c):
    logits, mask = cases.ce_inputs(c)
    ref, bound = R.ce_ref(logits, mask)
    B, H, W = c["shape"]
    m = torch.from_numpy(mask)
    if tuple(c["mask"]) != (H, W):
        m = F.interpolate(m[:, None].float(), size=(H, W), mode="nearest")[:, 0]
    want = F.cross_entropy(T64(logits), m.long(), reduction="none").mean(dim=(1, 2)).numpy()
    ratios = dict(torch64=R.ratio(want, ref, bound * U64 + 4 * 2.0 ** -53 * np.abs(want)))
    if math.prod(c["shape"]) <= 1000:
        ratios["brute"] = R.ratio(R.ce_brute(logits, mask), ref, bound * U64 + 4 * 2.0 ** -53 * np.abs(want))
    # float32 restatement of the per-pixel term (numpy's expf / logf, T = 1), summed pairwise in fp32
    l = logits.reshape(B, c["nc"], -1)
    mx = l.max(axis=1, keepdims=True)
    se = np.exp((l - mx).astype(F32)).astype(F32).sum(axis=1, dtype=F32)
    t = R.ce_targets(mask, H, W).reshape(B, 1, -1).astype(np.int64)
    term = ((mx[:, 0] + np.log(se).astype(F32)).astype(F32) - np.take_along_axis(l, t, axis=1)[:, 0]).astype(F32)
    ratios["restated"] = R.ratio((term.sum(axis=1, dtype=np.float64) / (H * W)), *R.ce_ref(logits, mask, t_ulps=1.0))
    _report(f"ce {c['id']}", **ratios)


def test_ce_table():
    cs = cases.ce_cases()
    assert {c["nc"] for c in cs} == set(range(2, 9)) and {c["shape"][0] for c in cs} >= {1, 3}
    assert {c["shape"][1] * c["shape"][2] for c in cs} >= {1, 255, 2047, 2048, 2049, 5 * 2048 + 1, 257 * 512}
    assert R.ce_workspace_floats(1, 257, 512) == 65 and R.ce_workspace_floats(3, 32, 64) == 3 and R.ce_workspace_floats(1, 3, 683) == 2
    assert {(tuple(c["mask"]), c["shape"][1:]) for c in cs if tuple(c["mask"]) != c["shape"][1:]} == set(cases.CE_MASK_RESIZES)
    assert {c["kind"] for c in cs} == {"randn", "spread200", "equal", "big"}
    m = np.arange(45 * 56, dtype=np.int32).reshape(1, 45, 56)
    want = F.interpolate(torch.from_numpy(m)[:, None].float(), size=(91, 113), mode="nearest")[0, 0].numpy()
    assert np.array_equal(R.ce_targets(m, 91, 113)[0], want)


# ------------------------------------------------------------------------------------------------ avgpool + linear
def _avgpool_fp32(x, w, b):
    """the kernel's tree in numpy float32: four slices, four chains 16 pixels apart, the tail onto the first chain"""
    B, H, W, C = x.shape
    HW = H * W
    v = x.reshape(B, HW, C)
    part = []
    for sl in range(4):
        s = [np.zeros((B, C), dtype=F32) for _ in range(4)]
        i = sl
        while i + 12 < HW:
            for k in range(4):
                s[k] = (s[k] + v[:, i + 4 * k]).astype(F32)
            i += 16
        while i < HW:
            s[0] = (s[0] + v[:, i]).astype(F32)
            i += 4
        part.append(((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32))
    feat = (((part[0] + part[1]).astype(F32) + (part[2] + part[3]).astype(F32)).astype(F32) / F32(HW)).astype(F32)
    out = np.zeros((B, w.shape[0]), dtype=F32)
    for o in range(w.shape[0]):
        lane = np.zeros((B, 64), dtype=F32)
        for c0 in range(0, C, 64):
            n = min(64, C - c0)
            lane[:, :n] = (lane[:, :n] + (feat[:, c0:c0 + n] * w[o, c0:c0 + n]).astype(F32)).astype(F32)
        k = 32
        while k:
            lane[:, :k] = (lane[:, :k] + lane[:, k:2 * k]).astype(F32)
            k >>= 1
        out[:, o] = (lane[:, 0] + b[o]).astype(F32)
    return feat, out


AVG_CASES = cases.avgpool_cases()


@pytest.mark.parametrize("c", AVG_CASES, ids=[c["id"] for c in AVG_CASES])
def test_avgpool_linear_ref(c):
    x = cases.avgpool_inputs(c)
    rf, bf, ro, bo = R.avgpool_linear_ref(x["x"], x["w"], x["b"])
    tf = F.adaptive_avg_pool2d(T64(x["x"]).permute(0, 3, 1, 2), 1).flatten(1)
    to = F.linear(tf, T64(x["w"]), T64(x["b"]))
    kf, ko = _avgpool_fp32(x["x"], x["w"], x["b"])
    _report(f"avgpool {c['id']}", torch_feat=R.ratio(tf.numpy(), rf, bf * U64 * 16), torch_out=R.ratio(to.numpy(), ro, bo * U64 * 16),
            feat=R.ratio(kf, rf, bf), out=R.ratio(ko, ro, bo))
    # a wrong divisor or a dropped pixel is far outside the bound
    HW = c["shape"][1] * c["shape"][2]
    assert (np.abs(rf * HW / (HW + 1) - rf) > 1000 * bf).all()


def test_avgpool_table():
    cs = cases.avgpool_cases()
    assert {c["shape"][1] * c["shape"][2] for c in cs} >= {1, 3, 4, 12, 13, 16, 17, 29, 240}
    assert {c["shape"][3] for c in cs} == set(cases.AVG_C) and {c["nout"] for c in cs} == set(cases.AVG_NOUT)
    assert {c["shape"][0] for c in cs} == {1, 3}


# ------------------------------------------------------------------------------------------------ compose_up_weights
@pytest.mark.parametrize("padded", [False, True])
def test_compose_up_identity(padded):
    """conv3x3(pad(ConvTranspose2d(x))) = the 2x2 conv with w2 over the low-resolution x per output parity plus shift_border
    unfolded from scale and shift - in fp64 on tiny tensors, for every output parity and every one of the sixteen border
    classes, the F.pad case (a skip tensor one row and one column larger) included"""
    c1, c0, cout, cx, H, W = 3, 2, 2, 3, 2, 3
    x = cases.compose_inputs(c1, c0, cout, cx, dtype=np.float64, name=f"host-compose-{padded}")
    xin = torch.from_numpy(cases._rng("host-compose-x").standard_normal((1, cx, H, W)))
    u = F.conv_transpose2d(xin, T64(x["wt"]), T64(x["bt"]), stride=2)
    if padded:
        u = F.pad(u, [0, 1, 0, 1])
    z = F.conv2d(u, T64(x["wconv"])[:, c0:], padding=1)[0].numpy()
    sc, sh = x["scale4"], x["shift4"]
    w2, bw, sb, bs = R.compose_up_ref(x["wconv"], c0, x["wt"], x["bt"], sc, sh)
    xz = np.zeros((cx, H + 2, W + 2))
    xz[:, 1:H + 1, 1:W + 1] = xin[0].numpy()
    seen = set()
    worst = 0.0
    for r in range(z.shape[1]):
        for c in range(z.shape[2]):
            py, px, Y, X = r & 1, c & 1, r >> 1, c >> 1
            cls = 4 * R.border_class(r, 2 * H, padded) + R.border_class(c, 2 * W, padded)
            seen.add((py, px, cls))
            for co in range(cout):
                cv = (py * 2 + px) * cout + co
                win = xz[:, Y + py:Y + py + 2, X + px:X + px + 2]           # x[Y + py - 1 + a][X + px - 1 + b], zero outside
                conv = float((w2[cv] * win).sum())
                # shift_border = shift + scale * bias part; the epilogue is scale * conv + shift_border
                got = sc[cv] * conv + sb[cls, cv]
                want = sc[cv] * z[co, r, c] + sh[cv]
                mag = abs(sc[cv]) * np.abs(w2[cv] * win).sum() + abs(sb[cls, cv]) + abs(sh[cv])
                worst = max(worst, abs(got - want) / (64 * 2.0 ** -53 * mag))
    assert {(py, px) for py, px, _ in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if padded:
        assert {cls for _, _, cls in seen} == set(range(16))
    _report(f"compose identity padded{int(padded)}", identity=worst)


def test_compose_up_ref_brute():
    """the einsum against loops over taps, and the taps per slot and class the bound counts"""
    c1, c0, cout, cx = 5, 3, 2, 2
    x = cases.compose_inputs(c1, c0, cout, cx, dtype=np.float64, name="host-compose-brute")
    w2, _, sb, _ = R.compose_up_ref(x["wconv"], c0, x["wt"], x["bt"], x["scale4"], x["shift4"])
    want, mag = np.zeros_like(w2), np.zeros_like(w2)
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    (a, dy), (b, dx) = R.up_tap(py, ky), R.up_tap(px, kx)
                    assert 0 <= a <= 1 and 0 <= b <= 1
                    for co in range(cout):
                        for xx in range(cx):
                            t = x["wconv"][co, c0:, ky, kx] * x["wt"][xx, :, dy, dx]
                            want[(py * 2 + px) * cout + co, xx, a, b] += t.sum()
                            mag[(py * 2 + px) * cout + co, xx, a, b] += np.abs(t).sum()
    assert R.ratio(w2, want, 64 * 2.0 ** -53 * mag) <= 1.0
    for cls in range(16):
        for cv in range(4 * cout):
            taps = [x["wconv"][cv % cout, c0:, ky, kx] * x["bt"] for ky in range(3) for kx in range(3)
                    if R.tap_inside(cls >> 2, ky) and R.tap_inside(cls & 3, kx)]
            acc, aacc = sum(t.sum() for t in taps), sum(np.abs(t).sum() for t in taps)
            want_sb = x["shift4"][cv] + x["scale4"][cv] * acc
            assert abs(sb[cls, cv] - want_sb) <= 64 * 2.0 ** -53 * (abs(x["shift4"][cv]) + abs(x["scale4"][cv]) * aacc)
    assert max(sum(1 for k in range(3) if R.up_tap(p, k)[0] == a) for p in range(2) for a in range(2)) == 2     # 2 x 2 = 4 taps per slot at most


def test_compose_table():
    g = cases.COMPOSE_CASES
    assert {c[0] for c in g} == {16, 32, 48, 80} and {c[1] for c in g} == {0, 16, 80}
    assert {c[2] for c in g} == {16, 48} and {c[3] for c in g} == {16, 48}
