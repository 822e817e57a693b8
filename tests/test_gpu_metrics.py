"""The registration metrics on the GPU (csrc/metrics.hip, sfh_amd.metrics) against the numpy restatement tests/metrics_ref.py,
which tests/test_metrics_host.py holds against counts derived by hand.

Conventions of tests/test_gpu_step_tail.py, whose helpers are imported: every output ends in a guard of 64 sentinel elements that
must come back untouched, and starts as garbage, because the entries overwrite.  The confusion and region counts are integers and
must be EQUAL; the point errors lie within the one bound that metrics_ref.py derives (printed as RATIO, asserted <= 1), their
counts are exact, and the cases that must be exact are asserted exact."""
import numpy as np
import pytest
import torch

import metrics_cases as C
import metrics_ref as R
from test_gpu_step_tail import GUARD, NAN, Guarded, K, _dev, _report  # noqa: F401  (K is the fixture)

pytestmark = pytest.mark.gpu

GARBAGE = -0x0123456789ABCDEF


def _ok(K, rc):
    assert rc == 0, K[0].sfh_last_error()


def _flag(value=0):
    return Guarded((1,), torch.int32, value)


def _confusion(K, pred, kind, gt, nc, flag=None):
    lib, _ptr, _stream = K
    B, H, W = gt.shape
    out = Guarded((B, nc, nc), torch.int64, GARBAGE)
    flag = flag or _flag()
    pd, gd = _dev(pred), _dev(gt)
    _ok(K, lib.sfh_metrics_confusion(_ptr(pd), kind, _ptr(gd), nc, B, H, W, _ptr(out.t), _ptr(flag.t), _stream()))
    return out.result(), int(flag.result()[0])


def _check_confusion(K, pred, kind, gt, nc, want_flag=0, what=""):
    got, flag = _confusion(K, pred, kind, gt, nc)
    want, ref_flag = R.confusion_ref(pred, kind, gt, nc)
    assert ref_flag == want_flag and flag == want_flag, (what, flag, want_flag)
    assert np.array_equal(got, want), (what, got, want)
    if not want_flag & 2:      # every pixel with a valid gt id is in its row
        assert np.array_equal(got.sum(axis=2), np.stack([(gt == g).sum(axis=(1, 2)) for g in range(nc)], axis=1)), what
    return got


# ------------------------------------------------------------------------------------------------ sfh_metrics_confusion
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_confusion_counts(K, shape, kind):
    """every count equal to np.add.at over the reference classes; kind 2 against the logits' argmax rule; B 1 and 3 (the full
    frame: 1), nc 2, 4, 7, 8; ignored pixels scattered through every frame"""
    for B in C.batches_of(shape):
        for nc in C.CLASSES:
            pred, gt = C.random_case(shape, B, nc, kind)
            _check_confusion(K, pred, kind, gt, nc, what=(shape, kind, B, nc))


@pytest.mark.parametrize("name", C.SPECIAL_NAMES)
@pytest.mark.parametrize("shape", C.SPECIAL_SHAPES, ids=str)
def test_confusion_special_cases(K, shape, name):
    """all ignored; ignored scattered; one class everywhere; every key inside every wave; exact ties; the header's non-finite
    rows; the warp value whose fp32 product rounds up; flag bit 1, bit 2, both - on the scalar and on the 16-byte path"""
    pred, kind, nc, gt, flag = C.special_cases(shape)[name]
    got = _check_confusion(K, pred, kind, gt, nc, want_flag=flag, what=(shape, name))
    if name.startswith("all-ignored"):
        assert not got.any()
    if name.startswith("single-class"):
        assert got[:, 1, 1].tolist() == [shape[0] * shape[1]] * 2 and got.sum() == 2 * shape[0] * shape[1]
    if name == "warp-rounds-up":
        v, k, ncu = C.rounds_up_value()
        assert got[0, :, k].sum() >= (shape[0] * shape[1] + 1) // 2


def test_confusion_unaligned_and_sticky_flag(K):
    """a prediction and a mask that start off the 16-byte grid take the scalar path to the same counts; the flag is only ever
    ORed into"""
    lib, _ptr, _stream = K
    pred, gt = C.random_case((65, 64), 1, 4, 3)
    want, _ = R.confusion_ref(pred, 3, gt, 4)
    n = gt.size
    pbuf, gbuf = torch.zeros(n + 1, dtype=torch.float32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    pbuf[1:] = _dev(pred).reshape(-1)
    gbuf[1:] = _dev(gt).reshape(-1)
    out, flag = Guarded((1, 4, 4), torch.int64, GARBAGE), _flag(2)
    _ok(K, lib.sfh_metrics_confusion(_ptr(pbuf[1:]), 3, _ptr(gbuf[1:]), 4, 1, 65, 64, _ptr(out.t), _ptr(flag.t), _stream()))
    assert np.array_equal(out.result(), want) and int(flag.result()[0]) == 2
    bad = gt.copy()
    bad[0, 0, 0] = 9
    _, got = _confusion(K, pred, 3, bad, 4, flag=flag)
    assert got == 3


# ------------------------------------------------------------------------------------------------ sfh_metrics_region
def _region(K, tp, tg, mode, raster, margin):
    lib, _ptr, _stream = K
    tp, tg = np.asarray(tp, np.float32).reshape(-1, 9), np.asarray(tg, np.float32).reshape(-1, 9)
    out = Guarded((len(tp), 3), torch.int64, GARBAGE)
    a, b = _dev(tp), _dev(tg)
    _ok(K, lib.sfh_metrics_region(_ptr(a), _ptr(b), len(tp), mode, raster[0], raster[1], margin[0], margin[1], _ptr(out.t),
                                  _stream()))
    return out.result()


@pytest.mark.parametrize("case", C.hand_cases(), ids=lambda c: c[0])
def test_region_hand_counts(K, case):
    """identity; diag(.5, .5, 1) with the boundary between and ON pixel centres; a rank-deficient and an all-NaN theta"""
    _, mode, raster, margin, tp, tg, expect = case
    assert _region(K, tp, tg, mode, raster, margin)[0].tolist() == expect


@pytest.mark.parametrize("raster", C.RASTERS, ids=str)
def test_region_counts(K, raster):
    """equal to the restatement, count for count: both modes, margins 0, 1 and half the raster, B 1 and 3 with a different theta
    per frame (the horizon theta among them); equal thetas give three equal counts; swapping swaps nA and nB in mode 0"""
    for margin in C.margins(raster):
        for mode in (0, 1):
            for tp, tg in C.region_batches():
                got = _region(K, tp, tg, mode, raster, margin)
                assert np.array_equal(got, R.region_ref(tp, tg, mode, *raster, *margin)), (raster, margin, mode, got)
                if mode == 0:
                    assert np.array_equal(_region(K, tg, tp, 0, raster, margin), got[:, [1, 0, 2]])
            for theta in (C.DYADIC,) + ((C.perspective("a"),) if mode == 0 else ()):
                n = _region(K, theta, theta, mode, raster, margin)[0]
                assert n[0] == n[1] == n[2] > 0, (raster, margin, mode, n)
                assert np.array_equal(n, R.region_ref(theta, theta, mode, *raster, *margin)[0])


def test_region_horizon_is_sign_blind(K):
    blind = R.region_ref(C.HORIZON, C.IDENTITY, 0, 320, 180, 0, 0)
    signed = R.region_ref(C.HORIZON, C.IDENTITY, 0, 320, 180, 0, 0, signed=True)
    got = _region(K, C.HORIZON, C.IDENTITY, 0, (320, 180), (0, 0))
    assert np.array_equal(got, blind) and got[0, 0] > signed[0, 0]


# ------------------------------------------------------------------------------------------------ sfh_metrics_points
SCALES = (320.0, 180.0, 32.2326 / 2, 17.145 / 2)


def _points(K, tp, tg, pts, lattice=(16, 9), scales=SCALES):
    lib, _ptr, _stream = K
    tp, tg = np.asarray(tp, np.float32).reshape(-1, 9), np.asarray(tg, np.float32).reshape(-1, 9)
    out = Guarded((len(tp), 4), torch.float64, 12345.0)
    a, b, p = _dev(tp), _dev(tg), _dev(np.asarray(pts, dtype=np.float64))
    _ok(K, lib.sfh_metrics_points(_ptr(a), _ptr(b), len(tp), _ptr(p), len(pts), lattice[0], lattice[1], *scales, _ptr(out.t),
                                  _stream()))
    return out.result()


def test_points_exact_cases(K):
    """identical thetas: 0 exactly.  A dyadic translation t along one axis against the identity: every point is counted, every
    court point moves by exactly t in the frame (u - t and the scaling by 320 or 180 are exact, sqrt(d d) = |d|), every lattice
    point by exactly t on the court (scale 1/2), and n equal terms of a few bits sum exactly: the means are |t| * scale."""
    pts = C.court_points()
    same = C.random_pairs(3, "same")[0]
    got = _points(K, same, same, pts)
    want, _ = R.points_ref(same, same, pts, 16, 9, *SCALES)
    assert (got[:, [0, 2]] == 0).all() and np.array_equal(got, want)
    tp = np.stack([C.translation(.125, 0), C.translation(0, -.25), C.translation(-.5, 0)])
    got = _points(K, tp, np.stack([C.IDENTITY] * 3), pts, scales=(320.0, 180.0, 0.5, 0.5))
    assert got.tolist() == [[40.0, 35.0, 0.0625, 144.0], [45.0, 35.0, 0.125, 144.0], [160.0, 35.0, 0.25, 144.0]]


@pytest.mark.parametrize("name,B,lattice", [("one", 1, (16, 9)), ("three", 3, (16, 9)), ("odd", 3, (7, 5)), ("wide", 2, (67, 3))])
def test_points_bound(K, name, B, lattice):
    """general thetas, more points than lanes: the means within the bound of metrics_ref.py, the counts exact"""
    tp, tg = C.random_pairs(B, name)
    pts = C.many_points()
    got = _points(K, tp, tg, pts, lattice)
    want, bound = R.points_ref(tp, tg, pts, *lattice, *SCALES)
    assert (want[:, 1] > 64).any() and (bound[:, [0, 2]] > 0).all()
    _report(f"points {name}", worst=R.points_ratio(got, want, bound))


def test_points_without_points_and_degenerate(K):
    """no visible point / no lattice point on the court: 0 / 0 = NaN; a theta_pred that is not usable, and one whose Wp is 0 at
    a counted point: a mean that is not finite, with the count intact"""
    pts = C.court_points()
    tiny, huge = np.diag([.01, .01, 1]).reshape(9), np.diag([100., 100., 1]).reshape(9)
    zero_w = np.array([1, 0, 0, 0, 1, 0, 16, 0, -1], dtype=np.float32)       # adj's last row (-16, 0, 1): Wp = 0 at u = 1/16
    tp = np.stack([C.IDENTITY, C.IDENTITY, np.zeros(9), C.RANK2, zero_w]).astype(np.float32)
    tg = np.stack([tiny, huge, C.IDENTITY, C.IDENTITY, C.IDENTITY]).astype(np.float32)
    got = _points(K, tp, tg, pts)
    want, bound = R.points_ref(tp, tg, pts, 16, 9, *SCALES)
    assert want[0, 1] == 0 and want[0, 3] == 144 and want[1, 1] == 35 and want[1, 3] == 0
    assert np.isnan(got[0, 0]) and np.isnan(got[1, 2]) and np.isfinite(got[0, 2]) and np.isfinite(got[1, 0])
    assert not np.isfinite(got[2:, 0]).any() and not np.isfinite(got[2:4, 2]).any() and (got[2:, 1] == 35).all()
    _report("points degenerate", worst=R.points_ratio(got, want, bound))


# ------------------------------------------------------------------------------------------------ the Python layer
def _scene(B, seed, H=36, W=64, nc=4):
    r = C.rng(("scene", B, seed))
    tp, tg = C.random_pairs(B, ("scene", seed), 0.1)
    gt = r.integers(0, nc, (B, H, W)).astype(np.int64)
    gt[r.random(gt.shape) < 0.05] = C.IGNORE
    logits = r.standard_normal((B, nc, H, W)).astype(np.float32)
    warp = r.integers(0, nc, (B, H, W)).astype(np.int32)
    return tp.reshape(B, 3, 3), tg.reshape(B, 3, 3), gt, logits, warp


def test_accumulator_rows_are_the_entries(K):
    """add twice, then table(): row for row the direct entries (through the raw C calls above)"""
    from sfh_amd import metrics as M
    pts = C.court_points()
    m = M.RegistrationMetrics(4, (80, 45), (64, 36), pts, units="meters", lattice=(7, 5))
    rows = []
    for B, seed in ((3, 1), (2, 2)):
        tp, tg, gt, logits, warp = _scene(B, seed)
        m.add(_dev(tp).view(B, 1, 3, 3), _dev(tg), _dev(gt), logits=_dev(logits), warp_mask=_dev(warp),
              names=[f"f{seed}-{i}" for i in range(B)] if seed == 1 else None)
        rows.append((_region(K, tp, tg, 0, (80, 45), (0, 0)), _region(K, tp, tg, 1, (80, 45), (40, 22)),
                     _points(K, tp, tg, pts, (7, 5), (32.0, 18.0, 32.2326 / 2, 17.145 / 2)),
                     _confusion(K, logits, 2, gt, 4)[0], _confusion(K, warp, 0, gt, 4)[0]))
    assert len(m) == 5
    t = m.table()
    part, whole, pt, cs, cw = (np.concatenate([r[k] for r in rows]) for k in range(5))
    assert t["names"].tolist() == ["f1-0", "f1-1", "f1-2", "3", "4"]
    assert np.array_equal(t["part_counts"], part) and np.array_equal(t["whole_counts"], whole)
    assert np.array_equal(t["reproj_px"], pt[:, 0]) and np.array_equal(t["proj_err"], pt[:, 2])
    assert np.array_equal(t["n_pts"], pt[:, 1]) and np.array_equal(t["n_lattice"], pt[:, 3])
    assert np.array_equal(t["conf_seg"], cs) and np.array_equal(t["conf_warp"], cw)
    assert np.array_equal(t["iou_part"], M.iou_ratio(part[:, 0], part[:, 1], part[:, 2]))
    s = m.summary()
    assert s["frames"] == 5 and s["seg"]["pixels"] == int((np.concatenate([_scene(3, 1)[2], _scene(2, 2)[2]]) >= 0).sum())
    # the direct functions are those entries too
    tp, tg, gt, logits, warp = _scene(3, 1)
    assert np.array_equal(M.region_counts(_dev(tp), _dev(tg), "whole", (80, 45)).cpu().numpy(), rows[0][1])
    assert np.array_equal(M.point_errors(_dev(tp), _dev(tg), _dev(pts), (64, 36), lattice=(7, 5)).cpu().numpy(), rows[0][2])
    counts, flag = M.confusion(_dev(warp.astype(np.uint8)), _dev(gt), 4)
    assert np.array_equal(counts.cpu().numpy(), rows[0][4]) and flag.item() == 0
    with pytest.raises(ValueError, match="names"):
        m.add(_dev(tp), _dev(tg), _dev(gt), logits=_dev(logits), warp_mask=_dev(warp), names=["one"])
    with pytest.raises(ValueError, match="earlier batches"):
        m.add(_dev(tp), _dev(tg), _dev(gt), logits=_dev(logits))


def test_accumulator_flag_raises_at_table(K):
    from sfh_amd import metrics as M
    m = M.RegistrationMetrics(4, (8, 8), (64, 36), C.court_points())
    tp, tg, gt, logits, warp = _scene(2, 3)
    m.add(_dev(tp), _dev(tg), _dev(gt), warp_mask=_dev(warp))
    warp[1, 2, 3] = 4
    m.add(_dev(tp), _dev(tg), _dev(gt), warp_mask=_dev(warp))
    with pytest.raises(ValueError, match="predicted class outside"):
        m.table()


def _net(W, H, B, seed):
    from test_gpu_eval import _net as eval_net
    return eval_net(W, H, B, seed)


def _loader(sizes, H, W, seed):
    from sfh_amd import synth
    out = []
    for i, B in enumerate(sizes):
        r = C.rng(("loader", seed, i))
        gt = r.integers(0, 4, (B, H, W)).astype(np.int64)
        gt[r.random(gt.shape) < 0.02] = C.IGNORE
        out.append({"image": synth.smooth_frames(B, H, W, seed=seed + i), "mask": torch.from_numpy(gt),
                    "theta": torch.from_numpy(C.random_pairs(B, ("loader", seed, i), 0.1)[1].reshape(B, 3, 3)),
                    "name": [f"b{i}-{k}" for k in range(B)]})
    return out


def test_evaluate_registration(K):
    """two batches through predict(): without a refiner there is no theta_stn; with one both are scored, the theta_stn table is
    the metrics of predict()'s own outputs bit for bit, and the net is back in train mode; an empty loader raises"""
    from sfh_amd import metrics as M
    from sfh_amd.refine import ThetaRefiner
    W, H = 96, 64
    net = _net(W, H, 4, seed=43)
    loader = _loader([4, 3], H, W, seed=900)
    plain = M.evaluate_registration(net, loader, "cuda", lattice=(7, 5))
    assert net.training and "theta_stn" not in plain and "frames_stn" not in plain
    assert plain["theta"]["frames"] == 7 and plain["frames"]["names"].tolist() == [n for b in loader for n in b["name"]]
    assert "seg" in plain["theta"] and "warp" in plain["theta"]
    rescales = net.range_rescales

    net.refiner = ThetaRefiner(net.court_img, mask_classes=4, grid_size=net.warp_size, factors=(4, 2), iters=2)
    res = M.evaluate_registration(net, loader, "cuda", lattice=(7, 5))
    assert net.training and res["theta_stn"]["frames"] == res["theta"]["frames"] == 7
    direct = {k: M.RegistrationMetrics(4, (W, H), (W, H), net.court_poi[0], lattice=(7, 5)) for k in ("theta", "theta_stn")}
    net.eval()
    with torch.no_grad():
        for b in loader:
            p = net.predict(b["image"].cuda(), consistency=False)
            gt, th = b["mask"].cuda(), b["theta"].cuda()
            direct["theta"].add(p["theta"], th, gt, logits=p["logits"], warp_mask=p["warp_mask"], names=b["name"])
            direct["theta_stn"].add(p["theta_stn"], th, gt, logits=p["logits"], names=b["name"])
    net.train()
    for key, frames in (("theta", "frames"), ("theta_stn", "frames_stn")):
        want = direct[key].table()
        assert set(want) == set(res[frames])
        for col in want:
            a, b = res[frames][col], want[col]
            assert a.tolist() == b.tolist() if a.dtype == object else np.array_equal(a, b, equal_nan=True), (key, col)
    assert "conf_warp" not in res["frames_stn"] and "conf_warp" in res["frames"]
    # the STN's own theta is the plain model's: refinement changed theta, not what it started from
    if net.range_rescales == rescales:      # (a range event between the calls changes the forward's bits)
        assert np.array_equal(res["frames_stn"]["part_counts"], plain["frames"]["part_counts"])
    with pytest.raises(ValueError, match="empty"):
        M.evaluate_registration(net, [], "cuda")
    with pytest.raises(ValueError, match="theta"):
        M.evaluate_registration(net, [{k: v for k, v in loader[0].items() if k != "theta"}], "cuda")
    assert net.training
