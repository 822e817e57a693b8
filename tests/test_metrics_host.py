"""Registration metrics without a GPU: the numpy restatement (tests/metrics_ref.py) against counts derived by hand, the summary
arithmetic of sfh_amd.metrics on hand-made tables, every ValueError of the Python layer, the flag refusal, and the C entries'
argument checks (which return before anything touches a device)."""
import numpy as np
import pytest
import torch

import metrics_cases as C
import metrics_ref as R


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", C.hand_cases(), ids=lambda c: c[0])
def test_restatement_gives_the_hand_counts(case):
    _, mode, (wc, hc), (mx, my), tp, tg, expect = case
    assert R.region_ref(tp, tg, mode, wc, hc, mx, my)[0].tolist() == expect


def test_restatement_region_properties():
    """theta_pred == theta_gt: the three counts agree, in both modes (whole: on the dyadic theta, where theta adj(theta) is exact);
    swapping the thetas swaps nA and nB in mode 0"""
    for wc, hc in C.RASTERS:
        for m in C.margins((wc, hc)):
            for mode, theta in ((0, C.perspective("a")), (0, C.DYADIC), (1, C.DYADIC)):
                n = R.region_ref(theta, theta, mode, wc, hc, *m)[0]
                assert n[0] == n[1] == n[2], (wc, hc, m, mode, n)
            if mode == 1:
                assert n[0] == wc * hc
            for tp, tg in C.region_batches():
                a, b = R.region_ref(tp, tg, 0, wc, hc, *m), R.region_ref(tg, tp, 0, wc, hc, *m)
                assert np.array_equal(a[:, [1, 0, 2]], b)


def test_predicate_is_blind_to_the_sign_of_w():
    """the horizon theta: W changes sign inside the canvas, and the stated rule counts the far side too"""
    blind = R.region_ref(C.HORIZON, C.IDENTITY, 0, 80, 45, 0, 0)[0]
    signed = R.region_ref(C.HORIZON, C.IDENTITY, 0, 80, 45, 0, 0, signed=True)[0]
    assert blind[0] > signed[0] > 0 and blind[1] == signed[1] == 3600
    # by hand: rows with yn <= 1/4 (W > 0), and rows with yn >= 1/2 under |xn| <= 3 yn - 1
    a, b, c = R.canvas(80, 45, 0, 0)
    xn, yn = a / c, b / c
    assert signed[0] == int(((yn <= 0.25) & (np.abs(xn) <= 1 - 3 * yn)).sum())
    assert blind[0] - signed[0] == int(((yn >= 0.5) & (np.abs(xn) <= 3 * yn - 1)).sum())


def test_restatement_classes():
    rows = np.array([[1, np.nan, 3, .5], [1, 2, np.inf, 0], [np.nan, 5, 6, 7], [2, 2, 1, 2], [0, 0, 0, 0]], dtype=np.float32)
    assert R.argmax_rule(rows.T.reshape(1, 4, 5, 1)).reshape(-1).tolist() == [2, 2, 0, 0, 0]
    v, k, nc = C.rounds_up_value()
    ids, ok = R.predicted_classes(np.array([[[v]]], dtype=np.float32), 3, nc)
    assert ok.all() and ids.item() == k and int(float(v) * nc) == k - 1
    ids, ok = R.predicted_classes(np.array([[[np.nan, 1.0, -0.2, -0.25, 0.99]]], dtype=np.float32), 3, 4)
    assert ok.reshape(-1).tolist() == [False, False, True, False, True] and ids.reshape(-1).tolist() == [0, 0, 0, 0, 3]


@pytest.mark.parametrize("name", C.SPECIAL_NAMES)
def test_restatement_confusion_cases(name):
    pred, kind, nc, gt, flag = C.special_cases((5, 7))[name]
    out, got = R.confusion_ref(pred, kind, gt, nc)
    assert got == flag
    if not flag & 2:
        assert np.array_equal(out.sum(axis=2), np.stack([(gt == g).sum(axis=(1, 2)) for g in range(nc)], axis=1))


def test_restatement_points():
    pts = C.court_points()
    same = C.random_pairs(3, "same")[0]
    out, bound = R.points_ref(same, same, pts, 16, 9, 320.0, 180.0, 16.1163, 8.5725)
    assert (out[:, [0, 2]] == 0).all() and (bound == 0).all()
    # a dyadic translation along one axis against the identity: every point is counted and every error is |t| * scale
    tp = np.stack([C.translation(.125, 0), C.translation(0, -.25)])
    out, _ = R.points_ref(tp, np.stack([C.IDENTITY] * 2), pts, 16, 9, 320.0, 180.0, 0.5, 0.5)
    assert out.tolist() == [[40.0, 35.0, 0.0625, 144.0], [45.0, 35.0, 0.125, 144.0]]


# ------------------------------------------------------------------------------------------------ summary arithmetic
def test_class_scores_by_hand():
    from sfh_amd import metrics as M
    conf = np.array([[[5, 1, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 3]],
                     [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]])
    s = M.class_scores(conf)
    # summed: class 0 tp 6 of 6 + 1 + 2, class 1 tp 2 of 2 + 2 + 2, class 2 absent from both sides, class 3 tp 3 of 3 + 1
    assert s["iou"][:2].tolist() == [6 / 9, 2 / 6] and np.isnan(s["iou"][2]) and s["iou"][3] == 3 / 4
    assert s["miou"] == pytest.approx((6 / 9 + 2 / 6 + 3 / 4) / 3, rel=1e-15) and s["pixel_acc"] == 11 / 15 and s["pixels"] == 15
    empty = M.class_scores(np.zeros((4, 4), dtype=np.int64))
    assert np.isnan(empty["iou"]).all() and np.isnan(empty["miou"]) and np.isnan(empty["pixel_acc"])
    with pytest.raises(ValueError, match="shape"):
        M.class_scores(np.zeros((3, 4)))


def test_figure_stats_by_hand():
    from sfh_amd import metrics as M
    s = M.figure_stats([4.0, np.nan, 1.0, np.inf, 3.0, 2.0])
    assert (s["mean"], s["median"], s["n"], s["nonfinite"]) == (2.5, 2.5, 4, 2)          # even count: the two middle ones
    assert s["p90"] == pytest.approx(3.7, rel=1e-15)                                   # 1 2 3 4 at rank 2.7
    s = M.figure_stats([np.nan, -np.inf])
    assert np.isnan([s["mean"], s["median"], s["p90"]]).all() and (s["n"], s["nonfinite"]) == (0, 2)


def test_table_and_summary_by_hand():
    from sfh_amd import metrics as M
    part = [[10, 20, 10], [0, 0, 0], [8, 8, 8]]
    whole = [[100, 100, 50], [100, 100, 100], [0, 100, 0]]
    pts = [[1.5, 30, 0.25, 144], [np.nan, 0, 0.5, 100], [np.inf, 33, np.nan, 0]]
    conf = np.zeros((3, 2, 2), dtype=np.int64)
    conf[:, 0, 0], conf[:, 1, 0] = 3, 1
    t = M.rows_to_table(["a", "b", "c"], part, whole, pts, conf_seg=conf)
    assert t["iou_part"][[0, 2]].tolist() == [0.5, 1.0] and np.isnan(t["iou_part"][1])
    assert t["iou_whole"].tolist() == [50 / 150, 1.0, 0.0]
    assert t["n_pts"].tolist() == [30, 0, 33] and t["n_lattice"].tolist() == [144, 100, 0] and t["names"].tolist() == ["a", "b", "c"]
    s = M.summarize(t)
    assert s["frames"] == 3 and "warp" not in s and s["seg"]["iou"].tolist() == [0.75, 0.0] and s["seg"]["pixel_acc"] == 0.75
    assert (s["iou_part"]["n"], s["iou_part"]["nonfinite"], s["iou_part"]["median"]) == (2, 1, 0.75)
    assert (s["reproj_px"]["n"], s["reproj_px"]["nonfinite"], s["reproj_px"]["mean"]) == (1, 2, 1.5)
    assert (s["proj_err"]["n"], s["proj_err"]["nonfinite"], s["proj_err"]["median"]) == (2, 1, 0.375)
    with pytest.raises(ValueError, match="names"):
        M.rows_to_table(["a"], part, whole, pts)
    with pytest.raises(ValueError, match="conf_warp"):
        M.rows_to_table(["a", "b", "c"], part, whole, pts, conf_warp=conf[:2])


def test_flag_refusal():
    from sfh_amd import metrics as M
    M.check_flag(0)
    with pytest.raises(ValueError, match=r"mask id outside \[0, mask_classes\) other than -100; F.cross_entropy"):
        M.check_flag(1)
    with pytest.raises(ValueError, match=r"^registration metrics: a predicted class outside .*non-finite warp included"):
        M.check_flag(np.int64(2))
    with pytest.raises(ValueError, match="other than -100 and a predicted class"):
        M.check_flag(3)


# ------------------------------------------------------------------------------------------------ every ValueError
def test_argument_errors():
    """the checks run in front of anything that needs a device; a well-formed CPU tensor is refused last, for being one"""
    from sfh_amd import metrics as M
    gt = torch.zeros((2, 4, 6), dtype=torch.int64)
    ids = torch.zeros((2, 4, 6), dtype=torch.int32)
    th = torch.eye(3).repeat(2, 1, 1)
    pts = torch.zeros((5, 2), dtype=torch.float64)
    for nc in (1, 9):
        with pytest.raises(ValueError, match="n_classes"):
            M.confusion(ids, gt, nc)
    with pytest.raises(ValueError, match="gt: dtype"):
        M.confusion(ids, gt.int(), 4)
    with pytest.raises(ValueError, match="gt: 2 dimensions"):
        M.confusion(ids, gt[0], 4)
    with pytest.raises(ValueError, match="pred: dtype"):
        M.confusion(ids.double(), gt, 4)
    with pytest.raises(ValueError, match="gt: not contiguous"):
        M.confusion(ids, gt.transpose(1, 2), 4)
    with pytest.raises(ValueError, match="pred: expected a tensor"):
        M.confusion(ids.numpy(), gt, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        M.confusion(ids, gt, 4)
    for bad in ((1, 5), (5, 1), (5,), "ab"):
        with pytest.raises(ValueError, match="court_size"):
            M.region_counts(th, th, "part", bad)
    with pytest.raises(ValueError, match="mode"):
        M.region_counts(th, th, 2, (8, 8))
    with pytest.raises(ValueError, match="margin"):
        M.region_counts(th, th, "whole", (8, 8), margin=(-1, 0))
    with pytest.raises(ValueError, match="theta_pred: dtype"):
        M.region_counts(th.double(), th, "part", (8, 8))
    with pytest.raises(ValueError, match=r"theta_gt: \(2, 9\)|theta_gt: 2 dimensions"):
        M.region_counts(th, th.reshape(2, 9), "part", (8, 8))
    with pytest.raises(ValueError, match="theta_pred: not contiguous"):
        M.region_counts(th.transpose(1, 2), th, "part", (8, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        M.region_counts(th, th, "whole", (8, 8))
    with pytest.raises(ValueError, match="units"):
        M.point_errors(th, th, pts, (640, 360), units="yards")
    with pytest.raises(ValueError, match="lattice"):
        M.point_errors(th, th, pts, (640, 360), lattice=(0, 9))
    with pytest.raises(ValueError, match="frame_size"):
        M.point_errors(th, th, pts, (0, 360))
    with pytest.raises(ValueError, match="no CPU path"):
        M.point_errors(th, th, pts, (640, 360))
    for kw, what in ((dict(mask_classes=9), "n_classes"), (dict(court_size=(1, 1)), "court_size"), (dict(units="yards"), "units"),
                     (dict(court_pts=np.zeros((3, 3))), "court_pts"), (dict(frame_size=(0, 0)), "frame_size")):
        args = dict(mask_classes=4, court_size=(8, 8), frame_size=(64, 36), court_pts=np.zeros((3, 2)))
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            M.RegistrationMetrics(**args)
    m = M.RegistrationMetrics(4, (8, 8), (64, 36), np.zeros((3, 2)))
    with pytest.raises(ValueError, match="no batch"):
        m.table()
    assert M.court_scale("meters") == (32.2326 / 2, 17.145 / 2) and M.default_margin((81, 45)) == (40, 22)


def test_driver_refuses_an_empty_loader_and_a_cpu_device():
    from sfh_amd import metrics as M
    with pytest.raises(ValueError, match="empty"):
        M.evaluate_registration(None, [], "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.evaluate_registration(None, [{}], "cpu")


# ------------------------------------------------------------------------------------------------ the C entries' refusals
def test_entries_refuse_bad_arguments_without_a_device():
    from sfh_amd import _lib
    lib = _lib.load()
    one = _lib.C.c_void_p(64)                  # never dereferenced: every call below returns at its argument check
    conf = lambda kind, nc, B, H, W: lib.sfh_metrics_confusion(one, kind, one, nc, B, H, W, one, one, None)  # noqa: E731
    for args in ((4, 4, 1, 4, 4), (-1, 4, 1, 4, 4), (2, 1, 1, 4, 4), (2, 9, 1, 4, 4), (0, 4, 0, 4, 4), (0, 4, 1, 0, 4),
                 (0, 4, 1, 65536, 32768)):
        assert conf(*args) == -1, args
    assert lib.sfh_metrics_confusion(None, 0, one, 4, 1, 4, 4, one, one, None) == -1 and b"null" in lib.sfh_last_error()
    region = lambda mode, wc, hc, mx, my: lib.sfh_metrics_region(one, one, 1, mode, wc, hc, mx, my, one, None)  # noqa: E731
    for args in ((2, 8, 8, 0, 0), (0, 1, 8, 0, 0), (0, 8, 1, 0, 0), (0, 8, 8, -1, 0), (1, 1 << 20, 1 << 20, 0, 0),
                 (0, (1 << 20) + 1, 8, 0, 0), (1, 8, 8, (1 << 20) + 1, 0)):
        assert region(*args) == -1, args
    assert lib.sfh_metrics_region(one, one, 0, 0, 8, 8, 0, 0, one, None) == -1
    points = lambda n, gx, gy, pts=one: lib.sfh_metrics_points(one, one, 1, pts, n, gx, gy, 1.0, 1.0, 1.0, 1.0, one, None)  # noqa: E731
    for args in ((-1, 16, 9), (3, 0, 9), (3, 16, 4097), (3, 16, 9, None)):
        assert points(*args) == -1, args
    assert b"metrics_points" in lib.sfh_last_error()
