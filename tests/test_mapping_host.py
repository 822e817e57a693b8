"""CPU-side checks of the frame <-> court mapping (sfh_amd.mapping, csrc/mapping.hip): tests/mapping_ref.py against itself, the
argument checks of the C entries (they fire before anything touches a device), the host classes, and - only where OpenCV can
be imported - a pin of the point rule against cv2.perspectiveTransform."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mapping_ref as R
from sfh_amd import synth


# ------------------------------------------------------------------------------------------ the restatement against itself
def test_inverse_times_theta_is_the_identity():
    inv, det = R.inverse_theta_f64(synth.REALISTIC_THETAS)
    for t, m in zip(synth.REALISTIC_THETAS.astype(np.float64), inv):
        for prod in (t @ m, m @ t):
            assert np.abs(prod - np.eye(3)).max() <= 1e-12 * max(1.0, np.abs(prod).max())
    c2f, status = R.inverse_theta(synth.REALISTIC_THETAS)
    assert status.tolist() == [1, 1] and c2f.dtype == np.float32
    assert np.array_equal(c2f, inv.astype(np.float32))
    # the formula of tests/prep_ref.py:inverse_h33 without its final normalisation
    import prep_ref
    for t, m in zip(synth.REALISTIC_THETAS, inv):
        np.testing.assert_allclose((m / m[2, 2]).reshape(9), prep_ref.inverse_h33(t), rtol=1e-13)


def test_inverse_status_of_degenerate_matrices():
    eye = np.eye(3, dtype=np.float32)
    zero_row = eye.copy(); zero_row[2] = 0
    twin = eye.copy(); twin[0] = twin[1] = (1.0, 0.5, 0.25)
    nan = eye.copy(); nan[1, 1] = np.nan
    inf = eye.copy(); inf[0, 2] = np.inf
    c2f, status = R.inverse_theta(np.stack([eye, zero_row, twin, nan, inf]))
    assert status.tolist() == [1, 0, 0, 0, 0]
    assert np.array_equal(c2f[0], eye) and not c2f[1:].any()


def test_the_example_point_lands_inside_the_court():
    """utils/mapping_example.py:25: frame point (590, 418) of a 1280 x 720 frame under the first theta"""
    out, flag = R.map_points([[590, 418]], 0, synth.REALISTIC_THETAS, in_size=(1280, 720))
    assert flag.tolist() == [1] and out.dtype == np.float32
    assert 0.0 < out[0, 0] < 1.0 and 0.0 < out[0, 1] < 1.0
    px, _ = R.map_points([[590, 418]], 0, synth.REALISTIC_THETAS, in_size=(1280, 720), out_scale=(1280, 720))
    np.testing.assert_allclose(px, out * np.float32([1280, 720]), rtol=1e-6)


def test_court_poi_to_the_frame_and_back():
    poi = synth.load_court_poi("pitch")[0].numpy().astype(np.float64)
    inv, _ = R.inverse_theta_f64(synth.REALISTIC_THETAS)
    for t, m in zip(synth.REALISTIC_THETAS.astype(np.float64), inv):
        n = poi.shape[0]
        fu, fv, w1 = R.project_f64(poi[:, 0], poi[:, 1], np.tile(m.reshape(1, 9), (n, 1)))
        bu, bv, w2 = R.project_f64(fu, fv, np.tile(t.reshape(1, 9), (n, 1)))
        assert (w1 != 0).all() and (w2 != 0).all()
        assert np.abs(bu - poi[:, 0]).max() < 1e-9 and np.abs(bv - poi[:, 1]).max() < 1e-9


def test_point_rule_flags():
    th = np.stack([np.eye(3, dtype=np.float32), np.zeros((3, 3), dtype=np.float32)])
    out, flag = R.map_points([[0.5, -0.5]] * 4, [0, 1, 2, -1], th)
    assert flag.tolist() == [1, 0, 0, 0]                   # w' == 0 on the zero matrix, indices outside [0, F)
    assert out[0].tolist() == [0.75, 0.25] and not out[1:].any()
    out, flag = R.map_points([[np.nan, 0.0], [np.inf, 0.0]], 0, th)
    assert flag.tolist() == [0, 0] and not out.any()


def test_mosaic_integer_rule():
    s = np.array([[[0, 1, 255], [3, 4, 510]]], dtype=np.uint32)
    n = np.array([[0, 2]], dtype=np.uint32)
    assert R.mosaic_finish(s, n).tolist() == [[[0, 0, 0], [2, 2, 255]]]       # 0 where count == 0; 1.5 -> 2 (halves up)
    big = np.array([[[255 * 16843008] * 3]], dtype=np.uint64).astype(np.uint32)
    assert R.mosaic_finish(big, np.array([[16843008]], dtype=np.uint32)).tolist() == [[[255] * 3]]   # 2 * sum > 2^32


@pytest.mark.skipif(not __import__("importlib").util.find_spec("cv2"), reason="OpenCV is not installed: the point rule is pinned "
                    "against cv2.perspectiveTransform only where it can be imported")
def test_point_rule_against_opencv():
    import cv2
    g = np.random.default_rng(3)
    pts = g.uniform(-1, 1, (257, 2)).astype(np.float32)
    for t in synth.REALISTIC_THETAS:
        want = cv2.perspectiveTransform(pts[None], t.astype(np.float64))[0] / 2.0 + 0.5
        got, flag = R.map_points(pts, 0, t[None])
        assert flag.all()
        np.testing.assert_allclose(got, want, rtol=2.0 ** -22, atol=2.0 ** -22)       # cv2 rounds to fp32 before / 2 + 0.5


# ---------------------------------------------------------------------------------------------------- the C entries
def _lib():
    from sfh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import sfh_amd.build as b
        b.build(verbose=False)
    return _lib.load()


ONE = ctypes.c_void_p(0x1000)      # plausible non-null dummy: never dereferenced, every case fails an argument check


def _render(lib, **kw):
    a = dict(frames=ONE, batch=2, H=8, W=8, c2f=ONE, status=ONE, score=None, max_score=0.0, hc=8, wc=8, mode=0, top=ONE, valid=ONE)
    a.update(kw)
    return lib.sfh_topview_render(a["frames"], a["batch"], a["H"], a["W"], a["c2f"], a["status"], a["score"], a["max_score"],
                                  a["hc"], a["wc"], a["mode"], a["top"], a["valid"], None)


def _accum(lib, **kw):
    a = dict(frames=ONE, batch=2, H=8, W=8, c2f=ONE, status=ONE, score=None, max_score=0.0, hc=8, wc=8, sum=ONE, count=ONE)
    a.update(kw)
    return lib.sfh_topview_accumulate(a["frames"], a["batch"], a["H"], a["W"], a["c2f"], a["status"], a["score"], a["max_score"],
                                      a["hc"], a["wc"], a["sum"], a["count"], None)


def _points(lib, **kw):
    a = dict(points=ONE, index=ONE, frame0=0, n=4, thetas=ONE, F=2, in_w=0.0, in_h=0.0, sx=1.0, sy=1.0, out=ONE, flag=ONE)
    a.update(kw)
    return lib.sfh_map_points(a["points"], a["index"], a["frame0"], a["n"], a["thetas"], a["F"], a["in_w"], a["in_h"], a["sx"],
                              a["sy"], a["out"], a["flag"], None)


def test_mapping_entries_check_their_arguments_without_a_gpu():
    lib = _lib()
    err = lambda: lib.sfh_last_error().decode()
    assert lib.sfh_theta_invert(None, 2, ONE, ONE, None) == -1 and "theta_invert" in err() and "null" in err()
    assert lib.sfh_theta_invert(ONE, 2, ONE, None, None) == -1 and "null" in err()
    assert lib.sfh_theta_invert(ONE, 0, ONE, ONE, None) == -1 and "batch 0" in err()

    for fn, name in ((_render, "topview_render"), (_accum, "topview_accumulate")):
        assert fn(lib, frames=None) == -1 and name in err() and "null" in err()
        assert fn(lib, c2f=None) == -1 and "null" in err()
        assert fn(lib, status=None) == -1 and "null" in err()
        assert fn(lib, batch=0) == -1 and "batch 0" in err()
        assert fn(lib, batch=65536) == -1 and "batch 65536" in err()
        assert fn(lib, H=4096, W=4096) == -1 and "2^24" in err()                 # H * W < 2^24
        assert fn(lib, H=0) == -1 and "frame" in err()
        assert fn(lib, hc=1) == -1 and "court view" in err()
        assert fn(lib, wc=16385) == -1 and "court view" in err()
        assert fn(lib, score=ONE, max_score=float("nan")) == -1 and "NaN" in err()
    assert _render(lib, top=None) == -1 and "null" in err()
    assert _render(lib, valid=None) == -1 and "null" in err()
    assert _render(lib, mode=2) == -1 and "mode 2" in err()
    assert _accum(lib, sum=None) == -1 and "null" in err()
    assert _accum(lib, count=None) == -1 and "null" in err()

    assert lib.sfh_topview_finish(None, ONE, 8, 8, ONE, None) == -1 and "topview_finish" in err() and "null" in err()
    assert lib.sfh_topview_finish(ONE, ONE, 0, 8, ONE, None) == -1 and "court view" in err()

    assert _points(lib, points=None) == -1 and "map_points" in err() and "null" in err()
    assert _points(lib, thetas=None) == -1 and "null" in err()
    assert _points(lib, flag=None) == -1 and "null" in err()
    assert _points(lib, n=0) == -1 and "0 points" in err()
    assert _points(lib, F=0) == -1 and "0 frames" in err()
    assert _points(lib, in_w=1280.0, in_h=0.0) == -1 and "in_size" in err()
    assert _points(lib, in_w=-1.0, in_h=720.0) == -1 and "in_size" in err()
    assert _points(lib, sx=float("inf")) == -1 and "out_scale" in err()


# ---------------------------------------------------------------------------------------------------- the host classes
def test_court_sizes():
    from sfh_amd.mapping import CourtSizes as CS, UNITS
    assert CS.COURT_IN_PIXELS == (1280, 720) and CS.FRAME_IN_PIXELS == (1280, 720)
    assert CS.COURT_IN_METERS == (32.2326, 17.145) and CS.METERS2FEET == 3.28084
    assert CS.METERS2PIXELS == (1280 / 32.2326, 720 / 17.145)
    assert CS.PIXELS2METERS == (32.2326 / 1280, 17.145 / 720)
    assert UNITS["norm"] == (1.0, 1.0) and UNITS["pixels"] == (1280.0, 720.0) and UNITS["meters"] == CS.COURT_IN_METERS
    assert UNITS["feet"] == (32.2326 * 3.28084, 17.145 * 3.28084)


def test_court_mapping_round_trips_a_court_json(tmp_path):
    from sfh_amd import mapping as M
    from sfh_amd import outputs as O
    g = np.random.default_rng(11)
    thetas = (np.eye(3) + g.normal(0, 0.2, (5, 1, 3, 3))).astype(np.float32)
    thetas[:2, 0] = synth.REALISTIC_THETAS
    scores = [0.012345, 0.5, 1.25, 0.0, 3.0]
    names = [f"{k:06d}" for k in (7, 8, 9, 12, 13)]
    with O.CourtJsonWriter(str(tmp_path), "game", "model-x") as w:
        for n, s, t in zip(names, scores, thetas):
            w.add(n, score=s, theta=t)
    cm = M.CourtMapping(os.path.join(str(tmp_path), "game_court.json"))
    assert cm.model == "model-x" and len(cm) == 5 and cm.names == names
    assert cm.theta.dtype == np.float32 and np.array_equal(cm.theta, thetas.reshape(5, 3, 3))        # bit for bit
    assert np.array_equal(cm.scores, np.float32([O.format_score(s) for s in scores]))
    assert cm.rows == {n: k for k, n in enumerate(names)} and cm.row("000012") == 3
    # from tensors: the same host state
    cm2 = M.CourtMapping(torch.from_numpy(thetas), scores=torch.tensor(scores), names=names)
    assert np.array_equal(cm2.theta, cm.theta) and cm2.rows == cm.rows
    assert M.CourtMapping(thetas).names == ["0", "1", "2", "3", "4"]
    with pytest.raises(ValueError, match="scores"):
        M.CourtMapping(thetas, scores=[1.0])
    with pytest.raises(ValueError, match="unique"):
        M.CourtMapping(thetas, names=["a"] * 5)
    with pytest.raises(ValueError, match="theta"):
        M.CourtMapping(np.zeros((2, 4)))


def test_cpu_tensors_are_refused():
    from sfh_amd import mapping as M
    fr = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    th = torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.TopViewRenderer((16, 8))(fr, th)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.CourtMosaic((16, 8)).add(fr, th)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.CourtMosaic((16, 8)).result()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.invert_theta(th)
    cm = M.CourtMapping(th.numpy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.tables("cpu")
    mapper = M.FrameCourtMapper(cm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mapper.frame_to_court(torch.zeros((3, 2)), 0, (1280, 720))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mapper.court_to_frame(torch.zeros((3, 2)), 0)
    with pytest.raises(ValueError, match="units"):
        mapper.frame_to_court(torch.zeros((3, 2)), 0, units="yards")
    with pytest.raises(ValueError, match="mode"):
        M.TopViewRenderer(mode="cubic")
    with pytest.raises(ValueError, match="out_size"):
        M.TopViewRenderer(out_size=(1, 720))


def test_module_is_exported():
    import sfh_amd
    assert sfh_amd.mapping.TopViewRenderer is not None and hasattr(sfh_amd.mapping, "rectify_game")
