"""Host-side checks of sfh_amd.preparation (no GPU): argument validation of the three library entries, the host rules
(uv_tables, rescale_theta, preprocess_weight) against their restatements in tests/prep_ref.py, the fixtures the GPU tests
stand on, and prepare_dataset's file layout with the device replaced by the restatement."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import prep_fixtures as F
import prep_ref as R
from sfh_amd import _lib
from sfh_amd import outputs as O
from sfh_amd import preparation as P


def _err(lib):
    return lib.sfh_last_error().decode()


def test_argument_validation_without_gpu():
    lib = _lib.load()
    x = ctypes.c_void_p(256)      # never dereferenced: every call below is refused before a launch
    fit = lambda *a: lib.sfh_prep_fit(*a)
    assert fit(None, x, None, 2, 33, 1.0, 1.0, 10, x, x, x, x, x, x, x, None) == -1 and "null" in _err(lib)
    assert fit(x, x, None, 2, 33, 1.0, 1.0, 10, x, x, None, x, x, x, None, None) == -1 and "null" in _err(lib)
    assert fit(x, x, None, 0, 33, 1.0, 1.0, 10, x, x, x, x, x, x, x, None) == -1 and "batch" in _err(lib)
    assert fit(x, x, None, 2, 0, 1.0, 1.0, 10, x, x, x, x, x, x, x, None) == -1 and "points" in _err(lib)
    assert fit(x, x, None, 2, 257, 1.0, 1.0, 10, x, x, x, x, x, x, x, None) == -1
    assert fit(x, x, None, 2, 33, 0.0, 1.0, 10, x, x, x, x, x, x, x, None) == -1 and "norm_size" in _err(lib)
    assert fit(x, x, None, 2, 33, 1.0, 1.0, -1, x, x, x, x, x, x, x, None) == -1 and "refine" in _err(lib)
    ren = lambda *a: lib.sfh_prep_render(*a)
    assert ren(None, x, 360, 640, None, None, 2, 360, 640, 0, x, None, None) == -1 and "null" in _err(lib)
    assert ren(x, x, 360, 640, None, None, 2, 360, 640, 0, None, None, None) == -1
    assert ren(x, x, 360, 640, None, None, 0, 360, 640, 0, x, None, None) == -1 and "geometry" in _err(lib)
    assert ren(x, x, 0, 640, None, None, 2, 360, 640, 0, x, None, None) == -1
    assert ren(x, x, 360, 640, None, None, 2, 360, 640, 1, x, x, None) == -1 and "uv requested" in _err(lib)   # no tables
    assert ren(x, x, 360, 640, x, x, 2, 360, 640, 1, x, None, None) == -1 and "uv requested" in _err(lib)      # no output
    assert ren(x, x, 360, 640, None, None, 2, 360, 642, 0, x, None, None) == -1 and "multiple of 4" in _err(lib)
    rgb = lambda *a: lib.sfh_prep_rgb_to_ids(*a)
    assert rgb(None, 16, 4, x, None) == -1 and "null" in _err(lib)
    assert rgb(x, 0, 4, x, None) == -1 and "pixels" in _err(lib)
    assert rgb(x, 16, 5, x, None) == -1 and "5 classes" in _err(lib)
    with pytest.raises(ValueError):
        _lib.check(-1, "prep")


def test_module_argument_checks():
    ids, poi = F.court_ids(), F.court_poi()
    with pytest.raises(NotImplementedError):
        P.LabelMaker(ids, poi, (640, 360), 5)
    with pytest.raises(ValueError, match="multiple of 4"):
        P.LabelMaker(ids, poi, (642, 360), 4)
    with pytest.raises(ValueError, match="ignore_pts"):
        P.LabelMaker(ids, poi, (640, 360), 4, ignore_pts=[40])
    with pytest.raises(ValueError, match="court_ids"):
        P.LabelMaker(ids.astype(np.float32), poi, (640, 360), 4)
    lm = P.LabelMaker(ids, poi, (640, 360), 4, ignore_pts=P.FOOTBALL_PITCH_IGNORE_POINTS, device="cpu")
    assert lm.ignore.sum() == 5 and tuple(P.FOOTBALL_PITCH_IGNORE_POINTS) == (12, 13, 16, 19, 20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.make(np.zeros((1, 33, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.rgb_to_ids(torch.zeros((2, 2, 3), dtype=torch.uint8), 4)


@pytest.mark.parametrize("size", [(640, 360), (1280, 720)])
@pytest.mark.parametrize("offsets", [((0, 0), (0, 0)), ((30, 17), (9, 22))])
def test_uv_tables_equal_generate_uv_template(size, offsets):
    xo, yo = offsets
    u_tab, v_tab = P.uv_tables(size, xo, yo)
    u, v = R.generate_uv_template(size, xo, yo)
    W, H = size
    assert u_tab.dtype == np.uint16 and v_tab.dtype == np.uint16 and u_tab.shape == (W,) and v_tab.shape == (H,)
    uq = np.rint(u.astype(np.float64) * 65535).astype(np.uint16)
    vq = np.rint(v.astype(np.float64) * 65535).astype(np.uint16)
    # the template is the outer composition of the two tables inside the window and zero outside it
    in_x, in_y = u_tab != 0, v_tab != 0
    assert np.array_equal(uq, np.where(in_y[:, None], u_tab[None, :], 0))
    assert np.array_equal(vq, np.where(in_x[None, :], v_tab[:, None], 0))
    assert in_x.sum() == W - xo[0] - xo[1] - 1 and in_y.sum() == H - yo[0] - yo[1] - 1
    # preprocess_uv_mask's / 65535 returns the template value to within half a step
    back = (u_tab / 65535.0).astype(np.float32)
    assert np.abs(back - u[yo[0]]).max() <= 0.5 / 65535 + 1e-7


def test_rescale_theta_and_weight_match_their_restatements():
    g = np.random.default_rng(2)
    for th in F.fixture_thetas():
        got, want = P.rescale_theta((1280, 720), (640, 360), th), R.rescale_theta((1280, 720), (640, 360), th)
        assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps * np.abs(want).max()
    mse = np.concatenate([[0.0, 0.005, 0.01, 1.0], g.random(64) * 0.03])
    got, want = P.preprocess_weight(mse), R.preprocess_weight(mse)
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= np.finfo(np.float32).eps
    assert got[0] > 0.99 and got[2] < 0.01 and np.all(np.diff(P.preprocess_weight(np.linspace(0, 0.02, 50))) <= 0)


def test_fixtures_are_usable_and_counted():
    """every fixture theta leaves at least 4 template points inside the frame; the status-0 share of a fixture is exactly
    the number of frames built with 3 points"""
    for name in ("pitch", "ncaa"):
        court = F.court_poi(name)
        th = F.fixture_thetas()
        for k, t in enumerate(th):
            assert int(F.inside(F.project(t, court)).sum()) >= 4, (name, k)
        manual, n_short = F.exact_annotations(court, th, seed=3, n_short=2)
        ref = R.fit_batch(court, manual, refine=0)
        assert int((ref["status"] == 0).sum()) == n_short == 2
        assert np.array_equal(ref["status"][-2:], [0, 0]) and not ref["theta"][-2:].any()


def test_restatement_recovers_a_known_theta():
    court = F.court_poi("pitch")
    th = F.fixture_thetas()
    manual, n_short = F.exact_annotations(court, th, seed=5, n_short=1)
    wh = np.array([1280.0, 720.0])
    for refine in (0, 10):
        ref = R.fit_batch(court, manual, ignore_pts=P.FOOTBALL_PITCH_IGNORE_POINTS, refine=refine)
        for b in range(th.shape[0] - n_short):
            want = F.project(th[b], court) * wh
            got = F.project_c2f(ref["theta_c2f"][b], court) * wh
            # the eigenvector of L^T L moves by about eps * lambda_max / (lambda_2 - lambda_1) under rounding of size
            # eps * lambda_max; 64: the 45 accumulated entries and the two changes of coordinates; in pixels at 1280x720
            eig = np.sort(ref["eig"][b])
            bound = 64 * np.finfo(np.float64).eps * (eig[-1] / eig[1]) * np.abs(want).max()
            assert np.abs(got - want).max() <= bound, (refine, b, np.abs(got - want).max(), bound)
            prod = ref["theta"][b] @ ref["theta_c2f"][b]
            assert np.abs(prod / prod[2, 2] - np.eye(3)).max() < 1e-9
            flags = ref["poi"][b, :, 2]
            assert not flags[list(P.FOOTBALL_PITCH_IGNORE_POINTS)].any()
            assert ref["num_nonzero"][b] == int(flags.sum())
            # the poi carry Kornia's 1e-8 in the divisor: a point moves by 1e-8 of its coordinate (below 3 frame widths here)
            assert ref["reproj_mse"][b] < 3e-8
    # noisy clicks: the polish never raises the cost of the DLT start
    noisy, _ = F.exact_annotations(court, th, seed=6, n_short=0, noise_px=2.0)
    for b in range(th.shape[0]):
        use = R.usable_points(noisy[b])
        dst = noisy[b] * 2 - 1
        h0, _ = R.dlt(court, dst, use)
        h1 = R.refine_gn(h0, court, dst, use, 10)
        assert R.forward_cost(h1, court, dst, use) <= R.forward_cost(h0, court, dst, use)


def test_rgb_rule_inverts_the_palette():
    for nc in (4, 7, 8):
        pal = O._palette_bytes(nc)
        ids = np.random.default_rng(nc).integers(0, nc, (5, 7), dtype=np.uint8)
        assert np.array_equal(R.rgb_to_ids(pal[ids], nc), ids)
        for k in range(1, nc):
            assert tuple(pal[k]) == R.PALETTE[k]


def test_prepare_dataset_layout_with_the_restatement(tmp_path):
    court, ids = F.court_poi("pitch"), F.court_ids("pitch_v3_nc4_640x360")
    th = F.fixture_thetas()[:5]
    manual, n_short = F.exact_annotations(court, th, seed=8, n_short=1)
    anno = tmp_path / "anno"
    games = {"game_a": [0, 1, 2], "game_b": [3, 4]}
    for game, rows in games.items():
        os.makedirs(anno / game)
        with open(anno / game / "manual_anno.json", "w") as f:
            json.dump({f"{r:06d}": {"poi": manual[r].tolist(), "theta": None} for r in rows}, f)
    (anno / "stray.txt").write_text("not a game")
    size = (64, 36)
    tables = P.uv_tables((ids.shape[1], ids.shape[0]))
    for uv in (False, True):
        dst = tmp_path / ("out_uv" if uv else "out")
        maker = R.RefMaker(ids, court, size, uv=uv, tables=tables)
        rep = P.prepare_dataset(str(anno), str(dst), size=size, batch=2, maker=maker)
        assert rep["skipped"] == ["game_b/000004"] and len(rep["skipped"]) == n_short
        assert rep["written"] == ["game_a/000000", "game_a/000001", "game_a/000002", "game_b/000003"]
        assert sorted(os.listdir(dst)) == ["game_a", "game_b"]
        exts = [".json", ".npy", ".png"] if uv else [".json", ".png"]
        assert sorted(os.listdir(dst / "game_b")) == ["000003" + e for e in exts]
        whole = maker.make(manual)
        for key in rep["written"]:
            r = int(key.split("/")[1])
            with open(dst / (key + ".json")) as f:
                a = json.load(f)
            assert sorted(a) == ["poi", "reproj_mse", "theta"]
            assert np.array_equal(np.asarray(a["theta"]), whole["theta"][r])          # fp64 survives the json trip
            assert np.array_equal(np.asarray(a["poi"]), whole["poi"][r]) and a["reproj_mse"] == whole["reproj_mse"][r]
            png = O.decode_png(np.fromfile(dst / (key + ".png"), dtype=np.uint8))
            assert np.array_equal(png, whole["mask"][r]) and png.any()
            if uv:
                assert np.array_equal(np.load(dst / (key + ".npy")), whole["uv"][r])
        # the reader gives what to_batch gives for the same frames
        labels = {k: torch.from_numpy(np.asarray(v)) for k, v in whole.items()}
        batch, dropped = P.to_batch(labels, names=[f"{g}/{r:06d}" for g, rows in games.items() for r in rows])
        assert dropped == rep["skipped"] and batch["name"] == rep["written"]
        back = P.read_dataset(str(dst), rep["written"], use_uv=uv)
        assert sorted(back) == sorted(batch)
        for k in batch:
            if k == "name":
                continue
            assert back[k].dtype == batch[k].dtype and torch.equal(back[k], batch[k]), k
        assert batch["mask"].dtype == torch.int64 and batch["weight"].shape == (4, 1)
        if uv:
            assert batch["uv"].dtype == torch.float32 and tuple(batch["uv"].shape) == (4, 2, 36, 64)
