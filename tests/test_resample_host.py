"""CPU-side checks of the Pillow-exact resize (sfh_amd.resample, csrc/resample.hip): the numpy restatement
tests/resample_ref.py is pinned to the installed Pillow byte for byte, the C table functions to the restatement, and the
refusals fire without a device.  Every comparison is byte equality."""
import ctypes

import numpy as np
import pytest
from PIL import Image

import resample_cases as RC
import resample_ref as R

PIL_FILTERS = {R.BOX: Image.BOX, R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC}
CASES = RC.host_cases()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    from sfh_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_pillow(name):
    img, (hd, wd) = CASES[name]
    pil = Image.fromarray(img)
    assert pil.mode == ("L" if img.ndim == 2 else "RGB")
    for filt, pf in PIL_FILTERS.items():
        want = np.asarray(pil.resize((wd, hd), pf))
        got = R.resize(img, (wd, hd), filt)
        assert got.shape == want.shape and np.array_equal(got, want), (name, filt, int((got != want).sum()))
    # Image.resize(size) without a filter is BICUBIC
    assert np.array_equal(np.asarray(pil.resize((wd, hd))), R.resize(img, (wd, hd), R.BICUBIC)), name


def test_checker_overshoots():
    """the checker reaches both clamps, so a missing clamp or a logical shift cannot pass"""
    bounds, coef, _ = R.coeffs(64, 100, R.BICUBIC)
    row = RC.checker()[0].astype(np.int64)
    acc = [(1 << 21) + sum(int(row[lo + t]) * int(coef[x, t]) for t in range(n)) for x, (lo, n) in enumerate(bounds)]
    assert min(acc) < 0 and max(acc) >> 22 > 255


def test_c_tables_equal_the_restatement(lib):
    for insize, outsize in RC.axis_pairs():
        for filt in (R.BOX, R.BILINEAR, R.BICUBIC):
            bounds, coef, ksize = R.coeffs(insize, outsize, filt)
            gb = np.full((outsize, 2), -7, np.int32)
            gk = np.full((outsize, ksize), -7, np.int32)
            assert lib.sfh_resample_tab(insize, outsize, filt, _vp(gb), _vp(gk), gk.size) == ksize, (insize, outsize, filt)
            assert np.array_equal(gb, bounds) and np.array_equal(gk, coef), (insize, outsize, filt)
            # one element short: refused
            assert lib.sfh_resample_tab(insize, outsize, filt, _vp(gb), _vp(gk), gk.size - 1) == -1


def test_c_table_refusals(lib):
    b, k = np.zeros((8, 2), np.int32), np.zeros((8, 64), np.int32)
    assert lib.sfh_resample_tab(16, 8, R.BICUBIC, _vp(b), _vp(k), k.size) == 9
    assert lib.sfh_resample_tab(0, 8, R.BICUBIC, _vp(b), _vp(k), k.size) == -1
    assert lib.sfh_resample_tab(16, 0, R.BICUBIC, _vp(b), _vp(k), k.size) == -1
    assert lib.sfh_resample_tab(-3, 8, R.BICUBIC, _vp(b), _vp(k), k.size) == -1
    assert lib.sfh_resample_tab(16, 8, 1, _vp(b), _vp(k), k.size) == -1           # LANCZOS
    assert lib.sfh_resample_tab(16, 8, 5, _vp(b), _vp(k), k.size) == -1           # HAMMING
    assert lib.sfh_resample_tab(16, 8, R.BICUBIC, None, _vp(k), k.size) == -1
    assert lib.sfh_resample_tab(16, 8, R.BICUBIC, _vp(b), None, k.size) == -1
    idx = np.zeros(8, np.int32)
    assert lib.sfh_nearest_tab(16, 8, R.NEAREST_PIL, _vp(idx), 8) == 8
    assert lib.sfh_nearest_tab(16, 8, R.NEAREST_PIL, _vp(idx), 7) == -1
    assert lib.sfh_nearest_tab(0, 8, R.NEAREST_PIL, _vp(idx), 8) == -1
    assert lib.sfh_nearest_tab(16, 0, R.NEAREST_CV2, _vp(idx), 8) == -1
    assert lib.sfh_nearest_tab(16, 8, 2, _vp(idx), 8) == -1
    assert lib.sfh_nearest_tab(16, 8, R.NEAREST_CV2, None, 8) == -1


def test_tap_bound_and_tile_rows(lib):
    from sfh_amd import resample as RS
    T = lib.sfh_resample_max_taps()
    assert T == RS.MAX_TAPS and T >= 23
    assert int(R.coeffs(3421, 640, R.BICUBIC)[0][:, 1].max()) <= 23 <= T          # the NCAA template's width
    # an integer bicubic downscale by s has exactly 4 s taps
    s = T // 4
    assert int(R.coeffs(s * 11, 11, R.BICUBIC)[0][:, 1].max()) == 4 * s
    assert lib.sfh_resample_tile_rows(s * 11, 11, R.BICUBIC) >= 1
    win = over_bound_size(T)
    assert lib.sfh_resample_tile_rows(win, 11, R.BICUBIC) == -1
    assert lib.sfh_resample_tile_rows(720, 360, R.BICUBIC) == 16
    assert lib.sfh_resample_tile_rows(0, 360, R.BICUBIC) == -1 and lib.sfh_resample_tile_rows(720, 360, 1) == -1
    # every tile of the chosen height reaches at most SFH_RESAMPLE_MAX_ROWS source rows
    for insize, outsize in ((1080, 360), (720, 361), (360, 720), (2000, 360), (24 * 40, 40)):
        for filt in (R.BOX, R.BILINEAR, R.BICUBIC):
            th = lib.sfh_resample_tile_rows(insize, outsize, filt)
            b = R.coeffs(insize, outsize, filt)[0]
            if int(b[:, 1].max()) > T:
                assert th == -1
                continue
            assert th in (1, 2, 4, 8, 16)
            for y0 in range(0, outsize, th):
                t = b[y0:y0 + th]
                assert int((t[:, 0] + t[:, 1]).max() - t[:, 0].min()) <= 64


def over_bound_size(T, out=11):
    """the smallest source size whose bicubic table for `out` outputs has an index with T + 1 taps or more"""
    size = T // 4 * out
    while int(R.coeffs(size, out, R.BICUBIC)[0][:, 1].max()) <= T:
        size += 1
    return size


def test_nearest_pil_rule_equals_pillow(lib):
    pairs = RC.nearest_pairs()
    assert len(pairs) >= 306
    for insize, outsize in pairs:
        idx = np.zeros(outsize, np.int32)
        assert lib.sfh_nearest_tab(insize, outsize, R.NEAREST_PIL, _vp(idx), outsize) == outsize
        assert np.array_equal(idx, R.nearest_index(insize, outsize, R.NEAREST_PIL)), (insize, outsize)
        line = (np.arange(insize, dtype=np.int64) * 2654435761 >> 7).astype(np.uint8)       # neighbours differ
        # horizontally: a 2-row image; vertically: a 2-column image
        want = np.asarray(Image.fromarray(np.stack([line, line])).resize((outsize, 2), Image.NEAREST))
        assert np.array_equal(np.stack([line[idx], line[idx]]), want), ("x", insize, outsize)
        want = np.asarray(Image.fromarray(np.stack([line, line], axis=1)).resize((2, outsize), Image.NEAREST))
        assert np.array_equal(np.stack([line[idx], line[idx]], axis=1), want), ("y", insize, outsize)
    # the closed form is not Pillow's rule: with it this test could not pass
    line = (np.arange(1000, dtype=np.int64) * 2654435761 >> 7).astype(np.uint8)
    want = np.asarray(Image.fromarray(np.stack([line, line])).resize((999, 2), Image.NEAREST))[0]
    assert not np.array_equal(line[R.nearest_index_closed_form(1000, 999)], want)
    assert not np.array_equal(R.nearest_index_closed_form(1000, 999), R.nearest_index(1000, 999))


def test_nearest_images_equal_pillow():
    for k, (src, dst) in enumerate(RC.NEAREST_IMAGE_PAIRS):
        for shape in (src, src + (3,)):
            img = RC.noise(shape, 200 + k)
            want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.NEAREST))
            assert np.array_equal(R.resize_nearest(img, (dst[1], dst[0]), R.NEAREST_PIL), want), (src, dst)


def test_nearest_cv2_rule_equals_the_oracle(lib):
    from oracle import post_ref
    for insize, outsize in RC.nearest_pairs(60):
        idx = np.zeros(outsize, np.int32)
        assert lib.sfh_nearest_tab(insize, outsize, R.NEAREST_CV2, _vp(idx), outsize) == outsize
        assert np.array_equal(idx, R.nearest_index(insize, outsize, R.NEAREST_CV2))
        src = np.arange(insize, dtype=np.int64)
        assert np.array_equal(post_ref.resize_nearest(src[None, :], (outsize, 1))[0], idx), (insize, outsize)
        assert np.array_equal(post_ref.resize_nearest(src[:, None], (1, outsize))[:, 0], idx), (insize, outsize)


def test_python_tables_and_refusals_without_a_device():
    import torch
    from sfh_amd import ops, preparation, resample as RS
    from sfh_amd.pipeline import FramePipeline
    b, k, ks = RS.axis_table(1280, 640, "bicubic")
    rb, rk, rks = R.coeffs(1280, 640, R.BICUBIC)
    assert ks == rks and np.array_equal(b, rb) and np.array_equal(k, rk)
    assert np.array_equal(RS.nearest_table(1000, 999, "pil"), R.nearest_index(1000, 999))
    with pytest.raises(ValueError):
        RS.axis_table(1280, 640, "lanczos")
    with pytest.raises(ValueError):
        RS.axis_table(0, 640)
    with pytest.raises(ValueError):
        RS.nearest_table(10, 5, "torch")
    with pytest.raises(ValueError):
        RS.Resampler((720, 1280), (360, 640), channels=4)
    with pytest.raises(ValueError):
        RS.Resampler((720, 1280), (360, 0))
    with pytest.raises(ValueError):
        RS.Resampler((720, 1280), (360, 640), filter="hamming")
    with pytest.raises(NotImplementedError, match=str(RS.MAX_TAPS)):
        RS.Resampler((8, over_bound_size(RS.MAX_TAPS)), (8, 11))
    with pytest.raises(NotImplementedError, match=str(RS.MAX_TAPS)):
        RS.Resampler((over_bound_size(RS.MAX_TAPS), 8), (11, 8))
    r = RS.Resampler((8, 12), (4, 6))
    with pytest.raises(ValueError):
        r.resize(torch.zeros((1, 8, 12, 3), dtype=torch.uint8))              # a CPU tensor
    with pytest.raises(ValueError):
        r.to_input(torch.zeros((1, 8, 12, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        r.both(np.zeros((1, 8, 12, 3), np.uint8))
    with pytest.raises(ValueError):
        RS.resize_nearest(torch.zeros((1, 8, 12), dtype=torch.uint8), (4, 6))    # a CPU tensor
    with pytest.raises(ValueError):
        RS.resize_nearest(torch.zeros((1, 8, 12), dtype=torch.int32), (4, 6))
    with pytest.raises(ValueError):
        RS.resize_nearest(torch.zeros((1, 8, 12), dtype=torch.uint8), (4, 6), rule="nearest")
    with pytest.raises(ValueError):
        RS.pil_resize_device(torch.zeros((8, 12), dtype=torch.uint8), (6, 4))
    with pytest.raises(ValueError):
        ops.frames_u8_to_input(torch.zeros((1, 8, 12, 3), dtype=torch.uint8), (6, 4), resize="pil")
    with pytest.raises(ValueError):
        ops.frames_u8_to_input(torch.zeros((1, 8, 12, 3), dtype=torch.uint8), (6, 4), resize="cubic")
    with pytest.raises(ValueError):
        preparation.to_batch({}, frame_resize="area")
    with pytest.raises(ValueError):
        FramePipeline(None, 1, (8, 12), resize="lanczos")


def test_c_entry_points_refuse_without_a_device(lib):
    one = ctypes.c_void_p(64)       # never dereferenced: every refusal below fires before anything touches a device
    T = lib.sfh_resample_max_taps()
    ok = dict(batch=1, C=3, Hs=8, Ws=12, Hd=4, Wd=6)

    def call(src=one, u8=one, f32=None, xb=one, xk=one, xs=9, xt=8, yb=one, yk=one, ys=9, yt=8, rows=16, **kw):
        g = dict(ok, **kw)
        return lib.sfh_resample_u8(src, u8, f32, g["batch"], g["C"], g["Hs"], g["Ws"], g["Hd"], g["Wd"], xb, xk, xs, xt, yb, yk, ys, yt,
                                   rows, None)
    assert call(src=None) == -1
    assert call(u8=None, f32=None) == -1 and b"destination" in lib.sfh_last_error()
    assert call(C=2) == -1 and call(C=4) == -1
    assert call(batch=0) == -1 and call(Hs=0) == -1 and call(Wd=0) == -1 and call(Hd=-1) == -1
    assert call(xb=None) == -1 and call(xk=None) == -1 and call(yb=None) == -1 and call(yk=None) == -1
    assert call(xt=T + 1) == -1 and str(T).encode() in lib.sfh_last_error()
    assert call(yt=T + 1) == -1 and str(T).encode() in lib.sfh_last_error()
    assert call(rows=3) == -1 and call(rows=32) == -1 and call(rows=0) == -1
    g = lambda **kw: lib.sfh_resize_gather(kw.get("src", one), kw.get("dst", one), kw.get("batch", 1), kw.get("C", 3), kw.get("eb", 1),
                                           kw.get("Hs", 8), 12, kw.get("Hd", 4), 6, kw.get("yi", one), kw.get("xi", one), None)
    assert g(src=None) == -1 and g(dst=None) == -1 and g(yi=None) == -1 and g(xi=None) == -1
    assert g(C=2) == -1 and g(C=1, eb=2) == -1 and g(eb=4) == -1 and g(batch=0) == -1 and g(Hs=0) == -1 and g(Hd=70000) == -1
