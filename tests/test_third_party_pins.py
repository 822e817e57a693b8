"""Conditional pins for the third-party legs of the hot path (VERDICT r05 missing #4 / next #3).

The reference gets its warp / point arithmetic from Kornia (models/reconstructor.py:100-130) and its resizes / PNG
stream from OpenCV (utils/dataset.py:310-330, predict.py:26-37, utils/postprocess.py).  Neither package is in this image
(ordinary ModuleNotFoundError), so `oracle/warp_ref.py` and `oracle/post_ref.py` restate the published
algorithms and the goldens under tests/golden/ carry the "Kornia leg unpinned" caveat.  The tests below are skipped here
and ACTIVATE on any box where the packages import: they pin the restatements (and through them the HIP kernels, which
tests/test_gpu_parity.py::test_warp_vs_oracle holds bit-exact to the restatement) against the real thing - a Kornia
release with another `eps` rule or another `align_corners` default in its warper would fail them instead of passing
unnoticed.  CPU only; nothing here touches the GPU or /root/reference."""
import os

import numpy as np
import pytest
import torch

from oracle import golden, post_ref, warp_ref
from sfh_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIE_ULPS = 4        # the tie band tests/test_oracle.py::test_warp_grid_matmul_vs_pinned_order_ties defines


def _pin_thetas():
    """identity, the two trained-model matrices of utils/mapping_example.py:12-22,48-58, the C2 / C5 golden thetas,
    a near-singular one (Z crosses zero inside the frame) and one that maps the whole frame out of bounds"""
    t = [np.eye(3, dtype=np.float32)] + [m for m in synth.REALISTIC_THETAS]
    for f in ("c2_640x360_b16.npz", "c5_1280x720_b16.npz"):
        g = golden.load(os.path.join(GOLDEN, f))
        t += [m for m in g["theta"].reshape(-1, 3, 3)[:4]]
    sing = np.eye(3, dtype=np.float32)
    sing[2] = (0.9, 0.4, 1e-3)                     # Z = 0.9 x + 0.4 y + 0.001: zero along a line through the frame
    far = np.eye(3, dtype=np.float32)
    far[0, 2] = 5.0
    tiny = np.eye(3, dtype=np.float32)
    tiny[2] = (0.0, 0.0, 5e-9)                     # |Z| < 1e-8 everywhere: the "scale = 1" branch of Kornia's rule
    return torch.from_numpy(np.stack(t + [sing, far, tiny])).reshape(-1, 1, 3, 3)


def _templates(B, wh):
    w, h = wh
    name = "ncaa_nc4_640x360" if (w, h) == (640, 360) else "pitch_v3_nc4_1280x720"
    return synth.load_court_template(name, 4, B)


def _near_tie(theta, h, w, ht, wt):
    """pixels whose unnormalised template coordinate is within TIE_ULPS ulp of a rounding tie (x or y), or not finite"""
    grid = warp_ref.warp_grid(theta, h, w)
    band = torch.zeros(grid.shape[:-1], dtype=torch.bool)
    for k, size in ((0, wt), (1, ht)):
        p = warp_ref.unnormalize(grid[..., k], size)
        ulp = torch.finfo(torch.float32).eps * p.abs().clamp(min=1.0)
        band |= ((p - torch.floor(p) - 0.5).abs() <= TIE_ULPS * ulp) | ~torch.isfinite(p)
    return band


# ------------------------------------------------------------------------------------------ Kornia
@pytest.mark.parametrize("wh", [(640, 360), (1280, 720)])
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_kornia_homography_warper_vs_restatement(mode, wh):
    """models/reconstructor.py:100-118: HomographyWarper(h, w[, mode='nearest'], normalized_coordinates=True)(template,
    theta).squeeze(1) against oracle/warp_ref.homography_warp - nearest EQUAL outside the 4-ulp tie band, bilinear to
    fp32 rounding."""
    kornia = pytest.importorskip("kornia")
    w, h = wh
    theta = _pin_thetas()
    B = theta.shape[0]
    tmpl = _templates(B, wh)
    if mode == "nearest":
        warper = kornia.geometry.transform.HomographyWarper(h, w, mode="nearest", normalized_coordinates=True)
    else:
        warper = kornia.geometry.transform.HomographyWarper(h, w, normalized_coordinates=True)
    with torch.no_grad():
        want = warper(tmpl, theta).squeeze(1)
    got = warp_ref.homography_warp(theta, tmpl, h, w, mode)
    assert tuple(want.shape) == tuple(got.shape) == (B, h, w)
    if mode == "nearest":
        band = _near_tie(theta, h, w, h, w)
        assert torch.equal(got[~band], want[~band]), int((got != want)[~band].sum())
        assert float(band.float().mean()) < 5e-3       # (the identity's border pixels sit exactly on ties: x = +-1)
        # predict-mode epilogue (models/reconstructor.py:223,240): * mask_classes -> int32 gives whole class ids
        assert torch.equal((want * 4).to(torch.int32).float(), want * 4)
    else:
        sing = B - 3                                    # the near-singular matrix: compare away from its pole only
        ok = torch.ones(B, dtype=torch.bool)
        ok[sing] = False
        assert float((got[ok] - want[ok]).abs().max()) < 2e-5
        z = (theta[sing, 0, 2, 0] * warp_ref.normalized_axis(w)[None, :] + theta[sing, 0, 2, 1] * warp_ref.normalized_axis(h)[:, None]
             + theta[sing, 0, 2, 2])
        away = z.abs() > 1e-2
        assert float((got[sing][away] - want[sing][away]).abs().max()) < 1e-3


def test_kornia_transform_points_vs_restatement():
    """models/reconstructor.py:120-130: transform_points(inverse(theta), court_poi) / 2 + 0.5"""
    pytest.importorskip("kornia")
    from kornia.geometry.linalg import transform_points
    theta = _pin_thetas()[:-3]                           # invertible ones
    B = theta.shape[0]
    poi = synth.load_court_poi("pitch", B)
    inv = torch.inverse(theta)
    want = transform_points(inv, poi) / 2.0 + 0.5
    got = warp_ref.transform_points(inv, poi) / 2.0 + 0.5
    assert float((got - want).abs().max()) < 1e-6
    # the degenerate rule: |Z| <= 1e-8 -> scale 1 (kornia convert_points_from_homogeneous)
    t0 = torch.zeros(1, 1, 3, 3)
    t0[0, 0] = torch.tensor([[2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 5e-9]])
    p = torch.tensor([[[0.25, -0.5], [1.0, 1.0]]])
    assert torch.equal(transform_points(t0, p), warp_ref.transform_points(t0, p))


def test_kornia_meshgrid_is_the_pinned_axis():
    """create_meshgrid(h, w, normalized_coordinates=True): (linspace(0, n-1, n) / (n-1) - 0.5) * 2 in fp32, in that order
    (the order decides nearest rounding)"""
    kornia = pytest.importorskip("kornia")
    for h, w in ((360, 640), (720, 1280), (61, 97)):
        g = kornia.utils.create_meshgrid(h, w, normalized_coordinates=True)
        assert torch.equal(g[0, 0, :, 0], warp_ref.normalized_axis(w))
        assert torch.equal(g[0, :, 0, 1], warp_ref.normalized_axis(h))


# ------------------------------------------------------------------------------------------ OpenCV
def _frames(h, w, seed):
    return synth.synth_frames_u8(1, h, w, seed=seed)[0]


@pytest.mark.parametrize("src,dst", [((640, 360), (1280, 720)), ((1280, 720), (640, 360)), ((640, 360), (427, 240)),
                                     ((97, 61), (640, 360))])
def test_cv2_inter_nearest_vs_restatement(src, dst):
    """predict.py:286-315 resizes its masks with cv2.INTER_NEAREST"""
    cv2 = pytest.importorskip("cv2")
    img = _frames(src[1], src[0], 11)
    assert np.array_equal(cv2.resize(img, dst, interpolation=cv2.INTER_NEAREST), post_ref.resize_nearest(img, dst))
    ids = (img[..., 0] & 3).astype(np.uint8)
    assert np.array_equal(cv2.resize(ids, dst, interpolation=cv2.INTER_NEAREST), post_ref.resize_nearest(ids, dst))


@pytest.mark.parametrize("k", [(2, 2), (3, 3), (4, 4), (5, 5), (3, 2)])
def test_cv2_inter_area_integer_factor_vs_restatement(k):
    """utils/dataset.py:312-316 (video frames down to the UNet size): INTER_AREA with integer factors"""
    cv2 = pytest.importorskip("cv2")
    kx, ky = k
    img = _frames(36 * ky, 64 * kx, 13)
    want = cv2.resize(img, (64, 36), interpolation=cv2.INTER_AREA)
    assert np.array_equal(want, post_ref.resize_area_int(img, kx, ky))


@pytest.mark.parametrize("src,dst", [((480, 270), (256, 144)), ((400, 225), (160, 90)), ((250, 175), (160, 90))])
def test_cv2_inter_area_generic_vs_restatement(src, dst):
    """the generic INTER_AREA path (non-integer factors: 1920x1080 -> 1024x576 is this test's 1.875, 1600x900 -> 640x360 its
    2.5) at sizes the oracle's Python loop finishes in a second"""
    cv2 = pytest.importorskip("cv2")
    img = _frames(src[1], src[0], 17)
    want = cv2.resize(img, dst, interpolation=cv2.INTER_AREA)
    got = post_ref.resize_area(img, dst)
    assert np.array_equal(want, got), int((want != got).sum())


def test_cv2_png_stream_interchange(tmp_path):
    """predict.py:26-37 writes cv2.imencode('.png') buffers into a pickle stream, viz_preds.py:52-75 reads them with
    cv2.imdecode: our encoder's buffers decode with OpenCV and OpenCV's decode with ours"""
    cv2 = pytest.importorskip("cv2")
    from sfh_amd import outputs
    ids = (_frames(90, 160, 19)[..., 0] & 3).astype(np.uint8)
    rgb = post_ref.onehot_to_image(ids, 4)[0]
    for img in (ids, rgb):
        ours = outputs.encode_png(img)
        back = cv2.imdecode(np.frombuffer(bytes(ours), np.uint8), cv2.IMREAD_UNCHANGED)
        want = img if img.ndim == 2 else img[..., ::-1]          # cv2 arrays are BGR: predict.py hands BGR to imencode
        assert np.array_equal(back, want if img.ndim == 3 else img)
        ok, theirs = cv2.imencode(".png", img)
        assert ok
        dec = outputs.decode_png(bytes(theirs))
        assert np.array_equal(dec, img if img.ndim == 2 else img[..., ::-1])


# ------------------------------------------------------------------------------------------ always on
def test_the_pins_are_wired_to_what_is_importable():
    """this file must SKIP, not silently pass, where the packages are absent - and say which legs stay unpinned"""
    import importlib.util
    have = {m: importlib.util.find_spec(m) is not None for m in ("kornia", "cv2")}
    print("third-party pins active:", have)
    assert set(have) == {"kornia", "cv2"}


def test_argmax_of_softmax_tie_rule():
    """utils/postprocess.py:10-11 takes argmax(softmax(logits)); the HIP path takes argmax(logits) (outputs.py
    preds_to_masks / sfh_outconv_fwd).  exp and the division are only WEAKLY monotone in fp32: two logits closer than about
    1.2e-7 x their magnitude can round to the same probability, and argmax then returns the LOWER index where argmax(logits)
    returns the larger logit's.  The rule, made concrete: the two can differ only where the top-2 margin is below
    SOFTMAX_TIE_MARGIN; the parity tests count the golden pixels inside that band (tests/test_gpu_configs.py)."""
    from oracle.torch_ref import SOFTMAX_TIE_MARGIN, softmax_argmax_may_differ
    from oracle.torch_ref import preds_to_masks
    g = torch.Generator().manual_seed(4)
    lg = torch.randn(4, 4, 64, 64, generator=g) * 3
    # plant near-ties: class 3 ONE ulp above class 1 at magnitude 0.25 (margin 2^-25), both far above the rest
    lg[:, 0, ::4, ::4] = -9.0
    lg[:, 2, ::4, ::4] = -7.0
    lg[:, 1, ::4, ::4] = 0.25
    lg[:, 3, ::4, ::4] = torch.nextafter(torch.tensor(0.25), torch.tensor(1.0))
    a, b = lg.argmax(1), preds_to_masks(lg)
    differ = a != b
    assert int(differ.sum()) >= 4 * 16 * 16                       # the reference's rule is observable: every planted pixel ...
    assert bool((b[differ] == 1).all()) and bool((a[differ] == 3).all())   # ... goes to the LOWER index
    band = softmax_argmax_may_differ(lg)
    assert bool((differ <= band).all())                           # and only inside the stated band
    top2 = lg.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1])[differ].max()) < SOFTMAX_TIE_MARGIN
    # two ulps apart (6e-8) no longer ties: the band is conservative
    lg[:, 3, ::4, ::4] = torch.nextafter(lg[:, 3, ::4, ::4], torch.tensor(1.0))
    assert torch.equal(lg.argmax(1), preds_to_masks(lg))
