"""GPU checks of the Pillow-exact resize (sfh_amd.resample, csrc/resample.hip): the device bytes against the numpy restatement
tests/resample_ref.py (which tests/test_resample_host.py pins to Pillow), the float output against frames_u8_to_input of the
device's own bytes, guards and repeatability, the nearest resizes, and the opt-in wiring.  Every comparison is byte or bit
equality."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import resample_cases as RC
import resample_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64
FILTERS = ("box", "bilinear", "bicubic")


def _RS():
    from sfh_amd import resample as RS
    return RS


def _images(src_hw, C, B, seed=0, base=None):
    """B different images (B,H,W[,C]) uint8: variants of `base` or of seeded noise"""
    if base is None:
        base = RC.noise(src_hw if C == 1 else src_hw + (3,), seed)
    return np.stack([RC.variant(base, k) for k in range(B)])


@functools.lru_cache(maxsize=None)
def _want(src_hw, dst_hw, C, B, filt, seed, checker=False):
    """the restatement's bytes, computed once per case and shared (treated as read-only)"""
    base = (RC.checker(channels=None if C == 1 else 3) if checker else None)
    imgs = _images(src_hw, C, B, seed, base)
    want = np.stack([R.resize(im, (dst_hw[1], dst_hw[0]), R.FILTERS[filt]) for im in imgs])
    want.setflags(write=False)
    return imgs, want


def _max_tap_width(out=11):
    """source width whose bicubic table for `out` outputs has exactly MAX_TAPS coefficients: the integer factor MAX_TAPS / 4"""
    T = _RS().MAX_TAPS
    assert T % 4 == 0
    return T // 4 * out


def _over_bound_width(out=11):
    T = _RS().MAX_TAPS
    size = _max_tap_width(out)
    while int(R.coeffs(size, out, R.BICUBIC)[0][:, 1].max()) <= T:
        size += 1
    return size


# (source H, W), (destination H, W): the smallest shapes at which the kernel can go wrong
SMALL = (((1, 1), (5, 7)), ((5, 7), (1, 1)), ((37, 50), (16, 17)), ((9, 200), (9, 64)), ((64, 9), (3, 9)), ((17, 33), (34, 66)),
         ((40, 70), (39, 69)))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("shapes", SMALL, ids=lambda s: f"{s[0][0]}x{s[0][1]}_to_{s[1][0]}x{s[1][1]}")
def test_small_shapes_equal_the_restatement(shapes, filt, C):
    RS = _RS()
    src, dst = shapes
    for B in (1, 3):
        imgs, want = _want(src, dst, C, B, filt, 1)
        r = RS.Resampler(src, dst, C, filt)
        got = r.resize(torch.from_numpy(imgs).cuda())
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (shapes, filt, C, B)


@pytest.mark.parametrize("filt", FILTERS)
def test_batch_of_17_different_images(filt):
    RS = _RS()
    for C in (1, 3):
        imgs, want = _want((37, 50), (16, 17), C, 17, filt, 2)
        assert len({im.tobytes() for im in imgs}) == 17
        got = RS.Resampler((37, 50), (16, 17), C, filt).resize(torch.from_numpy(imgs).cuda())
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("C", [1, 3])
def test_largest_tap_count_and_the_refusal_beyond_it(C):
    RS = _RS()
    T = RS.MAX_TAPS
    w = _max_tap_width()
    assert int(R.coeffs(w, 11, R.BICUBIC)[0][:, 1].max()) == T
    for src, dst in (((8, w), (8, 11)), ((w, 8), (11, 8))):
        imgs, want = _want(src, dst, C, 2, "bicubic", 3)
        got = RS.Resampler(src, dst, C, "bicubic").resize(torch.from_numpy(imgs).cuda())
        assert np.array_equal(got.cpu().numpy(), want), (src, dst)
    # the bound + 1: refused on the host, nothing launched (the constructor needs no device)
    wo = _over_bound_width()
    assert int(R.coeffs(wo, 11, R.BICUBIC)[0][:, 1].max()) > T >= int(R.coeffs(wo - 1, 11, R.BICUBIC)[0][:, 1].max())
    for src, dst in (((8, wo), (8, 11)), ((wo, 8), (11, 8))):
        with pytest.raises(NotImplementedError, match=str(T)):
            RS.Resampler(src, dst, C, "bicubic")
        with pytest.raises(NotImplementedError, match=str(T)):
            RS.pil_resize_device(torch.zeros((1,) + src + (3,), dtype=torch.uint8, device="cuda"), (dst[1], dst[0]))


@pytest.mark.parametrize("filt", FILTERS)
def test_checker_reaches_both_clamps(filt):
    RS = _RS()
    for C in (1, 3):
        imgs, want = _want((64, 64), (90, 100), C, 1, filt, 0, True)
        got = RS.Resampler((64, 64), (90, 100), C, filt).resize(torch.from_numpy(imgs).cuda())
        assert np.array_equal(got.cpu().numpy(), want)
        assert want.min() == 0 and want.max() == 255


@pytest.mark.parametrize("src", [(720, 1280), (1080, 1920)])
def test_real_sizes(src):
    RS = _RS()
    imgs, want = _want(src, (360, 640), 3, 2, "bicubic", 4)
    u8, f32 = RS.Resampler(src, (360, 640)).both(torch.from_numpy(imgs).cuda())
    assert np.array_equal(u8.cpu().numpy(), want)
    assert torch.equal(f32.cpu(), torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)))


@pytest.mark.parametrize("shapes", [((37, 50), (16, 17)), ((9, 200), (9, 64)), ((64, 9), (3, 9)), ((17, 33), (34, 66)),
                                    ((12, 20), (12, 20))], ids=str)
def test_float_output_and_both(shapes):
    """to_input == frames_u8_to_input of the device's own bytes, bit for bit; both == the two single outputs"""
    from sfh_amd import engine as E
    RS = _RS()
    src, dst = shapes
    for C in (1, 3):
        imgs = torch.from_numpy(_images(src, 3, 3, 5)[..., :C].copy()).cuda()
        r = RS.Resampler(src, dst, C)
        u8 = r.resize(imgs)
        f32 = r.to_input(imgs)
        assert f32.dtype == torch.float32 and tuple(f32.shape) == (3, C) + dst
        assert torch.equal(f32, E.frames_u8_to_input(u8))
        bu8, bf32 = r.both(imgs)
        assert torch.equal(bu8, u8) and torch.equal(bf32, f32)
        if src == dst:
            assert torch.equal(u8, imgs) and u8.data_ptr() != imgs.data_ptr()        # equal sizes: a copy


def _guarded_call(lib, RS, imgs, src, dst, C, filt, want_u8, want_f32):
    """sfh_resample_u8 into buffers that end in a 64-element guard and start as a non-zero fill"""
    import ctypes
    from sfh_amd import _lib
    B = imgs.shape[0]
    n = B * dst[0] * dst[1] * C
    u8 = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if want_u8 else None
    f32 = torch.full((n + GUARD,), -7.5, dtype=torch.float32, device="cuda") if want_f32 else None
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    xb = xk = yb = yk = None
    xs = xt = ys = yt = 0
    rows = 16
    if src[1] != dst[1]:
        xb, xk, xs, xt, _ = RS._axis_tab(src[1], dst[1], filt, imgs.device)
    if src[0] != dst[0]:
        yb, yk, ys, yt, rows = RS._axis_tab(src[0], dst[0], filt, imgs.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.sfh_resample_u8(p(imgs), p(u8), p(f32), B, C, src[0], src[1], dst[0], dst[1], p(xb), p(xk), xs, xt, p(yb), p(yk),
                                   ys, yt, rows, st), "resample_u8")
    torch.cuda.synchronize()
    return u8, f32, n


@pytest.mark.parametrize("shapes", [((37, 50), (16, 17)), ((9, 200), (9, 64)), ((64, 9), (3, 9)), ((17, 33), (34, 66))], ids=str)
def test_guards_fill_and_repeatability(shapes):
    from sfh_amd import _lib
    RS = _RS()
    lib = _lib.load()
    src, dst = shapes
    for C in (1, 3):
        for filt in ("bicubic", "box"):
            host, want = _want(src, dst, C, 3, filt, 1)
            imgs = torch.from_numpy(host).cuda()
            runs = []
            for want_u8, want_f32 in ((True, False), (False, True), (True, True), (True, True)):
                u8, f32, n = _guarded_call(lib, RS, imgs, src, dst, C, filt, want_u8, want_f32)
                if u8 is not None:
                    assert bool((u8[n:] == 0xA5).all()), "uint8 guard touched"
                    assert np.array_equal(u8[:n].cpu().numpy().reshape(want.shape), want)
                if f32 is not None:
                    assert bool((f32[n:] == -7.5).all()), "float guard touched"
                    assert torch.equal(f32[:n].cpu().reshape(3, C, *dst),
                                       torch.from_numpy(want.reshape(3, *dst, C).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)))
                runs.append((u8, f32))
            assert torch.equal(runs[2][0], runs[3][0]) and torch.equal(runs[2][1], runs[3][1])      # two calls, the same bytes


def test_views_and_wrong_inputs_are_refused():
    RS = _RS()
    r = RS.Resampler((8, 12), (4, 6))
    base = torch.zeros((2, 8, 12, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((2, 8, 24, 3), dtype=torch.uint8, device="cuda")[:, :, ::2],               # strided
                torch.zeros((2, 12, 8, 3), dtype=torch.uint8, device="cuda").transpose(1, 2),          # transposed
                torch.zeros((1, 8, 12, 3), dtype=torch.uint8, device="cuda").expand(2, 8, 12, 3),      # expanded
                base.float(), base.cpu(), base[:, :, :, :1], base[:, :7], base[0]):
        for call in (r.resize, r.to_input, r.both):
            with pytest.raises(ValueError):
                call(bad)
    m = torch.zeros((2, 8, 12), dtype=torch.uint8, device="cuda")
    for bad in (m.transpose(1, 2), m.expand(3, 2, 8, 12)[0:1, :, :, ::2], m.to(torch.int32), m.cpu(),
                torch.zeros((2, 8, 12, 2), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            RS.resize_nearest(bad, (4, 6))
    with pytest.raises(ValueError):
        RS.resize_nearest(m, (4, 6), rule="area")
    with pytest.raises(ValueError):
        RS.resize_nearest(m, (0, 6))


@pytest.mark.parametrize("pair", RC.NEAREST_IMAGE_PAIRS, ids=str)
def test_resize_nearest_equals_the_restatement(pair):
    RS = _RS()
    src, dst = pair
    size = (dst[1], dst[0])
    for rule, code in (("pil", R.NEAREST_PIL), ("cv2", R.NEAREST_CV2)):
        for shape, dtype in ((src, np.uint8), (src + (1,), np.uint8), (src + (3,), np.uint8), (src + (3,), np.uint16)):
            imgs = np.stack([RC.noise(shape, 300 + k, dtype) for k in range(2)])
            t = torch.from_numpy(imgs.view(np.int16) if dtype == np.uint16 else imgs).cuda()
            if dtype == np.uint16:
                t = t.view(torch.uint16)
            got = RS.resize_nearest(t, dst, rule)
            assert got.dtype == t.dtype and tuple(got.shape) == (2,) + dst + shape[2:]
            g = got.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == np.uint16 else got.cpu().numpy()
            want = np.stack([R.resize_nearest(im, size, code) for im in imgs])
            assert np.array_equal(g, want), (pair, rule, shape, dtype)
            assert torch.equal(RS.resize_nearest(t, dst, rule).view(torch.uint8), got.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ wiring
def test_frames_u8_to_input_pil():
    from sfh_amd import engine as E
    RS = _RS()
    for src, dst in (((37, 50), (16, 17)), ((17, 33), (34, 66)), ((9, 200), (9, 64))):
        imgs = torch.from_numpy(_images(src, 3, 2, 6)).cuda()
        got = E.frames_u8_to_input(imgs, (dst[1], dst[0]), resize="pil")
        u8 = RS.Resampler(src, dst).resize(imgs)
        assert torch.equal(got, E.frames_u8_to_input(u8))
        assert torch.equal(got, RS.pil_resize_to_input(imgs, (dst[1], dst[0])))
        assert torch.equal(RS.pil_resize_device(imgs, (dst[1], dst[0])), u8)
    # same size: the plain / 255, whichever resize is named; the default is still INTER_AREA
    imgs = torch.from_numpy(_images((36, 64), 3, 2, 7)).cuda()
    assert torch.equal(E.frames_u8_to_input(imgs, (64, 36), resize="pil"), E.frames_u8_to_input(imgs))
    assert torch.equal(E.frames_u8_to_input(imgs, (32, 18), resize="area"), E.frames_u8_to_input(imgs, (32, 18)))
    assert not torch.equal(E.frames_u8_to_input(imgs, (32, 18), resize="pil"), E.frames_u8_to_input(imgs, (32, 18)))
    with pytest.raises(NotImplementedError):
        E.frames_u8_to_input(imgs, (128, 72))                    # an upscale is still not on the INTER_AREA path
    assert tuple(E.frames_u8_to_input(imgs, (128, 72), resize="pil").shape) == (2, 3, 72, 128)


def test_frame_pipeline_pil():
    """FramePipeline(resize="pil") on 720x1280 frames == a default pipeline fed the same frames resized by Pillow on the host,
    bit for bit, overlay and top view included; resize="area" is the default"""
    from PIL import Image
    from sfh_amd import mapping as M, synth, visualize as V
    from sfh_amd.pipeline import FramePipeline
    from sfh_amd.reconstructor import Reconstructor
    B = 2
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.cuda().eval()
    assert tuple(net.unet_size) == (640, 360)
    big = [synth.synth_frames_u8(B, 720, 1280, seed=70 + k) for k in range(3)]
    small = [np.stack([np.asarray(Image.fromarray(f).resize((640, 360))) for f in b]) for b in big]
    req = ("theta", "warp_mask", "segm_mask", "poi", "overlay")
    tmpl = synth.load_court_template("ncaa_nc4_640x360", 4, 1)

    def run(frame_hw, batches, **kw):
        r = V.OverlayRenderer(tmpl.cuda(), source="warp")
        tv = M.TopViewRenderer(out_size=(160, 90))
        pipe = FramePipeline(net, B, frame_hw, req_outputs=req, overlay=r, top_view=tv, **kw)
        return list(pipe.run(iter([torch.from_numpy(b).pin_memory() for b in batches])))

    with torch.no_grad():
        got = run((720, 1280), big, resize="pil")
        want = run((360, 640), small)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert set(g) == set(w) and {"overlay", "top_view", "top_view_valid", "theta", "segm_mask"} <= set(g)
            for k in w:
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), k
        # on same-size frames nothing is resized: "area", "pil" and no argument are the same pipeline
        again = run((360, 640), small, resize="area")
        for g, w in zip(again, want):
            for k in w:
                assert np.array_equal(g[k], w[k]), k
        # and "area" on larger frames is what the pipeline did before the argument existed
        a = run((720, 1280), big[:1], resize="area")
        b = run((720, 1280), big[:1])
        for k in b[0]:
            assert np.array_equal(a[0][k], b[0][k]), k
        assert a[0]["overlay"].shape == (B, 720, 1280, 3) and got[0]["overlay"].shape == (B, 360, 640, 3)
        assert not np.array_equal(a[0]["theta"], got[0]["theta"])


def test_to_batch_frame_resize():
    from PIL import Image
    import prep_fixtures as F
    from sfh_amd import preparation as P, synth
    W, H = 128, 96
    court, th = F.court_poi("pitch"), F.fixture_thetas()[:5]
    manual, n_short = F.exact_annotations(court, th, seed=13, n_short=1)
    lm = P.LabelMaker(F.court_ids("pitch_v3_nc4_640x360"), court, (W, H), 4)
    labels = lm.make(manual)
    frames = synth.synth_frames_u8(5, 270, 480, seed=3)
    with pytest.raises(ValueError):
        P.to_batch(labels, torch.from_numpy(frames).cuda())
    batch, dropped = P.to_batch(labels, torch.from_numpy(frames).cuda(), frame_resize="pil")
    keep = [k for k in range(5) if int(labels["status"][k]) == 1]
    assert len(dropped) == n_short and len(keep) == 5 - n_short
    want = np.stack([np.asarray(Image.fromarray(frames[k]).resize((W, H))) for k in keep])
    assert np.array_equal(batch["frames_u8"].cpu().numpy(), want)
    assert torch.equal(batch["image"].cpu(), torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)))
    # frames of the labels' size: unchanged by the argument
    same = synth.synth_frames_u8(5, H, W, seed=4)
    a, _ = P.to_batch(labels, torch.from_numpy(same).cuda(), frame_resize="pil")
    b, _ = P.to_batch(labels, torch.from_numpy(same).cuda())
    assert torch.equal(a["frames_u8"], b["frames_u8"]) and torch.equal(a["image"], b["image"])


def test_read_dataset_size(tmp_path):
    import prep_fixtures as F
    from sfh_amd import outputs as O, preparation as P
    court, ids = F.court_poi("pitch"), F.court_ids("pitch_v3_nc4_640x360")
    manual, _ = F.exact_annotations(court, F.fixture_thetas()[:4], seed=8, n_short=0)
    anno = tmp_path / "anno" / "game_a"
    os.makedirs(anno)
    with open(anno / "manual_anno.json", "w") as f:
        json.dump({f"{r:06d}": {"poi": manual[r].tolist(), "theta": None} for r in range(4)}, f)
    size = (100, 57)
    for uv in (False, True):
        dst = tmp_path / ("out_uv" if uv else "out")
        rep = P.prepare_dataset(str(tmp_path / "anno"), str(dst), ids, court, size=(188, 111), uv=uv, batch=4)
        assert len(rep["written"]) == 4
        plain = P.read_dataset(str(dst), rep["written"], use_uv=uv, device="cuda")
        got = P.read_dataset(str(dst), rep["written"], use_uv=uv, device="cuda", size=size)
        assert sorted(got) == sorted(plain)
        for k in ("poi", "nonzeros", "theta", "weight", "num_nonzero"):
            assert torch.equal(got[k], plain[k]), k
        for n, key in enumerate(rep["written"]):
            stem = os.path.join(str(dst), *key.split("/"))
            if uv:
                lab = R.resize_nearest(np.load(stem + ".npy"), size, R.NEAREST_CV2)
                m, uvp = P.split_uv(lab)
                assert np.array_equal(got["uv"][n].cpu().numpy(), uvp) and got["uv"].dtype == torch.float32
            else:
                m = R.resize_nearest(O.decode_png(np.fromfile(stem + ".png", dtype=np.uint8)), size, R.NEAREST_PIL)
            assert m.any() and np.array_equal(got["mask_u8"][n].cpu().numpy(), m)
        assert got["mask"].dtype == torch.int64 and torch.equal(got["mask"], got["mask_u8"].to(torch.int64))
        assert tuple(got["mask_u8"].shape) == (4, 57, 100)
    with pytest.raises(ValueError):
        P.read_dataset(str(dst), rep["written"], size=size)            # the resize runs on the device
