"""sfh_amd.jpegenc on the MI355X: the device encoder against the numpy restatement tests/jpegenc_ref.py (which
tests/test_jpegenc_host.py holds to libjpeg's bytes), byte for byte."""
import os

import numpy as np
import pytest
import torch

import jpegenc_cases as cases
import jpegenc_ref as R

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 17)
_SMALL = cases.small_cases()
_FULL = {f"template_{n}": (lambda n=n: (cases.template_over_noise(n), 90)) for n in cases.TEMPLATES}
_REFS = {}


def _batch_and_refs(name, bgr=True):
    """the images of a case's batch and their reference files, computed once.  Small cases: 17 different images (rolled
    variants, whose files differ in size).  The full-size templates (360x640 and 720x1280 colour): one image."""
    key = (name, bgr)
    if key not in _REFS:
        img, q = _SMALL[name] if name in _SMALL else _FULL[name]()
        n = max(BATCHES) if name in _SMALL else 1
        imgs = [cases.variant(img, k) for k in range(n)]
        _REFS[key] = (np.stack(imgs), [np.frombuffer(R.ref_encode(im, q, bgr=bgr), np.uint8) for im in imgs], q)
    return _REFS[key]


def _encoder(img, batch, quality, **kw):
    from sfh_amd.jpegenc import JpegEncoder
    return JpegEncoder(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, batch, quality=quality, **kw)


def _assert_files(out, refs, b, what, capacity=None):
    files = out.to_host()
    sizes, off = out.sizes.cpu().numpy(), out.offsets.cpu().numpy()
    assert len(files) == b
    for k in range(b):
        assert int(sizes[k]) == refs[k].size, f"{what} image {k}: {int(sizes[k])} bytes, restatement {refs[k].size}"
        assert np.array_equal(files[k], refs[k]), f"{what} image {k}: first difference at byte " \
                                                  f"{int(np.flatnonzero(files[k] != refs[k])[0])}"
    if capacity is None:
        assert off[0] == 0 and np.array_equal(np.diff(off), sizes)            # compact: back to back
    else:
        assert off.tolist() == [k * capacity for k in range(b + 1)]


# every case in the memory order of cv2 (bgr=True, the default); every small 3-channel case in RGB order too (the full-size
# templates add no shape or content to those, and their restatement takes seconds)
_ORDERS = [(n, True) for n in list(_SMALL) + list(_FULL)] + [(n, False) for n in _SMALL if not n.endswith("_gray")]


@pytest.mark.parametrize("name,bgr", _ORDERS, ids=[n + ("" if o else "-rgb_order") for n, o in _ORDERS])
def test_bytes_equal_restatement(name, bgr):
    imgs, refs, q = _batch_and_refs(name, bgr)
    assert bgr or imgs.ndim == 4
    dev = torch.from_numpy(imgs).cuda()
    for compact in (True, False):
        enc = _encoder(imgs[0], len(imgs), q, compact=compact, bgr=bgr)
        for b in [b for b in BATCHES if b <= len(imgs)]:
            out = enc.encode(dev[:b].contiguous())
            _assert_files(out, refs, b, f"{name} batch {b} compact {compact} bgr {bgr}", None if compact else enc.capacity)


def test_refuses_what_is_not_a_contiguous_batch_of_its_shape():
    """on the device too, where the tensor passes the device check: a strided view is refused, not encoded as if it were dense"""
    img = _SMALL["noise_16x24_rgb"][0]
    enc = _encoder(img, 2, 90)
    dev = torch.from_numpy(np.stack([img, cases.variant(img, 1)])).cuda()
    enc.encode(dev)
    before = enc.out.data.clone()
    wide = torch.full((2, 16, 48, 3), 7, dtype=torch.uint8, device="cuda")
    square = torch.full((2, 24, 24, 3), 7, dtype=torch.uint8, device="cuda")
    for bad in (wide[:, :, ::2], square.transpose(1, 2)[:, :16], dev[:1].expand(2, 16, 24, 3)):
        assert tuple(bad.shape) == (2, 16, 24, 3) and not bad.is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            enc.encode(bad)
    for bad in (dev[0], dev[:, :, :23], dev[:, :15], torch.cat([dev, dev[:1]])):
        with pytest.raises(ValueError, match="expected"):
            enc.encode(bad.contiguous())
    with pytest.raises(ValueError, match="dtype"):
        enc.encode(dev.to(torch.int16))
    assert torch.equal(enc.out.data, before)                                  # nothing was launched


def test_one_off_entry_point():
    from sfh_amd.jpegenc import encode_jpeg_device
    from sfh_amd.outputs import decode_jpeg, encode_jpeg
    img, q = _SMALL["noise_333x187_rgb"]
    buf = encode_jpeg_device(torch.from_numpy(img).cuda(), quality=q)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and np.array_equal(buf, encode_jpeg(img, q))
    assert decode_jpeg(buf).shape == img.shape
    gray = np.stack([_SMALL["noise_37x50_gray"][0], cases.variant(_SMALL["noise_37x50_gray"][0], 2)])
    files = encode_jpeg_device(torch.from_numpy(gray).cuda(), quality=75)
    assert [np.array_equal(f, encode_jpeg(g, 75)) for f, g in zip(files, gray)] == [True, True]


def test_deterministic():
    imgs, _, q = _batch_and_refs("noise_333x187_rgb")
    enc = _encoder(imgs[0], 17, q)
    dev = torch.from_numpy(imgs).cuda()
    a, b = enc.new_output(), enc.new_output()
    a.data.zero_()
    b.data.zero_()
    enc.encode(dev, out=a)
    enc.encode(dev, out=b)
    assert torch.equal(a.data, b.data) and torch.equal(a.offsets, b.offsets) and torch.equal(a.sizes, b.sizes)


@pytest.mark.parametrize("compact", [True, False])
def test_guard_after_capacity_untouched(compact):
    from sfh_amd.jpegenc import JpegBatch
    imgs, refs, _ = _batch_and_refs("noise_37x50_q100_rgb")
    B, guard = 3, 4096
    enc = _encoder(imgs[0], B, 100, compact=compact)
    buf = torch.full((B * enc.capacity + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = JpegBatch(buf[:B * enc.capacity], torch.empty(B + 1, dtype=torch.int64, device="cuda"),
                    torch.empty(B, dtype=torch.int32, device="cuda"))
    enc.encode(torch.from_numpy(imgs[:B]).cuda(), out=out)
    torch.cuda.synchronize()
    assert bool((buf[B * enc.capacity:] == 0xA5).all())
    assert out.sizes.cpu().tolist() == [r.size for r in refs[:B]]


def test_multi_pass_branch():
    """16 x 1920 noise at quality 100: the interval's bit stream is longer than the LDS bit window, so it is emitted in several
    passes (the encoder's counter says so), and the bytes are still the restatement's.  The same with a window of a few dwords
    on small images, where a block spans several windows."""
    img = _SMALL["noise_16x1920_rgb"][0]
    ref = np.frombuffer(R.ref_encode(img, 100), np.uint8)
    enc = _encoder(img, 1, 100)
    out = enc.encode(torch.from_numpy(img[None]).cuda())
    assert int(enc.passes().min()) >= 2
    _assert_files(out, [ref], 1, "16x1920 noise q100")
    for name, win in (("noise_37x50_rgb", 1), ("noise_37x50_gray", 7), ("blocks0_255_q100_rgb", 40)):
        imgs, refs, q = _batch_and_refs(name)
        enc = _encoder(imgs[0], 3, q, _window_dwords=win)
        out = enc.encode(torch.from_numpy(imgs[:3]).cuda())
        assert int(enc.passes().max()) >= 2
        _assert_files(out, refs, 3, f"{name} window {win}")


_NET = {}


def _small_pipeline(**kw):
    from sfh_amd import synth
    from sfh_amd.pipeline import FramePipeline
    from sfh_amd.reconstructor import Reconstructor
    from sfh_amd.visualize import OverlayRenderer
    w, h, B = 640, 360, 2
    if not _NET:                                       # one model and renderer for every pipeline of this file
        court = synth.load_court_template("ncaa_nc4_640x360", 4, B)
        poi = synth.load_court_poi("pitch", B)
        net = Reconstructor(court.cuda(), poi.cuda(), target_size=(w, h), unet_size=(w, h), warp_size=(w, h), warp_with_nearest=True)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
        _NET["net"] = net.cuda().eval()
        _NET["renderer"] = OverlayRenderer(court[:1].cuda(), mask_classes=4, source="warp")
    return FramePipeline(_NET["net"], B, (h, w), req_outputs=("theta", "warp_mask", "overlay"), overlay=_NET["renderer"], **kw)


@pytest.mark.parametrize("budget", [None, 64])
def test_pipeline_jpeg_outputs(budget):
    """FramePipeline(overlay=r, jpeg=("overlay",)) against the same pipeline without jpeg on 4 synthetic frames at 360x640: every
    other output bit-identical, the files equal JpegEncoder applied to the raw overlay.  budget 64: every batch overflows."""
    from sfh_amd import synth
    from sfh_amd.jpegenc import JpegEncoder
    frames = [torch.from_numpy(synth.synth_frames_u8(2, 360, 640, seed=40 + k)).pin_memory() for k in range(2)]
    with torch.no_grad():
        plain = list(_small_pipeline().run(frames))
        coded = list(_small_pipeline(jpeg=("overlay",), jpeg_budget=budget).run(frames))
    assert len(plain) == len(coded) == 2
    enc = JpegEncoder(360, 640, 3, 2, quality=90)
    for p, c in zip(plain, coded):
        assert sorted(c) == sorted([k for k in p if k != "overlay"] + ["overlay_jpeg"])
        for k in c:
            if k != "overlay_jpeg":
                assert np.array_equal(p[k], c[k]), k
        want = enc.encode(torch.from_numpy(p["overlay"]).cuda()).to_host()
        assert len(c["overlay_jpeg"]) == 2
        assert all(np.array_equal(f, w) for f, w in zip(c["overlay_jpeg"], want))
    with pytest.raises(ValueError, match="both"):
        _small_pipeline(png=("overlay",), jpeg=("overlay",))
    with pytest.raises(ValueError):
        _small_pipeline(jpeg=("warp_mask",))


def test_rectify_game_device_leg_equals_host_leg(tmp_path):
    """rectify_game(image_format="jpeg"): <name>.jpeg and mosaic.jpeg, the same bytes from either leg, and the JPEG of the very
    views that the default writes as PNG"""
    from sfh_amd import synth
    from sfh_amd.mapping import rectify_game
    from sfh_amd.outputs import CourtJsonWriter, decode_png, encode_jpeg
    frames = list(synth.synth_frames_u8(3, 90, 112, seed=11))
    thetas = [np.eye(3, dtype=np.float32), synth.REALISTIC_THETAS[0], synth.REALISTIC_THETAS[1]]
    with CourtJsonWriter(str(tmp_path), "game", "model-x") as wr:
        for k, th in enumerate(thetas):
            wr.add(str(k), score=0.01 * (k + 1), theta=np.asarray(th, dtype=np.float32).reshape(1, 3, 3))
    names = ["0", "1", "2", "mosaic"]
    files = {}
    for leg, fmt in (("host", "jpeg"), ("device", "jpeg"), ("host", "png")):
        dst = os.path.join(str(tmp_path), leg + fmt)
        paths = rectify_game(wr.path, iter(frames), dst, out_size=(160, 96), batch=2, png=leg, image_format=fmt, jpeg_quality=75)
        assert [os.path.basename(p) for p in paths] == [f"{n}.{fmt}" for n in names]
        files[leg, fmt] = [np.fromfile(p, dtype=np.uint8) for p in paths]
    assert decode_png(files["host", "png"][0]).any()                          # the identity's view is the frame, resized
    for host, dev, png in zip(files["host", "jpeg"], files["device", "jpeg"], files["host", "png"]):
        view = decode_png(png)
        assert view.shape == (96, 160, 3)
        assert np.array_equal(host, dev) and np.array_equal(dev, encode_jpeg(view, 75))


def test_visualize_device_leg_equals_host_leg(tmp_path):
    from sfh_amd import synth
    from sfh_amd.outputs import CourtJsonWriter
    from sfh_amd.visualize import visualize
    frames = list(synth.synth_frames_u8(3, 90, 112, seed=7))
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    with CourtJsonWriter(str(tmp_path), "game", "model-x") as wr:
        for k in range(3):
            wr.add(str(k), score=0.01 * (k + 1), theta=np.eye(3, dtype=np.float32).reshape(1, 3, 3))
    preds = os.path.join(str(tmp_path), "game_court.json")
    paths = {}
    for leg in ("host", "device"):
        dst = os.path.join(str(tmp_path), leg)
        paths[leg] = visualize(frames, preds, dst, court, png=leg, image_format="jpeg", jpeg_quality=90, batch=2)
        assert [os.path.basename(p) for p in paths[leg]] == ["0.jpeg", "1.jpeg", "2.jpeg"]
    for a, b in zip(paths["host"], paths["device"]):
        assert open(a, "rb").read() == open(b, "rb").read()
