"""sfh_amd.jpegdec on the MI355X: the device decoder against the numpy restatement tests/jpegdec_ref.py (which
tests/test_jpegdec_host.py holds to PIL's pixels), byte for byte.  Only well-formed files are decoded here: corrupt streams go
through the stand-alone host program of tests/test_jpegdec_host.py."""
import os

import numpy as np
import pytest
import torch

import jpegdec_cases as DC
import jpegdec_ref as R
import jpegenc_cases as EC

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 17)
GUARD = 64
_FILES = DC.small_files()
SMALL = sorted(n for n in _FILES if "16x1280" not in n)        # sizes up to 333 x 187
_REF = {}


def _ref(data, bgr=True):
    """the restatement's frame of a file, computed once and never written to"""
    key = (bytes(data), bgr)
    if key not in _REF:
        p = R.parse(data)
        coef, statuses = R.decode_serial(p, data)
        assert not any(statuses)
        _REF[key] = R.pixels(p, coef, bgr)
        _REF[key].setflags(write=False)
    return _REF[key]


def _decoder(data, batch, **kw):
    from sfh_amd.jpegdec import JpegDecoder
    p = R.parse(data)
    return JpegDecoder(p["height"], p["width"], p["ncomp"], batch, **kw)


def _guarded(dec, n, fill=0xA5):
    """an output of n images that starts non-zero, with GUARD elements behind it -> (flat buffer, view to decode into)"""
    shape = (n, dec.H, dec.W) + ((3,) if dec.C == 3 else ())
    numel = int(np.prod(shape))
    flat = torch.full((numel + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return flat, flat[:numel].view(shape)


@pytest.mark.parametrize("name", SMALL)
def test_frames_equal_restatement(name):
    data = _FILES[name]
    dec = _decoder(data, 3)
    colour = dec.C == 3
    for b in (1, 3):
        flat, out = _guarded(dec, b)
        got = dec.decode([data] * b, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert not dec.status.any(), dec.status
        assert dec.rounds() >= 1
        host = flat.cpu().numpy()
        want = _ref(data)
        for k in range(b):
            assert np.array_equal(host[k * want.size:(k + 1) * want.size].reshape(want.shape), want), f"{name} image {k} of {b}"
        assert (host[b * want.size:] == 0xA5).all(), "guard elements behind the output were written"
    if colour:
        rgb = _decoder(data, 1, bgr=False).decode([data])
        assert np.array_equal(rgb[0].cpu().numpy(), _ref(data, bgr=False))


@pytest.mark.parametrize("kind,dri", [("420", None), ("444", "blocks"), ("gray", "rows"), ("420", "rows")])
def test_batch_of_17_different_files(kind, dri):
    """17 different files of different lengths in one call; then fewer files through the same decoder, twice: same bytes"""
    src = EC.small_cases()["noise_160x48_gray" if kind == "gray" else "noise_160x48_rgb"][0]
    files = [DC.pil_file(EC.variant(src, k), 50 + 3 * k, subsampling=0 if kind == "444" else None, dri=dri, optimize=bool(k & 1))
             for k in range(17)]
    assert len({len(f) for f in files}) > 8
    dec = _decoder(files[0], 17, max_file_bytes=max(len(f) for f in files))
    want = np.stack([_ref(f) for f in files])
    for b in BATCHES:
        got = dec.decode(files[:b]).cpu().numpy()
        assert not dec.status.any()
        assert np.array_equal(got, want[:b]), f"batch {b}"
    again = dec.decode([np.frombuffer(f, np.uint8) for f in files]).cpu().numpy()
    assert np.array_equal(again, want)


def test_many_subsequences_and_stuffed_bytes():
    """333 x 187 noise at quality 100 without DRI: more subsequences than the workgroup has threads, stuffed 0xFF bytes at
    subsequence boundaries; every subsequence size gives the same bytes"""
    data = _FILES["noise_333x187_q100_420"]
    p = R.parse(data)
    scan = data[p["scan_begin"]:p["scan_end"]]
    assert len(scan) * 8 > 256 * 1024
    ff = np.flatnonzero(np.frombuffer(scan, np.uint8) == 0xFF)
    assert (ff % 128 == 127).any() and (ff % 128 == 0).any()      # a stuffing byte is the first / second byte of a subsequence
    want = _ref(data)
    dec = _decoder(data, 1)
    assert dec.subseq_bits == 1024
    got = dec.decode([data])[0].cpu().numpy()
    assert np.array_equal(got, want) and not dec.status.any()
    assert dec.rounds() >= 2
    for bits in (32, 64, 4096):
        d = _decoder(data, 1, max_file_bytes=len(data), _subseq_bits=bits)
        assert d.subseq_bits == bits
        assert np.array_equal(d.decode([data])[0].cpu().numpy(), want), bits
        assert not d.status.any() and d.rounds() >= 2


@pytest.mark.parametrize("hw,dri", [((720, 1280), None), ((1080, 1920), "rows")])
def test_full_size_template_over_noise(hw, dri):
    # PIL's pixels are the reference here: the restatement equals them (tests/test_jpegdec_host.py) and takes a minute at this size
    data = DC.big_file(hw[0], hw[1], dri=dri)
    dec = _decoder(data, 1, max_file_bytes=len(data))
    got = dec.decode([data])[0].cpu().numpy()
    assert not dec.status.any()
    assert np.array_equal(got, DC.pil_decode(data, bgr=True))


def test_encoder_round_trip_on_the_device():
    """JpegEncoder's JpegBatch goes into the decoder as it is; the frames equal outputs.decode_jpeg of the same files"""
    from sfh_amd.jpegenc import JpegEncoder
    from sfh_amd.outputs import decode_jpeg
    for name in ("noise_37x50_rgb", "noise_160x48_gray", "hramp_rgb"):
        img = EC.small_cases()[name][0]
        imgs = torch.from_numpy(np.stack([EC.variant(img, k) for k in range(3)])).cuda()
        enc = JpegEncoder(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, 3, quality=90)
        batch = enc.encode(imgs)
        dec = _decoder(batch.to_host()[0].tobytes(), 3)
        got = dec.decode(batch).cpu().numpy()
        assert not dec.status.any()
        for k, f in enumerate(batch.to_host()):
            assert np.array_equal(got[k], decode_jpeg(f)), (name, k)


def test_decode_jpeg_device_and_repeatability():
    from sfh_amd.jpegdec import decode_jpeg_device
    data = _FILES["noise_37x50_444"]
    one = decode_jpeg_device(data)
    assert tuple(one.shape) == (37, 50, 3) and np.array_equal(one.cpu().numpy(), _ref(data))
    many = decode_jpeg_device([data, data], bgr=False)
    assert tuple(many.shape) == (2, 37, 50, 3) and np.array_equal(many[1].cpu().numpy(), _ref(data, bgr=False))
    gray = decode_jpeg_device(np.frombuffer(_FILES["noise_17x33_gray"], np.uint8))
    assert tuple(gray.shape) == (17, 33) and np.array_equal(gray.cpu().numpy(), _ref(_FILES["noise_17x33_gray"]))
    dec = _decoder(data, 1)
    a = dec.decode([data]).clone()
    b = dec.decode([data])
    assert torch.equal(a, b)


def test_wrong_out_and_refused_files_launch_nothing():
    data = _FILES["noise_16x24_420"]
    dec = _decoder(data, 2)
    good = dec.decode([data, data]).clone()
    assert np.array_equal(good[0].cpu().numpy(), _ref(data))
    base = torch.full((2, 16, 48, 3), 7, dtype=torch.uint8, device="cuda")
    bad = [base[:, :, ::2],                                                       # strided
           torch.zeros((2, 16, 24), dtype=torch.uint8, device="cuda"),              # shape
           torch.zeros((2, 24, 16, 3), dtype=torch.uint8, device="cuda"),
           torch.zeros((1, 16, 24, 3), dtype=torch.uint8, device="cuda"),           # too few images
           torch.zeros((2, 16, 24, 3), dtype=torch.int8, device="cuda")]            # dtype
    for out in bad:
        with pytest.raises(ValueError):
            dec.decode([data, data], out=out)
    assert (base == 7).all()
    with pytest.raises(ValueError):
        dec.decode([data, data], out=np.zeros((2, 16, 24, 3), np.uint8))
    with pytest.raises(ValueError, match="size"):
        dec.decode([data, _FILES["noise_24x16_420"]])
    with pytest.raises(NotImplementedError, match="progressive"):
        import io
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(EC.small_cases()["noise_16x24_rgb"][0]).save(buf, "JPEG", progressive=True)
        dec.decode([data, buf.getvalue()])
    with pytest.raises(ValueError, match="max_file_bytes"):
        _decoder(data, 1, max_file_bytes=len(data) - 1).decode([data])
    torch.cuda.synchronize()
    assert torch.equal(dec.out, good), "a refused call wrote into the decoder's frames"


def _net_and_frames(B):
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    w, h = 112, 90
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :h, :w].contiguous()
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(w, h), unet_size=(w, h), warp_size=(w, h), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    return net.cuda().eval(), court


def test_frame_pipeline_submit_jpeg():
    """submit_jpeg(files) == submit(the frames PIL decodes from the same files), bit for bit, with and without resize="pil" """
    from sfh_amd import mapping as M, synth, visualize as V
    from sfh_amd.pipeline import FramePipeline
    B = 2
    net, court = _net_and_frames(B)
    req = ("theta", "warp_mask", "segm_mask", "poi", "overlay")

    def run(frame_hw, batches, jpeg, **kw):
        r = V.OverlayRenderer(court[:1].cuda(), source="warp")
        tv = M.TopViewRenderer(out_size=(80, 48))
        pipe = FramePipeline(net, B, frame_hw, req_outputs=req, overlay=r, top_view=tv, **kw)
        return list(pipe.run(iter(batches), jpeg=jpeg))

    for hw, kw in (((90, 112), {}), ((135, 168), {"resize": "pil"}), ((180, 224), {})):
        frames = [synth.synth_frames_u8(B, hw[0], hw[1], seed=40 + k) for k in range(3)]
        files = [[DC.pil_file(np.ascontiguousarray(f[:, :, ::-1]), 90, dri=("rows", None)[k & 1]) for f in b]
                 for k, b in enumerate(frames)]
        decoded = [torch.from_numpy(np.stack([DC.pil_decode(f, bgr=True) for f in b])).pin_memory() for b in files]
        with torch.no_grad():
            want = run(hw, decoded, False, **kw)
            got = run(hw, files, True, jpeg_in_max_bytes=max(len(f) for b in files for f in b), **kw)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert set(g) == set(w) and {"overlay", "top_view", "theta", "segm_mask"} <= set(g)
            for k in w:
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), (hw, k)


def test_visualize_and_rectify_game_from_jpeg_files(tmp_path):
    from sfh_amd import synth
    from sfh_amd.mapping import rectify_game
    from sfh_amd.outputs import CourtJsonWriter
    from sfh_amd.visualize import visualize
    frames = list(synth.synth_frames_u8(3, 90, 112, seed=7))
    files = [DC.pil_file(np.ascontiguousarray(f[:, :, ::-1]), 90) for f in frames]
    decoded = [DC.pil_decode(f, bgr=True) for f in files]
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    with CourtJsonWriter(str(tmp_path), "game", "model-x") as wr:
        for k in range(3):
            wr.add(str(k), score=0.01 * (k + 1), theta=np.eye(3, dtype=np.float32).reshape(1, 3, 3))
    preds = os.path.join(str(tmp_path), "game_court.json")
    for what, call in (("viz", lambda fr, dst, **kw: visualize(fr, preds, dst, court, batch=2, **kw)),
                       ("top", lambda fr, dst, **kw: rectify_game(preds, fr, dst, out_size=(160, 96), batch=2, **kw))):
        a = call(iter(decoded), os.path.join(str(tmp_path), what + "_arrays"))
        b = call(iter(files), os.path.join(str(tmp_path), what + "_files"), frames_format="jpeg")
        assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] and len(a) >= 3
        for x, y in zip(a, b):
            assert open(x, "rb").read() == open(y, "rb").read(), (what, os.path.basename(x))
    with pytest.raises(ValueError, match="frames_format"):
        visualize(iter(files), preds, os.path.join(str(tmp_path), "bad"), court, frames_format="png")
