"""sfh_amd.pngdec on the MI355X: the device decoder against outputs.decode_png (which tests/test_pngdec_host.py holds to PIL's
pixels), byte for byte, and what PngDecoder.segmented() says against what the file allows.  Only well-formed files are decoded
here: corrupt streams go through the stand-alone host program of tests/test_pngdec_host.py."""
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch

import pngdec_cases as PC

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 17)
GUARD = 64
FILES = PC.all_files()
NAMES = sorted(n for n in FILES if not n.startswith("fixture_"))
_REF = {}


def _ref(data):
    """outputs.decode_png of a file (BGR(A)), computed once and never written to"""
    from sfh_amd.outputs import decode_png
    key = bytes(data)
    if key not in _REF:
        _REF[key] = decode_png(np.frombuffer(key, np.uint8))
        _REF[key].setflags(write=False)
    return _REF[key]


def _file_order(px):
    return px if px.ndim == 2 else np.ascontiguousarray(px[:, :, [2, 1, 0] + ([3] if px.shape[2] == 4 else [])])


def _decoder(data, batch, **kw):
    from sfh_amd.pngdec import PngDecoder, parse_png
    p = parse_png(data)
    kw.setdefault("max_file_bytes", len(data))
    return PngDecoder(p["height"], p["width"], p["channels"], batch, **kw)


def _guarded(dec, n, fill=0xA5):
    """an output of n images that starts non-zero, with GUARD elements behind it -> (flat buffer, view to decode into)"""
    shape = dec._shape(n)
    numel = int(np.prod(shape))
    flat = torch.full((numel + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return flat, flat[:numel].view(shape)


@pytest.mark.parametrize("name", NAMES)
def test_images_equal_decode_png(name):
    data, segmented = FILES[name]
    want = _ref(data)
    dec = _decoder(data, 1)
    flat, out = _guarded(dec, 1)
    got = dec.decode([data], out=out)
    assert got.data_ptr() == out.data_ptr()
    assert dec.status.tolist() == [0]
    assert dec.segmented().tolist() == [segmented]
    host = flat.cpu().numpy()
    assert np.array_equal(host[:want.size].reshape(want.shape), want)
    assert (host[want.size:] == 0xA5).all(), "guard elements behind the output were written"
    again = dec.decode([np.frombuffer(data, np.uint8)])                         # into the decoder's own buffer: the same bytes
    assert np.array_equal(again[0].cpu().numpy(), want) and dec.status.tolist() == [0]
    if want.ndim == 3:
        rgb = _decoder(data, 1, bgr=False).decode([data])
        assert np.array_equal(rgb[0].cpu().numpy(), _file_order(want))


def _seventeen(C):
    """17 different 37 x 50 files: every recipe and pattern, one chunk, arbitrary cuts and full-flush cuts mixed"""
    rng = np.random.default_rng(1700 + C)
    files, seg = [], []
    recipes = list(PC.RECIPES.values())
    for k in range(17):
        img = PC.labels(rng, 37, 50, C) if k % 3 else PC.noise(rng, 37, 50, C)
        pat = PC.pattern(PC.PATTERNS[k % len(PC.PATTERNS)], 37)
        if k % 4 == 1:
            files.append(PC.write_png(img, pat, recipes[k % 5], flushes={12: zlib.Z_FULL_FLUSH, 30: zlib.Z_FULL_FLUSH}, cut_at_flushes=True))
        elif k % 4 == 3:
            files.append(PC.write_png(img, pat, recipes[k % 5], cuts=(7, 8, 40 + k)))
        else:
            files.append(PC.write_png(img, pat, recipes[k % 5]))
        seg.append(k % 4 == 1)
    return files, seg


@pytest.mark.parametrize("C", (1, 3, 4))
def test_batches_of_different_files(C):
    """17 different files of different lengths and both legs in one call; then fewer files through the same decoder"""
    files, seg = _seventeen(C)
    assert len({len(f) for f in files}) > 8
    want = np.stack([_ref(f) for f in files])
    dec = _decoder(files[0], 17, max_file_bytes=max(len(f) for f in files))
    for b in BATCHES:
        flat, out = _guarded(dec, b)
        dec.decode(files[:b], out=out)
        assert not dec.status.any()
        assert dec.segmented().tolist() == seg[:b]
        host = flat.cpu().numpy()
        assert np.array_equal(host[:want[:b].size].reshape(want[:b].shape), want[:b]), f"batch {b}"
        assert (host[want[:b].size:] == 0xA5).all()
    again = dec.decode([np.frombuffer(f, np.uint8) for f in files]).cpu().numpy()
    assert np.array_equal(again, want)
    # the serial leg alone on the same files: the same bytes
    ser = _decoder(files[0], 17, max_file_bytes=max(len(f) for f in files), _serial_only=True)
    assert np.array_equal(ser.decode(files).cpu().numpy(), want)
    assert not ser.status.any() and not ser.segmented().any()


def test_default_file_capacity_and_decode_png_device():
    from sfh_amd.pngdec import PngDecoder, decode_png_device
    data = FILES["recipe_stored_noise_333x187x4"].data                         # larger than its pixels
    dec = PngDecoder(333, 187, 4, 2)
    assert dec.max_file_bytes >= len(data)
    assert np.array_equal(dec.decode([data, data])[1].cpu().numpy(), _ref(data))
    one = decode_png_device(data)
    assert tuple(one.shape) == (333, 187, 4) and np.array_equal(one.cpu().numpy(), _ref(data))
    files, _ = _seventeen(1)
    many = decode_png_device(files[:5], bgr=False)
    assert np.array_equal(many.cpu().numpy(), np.stack([_ref(f) for f in files[:5]]))


@pytest.mark.parametrize("name", PC.FIXTURES)
def test_fixtures_equal_pil(name):
    from PIL import Image
    from sfh_amd.pngdec import decode_png_device
    data = PC.fixture(name)
    with Image.open(io.BytesIO(data)) as im:
        want = np.array(im)
    got = decode_png_device(data, bgr=False)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def test_encoder_round_trip_on_the_device():
    """PngEncoder's PngBatch goes into the decoder as it is: the images come back, every file with more than one strip on the
    segmented leg"""
    import pngenc_cases as EC
    from sfh_amd.pngenc import PngEncoder
    for name in ("alternating", "333x187_rgb", "wide_3000x23", "1x1", "noise_rgb", "runs", "7x5_rgb"):
        img = np.asarray(EC.small_cases()[name])
        img = img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img
        C = 1 if img.ndim == 2 else 3
        imgs = torch.from_numpy(np.stack([EC.variant(img, k) for k in range(3)])).cuda()
        batch = PngEncoder(img.shape[0], img.shape[1], C, 3).encode(imgs)
        files = batch.to_host()
        dec = _decoder(files[0], 3, max_file_bytes=max(f.size for f in files))
        got = dec.decode(batch)
        assert not dec.status.any(), name
        assert torch.equal(got, imgs), name
        strips = -(-img.shape[0] // max(1, min(16, 32768 // (1 + img.shape[1] * C))))
        assert dec.segmented().tolist() == [strips > 1] * 3, name


def test_wrong_out_and_refused_files_launch_nothing():
    files, _ = _seventeen(3)
    dec = _decoder(files[0], 3, max_file_bytes=max(len(f) for f in files))
    flat, out = _guarded(dec, 3)
    bad_outs = [(ValueError, out.cpu().numpy()), (ValueError, out.to(torch.int32)), (ValueError, out[:2]), (ValueError, out[:, :, :, :2]),
                (ValueError, out.permute(0, 2, 1, 3)), (ValueError, flat[:out.numel()]), (RuntimeError, out.cpu())]
    for exc, o in bad_outs:
        with pytest.raises(exc, match="out"):
            dec.decode(files[:3], out=o)
    gray = PC.write_png(PC.labels(np.random.default_rng(1), 37, 50, 1), PC.pattern("all1", 37))
    palette = PC.SIG + PC.ihdr(37, 50, 1, ctype=3) + PC.chunk(b"PLTE", bytes(12)) + files[0][33:]
    crc = bytearray(files[1])
    crc[60] ^= 1
    for exc, lst in ((ValueError, [files[0], gray]), (NotImplementedError, [files[0], files[1], palette]), (ValueError, [bytes(crc)]),
                     (ValueError, [files[0][:-12]]), (ValueError, []), (ValueError, files[:4])):
        with pytest.raises(exc):
            dec.decode(lst, out=out)
    with pytest.raises(ValueError, match="max_file_bytes"):
        _decoder(files[0], 1, max_file_bytes=len(files[0]) - 1).decode([files[0]])
    with pytest.raises(RuntimeError, match="stage"):
        dec.decode_staged()
    torch.cuda.synchronize()
    assert (flat.cpu().numpy() == 0xA5).all(), "a refused call wrote to its output"
    assert np.array_equal(dec.decode(files[:3], out=out).cpu().numpy(), np.stack([_ref(f) for f in files[:3]]))


def _write_preds(tmp_path, n, masks=None):
    from sfh_amd import outputs as O
    with O.CourtJsonWriter(str(tmp_path), "game", "model-x") as wr:
        for k in range(n):
            wr.add(str(k), score=(0.01, 0.5, 0.3)[k % 3], theta=np.eye(3, dtype=np.float32).reshape(1, 3, 3))
    mpath = None
    if masks is not None:
        with O.MaskPickleWriter(str(tmp_path), "mask") as mw:
            for k, m in enumerate(masks):
                mw.write(str(k), m)
        mpath = mw.path
    return os.path.join(str(tmp_path), "game_court.json"), mpath


def _same_files(a, b):
    assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] and len(a) >= 3
    for x, y in zip(a, b):
        assert open(x, "rb").read() == open(y, "rb").read(), os.path.basename(x)


def test_visualize_masks_decoded_on_the_device(tmp_path):
    from sfh_amd import synth
    from sfh_amd.visualize import visualize
    frames = list(synth.synth_frames_u8(3, 90, 112, seed=7))
    masks = np.random.default_rng(4).integers(0, 4, (3, 45, 56), dtype=np.uint8)
    masks[:, 10:30] = 2
    preds, mpath = _write_preds(tmp_path, 3, masks)
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    a = visualize(iter(frames), preds, str(tmp_path / "host"), court, masks_path=mpath, batch=2)
    b = visualize(iter(frames), preds, str(tmp_path / "device"), court, masks_path=mpath, batch=2, masks_decode="device")
    _same_files(a, b)
    with pytest.raises(ValueError, match="masks_decode"):
        visualize(iter(frames), preds, str(tmp_path / "bad"), court, masks_path=mpath, masks_decode="gpu")


def test_visualize_and_rectify_game_from_png_files(tmp_path):
    from sfh_amd import synth
    from sfh_amd.mapping import rectify_game
    from sfh_amd.outputs import encode_png
    from sfh_amd.visualize import visualize
    frames = list(synth.synth_frames_u8(3, 90, 112, seed=9))
    files = [encode_png(f).tobytes() for f in frames[:2]] + [PC.write_png(frames[2][:, :, ::-1], PC.pattern("cycle", 90))]
    preds, _ = _write_preds(tmp_path, 3)
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    for what, call in (("viz", lambda fr, dst, **kw: visualize(fr, preds, dst, court, batch=2, **kw)),
                       ("top", lambda fr, dst, **kw: rectify_game(preds, fr, dst, out_size=(160, 96), batch=2, **kw))):
        a = call(iter(frames), os.path.join(str(tmp_path), what + "_arrays"))
        b = call(iter(files), os.path.join(str(tmp_path), what + "_files"), frames_format="png")
        _same_files(a, b)
    gray = [PC.write_png(f[:, :, :1], PC.pattern("all1", 90)) for f in frames]
    with pytest.raises(ValueError, match="frames_format='png'"):
        visualize(iter(gray), preds, os.path.join(str(tmp_path), "bad"), court, frames_format="png")
    with pytest.raises(ValueError, match="frames_format"):
        visualize(iter(frames), preds, os.path.join(str(tmp_path), "bad"), court, frames_format="png")


def test_read_dataset_decodes_on_the_device(tmp_path):
    import prep_fixtures as F
    from sfh_amd import preparation as P
    court, ids = F.court_poi("pitch"), F.court_ids("pitch_v3_nc4_640x360")
    manual, _ = F.exact_annotations(court, F.fixture_thetas()[:4], seed=8, n_short=0)
    anno = tmp_path / "anno" / "game_a"
    os.makedirs(anno)
    with open(anno / "manual_anno.json", "w") as f:
        json.dump({f"{r:06d}": {"poi": manual[r].tolist(), "theta": None} for r in range(4)}, f)
    for png in ("host", "device"):                                               # zlib's files and sfh_amd.pngenc's
        dst = tmp_path / f"out_{png}"
        rep = P.prepare_dataset(str(tmp_path / "anno"), str(dst), ids, court, size=(188, 111), batch=4, png=png)
        want = P.read_dataset(str(dst), rep["written"], device="cuda")
        for size in (None, (100, 57)):
            got = P.read_dataset(str(dst), rep["written"], device="cuda", size=size, decode="device")
            ref = want if size is None else P.read_dataset(str(dst), rep["written"], device="cuda", size=size)
            assert sorted(got) == sorted(ref)
            for k in ref:
                assert got[k] == ref[k] if k == "name" else (got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k])), k
        assert want["mask_u8"].any()
    with pytest.raises(ValueError, match="decode"):
        P.read_dataset(str(dst), rep["written"], decode="device")               # the decode runs on the device
