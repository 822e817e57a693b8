"""sfh_amd.tiffdec / sfh_amd.tiffenc on the MI355X: the device decoder against the source arrays of tests/tiff_cases.py (whose
strips are libtiff's), the device encoder against outputs.encode_tiff byte for byte, and the ``uv_format=`` / ``tif=`` switches of
prepare_dataset / read_dataset against the ``.npy`` route.  Only well-formed files are decoded here: corrupt streams go through
the stand-alone host program of tests/test_tiff_host.py."""
import json
import os

import numpy as np
import pytest
import torch

import tiff_cases as tc

pytestmark = pytest.mark.gpu

GUARD = 64
CASES = tc.cases()
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault((_c.H, _c.W, _c.C, _c.bits), []).append(_c)
GROUP_IDS = ["x".join(map(str, k)) for k in GROUPS]


def _np_dtype(bits):
    return np.uint16 if bits == 16 else np.uint8


def _device(a):
    """a uint8 / uint16 host array -> the GPU (uint16 through int16: few operators know uint16)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to("cuda").view(torch.uint16)
    return torch.from_numpy(a).to("cuda")


def _host(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def _guarded(shape, bits, fill):
    """an output that starts as a sentinel, with GUARD elements behind it -> (flat buffer, view to decode into)"""
    numel = int(np.prod(shape))
    flat = _device(np.full(numel + GUARD, fill, dtype=_np_dtype(bits)))
    return flat, flat[:numel].view(shape)


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
@pytest.mark.parametrize("bgr", (True, False))
def test_decode_equals_the_source(key, bgr):
    """every case, in batches that mix contents, byte orders, predictors, compressions and strip sizes"""
    from sfh_amd.tiffdec import TiffDecoder
    H, W, C, bits = key
    group = GROUPS[key]
    want = np.stack([c.expected(bgr) for c in group])
    fill = 0xA5A5 if bits == 16 else 0xA5
    dec = TiffDecoder(H, W, C, bits, batch=len(group), bgr=bgr, max_file_bytes=max(len(c.file) for c in group))
    flat, out = _guarded(want.shape, bits, fill)
    got = dec.decode([c.file for c in group], out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == want.shape
    assert dec.status.tolist() == [0] * len(group)
    host = _host(flat)
    assert np.array_equal(host[:want.size].reshape(want.shape), want)
    assert (host[want.size:] == fill).all(), "guard elements behind the output were written"
    again = dec.decode([np.frombuffer(c.file, np.uint8) for c in group])       # the decoder's own buffer: the same bits
    assert np.array_equal(_host(again), want) and not dec.status.any()


def test_out_and_partial_batches():
    from sfh_amd.tiffdec import TiffDecoder, decode_tiff_device
    group = GROUPS[(37, 53, 3, 16)]
    files = [c.file for c in group]
    want = np.stack([c.expected(True) for c in group])
    dec = TiffDecoder(37, 53, batch=len(files))
    assert dec.out.dtype == torch.uint16 and tuple(dec.out.shape) == (len(files), 37, 53, 3)
    part = dec.decode(files[:3])
    assert tuple(part.shape) == (3, 37, 53, 3) and np.array_equal(_host(part), want[:3]) and dec.status.tolist() == [0, 0, 0]
    flat, out = _guarded((5, 37, 53, 3), 16, 0x5A5A)                          # more images than files: the rest is untouched
    dec.decode(files[:2], out=out)
    host = _host(flat)
    assert np.array_equal(host[:want[:2].size].reshape(want[:2].shape), want[:2]) and (host[want[:2].size:] == 0x5A5A).all()
    with pytest.raises(ValueError, match="uint16 only"):
        dec.decode(files[:1], out=torch.empty((1, 37, 53, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        dec.decode(files[:2], out=out[:1])
    with pytest.raises(ValueError, match="files"):
        dec.decode(files + files[:1])
    one = decode_tiff_device(files[0])
    assert tuple(one.shape) == (37, 53, 3) and np.array_equal(_host(one), want[0])
    gray = GROUPS[(37, 53, 1, 8)]
    many = decode_tiff_device([c.file for c in gray], bgr=False)
    assert many.dtype == torch.uint8 and np.array_equal(_host(many), np.stack([c.expected(False) for c in gray]))


def test_refusals_leave_the_output_untouched():
    from sfh_amd.tiffdec import TiffDecoder
    good = tc.Case("good", tc.uv_label(6, 5), rps=4, predictor=2)
    dec = TiffDecoder(6, 5, batch=2)
    flat, out = _guarded((2, 6, 5, 3), 16, 0x1234)
    for name, data, reason in tc.refusals():
        with pytest.raises(NotImplementedError if reason >= 100 else ValueError, match=r"\(file 1\)"):
            dec.decode([good.file, data], out=out)
    other = tc.Case("other", tc.uv_label(6, 4), rps=4)
    with pytest.raises(ValueError, match="other than the decoder's"):
        dec.decode([other.file], out=out)
    small = TiffDecoder(6, 5, batch=1, max_file_bytes=len(good.file) - 1)
    with pytest.raises(ValueError, match="max_file_bytes"):
        small.decode([good.file], out=out)
    assert (_host(flat) == 0x1234).all()
    dec.decode([good.file, good.file], out=out)                                # and the decoder still works
    assert np.array_equal(_host(out)[1], good.expected(True)) and not dec.status.any()


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_encode_equals_the_rule_and_round_trips(key):
    from sfh_amd.outputs import encode_tiff
    from sfh_amd.tiffdec import TiffDecoder
    from sfh_amd.tiffenc import TiffBatch, TiffEncoder
    H, W, C, bits = key
    kinds = {}
    for c in GROUPS[key]:
        kinds.setdefault((c.compression, c.predictor, c.rps), []).append(c)
    for (comp, pred, rps), group in kinds.items():
        comp = "lzw" if comp == 5 else "none"
        for bgr in ((True, False) if C == 3 else (True,)):
            imgs = np.stack([c.expected(bgr) for c in group])
            want = [encode_tiff(c.expected(bgr), comp, pred, rps, bgr=bgr) for c in group]
            enc = TiffEncoder(H, W, C, bits, batch=len(group), bgr=bgr, compression=comp, predictor=pred, rows_per_strip=rps)
            assert all(len(w) <= enc.capacity for w in want)
            data = torch.full((len(group) * enc.capacity + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            out = TiffBatch(data, torch.empty(len(group) + 1, dtype=torch.int64, device="cuda"),
                            torch.empty(len(group), dtype=torch.int32, device="cuda"))
            x = _device(imgs)
            batch = enc.encode(x, out=out)
            files = batch.to_host()
            assert [len(f) for f in files] == [len(w) for w in want]
            for f, w, c in zip(files, want, group):
                assert np.array_equal(f, w), c.name
            end = int(batch.offsets[-1])
            assert end == sum(len(w) for w in want) and (data[end:].cpu().numpy() == 0xA5).all(), "bytes behind the files were written"
            dec = TiffDecoder(H, W, C, bits, batch=len(group), bgr=bgr, max_file_bytes=enc.capacity)
            assert np.array_equal(_host(dec.decode(batch)), imgs) and not dec.status.any()
            assert [np.array_equal(f, w) for f, w in zip(enc.encode(x).to_host(), want)] == [True] * len(want)   # its own buffers


def test_encoder_refusals_and_one_off():
    from sfh_amd.outputs import encode_tiff
    from sfh_amd.tiffenc import TiffEncoder, encode_tiff_device
    lab = tc.uv_label(45, 80)[:, :, ::-1].copy()
    assert np.array_equal(encode_tiff_device(_device(lab)), encode_tiff(lab))
    gray = tc.random_image(9, 31, 1, 8, 3)[:, :, 0]
    files = encode_tiff_device(_device(np.stack([gray, gray[::-1]])), compression="none")
    assert np.array_equal(files[1], encode_tiff(gray[::-1], "none"))
    enc = TiffEncoder(45, 80, batch=2)
    with pytest.raises(ValueError, match="uint16 only"):
        enc.encode(torch.zeros((1, 45, 80, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        enc.encode(_device(np.zeros((3, 45, 80, 3), np.uint16)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.from_numpy(np.zeros((1, 45, 80, 3), np.int16)).view(torch.uint16))
    with pytest.raises(ValueError):
        TiffEncoder(45, 80, bits=12)
    with pytest.raises(ValueError):
        TiffEncoder(45, 80, rows_per_strip=46)


def test_dataset_round_trip_through_tif(tmp_path):
    """prepare_dataset writes <frame>.tif on the device; read_dataset reads it on the device and on the host: the .npy route's
    batch bit for bit, also with size="""
    import prep_fixtures as F
    from sfh_amd import outputs as O
    from sfh_amd import preparation as P
    court, ids = F.court_poi("pitch"), F.court_ids("pitch_v3_nc4_640x360")
    manual, _ = F.exact_annotations(court, F.fixture_thetas()[:2], seed=8, n_short=0)
    anno = tmp_path / "anno" / "game_a"
    os.makedirs(anno)
    with open(anno / "manual_anno.json", "w") as f:
        json.dump({f"{r:06d}": {"poi": manual[r].tolist(), "theta": None} for r in range(2)}, f)
    dst = tmp_path / "out"
    rep = P.prepare_dataset(str(tmp_path / "anno"), str(dst), ids, court, size=(188, 111), batch=2, uv=True, uv_format="both",
                            tif="device")
    assert sorted(os.listdir(dst / "game_a")) == [f"{r:06d}{e}" for r in range(2) for e in (".json", ".npy", ".png", ".tif")]
    for key in rep["written"]:
        lab = np.load(dst / (key + ".npy"))
        tif = np.fromfile(dst / (key + ".tif"), dtype=np.uint8)
        assert np.array_equal(tif, O.encode_tiff(lab)) and np.array_equal(O.decode_tiff(tif), lab)
        assert np.array_equal(O.decode_tiff(tif, bgr=False)[:, :, 2], lab[:, :, 0])      # the id is the file's third sample
    host_dst = tmp_path / "out_host"
    P.prepare_dataset(str(tmp_path / "anno"), str(host_dst), ids, court, size=(188, 111), batch=2, uv=True, uv_format="tif")
    assert sorted(os.listdir(host_dst / "game_a")) == [f"{r:06d}{e}" for r in range(2) for e in (".json", ".png", ".tif")]
    assert (host_dst / "game_a" / "000001.tif").read_bytes() == (dst / "game_a" / "000001.tif").read_bytes()
    for size in (None, (100, 57)):
        want = P.read_dataset(str(dst), rep["written"], use_uv=True, device="cuda", size=size)
        assert want["uv"].any() and want["mask_u8"].any()
        for decode in ("device", "host"):
            got = P.read_dataset(str(dst), rep["written"], use_uv=True, device="cuda", size=size, uv_format="tif", decode=decode)
            assert sorted(got) == sorted(want)
            for k in want:
                same = got[k] == want[k] if k == "name" else (got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]))
                assert same, (size, decode, k)
    with pytest.raises(ValueError, match="uv_format"):
        P.read_dataset(str(dst), rep["written"], use_uv=True, uv_format="tiff")
