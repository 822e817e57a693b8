"""CPU checks of the JPEG format rule: tests/jpegenc_ref.py (which the device encoder of sfh_amd.jpegenc must equal byte for byte)
against libjpeg's own bytes through PIL, the capacity bound, the refusals of the Python and C entry points and FramePipeline's
budget-overflow logic with JPEG files."""
import io

import numpy as np
import pytest
from PIL import Image

import jpegenc_cases as cases
import jpegenc_ref as R

_SMALL = cases.small_cases()
_TEMPLATES = cases.template_cases()
_ALL = {**_SMALL, **_TEMPLATES}


def _pil(img, quality, bgr=True, restart=True):
    kw = {"restart_marker_rows": 1} if restart else {}
    if img.ndim == 3:
        img, kw["subsampling"] = (img[:, :, ::-1] if bgr else img), 2
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def _shape3(img):
    return img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3


@pytest.mark.parametrize("name", list(_ALL))
def test_restatement_equals_pil_bytes_and_the_plain_file(name):
    """the pin: the whole file, header included, equals PIL's, for both channel orders; PIL decodes it, to the pixels of its
    own file without restart markers (what cv2.imwrite writes)"""
    img, q = _ALL[name]
    for bgr in ((True, False) if img.ndim == 3 and name in _SMALL else (True,)):
        ours = R.ref_encode(img, q, bgr=bgr)
        assert ours == _pil(img, q, bgr), name
        dec = Image.open(io.BytesIO(ours))
        dec.load()
        plain = Image.open(io.BytesIO(_pil(img, q, bgr, restart=False)))
        assert dec.size == (img.shape[1], img.shape[0]) and np.array_equal(np.array(dec), np.array(plain))
        assert len(ours) <= R.ref_capacity(*_shape3(img))


def test_outputs_pair_is_the_same_file():
    from sfh_amd.outputs import decode_jpeg, encode_jpeg
    for name in ("noise_37x50_rgb", "noise_37x50_gray", "checker_q25_rgb"):
        img, q = _SMALL[name]
        buf = encode_jpeg(img, q)
        assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.tobytes() == R.ref_encode(img, q)
        assert encode_jpeg(img, q, restart_rows=0).tobytes() == _pil(img, q, restart=False)
        dec = decode_jpeg(buf)
        assert dec.shape == img.shape and dec.dtype == np.uint8
        want = np.array(Image.open(io.BytesIO(buf.tobytes())))
        assert np.array_equal(dec, want if img.ndim == 2 else want[:, :, ::-1])
    with pytest.raises(ValueError):
        encode_jpeg(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError):
        encode_jpeg(np.zeros((4, 4), np.uint8), quality=0)
    with pytest.raises(ValueError):
        encode_jpeg(np.zeros((4, 4, 2), np.uint8))


def test_quant_tables_and_header_layout():
    assert R.quant_table(R.BASE_LUMA, 90)[:8].tolist() == [3, 2, 2, 3, 5, 8, 10, 12]
    assert (R.quant_table(R.BASE_LUMA, 100) == 1).all() and R.quant_table(R.BASE_CHROMA, 1).max() == 255
    assert np.array_equal(R.quant_table(R.BASE_LUMA, 50), R.BASE_LUMA)
    h = R.header(37, 50, 3, 90)
    marks, pos = [], 2
    while pos < len(h):
        marks.append(h[pos + 1])
        pos += 2 + int.from_bytes(h[pos + 2:pos + 4], "big")
    assert h[:2] == b"\xff\xd8" and marks == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert len(h) == 629 and len(R.header(37, 50, 1, 90)) == 334


def _symbols(img, q):
    """(DC categories, AC symbols per block) of the restatement's coefficients, for the cases that claim a branch"""
    planes = R.ycc_planes(img)
    out = []
    for i, p in enumerate(planes):
        c = R.quantised_blocks(p, R.quant_table(R.BASE_LUMA if i == 0 else R.BASE_CHROMA, q))
        out.append(c.reshape(-1, 64))
    return out


def test_the_edge_cases_reach_their_branches():
    # 8x8 blocks alternating 0 and 255 at quality 100: DC -1024 / +1016, differences of category 11
    y = _symbols(*_SMALL["blocks0_255_q100_gray"])[0]
    assert np.abs(np.diff(y[:10, 0])).max() >= 1024
    # its lower half, shifted by half a block: AC coefficients of the largest category, 10
    assert np.abs(y[:, 1:]).max() >= 512
    # the one-pixel checkerboard at quality 25 keeps enough of its odd-odd frequencies that no run of zeros reaches 16: it codes
    # no ZRL at all (the stated deviation from the issue's wording).  The single cosines: ZRL once, twice, three times in a block
    def zrls(name):
        out = set()
        for blk in _symbols(*_SMALL[name])[0]:
            nz = np.flatnonzero(blk[1:]) + 1
            out |= {int(g - 1) // 16 for g in np.diff(np.concatenate([[0], nz]))}
        return out

    assert zrls("checker_q25_gray") == {0}
    assert 1 in zrls("cosine_zz20_q25_gray") and 2 in zrls("cosine_zz40_q25_gray") and 3 in zrls("cosine_zz63_q25_gray")
    # coefficient 63 survives: no EOB
    assert (_symbols(*_SMALL["last_ac_q100_gray"])[0][:, 63] != 0).any()
    # constant: after the first block every block is difference 0 and EOB (2 + 4 bits luma)
    bits = R.interval_bits(_SMALL["constant_gray"][0])[0]
    assert set(bits[1:]) == {"00" + "1010"}
    # noise makes 0xFF bytes to stuff; 160 rows wrap the RSTm counter past 7
    f = R.ref_encode(*_SMALL["noise_160x48_gray"])
    assert b"\xff\x00" in f and all(bytes([0xFF, 0xD0 + m]) in f for m in range(8)) and f.count(b"\xff\xd7") >= 2
    # half an MCU: dummy blocks code as difference 0 + EOB
    assert "001010" in R.interval_bits(_SMALL["noise_24x16_rgb"][0])[1]


def test_capacity_bound():
    from sfh_amd import _lib
    lib = _lib.load()
    for img, _ in _ALL.values():
        assert lib.sfh_jpeg_capacity(*_shape3(img)) == R.ref_capacity(*_shape3(img))
    # one full-width interval of noise at quality 100 stays below the bound (and above the raw size: 16 * 1280 * 3 = 61,440 raw)
    img = _SMALL["noise_16x1280_rgb"][0]
    n = len(R.ref_encode(img, 100))
    print("16x1280 noise at quality 100:", n, "bytes, capacity", R.ref_capacity(16, 1280, 3))
    assert 30000 < n <= R.ref_capacity(16, 1280, 3)
    # the bound per block: no block of the adversarial cases is longer than BLOCK_MAX_BITS
    for name in ("blocks0_255_q100_rgb", "last_ac_q100_rgb", "checker_q25_rgb", "noise_37x50_q100_rgb"):
        img, q = _SMALL[name]
        longest = max(len(b) for row in R.interval_bits(img, q) for b in row)
        print(name, "longest block", longest, "bits")
        assert longest <= R.BLOCK_MAX_BITS
    assert R.ref_capacity(1, 1, 1) == 334 + 2 * ((R.BLOCK_MAX_BITS + 7) // 8) + 2
    # the longest codes of the tables are what the bound assumes
    assert max(l for _, l in R.HUFF[("ac", 0)].values()) == 16 and max(l for _, l in R.HUFF[("ac", 1)].values()) == 16
    assert max(l for _, l in R.HUFF[("dc", 0)].values()) == 9 and max(l for _, l in R.HUFF[("dc", 1)].values()) == 11


def test_refusals():
    import torch
    from sfh_amd import _lib, jpegenc
    lib = _lib.load()
    for bad in ((4, 2049, 1), (4, 2049, 3), (4, 4, 2), (4, 4, 4), (0, 4, 1), (65536, 4, 1)):
        with pytest.raises(ValueError):
            jpegenc.jpeg_capacity(*bad)
        assert lib.sfh_jpeg_capacity(*bad) == -1
        with pytest.raises(ValueError):
            R.ref_capacity(*bad)
    assert jpegenc.jpeg_capacity(4, 2048, 3) == R.ref_capacity(4, 2048, 3)
    with pytest.raises(ValueError):
        R.ref_encode(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError):
        R.ref_encode(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        R.ref_encode(np.zeros((4, 4), np.uint8), quality=101)
    with pytest.raises(ValueError):
        jpegenc.encode_jpeg_device(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        jpegenc.encode_jpeg_device(torch.zeros((2, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        jpegenc.encode_jpeg_device(torch.zeros((4, 2049, 3), dtype=torch.uint8))
    for q in (0, 101, 89.5, True):
        with pytest.raises(ValueError):
            jpegenc.JpegEncoder(8, 8, 3, 1, quality=q)
    with pytest.raises(ValueError):
        jpegenc.JpegEncoder(8, 8, 2, 1)
    with pytest.raises(ValueError):
        jpegenc.JpegEncoder(720, 1280, 3, 4096)                               # 2 GiB or more
    with pytest.raises(ValueError):
        jpegenc.jpeg_files_from_batch(np.zeros((1, 4, 4), np.uint8), 1, "gpu")
    with pytest.raises(ValueError):
        jpegenc.image_files_from_batch(np.zeros((1, 4, 4), np.uint8), 1, "host", image_format="bmp")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpegenc.jpeg_files_from_batch(np.zeros((1, 4, 4, 3), np.uint8), 3, "device")
    # type, dtype, shape and contiguity are refused wherever the tensor lies, before anything touches a device; only a
    # well-formed tensor gets as far as the device check
    enc = jpegenc.JpegEncoder.__new__(jpegenc.JpegEncoder)
    enc.H, enc.W, enc.C, enc.B = 8, 8, 3, 2
    good = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="tensor"):
        enc._checked(good.numpy())
    with pytest.raises(ValueError, match="dtype"):
        enc._checked(good.to(torch.int16))
    for bad in (good[0], good[:, :, :7], good[:, :7], good[:, :, :, :1], torch.zeros((3, 8, 8, 3), dtype=torch.uint8),
                torch.zeros((0, 8, 8, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="expected"):
            enc._checked(bad)
    strided = torch.zeros((2, 8, 16, 3), dtype=torch.uint8)[:, :, ::2]
    transposed = torch.zeros((2, 8, 8, 3), dtype=torch.uint8).transpose(1, 2)
    assert strided.shape == transposed.shape == good.shape
    for bad in (strided, transposed):
        with pytest.raises(ValueError, match="contiguous"):
            enc._checked(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc._checked(good)
    enc.C = 1                                                                 # gray: (b,H,W) or (b,H,W,1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc._checked(good[:, :, :, :1].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        enc._checked(good[:, :, :, 0])
    with pytest.raises(ValueError, match="expected"):
        enc._checked(good)
    # the C entry points: argument checks fire before anything touches a device
    assert lib.sfh_jpeg_encode(None, 1, 4, 2049, 1, 1, 90, None, 0, 0, None) == -1 and b"width" in lib.sfh_last_error()
    assert lib.sfh_jpeg_encode(None, 1, 4, 4, 2, 1, 90, None, 0, 0, None) == -1 and b"channels" in lib.sfh_last_error()
    assert lib.sfh_jpeg_encode(None, 1, 4, 4, 1, 1, 0, None, 0, 0, None) == -1 and b"quality" in lib.sfh_last_error()
    assert lib.sfh_jpeg_encode(None, 1, 4, 4, 1, 1, 90, None, 0, 0, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_jpeg_encode(None, 4096, 720, 1280, 3, 1, 90, None, 0, 0, None) == -1 and b"2 GiB" in lib.sfh_last_error()
    assert lib.sfh_jpeg_pack(None, 0, 1, 4, 4, 4, 90, 1, None, 0, None, None, None) == -1
    assert lib.sfh_jpeg_pack(None, 0, 0, 4, 4, 1, 90, 1, None, 0, None, None, None) == -1
    with pytest.raises(ValueError):
        _lib.check(lib.sfh_jpeg_pack(None, 0, 1, 4, 4, 1, 90, 1, None, 0, None, None, None), "jpeg_pack")


def test_host_leg_of_the_drivers_switch():
    from sfh_amd.jpegenc import image_files_from_batch
    from sfh_amd.outputs import encode_png
    img = _SMALL["noise_37x50_rgb"][0]
    imgs = np.stack([img, cases.variant(img, 1)])
    files, ext = image_files_from_batch(imgs, 3, "host", "jpeg", 75)
    assert ext == "jpeg" and [f.tobytes() for f in files] == [R.ref_encode(i, 75) for i in imgs]
    files, ext = image_files_from_batch(imgs, 3, "host")
    assert ext == "png" and all(np.array_equal(f, encode_png(i)) for f, i in zip(files, imgs))      # today's bytes


def test_pipeline_budget_overflow_branch_with_jpeg_files():
    from sfh_amd.pipeline import png_files_from_head, png_head_bytes
    img, q = _SMALL["noise_37x50_rgb"]
    files = [np.frombuffer(R.ref_encode(cases.variant(img, k), q), np.uint8) for k in range(3)]
    data = np.concatenate(files)
    sizes = np.array([f.size for f in files], np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total, hb = int(offsets[-1]), png_head_bytes(3)
    calls = []

    def fetch(a, e):
        calls.append((a, e))
        return data[a:e]

    for budget in (total + 100, total, total - 1, files[0].size + 7, 64, 0):
        head = np.zeros(hb + budget, np.uint8)
        head[:32] = offsets.view(np.uint8)
        head[32:44] = sizes.view(np.uint8)
        head[hb:hb + min(budget, total)] = data[:min(budget, total)]
        calls.clear()
        got = png_files_from_head(head, 3, budget, fetch)
        assert calls == ([] if budget >= total else [(budget, total)])
        assert len(got) == 3 and all(np.array_equal(g, f) for g, f in zip(got, files))


def test_pipeline_arguments_are_opt_in():
    import inspect
    from sfh_amd import pipeline
    assert pipeline.JPEG_OUTPUTS == ("overlay", "top_view")
    sig = inspect.signature(pipeline.FramePipeline.__init__).parameters
    assert sig["jpeg"].default is None and sig["jpeg_quality"].default == 90 and sig["jpeg_budget"].default is None
    assert sig["png"].default is None and sig["png_budget"].default is None      # the defaults stay what they are
