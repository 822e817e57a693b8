"""CPU checks of the PNG format rule (tests/pngenc_ref.py, which the device encoder of sfh_amd.pngenc must equal byte for
byte), of the refusals of the C entry points and of FramePipeline's budget-overflow logic."""
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest

import pngenc_cases as cases
import pngenc_ref as R
from conftest import ROOT

_SMALL = cases.small_cases()
_TEMPLATES = cases.template_cases()
_ALL = {**_SMALL, **_TEMPLATES}

# IDAT bytes of the rule over IDAT bytes of zlib level 1 with filter 0 (outputs.encode_png) on the packaged templates: the
# figures of the issue's CPU prototype.  A property of the rule, not of a machine.
SIZE_RATIOS = {"ncaa_nc4_1280x720_gray": 1.76, "ncaa_nc4_1280x720_rgb": 1.33, "ncaa_nc4_640x360_gray": 1.86,
               "ncaa_nc4_640x360_rgb": 1.49, "pitch_v3_nc4_1280x720_gray": 1.78, "pitch_v3_nc4_1280x720_rgb": 1.34,
               "pitch_v3_nc4_640x360_gray": 2.18, "pitch_v3_nc4_640x360_rgb": 1.63}


def _chunks(buf):
    data = bytes(buf)
    assert data[:8] == R.SIG
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) & 0xFFFFFFFF == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        out.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def _shape3(img):
    return img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3


@pytest.mark.parametrize("name", list(_ALL))
def test_round_trip_stream_and_size(name):
    from PIL import Image
    from sfh_amd.outputs import decode_png
    img = _ALL[name]
    H, W, C = _shape3(img)
    buf, kinds = R.ref_encode_parts(img)
    # two independent decoders
    pil = np.array(Image.open(io.BytesIO(buf)))
    assert np.array_equal(pil, img if C == 1 else img[:, :, ::-1])             # PIL gives RGB, the array is BGR
    assert np.array_equal(decode_png(np.frombuffer(buf, np.uint8)), img)      # verifies every chunk CRC
    # the stream: one IDAT per strip, joined bodies inflate to the Sub-filtered scanlines
    ch = _chunks(buf)
    idat = [b for t, b in ch if t == b"IDAT"]
    nstrips = -(-H // R.strip_rows(W, C))
    assert [t for t, _ in ch] == [b"IHDR"] + [b"IDAT"] * nstrips + [b"IEND"] and len(kinds) == nstrips
    assert idat[0][:2] == b"\x78\x01"
    assert zlib.decompress(b"".join(idat)) == R.filtered_stream(img).tobytes()
    assert len(buf) <= R.ref_capacity(H, W, C)


def test_capacity_is_reached_by_noise_and_matches_the_library():
    from sfh_amd import _lib
    lib = _lib.load()
    for name in ("noise", "noise_rgb"):
        img = _SMALL[name]
        buf, kinds = R.ref_encode_parts(img)
        assert set(kinds) == {"stored"} and len(buf) == R.ref_capacity(*_shape3(img))
    for img in _ALL.values():
        assert lib.sfh_png_capacity(*_shape3(img)) == R.ref_capacity(*_shape3(img))
    assert R.ref_capacity(1, 1, 1) == 8 + 25 + 12 + 17 + 2 + 6


def test_branches_and_tokens_of_the_edge_cases():
    # exact run lengths: n equal bytes = a literal + the matches of n - 1 + at most two literals
    toks = R.strip_tokens(R.filtered_stream(cases.runs_image())[0])
    m = [v for k, v in toks if k == "match"]
    # runs 2, 3: literals only; 4 -> 3; 258 -> 257; 259 -> 258; 260 -> 258 + literal; 261 -> 258 + 2 literals;
    # 517 -> 258 + 258
    assert m == [3, 257, 258, 258, 258, 258, 258]
    assert [v for k, v in toks if k == "lit"].count(5) == 2 + 3 + 1 + 1 + 1 + 2 + 3 + 1
    # strips alternate between the stored and the fixed form
    assert R.ref_encode_parts(_SMALL["alternating"])[1] == ["stored", "fixed", "stored", "fixed", "stored"]
    assert set(R.ref_encode_parts(_SMALL["constant"])[1]) == {"fixed"}
    # a run over every row end of a strip, stopping at the strip's end: one literal and matches per strip
    ramp = R.filtered_stream(_SMALL["ramp_run_over_rows"])
    assert (ramp == 1).all()
    toks = R.strip_tokens(ramp[:16].reshape(-1))
    assert toks == [("lit", 1)] + [("match", 258)] * 18 + [("match", 16 * 301 - 1 - 18 * 258)]      # 4815 = 18 * 258 + 171
    # every byte value occurs as a literal: both literal code lengths
    lits = {v for k, v in R.strip_tokens(R.filtered_stream(_SMALL["all_literals"])[0]) if k == "lit"}
    assert lits == set(range(256))
    # strip heights: below 16 for wide rows, a last strip that is shorter
    assert R.strip_rows(3000, 1) == 10 and R.strip_rows(1100, 3) == 9 and R.strip_rows(333, 1) == 16
    assert R.strip_rows(32767, 1) == 1 and 187 % 16 != 0


def test_template_sizes_against_zlib_level_1():
    """records the ratios in profiles/pngenc_size.jsonl when SFH_WRITE_PROFILES is set; asserts them always"""
    from sfh_amd.outputs import encode_png
    rows = []
    for name, want in SIZE_RATIOS.items():
        img = _TEMPLATES[name]
        ours = sum(len(b) for t, b in _chunks(R.ref_encode(img)) if t == b"IDAT")
        zl = sum(len(b) for t, b in _chunks(encode_png(img, level=1)) if t == b"IDAT")
        ratio = ours / zl
        rows.append({"image": name, "idat_bytes": ours, "zlib1_idat_bytes": zl, "ratio": round(ratio, 4),
                     "raw_over_ours": round(img.size / ours, 2)})
        print(rows[-1])
        assert abs(ratio - want) <= 0.10 * want, f"{name}: {ours} / {zl} = {ratio:.3f}, issue table {want}"
    if os.environ.get("SFH_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "pngenc_size.jsonl"), "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def test_refusals():
    import torch
    from sfh_amd import _lib, pngenc
    lib = _lib.load()
    for bad in ((4, 32768, 1), (4, 10923, 3), (4, 4, 2), (4, 4, 4), (0, 4, 1)):
        with pytest.raises(ValueError):
            pngenc.png_capacity(*bad)
        assert lib.sfh_png_capacity(*bad) == -1
        with pytest.raises(ValueError):
            R.ref_capacity(*bad)
    assert pngenc.png_capacity(4, 32767, 1) == R.ref_capacity(4, 32767, 1)
    with pytest.raises(ValueError):
        R.ref_encode(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError):
        R.ref_encode(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        pngenc.encode_png_device(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        pngenc.encode_png_device(torch.zeros((2, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        pngenc.files_from_batch(np.zeros((1, 4, 4), np.uint8), 1, png="gpu")
    # the C entry points: argument checks fire before anything touches a device
    assert lib.sfh_png_encode(None, 1, 4, 32768, 1, 1, None, 0, None) == -1 and b"scanline" in lib.sfh_last_error()
    assert lib.sfh_png_encode(None, 1, 4, 4, 2, 1, None, 0, None) == -1 and b"channels" in lib.sfh_last_error()
    assert lib.sfh_png_encode(None, 1, 4, 4, 1, 1, None, 0, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_png_pack(None, 0, 1, 4, 4, 4, 1, None, 0, None, None, None) == -1
    assert lib.sfh_png_pack(None, 0, 0, 4, 4, 1, 1, None, 0, None, None, None) == -1
    with pytest.raises(ValueError):
        _lib.check(lib.sfh_png_pack(None, 0, 1, 4, 4, 1, 1, None, 0, None, None, None), "png_pack")


def test_host_switch_keeps_todays_bytes():
    from sfh_amd.outputs import encode_png
    from sfh_amd.pngenc import files_from_batch
    imgs = np.stack([_SMALL["7x5_rgb"], cases.variant(_SMALL["7x5_rgb"], 1)])
    got = files_from_batch(imgs, 3, "host")
    assert all(np.array_equal(g, encode_png(i)) for g, i in zip(got, imgs))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        files_from_batch(imgs, 3, "device")


def test_write_encoded_stream(tmp_path):
    from sfh_amd.outputs import MaskPickleWriter, MaskReader
    masks = [_SMALL["7x5"], _SMALL["63x40"]]
    with MaskPickleWriter(str(tmp_path)) as wr:
        wr.write_encoded("a", np.frombuffer(R.ref_encode(masks[0]), np.uint8))
        wr.write_encoded("b", R.ref_encode(masks[1]))
        wr.write("c", masks[0])
        with pytest.raises(ValueError):
            wr.write_encoded("d", np.zeros(20, np.uint8))
    got = list(MaskReader(os.path.join(str(tmp_path), "mask", "data.pkl")).get(decode=True))
    assert [n for n, _ in got] == ["a", "b", "c"]
    assert all(np.array_equal(m, w) for (_, m), w in zip(got, masks + [masks[0]]))


def _head(files, batch, budget):
    """what FramePipeline downloads first: offsets, sizes and the first `budget` bytes of the files laid back to back"""
    from sfh_amd.pipeline import png_head_bytes
    data = np.concatenate(files)
    sizes = np.array([f.size for f in files], np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    head = np.zeros(png_head_bytes(batch) + budget, np.uint8)
    head[:8 * (batch + 1)] = offsets.view(np.uint8)
    head[8 * (batch + 1):8 * (batch + 1) + 4 * batch] = sizes.view(np.uint8)
    n = min(budget, data.size)
    head[png_head_bytes(batch):png_head_bytes(batch) + n] = data[:n]
    return head, data


def test_pipeline_budget_overflow_branch():
    from sfh_amd.pipeline import png_files_from_head
    files = [np.frombuffer(R.ref_encode(cases.variant(_SMALL["63x40"], k)), np.uint8) for k in range(3)]
    total = sum(f.size for f in files)
    calls = []

    def fetch(a, e):
        calls.append((a, e))
        return data[a:e]

    # inside the budget (also exactly at it): no further copy
    for budget in (total + 100, total):
        head, data = _head(files, 3, budget)
        got = png_files_from_head(head, 3, budget, fetch)
        assert calls == [] and all(np.array_equal(g, f) for g, f in zip(got, files))
    # beyond it: exactly one fetch of [budget, offsets[B]), also when the cut falls inside the first file or at 0
    for budget in (total - 1, files[0].size + 7, 5, 0):
        calls.clear()
        head, data = _head(files, 3, budget)
        got = png_files_from_head(head, 3, budget, fetch)
        assert calls == [(budget, total)]
        assert len(got) == 3 and all(np.array_equal(g, f) for g, f in zip(got, files))
    head, data = _head(files, 3, 5)
    with pytest.raises(RuntimeError):
        png_files_from_head(head, 3, 5, lambda a, e: data[a:e - 1])
