"""CPU-side pins of sfh_amd.pngdec: outputs.decode_png - the pixels the device must give - equals PIL's on every case PIL opens;
the library's host parse equals a restated parse field by field; every refusal fires without a device; the decode core
(csrc/pngdec_core.h), built as a stand-alone program under the address and undefined-behaviour sanitizers, gives zlib's filtered
stream, decode_png's pixels and the expected acceptance decision on well-formed files, and a clean run on corrupt ones.
All comparisons are equality."""
import struct
import subprocess
import zlib
import io

import numpy as np
import pytest
from PIL import Image

import pngdec_cases as PC
from host_program import build_host_program

FILES = PC.all_files()
NAMES = sorted(FILES)

R_TRUNCATED, R_NOT_PNG, R_CRC, R_BAD_IHDR, R_IDAT_ORDER, R_NO_IDAT, R_NO_IEND, R_ZLIB, R_ZLIB_DICT, R_CRITICAL, R_SIZE, R_TOO_LONG = range(1, 13)
R_BIT_DEPTH, R_PALETTE, R_GRAY_ALPHA, R_INTERLACE, R_APNG = range(100, 105)


def _file_order(px):
    """decode_png's BGR(A) -> the file's RGB(A)"""
    if px.ndim == 2:
        return px
    return np.ascontiguousarray(px[:, :, [2, 1, 0] + ([3] if px.shape[2] == 4 else [])])


@pytest.mark.parametrize("name", NAMES)
def test_decode_png_equals_pil(name):
    from sfh_amd.outputs import decode_png
    data = FILES[name].data
    got = decode_png(np.frombuffer(data, np.uint8))
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode in ("L", "RGB", "RGBA")
        want = np.array(im)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(_file_order(got), want)


def test_case_list_covers_what_it_names():
    from sfh_amd.pngdec import parse_png
    parses = {n: parse_png(c.data) for n, c in PC.cases().items()}
    assert {(p["height"], p["width"]) for p in parses.values()} >= set(PC.SHAPES)
    assert {p["channels"] for p in parses.values()} == {1, 3, 4}
    for pat in PC.PATTERNS:
        for C in (1, 3, 4):
            filt = np.frombuffer(PC.expected_filtered(PC.cases()[f"pattern_37x50x{C}_{pat}"].data), np.uint8).reshape(37, -1)[:, 0]
            assert list(filt) == PC.pattern(pat, 37)
            assert (filt.max() <= 1) == (pat in PC.ROWS_KERNEL)
    assert max(p["nidat"] for p in parses.values()) > 1024          # more chunks than the segmented leg takes
    assert any(c.segmented for c in FILES.values()) and any(p["nidat"] > 1 and not FILES[n].segmented for n, p in parses.items())
    # the block types the recipes name
    def first_btype(name):
        return (PC.joined_idat(FILES[name].data)[2] >> 1) & 3
    assert [first_btype(f"recipe_{r}_333x187x3") for r in ("stored", "fixed", "dynamic")] == [0, 1, 2]
    assert len(PC.joined_idat(FILES["recipe_small_blocks_noisy_333x187x1"].data)) > 10000 and first_btype("recipe_small_blocks_noisy_333x187x1") == 2
    assert parses["recipe_window512_37x50x1"]["cmf"] == 0x18
    # the three fixtures: what the issue's table says of them
    fx = {n: parse_png(PC.fixture(n)) for n in PC.FIXTURES}
    assert [(fx[n]["width"], fx[n]["height"], fx[n]["channels"]) for n in PC.FIXTURES] == [(3421, 1819, 1), (1280, 720, 4), (2539, 1350, 3)]
    assert fx[PC.FIXTURES[0]]["nidat"] >= 7 and fx[PC.FIXTURES[1]]["nidat"] == 1 and fx[PC.FIXTURES[2]]["nidat"] > 1


# ------------------------------------------------------------------------------------------------------------ the parse

class Refused(Exception):
    def __init__(self, reason):
        super().__init__(f"reason {reason}")
        self.reason = reason


def ref_parse(data):
    """the rule of sfh_png_parse, restated"""
    data = bytes(data)
    if len(data) < 8:
        raise Refused(R_TRUNCATED if PC.SIG.startswith(data) else R_NOT_PNG)
    if data[:8] != PC.SIG:
        raise Refused(R_NOT_PNG)
    pos, hdr, later, idat, closed, end = 8, None, 0, [], False, False
    while not end:
        short = R_NO_IEND if hdr else R_TRUNCATED
        if len(data) - pos < 12:
            raise Refused(short)
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if n > len(data) - pos - 12:
            raise Refused(short)
        body = data[pos + 8:pos + 8 + n]
        if zlib.crc32(tag + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise Refused(R_CRC)
        if hdr is None:
            if tag != b"IHDR" or n != 13:
                raise Refused(R_BAD_IHDR)
            hdr = struct.unpack(">IIBBBBB", body)
            w, h, depth, ctype, comp, filt, lace = hdr
            if (w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF or comp or filt or lace > 1 or ctype not in (0, 2, 3, 4, 6)
                    or depth not in (1, 2, 4, 8, 16)):
                raise Refused(R_BAD_IHDR)
            later = (R_PALETTE if ctype == 3 else R_GRAY_ALPHA if ctype == 4 else R_BIT_DEPTH if depth != 8 else
                     R_INTERLACE if lace else 0)
        elif tag == b"IHDR":
            raise Refused(R_BAD_IHDR)
        elif tag == b"IDAT":
            if closed:
                raise Refused(R_IDAT_ORDER)
            idat.append((pos + 8, pos + 8 + n))
        elif tag == b"IEND":
            end = True
        elif tag in (b"acTL", b"fcTL", b"fdAT"):
            later = later or R_APNG
        elif not tag[0] & 0x20 and tag != b"PLTE":
            raise Refused(R_CRITICAL)
        if idat and tag != b"IDAT":
            closed = True
        pos += 12 + n
    if later:
        raise Refused(later)
    if not idat:
        raise Refused(R_NO_IDAT)
    joined = b"".join(data[a:b] for a, b in idat)
    if len(joined) < 6:
        raise Refused(R_ZLIB)
    cmf, flg = joined[0], joined[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or ((cmf << 8) | flg) % 31:
        raise Refused(R_ZLIB)
    if flg & 0x20:
        raise Refused(R_ZLIB_DICT)
    w, h, depth, ctype = hdr[:4]
    return {"width": w, "height": h, "channels": {0: 1, 2: 3, 6: 4}[ctype], "bit_depth": depth, "color_type": ctype, "interlace": 0,
            "nidat": len(idat), "idat_bytes": len(joined), "cmf": cmf, "flg": flg, "adler": struct.unpack(">I", joined[-4:])[0],
            "idat": idat}


@pytest.mark.parametrize("name", NAMES)
def test_library_parse_equals_restatement(name):
    from sfh_amd.pngdec import parse_png
    data = FILES[name].data
    want = ref_parse(data)
    assert parse_png(data) == want
    assert parse_png(np.frombuffer(data, np.uint8)) == want
    assert want["adler"] == zlib.adler32(PC.expected_filtered(data)) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ refusals

def _refusals():
    base = PC.cases()["pattern_37x50x3_cycle"].data
    z = PC.joined_idat(base)
    idat = PC.chunk(b"IDAT", z)
    end = PC.chunk(b"IEND", b"")
    head = PC.SIG + PC.ihdr(37, 50, 3)
    assert head + idat + end == base
    c = {}
    c["depth16"] = (PC.SIG + PC.ihdr(37, 50, 1, depth=16) + idat + end, NotImplementedError, R_BIT_DEPTH, "bit depth")
    c["depth1"] = (PC.SIG + PC.ihdr(37, 50, 1, depth=1) + idat + end, NotImplementedError, R_BIT_DEPTH, "bit depth")
    c["palette"] = (PC.SIG + PC.ihdr(37, 50, 1, ctype=3) + PC.chunk(b"PLTE", bytes(range(12))) + idat + end, NotImplementedError, R_PALETTE,
                    "palette")
    c["gray_alpha"] = (PC.SIG + PC.ihdr(37, 50, 1, ctype=4) + idat + end, NotImplementedError, R_GRAY_ALPHA, r"gray \+ alpha")
    c["adam7"] = (PC.SIG + PC.ihdr(37, 50, 3, interlace=1) + idat + end, NotImplementedError, R_INTERLACE, "Adam7")
    c["apng"] = (head + PC.chunk(b"acTL", struct.pack(">II", 1, 0)) + idat + end, NotImplementedError, R_APNG, "APNG")
    flipped = bytearray(base)
    flipped[len(head) + 8 + 20] ^= 0x10
    c["crc_idat"] = (bytes(flipped), ValueError, R_CRC, "CRC")
    flipped = bytearray(head + PC.chunk(b"tEXt", b"Comment\0hello") + idat + end)
    flipped[len(head) + 8 + 9] ^= 1
    c["crc_ancillary"] = (bytes(flipped), ValueError, R_CRC, "CRC")
    c["idat_not_consecutive"] = (head + PC.chunk(b"IDAT", z[:30]) + PC.chunk(b"tEXt", b"Comment\0x") + PC.chunk(b"IDAT", z[30:]) + end,
                                 ValueError, R_IDAT_ORDER, "not consecutive")
    c["no_idat"] = (head + end, ValueError, R_NO_IDAT, "no IDAT")
    c["no_iend"] = (head + idat, ValueError, R_NO_IEND, "IEND")
    c["cut_in_idat"] = (base[:len(head) + 40], ValueError, R_NO_IEND, "IEND")
    c["not_png"] = (b"\xff\xd8\xff\xe0" + base[4:], ValueError, R_NOT_PNG, "signature")
    c["truncated"] = (base[:20], ValueError, R_TRUNCATED, "end inside the header")
    c["no_ihdr"] = (PC.SIG + idat + end, ValueError, R_BAD_IHDR, "IHDR")
    c["ihdr_twice"] = (head + PC.ihdr(37, 50, 3) + idat + end, ValueError, R_BAD_IHDR, "IHDR")
    c["width0"] = (PC.SIG + PC.ihdr(37, 0, 3) + idat + end, ValueError, R_BAD_IHDR, "IHDR")
    c["zlib_cm"] = (head + PC.chunk(b"IDAT", b"\x77\x09" + z[2:]) + end, ValueError, R_ZLIB, "zlib header")
    c["zlib_window_64k"] = (head + PC.chunk(b"IDAT", b"\x88\x1c" + z[2:]) + end, ValueError, R_ZLIB, "zlib header")
    c["zlib_check_bits"] = (head + PC.chunk(b"IDAT", b"\x78\x02" + z[2:]) + end, ValueError, R_ZLIB, "zlib header")
    c["zlib_short"] = (head + PC.chunk(b"IDAT", z[:5]) + end, ValueError, R_ZLIB, "zlib header")
    c["zlib_dictionary"] = (head + PC.chunk(b"IDAT", b"\x78\x20" + z[2:]) + end, ValueError, R_ZLIB_DICT, "preset dictionary")
    c["unknown_critical"] = (head + PC.chunk(b"ABCD", b"") + idat + end, ValueError, R_CRITICAL, "critical")
    for v in (0x7709, 0x881c, 0x7820):
        assert v % 31 == 0
    return c


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_without_device(name):
    from sfh_amd.pngdec import parse_png
    data, exc, reason, word = REFUSALS[name]
    with pytest.raises(Refused) as ref:
        ref_parse(data)
    assert ref.value.reason == reason
    with pytest.raises(exc, match=word):
        parse_png(data)


def test_stage_refuses_wrong_size_and_oversize_files():
    """what depends on the decoder, not on the file alone: sfh_png_dec_stage, host code"""
    import ctypes
    from sfh_amd import _lib
    lib = _lib.load()
    data = PC.cases()["pattern_37x50x3_cycle"].data
    arr = np.frombuffer(data, np.uint8)

    def stage(H, W, C, max_bytes, files=(arr,)):
        need = lib.sfh_png_dec_staging_bytes(len(files), H, W, C, max_bytes)
        assert need > 0
        buf = np.zeros(need + 16, np.uint8)
        off = (-buf.ctypes.data) % 16
        ptrs = (ctypes.c_void_p * len(files))(*[f.ctypes.data for f in files])
        sizes = (ctypes.c_int64 * len(files))(*[f.size for f in files])
        reason, index = ctypes.c_int32(0), ctypes.c_int32(-1)
        used = lib.sfh_png_dec_stage(ptrs, sizes, len(files), H, W, C, max_bytes, ctypes.c_void_p(buf.ctypes.data + off), need,
                                     ctypes.byref(reason), ctypes.byref(index))
        return used, reason.value, index.value

    used, reason, _ = stage(37, 50, 3, len(data))
    assert used > len(data) and reason == 0
    assert stage(37, 51, 3, len(data))[:2] == (-1, R_SIZE)
    assert stage(50, 37, 3, len(data))[:2] == (-1, R_SIZE)
    assert stage(37, 50, 1, len(data))[:2] == (-1, R_SIZE)
    assert stage(37, 50, 4, len(data))[:2] == (-1, R_SIZE)
    assert stage(37, 50, 3, len(data) - 1)[:2] == (-1, R_TOO_LONG)
    other = np.frombuffer(PC.cases()["pattern_37x50x4_cycle"].data, np.uint8)
    assert stage(37, 50, 3, max(len(data), other.size), files=(arr, other)) == (-1, R_SIZE, 1)
    bad = np.frombuffer(REFUSALS["crc_idat"][0], np.uint8)
    assert stage(37, 50, 3, len(data), files=(arr, arr, bad)) == (-1, R_CRC, 2)
    assert lib.sfh_png_dec_scratch_bytes(1, 37, 50, 2) == -1
    assert lib.sfh_png_dec_scratch_bytes(1, 65535, 65535, 4) == -1                        # a filtered stream of 2 GiB or more
    assert lib.sfh_png_decode(None, None, 0, 1, 37, 50, 3, 1, len(data), 0, None, 0, None, None, None, None) == -1


def test_decoder_refuses_cpu_device():
    from sfh_amd.pngdec import PngDecoder
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PngDecoder(37, 50, device="cpu")


# ------------------------------------------------------------------------------------------------------------ the stand-alone program

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "pngdec")


def _run(program, tmp_path, files):
    paths = []
    for k, data in enumerate(files):
        paths.append(str(tmp_path / f"{k}.png"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lines = []
    for i in range(0, len(paths), 500):
        r = subprocess.run([program] + paths[i:i + 500], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]           # a sanitizer report ends the program non-zero
        lines += r.stdout.split("\n")[:-1]
    assert len(lines) == len(paths)
    return [ln.split() for ln in lines]


def _dumped(tmp_path, k, suffix):
    return np.fromfile(str(tmp_path / f"{k}.png{suffix}"), dtype=np.uint8)


def test_host_program_equals_zlib_and_decode_png_on_wellformed_files(host_program, tmp_path):
    """both legs, lane by lane: the serial leg's filtered stream is zlib's and its pixels are decode_png's; the segmented leg
    accepts exactly the files it should, and its filtered stream is the serial leg's"""
    from sfh_amd.outputs import decode_png
    for k, (name, out) in enumerate(zip(NAMES, _run(host_program, tmp_path, [FILES[n].data for n in NAMES]))):
        assert out == ["ok", "0", str(int(FILES[name].segmented)), "1"], (name, out)
        assert _dumped(tmp_path, k, ".filt").tobytes() == PC.expected_filtered(FILES[name].data), name
        want = _file_order(decode_png(np.frombuffer(FILES[name].data, np.uint8)))
        assert np.array_equal(_dumped(tmp_path, k, ".px"), want.reshape(-1)), name


CORRUPTED = ("corrupt_dynamic_20x20x1", "corrupt_fixed_7x9x3", "corrupt_stored_7x9x3")


def test_host_program_on_corrupt_streams(host_program, tmp_path):
    """every truncation point of the compressed stream and 200 single-bit flips in it, of three small files (dynamic, fixed and
    stored blocks), every chunk CRC right: a clean run every time (no sanitizer report, exit 0), and per file either a status or
    the output of exactly the expected size - then, with the Adler-32 right, the expected bytes"""
    rng = np.random.default_rng(20261018)
    variants = []
    for name in CORRUPTED:
        data = PC.cases()[name].data
        z = PC.joined_idat(data)
        assert len(z) < 400
        for t in range(6, len(z)):
            variants.append((name, PC.rewrap(data, z[:t - 4] + z[-4:])))      # the deflate bytes cut, the Adler-32 kept
        for bit in rng.integers(16, (len(z) - 4) * 8, 200):
            b = bytearray(z)
            b[bit >> 3] ^= 1 << (bit & 7)
            variants.append((name, PC.rewrap(data, bytes(b))))
    clean = failed = 0
    for k, ((name, v), out) in enumerate(zip(variants, _run(host_program, tmp_path, [v for _, v in variants]))):
        assert out[0] == "ok", out                                               # the chunks are right: never refused
        if int(out[1]) == 0:                                                     # the output has exactly the expected size ...
            want = PC.expected_filtered(PC.cases()[name].data)
            assert _dumped(tmp_path, k, ".filt").size == len(want)
            assert _dumped(tmp_path, k, ".filt").tobytes() == want               # ... and, the Adler-32 being right, the bytes
            clean += 1
        else:
            failed += 1
        try:
            zlib_ok = len(PC.expected_filtered(v)) > 0
        except zlib.error:
            zlib_ok = False
        assert zlib_ok == (int(out[1]) == 0), (name, out)                        # zlib agrees on which streams are sound
    assert failed > 500 and clean >= 0
