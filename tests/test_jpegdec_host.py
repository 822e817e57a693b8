"""CPU-side pins of sfh_amd.jpegdec: the numpy restatement (tests/jpegdec_ref.py) equals PIL's pixels byte for byte; the library's
host parse equals the restatement's field by field; every refusal fires without a device; the restated subsequence iteration
equals the serial decode; the decode core (csrc/jpegdec_core.h), built as a stand-alone program under the address and
undefined-behaviour sanitizers, gives the restatement's coefficients on well-formed files and a clean run on corrupt ones.
All comparisons are equality."""
import functools
import io
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpegdec_cases as DC
import jpegdec_ref as R
from host_program import build_host_program

SMALL = sorted(DC.small_files())
TEMPLATES = sorted(DC.template_files())


def _file(name):
    return DC.small_files()[name] if name in DC.small_files() else DC.template_files()[name]


@functools.lru_cache(maxsize=None)
def _decoded(name):
    """-> (parse, coefficients, statuses) of the restatement's serial decode: computed once, shared, never written to"""
    data = _file(name)
    p = R.parse(data)
    coef, statuses = R.decode_serial(p, data)
    coef.setflags(write=False)
    return p, coef, statuses


@pytest.mark.parametrize("name", SMALL + TEMPLATES)
def test_restatement_equals_pil(name):
    data = _file(name)
    p, coef, statuses = _decoded(name)
    assert statuses == [0] * p["nsegments"]
    if DC.has_dri(data):
        assert p["nsegments"] > 8, "a case with a restart interval must reach the RST7 -> RST0 wrap"
    want = DC.pil_decode(data)
    got = R.pixels(p, coef, bgr=False)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want)
    if want.ndim == 3:
        assert np.array_equal(R.pixels(p, coef, bgr=True), want[:, :, ::-1])


def test_case_list_covers_what_it_names():
    files = DC.small_files()
    parses = {n: R.parse(f) for n, f in files.items()}
    assert {(p["height"], p["width"]) for p in parses.values()} >= set(DC.SIZES)
    assert {(p["ncomp"], p["hsamp"]) for p in parses.values()} == {(1, 1), (3, 1), (3, 2)}
    assert any(p["restart_interval"] == 1 for p in parses.values())
    assert any(p["restart_interval"] == p["mcus_x"] > 1 for p in parses.values())
    assert any(p["restart_interval"] == 0 for p in parses.values())
    # optimised tables are not Annex K's
    std = R.parse(files["noise_37x50_420"])["ac"][0]["vals"]
    assert any(not np.array_equal(p["ac"][p["acsel"][0]]["vals"], std) for p in parses.values())


def _same_tab(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("look", "maxcode", "valoff", "vals"))


@pytest.mark.parametrize("name", SMALL + TEMPLATES)
def test_library_parse_equals_restatement(name):
    from sfh_amd.jpegdec import parse_jpeg
    data = _file(name)
    want = R.parse(data)
    got = parse_jpeg(data)
    for k in ("width", "height", "ncomp", "hsamp", "vsamp", "mcus_x", "mcus_y", "blocks_per_mcu", "restart_interval", "nsegments",
              "scan_begin", "scan_end", "qsel", "dcsel", "acsel", "segments"):
        assert got[k] == want[k], k
    assert sorted(got["quant"]) == sorted(set(want["qsel"]))
    for q in got["quant"]:
        assert np.array_equal(got["quant"][q], want["quant"][q])
    for kind, sel in (("dc", "dcsel"), ("ac", "acsel")):
        assert sorted(got[kind]) == sorted(set(want[sel]))
        for t in got[kind]:
            assert _same_tab(got[kind][t], want[kind][t]), (kind, t)
    assert parse_jpeg(np.frombuffer(data, np.uint8))["segments"] == want["segments"]


# ------------------------------------------------------------------------------------------------------------ refusals

def _pil(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _patched(data, marker, fn):
    """the file with the body of the first segment `marker` rewritten by fn(bytearray body) -> body (the length is updated)"""
    b = bytes(data)
    i = b.index(bytes([0xFF, marker]))
    ln = (b[i + 2] << 8) | b[i + 3]
    body = bytes(fn(bytearray(b[i + 4:i + 2 + ln])))
    return b[:i + 2] + (len(body) + 2).to_bytes(2, "big") + body + b[i + 2 + ln:]


def _refusals():
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    base = _pil(rgb, quality=90, subsampling=2)
    c = {}
    c["progressive"] = (_pil(rgb, quality=90, progressive=True), NotImplementedError, R.R_PROGRESSIVE, "progressive")
    c["422"] = (_pil(rgb, quality=90, subsampling=1), NotImplementedError, R.R_SAMPLING, "4:2:2")
    c["cmyk"] = (_pil_cmyk(rgb), NotImplementedError, R.R_COMPONENTS, "4 components")
    # a 16-bit DQT: precision nibble 1 and 128 bytes of table
    c["dqt16"] = (_patched(base, 0xDB, lambda b: bytearray([0x10 | b[0]]) + bytearray(x for v in b[1:65] for x in (0, v)) + b[65:]),
                  NotImplementedError, R.R_DQT16, "16-bit quantisation")
    c["precision12"] = (_patched(base, 0xC0, lambda b: bytearray([12]) + b[1:]), NotImplementedError, R.R_PRECISION, "12-bit")
    c["sof4"] = (_patched(base, 0xC0, lambda b: b[:5] + bytearray([4]) + b[6:] + bytearray([4, 0x11, 1])), NotImplementedError,
                 R.R_COMPONENTS, "4 components")
    c["arithmetic"] = (base.replace(b"\xff\xc0", b"\xff\xc9", 1), NotImplementedError, R.R_ARITHMETIC, "arithmetic")
    c["height0"] = (_patched(base, 0xC0, lambda b: b[:1] + bytearray([0, 0]) + b[3:]), NotImplementedError, R.R_DNL, "DNL")
    c["rgb_ids"] = (_patched(_patched(base.replace(b"\xff\xe0\x00\x10JFIF\x00", b"\xff\xe1\x00\x10Jfif\x00", 1), 0xC0,
                                      lambda b: b[:6] + bytearray([82]) + b[7:9] + bytearray([71]) + b[10:12] + bytearray([66]) + b[13:]),
                             0xDA, lambda b: b[:1] + bytearray([82]) + b[2:3] + bytearray([71]) + b[4:5] + bytearray([66]) + b[6:]),
                    NotImplementedError, R.R_COLORSPACE, "RGB")
    c["truncated_header"] = (base[:200], ValueError, R.R_TRUNCATED, "end inside the header")
    c["not_jpeg"] = (b"\x89PNG" + base[4:], ValueError, R.R_NOT_JPEG, "SOI")
    c["no_tables"] = (base[:2] + base[base.index(b"\xff\xc0"):], ValueError, R.R_BAD_TABLE, "table")
    c["bad_sos"] = (_patched(base, 0xDA, lambda b: b[:-3] + bytearray([1, 63, 0])), ValueError, R.R_BAD_SOS, "SOS")
    dri = _pil(rgb, quality=90, subsampling=2, restart_marker_blocks=1)
    i = dri.index(b"\xff\xd1", dri.index(b"\xff\xda"))
    c["restart_order"] = (dri[:i + 1] + b"\xd3" + dri[i + 2:], ValueError, R.R_RESTART, "restart")
    return c


def _pil_cmyk(rgb):
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(buf, "JPEG", quality=90)
    return buf.getvalue()


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_without_device(name):
    from sfh_amd.jpegdec import parse_jpeg
    data, exc, reason, word = REFUSALS[name]
    with pytest.raises(R.Refused) as ref:
        R.parse(data)
    assert ref.value.reason == reason
    with pytest.raises(exc, match=word):
        parse_jpeg(data)


def test_stage_refuses_wrong_size_and_oversize_files():
    """what depends on the decoder, not on the file alone: sfh_jpeg_dec_stage, host code"""
    import ctypes
    from sfh_amd import _lib
    lib = _lib.load()
    data = DC.small_files()["noise_37x50_420"]
    arr = np.frombuffer(data, np.uint8)

    def stage(H, W, C, max_bytes, files=(arr,)):
        need = lib.sfh_jpeg_dec_staging_bytes(len(files), H, W, C, max_bytes)
        assert need > 0
        buf = np.zeros(need + 16, np.uint8)
        off = (-buf.ctypes.data) % 16
        ptrs = (ctypes.c_void_p * len(files))(*[f.ctypes.data for f in files])
        sizes = (ctypes.c_int64 * len(files))(*[f.size for f in files])
        reason, index = ctypes.c_int32(0), ctypes.c_int32(-1)
        used = lib.sfh_jpeg_dec_stage(ptrs, sizes, len(files), H, W, C, max_bytes, 1024, ctypes.c_void_p(buf.ctypes.data + off), need,
                                      ctypes.byref(reason), ctypes.byref(index))
        return used, reason.value, index.value

    used, reason, _ = stage(37, 50, 3, len(data))
    assert used > len(data) and reason == 0
    assert stage(37, 51, 3, len(data))[:2] == (-1, R.R_SIZE)
    assert stage(50, 37, 3, len(data))[:2] == (-1, R.R_SIZE)
    assert stage(37, 50, 1, len(data))[:2] == (-1, R.R_SIZE)
    assert stage(37, 50, 3, len(data) - 1)[:2] == (-1, R.R_TOO_LONG)
    other = np.frombuffer(DC.small_files()["noise_37x50_444"], np.uint8)                  # another sampling than the first file's
    assert stage(37, 50, 3, max(len(data), other.size), files=(arr, other)) == (-1, R.R_SIZE, 1)
    assert lib.sfh_jpeg_dec_scratch_bytes(1, 37, 50, 3, len(data), 1000) == -1           # not a multiple of 32
    assert lib.sfh_jpeg_dec_scratch_bytes(1, 37, 50, 2, len(data), 1024) == -1


def test_decoder_refuses_cpu_device():
    from sfh_amd.jpegdec import JpegDecoder
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        JpegDecoder(37, 50, device="cpu")


# ------------------------------------------------------------------------------------------------------------ subsequences

ITERATION = ("noise_37x50_420", "noise_17x33_gray", "noise_160x48_444", "noise_160x48_420_rows", "noise_37x50_q100_444_blocks",
             "blocks0_255_q100_420", "noise_37x50_q25_420_opt")


@pytest.mark.parametrize("subseq_bits", (32, 64, 1024, 4096))
def test_subsequence_iteration_equals_serial_decode(subseq_bits):
    for name in ITERATION:
        p, coef, statuses = _decoded(name)
        got, st, rounds = R.decode_subsequences(p, _file(name), subseq_bits)
        assert np.array_equal(got, coef), name
        assert st == statuses, name
        assert rounds >= 1


# ------------------------------------------------------------------------------------------------------------ the stand-alone program

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "jpegdec")


def _run(program, paths, subseq_bits):
    r = subprocess.run([program, "--subseq", str(subseq_bits)] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]               # a sanitizer report ends the program non-zero
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(paths)
    return [ln.split() for ln in lines]


def test_host_program_equals_restatement_on_wellformed_files(host_program, tmp_path):
    names = SMALL + TEMPLATES
    paths = []
    for k, name in enumerate(names):
        paths.append(str(tmp_path / f"{k}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(_file(name))
    for subseq_bits in (1024, 64):
        for name, out in zip(names, _run(host_program, paths, subseq_bits)):
            _, coef, statuses = _decoded(name)
            status, h = R.checksum(coef, statuses)
            assert out[:3] == ["ok", str(status), f"{h:016x}"], (name, subseq_bits)
            assert status == 0


def test_host_program_on_corrupt_streams(host_program, tmp_path):
    """every truncation point of the scan and 200 single-bit flips in the scan of three small files: a clean run every time (no
    sanitizer report, exit 0), and per file either a clean status with the restatement's coefficients or a non-zero status"""
    rng = np.random.default_rng(20261018)
    variants = []
    for name in ("noise_16x16_420", "noise_17x33_gray", "noise_37x50_q75_444_blocks"):
        data = _file(name)
        p = R.parse(data)
        for t in range(p["scan_begin"], p["scan_end"] + 1):
            variants.append(data[:t])
        for bit in rng.integers(p["scan_begin"] * 8, p["scan_end"] * 8, 200):
            b = bytearray(data)
            b[bit >> 3] ^= 0x80 >> (bit & 7)
            variants.append(bytes(b))
    paths = []
    for k, v in enumerate(variants):
        paths.append(str(tmp_path / f"{k}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(v)
    clean = 0
    for subseq_bits in (32, 1024):
        for v, out in zip(variants, _run(host_program, paths, subseq_bits)):
            try:
                p = R.parse(v)
            except R.Refused as e:
                assert out == ["refused", str(e.reason)]
                continue
            coef, statuses = R.decode_serial(p, v)
            status, h = R.checksum(coef, statuses)
            assert out[0] == "ok" and int(out[1]) == status
            if status == 0:
                assert out[2] == f"{h:016x}"
                clean += 1
    assert clean > 0
