"""CPU checks of the TIFF codec (sfh_amd.tiffdec / sfh_amd.tiffenc): the written-down rule ``outputs.decode_tiff`` /
``outputs.encode_tiff`` against libtiff's own strips and Pillow on the files of tests/tiff_cases.py, the host parse
``sfh_tiff_parse`` on every case and on one handcrafted file per refusal, and the core csrc/tiff_core.h run lane by lane in the
stand-alone program tests/tiff_host_main.cpp under AddressSanitizer and UBSan - the ONE place where corrupt streams are decoded.

Pillow opens a 3 x 16-bit file only as 8-bit RGB, so for those files only the STRIPS are libtiff's: the predictor at a stride of 3
samples is this project's restatement (tests/tiff_cases.py differences in numpy), checked against libtiff by re-wrapping every
strip as a one-strip gray file."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import tiff_cases as tc
from host_program import build_host_program
from sfh_amd import outputs as O

CASES = tc.cases()
REFUSALS = tc.refusals()
by_name = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])


# ---------------------------------------------------------------------------------------------- the rule
@by_name
def test_decode_rule_equals_the_source_and_pillow(case):
    for bgr in (False, True):
        got = O.decode_tiff(case.file, bgr=bgr)
        assert got.dtype == case.arr.dtype and np.array_equal(got, case.expected(bgr))
    if case.C == 1 or case.bits == 8:                      # Pillow reads these exactly
        assert np.array_equal(np.array(Image.open(io.BytesIO(case.file))), case.expected(False))


@by_name
def test_encode_rule(case):
    img = case.expected(True)
    comp = "lzw" if case.compression == 5 else "none"
    enc = O.encode_tiff(img, comp, case.predictor, case.rps)
    assert enc.dtype == np.uint8 and enc.ndim == 1
    assert np.array_equal(O.decode_tiff(enc), img)
    head = O.tiff_parse(bytes(enc))
    assert head["rows_per_strip"] == case.rps and not head["big_endian"] and head["strips"][0][0] == 8
    assert all(off % 2 == 0 for off, _, _, _ in head["strips"])
    pil = Image.open(io.BytesIO(bytes(enc)))
    assert pil.size == (case.W, case.H)
    if case.C == 1 or case.bits == 8:
        assert np.array_equal(np.array(pil), case.expected(False))
    if case.compression != 5:
        return
    rows = tc.stored_rows(case.arr, case.predictor, False)
    for off, cnt, r0, nr in head["strips"]:
        strip, part = bytes(enc[off:off + cnt]), rows[r0:r0 + nr]
        if part.nbytes > 65536:                            # above Pillow's strip size: the round trip alone
            continue
        # libtiff's decoder gives the differenced samples of the strip back, table-full strips included
        assert np.array_equal(tc.libtiff_decode_strip(strip, nr, part.shape[1], case.bits), part)
        if not case.fills:
            assert strip == tc.libtiff_strip(part)


def test_default_strip_rows():
    assert O.tiff_strip_rows(720, 1280, 3, 16) == 1 and O.tiff_strip_rows(360, 640, 3, 16) == 2
    assert O.tiff_strip_rows(37, 53, 1, 8) == 37 and O.tiff_strip_rows(9000, 1, 1, 8) == 8192
    lab = tc.uv_label(45, 80)
    assert O.tiff_parse(bytes(O.encode_tiff(lab)))["rows_per_strip"] == 17
    assert np.array_equal(O.decode_tiff(O.encode_tiff(lab, "none")), lab)
    with pytest.raises(ValueError):
        O.encode_tiff(lab.astype(np.int32))
    with pytest.raises(ValueError):
        O.encode_tiff(lab, rows_per_strip=46)


@pytest.mark.parametrize("name,data,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_rule_refusals(name, data, reason):
    with pytest.raises(NotImplementedError if reason >= 100 else ValueError) as e:
        O.decode_tiff(data)
    assert O.TIFF_REASONS[reason] in str(e.value)


def test_dataset_switches_on_the_host(tmp_path):
    """prepare_dataset(uv_format=, tif="host") and read_dataset(uv_format="tif", decode="host") with the device replaced by the
    restatement of tests/prep_ref.py: the files, and the .npy route's batch bit for bit"""
    import json
    import torch
    import prep_fixtures as F
    import prep_ref as R
    from sfh_amd import preparation as P
    court, ids = F.court_poi("pitch"), F.court_ids("pitch_v3_nc4_640x360")
    manual, _ = F.exact_annotations(court, F.fixture_thetas()[:3], seed=8, n_short=0)
    os.makedirs(tmp_path / "anno" / "game_a")
    with open(tmp_path / "anno" / "game_a" / "manual_anno.json", "w") as f:
        json.dump({f"{r:06d}": {"poi": manual[r].tolist(), "theta": None} for r in range(3)}, f)
    size = (64, 36)
    maker = R.RefMaker(ids, court, size, uv=True, tables=P.uv_tables((ids.shape[1], ids.shape[0])))
    both, tif = tmp_path / "both", tmp_path / "tif"
    rep = P.prepare_dataset(str(tmp_path / "anno"), str(both), size=size, batch=2, maker=maker, uv_format="both")
    P.prepare_dataset(str(tmp_path / "anno"), str(tif), size=size, batch=2, maker=maker, uv_format="tif")
    assert sorted(os.listdir(both / "game_a")) == [f"{r:06d}{e}" for r in range(3) for e in (".json", ".npy", ".png", ".tif")]
    assert sorted(os.listdir(tif / "game_a")) == [f"{r:06d}{e}" for r in range(3) for e in (".json", ".png", ".tif")]
    for key in rep["written"]:
        lab = np.load(both / (key + ".npy"))
        data = np.fromfile(both / (key + ".tif"), dtype=np.uint8)
        assert np.array_equal(data, O.encode_tiff(lab)) and np.array_equal(data, np.fromfile(tif / (key + ".tif"), dtype=np.uint8))
        stored = O.decode_tiff(data, bgr=False)                 # the file holds (v, u, id): cv2's BGR read puts the id first
        assert np.array_equal(stored[:, :, 2], lab[:, :, 0]) and np.array_equal(stored[:, :, 0], lab[:, :, 2])
    want = P.read_dataset(str(both), rep["written"], use_uv=True)
    got = P.read_dataset(str(tif), rep["written"], use_uv=True, uv_format="tif")
    assert sorted(got) == sorted(want) and want["uv"].any()
    for k in want:
        assert got[k] == want[k] if k == "name" else (got[k].dtype == want[k].dtype and torch.equal(got[k], want[k])), k
    with pytest.raises(ValueError, match="uv_format"):
        P.prepare_dataset(str(tmp_path / "anno"), str(tif), size=size, maker=maker, uv_format="tiff")
    with pytest.raises(ValueError, match="tif="):
        P.prepare_dataset(str(tmp_path / "anno"), str(tif), size=size, maker=maker, uv_format="tif", tif="gpu")
    with pytest.raises(ValueError, match="decode"):
        P.read_dataset(str(tif), rep["written"], use_uv=True, uv_format="tif", decode="device")   # device="cpu"


# ---------------------------------------------------------------------------------------------- the host parse in C
@pytest.fixture(scope="module")
def parse():
    from sfh_amd import _lib, tiffdec
    if not os.path.exists(_lib.LIB_PATH):
        import sfh_amd.build as b
        b.build(verbose=False)
    return tiffdec.parse_tiff


@by_name
def test_parse_fields(case, parse):
    got = parse(case.file)
    want = O.tiff_parse(case.file)
    assert got == want
    assert (got["width"], got["height"], got["channels"], got["bits"]) == (case.W, case.H, case.C, case.bits)
    assert got["big_endian"] == (case.byte_order == "MM") and got["compression"] == case.compression
    assert got["predictor"] == (case.predictor if case.compression == 5 else 1)
    assert [(s[1], s[2]) for s in got["strips"]] == [(len(s), i * case.rps) for i, s in enumerate(case.strips)]
    assert sum(s[3] for s in got["strips"]) == case.H


@pytest.mark.parametrize("name,data,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_parse_refusals(name, data, reason, parse):
    from sfh_amd import _lib, tiffdec
    info = tiffdec.TiffInfo()
    a = np.frombuffer(data, dtype=np.uint8)
    assert _lib.load().sfh_tiff_parse(a.ctypes.data_as(ctypes.c_void_p), a.size, ctypes.byref(info), None, 0) == -1
    assert info.reason == reason
    with pytest.raises(NotImplementedError if reason >= 100 else ValueError):
        parse(data)


def test_stage_refuses_on_the_host(parse):
    """size, channels and bits other than the decoder's and a file above max_file_bytes, without a device"""
    from sfh_amd import _lib
    lib = _lib.load()
    c = next(c for c in CASES if c.name == "size_12x213_rps5")
    need = lib.sfh_tiff_dec_staging_bytes(1, 12, 213, 3, 16, 1 << 16)
    assert need > 0 and lib.sfh_tiff_dec_scratch_bytes(1, 12, 213, 3, 16) >= 12 * 213 * 6
    assert lib.sfh_tiff_dec_staging_bytes(1, 12, 213, 2, 16, 1 << 16) == -1 and lib.sfh_tiff_dec_scratch_bytes(1, 12, 213, 3, 12) == -1
    staging = np.zeros(need + 16, dtype=np.uint8)
    base = staging.ctypes.data + (-staging.ctypes.data) % 16
    a = np.frombuffer(c.file, dtype=np.uint8)
    ptrs, sizes = (ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_int64 * 1)(a.size)

    def stage(H, W, C, bits, max_bytes):
        reason, index = ctypes.c_int32(0), ctypes.c_int32(-1)
        n = lib.sfh_tiff_dec_stage(ptrs, sizes, 1, H, W, C, bits, max_bytes, ctypes.c_void_p(base),
                                   lib.sfh_tiff_dec_staging_bytes(1, H, W, C, bits, max_bytes), ctypes.byref(reason), ctypes.byref(index))
        return n, reason.value, index.value

    assert stage(12, 213, 3, 16, 1 << 16)[0] > 0
    assert stage(12, 212, 3, 16, 1 << 16)[1:] == (11, 0) and stage(12, 213, 1, 16, 1 << 16)[1:] == (11, 0)
    assert stage(12, 213, 3, 8, 1 << 16)[1:] == (11, 0)
    assert stage(12, 213, 3, 16, a.size - 1)[1:] == (12, 0)


# ---------------------------------------------------------------------------------------------- the core under the sanitizers
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "tiff")


def run(program, *args):
    r = subprocess.run([program, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_core_decodes_every_case(program, tmp_path):
    paths = []
    for c in CASES:
        paths.append(str(tmp_path / (c.name + ".tif")))
        with open(paths[-1], "wb") as f:
            f.write(c.file)
    for bgr in (0, 1):
        lines = run(program, "decode", bgr, *paths)
        assert len(lines) == len(CASES)
        for c, path, line in zip(CASES, paths, lines):
            want = f"ok 0 {c.W} {c.H} {c.C} {c.bits} {c.compression} {c.predictor if c.compression == 5 else 1} " \
                   f"{int(c.byte_order == 'MM')} {c.rps} {len(c.strips)}"
            assert line == want, c.name
            px = np.fromfile(path + ".px", dtype="<u2" if c.bits == 16 else np.uint8)
            assert np.array_equal(px.reshape(c.expected(bool(bgr)).shape), c.expected(bool(bgr))), c.name


def pack_codes(codes):
    """(code, width) pairs -> bytes, MSB first"""
    acc = nb = 0
    for code, width in codes:
        acc, nb = (acc << width) | code, nb + width
    return (acc << (-nb % 8)).to_bytes((nb + 7) // 8, "big")


def corrupt_streams():
    """[(name, file, status bits of which at least one must be set; None: any outcome without a report)]"""
    z = np.zeros((3, 7, 1), np.uint8)
    three_rows = tc.Case("z3", z, rps=3).strips[0]
    uv = tc.Case("uv", tc.uv_label(12, 213), rps=5, predictor=2)
    gray = lambda strips, H=2, W=7, rps=2, comp=5: tc.container(H, W, 1, 8, strips, rps, "II", comp, 1)
    out = [("code_above_next", gray([pack_codes([(256, 9), (65, 9), (300, 9), (257, 9)])]), 1),
           ("kwkwk_without_room_is_fine_but_short", gray([pack_codes([(256, 9), (65, 9), (258, 9), (257, 9)])]), 4),
           ("non_literal_after_clear", gray([pack_codes([(256, 9), (300, 9)])]), 2),
           ("non_literal_after_second_clear", gray([pack_codes([(256, 9), (65, 9), (256, 9), (258, 9)])]), 2),
           ("count_overrun", gray([three_rows]), 4),                   # 3 rows of zeros in a strip of 2: a string crosses the end
           ("count_underrun", gray([three_rows], H=4, rps=4), 4),       # EOI before the strip's rows are complete
           ("uncompressed_short", gray([b"\x01" * 13], comp=1), 4),
           ("empty_strip", gray([b""]), 8)]
    for cut in (1, 2, 7, len(uv.strips[0]) // 2):
        strips = [uv.strips[0][:-cut]] + uv.strips[1:]
        # the decode ends with the strip's last byte, so cutting into the EOI and the padding alone may change nothing
        out.append((f"truncated_{cut}", tc.container(12, 213, 3, 16, strips, 5, "II", 5, 2), 8 if cut > 2 else None))
    rng = np.random.default_rng(5)
    for i in range(24):
        s = bytearray(uv.strips[i % 3])
        for _ in range(1 + i % 3):
            s[int(rng.integers(1, len(s)))] ^= 1 << int(rng.integers(0, 8))
        strips = list(uv.strips)
        strips[i % 3] = bytes(s)
        out.append((f"flipped_{i}", tc.container(12, 213, 3, 16, strips, 5, "II", 5, 2), None))
    return out


def test_core_corrupt_streams(program, tmp_path):
    """truncated strips, flipped bits, a code above the next free code, a non-literal after Clear, counts that over- and
    under-run: no sanitizer report (every buffer has exactly its size), the expected status bit, and the rule refuses too"""
    streams = corrupt_streams()
    paths = []
    for name, data, _ in streams:
        paths.append(str(tmp_path / (name + ".tif")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lines = run(program, "decode", 0, *paths)
    assert len(lines) == len(streams)
    for (name, data, bits), path, line in zip(streams, paths, lines):
        word = line.split()
        assert word[0] == "ok", (name, line)
        status = int(word[1])
        if bits is not None:
            assert status & bits and status < 16, (name, line)
        try:
            ref = O.decode_tiff(data, bgr=False)
        except ValueError:
            assert status != 0, name
        else:                                                  # a flipped bit can leave a valid stream: then the same pixels
            assert status == 0, name
            px = np.fromfile(path + ".px", dtype="<u2" if ref.dtype == np.uint16 else np.uint8)
            assert np.array_equal(px.reshape(ref.shape), ref), name


def strip_capacity(n):
    """the bound derived in csrc/tiff_core.h: at most n data codes, 2 + n // 3836 Clear codes and an EOI of at most 12 bits"""
    return (12 * (n + n // 3836 + 4) + 7) // 8


def encoder_inputs():
    rng = np.random.default_rng(11)
    steps = np.concatenate([(np.arange(256) * s) % 256 for s in range(1, 128, 2)]).astype(np.uint8)   # every pair of bytes is new
    out = [(c.name, c.expected(True), c.rps, c.predictor) for c in CASES
           if c.compression == 5 and c.name.split("_")[0] in ("size", "zeros", "random", "codes", "big", "tile", "ramp")]
    out += [("noise8", rng.integers(0, 256, (3, 9000, 1), dtype=np.uint8), 1, 1),
            ("noise16", rng.integers(0, 65536, (2, 700, 3), dtype=np.uint16), 2, 2),
            ("all_pairs_new", steps.reshape(1, -1, 1), 1, 1),
            ("combo_8b_c3", tc.uv_label(37, 53, 8, 3), 5, 2)]
    return out


def test_core_encoder_equals_the_rule_within_capacity(program, tmp_path, parse):
    from sfh_amd import _lib
    lib = _lib.load()
    for name, img, rps, pred in encoder_inputs():
        img = np.ascontiguousarray(img)
        H, W = img.shape[:2]
        C = 1 if img.ndim == 2 else img.shape[2]
        bits = 8 * img.dtype.itemsize
        path = str(tmp_path / (name + ".raw"))
        img.astype("<u2" if bits == 16 else np.uint8).tofile(path)
        assert run(program, "encode", path, H, W, C, bits, 1, 5, pred, rps) == ["ok"], name
        blob = np.fromfile(path + ".enc", dtype=np.uint8).tobytes()
        want = bytes(O.encode_tiff(img.reshape(H, W, C), "lzw", pred, rps))
        head, pos = O.tiff_parse(want), 0
        for off, cnt, r0, nr in head["strips"]:
            n = int.from_bytes(blob[pos:pos + 4], "little")
            raw_bytes = nr * W * C * bits // 8
            assert n <= strip_capacity(raw_bytes) == lib.sfh_tiff_strip_capacity(raw_bytes, 5), (name, r0)
            assert blob[pos + 4:pos + 4 + n] == want[off:off + cnt], (name, r0)
            pos += 4 + n
        assert pos == len(blob), name
    # the bound is nearly met where every pair of bytes is new: one 9 .. 12-bit code per byte
    steps = encoder_inputs()[-2][1].tobytes()
    assert len(O.tiff_lzw_encode(steps)) > 0.9 * strip_capacity(len(steps))
