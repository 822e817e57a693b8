"""csrc/conv_geom.h, compiled for the host (tests/conv_geom_host_main.cpp: AddressSanitizer, UBSan, nothing preloaded): the
workgroup orders are bijections, the reciprocal row split is exact wherever the guard admits a geometry, the fill function
gives the numbers the launchers computed before they shared it, and engine.py's restatement agrees with it.  No GPU."""
import subprocess
import types

import pytest

from host_program import build_host_program

TILES = ((8, 32), (16, 16), (32, 8), (8, 16), (16, 8))
SIZES = ((7, 5), (12, 20), (23, 41), (45, 80), (360, 640))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "conv_geom")


def _run(program, mode, stdin=None):
    r = subprocess.run([program, mode], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def test_every_workgroup_order_is_a_bijection(program):
    """ntiles 1 .. 200, nblk in {1, 2, 3, 4, 8, 16, 32}, every divisor nb_group, both reverse_tiles values: over the grid
    cdiv(ntiles, 8) * 8 * nblk the live workgroups map one-to-one onto {tile < ntiles} x {nb < nblk}; with reverse_tiles every
    XCD walks its own range backwards and nothing else changes; the specialisations equal the general form."""
    got = {}
    for line in _run(program, "orders"):
        name, conf, fail = line.split()
        got[name] = (int(conf.split("=")[1]), int(fail.split("=")[1]))
        print(line)
    ndiv = sum(sum(1 for g in range(1, n + 1) if n % g == 0) for n in (1, 2, 3, 4, 8, 16, 32))
    assert got == {"xcd_range": (200 * ndiv * 2, 0), "xcd_range_reverse": (200 * ndiv, 0), "xcd_range_all": (200 * 7, 0),
                   "xcd_range_one": (200 * 2, 0), "round_robin": (200 * 7, 0), "weight_stationary": (200 * 3, 0)}


def test_the_reciprocal_row_split_is_exact_where_the_guard_admits(program):
    """rows_per_img in {1, 2, 3, 8, 17, 46, 182, 362, 722, 65535}: for the largest batch the guard admits, umulhi(r, magic) ==
    r / rows_per_img at k * rows_per_img - 1, + 0, + 1 (k = 0, 1, 2, a middle one, the last), over the 64 rows behind
    rows_total that the last tile can reach and on a sweep of the rest; the guard refuses the next batch.  (One row per frame
    has no 32-bit reciprocal and 65535 rows leave no room for the 64 rows behind the end: the guard admits no batch of those.)"""
    want = (1, 2, 3, 8, 17, 46, 182, 362, 722, 65535)
    lines = _run(program, "rows")
    assert len(lines) == len(want)
    for d, line in zip(want, lines):
        print(line)
        f = dict(tok.split("=") for tok in line.split())
        assert int(f["rows_per_img"]) == d
        b = int(f["max_batch"])
        # the guard itself: (batch * rows_per_img + 64) * rows_per_img < 2^32, and at least two rows per frame
        assert b == (((1 << 32) - 1) // d - 64) // d if d >= 2 and ((1 << 32) - 1) // d - 64 >= d else b == 0
        assert int(f["wrong"]) == 0 and int(f["next_refused"]) == 1
        assert (int(f["checked"]) > 128) == (b > 0)


def _table():
    return [(b, H, W, k, s, split, th, tw) for k in (1, 2, 3, 4) for s in (1, 2) for split in (False, True) for H, W in SIZES
            for b in (1, 3, 16) for th, tw in TILES]


def _parent(b, H, W, k, s, split, th, tw):
    """the launchers' own formulas before they shared sfh_conv_grid (launch_s3 / launch_conv) -> Ho, Wo, rows_per_img, ntiles"""
    pad, pada = k // 2, (k - 1) // 2
    ho, wo = (H + pad + pada - k) // s + 1, (W + pad + pada - k) // s + 1
    tiles_x = (wo + tw - 1) // tw
    if s == 1:
        zr = pad
        if split:                     # conv_s3.hip; conv_mfma.hip has ZROWS = PAD
            if (ho + zr) & 1:
                zr += 1
            if zr == 0:
                zr = 1 if ho & 1 else 0
        rpi = ho + zr
        return ho, wo, rpi, tiles_x * ((b * rpi + th - 1) // th)
    return ho, wo, ho, tiles_x * ((ho + th - 1) // th) * b


@pytest.fixture(scope="module")
def filled(program):
    table = _table()
    text = "".join(f"{b} {H} {W} {k} {s} {int(s == 1)} {int(split)} {th} {tw}\n" for b, H, W, k, s, split, th, tw in table)
    out = [tuple(int(v) for v in line.split()) for line in _run(program, "grid", text)]
    assert len(out) == len(table)
    return list(zip(table, out))


def test_the_fill_function_reproduces_the_launchers_numbers(filled):
    assert len(filled) == 4 * 2 * 2 * 5 * 3 * 5
    for case, (ok, ho, wo, rpi, rows_total, magic, tiles_x, tiles_y, ntiles) in filled:
        assert ok == 1, case
        assert (ho, wo, rpi, ntiles) == _parent(*case), case
        b, s = case[0], case[4]
        assert tiles_x * tiles_y * (b if s == 2 else 1) == ntiles, case
        assert (rows_total, magic) == ((b * rpi, (1 << 32) // rpi + 1) if s == 1 else (0, 0)), case


def test_engine_agrees_with_the_header(filled):
    from sfh_amd import engine as E
    for (b, H, W, k, s, split, th, tw), (ok, ho, wo, rpi, rows_total, magic, tiles_x, tiles_y, ntiles) in filled:
        conv = types.SimpleNamespace(ksize=k, stride=s, fmt="h2" if split else None)
        g = E.PackedConv._out_geometry(conv, H, W)
        assert g[:2] == (ho, wo), (b, H, W, k, s, split)
        zr = E._zero_rows(k, ho, split)
        assert g[2] == zr
        if s == 1:
            assert zr == rpi - ho, (H, k, split)
        assert E._ntiles(b, ho, wo, s, zr, th, tw) == ntiles, (b, H, W, k, s, split, th, tw)
