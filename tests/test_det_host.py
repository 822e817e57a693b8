"""CPU checks of the deterministic training mode (include/sfh_amd.h "Deterministic training mode"; csrc/det_core.h):

- tests/det_ref.py, the numpy restatement of the sum pass, on inputs where the order shows;
- tests/det_host_main.cpp, a stand-alone program under AddressSanitizer and UBSan that walks csrc/det_core.h for every kernel
  family over the case geometries of the GPU suites: every tile / pixel / block belongs to exactly one slab, every slab index
  is below the count, the store pass writes every workspace element exactly once, and the bytes equal what the library's size
  queries answer (compared here); its sum pass equals det_ref on random and on cancelling slabs, bit for bit.
  What this shares with the device code: the split plans, the block counts, the bytes, det_slab_offset, det_wgrad_elem,
  det_sum and det_dst_offset - the functions launchers and DET kernels call.  The kernels' tile and pixel LOOPS and lane maps
  are restated in the program (the kernels keep the loops their default instantiation always had), so the "exactly one
  slab" and "written exactly once" walks check the plans against a restatement, not against what the device evaluates: that
  is the GPU suite's part (NaN-filled workspaces, slabs read back);
- the size queries and the refusals of a missing or short workspace through ctypes, without a device;
- for every rule of every family's plan, a geometry that the size query, the plain entry and the sibling refuse alike.
No sanitizer runs on code loaded into Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dense_conv_cases as DK
import det_ref
import grouped_conv_cases as GK
import host_program
import theta_grad_cases as TK
import train_kernel_cases as cases


# ------------------------------------------------------------------------------------------------ det_ref
def test_det_ref_is_the_ascending_chain():
    """fp32: (1 + 1e8) - 1e8 + 1 = 1 in that order (1 is lost in 1e8, the last 1 survives); the reversed order gives 0 + ... ;
    the chain starts from dst0; fp64 alike at 1e17"""
    for dtype, big in ((np.float32, 1e8), (np.float64, 1e17)):
        p = np.array([[big], [-big], [1.0]], dtype=dtype)
        assert det_ref.det_sum(np.array([1.0], dtype=dtype), p)[0] == dtype(1.0)          # ((1 + big) - big) + 1
        assert det_ref.det_sum(np.array([1.0], dtype=dtype), p[::-1])[0] == dtype(0.0)    # ((1 + 1) - big) + big
        assert det_ref.det_sum(np.array([0.0], dtype=dtype), p[[2, 0, 1]])[0] == dtype(0.0)
    c = det_ref.cancelling(64, 8, np.float32)
    assert not np.array_equal(det_ref.det_sum(np.zeros(8, np.float32), c), det_ref.det_sum(np.zeros(8, np.float32), c[::-1]))
    dst0 = np.arange(12, dtype=np.float32).reshape(2, 6)
    out = det_ref.det_sum_columns(dst0, np.ones((3, 4), np.float32), 2, 3)
    assert np.array_equal(out[:, 3:5], dst0[:, 3:5] + 3) and np.array_equal(out[:, :3], dst0[:, :3]) and out[0, 5] == 5


# ------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    return host_program.build_host_program(tmp_path_factory, "det")


def _geometries():
    """(line of the host program, size query name, its arguments, element bytes) over the cases of the GPU suites"""
    out = []
    for c in DK.WGRAD:
        srcs = [(c.N, c.H, c.W, (0, 0))] + ([(c.N1, c.H - 1, c.W - 1, c.pad)] if c.N1 else [])
        for N, xh, xw, pad in srcs:
            if c.kern == "f32":
                args = (c.M, N, xh, xw, N, pad[0], pad[1], c.B, c.H, c.W, c.ks)
                out.append((f"wgrad {c.M} {N} {c.ks} {N} {xh} {xw} {pad[0]} {pad[1]} {c.B} {c.H} {c.W}", "sfh_conv_wgrad", args, 4))
            else:
                out.append((f"wgrad_s3 {c.M} {N} {c.ks} {c.B} {c.H} {c.W}", "sfh_conv_wgrad_s3", (c.M, N, c.B, c.H, c.W, c.ks), 4))
    # the first-layer form, shapes of the step (the geometry the training tests run) and splits that do not divide the tiles
    for M, B, H, W in ((12, 2, 9, 20), (72, 3, 7, 37), (64, 2, 72, 128), (64, 16, 360, 640)):
        out.append((f"wgrad {M} 4 3 4 {H} {W} 0 0 {B} {H} {W}", "sfh_conv_wgrad", (M, 4, H, W, 4, 0, 0, B, H, W, 3), 4))
    for M, N, ks, B, H, W in ((64, 64, 3, 2, 9, 11), (64, 64, 3, 3, 23, 41), (128, 64, 3, 2, 45, 80), (512, 512, 3, 2, 4, 8),
                              (64, 32, 4, 2, 36, 64), (256, 128, 1, 2, 9, 16)):
        out.append((f"wgrad {M} {N} {ks} {N} {H} {W} 0 0 {B} {H} {W}", "sfh_conv_wgrad", (M, N, H, W, N, 0, 0, B, H, W, ks), 4))
        if ks != 4:
            out.append((f"wgrad_s3 {M} {N} {ks} {B} {H} {W}", "sfh_conv_wgrad_s3", (M, N, B, H, W, ks), 4))
    for c in GK.CASES:
        out.append(("grouped " + " ".join(map(str, c)), "sfh_conv_grouped_wgrad", tuple(c), 4))
    for npix, C in cases.REDUCTIONS + [(255, 12), (256, 96), (257, 12)]:
        out.append((f"red {npix} {C}", "sfh_bn_stats", (npix, C), 8))
        out.append((f"red {npix} {C}", "sfh_bn_bwd_reduce", (npix, C), 8))
        out.append((f"colsum {npix} {C}", "sfh_colsum", (npix, C), 8))
    for B, H, W, cin, nc in cases.OUTCONV_SHAPES + [(16, 360, 640, 64, 4)]:
        out.append((f"outconv {B * H * W} {nc} {cin}", "sfh_outconv_bwd", (cin, nc, B, H, W), 8))
    for B, H, W, C, nout in TK.AVGPOOL_SHAPES:
        out.append((f"avgpool {B} {C} {nout}", "sfh_avgpool_linear_bwd", (B, C, nout), 8))
    for B, H, W in ((1, 1, 1), (2, 9, 13), (2, 512, 513), (16, 360, 640)):
        out.append((f"losses {B * H * W}", "sfh_train_losses", (B, H, W), 8))
        out.append((f"uv {B * 2 * H * W}", "sfh_uv_loss", (B, 2, H, W), 8))
    for batch in TK.POI_BATCHES:
        out.append((f"reproj {batch}", "sfh_reproj_loss", (batch,), 8))
    for w, h in TK.FRAMES + [(640, 360)]:
        for B in (1, 3, 17):
            out.append((f"warp {B} {h} {w}", "sfh_homography_warp_bwd_theta", (B, h, w), 8))
    return out


def test_host_walk_of_every_family(host_bin, tmp_path):
    """the partition walk (see the program's header) and, per geometry, bytes == the library's size query == slabs * elems *
    the element size; the closed-form slab counts of det_ref (restated from the header's table) agree as well"""
    from sfh_amd import _lib
    lib = _lib.load()
    geo = _geometries()
    path = tmp_path / "cases.txt"
    path.write_text("".join(g[0] + "\n" for g in geo))
    r = subprocess.run([host_bin, "walk", str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(geo)
    families = set()
    for line, (text, name, args, item) in zip(lines, geo):
        head, tail = line.split(" -> ")
        assert head == text
        slabs, elems, nbytes = map(int, tail.split())
        assert nbytes == slabs * elems * item and slabs >= 1
        assert getattr(lib, name + "_det_bytes")(*args) == nbytes, (text, name)
        fam, nums = text.split()[0], list(map(int, text.split()[1:]))
        families.add(fam)
        want = {"red": lambda: det_ref.bn_slabs(*nums), "colsum": lambda: det_ref.colsum_slabs(*nums),
                "outconv": lambda: det_ref.outconv_slabs(*nums), "avgpool": lambda: det_ref.avgpool_slabs(*nums),
                "losses": lambda: det_ref.losses_slabs(*nums), "uv": lambda: det_ref.uv_slabs(*nums),
                "reproj": lambda: det_ref.reproj_slabs(*nums), "warp": lambda: det_ref.warp_slabs(*nums),
                "grouped": lambda: det_ref.grouped_slabs(*nums)}.get(fam)
        if want is not None:
            assert want() == (slabs, elems), text
        elif fam in ("wgrad", "wgrad_s3"):
            assert elems == nums[0] * nums[2] ** 2 * nums[1]
    assert families == {"wgrad", "wgrad_s3", "grouped", "red", "colsum", "outconv", "avgpool", "losses", "uv", "reproj", "warp"}
    # the 1x1 map: one tile, one slab
    one = [ln for ln in lines if ln.startswith(("wgrad 64 32 3 32 1 1 ", "wgrad_s3 64 32 3 1 1 1 "))]
    assert len(one) == 3 and all(ln.split(" -> ")[1].split()[0] == "1" for ln in one)     # the fp32, S3 and H2 cases


@pytest.mark.parametrize("kind", ["randn", "cancelling"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_sum_pass_equals_det_ref(host_bin, tmp_path, dtype, kind):
    """det_sum / det_dst_offset of csrc/det_core.h against the numpy restatement, bit for bit: one slab, the BatchNorm shape
    (few elements, 1024 slabs), a backward-filter source at a column offset of a wider raw"""
    for i, (Rn, rows, ncol, raw_n, n_off) in enumerate(((1, 1, 1, 1, 0), (7, 3, 5, 9, 2), (1024, 1, 24, 24, 0), (33, 64, 32, 96, 32))):
        E = rows * ncol
        rng = np.random.default_rng([i, len(kind)])
        p = det_ref.cancelling(Rn, E, dtype, seed=i) if kind == "cancelling" else rng.standard_normal((Rn, E)).astype(dtype)
        dst0 = rng.standard_normal((rows, raw_n)).astype(dtype)
        d = tmp_path / f"s{i}"
        os.makedirs(d)
        np.asarray([dtype == np.float64, Rn, E, ncol, raw_n, n_off], dtype=np.int64).tofile(d / "dims.i64")
        p.tofile(d / "partial.bin")
        dst0.tofile(d / "dst0.bin")
        r = subprocess.run([host_bin, "sum", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(d / "dst.bin", dtype=dtype).reshape(rows, raw_n)
        want = det_ref.det_sum_columns(dst0, p, ncol, n_off)
        bits = np.uint32 if dtype == np.float32 else np.uint64
        assert np.array_equal(got.view(bits), want.view(bits)), (Rn, rows, ncol)


# ------------------------------------------------------------------------------------------------ the C interface, no device
def test_every_accumulating_entry_has_its_sibling_and_query():
    from sfh_amd import _lib
    assert _lib.DET_ENTRIES == tuple(sorted(
        ["sfh_conv_wgrad", "sfh_conv_wgrad_s3", "sfh_conv_grouped_wgrad", "sfh_bn_stats", "sfh_bn_bwd_reduce", "sfh_colsum",
         "sfh_outconv_bwd", "sfh_avgpool_linear_bwd", "sfh_train_losses", "sfh_reproj_loss", "sfh_uv_loss",
         "sfh_homography_warp_bwd_theta"]))
    for n in _lib.DET_ENTRIES:
        res, args = _lib.SIGNATURES[n]
        assert _lib.SIGNATURES[n + "_det"] == (res, args[:-1] + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p])
        assert _lib.SIGNATURES[n + "_det_bytes"][0] is ctypes.c_int64


_HOST_BUFFER = (ctypes.c_double * 4096)()


def _host_pointer():
    """host memory for every pointer argument: nothing below may reach a launch"""
    return ctypes.cast(_HOST_BUFFER, ctypes.c_void_p)


def _entry_calls(p):
    """entry -> function of the geometry the size query sees -> (the query's arguments, the plain entry's arguments).  The
    defaults are an admitted geometry; what the query does not see (channel strides, raw_n, npts, ...) is always valid."""
    return {
        "sfh_bn_stats": lambda npix=10, C=4: ((npix, C), (p, npix, C, p)),
        "sfh_bn_bwd_reduce": lambda npix=10, C=4: ((npix, C), (p, None, p, p, p, p, 1, npix, C, p)),
        "sfh_colsum": lambda npix=10, C=4: ((npix, C), (p, npix, C, 1024, p)),
        "sfh_conv_wgrad": lambda M=64, x_cs=32, xh=5, xw=6, N=32, pad_top=0, pad_left=0, B=1, H=5, W=6, ks=3: (
            (M, x_cs, xh, xw, N, pad_top, pad_left, B, H, W, ks),
            (p, 1024, M, p, x_cs, xh, xw, N, pad_top, pad_left, B, H, W, ks, p, 1024, 0)),
        "sfh_conv_wgrad_s3": lambda M=64, N=32, B=1, H=5, W=6, ks=3: (
            (M, N, B, H, W, ks), (p, M, p, 1 << 20, H, W, N, 0, 0, B, H, W, ks, p, 1 << 20, 0, 2)),
        "sfh_conv_grouped_wgrad": lambda B=1, H=5, W=6, G=2, cg=4, stride=1: ((B, H, W, G, cg, stride), (p, p, p, B, H, W, G, cg, stride)),
        "sfh_outconv_bwd": lambda cin=8, nc=3, B=1, H=5, W=6: ((cin, nc, B, H, W), (p, cin, p, p, nc, B, H, W, p, p, p)),
        "sfh_avgpool_linear_bwd": lambda B=2, C=8, nout=9: ((B, C, nout), (p, p, p, B, 3, 3, C, nout, p, p, p)),
        "sfh_train_losses": lambda B=1, H=5, W=6: ((B, H, W), (p, p, p, p, 4, B, H, W, 2.0, 2.0, 0, 1.0, 0, p, p, p)),
        "sfh_reproj_loss": lambda batch=3: ((batch,), (p, p, p, p, batch, 5, 8.0, p, p)),
        "sfh_uv_loss": lambda B=1, C=2, H=5, W=6: ((B, C, H, W), (p, p, p, 1, B, C, H, W, 2.0, 1, p, p)),
        "sfh_homography_warp_bwd_theta": lambda B=2, h=5, w=6: ((B, h, w), (p, p, 0, 9, 16, B, h, w, p, p)),
    }


def test_size_queries_and_refusals_without_a_device():
    """closed forms of the queries; refused geometries answer -1; a NULL or short workspace returns -1 before anything could be
    launched (the pointers below are host memory: a launch would be an error of its own, not -1)"""
    from sfh_amd import _lib
    lib = _lib.load()
    assert lib.sfh_bn_stats_det_bytes(262401, 4) == 1024 * 8 * 8 and lib.sfh_bn_stats_det_bytes(1, 4) == 64
    assert lib.sfh_bn_bwd_reduce_det_bytes(257, 12) == 2 * 24 * 8 and lib.sfh_colsum_det_bytes(257, 12) == 2 * 12 * 8
    assert lib.sfh_bn_stats_det_bytes(10, 6) == -1 and lib.sfh_colsum_det_bytes(0, 4) == -1
    assert lib.sfh_conv_wgrad_det_bytes(64, 32, 1, 1, 32, 0, 0, 1, 1, 1, 3) == 64 * 9 * 32 * 4           # one tile, one slab
    assert lib.sfh_conv_wgrad_det_bytes(64, 32, 1, 1, 32, 0, 0, 1, 1, 1, 5) == -1
    assert lib.sfh_conv_wgrad_s3_det_bytes(64, 32, 1, 1, 1, 3) == 64 * 9 * 32 * 4
    assert lib.sfh_conv_wgrad_s3_det_bytes(48, 32, 1, 1, 1, 3) == -1
    assert lib.sfh_conv_grouped_wgrad_det_bytes(2, 7, 5, 32, 4, 1) == 2 * 128 * 9 * 4 * 4
    assert lib.sfh_conv_grouped_wgrad_det_bytes(2, 7, 5, 32, 5, 1) == -1
    assert lib.sfh_outconv_bwd_det_bytes(64, 4, 1, 33, 32) == 2 * (4 * 64 + 4) * 8 and lib.sfh_outconv_bwd_det_bytes(64, 9, 1, 3, 3) == -1
    assert lib.sfh_avgpool_linear_bwd_det_bytes(3, 512, 9) == 3 * (9 * 512 + 9) * 8
    assert lib.sfh_train_losses_det_bytes(2, 512, 513) == 2048 * 3 * 8 and lib.sfh_uv_loss_det_bytes(1, 2, 1, 1) == 8
    assert lib.sfh_reproj_loss_det_bytes(65) == 16 and lib.sfh_reproj_loss_det_bytes(0) == -1
    assert lib.sfh_homography_warp_bwd_theta_det_bytes(3, 5, 257) == 2 * 2 * 27 * 8
    assert lib.sfh_homography_warp_bwd_theta_det_bytes(3, 1, 257) == -1
    p = _host_pointer()
    calls = {name: make() for name, make in _entry_calls(p).items()}
    assert sorted(calls) == list(_lib.DET_ENTRIES)
    for name, (query, args) in calls.items():
        need = getattr(lib, name + "_det_bytes")(*query)
        assert need > 0, name
        fn = getattr(lib, name + "_det")
        assert fn(*args, None, need, None) == -1 and b"workspace" in lib.sfh_last_error(), name
        assert fn(*args, p, need - 1, None) == -1 and b"workspace" in lib.sfh_last_error(), name
    assert lib.sfh_det_reduce_f32(None, 1, 1, 1, 1, None, 1, None) == -1
    assert lib.sfh_det_reduce_f64(p, 2, 3, 4, 1, p, 1, None) == -1        # slab_stride < elems


# (entry, the geometry it must refuse): every rule of the family's plan (csrc/det_core.h) at least once
_PIXELS = [dict(npix=0), dict(C=0), dict(C=6)]
_FRAME = [dict(B=0), dict(H=0), dict(W=0)]
REFUSED = (
    [(n, g) for n in ("sfh_bn_stats", "sfh_bn_bwd_reduce", "sfh_colsum") for g in _PIXELS]
    + [("sfh_conv_wgrad", g) for g in _FRAME + [
        dict(xh=0), dict(xw=0), dict(M=0), dict(M=6), dict(N=0, x_cs=8), dict(N=6, x_cs=8),
        dict(x_cs=16),                                   # x_cs < N
        dict(x_cs=34),                                   # x_cs % 4 != 0
        dict(pad_top=1),                                 # a source of the frame's height, one row down: one row too tall
        dict(pad_left=1), dict(pad_top=-1, xh=4), dict(pad_left=-1, xw=5),
        dict(ks=5), dict(ks=2), dict(ks=4, N=64, x_cs=64)]]
    + [("sfh_conv_wgrad_s3", g) for g in _FRAME + [
        dict(ks=4), dict(ks=5), dict(M=0), dict(M=48), dict(N=0), dict(N=16),
        dict(M=1 << 20, N=1 << 20, H=1, W=1)]]           # 2^29 workgroups per split round: the grid does not fit
    + [("sfh_conv_grouped_wgrad", g) for g in _FRAME + [
        dict(cg=5), dict(cg=128), dict(stride=3), dict(stride=0), dict(G=0), dict(G=16385),   # G * cg > 65536
        dict(B=2, H=8192, W=8192)]]                      # 2^27 pixels
    + [("sfh_outconv_bwd", g) for g in _FRAME + [dict(cin=0), dict(cin=6), dict(cin=260), dict(nc=0), dict(nc=9)]]
    + [("sfh_avgpool_linear_bwd", g) for g in [dict(B=0), dict(C=0), dict(nout=0), dict(nout=257)]]
    + [("sfh_train_losses", g) for g in _FRAME]
    + [("sfh_uv_loss", g) for g in _FRAME + [dict(C=0)]]
    + [("sfh_reproj_loss", dict(batch=0))]
    + [("sfh_homography_warp_bwd_theta", g) for g in [dict(B=0), dict(B=65536), dict(h=1), dict(w=1)]]
)


def test_every_entry_has_refused_geometries():
    from sfh_amd import _lib
    assert sorted({n for n, _ in REFUSED}) == list(_lib.DET_ENTRIES)


@pytest.mark.parametrize("name,geometry", REFUSED, ids=[f"{n[4:]}-{'-'.join(f'{k}={v}' for k, v in g.items())}" for n, g in REFUSED])
def test_query_entry_and_sibling_refuse_alike(name, geometry):
    """one plan per family: what the size query answers -1 for, the plain entry and the sibling refuse, and the sibling's
    refusal is the geometry's - it comes before the workspace (here a usable pointer and 2^40 bytes) is looked at.  All three
    return before any device call (the pointers are host memory, and this machine may have no device)."""
    from sfh_amd import _lib
    lib = _lib.load()
    p = _host_pointer()
    query, args = _entry_calls(p)[name](**geometry)
    assert getattr(lib, name + "_det_bytes")(*query) == -1
    assert getattr(lib, name)(*args, None) == -1
    assert getattr(lib, name + "_det")(*args, p, 1 << 40, None) == -1
    assert b"workspace" not in lib.sfh_last_error(), lib.sfh_last_error()
