"""The deterministic training mode (fixed-order slab sums; include/sfh_amd.h "Deterministic training mode", csrc/det_core.h).

Per kernel, through the raw C entries NAME_det, on the cases and inside the bounds of the existing suites (imported from
tests/dense_conv_*.py, grouped_conv_*.py, train_kernel_*.py, theta_grad_*.py - not copied).  Every launch goes through
_det_launch, which asserts for every accumulator:
  1. the result equals tests/det_ref.py's ascending chain over the slabs READ BACK from the workspace, bit for bit (this pins
     the order, not just repeatability);
  3. a second call into fresh outputs and the workspace the first call left behind gives the same bits;
  4. so does a call beside a busy side stream;
  5. the 64-element guards behind every output and behind the workspace keep their bytes;
  6. a workspace one byte short returns -1 and the outputs keep what they held.
and the tests add 2.: the result lies inside the per-element bound the existing test holds the atomic form to (the adds are
the same in number, only their order is fixed), printed next to the atomic form's ratio.  Entries without a case file of
their own (losses, uv, reprojection) are held to the atomic form's result within the distance of two fp64 summations of the
same R + 1 terms: 2.02 * (R + 1) * 2^-53 * (|dst0| + sum |slab|).

The whole step: TrainStep(deterministic=True) twice from one state, bit for bit after every step, in three precisions and three
models; the autograd node under net.train_deterministic; accuracy of the mode's gradients next to the default mode's, against
fp64 autograd under the pass's own ReLU decisions (the ResNet-STN, which training.CAPTURE records; the UNet's legs per kernel).
"""
import ctypes

import numpy as np
import pytest
import torch

import dense_conv_cases as DK
import dense_conv_ref as DR
import det_ref
import grouped_conv_cases as GK
import grouped_conv_ref as GR
import theta_grad_cases as TK
import theta_grad_ref as TR
import train_kernel_cases as cases
import train_kernel_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
FMT = {"f32": 0, "s3": 1, "h2": 2}
NPL = {"s3": 3, "h2": 2}
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


@pytest.fixture(scope="module")
def lib():
    from sfh_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() if a is not None else None


def _sync():
    """a HIP error ends the run: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"GPU error, stopping: {err}", 3)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class _Buf:
    """n elements followed by a 64-element guard; starts as NaN or as `init` (numpy)"""

    def __init__(self, shape, dtype=np.float32, init=None):
        self.shape, self.n, self.dtype = tuple(shape), int(np.prod(shape)), dtype
        self.buf = torch.full((self.n + GUARD,), NAN, dtype=TORCH[dtype], device="cuda")
        self.init = None if init is None else np.ascontiguousarray(init, dtype=dtype).reshape(self.shape)
        if init is not None:
            self.buf[:self.n] = torch.from_numpy(self.init.reshape(-1)).cuda()

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def numpy(self):
        _sync()
        assert bool(torch.isnan(self.buf[self.n:]).all()), "the guard behind an output was written"
        return self.buf[:self.n].cpu().numpy().reshape(self.shape)

    def kept(self):
        """still what it started as (NaN, or init's bits)"""
        got = self.numpy()
        return bool(np.isnan(got).all()) if self.init is None else np.array_equal(_bits(got), _bits(self.init))


class _Busy:
    """an unrelated launch sequence on a side stream, started right before the call under test.  One launch moves 128 MB
    (about 0.03 ms on this device): 6 launches outlast a single kernel entry; `launches` = 2000 (about 70 ms of device time,
    enqueued in a few ms) outlasts a whole training step of this file, so the step runs beside it from end to end"""

    def __init__(self):
        self.side = torch.cuda.Stream()
        self.a = torch.ones(1 << 24, device="cuda")

    def start(self, launches=6):
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            for _ in range(launches):
                self.a.mul_(1.0000001)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.side)


_BUSY = []


def _busy():
    if not _BUSY:
        _BUSY.append(_Busy())
    return _BUSY[0]


def _det_launch(lib, name, query, E, dtype, call, accs, outs=()):
    """One deterministic entry, checks 1 and 3-6 of the file's docstring.
    query: arguments of NAME_det_bytes; E: elements per slab; dtype: the accumulator's numpy type;
    call(fn, acc_ptrs, out_ptrs, tail) -> rc, `tail` = the arguments behind the entry's own (workspace, bytes, stream);
    accs: [(init 2-D (rows, row_stride), slab offset, ncol, n_off)] - the slab part [offset, offset + rows * ncol) lands on
    columns [n_off, n_off + ncol) of the accumulator; outs: [(shape, numpy dtype)] overwritten outputs (start as NaN).
    -> (accumulators after the call, outputs, slabs (R, E))"""
    need = getattr(lib, name + "_det_bytes")(*query)
    item = np.dtype(dtype).itemsize
    assert need > 0 and need % (E * item) == 0, (name, query, need, E)
    Rn = need // (E * item)
    fn = getattr(lib, name + "_det")
    ws = _Buf((Rn * E,), dtype)                           # NaN-filled: an element the store pass misses poisons the sum

    def run(busy=False):
        a = [_Buf(i.shape, dtype, i) for (i, _, _, _) in accs]
        o = [_Buf(s, d) for (s, d) in outs]
        if busy:
            _busy().start()
        rc = call(fn, [x.ptr() for x in a], [x.ptr() for x in o], (ws.ptr(), need, _st()))
        if busy:
            _busy().join()
        _sync()
        assert rc == 0, (name, lib.sfh_last_error())
        return [x.numpy() for x in a], [x.numpy() for x in o]

    got, got_o = run()
    slabs = ws.numpy().reshape(Rn, E)
    assert not np.isnan(slabs).any(), f"{name}: a slab element was not written"
    for g, (init, off, ncol, n_off) in zip(got, accs):                         # 1. the order
        rows = init.shape[0]
        want = det_ref.det_sum_columns(np.ascontiguousarray(init, dtype=dtype), slabs[:, off:off + rows * ncol], ncol, n_off)
        assert np.array_equal(_bits(g), _bits(want)), f"{name}: not the ascending chain over the slabs"
    for tag, busy in (("again", False), ("busy side stream", True)):           # 3. and 4.
        g2, o2 = run(busy)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got + got_o, g2 + o2)), f"{name}: {tag}"
        assert np.array_equal(_bits(ws.numpy().reshape(Rn, E)), _bits(slabs)), f"{name}: slabs, {tag}"
    a = [_Buf(i.shape, dtype, i) for (i, _, _, _) in accs]                     # 6. one byte short
    o = [_Buf(s, d) for (s, d) in outs]
    wsn = _Buf((Rn * E,), dtype)
    for short in ((wsn.ptr(), need - 1, _st()), (None, need, _st())):
        assert call(fn, [x.ptr() for x in a], [x.ptr() for x in o], short) == -1, f"{name}: short workspace accepted"
    assert all(x.kept() for x in a + o) and bool(torch.isnan(wsn.buf).all()), f"{name}: a refused call wrote"
    return got, got_o, slabs


def _two_sums_bound(init, slabs_part):
    """the distance of two fp64 summations of the same R + 1 terms (dst0 and the R slab values), in any two orders"""
    Rn = slabs_part.shape[0]
    return 2.02 * (Rn + 1) * 2.0 ** -53 * (np.abs(init.reshape(-1)) + np.abs(slabs_part).sum(axis=0))


def _report(name, det, atomic):
    print(f"RATIO {name}: deterministic {det:.3f} atomic {atomic:.3f}")
    assert det <= 1.0 and atomic <= 1.0, (name, det, atomic)


# ------------------------------------------------------------------------------------------------ backward-filter, dense
def _split(lib, x, fmt, exp=2):
    B, H, W, cs = x.shape
    out = torch.full((B * H * W * cs * NPL[fmt],), 0x7FC1, dtype=torch.int16, device="cuda")
    if fmt == "s3":
        assert lib.sfh_f32_to_s3(_p(x), _p(out), B * H, W, cs, _st()) == 0, lib.sfh_last_error()
    else:
        assert lib.sfh_f32_to_h2(_p(x), _p(out), B * H, W, cs, exp, None, None, _st()) == 0, lib.sfh_last_error()
    return out


def _dense_sources(case, x0, x1):
    return [(x, n_off, pad) for x, n_off, pad in ((x0, 0, (0, 0)), (x1, case.N, case.pad)) if x is not None]


def _dense_wgrad(lib, case, dz, x0, x1, raw0, det):
    """the launches of one case (a second source at n_off = N), atomic or deterministic -> raw, splits per launch"""
    B, H, W, M = dz.shape
    kk, raw_n = case.ks * case.ks, raw0.shape[2]
    dzd = _dev(dz)
    dzs = dzd if case.kern == "f32" else _split(lib, dzd, case.kern)
    raw, splits = raw0, []
    for x, n_off, pad in _dense_sources(case, x0, x1):
        xd = _dev(x)
        _, xh, xw, N = x.shape
        xs = xd if case.kern == "f32" else _split(lib, xd, case.kern)

        def call(fn, acc, out, tail, xs=xs, xh=xh, xw=xw, N=N, pad=pad, n_off=n_off):
            if case.kern == "f32":
                return fn(_p(dzd), M, M, _p(xs), N, xh, xw, N, pad[0], pad[1], B, H, W, case.ks, acc[0], raw_n, n_off, *tail)
            return fn(_p(dzs), M, _p(xs), N, xh, xw, N, pad[0], pad[1], B, H, W, case.ks, acc[0], raw_n, n_off, FMT[case.kern],
                      *tail)
        if det:
            name, query = (("sfh_conv_wgrad", (M, N, xh, xw, N, pad[0], pad[1], B, H, W, case.ks)) if case.kern == "f32"
                           else ("sfh_conv_wgrad_s3", (M, N, B, H, W, case.ks)))
            (got,), _, slabs = _det_launch(lib, name, query, M * kk * N, np.float32, call,
                                           [(raw.reshape(M * kk, raw_n), 0, N, n_off)])
            splits.append(slabs.shape[0])
            raw = got.reshape(raw0.shape)
        else:
            buf = _Buf(raw.shape, np.float32, raw)
            fn = lib.sfh_conv_wgrad if case.kern == "f32" else lib.sfh_conv_wgrad_s3
            assert call(fn, [buf.ptr()], [], (_st(),)) == 0, lib.sfh_last_error()
            raw = buf.numpy()
    return raw, splits


@pytest.mark.parametrize("case", DK.WGRAD, ids=lambda c: c.name)
def test_dense_backward_filter(lib, case):
    """sfh_conv_wgrad_det / sfh_conv_wgrad_s3_det on the backward-filter cases of dense_conv_cases.py as they are (the 1x1 map -
    one tile, one slab; three frames; M 64 and 192; N 32 and 96; a second source through n_off; raw0 non-zero; both split
    formats): integers bit for bit the fp64 value, randn inside dense_conv_ref.wgrad's bound, next to the atomic form"""
    want, bound = None, None

    def ref(dz, x0, x1, raw0):
        w, b = raw0.astype(np.float64), np.zeros(raw0.shape)
        for x, n_off, pad in _dense_sources(case, x0, x1):
            sl = slice(n_off, n_off + x.shape[3])
            w[..., sl], b[..., sl] = DR.wgrad(dz, x, raw0[..., sl], case.ks, case.kern, pad)
        return w, b
    dz, x0, x1, raw0 = DK.wg_inputs(case, "int")
    want, _ = ref(dz, x0, x1, raw0)
    got, splits = _dense_wgrad(lib, case, dz, x0, x1, raw0, True)
    assert np.array_equal(got.astype(np.float64), want)
    dz, x0, x1, raw0 = DK.wg_inputs(case, "randn")
    want, bound = ref(dz, x0, x1, raw0)
    got, splits = _dense_wgrad(lib, case, dz, x0, x1, raw0, True)
    atom, _ = _dense_wgrad(lib, case, dz, x0, x1, raw0, False)
    print(f"SPLITS {case.name}: {splits}")
    if case.name.endswith("_1x1"):
        assert splits == [1]
    _report(f"{case.kern} backward-filter {case.name}", DR.ratio(got, want, bound), DR.ratio(atom, want, bound))


# ------------------------------------------------------------------------------------------------ backward-filter, grouped
@pytest.mark.parametrize("case", GK.CASES, ids=GK.case_id)
def test_grouped_backward_filter(lib, case):
    """sfh_conv_grouped_wgrad_det on every case of grouped_conv_cases.py (cg 4 .. 64 at strides 1 and 2, degenerate maps, tile
    edges, 240 tiles): integers bit for bit, randn inside grouped_conv_ref.wgrad_bound, next to the atomic form"""
    B, H, W, G, cg, s = case
    C = G * cg
    Rn, E = det_ref.grouped_slabs(B, H, W, G, cg, s)

    def run(x, dz, raw0, det):
        xd, dzd = _dev(x), _dev(dz)

        def call(fn, acc, out, tail):
            return fn(_p(dzd), _p(xd), acc[0], B, H, W, G, cg, s, *tail)
        if not det:
            buf = _Buf(raw0.shape, np.float32, raw0)
            assert call(lib.sfh_conv_grouped_wgrad, [buf.ptr()], [], (_st(),)) == 0
            return buf.numpy()
        (got,), _, slabs = _det_launch(lib, "sfh_conv_grouped_wgrad", (B, H, W, G, cg, s), E, np.float32, call,
                                       [(raw0.reshape(C * 9, cg), 0, cg, 0)])
        assert slabs.shape == (Rn, E)
        return got.reshape(raw0.shape)
    x, w, dz, raw0 = GK.int_inputs(case)
    assert np.array_equal(GR.raw_to_oihw(run(x, dz, raw0, True), cg).astype(np.float64),
                          GR.wgrad(dz, x, cg, s)[0] + GR.raw_to_oihw(raw0, cg))
    x, w, dz, raw0 = GK.randn_inputs(case)
    dw, Aw = GR.wgrad(dz, x, cg, s)
    r0 = GR.raw_to_oihw(raw0, cg).astype(np.float64)
    bound = GR.wgrad_bound(Aw, r0, *GK.wgrad_plan(case))
    _report(f"grouped backward-filter {GK.case_id(case)}", R.ratio(GR.raw_to_oihw(run(x, dz, raw0, True), cg), dw + r0, bound),
            R.ratio(GR.raw_to_oihw(run(x, dz, raw0, False), cg), dw + r0, bound))


# ------------------------------------------------------------------------------------------------ pixel reductions
RED_IDS = [f"{n}x{c}" for n, c in cases.REDUCTIONS]


def _atomic(lib, fn, dtype, call, inits, outs=()):
    a = [_Buf(i.shape, dtype, i) for i in inits]
    o = [_Buf(s, d) for (s, d) in outs]
    assert call(fn, [x.ptr() for x in a], [x.ptr() for x in o], (_st(),)) == 0, lib.sfh_last_error()
    return [x.numpy() for x in a], [x.numpy() for x in o]


@pytest.mark.parametrize("kind", cases.REDUCTION_DATA)
@pytest.mark.parametrize("shape", cases.REDUCTIONS, ids=RED_IDS)
def test_bn_stats(lib, shape, kind):
    """the cases and the bound of test_gpu_train_kernels.test_bn_stats (a single pixel .. the saturated grid of 1024 blocks, C up
    to 2048 in two chunks, the constant and the all-zero channel, the cancelling 100 + 0.01 randn)"""
    npix, C = shape
    c = cases.bn_case(npix, C, kind)
    s, A = c["stats"]
    pre = c["acc_pre"].numpy()
    bound = R.bn_stats_bound(npix, A, pre)
    z = c["z"].cuda()

    def call(fn, acc, out, tail):
        return fn(_p(z), npix, C, acc[0], *tail)
    (got,), _, slabs = _det_launch(lib, "sfh_bn_stats", (npix, C), 2 * C, np.float64, call, [(pre.reshape(1, 2 * C), 0, 2 * C, 0)])
    assert slabs.shape == det_ref.bn_slabs(npix, C)
    (atom,), _ = _atomic(lib, lib.sfh_bn_stats, np.float64, call, [pre.reshape(1, 2 * C)])
    _report(f"bn_stats {c['id']}", R.ratio(got.reshape(2, C), s + pre, bound), R.ratio(atom.reshape(2, C), s + pre, bound))


@pytest.mark.parametrize("kind", cases.REDUCTION_DATA)
@pytest.mark.parametrize("shape", cases.REDUCTIONS + [cases.COLSUM_SLICE], ids=RED_IDS + ["slice"])
def test_colsum(lib, shape, kind):
    npix, C, cs, c_off = shape if len(shape) == 4 else (shape[0], shape[1], shape[1], 0)
    c = cases.bn_case(npix, cs, kind)
    s, A = R.colsum_ref(c["z"], C, c_off)
    pre = c["acc_pre"][0, :C].numpy()
    bound = R.colsum_bound(npix, A, pre)
    z = c["z"].cuda()

    def call(fn, acc, out, tail):
        return fn(_p(z[:, c_off:]), npix, C, cs, acc[0], *tail)
    (got,), _, slabs = _det_launch(lib, "sfh_colsum", (npix, C), C, np.float64, call, [(pre.reshape(1, C), 0, C, 0)])
    assert slabs.shape == det_ref.colsum_slabs(npix, C)
    (atom,), _ = _atomic(lib, lib.sfh_colsum, np.float64, call, [pre.reshape(1, C)])
    _report(f"colsum {c['id']} C{C}", R.ratio(got.reshape(C), s + pre, bound), R.ratio(atom.reshape(C), s + pre, bound))


@pytest.mark.parametrize("mode", cases.BWD_MODES)
@pytest.mark.parametrize("kind", cases.REDUCTION_DATA)
@pytest.mark.parametrize("shape", cases.REDUCTIONS, ids=RED_IDS)
def test_bn_bwd_reduce(lib, shape, kind, mode):
    npix, C = shape
    c = cases.bn_case(npix, C, kind)
    y, relu = cases.bwd_inputs(c, mode)
    s, info = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
    pre = c["acc_pre"].numpy()
    bound = R.bn_bwd_reduce_bound(npix, info, pre)
    dev = {k: c[k].cuda() for k in ("dy", "z", "mi", "gamma", "beta")}
    yg = y.cuda() if y is not None else None

    def call(fn, acc, out, tail):
        return fn(_p(dev["dy"]), _p(yg), _p(dev["z"]), _p(dev["mi"]), _p(dev["gamma"]), _p(dev["beta"]), relu, npix, C, acc[0],
                  *tail)
    (got,), _, slabs = _det_launch(lib, "sfh_bn_bwd_reduce", (npix, C), 2 * C, np.float64, call,
                                   [(pre.reshape(1, 2 * C), 0, 2 * C, 0)])
    assert slabs.shape == det_ref.bn_slabs(npix, C)
    (atom,), _ = _atomic(lib, lib.sfh_bn_bwd_reduce, np.float64, call, [pre.reshape(1, 2 * C)])
    got, atom = got.reshape(2, C), atom.reshape(2, C)
    _report(f"bn_bwd_reduce {c['id']} {mode}",
            max(R.ratio(got[0], s[0] + pre[0], bound[0]), R.ratio(got[1], s[1] + pre[1], bound[1])),
            max(R.ratio(atom[0], s[0] + pre[0], bound[0]), R.ratio(atom[1], s[1] + pre[1], bound[1])))


@pytest.mark.parametrize("shape", cases.OUTCONV_SHAPES, ids=cases.ident)
def test_outconv_bwd(lib, shape):
    """nc 1 .. 8; a single pixel, a second block, a block across two frames, the 64-term flush"""
    B, H, W, cin, nc = shape
    c = cases.outconv_case(shape)
    r = R.outconv_bwd_ref(c["x"], c["w"], c["dl"])
    pw, pb = c["acc_w"].numpy(), c["acc_b"].numpy()
    b = R.outconv_bwd_bound(r, pw, pb)
    x, w, dl = c["x"].cuda(), c["w"].cuda(), c["dl"].cuda()

    def call(fn, acc, out, tail):
        return fn(_p(x), cin, _p(w), _p(dl), nc, B, H, W, out[0], acc[0], acc[1], *tail)
    outs = [((B * H * W, cin), np.float32)]
    Rn, E = det_ref.outconv_slabs(B * H * W, nc, cin)
    (gw, gb), (dx,), slabs = _det_launch(lib, "sfh_outconv_bwd", (cin, nc, B, H, W), E, np.float64, call,
                                         [(pw.reshape(1, nc * cin), 0, nc * cin, 0), (pb.reshape(1, nc), nc * cin, nc, 0)], outs)
    assert slabs.shape == (Rn, E)
    (aw, ab), (adx,) = _atomic(lib, lib.sfh_outconv_bwd, np.float64, call, [pw.reshape(1, -1), pb.reshape(1, -1)], outs)
    assert np.array_equal(_bits(dx), _bits(adx))
    _report(f"outconv_bwd {cases.ident(shape)}",
            max(R.ratio(gw.reshape(nc, cin), r["acc_w"] + pw, b["acc_w"]), R.ratio(gb.reshape(nc), r["acc_b"] + pb, b["acc_b"]),
                R.ratio(dx.astype(np.float64), r["dx"], b["dx"])),
            max(R.ratio(aw.reshape(nc, cin), r["acc_w"] + pw, b["acc_w"]), R.ratio(ab.reshape(nc), r["acc_b"] + pb, b["acc_b"]),
                R.ratio(adx.astype(np.float64), r["dx"], b["dx"])))


def _ratio0(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert not np.isnan(err).any() and (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


@pytest.mark.parametrize("shape", TK.AVGPOOL_SHAPES, ids=cases.ident)
def test_avgpool_linear_bwd(lib, shape):
    """the cases and bounds of test_gpu_theta_gradient.test_avgpool_linear_bwd; slab per frame"""
    B, H, W, C, nout = shape
    c = TK.avgpool_case(shape)
    r = TR.avgpool_linear_bwd_ref(c["x"], c["w"], c["d"])
    pw, pb = c["acc_w"].numpy(), c["acc_b"].numpy()
    xg, wg, dg = c["x"].cuda(), c["w"].cuda(), c["d"].cuda()

    def call(fn, acc, out, tail):
        return fn(_p(xg), _p(wg), _p(dg), B, H, W, C, nout, out[0], acc[0], acc[1], *tail)
    outs = [((B, H, W, C), np.float32)]
    Rn, E = det_ref.avgpool_slabs(B, C, nout)
    (gw, gb), (dx,), slabs = _det_launch(lib, "sfh_avgpool_linear_bwd", (B, C, nout), E, np.float64, call,
                                         [(pw.reshape(1, nout * C), 0, nout * C, 0), (pb.reshape(1, nout), nout * C, nout, 0)], outs)
    assert slabs.shape == (Rn, E)
    (aw, ab), (adx,) = _atomic(lib, lib.sfh_avgpool_linear_bwd, np.float64, call, [pw.reshape(1, -1), pb.reshape(1, -1)], outs)
    assert np.array_equal(_bits(dx), _bits(adx))
    bw, bb = (H * W + 1) * TR.U24 * r["a_w"], TR.U50 * r["a_b"]
    _report(f"avgpool_linear_bwd {shape}",
            max(_ratio0(np.abs(gw.reshape(nout, C) - (pw + r["acc_w"])), bw), _ratio0(np.abs(gb.reshape(nout) - (pb + r["acc_b"])), bb)),
            max(_ratio0(np.abs(aw.reshape(nout, C) - (pw + r["acc_w"])), bw), _ratio0(np.abs(ab.reshape(nout) - (pb + r["acc_b"])), bb)))


WARP_CASES = [c for f in TK.FRAMES for k in ("real0", "z_cross") for c in TK.warp_randn_cases(f, k)]


@pytest.mark.parametrize("c", WARP_CASES, ids=lambda c: c["id"])
def test_warp_bwd_theta(lib, c):
    """the frames of theta_grad_cases.py (2x2, 80x45, 257x5: one pixel in the second 256-column block and a ragged 4-row band,
    259x9, 640x6: three column blocks) with the realistic and the sign-changing theta, batch 1 / 3 / 17, shared and own
    templates, inside theta_grad_ref.warp_bound; slab per (column block, row band)"""
    B, h, w = c["theta"].shape[0], c["h"], c["w"]
    ht, wt = c["tmpl"].shape[2:]
    ref, A = TR.warp_bwd_theta_ref(c["theta"], c["tmpl"], h, w, c["dout"], c["shared"])
    pre = (torch.randn(B * 9, generator=torch.Generator().manual_seed(B)).double() * 0.5).numpy()
    bound = TR.warp_bound(ref, A) + 2.0 ** -52 * np.abs(pre.reshape(B, 9)) * (A > 0)
    th, tm, dout = c["theta"].cuda(), c["tmpl"].cuda(), c["dout"].cuda()

    def call(fn, acc, out, tail):
        return fn(_p(th), _p(tm), 0 if c["shared"] else ht * wt, ht, wt, B, h, w, _p(dout), acc[0], *tail)
    Rn, E = det_ref.warp_slabs(B, h, w)
    (got,), _, slabs = _det_launch(lib, "sfh_homography_warp_bwd_theta", (B, h, w), E, np.float64, call, [(pre.reshape(1, 9 * B), 0, 9 * B, 0)])
    assert slabs.shape == (Rn, E)
    (atom,), _ = _atomic(lib, lib.sfh_homography_warp_bwd_theta, np.float64, call, [pre.reshape(1, -1)])
    want = pre.reshape(B, 9) + ref
    _report(f"warp_bwd_theta {c['id']}", _ratio0(np.abs(got.reshape(B, 9) - want), bound), _ratio0(np.abs(atom.reshape(B, 9) - want), bound))


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 9, 13, 2), (3, 17, 31, 8), (2, 512, 513, 4)], ids=cases.ident)
def test_train_losses(lib, shape):
    """a single pixel; two blocks; nc 2, 4 and 8; 525,312 pixels: the saturated grid of 2048 blocks.  Held to the atomic form:
    both add the same R block sums onto the loaded loss words, in fp64"""
    B, H, W, nc = shape
    g = torch.Generator().manual_seed(B * H * W + nc)
    logits, warp = torch.randn(B, nc, H, W, generator=g).cuda(), torch.rand(B, H, W, generator=g).cuda()
    gt, wgt = torch.randint(0, nc, (B, H, W), generator=g).cuda(), (torch.rand(B, generator=g) + 0.5).cuda()
    pre = torch.randn(3, generator=g).double().numpy()

    def call(fn, acc, out, tail):
        return fn(_p(logits), _p(gt), _p(wgt), _p(warp), nc, B, H, W, 2.0, 2.0, 0, 1.0, 0, out[0], out[1], acc[0], *tail)
    outs = [((B, nc, H, W), np.float32), ((B, H, W), np.float32)]
    Rn, E = det_ref.losses_slabs(B * H * W)
    (got,), o, slabs = _det_launch(lib, "sfh_train_losses", (B, H, W), E, np.float64, call, [(pre.reshape(1, 3), 0, 3, 0)], outs)
    assert slabs.shape == (Rn, E)
    (atom,), ao = _atomic(lib, lib.sfh_train_losses, np.float64, call, [pre.reshape(1, 3)], outs)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(o, ao))
    r = _ratio0(np.abs(got - atom).reshape(-1), _two_sums_bound(pre, slabs))
    print(f"RATIO train_losses {shape}: deterministic against atomic {r:.3f}")
    assert r <= 1.0 and (got.reshape(-1) != pre).all()


@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 2, 9, 13), (2, 2, 260, 253)], ids=cases.ident)
def test_uv_loss(lib, shape):
    """a single pixel; two blocks; 263,120 elements: the saturated grid of 1024 blocks"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * H * W)
    uv, gt = torch.rand(B, C, H, W, generator=g).cuda(), torch.rand(B, C, H, W, generator=g).cuda()
    wgt = torch.tensor([1.5]).cuda()
    pre = torch.randn(1, generator=g).double().numpy()

    def call(fn, acc, out, tail):
        return fn(_p(uv), _p(gt), _p(wgt), 1, B, C, H, W, 2.0, 1, out[0], acc[0], *tail)
    outs = [(shape, np.float32)]
    Rn, E = det_ref.uv_slabs(B * C * H * W)
    (got,), o, slabs = _det_launch(lib, "sfh_uv_loss", shape, E, np.float64, call, [(pre.reshape(1, 1), 0, 1, 0)], outs)
    assert slabs.shape == (Rn, E)
    (atom,), ao = _atomic(lib, lib.sfh_uv_loss, np.float64, call, [pre.reshape(1, 1)], outs)
    assert np.array_equal(_bits(o[0]), _bits(ao[0]))
    r = _ratio0(np.abs(got - atom).reshape(-1), _two_sums_bound(pre, slabs))
    print(f"RATIO uv_loss {shape}: deterministic against atomic {r:.3f}")
    assert r <= 1.0 and got[0, 0] != pre[0]


@pytest.mark.parametrize("batch", TK.POI_BATCHES)
def test_reproj_loss(lib, batch):
    """1, 64, 65 and 130 frames: one block, a full block, a second and a third.  The atomic form adds one term per frame, the
    deterministic one adds the 64 frames of a block in frame order first: two fp64 summations of the same batch + 1 terms"""
    npts = 5
    g = torch.Generator().manual_seed(batch)
    poi, gt = torch.rand(batch, npts, 2, generator=g).cuda(), torch.rand(batch, npts, 2, generator=g).cuda()
    nz = (torch.rand(batch, npts, generator=g) > 0.3).float()
    nn_ = nz.sum(1).clamp(min=1.0).cuda()
    nz = nz.cuda()
    pre = torch.randn(1, generator=g).double().numpy()

    def call(fn, acc, out, tail):
        return fn(_p(poi), _p(gt), _p(nz), _p(nn_), batch, npts, 8.0, out[0], acc[0], *tail)
    outs = [((batch, npts, 2), np.float32)]
    Rn, E = det_ref.reproj_slabs(batch)
    (got,), o, slabs = _det_launch(lib, "sfh_reproj_loss", (batch,), E, np.float64, call, [(pre.reshape(1, 1), 0, 1, 0)], outs)
    assert slabs.shape == (Rn, E)
    (atom,), ao = _atomic(lib, lib.sfh_reproj_loss, np.float64, call, [pre.reshape(1, 1)], outs)
    assert np.array_equal(_bits(o[0]), _bits(ao[0]))
    bound = 2.02 * (batch + 1) * 2.0 ** -53 * (abs(pre[0]) + np.abs(slabs).sum())     # the terms are all of one sign
    assert abs(got[0, 0] - atom[0, 0]) <= bound and got[0, 0] != pre[0]


def test_det_reduce_order_on_cancelling_slabs(lib):
    """the sum pass alone, on slabs whose sum shows the order (1e8, 1, -1e8, 1, ... shuffled per column): the ascending chain of
    det_ref bit for bit, in both precisions, onto a loaded destination with a column offset"""
    for dtype, fn in ((np.float32, lib.sfh_det_reduce_f32), (np.float64, lib.sfh_det_reduce_f64)):
        for Rn, rows, ncol, raw_n, n_off in ((1, 1, 1, 1, 0), (7, 3, 5, 9, 2), (1024, 1, 24, 24, 0), (33, 64, 32, 96, 32)):
            E = rows * ncol
            p = det_ref.cancelling(Rn, E, dtype, seed=Rn)
            dst0 = np.random.default_rng(Rn).standard_normal((rows, raw_n)).astype(dtype)
            want = det_ref.det_sum_columns(dst0, p, ncol, n_off)
            pd = torch.from_numpy(p).cuda()
            dst = _Buf(dst0.shape, dtype, dst0)
            assert fn(_p(pd), Rn, E, E, ncol, ctypes.c_void_p(dst.buf.data_ptr() + n_off * np.dtype(dtype).itemsize), raw_n,
                      _st()) == 0, lib.sfh_last_error()
            got = dst.numpy()
            assert np.array_equal(_bits(got), _bits(want)), (dtype, Rn, rows, ncol)
            if Rn > 4:      # the order shows: the reversed chain gives other bits somewhere
                assert not np.array_equal(_bits(det_ref.det_sum_columns(dst0, p[::-1], ncol, n_off)), _bits(want))


# ------------------------------------------------------------------------------------------------ the whole step
H_, W_, B_ = 72, 128, 2


def _nb(kind):
    """frames per batch: 2; the UV model 1 - the reference's UV criterion broadcasts its per-sample weights along the last axis
    of a (B, W) map, which is legal for B == 1 or B == W only (sfh_uv_loss refuses the rest)"""
    return 1 if kind == "uv" else B_


def _net(kind, seed=47):
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    B = _nb(kind)
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :H_, :W_].contiguous()
    poi = synth.load_court_poi("pitch", B)
    kw = dict(target_size=(W_, H_), unet_size=(W_, H_), warp_size=(W_, H_))
    if kind == "uv":
        kw.update(unet_uv=True, resnet_input="img+mask+uv")
    if kind == "resnext":
        kw.update(resnet_name="resnext50_32x4d")
    net = Reconstructor(court.cuda(), poi.cuda(), **kw)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed))
    return net.cuda().train()


def _batches(net, n, uv):
    from sfh_amd import synth
    out = []
    npoi = net.court_poi.shape[1]
    B = 1 if uv else B_
    for k in range(n):
        g = torch.Generator().manual_seed(100 + k)
        b = {"mask": torch.randint(0, 4, (B, H_, W_), generator=g), "weight": torch.rand(B, generator=g) + 0.5,
             "poi": torch.rand(B, npoi, 2, generator=g), "nonzeros": (torch.rand(B, npoi, generator=g) > 0.3).float()}
        b["num_nonzero"] = b["nonzeros"].sum(1).clamp(min=1.0)
        if uv:
            b["uv"] = torch.rand(B, 2, H_, W_, generator=g)
        out.append((synth.smooth_frames(B, H_, W_, seed=60 + k).cuda(), {k_: v.cuda() for k_, v in b.items()}))
    return out


def _state(net, ts, losses):
    torch.cuda.synchronize()
    s = {f"p.{k}": v.detach().clone() for k, v in net.named_parameters()}
    s.update({f"b.{k}": v.detach().clone() for k, v in net.named_buffers()})
    for name, lst in (("g", ts.grads), ("sq", ts.sq), ("buf", ts.buf)):
        s.update({f"{name}.{i}": t.detach().clone() for i, t in enumerate(lst)})
    s["losses"] = losses.clone()
    return s


@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("kind", ["default", "uv", "resnext"])
def test_train_step_repeats_bit_for_bit(monkeypatch, kind, precision):
    """two models from one synthetic state dict, both under TrainStep(deterministic=True), three steps each on the same batches,
    the second beside a busy side stream: after every step every parameter, every entry of ts.grads / ts.sq / ts.buf, every
    BatchNorm running statistic and counter and the loss vector are torch.equal.  (The keyword does not exist without the
    feature.)  72x128, two frames; the UV model one frame (_nb).  The default mode never touches the workspace."""
    from sfh_amd.training import TrainStep
    monkeypatch.setenv("SFH_TRAIN_PRECISION", precision)
    uv = kind == "uv"
    runs = []
    for rep in range(2):
        net = _net(kind)
        ts = TrainStep(net, deterministic=True, uv_loss="MSE" if uv else None)
        assert ts.deterministic is True and ts.det_workspace_bytes == 0
        states, overlapped = [], 0
        for x, b in _batches(net, 3, uv):
            if rep:
                _busy().start(launches=2000)
            losses = ts.step(x, b)
            if rep:
                still = not _busy().side.query()      # the side stream outlasted the step's enqueue
                _busy().join()
                overlapped += still
            states.append(_state(net, ts, losses))
        assert ts.det_workspace_bytes > 0 and ts.range_fallbacks == 0
        assert "deterministic" not in ts.state_dict()
        if rep:
            print(f"side stream still busy when the step's last launch was enqueued: {overlapped} of 3 steps")
        runs.append((states, ts.det_workspace_bytes))
    (a, wa), (b, wb) = runs
    assert wa == wb
    print(f"det_workspace_bytes {kind} {precision}: {wa}")
    for step, (sa, sb) in enumerate(zip(a, b)):
        assert sorted(sa) == sorted(sb)
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not bad, (step, bad[:8], len(bad))
        assert bool(torch.isfinite(sa["losses"]).all())
    assert not torch.equal(a[0]["losses"], a[1]["losses"])          # the steps differ: the comparison is not vacuous
    net = _net(kind)
    ts = TrainStep(net, uv_loss="MSE" if uv else None)
    x, bt = _batches(net, 1, uv)[0]
    ts.step(x, bt)
    assert ts.deterministic is False and ts.det_workspace_bytes == 0


def _autograd_grads(net, x, batch, deterministic):
    from oracle import train_ref
    net.train_deterministic = deterministic
    net.zero_grad(set_to_none=True)
    preds = net(x)
    train_ref.losses(preds, batch, mask_classes=4)["total"].backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def test_autograd_node_repeats(monkeypatch):
    """under net.train_deterministic = True the autograd node of the whole model gives torch.equal parameter gradients twice"""
    monkeypatch.setenv("SFH_TRAIN_PRECISION", "f16x3")
    net = _net("default")
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x, batch = _batches(net, 1, False)[0]
    g1 = _autograd_grads(net, x, batch, True)
    net.load_state_dict(sd)
    g2 = _autograd_grads(net, x, batch, True)
    bad = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not bad, bad[:8]
    assert net.__dict__["_det_workspace"].nbytes > 0


def _e(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["resnet50", "resnext50_32x4d"])
def test_gradients_against_fp64_under_the_pass_own_relu_decisions(monkeypatch, name, precision):
    """Accuracy of the mode against fp64 autograd WITH THE PASS'S OWN RELU DECISIONS imposed (training.CAPTURE), the
    construction of tests/test_gpu_grouped_conv.py::_train_forward_errors (which says why: a ReLU input within 1e-8 of zero
    in the fp64 pass flips and puts 1e-4 .. 4e-3 into every upstream gradient, in both modes alike - an unmasked reference
    would let a leg that lost accuracy hide behind the flips).  train_forward on the STN alone (2 x 3 x 72 x 128), loss = a
    fixed random projection of theta and poi; a deterministic and a default pass are captured, each is held to
    grouped_conv_ref.resnet_stn(masks=its own decisions), and per tensor (theta, poi, every parameter gradient), with
    e = max |g - ref| / max |ref|: e_det <= 2 * e_default + 2^-20.  resnet50: the dense backward-filter legs (fp32 MFMA, and
    the split-operand kernel in f16x3); resnext50_32x4d: the grouped leg as well; BatchNorm sums, the pooled head and the
    stem in both.  training.CAPTURE records the ResNet's activations only: the UNet cannot be masked, its deterministic
    legs are held to fp64 per kernel above."""
    from sfh_amd import synth, training
    from sfh_amd.reconstructor import Reconstructor
    monkeypatch.setenv("SFH_TRAIN_PRECISION", precision)
    B, H, W = 2, 72, 128
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(None, poi.cuda(), use_unet=False, use_warper=False, resnet_input="img", resnet_name=name,
                        target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    sd = synth.synth_state_dict(net.state_dict(), 33)
    x = synth.smooth_frames(B, H, W, seed=33)
    g = torch.Generator().manual_seed(5)
    p_theta, p_poi = torch.randn(B, 1, 3, 3, generator=g), torch.randn(poi.shape, generator=g)
    open_ = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()
    refs = []          # (masks, reference outputs and gradients): a pass whose decisions equal an earlier one's shares it

    def reference(masks):
        for m, r in refs:
            if all(torch.equal(m[k], masks[k]) for k in masks):
                return r
        ref = {k: v.double().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
        theta = GR.resnet_stn(x.double(), ref, training=True, masks=masks)
        proj = GR.transform_poi(theta, poi.double())
        ((theta * p_theta.double()).sum() + (proj * p_poi.double()).sum()).backward()
        r = {"theta": theta.detach(), "poi": proj.detach()}
        r.update({k: v.grad for k, v in ref.items() if v.requires_grad})
        refs.append((masks, r))
        return r

    def errors(deterministic):
        net.load_state_dict(sd)
        net.cuda().train()
        net.train_deterministic = deterministic
        net.zero_grad(set_to_none=True)
        cap = training.CAPTURE = {}
        try:
            preds = net(x.cuda())
            ((preds["theta"] * p_theta.cuda()).sum() + (preds["poi"] * p_poi.cuda()).sum()).backward()
        finally:
            training.CAPTURE = None
        _sync()
        masks = {"resnet_reg.stem": open_(cap["stem"])}
        for k, v in cap.items():
            if k.startswith("layer"):
                masks.update({f"resnet_reg.{k}.{a}": open_(v[a]) for a in ("t1", "t", "out")})
        r = reference(masks)
        errs = {"theta": _e(preds["theta"], r["theta"].view_as(preds["theta"])), "poi": _e(preds["poi"], r["poi"])}
        errs.update({k: _e(p.grad, r[k]) for k, p in net.named_parameters()})
        return errs
    e_det, e_def = errors(True), errors(False)
    assert sorted(e_det) == sorted(e_def) and len(e_det) > 100
    for k in e_det:
        print(f"GRAD {name} {precision} {k}: deterministic {e_det[k]:.3e} default {e_def[k]:.3e}")
    print(f"WORST {name} {precision}: deterministic {max(e_det.values()):.3e} default {max(e_def.values()):.3e}; "
          f"references computed: {len(refs)}")
    bad = {k: (e_det[k], e_def[k]) for k in e_det if not e_det[k] <= 2.0 * e_def[k] + 2.0 ** -20}
    assert not bad, bad
