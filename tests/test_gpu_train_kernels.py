"""The plain training kernels of csrc/train_bn.hip and csrc/train_heads.hip - the anchor the fused kernels and the conv
epilogue sums are held to - one by one against the fp64 CPU references of tests/train_kernel_ref.py (which
tests/test_train_kernel_host.py holds against torch autograd), through the raw C entry points:

  sfh_bn_stats, sfh_bn_stats_partials, sfh_bn_finalize, sfh_bn_finalize_partials, sfh_bn_apply, sfh_bn_bwd_reduce,
  sfh_bn_bwd_apply, sfh_colsum, sfh_maxpool2_fwd, sfh_maxpool2_bwd, sfh_outconv_bwd, sfh_outconv_bwd_bn

and two siblings against those: sfh_bn_bwd_apply's launch with a split copy, and sfh_conv_wgrad_c4_bn against
sfh_bn_bwd_apply + sfh_conv_wgrad.

Every output buffer a test hands to a kernel ends in a guard of 64 sentinel elements that must come back untouched; an
output the kernel overwrites is pre-filled with NaN, one it accumulates into with non-zero values that the reference adds.
Every bound is derived (train_kernel_ref.py gives each rounding count) and built from the reference's own absolute sums;
an element whose bound is zero must be exact.  Each test prints its largest error / bound ratio (``pytest -s``).

Out of scope: NaN inputs of the max-pool backward.
"""
import math

import numpy as np
import pytest
import torch

import train_kernel_cases as cases
import train_kernel_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 777.25
NAN = float("nan")
EPS, MOM = cases.EPS, cases.MOMENTUM


@pytest.fixture(scope="module")
def K():
    """(lib, _ptr, _stream): the raw C entry points"""
    from sfh_amd import _lib
    from sfh_amd.engine import _ptr, _stream
    return _lib.load(), _ptr, _stream


class Guarded:
    """a device buffer of ``shape`` followed by GUARD sentinel elements; ``fill`` is a scalar or a CPU tensor"""

    def __init__(self, shape, dtype, fill):
        self.n = math.prod(shape)
        self.buf = torch.empty(self.n + GUARD, dtype=dtype, device="cuda")
        self.buf[self.n:] = SENTINEL
        self.guard = self.buf[self.n:].clone()              # as the dtype stores it
        self.t = self.buf[:self.n].view(*shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.to(dtype).reshape(shape))
        else:
            self.t.fill_(fill)

    def result(self):
        """the payload on the CPU, after checking that the guard is intact"""
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.n:], self.guard), "the kernel wrote behind its output"
        return self.t.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _report(name, **ratios):
    print(f"RATIO {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (name, ratios)


RED_IDS = [f"{n}x{c}" for n, c in cases.REDUCTIONS]


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("kind", cases.REDUCTION_DATA)
@pytest.mark.parametrize("shape", cases.REDUCTIONS, ids=RED_IDS)
def test_bn_stats(K, shape, kind):
    """acc (2,C) += [sum z | sum z^2] onto a loaded accumulator.  The terms are exact in fp64, npix additions in a free
    order: npix * (2^-53 + 2^-64) * (A + |pre|), A = sum |z| and sum z^2.  The constant channel, the all-zero channel (bound
    zero: the earlier content must come back exactly) and 100 + 0.01 randn included.  Two calls agree within the same bound
    (the order of the atomics is free)."""
    lib, _ptr, _stream = K
    npix, C = shape
    c = cases.bn_case(npix, C, kind)
    s, A = c["stats"]
    pre = c["acc_pre"].numpy()
    bound = R.bn_stats_bound(npix, A, pre)
    z = c["z"].cuda()
    got = []
    for _ in range(2):
        acc = Guarded((2, C), torch.float64, c["acc_pre"])
        assert lib.sfh_bn_stats(_ptr(z), npix, C, _ptr(acc.t), _stream()) == 0
        got.append(acc.result().numpy())
    assert (bound[:, 2] == 0).all()
    _report(f"bn_stats {c['id']}", ref=R.ratio(got[0], s + pre, bound), again=R.ratio(got[1], got[0], bound))


@pytest.mark.parametrize("kind", cases.REDUCTION_DATA)
@pytest.mark.parametrize("shape", cases.REDUCTIONS + [cases.COLSUM_SLICE], ids=RED_IDS + ["slice"])
def test_colsum(K, shape, kind):
    """acc (C,) += sum x over the pixels, the same cases and bound as the first row of bn_stats; and a slice of 32 channels at
    offset 32 of a 96-channel tensor (cs > C)"""
    lib, _ptr, _stream = K
    npix, C, cs, c_off = shape if len(shape) == 4 else (shape[0], shape[1], shape[1], 0)
    c = cases.bn_case(npix, cs, kind)
    s, A = R.colsum_ref(c["z"], C, c_off)
    pre = c["acc_pre"][0, :C]
    bound = R.colsum_bound(npix, A, pre.numpy())
    z = c["z"].cuda()
    got = []
    for _ in range(2):
        acc = Guarded((C,), torch.float64, pre)
        assert lib.sfh_colsum(_ptr(z[:, c_off:]), npix, C, cs, _ptr(acc.t), _stream()) == 0
        got.append(acc.result().numpy())
    _report(f"colsum {c['id']} C{C}", ref=R.ratio(got[0], s + pre.numpy(), bound), again=R.ratio(got[1], got[0], bound))


@pytest.mark.parametrize("C", cases.PARTIAL_C)
@pytest.mark.parametrize("rows", cases.PARTIAL_ROWS)
def test_bn_stats_partials(K, rows, C):
    """acc (2C,) += sum over the rows of a (rows, 2C) fp64 table: rows * (2^-53 + 2^-64) * (sum |partial| + |pre|).  Rows
    around the 4 row lanes and the 32-row-block grid (128), columns around the 64 of a block."""
    lib, _ptr, _stream = K
    c = cases.partials_case(rows, C)
    table = c["partial"].reshape(rows, 2 * C)
    s, A = R.bn_stats_partials_ref(table.numpy())
    pre = c["acc_pre"].numpy()
    acc = Guarded((2 * C,), torch.float64, c["acc_pre"])
    tg = table.cuda()
    assert lib.sfh_bn_stats_partials(_ptr(tg), rows, C, _ptr(acc.t), _stream()) == 0
    _report(f"bn_stats_partials {rows}x{C}", ref=R.ratio(acc.result().numpy(), s + pre, R.bn_stats_partials_bound(rows, A, pre)))


# ------------------------------------------------------------------------------------------------ finalize
def _finalize_outputs(c, C, running, counter):
    mi = Guarded((2 * C,), torch.float32, NAN)
    rm = Guarded((C,), torch.float32, c["running_mean"]) if running else None
    rv = Guarded((C,), torch.float32, c["running_var"]) if running else None
    cnt = Guarded((1,), torch.int64, 41) if counter else None
    return mi, rm, rv, cnt


def _check_finalize(name, r, b, C, mi, rm, rv, cnt):
    got = mi.result().double().numpy()
    ratios = {"mean": R.ratio(got[:C], r["mean"], b["mean"]), "invstd": R.ratio(got[C:], r["invstd"], b["invstd"])}
    if rm is not None:
        ratios["running_mean"] = R.ratio(rm.result().double().numpy(), r["running_mean"], b["running_mean"])
        ratios["running_var"] = R.ratio(rv.result().double().numpy(), r["running_var"], b["running_var"])
    if cnt is not None:
        assert int(cnt.result()[0]) == 42                      # advances by exactly 1
    _report(name, **ratios)
    return got


@pytest.mark.parametrize("counter", [True, False], ids=["cnt", "nocnt"])
@pytest.mark.parametrize("running", [True, False], ids=["run", "norun"])
@pytest.mark.parametrize("npix", cases.FINALIZE_NPIX)
@pytest.mark.parametrize("C", cases.FINALIZE_C)
def test_bn_finalize(K, C, npix, running, counter):
    """mean, invstd and the running statistics from given sums, against exact rational arithmetic (bn_finalize_ref):
    mean u |ref| + 2^-53 |ref|; invstd u |ref| + invstd^3 / 2 * e_var + 6 * 2^-53 |ref|, e_var the three fp64 roundings of
    acc1 / n - mean^2; the running pair u |ref| + the propagated error (bn_finalize_bound).  Channel 0's variance rounds
    below zero and is clamped: invstd = 1 / sqrt(eps).  npix = 1: the unbiased variance is the biased one.  The running
    pair and the counter may be NULL."""
    lib, _ptr, _stream = K
    c = cases.finalize_case(C, npix)
    rmc, rvc = (c["running_mean"], c["running_var"]) if running else (None, None)
    r = R.bn_finalize_ref(c["acc"].numpy(), npix, EPS, MOM, rmc, rvc)
    b = R.bn_finalize_bound(r, npix, EPS, MOM)
    mi, rm, rv, cnt = _finalize_outputs(c, C, running, counter)
    acc = c["acc"].cuda()
    assert lib.sfh_bn_finalize(_ptr(acc), npix, C, EPS, MOM, _ptr(rm.t) if running else None, _ptr(rv.t) if running else None,
                               _ptr(mi.t), _ptr(cnt.t) if counter else None, _stream()) == 0
    got = _check_finalize(f"bn_finalize C{C} n{npix}", r, b, C, mi, rm, rv, cnt)
    assert got[C] == np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))


@pytest.mark.parametrize("which", ["mean_only", "var_only"])
def test_bn_finalize_refuses_half_a_running_pair(K, which):
    """a running pair with one pointer is refused with -1 by both entry points, and nothing is written"""
    lib, _ptr, _stream = K
    C, rows = 33, 5
    c = cases.partials_case(rows, C)
    for partials in (False, True):
        mi, rm, rv, cnt = _finalize_outputs(c, C, True, True)
        p_rm, p_rv = (_ptr(rm.t), None) if which == "mean_only" else (None, _ptr(rv.t))
        if partials:
            tg = c["partial"].cuda()
            rc = lib.sfh_bn_finalize_partials(_ptr(tg), rows, c["npix"], C, EPS, MOM, p_rm, p_rv, _ptr(mi.t), _ptr(cnt.t), _stream())
        else:
            acc = c["partial"].sum(dim=0).cuda()
            rc = lib.sfh_bn_finalize(_ptr(acc), c["npix"], C, EPS, MOM, p_rm, p_rv, _ptr(mi.t), _ptr(cnt.t), _stream())
        assert rc == -1
        assert bool(torch.isnan(mi.result()).all()) and int(cnt.result()[0]) == 41
        assert torch.equal(rm.result(), c["running_mean"]) and torch.equal(rv.result(), c["running_var"])


@pytest.mark.parametrize("C", cases.PARTIAL_C)
@pytest.mark.parametrize("rows", cases.PARTIAL_ROWS)
def test_bn_finalize_partials(K, rows, C):
    """the (rows, 2, C) table summed in a fixed order and finalized in one launch: bn_finalize's bounds with the sums' own
    rows * (2^-53 + 2^-64) * sum |partial| carried through.  Rows around the 16 row lanes, channels around the 64 of a
    workgroup.  No atomics: two calls give the same bits.  Once more with the running pair and the counter NULL."""
    lib, _ptr, _stream = K
    c = cases.partials_case(rows, C)
    r, A = R.bn_finalize_partials_ref(c["partial"].numpy(), c["npix"], EPS, MOM, c["running_mean"], c["running_var"])
    b = R.bn_finalize_partials_bound(r, A, rows, c["npix"], EPS, MOM)
    tg = c["partial"].cuda()
    outs = []
    for _ in range(2):
        mi, rm, rv, cnt = _finalize_outputs(c, C, True, True)
        assert lib.sfh_bn_finalize_partials(_ptr(tg), rows, c["npix"], C, EPS, MOM, _ptr(rm.t), _ptr(rv.t), _ptr(mi.t),
                                            _ptr(cnt.t), _stream()) == 0
        _check_finalize(f"bn_finalize_partials {rows}x{C}", r, b, C, mi, rm, rv, cnt)
        outs.append((mi.result(), rm.result(), rv.result()))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(*outs))
    mi, _, _, _ = _finalize_outputs(c, C, False, False)
    assert lib.sfh_bn_finalize_partials(_ptr(tg), rows, c["npix"], C, EPS, MOM, None, None, _ptr(mi.t), None, _stream()) == 0
    assert torch.equal(_bits(mi.result()), _bits(outs[0][0]))


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("shape", cases.APPLY_SHAPES, ids=cases.ident)
def test_bn_apply(K, shape, with_res, relu):
    """y = [relu]((z - mean) * invstd * gamma + beta [+ residual]) per element:
    1.01 * u * (3 |xh gamma| + |xh gamma + beta| [+ |pre| with a residual]) - three roundings in front of the product with
    gamma, one for + beta, one for the residual; ReLU is 1-Lipschitz.  The constant and the all-zero channel have beta = 0:
    without a residual their bound is zero and y an exact zero."""
    lib, _ptr, _stream = K
    c = cases.shape_case(shape)
    r = R.bn_apply_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["residual"] if with_res else None, relu)
    y = Guarded((c["npix"], c["C"]), torch.float32, NAN)
    dev = {k: c[k].cuda() for k in ("z", "mi", "gamma", "beta", "residual")}
    assert lib.sfh_bn_apply(_ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]),
                            _ptr(dev["residual"]) if with_res else None, relu, c["npix"], c["C"], _ptr(y.t), None, 0, 0, None,
                            _stream()) == 0
    _report(f"bn_apply {c['id']} res{int(with_res)} relu{relu}", y=R.ratio(y.result().double().numpy(), r["y"], R.bn_apply_bound(r)))


@pytest.mark.parametrize("fmt", ["s3", "h2"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("shape", cases.SPLIT_SHAPES, ids=cases.ident)
def test_bn_apply_split_launch(K, shape, with_res, fmt):
    """the launch that also writes the split copy (C % 32 == 0): its fp32 y has the plain launch's bits (and so its bound,
    asserted too), its planes are engine.f32_to_split of that y bit for bit in both formats, with y == NULL the planes are the
    same, and the overflow word stays 0"""
    from sfh_amd import engine as E
    lib, _ptr, _stream = K
    B, H, W, C = shape
    c = cases.shape_case(shape)
    npix = c["npix"]
    r = R.bn_apply_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["residual"] if with_res else None, 1)
    dev = {k: c[k].cuda() for k in ("z", "mi", "gamma", "beta", "residual")}
    res = _ptr(dev["residual"]) if with_res else None
    args = (_ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]), res, 1, npix, C)
    plain = Guarded((B, H, W, C), torch.float32, NAN)
    assert lib.sfh_bn_apply(*args, _ptr(plain.t), None, 0, 0, None, _stream()) == 0
    want = plain.result()
    _report(f"bn_apply split {c['id']} {fmt}", y=R.ratio(want.double().numpy().reshape(npix, C), r["y"], R.bn_apply_bound(r)))
    planes_want = E.f32_to_split(plain.t, fmt).cpu()
    dtype, _, code = E._SPLIT[fmt]
    for with_y in (True, False):
        y = Guarded((B, H, W, C), torch.float32, NAN)
        planes = Guarded(tuple(planes_want.shape), dtype, NAN)
        over = Guarded((1,), torch.int32, 0)
        assert lib.sfh_bn_apply(*args, _ptr(y.t) if with_y else None, _ptr(planes.t), W, code, _ptr(over.t), _stream()) == 0
        assert torch.equal(_bits(planes.result()), _bits(planes_want)), (fmt, with_y)
        assert int(over.result()[0]) == 0
        if with_y:
            assert torch.equal(_bits(y.result()), _bits(want))
        else:
            assert bool(torch.isnan(y.result()).all())


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("mode", cases.BWD_MODES)
@pytest.mark.parametrize("kind", cases.REDUCTION_DATA)
@pytest.mark.parametrize("shape", cases.REDUCTIONS, ids=RED_IDS)
def test_bn_bwd_reduce(K, shape, kind, mode):
    """acc (2,C) += [sum g | sum g xhat] onto a loaded accumulator; g = dy (relu = 0), dy * (y > 0) with y read (exact
    decision), or with the decision recomputed from z (y == NULL: an element whose fp64 pre-activation lies within the forward
    bound of zero may fall either way and adds its own |dy|, |dy xhat| to the bounds; the exact zeros of the constant and the
    all-zero channel are not ambiguous: g = 0).
    s0: npix * (2^-53 + 2^-64) * (sum |g| + |pre|); s1: (2u + u^2) * sum |g xhat| (xhat's two fp32 roundings) + the same fp64 term."""
    lib, _ptr, _stream = K
    npix, C = shape
    c = cases.bn_case(npix, C, kind)
    y, relu = cases.bwd_inputs(c, mode)
    s, info = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
    assert info["namb"] <= R.AMBIGUITY_CAP * npix * C
    pre = c["acc_pre"].numpy()
    bound = R.bn_bwd_reduce_bound(npix, info, pre)
    dev = {k: c[k].cuda() for k in ("dy", "z", "mi", "gamma", "beta")}
    yg = y.cuda() if y is not None else None
    acc = Guarded((2, C), torch.float64, c["acc_pre"])
    assert lib.sfh_bn_bwd_reduce(_ptr(dev["dy"]), _ptr(yg), _ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]),
                                 relu, npix, C, _ptr(acc.t), _stream()) == 0
    got = acc.result().numpy()
    _report(f"bn_bwd_reduce {c['id']} {mode}", s0=R.ratio(got[0], s[0] + pre[0], bound[0]), s1=R.ratio(got[1], s[1] + pre[1], bound[1]))


@pytest.mark.parametrize("outputs", cases.BWD_OUTPUTS, ids=lambda o: f"dres{o[0]}-f32{o[1]}")
@pytest.mark.parametrize("mode", cases.BWD_MODES)
@pytest.mark.parametrize("shape", cases.APPLY_SHAPES, ids=cases.ident)
def test_bn_bwd_apply(K, shape, mode, outputs):
    """dz = gamma * invstd * (g - mg - xhat * mgx) per element, from the reference's own sums as acc:
    1.01 * u * |gamma invstd| * (3 |mg| + |g - mg| + 6 |c| + 3 |g - mg - c|), c = xhat * mgx (bn_bwd_apply_bound counts the
    roundings; the kernel multiplies by a rounded 1 / npix), + |gamma invstd dy| on an ambiguous element.  dres is g bit for
    bit, acc_f32 is acc.float() bit for bit; both are optional."""
    lib, _ptr, _stream = K
    want_dres, want_f32 = outputs
    c = cases.shape_case(shape)
    npix, C = c["npix"], c["C"]
    y, relu = cases.bwd_inputs(c, mode)
    s, _ = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
    acc = torch.from_numpy(s.astype(np.float64).reshape(-1))
    r = R.bn_bwd_apply_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], acc, relu, npix)
    assert r["amb"].sum() <= R.AMBIGUITY_CAP * npix * C
    dev = {k: c[k].cuda() for k in ("dy", "z", "mi", "gamma", "beta")}
    yg, accg = (y.cuda() if y is not None else None), acc.cuda()
    dz = Guarded((npix, C), torch.float32, NAN)
    dres = Guarded((npix, C), torch.float32, NAN) if want_dres else None
    a32 = Guarded((2 * C,), torch.float32, NAN) if want_f32 else None
    assert lib.sfh_bn_bwd_apply(_ptr(dev["dy"]), _ptr(yg), _ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]),
                                _ptr(accg), relu, npix, C, _ptr(dz.t), _ptr(dres.t) if want_dres else None, None, 0, 0, None,
                                _ptr(a32.t) if want_f32 else None, _stream()) == 0
    _report(f"bn_bwd_apply {c['id']} {mode}", dz=R.ratio(dz.result().double().numpy(), r["dz"], R.bn_bwd_apply_bound(r)))
    if want_dres:
        g = dres.result().numpy()
        keep = ~r["amb"]
        assert np.array_equal(g[keep], r["g"].astype(np.float32)[keep])
        assert ((g == 0) | (g == c["dy"].numpy()))[r["amb"]].all()
    if want_f32:
        assert torch.equal(_bits(a32.result()), _bits(acc.float()))


# ------------------------------------------------------------------------------------------------ max-pool 2x2
@pytest.mark.parametrize("kind", cases.POOL_DATA)
@pytest.mark.parametrize("shape", cases.POOL_SHAPES, ids=cases.ident)
def test_maxpool2_fwd(K, shape, kind):
    """bit for bit against the reference (F.max_pool2d's values): randn, ties (halves, a constant), mixed +0 / -0 - the
    project's nesting max(max(a, b), max(c, d)) with the later operand kept on a tie decides the sign of a zero -, and a NaN,
    which propagates"""
    lib, _ptr, _stream = K
    B, H, W, C = shape
    c = cases.pool_case(shape, kind)
    want = torch.from_numpy(R.maxpool2_fwd_ref(c["x"].numpy()))
    y = Guarded(tuple(want.shape), torch.float32, NAN)
    x = c["x"].cuda()
    assert lib.sfh_maxpool2_fwd(_ptr(x), _ptr(y.t), B, H, W, C, _stream()) == 0
    got = y.result()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert int(torch.isnan(want).sum()) == (2 if kind == "nan" else 0)
    ok = ~torch.isnan(want)
    assert torch.equal(_bits(got)[ok], _bits(want)[ok])


@pytest.mark.parametrize("kind", [k for k in cases.POOL_DATA if k != "nan"])
@pytest.mark.parametrize("shape", cases.POOL_SHAPES, ids=cases.ident)
def test_maxpool2_bwd(K, shape, kind):
    """bit for bit against the reference: dy goes to the first maximum of its window in scan order.  Even sizes into a
    NaN-filled buffer: every element is written.  Any size with accumulate: one fp32 addition onto the earlier content; a
    cropped last row / column keeps it exactly.  Odd sizes without accumulate are refused with -1 and nothing is written."""
    lib, _ptr, _stream = K
    B, H, W, C = shape
    c = cases.pool_case(shape, kind)
    x, dy = c["x"].cuda(), c["dy"].cuda()
    fresh = Guarded(shape, torch.float32, NAN)
    rc = lib.sfh_maxpool2_bwd(_ptr(x), _ptr(dy), _ptr(fresh.t), B, H, W, C, 0, _stream())
    if H % 2 == 0 and W % 2 == 0:
        assert rc == 0
        assert torch.equal(_bits(fresh.result()), _bits(torch.from_numpy(R.maxpool2_bwd_ref(c["x"].numpy(), c["dy"].numpy()))))
    else:
        assert rc == -1 and bool(torch.isnan(fresh.result()).all())
    acc = Guarded(shape, torch.float32, c["pre"])
    assert lib.sfh_maxpool2_bwd(_ptr(x), _ptr(dy), _ptr(acc.t), B, H, W, C, 1, _stream()) == 0
    want = torch.from_numpy(R.maxpool2_bwd_ref(c["x"].numpy(), c["dy"].numpy(), c["pre"].numpy()))
    got = acc.result()
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(got[:, H // 2 * 2:], c["pre"][:, H // 2 * 2:]) and torch.equal(got[:, :, W // 2 * 2:], c["pre"][:, :, W // 2 * 2:])


# ------------------------------------------------------------------------------------------------ OutConv backward
def _outconv_buffers(c, shape, want_dx=True):
    B, H, W, cin, nc = shape
    return (Guarded((B * H * W, cin), torch.float32, NAN) if want_dx else None,
            Guarded((nc, cin), torch.float64, c["acc_w"]), Guarded((nc,), torch.float64, c["acc_b"]))


@pytest.mark.parametrize("shape", cases.OUTCONV_SHAPES + [cases.OUTCONV_NO_DX],
                         ids=list(map(cases.ident, cases.OUTCONV_SHAPES)) + ["no_dx"])
def test_outconv_bwd(K, request, shape):
    """dx = sum_k dl_k w_k: nc * u * sum |dl w| (+ the reference's nc * 2^-53); acc_w += sum_p dl x: 64 * u * sum |dl x| - a
    thread's fp32 chain is promoted to fp64 in front of its 65th term - + npix * 2^-53 * (sum |dl x| + |pre|); acc_b: 63 * u *
    sum |dl| and the same fp64 term.  A single pixel; 3 quads; a second block; a block across two frames; the 64-term flush;
    and dx == NULL."""
    lib, _ptr, _stream = K
    B, H, W, cin, nc = shape
    want_dx = request.node.callspec.id != "no_dx"
    c = cases.outconv_case(shape)
    r = R.outconv_bwd_ref(c["x"], c["w"], c["dl"])
    b = R.outconv_bwd_bound(r, c["acc_w"].numpy(), c["acc_b"].numpy())
    dx, acc_w, acc_b = _outconv_buffers(c, shape, want_dx)
    x, w, dl = c["x"].cuda(), c["w"].cuda(), c["dl"].cuda()
    assert lib.sfh_outconv_bwd(_ptr(x), cin, _ptr(w), _ptr(dl), nc, B, H, W, _ptr(dx.t) if want_dx else None, _ptr(acc_w.t),
                               _ptr(acc_b.t), _stream()) == 0
    ratios = {"acc_w": R.ratio(acc_w.result().numpy(), r["acc_w"] + c["acc_w"].numpy(), b["acc_w"]),
              "acc_b": R.ratio(acc_b.result().numpy(), r["acc_b"] + c["acc_b"].numpy(), b["acc_b"])}
    if want_dx:
        ratios["dx"] = R.ratio(dx.result().double().numpy(), r["dx"], b["dx"])
    _report(f"outconv_bwd {request.node.callspec.id}", **ratios)


@pytest.mark.parametrize("shape", cases.OUTCONV_SHAPES, ids=cases.ident)
def test_outconv_bwd_bn(K, shape):
    """x = relu(bn(z)) recomputed in the pass, within e_x (bn_apply's bound): acc_w gains 1.01 * sum |dl| e_x; dx and acc_b as
    sfh_outconv_bwd.  acc_bn (2,cin) += [sum g | sum g xhat], g = the kernel's own dx where x > 0: bounded as bn_bwd_reduce with
    dx's error carried through and the ambiguous decisions added (outconv_bwd_bn_bound)."""
    lib, _ptr, _stream = K
    B, H, W, cin, nc = shape
    c = cases.outconv_case(shape)
    r = R.outconv_bwd_bn_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["w"], c["dl"])
    assert r["namb"] <= R.AMBIGUITY_CAP * r["npix"] * cin
    b = R.outconv_bwd_bn_bound(r, c["acc_w"].numpy(), c["acc_b"].numpy(), c["acc_bn"].numpy())
    dx, acc_w, acc_b = _outconv_buffers(c, shape)
    acc_bn = Guarded((2, cin), torch.float64, c["acc_bn"])
    dev = {k: c[k].cuda() for k in ("z", "mi", "gamma", "beta", "w", "dl")}
    assert lib.sfh_outconv_bwd_bn(_ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]), cin, _ptr(dev["w"]),
                                  _ptr(dev["dl"]), nc, B, H, W, _ptr(dx.t), _ptr(acc_w.t), _ptr(acc_b.t), _ptr(acc_bn.t),
                                  _stream()) == 0
    _report(f"outconv_bwd_bn {cases.ident(shape)}",
            dx=R.ratio(dx.result().double().numpy(), r["dx"], b["dx"]),
            acc_w=R.ratio(acc_w.result().numpy(), r["acc_w"] + c["acc_w"].numpy(), b["acc_w"]),
            acc_b=R.ratio(acc_b.result().numpy(), r["acc_b"] + c["acc_b"].numpy(), b["acc_b"]),
            acc_bn=R.ratio(acc_bn.result().numpy(), r["acc_bn"] + c["acc_bn"].numpy(), b["acc_bn"]))


# ------------------------------------------------------------------------------------------------ siblings of bn_bwd_apply
def _bwd_acc(c, mode):
    """the reference's own backward sums as the fp64 accumulator [sum g | sum g xhat] the apply kernels read"""
    y, relu = cases.bwd_inputs(c, mode)
    s, _ = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
    return torch.from_numpy(s.astype(np.float64).reshape(-1))


@pytest.mark.parametrize("fmt", ["s3", "h2"])
@pytest.mark.parametrize("mode", cases.BWD_MODES)
@pytest.mark.parametrize("shape", cases.SPLIT_SHAPES, ids=cases.ident)
def test_bn_bwd_apply_split_launch(K, shape, mode, fmt):
    """the launch that also writes the split copy of dz (C % 32 == 0), the mirror of test_bn_apply_split_launch: its fp32 dz
    and dres have the plain launch's bits (whose bound test_bn_bwd_apply asserts), its planes are engine.f32_to_split of the
    plain launch's dz bit for bit in both formats, with dz == NULL the planes and dres are the same, acc_f32 is acc.float(),
    and the overflow word stays 0"""
    from sfh_amd import engine as E
    lib, _ptr, _stream = K
    B, H, W, C = shape
    c = cases.shape_case(shape)
    npix = c["npix"]
    y, relu = cases.bwd_inputs(c, mode)
    acc = _bwd_acc(c, mode)
    dev = {k: c[k].cuda() for k in ("dy", "z", "mi", "gamma", "beta")}
    yg, accg = (y.cuda() if y is not None else None), acc.cuda()
    args = (_ptr(dev["dy"]), _ptr(yg), _ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]), _ptr(accg), relu,
            npix, C)
    plain, plain_res = Guarded((B, H, W, C), torch.float32, NAN), Guarded((B, H, W, C), torch.float32, NAN)
    assert lib.sfh_bn_bwd_apply(*args, _ptr(plain.t), _ptr(plain_res.t), None, 0, 0, None, None, _stream()) == 0
    want, want_res = plain.result(), plain_res.result()
    planes_want = E.f32_to_split(plain.t, fmt).cpu()
    dtype, _, code = E._SPLIT[fmt]
    for with_dz in (True, False):
        dz, dres = Guarded((B, H, W, C), torch.float32, NAN), Guarded((B, H, W, C), torch.float32, NAN)
        planes = Guarded(tuple(planes_want.shape), dtype, NAN)
        over = Guarded((1,), torch.int32, 0)
        a32 = Guarded((2 * C,), torch.float32, NAN)
        assert lib.sfh_bn_bwd_apply(*args, _ptr(dz.t) if with_dz else None, _ptr(dres.t), _ptr(planes.t), W, code, _ptr(over.t),
                                    _ptr(a32.t), _stream()) == 0
        assert torch.equal(_bits(planes.result()), _bits(planes_want)), (fmt, with_dz)
        assert int(over.result()[0]) == 0
        assert torch.equal(_bits(dres.result()), _bits(want_res))
        assert torch.equal(_bits(a32.result()), _bits(acc.float()))
        if with_dz:
            assert torch.equal(_bits(dz.result()), _bits(want))
        else:
            assert bool(torch.isnan(dz.result()).all())


WGRAD_C4_ONE_TILE = [(1, 8, 8), (1, 4, 16), (1, 2, 32), (1, 3, 5)]      # one 8x8, 4x16, 2x32 tile; a cropped one
WGRAD_C4_TILES = [(2, 9, 20), (3, 7, 37)]
WGRAD_C4_M = [12, 72]                                                    # one partial channel block; two, the second partial


@pytest.mark.parametrize("M", WGRAD_C4_M)
@pytest.mark.parametrize("frame", WGRAD_C4_ONE_TILE + WGRAD_C4_TILES, ids=cases.ident)
def test_conv_wgrad_c4_bn_vs_two_passes(K, frame, M):
    """sfh_conv_wgrad_c4_bn (the first layer's BatchNorm backward applied while the gradient tiles are loaded) against the two
    passes it replaces: sfh_bn_bwd_apply with the ReLU decision recomputed from z and the same acc, then sfh_conv_wgrad on
    the first-layer shape (x_cs = 4; the three input channels of the fused call are stored as four with a zero, which the
    plain entry point, N % 4 == 0, takes as N = 4: its fourth column multiplies zeros and the three real ones are compared).
    raw is zeroed.  A single-tile frame: every address receives exactly one add, the bits are equal.  Several tiles: the order
    of the fp32 atomics is free, |a - b| <= 2.02 * n * 2^-24 * S per output, n = B * H * W and S the fp64 sum of |dz x| over the
    pixels of that (m, tap, c) from the two-pass dz - the bound between two fp32 summations of the same n terms."""
    lib, _ptr, _stream = K
    B, H, W = frame
    c = cases.bn_case(B * H * W, M, "randn")
    npix = c["npix"]
    acc = _bwd_acc(c, "recompute")
    g = torch.Generator().manual_seed(1000 * npix + M)
    x = torch.randn(B, H, W, 4, generator=g)
    x[..., 3] = 0.0
    dev = {k: c[k].cuda() for k in ("dy", "z", "mi", "gamma", "beta")}
    accg, xg = acc.cuda(), x.cuda()
    fused = Guarded((M, 9, 4), torch.float32, 0.0)
    assert lib.sfh_conv_wgrad_c4_bn(_ptr(dev["dy"]), _ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]),
                                    _ptr(accg), M, _ptr(xg), 3, B, H, W, _ptr(fused.t), 4, _stream()) == 0
    dz = Guarded((B, H, W, M), torch.float32, NAN)
    assert lib.sfh_bn_bwd_apply(_ptr(dev["dy"]), None, _ptr(dev["z"]), _ptr(dev["mi"]), _ptr(dev["gamma"]), _ptr(dev["beta"]),
                                _ptr(accg), 1, npix, M, _ptr(dz.t), None, None, 0, 0, None, None, _stream()) == 0
    two = Guarded((M, 9, 4), torch.float32, 0.0)
    assert lib.sfh_conv_wgrad(_ptr(dz.t), M, M, _ptr(xg), 4, H, W, 4, 0, 0, B, H, W, 3, _ptr(two.t), 4, 0, _stream()) == 0
    a, b = fused.result(), two.result()
    assert bool((a[..., 3] == 0).all()) and bool((b[..., 3] == 0).all())
    assert bool((b[..., :3] != 0).any())
    if frame in WGRAD_C4_ONE_TILE:
        assert torch.equal(_bits(a), _bits(b))
        return
    dzc = dz.result().double().abs().numpy()
    xp = np.zeros((B, H + 2, W + 2, 4))
    xp[:, 1:-1, 1:-1] = x.double().abs().numpy()
    S = np.stack([np.einsum("bhwm,bhwc->mc", dzc, xp[:, ky:ky + H, kx:kx + W]) for ky in range(3) for kx in range(3)], axis=1)
    bound = 2.02 * npix * 2.0 ** -24 * S
    ratio = R.ratio(a.double().numpy(), b.double().numpy(), bound)
    _report(f"conv_wgrad_c4_bn {cases.ident(frame)} M{M}", fused_vs_two_pass=ratio)
