"""CPU tests that hold the fp64 references of tests/train_kernel_ref.py themselves.  No GPU, no kernel.

  * reference against torch fp64 autograd: the chain stats -> finalize -> apply and its backward against F.batch_norm
    (training, momentum 0.1) + residual + ReLU; the max-pool references against F.max_pool2d; the OutConv references
    against a 1x1 F.conv2d;
  * each kernel's arithmetic restated in fp32 twice - every operation rounded, and every multiply-add contracted (the fp64
    value of a * b + c rounded once) - stays inside the derived bound on every case tests/test_gpu_train_kernels.py runs:
    a correct kernel cannot fail there.  The largest error / bound ratio of each kernel is printed (``pytest -s``);
  * no case has more than 0.1 % of its recomputed ReLU decisions within the forward bound of zero;
  * the cancellation case: where the kernels' rule var = E[z^2] - mean^2 leaves a two-pass variance.
"""
import itertools
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_kernel_cases as cases
import train_kernel_ref as R
from host_program import build_host_program

U40 = 2.0 ** -40
f32 = np.float32


def test_longdouble_is_wider_than_double():
    """the references' sums rely on a 64-bit mantissa"""
    assert np.finfo(np.longdouble).nmant >= 63


def _np32(t):
    return t.numpy().astype(f32)


def _fma(a, b, c):
    """the contracted multiply-add: the fp64 value of a * b + c (the product of two fp32 is exact there) rounded to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _all_bn_cases():
    for (npix, C), kind in itertools.product(cases.REDUCTIONS, cases.REDUCTION_DATA):
        yield cases.bn_case(npix, C, kind)
    for shape in cases.APPLY_SHAPES + cases.SPLIT_SHAPES:
        yield cases.shape_case(shape)


# ------------------------------------------------------------------------------------------------ against autograd
def _chain_ref(c, relu, with_res):
    """the references chained as a training step chains the kernels, every stage in fp64 (nothing rounded to fp32 between)"""
    n, C = c["npix"], c["C"]
    rm, rv = torch.zeros(C) + 0.25, torch.ones(C) * 1.5
    s, _ = R.bn_stats_ref(c["z"])
    fin = R.bn_finalize_ref(s.astype(np.float64), n, cases.EPS, cases.MOMENTUM, rm, rv)
    mi = np.concatenate([fin["mean"], fin["invstd"]])
    res = c["residual"] if with_res else None
    fwd = R.bn_apply_ref(c["z"], mi, c["gamma"], c["beta"], res, relu)
    sums, info = R.bn_bwd_reduce_ref(c["dy"], fwd["y"] if relu else None, c["z"], mi, c["gamma"], c["beta"], relu)
    bwd = R.bn_bwd_apply_ref(c["dy"], fwd["y"] if relu else None, c["z"], mi, c["gamma"], c["beta"],
                             sums.astype(np.float64).reshape(-1), relu, n)
    return fin, fwd, sums.astype(np.float64), info, bwd, (rm, rv)


@pytest.mark.parametrize("relu,with_res", [(1, True), (1, False), (0, True)])
def test_batchnorm_chain_vs_autograd(relu, with_res):
    """stats -> finalize -> apply and bwd_reduce -> bwd_apply equal F.batch_norm(training=True, momentum=0.1) + residual + ReLU
    in fp64 - y, running_mean, running_var, dz, dgamma, dbeta, dres - within 2^-40 * A on every case.  A is the absolute sum
    of the terms of each output; where an output depends on invstd it carries the condition of the variance,
    kappa = 1 + invstd^2 / 2 * (E[z^2] + mean^2): the references take var = E[z^2] - mean^2 as the kernels do, from sums
    rounded to fp64, and F.batch_norm takes it in two passes (test_cancellation_case states the distance); xhat's two
    terms, |z| invstd and |mean| invstd, count separately.  A single pixel
    per channel is refused by F.batch_norm; there the closed form is asserted."""
    worst = 0.0
    for c in _all_bn_cases():
        n, C = c["npix"], c["C"]
        fin, fwd, sums, info, bwd, (rm, rv) = _chain_ref(c, relu, with_res)
        kappa = 1.0 + 0.5 * fin["invstd"] ** 2 * (fin["q"] + fin["msq"])
        if n == 1:
            assert (fin["var"] == 0).all() and (fin["mean"] == R.f64(c["z"])[0]).all()
            assert (fwd["xh"] == 0).all() and (bwd["dz"] == 0).all()
            assert np.allclose(fin["running_var"], 0.9 * 1.5, rtol=1e-7, atol=0)       # momentum is the fp32 0.1
            continue
        z = c["z"].double().requires_grad_(True)
        gam, bet = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
        res = c["residual"].double().requires_grad_(True)
        trm, trv = rm.double().clone(), rv.double().clone()
        out = F.batch_norm(z, trm, trv, gam, bet, True, float(np.float32(cases.MOMENTUM)), float(np.float32(cases.EPS)))
        if with_res:
            out = out + res
        if relu:
            out = torch.relu(out)
        out.backward(c["dy"].double())
        a_xh = (np.abs(R.f64(c["z"])) + np.abs(fin["mean"])) * fin["invstd"]          # the two terms of xhat = (z - mean) * invstd
        a_y = (kappa * a_xh * np.abs(R.f64(c["gamma"])) + np.abs(R.f64(c["beta"]))
               + (np.abs(R.f64(c["residual"])) if with_res else 0.0))
        a_dz = 3 * kappa * np.abs(bwd["k"]) * (np.abs(bwd["g"]) + np.abs(bwd["mg"]) + a_xh * np.abs(sums[1] / n))
        a_dgamma = kappa * (np.abs(bwd["g"]) * a_xh).sum(axis=0)
        a_rv = 0.9 * 1.5 + 0.1 * fin["unbias"] * (fin["q"] + fin["msq"])
        # the constant channel with beta = 0 and no residual sits exactly on the ReLU's kink (the reference: g = 0, the rule
        # y > 0); ATen's mean of a constant is off by an ulp, which decides its sign there: no backward comparison
        keep = np.arange(C) != (1 if relu and not with_res else -1)
        rs = [R.ratio(out.detach().numpy(), fwd["y"], U40 * a_y),
              R.ratio(trm.numpy(), fin["running_mean"], U40 * fin["a_rm"]),
              R.ratio(trv.numpy(), fin["running_var"], U40 * a_rv),
              R.ratio(z.grad.numpy()[:, keep], bwd["dz"][:, keep], U40 * a_dz[:, keep]),
              R.ratio(gam.grad.numpy()[keep], sums[1][keep], U40 * a_dgamma[keep]),
              R.ratio(bet.grad.numpy()[keep], sums[0][keep], U40 * info["A"][0][keep])]
        if with_res:
            assert np.array_equal(res.grad.numpy(), bwd["g"]), c["id"]
        assert max(rs) <= 1.0, (c["id"], rs)
        worst = max(worst, max(rs))
    print(f"RATIO chain vs autograd relu{relu} res{int(with_res)}: {worst:.3g} of 2^-40 A")


@pytest.mark.parametrize("kind", cases.POOL_DATA)
@pytest.mark.parametrize("shape", cases.POOL_SHAPES, ids=cases.ident)
def test_maxpool_refs_vs_torch(shape, kind):
    """the forward reference has F.max_pool2d(2)'s values, NaN included, and - wherever no tie between zeros of both signs
    decides - its bits; on the mixed-zero data the sign follows the project's later-operand rule and the differing signs are
    counted.  The scan the backward reference routes by (first maximum in scan order) is ATen's forward bit for bit, and the
    backward reference is the fp64 autograd gradient."""
    c = cases.pool_case(shape, kind)
    xt = c["x"].permute(0, 3, 1, 2).double().requires_grad_(True)
    yt = F.max_pool2d(xt, 2)
    want = yt.detach().permute(0, 2, 3, 1).float().contiguous().numpy()
    got = R.maxpool2_fwd_ref(_np32(c["x"]))
    scan = R.maxpool2_scan(_np32(c["x"]))[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(scan), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])
    assert np.array_equal(scan.view(np.int32)[ok], want.view(np.int32)[ok])
    nz = ok & (want != 0)
    assert np.array_equal(got.view(np.int32)[nz], want.view(np.int32)[nz])
    flipped = int((got.view(np.int32) != want.view(np.int32))[ok].sum())          # zeros only: halves has -0 too (round(-0.2))
    assert flipped == 0 or kind in ("zeros", "halves")
    print(f"maxpool {shape} {kind}: {flipped} of {got.size} results are a zero of the other sign than ATen's")
    if kind == "nan":
        assert np.isnan(got).sum() == 2
        return
    yt.backward(c["dy"].permute(0, 3, 1, 2).double())
    dx = R.maxpool2_bwd_ref(_np32(c["x"]), _np32(c["dy"]))
    assert np.array_equal(dx, xt.grad.permute(0, 2, 3, 1).float().numpy())
    acc = R.maxpool2_bwd_ref(_np32(c["x"]), _np32(c["dy"]), _np32(c["pre"]))
    assert np.array_equal(acc, _np32(c["pre"]) + dx)
    B, H, W, C = shape
    assert np.array_equal(acc[:, H // 2 * 2:], _np32(c["pre"])[:, H // 2 * 2:])
    assert np.array_equal(acc[:, :, W // 2 * 2:], _np32(c["pre"])[:, :, W // 2 * 2:])
    if kind == "constant":
        assert (dx[:, 0:H // 2 * 2:2, 0:W // 2 * 2:2] == _np32(c["dy"])).all()          # the first place of every window


@pytest.mark.parametrize("shape", cases.OUTCONV_SHAPES, ids=cases.ident)
def test_outconv_refs_vs_conv2d(shape):
    """dx, dW and db of a 1x1 F.conv2d in fp64 autograd, within 2^-40 * A; the BatchNorm form's acc_bn equals the plain
    references chained: bn_bwd_reduce_ref on its own dx and z"""
    B, H, W, cin, nc = shape
    c = cases.outconv_case(shape)
    r = R.outconv_bwd_ref(c["x"], c["w"], c["dl"])
    xt = c["x"].permute(0, 3, 1, 2).double().requires_grad_(True)
    wt = c["w"].double().reshape(nc, cin, 1, 1).requires_grad_(True)
    bt = torch.zeros(nc, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wt, bt).backward(c["dl"].double())
    assert R.ratio(xt.grad.permute(0, 2, 3, 1).reshape(-1, cin).numpy(), r["dx"], U40 * r["a_dx"]) <= 1.0
    assert R.ratio(wt.grad.reshape(nc, cin).numpy(), r["acc_w"], U40 * r["a_w"]) <= 1.0
    assert R.ratio(bt.grad.numpy(), r["acc_b"], U40 * r["a_b"]) <= 1.0
    rb = R.outconv_bwd_bn_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["w"], c["dl"])
    s, info = R.bn_bwd_reduce_ref(rb["dx"], None, c["z"].reshape(-1, cin), c["mi"], c["gamma"], c["beta"], 1)
    assert R.ratio(rb["acc_bn"], s, U40 * info["A"]) <= 1.0


# ------------------------------------------------------------------------------------------------ the fp32 restatements
def _xhat32(c):
    C = c["C"]
    mi = _np32(c["mi"])
    return (_np32(c["z"]) - mi[:C]) * mi[C:]


def _apply32(c, with_res, relu, contract):
    """bn_apply_kernel: ((z - mean) * invstd) * gamma + beta [+ residual], sfh_relu"""
    xh, gam, bet = _xhat32(c), _np32(c["gamma"]), _np32(c["beta"])
    o = _fma(xh, np.broadcast_to(gam, xh.shape), np.broadcast_to(bet, xh.shape)) if contract else xh * gam + bet
    if with_res:
        o = o + _np32(c["residual"])
    return np.where(o < 0, f32(0), o) if relu else o


def _gate32(c, mode, contract):
    y, relu = cases.bwd_inputs(c, mode)
    dy = _np32(c["dy"])
    if not relu:
        return dy
    yv = _np32(y) if y is not None else _apply32(c, False, 0, contract)
    return np.where(yv > 0, dy, f32(0))


def _sum64(t, pre, sequential):
    """an fp64 sum over the pixels in one of two orders - the kernels' order is free"""
    t = np.concatenate([np.asarray(pre, dtype=np.float64).reshape((1,) + t.shape[1:]), t])
    return np.cumsum(t, axis=0)[-1] if sequential else t.sum(axis=0)


def test_restated_reductions_inside_bounds():
    """bn_stats, colsum, bn_bwd_reduce (three modes), restated with their fp32 stage (xhat) rounded operation by operation and
    the fp64 sums in two orders, onto loaded accumulators"""
    worst = {"bn_stats": 0.0, "colsum": 0.0, "bn_bwd_reduce": 0.0}
    for (npix, C), kind in itertools.product(cases.REDUCTIONS, cases.REDUCTION_DATA):
        c = cases.bn_case(npix, C, kind)
        pre = c["acc_pre"].numpy()
        z = R.f64(c["z"])
        s, A = c["stats"]
        bound = R.bn_stats_bound(npix, A, pre)
        for seq in (False, True):
            got = np.stack([_sum64(z, pre[0], seq), _sum64(z * z, pre[1], seq)])
            worst["bn_stats"] = max(worst["bn_stats"], R.ratio(got, s + pre, bound))
            cs, cA = R.colsum_ref(c["z"], C)
            worst["colsum"] = max(worst["colsum"], R.ratio(_sum64(z, pre[0], seq), cs + pre[0], R.colsum_bound(npix, cA, pre[0])))
        for mode, contract in itertools.product(cases.BWD_MODES, (False, True)):
            y, relu = cases.bwd_inputs(c, mode)
            s, info = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
            g = _gate32(c, mode, contract).astype(np.float64)
            got = np.stack([_sum64(g, pre[0], contract), _sum64(g * _xhat32(c).astype(np.float64), pre[1], contract)])
            worst["bn_bwd_reduce"] = max(worst["bn_bwd_reduce"], R.ratio(got, s + pre, R.bn_bwd_reduce_bound(npix, info, pre)))
    for k, v in worst.items():
        print(f"RATIO restated {k}: {v:.3f}")
        assert v <= 1.0, k


def _bwd_acc(c, mode):
    """the reference's own backward sums [sum g | sum g xhat] as the fp64 accumulator bn_bwd_apply reads"""
    y, relu = cases.bwd_inputs(c, mode)
    sums, _ = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
    return sums.astype(np.float64).reshape(-1)


def _bwd_apply32(c, mode, acc, contract):
    """bn_bwd_apply_kernel: (g, dz), dz = (gamma * invstd) * ((g - mg) - xhat * mgx) with mg = (float)acc * (1 / (float)n)"""
    n, C = c["npix"], c["C"]
    xh, mi, gam = _xhat32(c), _np32(c["mi"]), _np32(c["gamma"])
    g = _gate32(c, mode, contract)
    inv_n = f32(1.0) / f32(n)
    mg, mgx = acc[:C].astype(f32) * inv_n, acc[C:].astype(f32) * inv_n
    gm = g - mg
    inner = _fma(-xh, np.broadcast_to(mgx, xh.shape), gm) if contract else gm - xh * mgx
    return g, (gam * mi[C:]) * inner


def test_restated_apply_inside_bounds():
    """bn_apply and bn_bwd_apply on every shape, residual, ReLU and backward mode"""
    worst = {"bn_apply": 0.0, "bn_bwd_apply": 0.0}
    for c in _all_bn_cases():
        n, C = c["npix"], c["C"]
        for with_res, relu, contract in itertools.product((False, True), (0, 1), (False, True)):
            r = R.bn_apply_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["residual"] if with_res else None, relu)
            worst["bn_apply"] = max(worst["bn_apply"], R.ratio(_apply32(c, with_res, relu, contract), r["y"], R.bn_apply_bound(r)))
        for mode, contract in itertools.product(cases.BWD_MODES, (False, True)):
            y, relu = cases.bwd_inputs(c, mode)
            acc = _bwd_acc(c, mode)
            r = R.bn_bwd_apply_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], acc, relu, n)
            g, got = _bwd_apply32(c, mode, acc, contract)
            worst["bn_bwd_apply"] = max(worst["bn_bwd_apply"], R.ratio(got, r["dz"], R.bn_bwd_apply_bound(r)))
            amb = r["amb"]
            assert np.array_equal(g[~amb].astype(np.float64), r["g"][~amb])                     # dres, bit for bit
    for k, v in worst.items():
        print(f"RATIO restated {k}: {v:.3f}")
        assert v <= 1.0, k


def _finalize64(acc, n, eps, mom, rm, rv, contract):
    """bn_finalize_kernel in fp64 operation by operation; contracted: var = fma(-mean, mean, acc1 / n), the running updates
    as fma(momentum, x, (1 - momentum) * running)"""
    def fma(a, b, c):
        return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(w))) for x, y, w in zip(a, b, c)])
    nn = np.float64(n)
    mean = acc[0] / nn
    q = acc[1] / nn
    var = fma(-mean, mean, q) if contract else q - mean * mean
    var = np.where(var > 0, var, 0.0)
    out = {"mean": mean.astype(f32), "invstd": (1.0 / np.sqrt(var + np.float64(f32(eps)))).astype(f32)}
    if rm is not None:
        unb = var * nn / (nn - 1.0) if n > 1 else var
        m = np.float64(f32(mom))
        a, b = (1.0 - m) * rm.astype(np.float64), (1.0 - m) * rv.astype(np.float64)
        mm = np.full_like(mean, m)
        out["running_mean"] = (fma(mm, mean, a) if contract else a + m * mean).astype(f32)
        out["running_var"] = (fma(mm, unb, b) if contract else b + m * unb).astype(f32)
    return out


def test_restated_finalize_inside_bounds():
    """bn_finalize on C x npix (negative rounded variance in channel 0 included), bn_finalize_partials and bn_stats_partials on
    rows x C with the rows summed lane by lane as the kernel does"""
    worst = {"bn_finalize": 0.0, "bn_finalize_partials": 0.0, "bn_stats_partials": 0.0}
    for C, npix, contract in itertools.product(cases.FINALIZE_C, cases.FINALIZE_NPIX, (False, True)):
        c = cases.finalize_case(C, npix)
        acc, rm, rv = c["acc"].numpy(), _np32(c["running_mean"]), _np32(c["running_var"])
        r = R.bn_finalize_ref(acc, npix, cases.EPS, cases.MOMENTUM, rm, rv)
        if npix == 1:
            assert r["unbias"] == 1.0                             # a single pixel: the unbiased variance is the biased one
        b = R.bn_finalize_bound(r, npix, cases.EPS, cases.MOMENTUM)
        got = _finalize64(acc, npix, cases.EPS, cases.MOMENTUM, rm, rv, contract)
        assert got["invstd"][0] == f32(1.0 / np.sqrt(np.float64(f32(cases.EPS))))     # channel 0: clamped to var = 0
        for k in b:
            worst["bn_finalize"] = max(worst["bn_finalize"], R.ratio(got[k], r[k], b[k]))
    for rows, C in itertools.product(cases.PARTIAL_ROWS, cases.PARTIAL_C):
        c = cases.partials_case(rows, C)
        p, rm, rv = c["partial"].numpy(), _np32(c["running_mean"]), _np32(c["running_var"])
        lanes = [p[l::16].sum(axis=0) if l < rows else np.zeros((2, C)) for l in range(16)]      # a lane's chain (numpy adds in order
        tot = lanes[0]                                                                           # below 8 terms, pairwise above)
        for l in range(1, 16):
            tot = tot + lanes[l]
        r, A = R.bn_finalize_partials_ref(p, c["npix"], cases.EPS, cases.MOMENTUM, rm, rv)
        b = R.bn_finalize_partials_bound(r, A, rows, c["npix"], cases.EPS, cases.MOMENTUM)
        got = _finalize64(tot, c["npix"], cases.EPS, cases.MOMENTUM, rm, rv, False)
        for k in b:
            worst["bn_finalize_partials"] = max(worst["bn_finalize_partials"], R.ratio(got[k], r[k], b[k]))
        pre = c["acc_pre"].numpy()
        s, A2 = R.bn_stats_partials_ref(p.reshape(rows, 2 * C))
        got = _sum64(p.reshape(rows, 2 * C), pre, True)
        worst["bn_stats_partials"] = max(worst["bn_stats_partials"], R.ratio(got, s + pre, R.bn_stats_partials_bound(rows, A2, pre)))
    for k, v in worst.items():
        print(f"RATIO restated {k}: {v:.3f}")
        assert v <= 1.0, k


def _outconv32(x, w, dl, contract, bn=None):
    """outconv_bwd_kernel with its thread mapping: a block of max(1024, ...) pixels, 256 / (cin / 4) pixel lanes, a lane's
    fp32 chain promoted to fp64 in front of every 65th term; the fp64 sums in lane, then block order"""
    B, H, W, cin = x.shape
    nc = w.shape[0]
    npix = B * H * W
    xp, dlp = x.reshape(npix, cin), np.moveaxis(dl, 1, -1).reshape(npix, nc)
    xh = None
    if bn is not None:
        mi, gam, bet = bn
        xh = (xp - mi[:cin]) * mi[cin:]
        o = _fma(xh, np.broadcast_to(gam, xh.shape), np.broadcast_to(bet, xh.shape)) if contract else xh * gam + bet
        xp = np.where(o < 0, f32(0), o)
    dx = np.zeros((npix, cin), dtype=f32)
    for k in range(nc):
        gk, wk = dlp[:, k:k + 1], np.broadcast_to(w[k], (npix, cin))
        dx = _fma(np.broadcast_to(gk, dx.shape), wk, dx) if contract else dx + gk * wk
    ppb = max(1024, (npix // 1024 + 255) // 256 * 256)
    lanes = 256 // (cin // 4)
    acc_w, acc_b = np.zeros((nc, cin)), np.zeros(nc)
    for p0 in range(0, npix, ppb):
        p1 = min(p0 + ppb, npix)
        steps = -(-(p1 - p0) // lanes)
        xs = np.zeros((steps * lanes, cin), dtype=f32)
        ds = np.zeros((steps * lanes, nc), dtype=f32)
        xs[:p1 - p0], ds[:p1 - p0] = xp[p0:p1], dlp[p0:p1]
        xs, ds = xs.reshape(steps, lanes, 1, cin), ds.reshape(steps, lanes, nc, 1)
        sw, sb = np.zeros((lanes, nc, cin), dtype=f32), np.zeros((lanes, nc, 1), dtype=f32)
        dsw, dsb = np.zeros((lanes, nc, cin)), np.zeros((lanes, nc, 1))
        for s in range(steps):
            if s and s % R.OUTCONV_FLUSH == 0:
                dsw, dsb = dsw + sw, dsb + sb
                sw, sb = sw * 0, sb * 0
            sb = sb + ds[s]
            dd, xx = np.broadcast_to(ds[s], sw.shape), np.broadcast_to(xs[s], sw.shape)
            sw = _fma(dd, xx, sw) if contract else sw + dd * xx
        acc_w += (dsw + sw).sum(axis=0)
        acc_b += (dsb + sb).sum(axis=0)[:, 0]
    out = {"dx": dx, "acc_w": acc_w, "acc_b": acc_b}
    if bn is not None:
        g = np.where(xp > 0, dx, f32(0)).astype(np.float64)
        out["acc_bn"] = np.stack([g.sum(axis=0), (g * xh.astype(np.float64)).sum(axis=0)])
    return out


def test_restated_outconv_inside_bounds():
    """sfh_outconv_bwd and sfh_outconv_bwd_bn on every shape, accumulators loaded"""
    worst = {"outconv_bwd": 0.0, "outconv_bwd_bn": 0.0}
    for shape, contract in itertools.product(cases.OUTCONV_SHAPES, (False, True)):
        c = cases.outconv_case(shape)
        w, dl = _np32(c["w"]), _np32(c["dl"])
        pw, pb, pbn = c["acc_w"].numpy(), c["acc_b"].numpy(), c["acc_bn"].numpy()
        r = R.outconv_bwd_ref(c["x"], c["w"], c["dl"])
        b = R.outconv_bwd_bound(r, pw, pb)
        got = _outconv32(_np32(c["x"]), w, dl, contract)
        rs = [R.ratio(got["dx"], r["dx"], b["dx"]), R.ratio(got["acc_w"] + pw, r["acc_w"] + pw, b["acc_w"]),
              R.ratio(got["acc_b"] + pb, r["acc_b"] + pb, b["acc_b"])]
        worst["outconv_bwd"] = max(worst["outconv_bwd"], max(rs))
        r = R.outconv_bwd_bn_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["w"], c["dl"])
        b = R.outconv_bwd_bn_bound(r, pw, pb, pbn)
        got = _outconv32(_np32(c["z"]), w, dl, contract, (_np32(c["mi"]), _np32(c["gamma"]), _np32(c["beta"])))
        rs = [R.ratio(got["dx"], r["dx"], b["dx"]), R.ratio(got["acc_w"] + pw, r["acc_w"] + pw, b["acc_w"]),
              R.ratio(got["acc_b"] + pb, r["acc_b"] + pb, b["acc_b"]), R.ratio(got["acc_bn"] + pbn, r["acc_bn"] + pbn, b["acc_bn"])]
        worst["outconv_bwd_bn"] = max(worst["outconv_bwd_bn"], max(rs))
    for k, v in worst.items():
        print(f"RATIO restated {k}: {v:.3f}")
        assert v <= 1.0, k


# ------------------------------------------------------------------------------------------------ ambiguity, cancellation
def test_ambiguity_cap():
    """every case that lets the device recompute a ReLU decision has at most 0.1 % of its elements within the forward bound
    of zero - from the reference alone; the exact zeros of the constant and the all-zero channel (beta = 0) are not ambiguous"""
    worst = 0.0
    for c in _all_bn_cases():
        r = R.bn_apply_ref(c["z"], c["mi"], c["gamma"], c["beta"], None, 1)
        amb = R.ambiguous(r)
        assert not amb[:, 1:3].any() and (r["pre"][:, 1:3] == 0).all(), c["id"]
        share = amb.mean()
        assert share <= R.AMBIGUITY_CAP, (c["id"], share)
        worst = max(worst, share)
    for shape in cases.OUTCONV_SHAPES:
        c = cases.outconv_case(shape)
        r = R.outconv_bwd_bn_ref(c["z"], c["mi"], c["gamma"], c["beta"], c["w"], c["dl"])
        share = r["amb"].mean()
        assert share <= R.AMBIGUITY_CAP, (shape, share)
        worst = max(worst, share)
    print(f"largest ambiguous share: {worst:.2e}")


def test_cancellation_case():
    """var = E[z^2] - mean^2 on 100 + 0.01 randn.  With exact sums the rule IS the two-pass variance; what the kernels lose is
    the rounding of the fp64 sums: sum z^2 arrives within N * 2^-53 * sum z^2, so var within N * 2^-53 * E[z^2] and a like
    amount from the mean - N * 2^-52 * E[z^2] in all - and invstd within N * 2^-52 * E[z^2] * invstd^3 / 2 of the two-pass
    one.  Here: the reference (longdouble sums) against a two-pass longdouble variance, and the same sums taken in fp64 in
    two orders, beside that worst case.  ATen's two-pass rule does not carry the factor E[z^2] / var (about 10^8 here)."""
    for npix, C in cases.REDUCTIONS:
        if npix == 1:
            continue
        c = cases.bn_case(npix, C, "offset")
        z = R.f64(c["z"]).astype(np.longdouble)
        m = z.mean(axis=0)
        var2 = (((z - m) ** 2).mean(axis=0)).astype(np.float64)
        inv2 = 1.0 / np.sqrt(var2 + float(f32(cases.EPS)))
        s, A = c["stats"]
        fin = R.bn_finalize_ref(s.astype(np.float64), npix, cases.EPS, cases.MOMENTUM)
        worst_case = npix * 2.0 ** -52 * (A[1] / npix) * 0.5 * np.maximum(fin["invstd"], inv2) ** 3
        dep_ref = np.abs(fin["invstd"] - inv2)
        z64 = R.f64(c["z"])
        dep = np.zeros(C)
        for seq in (False, True):
            acc = np.stack([_sum64(z64, np.zeros(C), seq), _sum64(z64 * z64, np.zeros(C), seq)])
            dep = np.maximum(dep, np.abs(R.bn_finalize_ref(acc, npix, cases.EPS, cases.MOMENTUM)["invstd"] - inv2))
        live = np.arange(C) != 2                                  # the all-zero channel has nothing to cancel
        print(f"cancellation {c['id']}: invstd departs from two-pass by {(dep[live] / inv2[live]).max():.2e} relative "
              f"(reference: {(dep_ref[live] / inv2[live]).max():.2e}); derived worst case {(worst_case[live] / inv2[live]).max():.2e}")
        assert (dep <= worst_case).all() and (dep_ref <= worst_case).all(), c["id"]
        assert (fin["var"][1] == 0) and fin["invstd"][1] == 1.0 / np.sqrt(float(Fraction(float(f32(cases.EPS))))), c["id"]


# ------------------------------------------------------------------------------------------------ the restatement is the code
# csrc/bn_math.h - the functions every training kernel and the conv epilogue call for this arithmetic - compiled for the host
# (tests/bn_math_host_main.cpp, a child process under AddressSanitizer and UBSan) against the every-operation-rounded
# restatements above: IEEE single and double sums, products, one division and one square root on both sides, so the bits are
# equal and no tolerance is involved.
@pytest.fixture(scope="module")
def bn_math_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "bn_math")


def _run_bn_math(program, tmp_path, mode, dims, inputs, outputs):
    """arrays -> raw little-endian files -> one run of the program -> the named outputs as flat arrays"""
    np.asarray(dims, dtype="<i8").tofile(tmp_path / "dims.i64")
    for name, a in inputs.items():
        np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<")).tofile(tmp_path / name)
    r = subprocess.run([program, mode, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [np.fromfile(tmp_path / name, dtype=dt) for name, dt in outputs]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                                 b.view(np.int32 if a.dtype == np.float32 else np.int64))


def _bn_inputs(c, *names):
    return {f"{k}.f32": _np32(c[k]) for k in names}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("shape", cases.APPLY_SHAPES + cases.SPLIT_SHAPES, ids=cases.ident)
def test_bn_math_header_apply_equals_restatement(bn_math_program, tmp_path, shape, with_res, relu):
    """y of bn_math.h (bn_load, BnChannels::y, sfh_relu) == _apply32(..., contract=False), bit for bit"""
    c = cases.shape_case(shape)
    inputs = _bn_inputs(c, "z", "mi", "gamma", "beta", *(["residual"] if with_res else []))
    y, = _run_bn_math(bn_math_program, tmp_path, "apply", [c["npix"], c["C"], relu, int(with_res)], inputs, [("y.f32", "<f4")])
    assert _same_bits(y.reshape(c["npix"], c["C"]), _apply32(c, with_res, relu, False))


@pytest.mark.parametrize("mode", cases.BWD_MODES)
@pytest.mark.parametrize("shape", cases.APPLY_SHAPES + cases.SPLIT_SHAPES, ids=cases.ident)
def test_bn_math_header_backward_equals_restatement(bn_math_program, tmp_path, shape, mode):
    """g (bn_gate: the strict y > 0, on y given or recomputed; the exact zeros of the constant and the all-zero channel gate to
    0) == _gate32(..., False) and dz (bn_dz) == _bwd_apply32(..., contract=False), bit for bit.  Without a recomputation beta is
    not handed over: the header must not read it."""
    c = cases.shape_case(shape)
    y, relu = cases.bwd_inputs(c, mode)
    acc = _bwd_acc(c, mode)
    inputs = _bn_inputs(c, "dy", "z", "mi", "gamma", *(["beta"] if relu and y is None else []))
    inputs["acc.f64"] = acc
    if y is not None:
        inputs["y.f32"] = _np32(y)
    g, dz = _run_bn_math(bn_math_program, tmp_path, "bwd", [c["npix"], c["C"], relu, int(y is not None)], inputs,
                         [("g.f32", "<f4"), ("dz.f32", "<f4")])
    want_g, want_dz = _bwd_apply32(c, mode, acc, False)
    assert _same_bits(want_g, _gate32(c, mode, False))
    if mode == "recompute":
        assert (want_g[:, 1:3] == 0).all()                  # beta = 0 there: the pre-activation is an exact (signed) zero
    assert _same_bits(g.reshape(want_g.shape), want_g)
    assert _same_bits(dz.reshape(want_dz.shape), want_dz)


@pytest.mark.parametrize("running", [True, False], ids=["run", "norun"])
@pytest.mark.parametrize("npix", cases.FINALIZE_NPIX)
@pytest.mark.parametrize("C", cases.FINALIZE_C)
def test_bn_math_header_finalize_equals_restatement(bn_math_program, tmp_path, C, npix, running):
    """mean, invstd and the running pair of bn_finalize_channel == _finalize64(..., contract=False), bit for bit"""
    c = cases.finalize_case(C, npix)
    acc, rm, rv = c["acc"].numpy(), _np32(c["running_mean"]), _np32(c["running_var"])
    inputs = {"acc.f64": acc, "params.f32": np.array([cases.EPS, cases.MOMENTUM], dtype=f32)}
    outputs = [("mean_invstd.f32", "<f4")]
    if running:
        inputs.update({"running_mean.f32": rm, "running_var.f32": rv})
        outputs += [("running_mean.out", "<f4"), ("running_var.out", "<f4")]
    got = _run_bn_math(bn_math_program, tmp_path, "finalize", [npix, C, int(running)], inputs, outputs)
    want = _finalize64(acc, npix, cases.EPS, cases.MOMENTUM, rm if running else None, rv if running else None, False)
    assert _same_bits(got[0], np.concatenate([want["mean"], want["invstd"]]))
    if running:
        assert _same_bits(got[1], want["running_mean"]) and _same_bits(got[2], want["running_var"])
