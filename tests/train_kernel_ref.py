"""fp64 CPU references (test infrastructure only) for the plain training kernels of csrc/train_bn.hip and
csrc/train_heads.hip (the OutConv pair), one per entry point:

  sfh_bn_stats, sfh_bn_stats_partials, sfh_bn_finalize, sfh_bn_finalize_partials, sfh_bn_apply, sfh_bn_bwd_reduce,
  sfh_bn_bwd_apply, sfh_colsum, sfh_maxpool2_fwd, sfh_maxpool2_bwd, sfh_outconv_bwd, sfh_outconv_bwd_bn

Plain numpy / torch-CPU; nothing here imports a kernel.  Every ``*_ref`` returns the reference and the absolute sums
``A = sum |term|`` its bound is built from; every ``*_bound`` is derived from the number of fp32 (u = 2^-24) and fp64 (2^-53)
roundings of the kernel's arithmetic - the count stands in its docstring - and none is fitted to a kernel's output.  Each
bound holds whether or not the compiler contracts a multiply-add: a contraction removes a rounding, it never adds one.

The reference's own error.  Sums over pixels are taken in np.longdouble (64-bit mantissa on x86, asserted by the host
test), so a sum of n terms carries at most n * 2^-64 * A: every sum bound adds exactly that.  Element-wise references are
fp64 expressions of a handful of operations, each within 2^-53 relative; the factor 1.01 of the element-wise bounds
(0.01 * u = 2^-30.6) covers that and the second-order terms (u^2) of the kernel's own roundings.

n * u rule.  A sum of n floating-point products accumulated in any order has error at most n * u * sum |a_i b_i|, and a
sum of n numbers at most (n - 1) * u * sum |x_i|, with no higher-order terms (Jeannerod and Rump, "Improved error bounds
for inner products in floating-point arithmetic", SIAM J. Matrix Anal. Appl. 34, 2013) - barring underflow, which the
test data (randn-scaled) stays clear of.

tests/test_train_kernel_host.py holds these references against torch fp64 autograd and shows that a correct kernel - its
arithmetic restated in fp32, with and without contraction - stays inside every bound.
"""
import math
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
E53 = 2.0 ** -53        # fp64 unit roundoff
E64 = 2.0 ** -64        # np.longdouble unit roundoff (the references' sums)
LD = np.longdouble
AMBIGUITY_CAP = 1e-3    # at most 0.1 % of a case's elements may have a ReLU decision within the forward bound of zero


def f64(a):
    """a torch tensor or array as a float64 numpy array (exact for fp32 / fp64 input)"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _ld(a):
    return f64(a).astype(LD)


def ratio(got, ref, bound):
    """max |got - ref| / bound, the difference taken in longdouble; an entry with a zero bound must be exact"""
    err = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert not np.isnan(err).any(), "NaN in the output"
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference leaves no room"
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def sum64_bound(n, A, pre=0.0):
    """|got - ref| for an fp64 sum of n terms that are exact in fp64, added in any order onto an earlier content ``pre``:
    n + 1 summands are n additions, each within 2^-53 of a partial sum that never exceeds A + |pre|; the reference's
    longdouble sum adds n * 2^-64 * A.  Where every term is zero (A == 0) the additions are exact and the bound is 0."""
    A = np.asarray(A, dtype=np.float64)
    return n * (E53 + E64) * (A + np.abs(np.asarray(pre, dtype=np.float64))) * (A > 0)


# ------------------------------------------------------------------------------------------------ column sums
def bn_stats_ref(z):
    """sfh_bn_stats: z (npix, C) fp32 -> (s (2,C) longdouble = [sum z | sum z^2], A (2,C) = [sum |z| | sum z^2]).
    Both terms are exact in fp64 (z^2 has 48 significant bits)."""
    zl = _ld(z)
    s = np.stack([zl.sum(axis=0), (zl * zl).sum(axis=0)])
    A = np.stack([np.abs(zl).sum(axis=0), (zl * zl).sum(axis=0)]).astype(np.float64)
    return s, A


def bn_stats_bound(npix, A, pre=0.0):
    """The kernel converts each z to fp64 (exact), squares it in fp64 (exact: 48 bits; so a contracted s1 += z * z rounds
    the same once) and adds: npix exact terms per accumulator in a free order (thread chains, the block's lanes, one fp64
    atomic per block).  Roundings: npix additions of 2^-53.  Bound: npix * (2^-53 + 2^-64) * (A + |pre|)."""
    return sum64_bound(npix, A, pre)


def colsum_ref(x, C, c_off=0):
    """sfh_colsum over the channel slice [c_off, c_off + C) of x (npix, cs) fp32 -> (s (C,) longdouble, A (C,))."""
    xl = _ld(x)[:, c_off:c_off + C]
    return xl.sum(axis=0), np.abs(xl).sum(axis=0).astype(np.float64)


colsum_bound = bn_stats_bound     # the same arithmetic: npix exact fp64 terms, npix additions


def bn_stats_partials_ref(partial):
    """sfh_bn_stats_partials: partial (rows, 2C) fp64 -> (s (2C,) longdouble, A (2C,) = sum |partial|)."""
    pl = np.asarray(partial, dtype=np.float64).astype(LD)
    return pl.sum(axis=0), np.abs(pl).sum(axis=0).astype(np.float64)


def bn_stats_partials_bound(rows, A, pre=0.0):
    """rows fp64 terms per column (row-lane chains, four lanes, one atomic per block of rows): rows additions of 2^-53."""
    return sum64_bound(rows, A, pre)


# ------------------------------------------------------------------------------------------------ finalize
def bn_finalize_ref(acc, npix, eps, momentum, running_mean=None, running_var=None):
    """sfh_bn_finalize from acc (2,C) fp64 = [sum z | sum z^2], exactly (rational arithmetic) up to the square root:

      mean = acc0 / n, var = max(acc1 / n - mean^2, 0), invstd = 1 / sqrt(var + eps),
      running_mean' = (1 - momentum) running_mean + momentum mean,
      running_var'  = (1 - momentum) running_var + momentum var n / (n - 1)     (n == 1: the biased variance)

    eps and momentum are the fp32 values the entry point receives.  Returns a dict of fp64 arrays: mean, var, invstd,
    q = acc1 / n, msq = mean^2, and - with a running pair - running_mean, running_var, a_rm, a_rv (the absolute sums of
    the two running updates) and unbias = n / (n - 1).  The rational values are rounded to fp64 once (2^-53); invstd takes
    two more fp64 operations (sqrt, divide): 3 * 2^-53 relative in all, which finalize_bound adds."""
    acc = np.asarray(acc, dtype=np.float64).reshape(2, -1)
    C = acc.shape[1]
    n = Fraction(int(npix))
    eps_q, mom_q = Fraction(float(np.float32(eps))), Fraction(float(np.float32(momentum)))
    out = {k: np.zeros(C) for k in ("mean", "var", "invstd", "q", "msq")}
    if running_mean is not None:
        out.update({k: np.zeros(C) for k in ("running_mean", "running_var", "a_rm", "a_rv")})
        out["unbias"] = float(n / (n - 1)) if npix > 1 else 1.0
        rm, rv = f64(running_mean), f64(running_var)
    for c in range(C):
        m = Fraction(float(acc[0, c])) / n
        q = Fraction(float(acc[1, c])) / n
        var = max(q - m * m, Fraction(0))
        out["mean"][c], out["q"][c], out["msq"][c], out["var"][c] = float(m), float(q), float(m * m), float(var)
        out["invstd"][c] = 1.0 / math.sqrt(float(var + eps_q))
        if running_mean is not None:
            unb = var * n / (n - 1) if npix > 1 else var
            a, b = (1 - mom_q) * Fraction(float(rm[c])), mom_q * m
            out["running_mean"][c], out["a_rm"][c] = float(a + b), float(abs(a) + abs(b))
            a, b = (1 - mom_q) * Fraction(float(rv[c])), mom_q * unb
            out["running_var"][c], out["a_rv"][c] = float(a + b), float(abs(a) + abs(b))
    return out


def bn_finalize_bound(r, npix, eps, momentum, e_acc=None):
    """Bounds {mean, invstd, running_mean, running_var} for sfh_bn_finalize; ``e_acc`` (2,C) is the error the sums arrive
    with (zero for sfh_bn_finalize, whose input is the test's; the fixed-order sum's for sfh_bn_finalize_partials).

    The kernel works in fp64 and casts each result to fp32 once (u * |ref|; a zero reference is stored exactly).
      mean   acc0 / n: one fp64 rounding.                    e_m = 2^-53 |mean| + e_acc0 / n
      var    q = acc1 / n (1), mean * mean (1, on a mean that carries e_m: 2 |mean| e_m), the subtraction (1) - or, contracted,
             fma(-mean, mean, q): one rounding less.         e_v = 1.01 * 2^-53 * (q + 3 mean^2 + |q - mean^2|)
                                                                   + e_acc1 / n + 2 |mean| e_acc0 / n
             The clamp max(., 0) is 1-Lipschitz and the reference clamps too.
      invstd var + eps (1), sqrt (1), 1 / . (1), and d invstd / d var = -invstd^3 / 2, steepest at the smaller argument:
             (1 - e_v / (var + eps))^-1.5 <= 1.01 is asserted.  u |ref| + 1.01 * invstd^3 / 2 * e_v + 6 * 2^-53 |ref|
             (three roundings of the kernel, three of the reference).
      running_mean  1 - momentum (1), two products (2), the sum (1):  u |ref| + 5 * 2^-53 * a_rm + momentum * e_m
      running_var   the same and var * n / (n - 1) (2):               u |ref| + 7 * 2^-53 * a_rv + momentum * n / (n - 1) * e_v
    """
    C = r["mean"].shape[0]
    e_acc = np.zeros((2, C)) if e_acc is None else np.asarray(e_acc, dtype=np.float64)
    n = float(npix)
    mom = float(np.float32(momentum))
    e_m = E53 * np.abs(r["mean"]) + e_acc[0] / n
    e_v = 1.01 * E53 * (r["q"] + 3 * r["msq"] + np.abs(r["q"] - r["msq"])) + e_acc[1] / n + 2 * np.abs(r["mean"]) * e_acc[0] / n
    assert (e_v <= 6e-3 * (r["var"] + float(np.float32(eps)))).all(), "variance error too large to linearise invstd"
    b = {"mean": U * np.abs(r["mean"]) + e_m,
         "invstd": U * r["invstd"] + 1.01 * 0.5 * r["invstd"] ** 3 * e_v + 6 * E53 * r["invstd"]}
    if "running_mean" in r:
        b["running_mean"] = U * np.abs(r["running_mean"]) + 5 * E53 * r["a_rm"] + mom * e_m
        b["running_var"] = U * np.abs(r["running_var"]) + 7 * E53 * r["a_rv"] + mom * r["unbias"] * e_v
    return b


def bn_finalize_partials_ref(partial, npix, eps, momentum, running_mean=None, running_var=None):
    """sfh_bn_finalize_partials: partial (rows, 2, C) fp64 summed over the rows (longdouble), then bn_finalize_ref.
    Returns (r, A (2,C) = sum |partial|)."""
    p = np.asarray(partial, dtype=np.float64)
    rows, _, C = p.shape
    s, A = bn_stats_partials_ref(p.reshape(rows, 2 * C))
    return bn_finalize_ref(s.astype(np.float64).reshape(2, C), npix, eps, momentum, running_mean, running_var), A.reshape(2, C)


def bn_finalize_partials_bound(r, A, rows, npix, eps, momentum):
    """rows fp64 terms in a fixed order (16 row lanes, then the 16 lane sums): rows - 1 additions of 2^-53 and the
    reference's own sum, rounded to fp64 once: e_acc = (rows * 2^-53 + rows * 2^-64) * A; the rest is bn_finalize_bound."""
    return bn_finalize_bound(r, npix, eps, momentum, e_acc=rows * (E53 + E64) * A)


# ------------------------------------------------------------------------------------------------ apply
def bn_apply_ref(z, mi, gamma, beta, residual=None, relu=1):
    """sfh_bn_apply: y = [relu]((z - mean) * invstd * gamma + beta [+ residual]) in fp64 from the fp32 inputs the kernel
    reads; z (npix, C), mi (2C,) = [mean | invstd].  Returns a dict: y, pre (before the ReLU), xh, t = xh * gamma, tb = t + beta."""
    z, mi, gamma, beta = f64(z), f64(mi), f64(gamma), f64(beta)
    C = z.shape[-1]
    xh = (z - mi[:C]) * mi[C:]
    t = xh * gamma
    tb = t + beta
    pre = tb + f64(residual) if residual is not None else tb
    return {"y": np.maximum(pre, 0.0) if relu else pre, "pre": pre, "xh": xh, "t": t, "tb": tb, "residual": residual is not None}


def bn_apply_bound(r):
    """fp32 roundings: z - mean (1), * invstd (1), * gamma (1): t within (3u + 3u^2) |t|; + beta (1): u |t + beta| (a
    contracted xh * gamma + beta drops the product's rounding); + residual (1, only with a residual): u |pre|.
    Bound: 1.01 * u * (3 |t| + |t + beta| [+ |pre|]).  ReLU is 1-Lipschitz, so the bound holds behind it.  Where t and beta
    are both zero and there is no residual the bound is zero: the kernel's value is an exact zero too."""
    b = 3 * np.abs(r["t"]) + np.abs(r["tb"])
    if r["residual"]:
        b = b + np.abs(r["pre"])
    return 1.01 * U * b


def ambiguous(r):
    """Elements whose ReLU decision, recomputed on the device from z, may fall either way: the fp64 pre-activation lies
    within the forward bound of zero.  A pre-activation that is exactly zero with a zero bound (beta = 0, z equal to the
    fp32 mean) is not ambiguous: the kernel's value is an exact zero, y > 0 is false, g = 0."""
    e = bn_apply_bound(r)
    return (np.abs(r["pre"]) <= e) & (e > 0)


def relu_gate(dy, y, z, mi, gamma, beta, relu):
    """(g, amb): g = dy where the ReLU passed (fp64 decision), amb = the elements where either decision is right.
    y given: the decision y > 0 is read, exact.  y None and relu: recomputed as bn_apply without a residual."""
    dy = f64(dy)
    if not relu:
        return dy, np.zeros(dy.shape, dtype=bool)
    if y is not None:
        return dy * (f64(y) > 0), np.zeros(dy.shape, dtype=bool)
    r = bn_apply_ref(z, mi, gamma, beta, None, 1)
    return dy * (r["pre"] > 0), ambiguous(r)


# ------------------------------------------------------------------------------------------------ backward
def bn_bwd_reduce_ref(dy, y, z, mi, gamma, beta, relu):
    """sfh_bn_bwd_reduce: s (2,C) longdouble = [sum g | sum g * xhat], g = dy * (y > 0 if relu), xhat in fp64 from the fp32
    mean and invstd.  Returns (s, info): info has A (2,C) = [sum |g| | sum |g xhat|], amb (2,C) = the same two sums of |dy|
    and |dy xhat| over the ambiguous elements only, namb (their number) and g."""
    z, mi = f64(z), f64(mi)
    C = z.shape[-1]
    g, amb = relu_gate(dy, y, z, mi, gamma, beta, relu)
    xh = (z - mi[:C]) * mi[C:]
    gl, tl = g.astype(LD), g.astype(LD) * xh.astype(LD)
    s = np.stack([gl.sum(axis=0), tl.sum(axis=0)])
    A = np.stack([np.abs(gl).sum(axis=0), np.abs(tl).sum(axis=0)]).astype(np.float64)
    da = np.abs(f64(dy)) * amb
    return s, {"A": A, "amb": np.stack([da.sum(axis=0), (da * np.abs(xh)).sum(axis=0)]), "namb": int(amb.sum()), "g": g}


def bn_bwd_reduce_bound(npix, info, pre=0.0):
    """s0: the terms g are exact; npix additions in fp64:  npix * (2^-53 + 2^-64) * (sum |g| + |pre|).
    s1: xhat = (z - mean) * invstd in fp32, two roundings: within (2u + u^2) |xhat|; g * xhat is exact in fp64 (24 x 24
        bits; a contracted multiply-add rounds the same once) and the kernel's terms are at most (1 + 3u) times the
        reference's:  (2u + u^2) * sum |g xhat| + npix * (2^-53 (1 + 3u) + 2^-64) * (sum |g xhat| + |pre|).
    A recomputed ReLU decision adds, for each ambiguous element, its own |dy| to s0 and |dy xhat| (1 + 3u) to s1."""
    A, amb = info["A"], info["amb"]
    pre = np.broadcast_to(np.abs(np.asarray(pre, dtype=np.float64)), A.shape)
    live = (A > 0) | (amb > 0)
    b0 = npix * (E53 + E64) * (A[0] + amb[0] + pre[0]) * live[0] + amb[0]
    b1 = ((2 * U + U * U) * A[1] + npix * (E53 * (1 + 3 * U) + E64) * (A[1] + amb[1] + pre[1]) * live[1] + amb[1] * (1 + 3 * U))
    return np.stack([b0, b1])


def bn_bwd_apply_ref(dy, y, z, mi, gamma, beta, acc, relu, npix):
    """sfh_bn_bwd_apply: dz = gamma * invstd * (g - mg - xhat * mgx), mg = acc0 / npix, mgx = acc1 / npix, in fp64 from the
    inputs the kernel reads (acc (2C,) fp64).  Returns a dict: dz, g, amb, and the magnitudes of the bound."""
    z, mi, gamma, acc = f64(z), f64(mi), f64(gamma), f64(acc)
    C = z.shape[-1]
    g, amb = relu_gate(dy, y, z, mi, gamma, beta, relu)
    xh = (z - mi[:C]) * mi[C:]
    mg, mgx = acc[:C] / npix, acc[C:] / npix
    c = xh * mgx
    k = gamma * mi[C:]
    return {"dz": k * (g - mg - c), "g": g, "amb": amb, "k": k, "mg": np.broadcast_to(mg, g.shape), "c": c,
            "gm": g - mg, "gmc": g - mg - c, "dy": f64(dy), "npix": int(npix)}


def bn_bwd_apply_bound(r):
    """fp32 roundings.  The kernel multiplies by a rounded reciprocal: inv_n = 1 / (float)npix is one rounding (the cast of
    npix is exact below 2^24, which is asserted: every case is far smaller).  mg = (float)acc0 * inv_n: the cast of acc0
    (1), inv_n (1), the product (1): within 1.01 * 3u |mg|; the same for mgx.  xhat = (z - mean) * invstd: 2.
    c = xhat * mgx: one more, 6 in all (a contracted (g - mg) - xhat * mgx drops it).  g - mg (1): u |g - mg|.
    (g - mg) - c (1), gamma * invstd (1) and the last product (1): 3u |g - mg - c|.  With k = gamma * invstd:
        1.01 * u * |k| * (3 |mg| + |g - mg| + 6 |c| + 3 |g - mg - c|)
    An ambiguous ReLU decision adds |k * dy| for that element."""
    assert r["npix"] < 2 ** 24
    b = 1.01 * U * np.abs(r["k"]) * (3 * np.abs(r["mg"]) + np.abs(r["gm"]) + 6 * np.abs(r["c"]) + 3 * np.abs(r["gmc"]))
    return b + np.abs(r["k"] * r["dy"]) * r["amb"]


# ------------------------------------------------------------------------------------------------ max-pool 2x2
def _windows(H, W):
    Ho, Wo = H // 2, W // 2
    return [(slice(dy, 2 * Ho, 2), slice(dx, 2 * Wo, 2)) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]


def maxpool2_scan(x):
    """(max, index) of every 2x2 window of x (B,H,W,C) fp32 numpy (floor: an odd last row / column is cropped), by ATen's
    scan: start at the first element, move on where the next is greater or NaN - the FIRST maximum in scan order wins a
    tie (a -0 in front of a +0 included), a NaN propagates.  The values keep their fp32 bits."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[1:3]
    win = _windows(H, W)
    m = x[:, win[0][0], win[0][1]].copy()
    idx = np.zeros(m.shape, dtype=np.int8)
    for k in (1, 2, 3):
        v = x[:, win[k][0], win[k][1]]
        take = (v > m) | np.isnan(v)
        m = np.where(take, v, m)
        idx = np.where(take, np.int8(k), idx)
    return m, idx


def _max_later(a, b):
    """the project's pooling maximum (sfh_max_nan): a where a > b or a is NaN, else b - of two equal values the LATER one"""
    return np.where((a > b) | np.isnan(a), a, b)


def maxpool2_fwd_ref(x):
    """sfh_maxpool2_fwd: (B,H/2,W/2,C) fp32, bit for bit.  The value is F.max_pool2d's and a NaN propagates as there.  The
    bits of a tie are the project's own rule, shared by every pooling kernel it has (the inference epilogues included, which
    are held to each other bit for bit): max(max(a, b), max(c, d)) over the window (a b / c d), each max keeping its second
    operand on a tie - so among tied zeros of both signs the result carries the sign of the last one of its nest, where
    ATen's scan keeps the first.  -0 == +0: no value differs (the host test counts the signs that do)."""
    x = np.asarray(x, dtype=np.float32)
    a, b, c, d = (x[:, sy, sx] for sy, sx in _windows(*x.shape[1:3]))
    return _max_later(_max_later(a, b), _max_later(c, d))


def maxpool2_bwd_ref(x, dy, pre=None):
    """sfh_maxpool2_bwd: dx (B,H,W,C) fp32 = dy at the first maximum of each window, +0 at its other three places; with
    ``pre`` (accumulate) those are added onto it in fp32 - one addition, so bit for bit - and a cropped row / column keeps
    its content.  Without ``pre`` the sizes are even and every element is written.  No NaN in x."""
    x, dy = np.asarray(x, dtype=np.float32), np.asarray(dy, dtype=np.float32)
    H, W = x.shape[1:3]
    _, idx = maxpool2_scan(x)
    out = np.zeros(x.shape, dtype=np.float32) if pre is None else np.asarray(pre, dtype=np.float32).copy()
    for k, (sy, sx) in enumerate(_windows(H, W)):
        o = np.where(idx == k, dy, np.float32(0.0))
        out[:, sy, sx] = o if pre is None else out[:, sy, sx] + o
    return out


# ------------------------------------------------------------------------------------------------ OutConv backward
OUTCONV_FLUSH = 64      # fp32 terms a thread adds before it promotes its partial sums to fp64


def outconv_bwd_ref(x, w, dl):
    """sfh_outconv_bwd: x (B,H,W,cin) fp32 NHWC, w (nc,cin), dl (B,nc,H,W) NCHW.
    dx[p,ci] = sum_k dl[k,p] w[k,ci]; acc_w[k,ci] = sum_p dl[k,p] x[p,ci]; acc_b[k] = sum_p dl[k,p].
    Returns a dict: dx (npix,cin) fp64 with a_dx = sum_k |dl w|, acc_w (nc,cin) and acc_b (nc,) longdouble with a_w, a_b."""
    x, w, dl = f64(x), f64(w), f64(dl)
    cin, nc = x.shape[-1], w.shape[0]
    xp = x.reshape(-1, cin)
    dlp = np.moveaxis(dl, 1, -1).reshape(-1, nc)                       # (npix, nc)
    return {"dx": dlp @ w, "a_dx": np.abs(dlp) @ np.abs(w),
            "acc_w": np.einsum("pk,pc->kc", dlp.astype(LD), xp.astype(LD)), "a_w": np.abs(dlp).T @ np.abs(xp),
            "acc_b": dlp.astype(LD).sum(axis=0), "a_b": np.abs(dlp).sum(axis=0), "dlp": dlp, "npix": xp.shape[0]}


def outconv_bwd_bound(r, pre_w=0.0, pre_b=0.0):
    """dx     nc products and nc - 1 additions in fp32 (contracted: nc roundings): nc * u * a_dx by the n * u rule; the
              reference's fp64 matrix product adds nc * 2^-53 * a_dx.
       acc_w  a thread adds at most 64 products in fp32 before it promotes the partial sum to fp64: 64 * u * a_w by the
              n * u rule.  (The issue allows 65; the chain is flushed in front of the 65th term, so 64.)  The promoted sums
              - fewer than npix of them, each at most (1 + 64u) times its absolute sum - are added in fp64 in a free order:
              npix * (2^-53 (1 + 64u) + 2^-64) * (a_w + |pre|).
       acc_b  at most 64 numbers, 63 additions: 63 * u * a_b, and the same fp64 term."""
    nc = r["dlp"].shape[1]
    n = r["npix"]
    f = n * (E53 * (1 + 64 * U) + E64)
    return {"dx": (nc * U + nc * E53) * r["a_dx"],
            "acc_w": 64 * U * r["a_w"] + f * (r["a_w"] + np.abs(pre_w)) * (r["a_w"] > 0),
            "acc_b": 63 * U * r["a_b"] + f * (r["a_b"] + np.abs(pre_b)) * (r["a_b"] > 0)}


def outconv_bwd_bn_ref(z, mi, gamma, beta, w, dl):
    """sfh_outconv_bwd_bn: as outconv_bwd_ref with x = relu(bn_apply(z)) recomputed (no residual), and the BatchNorm backward
    sums of the layer in front, acc_bn (2,cin) = [sum g | sum g xhat], g = dx * (x > 0).  Adds to the dict: fwd (bn_apply_ref's),
    e_x (its bound), amb, acc_bn (longdouble), g and xh."""
    cin = f64(z).shape[-1]
    zp = f64(z).reshape(-1, cin)
    fwd = bn_apply_ref(zp, mi, gamma, beta, None, 1)
    r = outconv_bwd_ref(fwd["y"].reshape(f64(z).shape), w, dl)
    amb = ambiguous(fwd)
    g = r["dx"] * (fwd["pre"] > 0)
    gl = g.astype(LD)
    r.update({"fwd": fwd, "e_x": bn_apply_bound(fwd), "amb": amb, "g": g, "xh": fwd["xh"], "namb": int(amb.sum()),
              "acc_bn": np.stack([gl.sum(axis=0), (gl * fwd["xh"].astype(LD)).sum(axis=0)])})
    return r


def outconv_bwd_bn_bound(r, pre_w=0.0, pre_b=0.0, pre_bn=0.0):
    """dx, acc_b: as outconv_bwd_bound (x does not enter).
       acc_w   x is recomputed within e_x (bn_apply_bound; ReLU is 1-Lipschitz): the terms move by |dl| e_x, and the 64 u of the
               chain applies to the moved terms: + 1.01 * sum_p |dl| e_x.
       acc_bn  g is the kernel's own fp32 dx, within e_dx of the reference's, where x > 0:
               s0  sum_{x>0} e_dx + npix * (2^-53 + 2^-64) * (sum |g| + sum_{x>0} e_dx + |pre|)
               s1  xhat carries its two fp32 roundings: (2u + u^2) sum |g xhat| + (1 + 3u) sum_{x>0} e_dx |xhat| + the fp64 term
               and each ambiguous element adds its own |dx| + e_dx, times |xhat| (1 + 3u) in s1."""
    b = outconv_bwd_bound(r, pre_w, pre_b)
    b["acc_w"] = b["acc_w"] + 1.01 * np.abs(r["dlp"]).T @ r["e_x"]
    n = r["npix"]
    on = (r["fwd"]["pre"] > 0) | r["amb"]
    e_dx = b["dx"] * on
    xa = np.abs(r["xh"])
    amb_dx = (np.abs(r["dx"]) + b["dx"]) * r["amb"]
    A0, A1 = np.abs(r["g"]).sum(axis=0), (np.abs(r["g"]) * xa).sum(axis=0)
    pre_bn = np.broadcast_to(np.abs(np.asarray(pre_bn, dtype=np.float64)), (2,) + A0.shape)
    m0 = A0 + e_dx.sum(axis=0) + amb_dx.sum(axis=0)
    m1 = (A1 + (e_dx * xa).sum(axis=0) + (amb_dx * xa).sum(axis=0)) * (1 + 3 * U)
    b0 = e_dx.sum(axis=0) + amb_dx.sum(axis=0) + n * (E53 + E64) * (m0 + pre_bn[0]) * (m0 > 0)
    b1 = ((2 * U + U * U) * A1 + (1 + 3 * U) * ((e_dx * xa).sum(axis=0) + (amb_dx * xa).sum(axis=0))
          + n * (E53 + E64) * (m1 + pre_bn[1]) * (m1 > 0))
    b["acc_bn"] = np.stack([b0, b1])
    return b
