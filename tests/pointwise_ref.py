"""fp64 CPU references (test infrastructure only) for the forward entries of csrc/pointwise.hip:

  sfh_nchw_to_nhwc, sfh_nhwc_to_nchw, sfh_space_to_depth2, sfh_maxpool3x3s2_fwd, sfh_resize_nchw (nearest and bilinear),
  sfh_upsample2x_bilinear_nhwc, sfh_fold_bn, sfh_outconv_fwd, sfh_consistency_ce_fwd, sfh_avgpool_linear_fwd,
  sfh_compose_up_weights

Plain numpy and torch on the CPU; nothing here imports the library.  The conventions are those of tests/step_tail_ref.py,
whose helpers are used, not restated (U, K2, ETA, T, f64, ratio, nearest_table, up2_weights, _softmax_parts): every
reference computes in fp64 from the fp32 inputs and returns, beside its values, a per-element bound - a count of the kernel's
roundings (u = 2^-24 each) over the reference's own ABSOLUTE quantities, times K2 = 1.01 for the second-order terms and the
reference's own fp64 error.  None is fitted to a kernel's output.  The library is built without multiply-add contraction.
Divisions and sqrtf are IEEE operations (one rounding, u), as in step_tail_ref.opt_step; expf and logf carry T ulps.

The movers (layout conversion, space-to-depth, max-pool, nearest resize) select and never compute: their references are
indexing and the comparison is bit for bit.

Decision rules, taken as the operations define them:

  nearest index    min(floor(fl32(o * fl32(fl32(in) / fl32(out)))), in - 1), decided in fp32 (step_tail_ref.nearest_table).  It
                   is NOT floor(o * in / out): 26 -> 22 at o = 11 gives 12 where the exact quotient is 13 (NEAREST_FP32_PAIRS).
                   align_corners does not enter.
  bilinear taps    ATen's area_pixel_compute_source_index: align_corners: src = o * (in - 1) / (out - 1) (0 for out = 1);
                   otherwise src = max(0, (o + 1/2) * in / out - 1/2); i0 = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1),
                   weights 1 - l and l with l = src - i0.  The reference takes src as the exact rational; the kernel's fp32 src
                   enters the bound (bilinear_weights).
  argmax           the first index of the largest logit under a strict `>` scan that starts at class 0 (argmax_scan).  On
                   finite logits that is np.argmax.  A NaN never wins and never loses its place: a NaN at class 0 stays the
                   answer, a NaN elsewhere is skipped; +inf wins like any large value.  torch's argmax(softmax(.)) - the
                   reference project's preds_to_masks - answers 0 for every row that holds a NaN or a +inf (softmax turns
                   the whole row into NaN, and argmax of an all-NaN row is its first element).  The two differ on such rows
                   and nowhere else outside SOFTMAX_TIE_MARGIN; the kernel's rule is pinned, not changed.
  max-pool         torch's: a NaN in the window is the result; padding never wins (a window of -inf gives -inf).
"""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

import step_tail_ref as S
from step_tail_ref import ETA, K2, T, U, f64, nearest_table, ratio, up2_weights  # noqa: F401  (shared, not restated)
from theta_grad_ref import pool_out

F32 = np.float32
NEAREST_FP32_PAIRS = ((26, 22), (62, 14))     # found by search below 2048: fl32 rule != exact floor (see the module docstring)


# ------------------------------------------------------------------------------------------------ movers
def nchw_to_nhwc_ref(x, cs):
    """(B,C,H,W) -> (B,H,W,cs): channel c at lane c, lanes C .. cs-1 are +0.0"""
    B, C, H, W = x.shape
    out = np.zeros((B, H, W, cs), dtype=F32)
    out[..., :C] = x.transpose(0, 2, 3, 1)
    return out


def nhwc_to_nchw_ref(y, C):
    """(B,H,W,cs) -> (B,C,H,W): lanes C .. cs-1 are not read into anything"""
    return np.ascontiguousarray(y[..., :C].transpose(0, 3, 1, 2))


def space_to_depth2_ref(x):
    """(B,H,W,cs) -> (B,ceil(H/2),ceil(W/2),4 cs): out[Y][X][(py * 2 + px) * cs + c] = in[2Y + py][2X + px][c], zeros beyond
    the odd row / column - the parity order (dy, dx) of the stem (tests/dense_conv_ref.py)"""
    B, H, W, cs = x.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, 2 * H2, 2 * W2, cs), dtype=F32)
    xp[:, :H, :W] = x
    out = np.zeros((B, H2, W2, 4 * cs), dtype=F32)
    for py in range(2):
        for px in range(2):
            out[..., (py * 2 + px) * cs:(py * 2 + px + 1) * cs] = xp[:, py::2, px::2]
    return out


def maxpool_ref(x):
    """MaxPool2d(3, 2, 1) on NHWC fp32 through torch in fp64 (selection: the result is an fp32 number, NaN propagates)"""
    t = torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2)
    y = F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).contiguous().numpy()
    out = y.astype(F32)
    assert np.array_equal(out.astype(np.float64), y, equal_nan=True)
    return out


def maxpool_brute(x):
    """the same by loops: the first NaN met in a window is the answer, otherwise the largest tap inside the map"""
    B, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    out = np.full((B, Ho, Wo, C), -np.inf, dtype=F32)
    for yo in range(Ho):
        for xo in range(Wo):
            taps = [x[:, yy, xx] for yy in range(2 * yo - 1, 2 * yo + 2) if 0 <= yy < H
                    for xx in range(2 * xo - 1, 2 * xo + 2) if 0 <= xx < W]
            t = np.stack(taps)                                      # (taps, B, C)
            m = np.where(np.isnan(t).any(axis=0), F32(np.nan), np.nanmax(np.where(np.isnan(t), -np.inf, t), axis=0))
            out[:, yo, xo] = m
    return out


def resize_nearest_ref(x, hd, wd):
    """F.interpolate(mode='nearest') on planes (P,hs,ws): a gather through the fp32 tables"""
    P, hs, ws = x.shape
    return np.ascontiguousarray(x[:, nearest_table(hs, hd)][:, :, nearest_table(ws, wd)])


def nearest_exact_table(insize, outsize):
    return np.minimum((np.arange(outsize, dtype=np.int64) * insize) // outsize, insize - 1)


# ------------------------------------------------------------------------------------------------ bilinear
def bilinear_src(o, insize, outsize, align):
    """the exact source coordinate of output index o as a Fraction (the rule of the module docstring)"""
    if align:
        return Fraction(o * (insize - 1), outsize - 1) if outsize > 1 else Fraction(0)
    return max(Fraction(0), Fraction((2 * o + 1) * insize, 2 * outsize) - Fraction(1, 2))


def bilinear_weights(insize, outsize, align):
    """the (out, in) matrix W of the rule along one axis from the exact src, and dW, the error of the kernel's fp32 weights.

    The kernel forms   align: sc = fl(fl(in - 1) / fl(out - 1)) (u), src = fl(sc * o) (u):            |dsrc| <= 2 u src
                       else:  sc = fl(in / out) (u), t = fl(sc * (o + 1/2)) (u), src = fl(t - 1/2) (u |src|), t = src + 1/2:
                                                                                                     |dsrc| <= 2 u (src + 1/2) + u src
    i0 = trunc(src) and l = src - i0 are exact on the fp32 src; 1 - l is one rounding (u), and at a clamped edge both weights
    meet on one pixel (u more).  So every weight is off by at most dW = dsrc + 2 u.  An fp32 src that lands across an integer
    moves that much weight to the next pixel, so dW stands on the two taps and on their outer neighbours.  (For the 2x case
    this is step_tail_ref.up2_weights' dW = 2 u src + 2 u.)  in = 1: one pixel carries both weights; dW = 0 and the rounding
    of (1 - l) v + l v is part of the six operations counted in bilinear_ref."""
    W, dW = np.zeros((outsize, insize)), np.zeros((outsize, insize))
    for o in range(outsize):
        src = bilinear_src(o, insize, outsize, align)
        i0 = min(int(src), insize - 1)
        i1 = i0 + (1 if i0 < insize - 1 else 0)
        l = float(src - i0)
        W[o, i0] += 1 - l
        W[o, i1] += l
        if insize > 1:
            s = float(src)
            dsrc = 2 * U * s if align else 2 * U * (s + 0.5) + U * s
            dW[o, max(i0 - 1, 0):min(i1 + 1, insize - 1) + 1] = dsrc + 2 * U
    return W, dW


def bilinear_taps_fp32(insize, outsize, align):
    """the kernel's bilinear_taps restated in numpy float32 -> (i0, i1, l) arrays; the host test holds it inside dW"""
    o = np.arange(outsize, dtype=F32)
    if align:
        sc = F32(insize - 1) / F32(outsize - 1) if outsize > 1 else F32(0)
        src = (sc * o).astype(F32)
    else:
        sc = F32(insize) / F32(outsize)
        src = ((sc * (o + F32(0.5))).astype(F32) - F32(0.5)).astype(F32)
        src = np.where(src < 0, F32(0), src)
    i0 = np.minimum(src.astype(np.int64), insize - 1)
    i1 = i0 + (i0 < insize - 1)
    return i0, i1, (src - i0.astype(F32)).astype(F32)


def bilinear_bound(Wy, dWy, Wx, dWx, ax, t):
    """|x| through (dWy x |Wx| + |Wy| x dWx + dWy x dWx) for the weights, and 6 u |Wy| |x| |Wx| for the six rounded operations
    of  (1 - ly) * ((1 - lx) a + lx b) + ly * ((1 - lx) c + lx d)  (a value passes two products and two sums; six is the
    count of operations on the longest expression and covers the case where both taps are one pixel)"""
    aWy, aWx = np.abs(Wy), np.abs(Wx)
    return K2 * (t(dWy, ax, aWx) + t(aWy, ax, dWx) + t(dWy, ax, dWx) + 6 * U * t(aWy, ax, aWx))


def bilinear_ref(x, hd, wd, align):
    """sfh_resize_nchw mode 1 on planes (P,hs,ws) -> (values (P,hd,wd) fp64, bound)"""
    x = f64(x)
    P, hs, ws = x.shape
    Wy, dWy = bilinear_weights(hs, hd, align)
    Wx, dWx = bilinear_weights(ws, wd, align)
    t = lambda a, v, b: np.matmul(np.matmul(a, v), b.T)             # "oy,pyx,qx->poq"
    return t(Wy, x, Wx), bilinear_bound(Wy, dWy, Wx, dWx, np.abs(x), t)


def up2_ref(x):
    """sfh_upsample2x_bilinear_nhwc on (B,H,W,C) -> (values (B,2H,2W,C) fp64, bound): Wy x Wx of step_tail_ref.up2_weights,
    the matrices of the backward test, through the same bound as bilinear_ref"""
    x = f64(x)
    B, H, W, C = x.shape
    Wy, dWy = up2_weights(H)
    Wx, dWx = up2_weights(W)
    t = lambda a, v, b: np.einsum("oy,byxc,qx->boqc", a, v, b, optimize=True)
    return t(Wy, x, Wx), bilinear_bound(Wy, dWy, Wx, dWx, np.abs(x), t)


def dot_bound(a, b_a, w):
    """the error of sum(a_kernel * w) accumulated in fp64 on the host, a_kernel within b_a of a: sum |w| b_a, plus the fp64
    sum itself (n * 2^-53 * sum |a w|, the products of two floats are exact in fp64)"""
    a, w = f64(a), f64(w)
    return float((np.abs(w) * b_a).sum() + a.size * S.E53 * (np.abs(a * w) + np.abs(w) * b_a).sum())


# ------------------------------------------------------------------------------------------------ sfh_fold_bn
def fold_bn_ref(cb, gamma, beta, mean, var, eps, n, repeat):
    """scale[i] = a[i % n], shift[i] = ((cb - mean) a + beta)[i % n], a = gamma / sqrt(var + eps), for i < n * repeat.

    Kernel: s = var + eps (u), r = sqrtf(s) (u/2 inherited + u), inv = 1 / r (u), a = gamma * inv (u): 3.5 u |a|.
    d = cb - mean (u |d|; d itself is exact input: a cancellation leaves a small d and a small bound), d * a carries
    |d| da + u |d a| (d's own rounding) + u |d a| (the product), the sum u |shift|.
    Without gamma: scale = 1 and shift = cb, both exact (bound 0)."""
    cbv = np.zeros(n) if cb is None else f64(cb)
    if gamma is None:
        a, sh, ba, bs = np.ones(n), cbv, np.zeros(n), np.zeros(n)
    else:
        a = f64(gamma) / np.sqrt(f64(var) + float(F32(eps)))
        da = 3.5 * U * np.abs(a)
        d = cbv - f64(mean)
        sh = d * a + f64(beta)
        ba = K2 * da
        bs = K2 * (np.abs(d) * da + 2 * U * np.abs(d * a) + U * np.abs(sh))
    idx = np.arange(n * repeat) % n
    return a[idx], sh[idx], ba[idx], bs[idx]


# ------------------------------------------------------------------------------------------------ sfh_outconv_fwd
def outconv_ref(x, w, bias):
    """logits (B,nc,H,W) fp64 from NHWC x (B,H,W,cin), w (nc,cin), bias (nc), and the per-logit bound.

    The kernel's tree: each of two threads takes cin / 2 channels in groups of four - four products (u), three sums, one add
    into the accumulator - then one shuffle add joins the halves and the bias is added.  The longest path of a product:
    1 + 3 + cin / 8 + 1 + 1 roundings, so gamma = (cin / 8 + 6) u over sum |x w| + |bias|."""
    x, w, bias = f64(x), f64(w), f64(bias)
    cin = x.shape[-1]
    lg = np.einsum("bhwc,kc->bkhw", x, w) + bias[None, :, None, None]
    A = np.einsum("bhwc,kc->bkhw", np.abs(x), np.abs(w)) + np.abs(bias)[None, :, None, None]
    return lg, K2 * (cin // 8 + 6) * U * A


def argmax_scan(logits):
    """the kernel's rule on (B,nc,H,W) fp32 logits: best = 0; for k = 1 ..: if l[k] > l[best]: best = k"""
    l = np.asarray(logits)
    best = np.zeros(l[:, 0].shape, dtype=np.int64)
    bv = l[:, 0].copy()
    for k in range(1, l.shape[1]):
        with np.errstate(invalid="ignore"):
            win = l[:, k] > bv
        best = np.where(win, k, best)
        bv = np.where(win, l[:, k], bv)
    return best.astype(np.uint8)


def top2_margin(logits):
    s = np.sort(f64(logits), axis=1)
    return s[:, -1] - s[:, -2]


def stn_in_ref(logits, frame, stn_cs):
    """(B,H,W,stn_cs): the logits' bits, the frame's first three channels' bits, then +0.0"""
    B, nc, H, W = logits.shape
    out = np.zeros((B, H, W, stn_cs), dtype=F32)
    out[..., :nc] = logits.transpose(0, 2, 3, 1)
    out[..., nc:nc + 3] = frame[..., :3]
    return out


# ------------------------------------------------------------------------------------------------ sfh_consistency_ce_fwd
CE_PIX_PER_BLOCK = 2048


def ce_workspace_floats(B, H, W):
    return B * ((H * W + CE_PIX_PER_BLOCK - 1) // CE_PIX_PER_BLOCK)


def ce_targets(mask, H, W):
    """mask (B,hm,wm) -> (B,H,W): itself at the logits' size, otherwise gathered through nearest_table per axis"""
    B, hm, wm = mask.shape
    if (hm, wm) == (H, W):
        return mask
    return mask[:, nearest_table(hm, H)][:, :, nearest_table(wm, W)]


def ce_ref(logits, mask, t_ulps=T):
    """score (B,) longdouble = mean over pixels of logsumexp(l) - l[target], and its bound.

    Per pixel (step_tail_ref._softmax_parts, the kernel's own order: z = l - mx, expf, the sum, logf, + mx): dlse, and u |term|
    for the subtraction of l[target].  The sum in fp32: a thread adds at most 8 terms, the wave tree 6 levels, the block 4
    adds, the final kernel ceil(partials / 64) adds per lane and 6 levels: n adds on the longest path, n u sum |term| (the
    terms are >= 0).  inv_hw = fl(1 / HW) and the product: 2 u |score|."""
    l = f64(logits)
    B, nc, H, W = l.shape
    N = H * W
    tgt = ce_targets(np.asarray(mask), H, W).reshape(B, N).astype(np.int64)
    l = l.reshape(B, nc, N)
    sm = S._softmax_parts(l, t_ulps)
    xt = np.take_along_axis(l, tgt[:, None, :], axis=1)[:, 0]
    term = sm["lse"] - xt
    dterm = sm["dlse"] + U * np.abs(term)
    bpi = (N + CE_PIX_PER_BLOCK - 1) // CE_PIX_PER_BLOCK
    n_add = 8 + 6 + 4 + (bpi + 63) // 64 + 6
    score = term.astype(S.LD).sum(axis=1) / N
    A = np.abs(term).sum(axis=1) / N
    bound = K2 * (dterm.sum(axis=1) / N + n_add * U * A + 2 * U * np.abs(score.astype(np.float64)))
    return score, bound


def ce_brute(logits, mask):
    """pixel by pixel with math.log / math.exp and the nearest rule restated as scalars in fp32"""
    B, nc, H, W = logits.shape
    _, hm, wm = mask.shape
    out = []
    for b in range(B):
        tot = 0.0
        for y in range(H):
            for x in range(W):
                if (hm, wm) == (H, W):
                    t = mask[b, y, x]
                else:
                    ys = min(int(math.floor(F32(y) * (F32(hm) / F32(H)))), hm - 1)
                    xs = min(int(math.floor(F32(x) * (F32(wm) / F32(W)))), wm - 1)
                    t = mask[b, ys, xs]
                v = [float(logits[b, k, y, x]) for k in range(nc)]
                m = max(v)
                tot += m + math.log(sum(math.exp(a - m) for a in v)) - v[t]
        out.append(tot / (H * W))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ sfh_avgpool_linear_fwd
def avgpool_linear_ref(x, w, b):
    """feat (B,C) = the channel means of NHWC x, out (B,nout) = w feat + b, with their bounds.

    feat: four slices of pixels (i mod 4), each summed in four chains 16 pixels apart, the tail (fewer than four pixels per
    slice) onto the first chain: at most ceil(HW / 16) + 3 adds on a chain, 2 for (s0 + s1) + (s2 + s3), 2 for the four
    slices, then the division: (ceil(HW / 16) + 7) u mean |x| + u |feat|.
    out: a lane adds ceil(C / 64) products (u each), 6 shuffle levels, the bias: (ceil(C / 64) + 8) u (sum |w feat| + |b|),
    and feat's own bound through |w|."""
    x, w, b = f64(x), f64(w), f64(b)
    B, H, W, C = x.shape
    HW = H * W
    feat = x.reshape(B, HW, C).mean(axis=1)
    n = -(-HW // 16) + 3 + 4
    b_feat = K2 * (n * U * np.abs(x).reshape(B, HW, C).mean(axis=1) + U * np.abs(feat))
    out = feat @ w.T + b
    m = -(-C // 64) + 8
    b_out = K2 * (b_feat @ np.abs(w).T + m * U * (np.abs(feat) @ np.abs(w).T + np.abs(b)))
    return feat, b_feat, out, b_out


# ------------------------------------------------------------------------------------------------ sfh_compose_up_weights
def up_tap(p, k):
    """conv tap k at output parity p reads up-sampled row 2 (Y + s) + d: window slot a = s + 1 - p, sub-position d"""
    t = p + k - 1
    s = -1 if t < 0 else t >> 1
    return s + 1 - p, t & 1


def tap_inside(cls, k):
    """border class of an output row / column: 0 the first of the up-sampled tensor (tap 0 outside), 2 its last (tap 2
    outside), 3 the padded one after it (only tap 0 inside), 1 the interior"""
    return cls == 1 or (cls == 0 and k != 0) or (cls == 2 and k != 2) or (cls == 3 and k == 0)


def compose_up_ref(wconv, c0, wt, bt, scale4, shift4):
    """w2 (4 cout, cx, 2, 2) and shift_border (16, 4 cout) in fp64 with bounds: the composition the kernel's comment states,
    as an explicit sum over conv taps (ky, kx), window slots (a, b), sub-positions (dy, dx) and intermediate channels cu:

      w2[(py 2 + px) cout + co, x, a, b] = sum over (ky, kx) with up_tap(py, ky) = (a, dy), up_tap(px, kx) = (b, dx) and over cu
                                           of wconv[co, c0 + cu, ky, kx] wt[x, cu, dy, dx]
      shift_border[4 cy + cx, cv] = shift4[cv] + scale4[cv] sum over the taps inside (cy, cx) of sum_cu wconv[co, c0 + cu, ky, kx] bt[cu]

    Bounds: a tap sum runs over c1 products (u + c1 u), a window slot collects at most 4 of them: (c1 + 5) u sum |wconv| |wt|;
    the bias: (c1 + 1) u per tap sum and at most 9 taps, |scale| (c1 + 10) u sum |wconv| |bt|, then the product and the sum."""
    wc, wt, bt, sc, sh = (f64(a) for a in (wconv, wt, bt, scale4, shift4))
    cout, cx, c1 = wc.shape[0], wt.shape[0], wt.shape[1]
    wu = wc[:, c0:c0 + c1]
    w2, A = np.zeros((2, 2, cout, cx, 2, 2)), np.zeros((2, 2, cout, cx, 2, 2))
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    (a, dy), (b, dx) = up_tap(py, ky), up_tap(px, kx)          # the einsum, one (tap, tap) term at a time
                    w2[py, px, :, :, a, b] += wu[:, :, ky, kx] @ wt[:, :, dy, dx].T
                    A[py, px, :, :, a, b] += np.abs(wu[:, :, ky, kx]) @ np.abs(wt[:, :, dy, dx]).T
    w2, A = w2.reshape(4 * cout, cx, 2, 2), A.reshape(4 * cout, cx, 2, 2)
    b_w2 = K2 * (c1 + 5) * U * A
    tb = np.einsum("ockl,c->okl", wu, bt)
    ta = np.einsum("ockl,c->okl", np.abs(wu), np.abs(bt))
    sb, b_sb = np.zeros((16, 4 * cout)), np.zeros((16, 4 * cout))
    for cy in range(4):
        for cxx in range(4):
            m = np.array([[tap_inside(cy, ky) and tap_inside(cxx, kx) for kx in range(3)] for ky in range(3)], dtype=np.float64)
            acc = np.tile((tb * m).sum(axis=(1, 2)), 4)
            aacc = np.tile((ta * m).sum(axis=(1, 2)), 4)
            v = sh + sc * acc
            sb[cy * 4 + cxx] = v
            b_sb[cy * 4 + cxx] = K2 * (np.abs(sc) * (c1 + 10) * U * aacc + U * np.abs(sc * acc) + U * np.abs(v))
    return w2, b_w2, sb, b_sb


def border_class(r, n_up, padded):
    """class of output row r of the conv over an up-sampled tensor of n_up rows (one padded row behind it if `padded`)"""
    if r == 0:
        return 0
    if padded and r == n_up:
        return 3
    return 2 if r == n_up - 1 else 1
