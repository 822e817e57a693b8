"""fp64 CPU references (test infrastructure only) for the kernels that open and close a training step (csrc/train_step.hip):

  sfh_train_losses, sfh_reproj_loss, sfh_uv_loss (and their _det siblings), sfh_rmsprop_step, sfh_sgd_step, sfh_adam_step,
  sfh_multi_copy, sfh_multi_copy_dscale, sfh_grad_scale

and the two resize backward kernels of csrc/pointwise.hip, sfh_upsample2x_bilinear_nhwc_bwd and sfh_resize_nearest_nchw_bwd.
(sfh_multi_copy is a gather: its reference is numpy's strided view, and one correctly rounded fp32 multiply.)

Plain numpy; nothing here imports the library.  Every reference computes in fp64 (np.longdouble for the sums over pixels)
from the fp32 inputs and returns, beside its values, a per-element bound.  A bound is a count of the kernel's roundings
(u = 2^-24 each) over the reference's own ABSOLUTE quantities, times 1.01 for the second-order terms and the reference's own
fp64 error (0.01 u = 2^-30.6, far above 2^-53 per operation); none is fitted to a kernel's output.  The library is built
without multiply-add contraction; a contraction would remove a rounding, never add one.

T.  The error of expf, logf and sqrtf on the device is carried as T ulps (1 ulp = 2 u relative).  T = 2 is a margin over the
1 ulp a device math library usually documents; it has not been measured on the device.  numpy's float32 exp / log / sqrt -
the host restatement of tests/test_step_tail_host.py - stay inside every bound with T = 1.  The optimizers' sqrtf and the
divisions everywhere are IEEE operations (one rounding, u): HIP compiles fp32 divide and sqrt correctly rounded by default.

Underflow.  An fp32 result below 2^-126 may be flushed: ETA = 2^-126 is added once wherever an exponential or a product of
probabilities can get there (the spread-200 logits), and only where the bound is not structurally zero.

Decision rules are not arithmetic to approximate; the references take them as the operations define them:

  consistency target   tc = clamp(trunc(fl32(warp * fl32(nc))), 0, nc - 1): the fp32 product is the reference project's own
                       (warp_mask * nc).to(long); the clamp is this project's addition (torch raises at warp = 1).
  reconstruction target  fl32(fl32(gt) / fl32(nc)), one IEEE division; d = warp - target in fp64.
  SmoothL1 branch      |d| < 1 on the fp64 d.  The kernel decides on the fp32 d.  At |d| = 1 both branches give 1/2 and both
                       gradients 1 and the first derivatives agree, so a decision taken on a d that is off by delta <= u
                       changes the term by delta^2 / 2 and the gradient by delta: both inside the rounding of d that the
                       bound counts anyway.  No exception is made for it, and `ad <= 1.f` in the kernel would pass as well.
  clip                 clamp as torch.clamp_: NaN stays NaN, +-inf go to +-clip, -0 stays -0.
  reprojection         dist == 0 gives the gradient 0 (torch: NaN) - the kernel's stated rule.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
E53 = 2.0 ** -53
E64 = 2.0 ** -64
ETA = 2.0 ** -126
T = 2.0                  # ulps of expf / logf / sqrtf on the device (see the module docstring); not measured
K2 = 1.01                # second-order terms and the reference's own fp64 error
LD = np.longdouble
F32 = np.float32
FOCAL_EPS_Q = float(F32(1e-8))    # the kernel's 1e-8f / 1e-6f, exactly
FOCAL_EPS_T = float(F32(1e-6))


def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def ratio(got, ref, bound):
    """max |got - ref| / bound, the difference in longdouble; a zero bound demands exactness; NaN must meet NaN"""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref.astype(np.float64))
    assert (np.isnan(got.astype(np.float64)) == nan).all(), "NaN where the reference has none (or the reverse)"
    err = np.abs(np.where(nan, 0, got).astype(LD) - np.where(nan, 0, ref).astype(LD)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference leaves no room"
    ok = (bound > 0) & ~nan
    return float((err[ok] / bound[ok]).max(initial=0.0))


def sum64_bound(n, A, pre=0.0):
    """an fp64 sum of n fp32-born terms in a free order onto `pre`: n additions of 2^-53 on partial sums <= A + |pre|, and the
    reference's longdouble sum (n * 2^-64 * A); zero where every term is zero"""
    A = np.asarray(A, dtype=np.float64)
    return n * (E53 + E64) * (A + np.abs(np.asarray(pre, dtype=np.float64))) * (A > 0)


# ------------------------------------------------------------------------------------------------ decision rules
def consistency_target(warp, nc):
    """tc = clamp(trunc(fl32(warp * fl32(nc))), 0, nc - 1) on fp32 warp values (any shape) -> int64"""
    prod = (np.asarray(warp, dtype=F32) * F32(nc)).astype(F32)
    return np.clip(np.trunc(prod.astype(np.float64)), 0, nc - 1).astype(np.int64)


def rec_target(gt, nc):
    """fl32(fl32(gt) / fl32(nc)) as fp64"""
    return (np.asarray(gt).astype(F32) / F32(nc)).astype(F32).astype(np.float64)


def pointwise_loss(d, mse):
    """(term, d term / d d) of MSE or SmoothL1(beta 1) on fp64 differences"""
    ad = np.abs(d)
    if mse:
        return d * d, 2.0 * d
    return np.where(ad < 1.0, 0.5 * d * d, ad - 0.5), np.where(ad < 1.0, d, np.sign(d))


# ------------------------------------------------------------------------------------------------ sfh_train_losses
def _softmax_parts(l, t_ulps):
    """l (B, nc, N) fp64 -> the shared per-pixel quantities with their absolute error bounds (d*), following the kernel:
    z = l - mx (u |z|); e = expf(z) (2 T u e, the argument's error with weight e, ETA); se = sum e ((nc - 1) u se);
    rs = 1 / se and p = e * rs (2 u p, ETA); lse = logf(se) + mx (2 T u |log se| + dse / se, then u |lse|)."""
    nc = l.shape[1]
    mx = l.max(axis=1, keepdims=True)
    z = l - mx
    dz = U * np.abs(z)
    e = np.exp(z)
    de = e * (2 * t_ulps * U + dz) + ETA
    se = e.sum(axis=1, keepdims=True)
    dse = de.sum(axis=1, keepdims=True) + (nc - 1) * U * se
    p = e / se
    dp = de / se + p * dse / se + 2 * U * p + ETA
    logse = np.log(se)
    lse = logse + mx
    dlse = 2 * t_ulps * U * np.abs(logse) + dse / se + U * np.abs(lse)
    return dict(p=p, dp=dp, lse=lse[:, 0], dlse=dlse[:, 0])


def _cls_term(l, sm, tgt, focal, coef, t_ulps, eps_q, eps_t):
    """one classification term at every pixel: (term (B,N), its error, c (B,nc,N) = coef * d term / d l, its error).
    coef (B,1,1) is the product of three floats and the fp32 `inv` (5 u relative, counted below).

    CE     term = lse - l[tgt]: dlse + u |term|.  c_k = coef (p_k - o_k): |coef| (dp_k + u |p_k - o_k|) + 6 u |c_k|.
    focal  q = p + eps_q (dp + u q); t = o + eps_t (u t); om = 1 - q (dq + u |om|); lg = logf(q) (2 T u |lg| + dq / q);
           term_k = t om^2 (-lg): 4 u |term_k| + t (2 |om lg| dom + om^2 dlg); the sum over k adds (nc - 1) u sum |term_k|.
           a = 2 om lg (u |a| + 2 |lg| dom + 2 |om| dlg); b = om^2 / q (2 u b + 2 |om| dom / q + b dq / q);
           dLdp = t (a - b): D = t (da + db + u (|a| + |b|)) + 2 u t (|a| + |b|);
           dot = sum dLdp p: Ddot = sum (D p + |dLdp| dp) + nc u sum |dLdp p|;
           c_k = coef p_k (dLdp_k - dot): |coef| p_k (D_k + Ddot + u (|dLdp_k| + |dot|)) + |coef| (|dLdp_k| + |dot|) (7 u p_k + dp_k)."""
    B, nc, N = l.shape
    p, dp = sm["p"], sm["dp"]
    o = (np.arange(nc)[None, :, None] == tgt[:, None, :]).astype(np.float64)
    ac = np.abs(coef)
    if not focal:
        lt = np.take_along_axis(l, tgt[:, None, :], axis=1)[:, 0]
        term = sm["lse"] - lt
        dterm = sm["dlse"] + U * np.abs(term)
        c = coef * (p - o)
        dc = ac * (dp + U * np.abs(p - o)) + 6 * U * np.abs(c)
        return term, dterm, c, dc
    q = p + eps_q
    dq = dp + U * q
    t = o + eps_t
    om = 1.0 - q
    dom = dq + U * np.abs(om)
    lg = np.log(q)
    dlg = 2 * t_ulps * U * np.abs(lg) + dq / q
    tk = t * om * om * (-lg)
    dtk = 4 * U * np.abs(tk) + t * (2 * np.abs(om * lg) * dom + om * om * dlg)
    term = tk.sum(axis=1)
    dterm = dtk.sum(axis=1) + (nc - 1) * U * np.abs(tk).sum(axis=1)
    a = 2 * om * lg
    da = U * np.abs(a) + 2 * np.abs(lg) * dom + 2 * np.abs(om) * dlg
    b = om * om / q
    db = 2 * U * b + 2 * np.abs(om) * dom / q + b * dq / q
    dLdp = t * (a - b)
    D = t * (da + db + U * (np.abs(a) + b)) + 2 * U * t * (np.abs(a) + b)
    dot = (dLdp * p).sum(axis=1, keepdims=True)
    Ddot = (D * p + np.abs(dLdp) * dp).sum(axis=1, keepdims=True) + nc * U * np.abs(dLdp * p).sum(axis=1, keepdims=True)
    mag = np.abs(dLdp) + np.abs(dot)
    c = coef * p * (dLdp - dot)
    dc = ac * p * (D + Ddot + U * mag) + ac * mag * (7 * U * p + dp)
    return term, dterm, c, dc


def losses_ref(logits, gt, weight, warp, lam_seg, lam_rec, rec_mse, lam_cons, focal_flags, pre=(0.0, 0.0, 0.0),
               t_ulps=T, eps_q=FOCAL_EPS_Q, eps_t=FOCAL_EPS_T):
    """sfh_train_losses on fp32 logits (B,nc,H,W), int64 gt (B,H,W), fp32 weight (B,), fp32 warp (B,H,W) or None; the lambdas
    are the floats the entry receives.  `pre`: what loss3 held before (the kernel accumulates).

      seg  = lam_seg  * mean_b(weight[b] * mean_pixels(cls(l, gt)))            cls = CE or focal (focal_flags bit 0)
      rec  = lam_rec  * mean_b(weight[b] * mean_pixels(pw(warp - fl32(gt / nc))))   pw = SmoothL1 or MSE
      cons = lam_cons * mean over all pixels of cls(l, tc)                      (focal_flags bit 1)
      focal: sum_k (onehot_k + eps_t) * -(1 - q_k)^2 log q_k, q = softmax + eps_q (gamma 2, alpha 1)

    Returns dlogits, dwarp (None without a warp), loss3 (longdouble, `pre` added), tc, and the bounds b_dlogits, b_dwarp,
    b_loss3.  Bounds:

      dlogits  1.01 * (sum over the active terms of dc (see _cls_term) + u * sum |c|, the rounding of the second += ) + ETA;
               exactly 0 where no term is active.
      dwarp    coef = lam * w * inv carries 5 u; d carries u |d|; the products 2 u more: 1.01 * (|coef| |g'| u |d| + 7 u |ref|)
               with g' = d^2 term / d d^2 (1 in the quadratic branch and MSE's 2, 0 beyond 1) - written as |coef| u |d| below.
      loss3    per pixel the fp32 term: w (dterm + u |term|) for a classification term, u w (|d| |g| + 2 |term|) for the
               pointwise one; 1.01 * lam * inv * their sum, plus 3 u |ref| for the fp32 `inv` = 1 / (HW * B), plus the fp64 sum
               over npix terms (sum64_bound: N * 2^-53 * A and the reference's longdouble sum), `pre` included."""
    lg = f64(logits)
    B, nc, H, W = lg.shape
    N = H * W
    l = lg.reshape(B, nc, N)
    gt = np.asarray(gt, dtype=np.int64).reshape(B, N)
    w = f64(weight).reshape(B, 1)
    inv = 1.0 / (N * B)
    lam_seg, lam_rec, lam_cons = (float(F32(x)) for x in (lam_seg, lam_rec, lam_cons))
    wv = None if warp is None else np.asarray(warp, dtype=F32).reshape(B, N)
    sm = _softmax_parts(l, t_ulps)
    dl, ddl, absc = np.zeros_like(l), np.zeros_like(l), np.zeros_like(l)
    loss = [LD(pre[0]), LD(pre[1]), LD(pre[2])]
    b_loss = [0.0, 0.0, 0.0]
    npix = B * N
    tc = consistency_target(wv, nc) if wv is not None else np.zeros((B, N), dtype=np.int64)

    def scalar(k, lam, val, err, pre_k):
        A = float(np.abs(val).sum()) * abs(lam) * inv
        ref = LD(lam) * LD(inv) * val.astype(LD).sum()
        loss[k] = LD(pre_k) + ref
        b_loss[k] = float(K2 * abs(lam) * inv * err.sum() + 3 * U * abs(float(ref)) + sum64_bound(npix, A, pre_k)) if A > 0 else 0.0

    if lam_seg != 0.0:
        term, dterm, c, dc = _cls_term(l, sm, gt, bool(focal_flags & 1), (lam_seg * w * inv)[:, :, None], t_ulps, eps_q, eps_t)
        dl += c; ddl += dc; absc += np.abs(c)
        scalar(0, lam_seg, w * term, w * (dterm + U * np.abs(term)), pre[0])
    if lam_cons != 0.0:
        term, dterm, c, dc = _cls_term(l, sm, tc, bool(focal_flags & 2), np.full((B, 1, 1), lam_cons * inv), t_ulps, eps_q, eps_t)
        dl += c; ddl += dc; absc += np.abs(c)
        scalar(2, lam_cons, term, dterm + U * np.abs(term), pre[2])
    active = lam_seg != 0.0 or lam_cons != 0.0
    b_dl = (K2 * (ddl + U * absc) + ETA) if active else np.zeros_like(l)
    out = dict(dlogits=dl.reshape(B, nc, H, W), b_dlogits=b_dl.reshape(B, nc, H, W), tc=tc.reshape(B, H, W), dwarp=None,
               b_dwarp=None)
    if wv is not None:
        d = wv.astype(np.float64) - rec_target(gt, nc)
        term, g = pointwise_loss(d, rec_mse)
        coef = lam_rec * w * inv
        dw = coef * g
        out["dwarp"] = dw.reshape(B, H, W)
        out["b_dwarp"] = (K2 * (np.abs(coef) * U * np.abs(d) * (2.0 if rec_mse else 1.0) + 7 * U * np.abs(dw))).reshape(B, H, W)
        if lam_rec != 0.0:
            scalar(1, lam_rec, w * term, U * w * (np.abs(d * g) + 2 * np.abs(term)), pre[1])
    out["loss3"] = np.array(loss, dtype=LD)
    out["b_loss3"] = np.array(b_loss)
    return out


# ------------------------------------------------------------------------------------------------ sfh_reproj_loss
def reproj_ref(poi, gt, nz, nn, lam, pre=0.0, t_ulps=T):
    """lam * mean_b(sum_n dist * nz / num_nonzero[b]), dist = |gt - poi|; dpoi = its gradient, 0 where dist == 0.

    Kernel roundings: sc = lam / (nn * B) 2 u; dx, dy u each; dx^2 + dy^2 4 u in all; sqrtf halves that and adds T ulps:
    (2 + 2 T) u; dist * nz u -> the term carries (3 + 2 T) u.  g = nz * sc / dist: u + 2 u + u + (2 + 2 T) u; -g * dx: 2 u more:
    dpoi within 1.01 * (8 + 2 T) u |ref|.  The loss: 1.01 * (5 + 2 T) u * sum |terms| (the term and the fp32 sc) plus the fp64 sums."""
    poi, gt, nz, nn = f64(poi), f64(gt), f64(nz), f64(nn)
    B, n = nz.shape
    lam = float(F32(lam))
    sc = (lam / (nn * B))[:, None]
    dx = gt - poi
    dist = np.sqrt((dx * dx).sum(axis=2))
    terms = dist * nz * sc
    loss = LD(pre) + terms.astype(LD).sum()
    A = float(np.abs(terms).sum())
    b_loss = float(K2 * (5 + 2 * t_ulps) * U * A + sum64_bound(B * n, A, pre)) if A > 0 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(dist > 0, nz * sc / dist, 0.0)
    dpoi = -g[:, :, None] * dx
    return dict(dpoi=dpoi, b_dpoi=K2 * (8 + 2 * t_ulps) * U * np.abs(dpoi), loss=loss, b_loss=b_loss)


# ------------------------------------------------------------------------------------------------ sfh_uv_loss
def uv_ref(uv, gt, weight, nweights, lam, mse, pre=0.0):
    """The header's rule: loss = lam * mean_{b,w}(weight[w or 0] * mean_{c,h} pw(uv - gt)) on (B,C,H,W), weights along the LAST
    axis, nweights in {1, W}; duv = its gradient.  inv = 1 / (B * C * H * W) is formed in fp32 from three products and a
    division (4 u); coef = lam * w * inv 6 u; d = uv - gt u |d|; two products: duv within 1.01 * (|coef| g' u |d| + 8 u |ref|).
    The scalar: u w (|d g| + 2 |term|) per element, 4 u |ref| for inv, the fp64 sum."""
    uv, gt, weight = f64(uv), f64(gt), f64(weight)
    B, C, H, W = uv.shape
    assert nweights in (1, W)
    lam = float(F32(lam))
    w = weight[:W] if (nweights == W and nweights != 1) else np.full(W, weight[0])
    inv = 1.0 / (B * C * H * W)
    d = uv - gt
    term, g = pointwise_loss(d, mse)
    coef = lam * w * inv
    duv = coef * g
    val = w * term
    A = float(np.abs(val).sum()) * abs(lam) * inv
    ref = LD(lam) * LD(inv) * val.astype(LD).sum()
    err = U * w * (np.abs(d * g) + 2 * np.abs(term))
    b_loss = float(K2 * abs(lam) * inv * err.sum() + 4 * U * abs(float(ref)) + sum64_bound(uv.size, A, pre)) if A > 0 else 0.0
    b_duv = K2 * (np.abs(coef) * U * np.abs(d) * (2.0 if mse else 1.0) + 8 * U * np.abs(duv))
    return dict(duv=duv, b_duv=b_duv, loss=LD(pre) + ref, b_loss=b_loss)


# ------------------------------------------------------------------------------------------------ optimizers
def clamp(g, clip):
    """torch.clamp_(-clip, clip): NaN stays, +-inf -> +-clip, -0 stays; clip <= 0: no clipping"""
    if not clip > 0:
        return g
    return np.where(g < -clip, -clip, np.where(g > clip, clip, g))


def complements(kind, hp, torch_like=False):
    """the gains 1 - beta of a rule, from the FLOATS the C entry receives.  Kernel rule: 1 - fl32(beta), exact (Sterbenz for
    beta >= 1/2, and a float below 1/2 with few enough bits).  torch_like: fl32(1 - beta_double), what torch forms from the
    Python double - `hp` then holds the doubles the user wrote."""
    names = {"rmsprop": ("alpha",), "adam": ("b1", "b2"), "sgd": ()}[kind]
    if torch_like:
        return tuple(float(F32(1.0 - float(hp[k]))) for k in names)
    return tuple(1.0 - float(F32(hp[k])) for k in names)


def opt_step(kind, state, grad, hp, step=1, comp=None, err_in=None, u=U, dcomp=None, cast=True):
    """One step of the kernel's documented rule in fp64, per element, with its error bound.

      g = clamp(grad * gscale, clip); g += wd * p
      rmsprop  sq' = alpha sq + c g g;  s = g / (sqrt(sq') + eps);  mu > 0: buf' = mu buf + s, s = buf';  p' = p - lr s
      sgd      mu > 0: buf' = mu buf + g, g = buf';  p' = p - lr g
      adam     m' = m + c1 (g - m);  v' = b2 v + c2 g g;  p' = p - (lr / bias1) * (m' / (sqrt(v') / sqrt(bias2) + eps)),
               bias_i = 1 - b_i^step formed in double from the floats (buf holds m, sq holds v)

    hp: lr, wd, clip, gscale and alpha, eps, mu | mu | b1, b2, eps - with cast=True rounded to the floats the C entry receives,
    with cast=False taken as the doubles they are (the fp64 comparison with torch.optim).  comp: the gains (c | c1, c2), default
    complements(kind, hp).  state: dict p, sq, buf of fp64 arrays.  Returns (new state, bounds) - a tensor the rule does not
    touch is returned as it came, with bound 0.

    Bound (u per rounding, every term over absolute values; err_in carries the bounds of an earlier step; dcomp = |difference
    of the gains| adds its first-order effect |dc| g^2 resp. |dc1| |g - m| - the distance between two rules):
      g0 = grad * gscale: u |g0|, and clamp is 1-Lipschitz: u |clamp g0|.   g = g0 + wd p: u |wd p| + wd dp + u |g|
      sq' / v': u |b sq| + b dsq + c (2 u g^2 + 2 |g| dg) + u |sq'|            (c * g * g: two products)
      r = sqrt(sq'): dsq' / (2 r) + u r;  avg = r + eps: + u avg      (adam: r / sqrt(bias2): 2 u more, the division and the float)
      s = g / avg: dg / avg + |s| davg / avg + u |s|
      buf' = mu buf + s: u |mu buf| + mu dbuf + ds + u |buf'|
      m' = m + c1 (g - m): dm + c1 (dg + dm + u |g - m|) + u c1 |g - m| + u |m'|
      p' = p - lr s: dp + 2 u |lr s| (+ u |lr s| for adam's float step size) + lr ds + u |p'|
    all times 1.01."""
    H = {k: (float(F32(v)) if cast else float(v)) for k, v in hp.items()}
    comp = complements(kind, hp) if comp is None else comp
    dcomp = (0.0,) * len(comp) if dcomp is None else dcomp
    e = {k: 0.0 for k in ("p", "sq", "buf")}
    if err_in:
        e.update(err_in)
    p, sq, buf = (f64(state[k]) for k in ("p", "sq", "buf"))
    ab = np.abs
    g0 = clamp(f64(grad) * H.get("gscale", 1.0), H["clip"])
    wd, lr = H["wd"], H["lr"]
    g = g0 + wd * p
    dg = u * ab(g0) + u * ab(wd * p) + wd * e["p"] + u * ab(g)
    new, bnd = dict(state), {k: np.zeros_like(p) for k in ("p", "sq", "buf")}
    bnd.update({k: e[k] + np.zeros_like(p) for k in e})          # untouched tensors keep what they came with

    def second_moment(b, c, dc):
        v = b * sq + c * g * g
        dv = u * ab(b * sq) + b * e["sq"] + c * (2 * u * g * g + 2 * ab(g) * dg) + u * ab(v) + dc * g * g
        r = np.sqrt(v)
        with np.errstate(divide="ignore", invalid="ignore"):
            dr = np.where(v > 0, dv / (2 * r), 0.0) + u * r
        return v, dv, r, dr

    if kind == "rmsprop":
        v, dv, r, dr = second_moment(H["alpha"], comp[0], dcomp[0])
        avg = r + H["eps"]
        davg = dr + u * avg
        s = g / avg
        ds = dg / avg + ab(s) * davg / avg + u * ab(s)
        new["sq"], bnd["sq"] = v, K2 * dv
        if H["mu"] > 0:
            nb = H["mu"] * buf + s
            ds = u * ab(H["mu"] * buf) + H["mu"] * e["buf"] + ds + u * ab(nb)
            s = nb
            new["buf"], bnd["buf"] = nb, K2 * ds
        extra = 0.0
    elif kind == "sgd":
        s, ds = g, dg
        if H["mu"] > 0:
            nb = H["mu"] * buf + g
            ds = u * ab(H["mu"] * buf) + H["mu"] * e["buf"] + dg + u * ab(nb)
            s = nb
            new["buf"], bnd["buf"] = nb, K2 * ds
        extra = 0.0
    else:
        assert kind == "adam" and step >= 1
        c1, c2 = comp
        m = buf + c1 * (g - buf)
        dm = e["buf"] + c1 * (dg + e["buf"] + u * ab(g - buf)) + u * c1 * ab(g - buf) + u * ab(m) + dcomp[0] * ab(g - buf)
        v, dv, r, dr = second_moment(H["b2"], c2, dcomp[1])
        bias1, bias2 = 1.0 - H["b1"] ** step, 1.0 - H["b2"] ** step
        rb = r / math.sqrt(bias2)
        denom = rb + H["eps"]
        dden = dr / math.sqrt(bias2) + 2 * u * rb + u * denom
        s = m / denom
        ds = dm / denom + ab(s) * dden / denom + u * ab(s)
        lr = lr / bias1
        extra = u * ab(lr * s)
        new["buf"], bnd["buf"] = m, K2 * dm
        new["sq"], bnd["sq"] = v, K2 * dv
    pn = p - lr * s
    new["p"] = pn
    bnd["p"] = K2 * (e["p"] + 2 * u * ab(lr * s) + extra + lr * ds + u * ab(pn))
    return new, bnd


# ------------------------------------------------------------------------------------------------ sfh_grad_scale
def _frac(bits):
    """the non-negative finite float with these bits, exactly"""
    ex, man = (bits >> 23) & 255, bits & 0x7FFFFF
    return Fraction(man, 1 << 149) if ex == 0 else Fraction((1 << 23) | man) * Fraction(2) ** (ex - 150)


def _frexp_e(bits):
    """e with value = f * 2^e, 1/2 <= f < 1 (value > 0), on the bit pattern"""
    ex, man = (bits >> 23) & 255, bits & 0x7FFFFF
    return man.bit_length() - 149 if ex == 0 else ex - 126


def grad_scale_ref(words, nheads, has_theta, shift, overflow_in=0):
    """The header's paragraph on the bit patterns (Python integers and Fractions only).  words: 2 per tensor, word 2 i = the
    bits of max |x| of tensor i (heads first, then theta).  Returns (S, 1 / S as Fractions, overflow word).

      a word >= 0x7F800000 (Inf or NaN): overflow |= 2, S = 1
      m = the largest head (no heads: theta); m > 0: S = 2^(target - e), target = (2 | 13) + shift, m = f 2^e
      heads and theta > 0 and theta * S < 2^-16: S2 = 2^(-15 - e_theta); largest head * S2 >= 64: overflow |= 4, else S = S2"""
    hb = [int(words[2 * i]) for i in range(nheads)]
    tb = int(words[2 * nheads]) if has_theta else 0
    over = int(overflow_in)
    S = Fraction(1)
    if any(b >= 0x7F800000 for b in hb) or (has_theta and tb >= 0x7F800000):
        return S, S, over | 2
    mh = max(hb, default=0)
    mt = tb
    mb = mh if nheads > 0 else mt
    target = (2 if nheads > 0 else 13) + shift
    if mb > 0:
        S = Fraction(2) ** (target - _frexp_e(mb))
    if nheads > 0 and mt > 0 and _frac(mt) * S < Fraction(1, 1 << 16):
        S2 = Fraction(2) ** (-15 - _frexp_e(mt))
        if _frac(mh) * S2 >= 64:
            over |= 4
        else:
            S = S2
    return S, 1 / S, over


def grad_scale_brute(words, nheads, has_theta, shift, overflow_in=0):
    """the same rule by search over S = 2^k: the k that puts the largest value into [2^(target-1), 2^target), then the
    smallest S2 = 2^j with theta * S2 >= 2^-16"""
    hb = [int(words[2 * i]) for i in range(nheads)]
    tb = int(words[2 * nheads]) if has_theta else 0
    over = int(overflow_in)
    if any(b >= 0x7F800000 for b in hb + ([tb] if has_theta else [])):
        return Fraction(1), Fraction(1), over | 2
    mh = max([_frac(b) for b in hb], default=Fraction(0))
    mt = _frac(tb)
    m = mh if nheads > 0 else mt
    target = (2 if nheads > 0 else 13) + shift
    S = Fraction(1)
    if m > 0:
        (S,) = [Fraction(2) ** k for k in range(-200, 200)
                if Fraction(2) ** (target - 1) <= m * Fraction(2) ** k < Fraction(2) ** target]
    if nheads > 0 and mt > 0 and mt * S < Fraction(1, 1 << 16):
        S2 = min(Fraction(2) ** j for j in range(-200, 200) if mt * Fraction(2) ** j >= Fraction(1, 1 << 16))
        if mh * S2 >= 64:
            over |= 4
        else:
            S = S2
    return S, 1 / S, over


# ------------------------------------------------------------------------------------------------ resize backward
def nearest_table(insize, outsize):
    """F.interpolate(mode='nearest'), the rule sfh_resize_nchw mode 0 states: source index min(floor(fl32(o * s)), in - 1)
    with s = fl32(fl32(in) / fl32(out)) - decisions taken in fp32, so the table is computed in fp32.  (The Pillow / OpenCV
    tables of tests/resample_ref.py and sfh_nearest_tab belong to the dataset resize, another operation.)"""
    s = F32(insize) / F32(outsize)
    o = np.arange(outsize, dtype=F32)
    return np.minimum(np.floor((o * s).astype(F32)).astype(np.int64), insize - 1)


def nearest_bwd_ref(dy, hs, ws):
    """sfh_resize_nearest_nchw_bwd: dy (planes, hd, wd) -> (dx (planes, hs, ws) fp64, bound): the transpose of the gather.  A
    source pixel sums its n readers in fp32: (n - 1) u sum |dy| (no second order, Jeannerod and Rump); one reader or none: exact."""
    dy = f64(dy)
    P, hd, wd = dy.shape
    ty, tx = nearest_table(hs, hd), nearest_table(ws, wd)
    My = (ty[:, None] == np.arange(hs)[None]).astype(np.float64)
    Mx = (tx[:, None] == np.arange(ws)[None]).astype(np.float64)
    dx = np.einsum("oy,pow,wx->pyx", My, dy, Mx)
    A = np.einsum("oy,pow,wx->pyx", My, np.abs(dy), Mx)
    n = My.sum(axis=0)[:, None] * Mx.sum(axis=0)[None, :]
    return dx, (np.maximum(n - 1, 0) * U)[None] * A


def up2_weights(n):
    """the (2n, n) matrix of nn.Upsample(scale_factor=2, bilinear, align_corners=True) along one axis, from the exact source
    coordinate o (n - 1) / (2n - 1), and the error of the kernel's fp32 weights: sc = fl32((n - 1) / (2n - 1)) and src = sc * o
    carry 2 u src, 1 - l and (1 - l) + l at a clamped edge u each: dW = 2 u src + 2 u, on the two taps and their outer
    neighbours (an fp32 src that lands across an integer moves weight there).  n == 1: src = 0, weights exact."""
    W, dW = np.zeros((2 * n, n)), np.zeros((2 * n, n))
    for o in range(2 * n):
        src = Fraction(o * (n - 1), 2 * n - 1) if n > 1 else Fraction(0)
        i0 = min(int(src), n - 1)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        l = float(src - i0)
        W[o, i0] += 1 - l
        W[o, i1] += l
        if n > 1:
            dW[o, max(i0 - 1, 0):min(i1 + 1, n - 1) + 1] = 2 * U * float(src) + 2 * U
    return W, dW


def up2_bwd_ref(dy):
    """sfh_upsample2x_bilinear_nhwc_bwd: dy (B, 2H, 2W, C) -> (dx (B, H, W, C) fp64, bound) = Wy^T dy Wx per channel.
    The kernel forms wy * wx * g (2 u) and adds at most nt = (ny + 2)(nx + 2) taps in fp32 (ny, nx the taps of the exact map, two
    more for the neighbours above): 1.01 * (|dy| through (dWy x |Wx| + |Wy| x dWx + dWy x dWx) + (nt + 2) u |dy| through |Wy| x |Wx|)."""
    dy = f64(dy)
    B, H2, W2, C = dy.shape
    Wy, dWy = up2_weights(H2 // 2)
    Wx, dWx = up2_weights(W2 // 2)
    t = lambda a, g, b: np.einsum("oy,bopc,px->byxc", a, g, b)
    dx = t(Wy, dy, Wx)
    ady = np.abs(dy)
    nt = ((Wy != 0).sum(axis=0) + 2)[:, None] * ((Wx != 0).sum(axis=0) + 2)[None, :]
    bound = K2 * (t(dWy, ady, np.abs(Wx)) + t(np.abs(Wy), ady, dWx) + t(dWy, ady, dWx)
                  + ((nt + 2) * U)[None, :, :, None] * t(np.abs(Wy), ady, np.abs(Wx)))
    return dx, bound
