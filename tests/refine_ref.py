"""numpy restatement (test infrastructure only) of the refinement rule stated in include/sfh_amd.h above the sfh_refine_*
entries.  Nothing here imports the library.

Staging, as on the device: the coordinates, the bilinear weights, the per-class bilinear value and the two tap differences
are float32, one rounding per operation (numpy's float32 arithmetic rounds every operation; the fused multiply-adds of the
rule - xn = fmaf(ax, j, cx) and the un-normalisation - are formed as the fp64 expression rounded once, exact products as in
oracle/warp_ref.unnormalize); everything behind them is float64.  The Levenberg-Marquardt step is written out in the kernel's
operation order on Python floats (IEEE double, no contraction), candidates are rounded to float32.

BOUNDS.  None is fitted to a kernel's output.

sums_bound(A, n).  Device and restatement share the float32 stage operation for operation, so the per-pixel float32
  quantities are the same numbers; the differences are float64 only.  A per-pixel term of a sum is a fixed expression of at
  most 16 float64 operations on them (class sums of up to 8 products, the products a_i a_j, three products and two
  additions): its two evaluations differ by at most 16 * 2^-53 of the term's ABSOLUTE expression (every product and partial
  sum taken in absolute value) - that absolute expression, summed over the pixels, is A.  The n terms of a frame are then
  added in two different orders: (n - 1) additions of 2^-53 on partial sums of at most A, each side.  Together
  |got - ref| <= (2 n + 32) * 2^-53 * A, times K2 = 1.01 for the second-order terms.  A == 0 demands exact zero.

evidence_bound.  Follows tests/step_tail_ref._softmax_parts (T ulps for expf, T taken from there): z = l - max (u |z|),
  e = expf(z) (2 T u e, the argument's error with weight e, ETA for a flushed result), se = sum e ((nc - 1) u se),
  p = e / se (one IEEE division: u p), then the f^2 probabilities are added ((f^2 - 1) u S) and divided by f^2 (u).

cost_margin(npix, cost).  The cost of a theta is evaluated here by one rule for both sides (eval_cost: the restatement's own
  sums).  What has to be allowed for is that the device DECIDED accept / reject on its own evaluation of the same costs,
  which differs from this one within sums_bound of the cost sum, whose A is the cost itself (squares): (2 n + 32) 2^-53 c.
"""
import numpy as np

import step_tail_ref as ST
from chol8_ref import chol8_solve

F32 = np.float32
U = 2.0 ** -24
E53 = 2.0 ** -53
K2 = 1.01
SUMS = 45
EPS = F32(1e-8)
TILE_W, TILE_H = 64, 64


def channels(nc):
    return 4 if nc <= 5 else 8


def slabs(he, we):
    return -(-we // TILE_W) * -(-he // TILE_H)


# ------------------------------------------------------------------------------------------------ planes
def template_planes(tmpl, nc, f):
    """tmpl (N,ht,wt) float32 valued k/nc -> (N, ht/f, wt/f, CP) float32, exact"""
    tmpl = np.asarray(tmpl, dtype=F32)
    N, ht, wt = tmpl.shape
    ids = np.rint((tmpl * F32(nc)).astype(F32)).astype(np.int64)
    out = np.zeros((N, ht // f, wt // f, channels(nc)), dtype=F32)
    blocks = ids.reshape(N, ht // f, f, wt // f, f)
    for c in range(1, nc):
        out[..., c - 1] = ((blocks == c).sum(axis=(2, 4)).astype(F32) / F32(f * f)).astype(F32)
    return out


def evidence_planes(logits, f, t_ulps=ST.T):
    """logits (B,nc,hl,wl) float32 -> (planes (B, hl/f, wl/f, CP) float64, bound of the same shape)"""
    l = np.asarray(logits, dtype=np.float64)
    B, nc, hl, wl = l.shape
    mx = l.max(axis=1, keepdims=True)
    z = l - mx
    dz = U * np.abs(z)
    e = np.exp(z)
    de = e * (2 * t_ulps * U + dz) + ST.ETA
    se = e.sum(axis=1, keepdims=True)
    dse = de.sum(axis=1, keepdims=True) + (nc - 1) * U * se
    p = e / se
    dp = de / se + p * dse / se + U * p + ST.ETA
    blk = lambda a: a.reshape(B, nc, hl // f, f, wl // f, f)
    S, dS = blk(p).sum(axis=(3, 5)), blk(dp).sum(axis=(3, 5))
    dS = dS + (f * f - 1) * U * S
    out, dout = S / (f * f), dS / (f * f) + U * S / (f * f)
    cp = channels(nc)
    planes, bound = np.zeros((B, hl // f, wl // f, cp)), np.zeros((B, hl // f, wl // f, cp))
    planes[..., :nc - 1] = np.moveaxis(out[:, 1:], 1, -1)
    bound[..., :nc - 1] = K2 * np.moveaxis(dout[:, 1:], 1, -1)
    return planes, bound


def evidence_planes_f32(logits, f):
    """the float32 restatement of the evidence kernel (numpy's exp in place of expf): what the restatement's own refinement
    runs on"""
    l = np.asarray(logits, dtype=F32)
    B, nc, hl, wl = l.shape
    e = np.exp((l - l.max(axis=1, keepdims=True)).astype(F32)).astype(F32)
    se = np.zeros_like(e[:, 0])
    for k in range(nc):
        se = (se + e[:, k]).astype(F32)
    out = np.zeros((B, hl // f, wl // f, channels(nc)), dtype=F32)
    for c in range(1, nc):
        p = (e[:, c] / se).astype(F32).reshape(B, hl // f, f, wl // f, f)
        s = np.zeros((B, hl // f, wl // f), dtype=F32)
        for dy in range(f):
            for dx in range(f):
                s = (s + p[:, :, dy, :, dx]).astype(F32)
        out[..., c - 1] = (s / F32(f * f)).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ coordinates
def axis(f, n, nl):
    """(ax, cx) as float32: ax = 2 f n / (nl (n - 1)), cx = (f n / nl - 1) / (n - 1) - 1, evaluated in fp64, rounded once"""
    return F32((2.0 * f * n) / (float(nl) * (n - 1))), F32(((float(f) * n / nl - 1.0) / (n - 1)) - 1.0)


def _fma32(a, b, c):
    """fl32(a * b + c) for float32 a, b, c: the fp64 product is exact"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def grid(f, H, W, hl, wl):
    ax, cx = axis(f, W, wl)
    ay, cy = axis(f, H, hl)
    xn = _fma32(ax, np.arange(wl // f, dtype=F32), cx)
    yn = _fma32(ay, np.arange(hl // f, dtype=F32), cy)
    return xn, yn


def coords(theta, xn, yn):
    """theta (B,9) float32 -> X, Y, Z, s, live (B,he,we) and xn, yn broadcast, in the pinned order of the warp"""
    t = [np.asarray(theta, dtype=F32).reshape(-1, 9)[:, k].reshape(-1, 1, 1) for k in range(9)]
    x = xn.reshape(1, 1, -1).astype(F32)
    y = yn.reshape(1, -1, 1).astype(F32)
    with np.errstate(all="ignore"):
        X = ((t[0] * x + t[1] * y) + t[2]).astype(F32)
        Y = ((t[3] * x + t[4] * y) + t[5]).astype(F32)
        Z = ((t[6] * x + t[7] * y) + t[8]).astype(F32)
        live = np.abs(Z) > EPS
        s = np.where(live, F32(1.0) / (Z + EPS), F32(1.0)).astype(F32)
    shape = X.shape
    return X, Y, Z, s, live, np.broadcast_to(x, shape), np.broadcast_to(y, shape)


def _taps(tp, x0, y0):
    """zero-padded taps of tp (B,htf,wtf,CP) at integral-valued float32 (x0, y0) (B,he,we) (NaN / inf: zero) -> (B,he,we,CP)"""
    B, htf, wtf, _ = tp.shape
    with np.errstate(invalid="ignore"):
        ok = (x0 >= 0) & (x0 <= wtf - 1) & (y0 >= 0) & (y0 <= htf - 1)
    ix = np.where(ok, x0, 0).astype(np.int64)
    iy = np.where(ok, y0, 0).astype(np.int64)
    bb = np.arange(B).reshape(B, 1, 1)
    return np.where(ok[..., None], tp[bb, iy, ix], F32(0.0)).astype(F32)


def pixel_terms(theta, tplanes, eplanes, H, W, f):
    """the per-pixel float64 quantities of the rule.  tplanes (B|1, ht/f, wt/f, CP), eplanes (B, hl/f, wl/f, CP) float32.
    Returns dict: S* the six class sums (B,he,we), their absolute versions A*, a, b (8,B,he,we)."""
    theta = np.asarray(theta, dtype=F32).reshape(-1, 9)
    B = theta.shape[0]
    tp = np.asarray(tplanes, dtype=F32)
    tp = np.broadcast_to(tp[:1], (B,) + tp.shape[1:]) if tp.shape[0] == 1 else tp[:B]
    ev = np.asarray(eplanes, dtype=F32)
    _, he, we, cp = ev.shape
    htf, wtf = tp.shape[1], tp.shape[2]
    xn, yn = grid(f, H, W, he * f, we * f)
    X, Y, Z, s, live, xb, yb = coords(theta, xn, yn)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        px = _fma32((s * X + one).astype(F32), F32(0.5 * wtf), F32(-0.5))
        py = _fma32((s * Y + one).astype(F32), F32(0.5 * htf), F32(-0.5))
        x0, y0 = np.floor(px), np.floor(py)
        wx1, wy1 = (px - x0).astype(F32), (py - y0).astype(F32)
        wx0, wy0 = (one - wx1).astype(F32), (one - wy1).astype(F32)
        t00, t01 = _taps(tp, x0, y0), _taps(tp, x0 + one, y0)
        t10, t11 = _taps(tp, x0, y0 + one), _taps(tp, x0 + one, y0 + one)
        w = [(a * b).astype(F32)[..., None] for a, b in ((wy0, wx0), (wy0, wx1), (wy1, wx0), (wy1, wx1))]
        val = (t00 * w[0]).astype(F32)
        for t, ww in ((t01, w[1]), (t10, w[2]), (t11, w[3])):
            val = (val + (t * ww).astype(F32)).astype(F32)
        e = lambda a: a[..., None]
        duf = ((e(wy0) * (t01 - t00).astype(F32)).astype(F32) + (e(wy1) * (t11 - t10).astype(F32)).astype(F32)).astype(F32)
        dvf = ((e(wx0) * (t10 - t00).astype(F32)).astype(F32) + (e(wx1) * (t11 - t01).astype(F32)).astype(F32)).astype(F32)
        assert val.dtype == F32 and duf.dtype == F32 and dvf.dtype == F32
        r = val.astype(np.float64) - ev.astype(np.float64)
        du, dv = duf.astype(np.float64) * (0.5 * wtf), dvf.astype(np.float64) * (0.5 * htf)
        out = {}
        for name, p in (("uu", du * du), ("uv", du * dv), ("vv", dv * dv), ("ur", du * r), ("vr", dv * r), ("rr", r * r)):
            acc, aacc = np.zeros(p.shape[:-1]), np.zeros(p.shape[:-1])
            for c in range(cp):                     # the kernel's class order
                acc = acc + p[..., c]
                aacc = aacc + np.abs(p[..., c])
            out["S" + name], out["A" + name] = acc, aacc
        ds, dx, dy = s.astype(np.float64), xb.astype(np.float64), yb.astype(np.float64)
        gu = np.where(live, -(X.astype(np.float64) * ds) * ds, 0.0)
        gv = np.where(live, -(Y.astype(np.float64) * ds) * ds, 0.0)
        z = np.zeros_like(ds)
        out["a"] = np.stack([ds * dx, ds * dy, ds, z, z, z, gu * dx, gu * dy])
        out["b"] = np.stack([z, z, z, ds * dx, ds * dy, ds, gv * dx, gv * dy])
    return out


def sums(theta, tplanes, eplanes, H, W, f, want_A=True):
    """the 45 sums per frame and A = sum of the absolute per-pixel expressions: (S (B,45), A (B,45))"""
    q = pixel_terms(theta, tplanes, eplanes, H, W, f)
    a, b = q["a"], q["b"]
    B = a.shape[1]
    S, A = np.zeros((B, SUMS)), np.zeros((B, SUMS))
    tot = lambda v: v.reshape(B, -1).sum(axis=1)
    with np.errstate(all="ignore"):
        e = 0
        for i in range(8):
            for j in range(i, 8):
                S[:, e] = tot((q["Suu"] * (a[i] * a[j]) + q["Suv"] * (a[i] * b[j] + b[i] * a[j])) + q["Svv"] * (b[i] * b[j]))
                if want_A:
                    A[:, e] = tot(q["Auu"] * np.abs(a[i] * a[j]) + q["Auv"] * (np.abs(a[i] * b[j]) + np.abs(b[i] * a[j]))
                                  + q["Avv"] * np.abs(b[i] * b[j]))
                e += 1
        for i in range(8):
            S[:, 36 + i] = tot(q["Sur"] * a[i] + q["Svr"] * b[i])
            if want_A:
                A[:, 36 + i] = tot(q["Aur"] * np.abs(a[i]) + q["Avr"] * np.abs(b[i]))
        S[:, 44] = tot(q["Srr"])
        A[:, 44] = tot(q["Arr"])
    return S, A


def sums_bound(A, npix):
    return K2 * (2 * npix + 32) * E53 * np.asarray(A, dtype=np.float64)


def cost_margin(npix, cost):
    return K2 * (2 * npix + 32) * E53 * float(cost)


# ------------------------------------------------------------------------------------------------ step
def lm_system(S, lam):
    """(L, b): the lower triangle of J^T J + lam diag(J^T J) as an 8 x 8 list of lists and b = -J^T r, from the 45 sums, as
    refine_step_kernel fills them"""
    S = [float(v) for v in S]
    L = [[0.0] * 8 for _ in range(8)]
    e = 0
    for i in range(8):
        for j in range(i, 8):
            L[j][i] = S[e] + lam * S[e] if i == j else S[e]
            e += 1
    return L, [-S[36 + i] for i in range(8)]


def lm_solve(S, lam):
    """(delta[8], ok) of (J^T J + lam diag) delta = -J^T r from the 45 sums (chol8_ref)"""
    L, g = lm_system(S, lam)
    ok = chol8_solve(L, g, True)
    return g, ok


def candidate(theta_acc, delta, ok):
    """(candidate (9,) float32, tie (9,) bool): tie marks an entry whose fp64 sum lies within 2^-40 (relative) of a float32
    rounding boundary - there one ulp of float64 in delta may move the float32 result by one ulp"""
    ta = np.asarray(theta_acc, dtype=F32).reshape(9)
    cand, tie = ta.copy(), np.zeros(9, dtype=bool)
    if ok:
        for k in range(8):
            v = float(ta[k]) + delta[k]
            cand[k] = F32(v)
            with np.errstate(all="ignore"):
                tie[k] = F32(v * (1 - 2.0 ** -40)) != F32(v * (1 + 2.0 ** -40))
    return cand, tie


class StepState:
    """the per-frame state of sfh_refine_step, one frame"""

    def __init__(self):
        self.theta = self.S = None
        self.lam, self.ok, self.accepted, self.cost_first = 1e-3, False, 0, None

    def step(self, S, theta_eval, first, last):
        """-> (theta_next (9,) float32, tie)"""
        S = np.asarray(S, dtype=np.float64)
        if first:
            take, self.lam, self.accepted, self.cost_first = True, 1e-3, 0, float(S[44])
        else:
            take = bool(self.ok and S[44] < self.S[44])
            self.lam = self.lam / 10.0 if take else self.lam * 10.0
            self.accepted += int(take)
        if take:
            self.theta, self.S = np.asarray(theta_eval, dtype=F32).reshape(9).copy(), S.copy()
        self.delta, self.ok = lm_solve(self.S, self.lam)
        if last:
            return self.theta.copy(), np.zeros(9, dtype=bool)
        return candidate(self.theta, self.delta, self.ok)


def refine(theta, tplanes_by_level, eplanes_by_level, H, W, factors=(4, 2, 1), iters=5):
    """the whole schedule, frame by frame: theta (B,9) float32 -> dict theta (B,9) float32, cost (B,L,2), accepted (B,L)"""
    theta = np.asarray(theta, dtype=F32).reshape(-1, 9)
    B, L = theta.shape[0], len(factors)
    out = {"theta": theta.copy(), "cost": np.zeros((B, L, 2)), "accepted": np.zeros((B, L), dtype=np.int32)}
    for b in range(B):
        cur = theta[b].copy()
        for li, f in enumerate(factors):
            tp = tplanes_by_level[li]
            tp = tp[:1] if tp.shape[0] == 1 else tp[b:b + 1]
            ev = eplanes_by_level[li][b:b + 1]
            ev_sums = lambda t: sums(t.reshape(1, 9), tp, ev, H, W, f, want_A=False)[0][0]
            st = StepState()
            cand, _ = st.step(ev_sums(cur), cur, True, iters == 0)
            for it in range(iters):
                cand, _ = st.step(ev_sums(cand), cand, False, it == iters - 1)
            cur = cand
            out["cost"][b, li] = (st.cost_first, st.S[44])
            out["accepted"][b, li] = st.accepted
        out["theta"][b] = cur
    return out


def eval_cost(theta, tplanes, eplanes, H, W, f):
    """the one evaluation of the cost both sides are measured with: (B,) float64"""
    return sums(theta, tplanes, eplanes, H, W, f, want_A=False)[0][:, 44]


# ------------------------------------------------------------------------------------------------ geometry of a result
def corner_px(theta, wt, ht):
    """the four frame corners (xn, yn = +-1) in template pixels, fp64: (B,4,2)"""
    t = np.asarray(theta, dtype=np.float64).reshape(-1, 9)
    out = []
    for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        Z = t[:, 6] * x + t[:, 7] * y + t[:, 8]
        u, v = (t[:, 0] * x + t[:, 1] * y + t[:, 2]) / Z, (t[:, 3] * x + t[:, 4] * y + t[:, 5]) / Z
        out.append(np.stack([(u + 1) * wt / 2 - 0.5, (v + 1) * ht / 2 - 0.5], axis=-1))
    return np.stack(out, axis=1)


def corner_error(theta, theta_true, wt, ht):
    """largest displacement of the four frame corners from theta_true, template pixels: (B,)"""
    d = corner_px(theta, wt, ht) - corner_px(theta_true, wt, ht)
    return np.sqrt((d ** 2).sum(axis=-1)).max(axis=1)
