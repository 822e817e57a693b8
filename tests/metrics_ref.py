"""numpy restatement of the three rules stated in include/sfh_amd.h above the sfh_metrics_* entries: confusion counts, region
counts, point errors.  It does not import the library.  Every fp64 operation is a separate numpy call, so each is rounded on
its own (numpy never contracts a product and a sum), in the order the header writes them.

THE ONE BOUND (point errors).  The products, sums, quotients and square roots behind the error e_n of a counted point are IEEE
operations, correctly rounded, applied in the header's order on both sides; so the device's e_n and its choice of counted points
are this restatement's, bit for bit, and n is exact.  What differs is the ORDER of the sum: the device adds the points of a lane
in turn and the 64 lanes by a shuffle tree, numpy adds pairwise.  With u = 2^-53 and gamma_k = k u / (1 - k u), any order of
summing n terms in fp64 gives |fl(S) - S| <= gamma_{n-1} sum |e_n| (Higham, Accuracy and Stability, 4.2), and the mean is one
more division, fl(S / n) = (S / n)(1 + d), |d| <= u.  Against the exact mean m = sum e_n / n each side is therefore within
(gamma_{n-1} (1 + u) + u) mean|e|, and the two sides within twice that of each other:

    bound = 2 (gamma_{n-1} (1 + u) + u) (sum |e_n| / n),    sum |e_n| by math.fsum (exact up to one rounding, absorbed by 1 + 4u)

There is no per-point term, on purpose: a device e_n that differs in one bit (a contracted multiply-add, a square root that
is not correctly rounded) breaks the stated rule and must fail.  A mean that is not finite (no counted point: 0 / 0; a theta_pred
that is not usable: NaN terms) must be non-finite on both sides - NaN where the reference has NaN, the same infinity otherwise.
"""
import math

import numpy as np

U = 2.0 ** -53
IGNORE = -100


def _quiet(fn):
    def run(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


# ------------------------------------------------------------------------------------------------ matrices and the predicate
@_quiet
def adj_checked(theta):
    """theta: 9 float32 -> (m, adj, usable): fp64 copies, both the zero matrix where det is not finite or 0"""
    t = np.asarray(theta, dtype=np.float32).reshape(9).astype(np.float64)
    a = np.empty(9)
    a[0] = t[4] * t[8] - t[5] * t[7]
    a[1] = t[2] * t[7] - t[1] * t[8]
    a[2] = t[1] * t[5] - t[2] * t[4]
    a[3] = t[5] * t[6] - t[3] * t[8]
    a[4] = t[0] * t[8] - t[2] * t[6]
    a[5] = t[2] * t[3] - t[0] * t[5]
    a[6] = t[3] * t[7] - t[4] * t[6]
    a[7] = t[1] * t[6] - t[0] * t[7]
    a[8] = t[0] * t[4] - t[1] * t[3]
    det = (t[0] * a[0] + t[1] * a[3]) + t[2] * a[6]
    ok = bool(np.isfinite(det) and det != 0.0)
    if not ok:
        return np.zeros(9), np.zeros(9), False
    return t, a, True


@_quiet
def apply3(M, a, b, c):
    X = (M[0] * a + M[1] * b) + M[2] * c
    Y = (M[3] * a + M[4] * b) + M[5] * c
    W = (M[6] * a + M[7] * b) + M[8] * c
    return X, Y, W


@_quiet
def inside(X, Y, W, signed=False):
    """the predicate; signed=True is the W > 0 variant that the rule deliberately is NOT (host test only)"""
    if signed:
        return (W > 0) & (np.abs(X) <= W) & (np.abs(Y) <= W)
    w = np.abs(W)
    return (w > 0) & (np.abs(X) <= w) & (np.abs(Y) <= w)


@_quiet
def compose(g, a):
    """theta_gt * adj(theta_pred), entry (i, j) = (g[i][0] a[0][j] + g[i][1] a[1][j]) + g[i][2] a[2][j]"""
    out = np.empty(9)
    for i in range(3):
        for j in range(3):
            out[3 * i + j] = (g[3 * i] * a[j] + g[3 * i + 1] * a[3 + j]) + g[3 * i + 2] * a[6 + j]
    return out


# ------------------------------------------------------------------------------------------------ confusion
def argmax_rule(logits):
    """logits (B,nc,H,W) float32 -> ids: best = 0; for k = 1 .. nc-1: if logit[k] > logit[best] then best = k (the rule above
    sfh_outconv_fwd: first index on ties, a NaN never compares greater)"""
    L = np.asarray(logits, dtype=np.float32)
    best, idx = L[:, 0].copy(), np.zeros(L[:, 0].shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(1, L.shape[1]):
            up = L[:, k] > best
            best = np.where(up, L[:, k], best)
            idx = np.where(up, k, idx)
    return idx


def predicted_classes(pred, kind, nc):
    """-> (ids int64 (B,H,W), valid bool (B,H,W)) for pred_kind 0 int32 ids, 1 uint8 ids, 2 logits, 3 warp mask k / nc"""
    if kind in (0, 1):
        p = np.asarray(pred).astype(np.int64)
        ok = (p >= 0) & (p < nc)
    elif kind == 2:
        p = argmax_rule(pred)
        ok = np.ones(p.shape, dtype=bool)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.asarray(pred, dtype=np.float32) * np.float32(nc)          # one fp32 product
            ok = (f > np.float32(-1)) & (f < np.float32(nc))
            p = np.where(ok, np.trunc(np.where(ok, f, 0)), 0).astype(np.int64)
    return np.where(ok, p, 0), ok


def confusion_ref(pred, kind, gt, nc):
    """-> (counts int64 (B,nc,nc) [gt][pred], flag): np.add.at over the pixels with a valid gt id and a valid class"""
    gt = np.asarray(gt, dtype=np.int64)
    p, pok = predicted_classes(pred, kind, nc)
    gok = (gt >= 0) & (gt < nc)
    flag = (1 if ((gt != IGNORE) & ~gok).any() else 0) | (2 if (~pok).any() else 0)
    out = np.zeros((gt.shape[0], nc, nc), dtype=np.int64)
    use = gok & pok
    b = np.broadcast_to(np.arange(gt.shape[0])[:, None, None], gt.shape)
    np.add.at(out, (b[use], gt[use], p[use]), 1)
    return out, flag


# ------------------------------------------------------------------------------------------------ region
def region_matrices(theta_pred, theta_gt, mode):
    mp, ap, okp = adj_checked(theta_pred)
    mg, ag, okg = adj_checked(theta_gt)
    if mode == 0:
        return ap, ag
    return (compose(mg, ap) if (okp and okg) else np.zeros(9)), np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


def canvas(wc, hc, mx, my):
    """q = (a, b, c) of every canvas pixel: exact integers as fp64"""
    x = np.arange(-mx, wc + mx, dtype=np.int64)
    y = np.arange(-my, hc + my, dtype=np.int64)
    a = ((2 * x - (wc - 1)) * (hc - 1)).astype(np.float64)[None, :]
    b = ((2 * y - (hc - 1)) * (wc - 1)).astype(np.float64)[:, None]
    assert max(np.abs(a).max(), np.abs(b).max()) < 2.0 ** 53
    return a, b, float((wc - 1) * (hc - 1))


def region_ref(theta_pred, theta_gt, mode, wc, hc, mx, my, signed=False):
    """theta (B,9) float32 each -> int64 (B,3) = [nA, nB, nAB]"""
    tp, tg = np.asarray(theta_pred, np.float32).reshape(-1, 9), np.asarray(theta_gt, np.float32).reshape(-1, 9)
    a, b, c = canvas(wc, hc, mx, my)
    out = np.zeros((len(tp), 3), dtype=np.int64)
    for f in range(len(tp)):
        A, B = region_matrices(tp[f], tg[f], mode)
        ia, ib = inside(*apply3(A, a, b, c), signed=signed), inside(*apply3(B, a, b, c), signed=signed)
        out[f] = ia.sum(), ib.sum(), (ia & ib).sum()
    return out


# ------------------------------------------------------------------------------------------------ points
@_quiet
def point_error(Mg, Mp, x, y, sx, sy):
    Xg, Yg, Wg = apply3(Mg, x, y, 1.0)
    Xp, Yp, Wp = apply3(Mp, x, y, 1.0)
    dx = (Xp / Wp - Xg / Wg) * sx
    dy = (Yp / Wp - Yg / Wg) * sy
    return np.sqrt(dx * dx + dy * dy), inside(Xg, Yg, Wg)


def lattice(gx, gy):
    k, l = np.arange(gx, dtype=np.float64), np.arange(gy, dtype=np.float64)
    x = -1.0 + (2.0 * k + 1.0) / float(gx)
    y = -1.0 + (2.0 * l + 1.0) / float(gy)
    return np.tile(x, gy), np.repeat(y, gx)          # row-major: n = l gx + k


def _mean_and_bound(e, counted):
    v = e[counted]
    n = int(v.size)
    if n == 0:
        return float("nan"), 0.0, n
    with np.errstate(all="ignore"):
        mean = float(np.sum(v) / n)
    if not np.isfinite(v).all():
        return mean, 0.0, n
    g = (n - 1) * U / (1.0 - (n - 1) * U)
    return mean, 2.0 * (g * (1.0 + U) + U) * (math.fsum(np.abs(v)) / n) * (1.0 + 4 * U), n


def points_ref(theta_pred, theta_gt, court_pts, gx, gy, frame_sx, frame_sy, court_sx, court_sy):
    """-> (out (B,4) = [reproj_mean, n_pts, proj_mean, n_lattice], bound (B,4)): the bound of the module docstring for the two
    means (0 where the mean must be exact or is not finite), 0 for the two counts"""
    tp, tg = np.asarray(theta_pred, np.float32).reshape(-1, 9), np.asarray(theta_gt, np.float32).reshape(-1, 9)
    pts = np.asarray(court_pts, dtype=np.float64).reshape(-1, 2)
    lx, ly = lattice(gx, gy)
    out, bound = np.zeros((len(tp), 4)), np.zeros((len(tp), 4))
    for f in range(len(tp)):
        mp, ap, _ = adj_checked(tp[f])
        mg, ag, _ = adj_checked(tg[f])
        e, c = point_error(ag, ap, pts[:, 0], pts[:, 1], frame_sx, frame_sy)
        out[f, 0], bound[f, 0], out[f, 1] = _mean_and_bound(e, c)
        e, c = point_error(mg, mp, lx, ly, court_sx, court_sy)
        out[f, 2], bound[f, 2], out[f, 3] = _mean_and_bound(e, c)
    return out, bound


def points_ratio(got, want, bound):
    """largest |got - want| / bound over the finite means; asserts the rest of the contract: counts exact, a zero bound means
    equality, a non-finite reference mean is met by NaN for NaN and by the same infinity otherwise"""
    got, want, bound = (np.asarray(v, dtype=np.float64) for v in (got, want, bound))
    assert got.shape == want.shape == bound.shape
    assert np.array_equal(got[:, 1], want[:, 1]) and np.array_equal(got[:, 3], want[:, 3]), (got[:, [1, 3]], want[:, [1, 3]])
    worst = 0.0
    for col in (0, 2):
        for f in range(len(want)):
            g, w, b = got[f, col], want[f, col], bound[f, col]
            if not np.isfinite(w):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (f, col, g, w)
            elif b == 0.0:
                assert g == w, (f, col, g, w)
            else:
                worst = max(worst, abs(g - w) / b)
    return worst
