"""numpy restatement (test infrastructure only) of the UV homography fit stated in include/sfh_amd.h above the sfh_uvfit_*
entries.  Nothing here imports the library.

Staging, as on the device: the pixel centres are float32 (x = fmaf(ax, j, cx0), formed as the fp64 expression rounded once -
the fp64 product of two float32 values is exact), the gate compares float32 values, and everything behind that is float64,
one rounding per operation (numpy's float64 arithmetic rounds every operation; the library is compiled with
-ffp-contract=off, so the device does too).  The step is written out in the kernel's operation order on Python floats.

BOUNDS.  None is fitted to a kernel's output.

sums_bound(A, n).  Device and restatement evaluate a pixel's term by the same IEEE operations on the same float32 inputs, in
  the same order: the terms are the same numbers, and the two sides differ only in the ORDER in which the n terms of a frame
  are added - (n - 1) additions of 2^-53 relative error on partial sums of at most A = sum |term| on each side, 2 n 2^-53 A
  together.  The constant c = 16 on top is for a compiler that contracts: behind omega a term is at most 3 products (q m[e]: cx
  cx, + cy cy, q * m) on top of m's 2, 6 roundings in all (counting q's addition), and a fused evaluation removes at most one
  rounding per operation - at most 6 * 2^-53 |term| per side, 12 together, rounded up to 16.  What NO constant of this form
  covers is a contracted evaluation of omega itself ((X / Wd - cx) cancels): that is why contraction is off for the whole
  library, and the bound is stated for the build as it is.  Times K2 = 1.01 for second-order terms.  A == 0 demands exact zero.

theta_margin_px(theta, wt, ht).  The court-pixel size of 64 float32 ulps of theta: a corner (x, y = +-1) moves by at most
  |dX| / |Wd| + |X| |dWd| / Wd^2 in normalised units for entry-wise changes d_k = 64 * 2^-24 |theta_k| (64 ulps are at most that),
  dX <= d0 + d1 + d2, dWd <= d6 + d7 (theta8 = 1 is exact), times wt / 2 (ht / 2); the two axes combined in quadrature, the
  largest of the four corners.
"""
import numpy as np

from chol8_ref import chol8_solve

F32 = np.float32
E53 = 2.0 ** -53
K2 = 1.01
SUMS = 27
TILE_W, TILE_H = 64, 64
DBL_MAX = np.finfo(np.float64).max


def slabs(h, w):
    return -(-w // TILE_W) * -(-h // TILE_H)


def axis(n, nl):
    """(a, c) float32 of sfh_refine_axis(1, n, nl): a = 2 n / (nl (n - 1)), c = (n / nl - 1) / (n - 1) - 1 in fp64, rounded once"""
    return F32((2.0 * n) / (float(nl) * (n - 1))), F32(((float(n) / nl - 1.0) / (n - 1)) - 1.0)


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def grid(H, W, h, w):
    """the pixel centres x (w,), y (h,) as float64 values of float32 numbers"""
    ax, cx0 = axis(W, w)
    ay, cy0 = axis(H, h)
    return (_fma32(ax, np.arange(w, dtype=F32), cx0).astype(np.float64),
            _fma32(ay, np.arange(h, dtype=F32), cy0).astype(np.float64))


def constants(wt, ht):
    """(u_min, v_min) float32, (kx, ky) float"""
    return F32(0.5 / wt), F32(0.5 / ht), 1.0 + 1.0 / wt, 1.0 + 1.0 / ht


def classes(logits):
    """the argmax rule stated above sfh_outconv_fwd: strict > scan, first maximum; logits (B,nc,h,w) float32 -> (B,h,w)"""
    lg = np.asarray(logits, dtype=F32)
    best = np.zeros(lg[:, 0].shape, dtype=np.int64)
    lb = lg[:, 0].copy()
    for k in range(1, lg.shape[1]):
        with np.errstate(invalid="ignore"):
            up = lg[:, k] > lb
        lb = np.where(up, lg[:, k], lb)
        best = np.where(up, k, best)
    return best


def gate(uv, logits, wt, ht):
    u_min, v_min, _, _ = constants(wt, ht)
    uv = np.asarray(uv, dtype=F32)
    with np.errstate(invalid="ignore"):
        g = (uv[:, 0] > u_min) & (uv[:, 1] > v_min)
    if logits is not None:
        g = g & (classes(logits) != 0)
    return g


def pixel_terms(uv, logits, theta, H, W, wt, ht, delta=2.0):
    """-> dict: gate (B,h,w) bool, om, r2 (B,h,w) float64 (r2 None without a theta), x, y, cx, cy, terms (27,B,h,w) float64 with
    zeros where a pixel adds nothing"""
    uv = np.asarray(uv, dtype=F32)
    B, _, h, w = uv.shape
    g = gate(uv, logits, wt, ht)
    _, _, kx, ky = constants(wt, ht)
    xs, ys = grid(H, W, h, w)
    x = np.broadcast_to(xs.reshape(1, 1, w), (B, h, w))
    y = np.broadcast_to(ys.reshape(1, h, 1), (B, h, w))
    with np.errstate(all="ignore"):
        cx = 2.0 * uv[:, 0].astype(np.float64) - kx
        cy = 2.0 * uv[:, 1].astype(np.float64) - ky
        zero = np.zeros((B, h, w))
        if theta is None:
            om, r2, inl, t26 = np.ones((B, h, w)), None, zero, zero
        else:
            t = [np.asarray(theta, dtype=F32).reshape(B, 9)[:, k].astype(np.float64).reshape(B, 1, 1) for k in range(9)]
            X = (t[0] * x + t[1] * y) + t[2]
            Y = (t[3] * x + t[4] * y) + t[5]
            Wd = (t[6] * x + t[7] * y) + t[8]
            ex = (X / Wd - cx) * (0.5 * wt)
            ey = (Y / Wd - cy) * (0.5 * ht)
            r2 = ex * ex + ey * ey
            d2 = float(delta) * float(delta)
            c = 1.0 + r2 / d2
            live = (np.abs(Wd) > 1e-8) & (np.abs(r2) <= DBL_MAX)
            om = np.where(live, (1.0 / c) / (Wd * Wd), 0.0)
            inl = np.where(g & (r2 <= d2), 1.0, 0.0)
            t26 = np.where(g & (om != 0.0), r2 / c, 0.0)
        add = g & (om != 0.0)
        wx, wy = om * x, om * y
        m = [wx * x, wx * y, wy * y, wx, wy, om]
        q = cx * cx + cy * cy
        terms = (m + [cx * m[e] for e in range(5)] + [cy * m[e] for e in range(5)] + [q * m[e] for e in range(3)]
                 + [om * cx, om * cy, q * wx, q * wy, om * q])
        terms = [np.where(add, v, 0.0) for v in terms] + [np.where(g, 1.0, 0.0), inl, t26]
    return {"gate": g, "om": om, "r2": r2, "x": x, "y": y, "cx": cx, "cy": cy, "terms": np.stack(terms)}


def sums(uv, logits, theta, H, W, wt, ht, delta=2.0):
    """(S (B,27), A (B,27) = the sums of the absolute terms, n (B,))"""
    q = pixel_terms(uv, logits, theta, H, W, wt, ht, delta)
    T = q["terms"]
    B = T.shape[1]
    with np.errstate(all="ignore"):
        S = T.reshape(SUMS, B, -1).sum(axis=2).T
        A = np.abs(T).reshape(SUMS, B, -1).sum(axis=2).T
    return S, A, q["gate"].reshape(B, -1).sum(axis=1)


def sums_bound(A, n):
    return K2 * (2 * np.asarray(n, dtype=np.float64).reshape(-1, 1) + 16) * E53 * np.asarray(A, dtype=np.float64)


def near_delta(uv, logits, theta, H, W, wt, ht, delta=2.0, rel=1e-9):
    """the gated pixels whose r2 lies within a relative `rel` of delta^2: where the inlier count could legitimately differ"""
    q = pixel_terms(uv, logits, theta, H, W, wt, ht, delta)
    d2 = float(delta) ** 2
    with np.errstate(invalid="ignore"):
        return int((q["gate"] & (np.abs(q["r2"] - d2) <= rel * d2)).sum())


# ------------------------------------------------------------------------------------------------ step
def assemble(S):
    """(A 8 x 8 list, g list) from the 27 sums, by the header's table"""
    S = [float(v) for v in S]
    A = [[0.0] * 8 for _ in range(8)]
    P = [[S[0], S[1], S[3]], [S[1], S[2], S[4]], [S[3], S[4], S[5]]]
    for i in range(3):
        for k in range(3):
            A[i][k] = A[3 + i][3 + k] = P[i][k]
    for col, rows in ((6, ((6, 7, 9), (11, 12, 14))), (7, ((7, 8, 10), (12, 13, 15)))):
        for i in range(3):
            A[i][col] = -S[rows[0][i]]
            A[3 + i][col] = -S[rows[1][i]]
    A[6][6], A[6][7], A[7][7] = S[16], S[17], S[18]
    for i in range(8):
        for k in range(i):
            A[i][k] = A[k][i]
    return A, [S[9], S[10], S[19], S[14], S[15], S[20], -S[21], -S[22]]


def solve(S, allowed=True):
    """(h[8], ok) of A h = g as uvfit_step_kernel solves it (chol8_ref); ok is False for n < 4, a non-finite sum, a pivot not > 0"""
    A, g = assemble(S)
    ok = bool(allowed and float(S[24]) >= 4.0 and np.isfinite(np.asarray(S, dtype=np.float64)).all())
    ok = chol8_solve(A, g, ok)      # A and g are this call's own: overwritten by the factor and the solution
    return g, ok


def step(S, pass_, last, theta_eval, status_in):
    """one frame of sfh_uvfit_step -> (theta_next (9,) float32, status, stats (4,) float64, tie (9,) bool).  tie marks an entry
    whose fp64 solution lies within 2^-40 (relative) of a float32 rounding boundary: both sides run the same IEEE operations,
    so their fp64 solutions are equal and the distance that could separate them is zero - the flag guards against a square
    root or a division that were off by an fp64 ulp (2^-53 relative per operation, < 2^-40 after the < 200 operations of a
    solve on these well-conditioned systems)"""
    S = np.asarray(S, dtype=np.float64)
    solved = int(status_in) if pass_ > 0 else 0
    dead = solved < pass_
    te = np.full(9, np.nan, dtype=F32) if theta_eval is None else np.asarray(theta_eval, dtype=F32).reshape(9).copy()
    hv, ok = solve(S, allowed=not dead and not last)
    tn, tie = te.copy(), np.zeros(9, dtype=bool)
    if ok:
        for k in range(8):
            tn[k] = F32(hv[k])
            with np.errstate(all="ignore"):
                tie[k] = F32(hv[k] * (1 - 2.0 ** -40)) != F32(hv[k] * (1 + 2.0 ** -40))
        tn[8] = F32(1.0)
    A, g = assemble(S)
    quad = lin = 0.0
    with np.errstate(all="ignore"):
        for i in range(8):
            row = 0.0
            for k in range(8):
                row += A[i][k] * float(tn[k])
            quad += float(tn[i]) * row
            lin += float(tn[i]) * g[i]
        stats = np.array([S[24], S[25], np.sqrt(np.float64(S[26]) / np.float64(S[24])), (quad - 2.0 * lin) + float(S[23])])
    return tn, solved + int(ok), stats, tie


def fit(uv, logits, theta0, H, W, wt, ht, iters=4, delta=2.0):
    """the whole schedule -> dict theta (B,9) float32, stats (B,4), status (B,) int32"""
    uv = np.asarray(uv, dtype=F32)
    B = uv.shape[0]
    cur = None if theta0 is None else np.asarray(theta0, dtype=F32).reshape(B, 9).copy()
    status, stats = np.zeros(B, dtype=np.int32), np.zeros((B, 4))
    for k in range(iters + 2):
        last = k == iters + 1
        S, _, _ = sums(uv, logits, cur, H, W, wt, ht, delta)
        nxt = np.zeros((B, 9), dtype=F32)
        for b in range(B):
            nxt[b], status[b], stats[b], _ = step(S[b], k, last, None if cur is None else cur[b], status[b])
        cur = nxt
    return {"theta": cur, "stats": stats, "status": status}


# ------------------------------------------------------------------------------------------------ geometry of a result
def corner_px(theta, wt, ht):
    """the four frame corners (x, y = +-1) in court pixels, fp64: (B,4,2)"""
    t = np.asarray(theta, dtype=np.float64).reshape(-1, 9)
    out = []
    with np.errstate(all="ignore"):
        for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
            Z = t[:, 6] * x + t[:, 7] * y + t[:, 8]
            u, v = (t[:, 0] * x + t[:, 1] * y + t[:, 2]) / Z, (t[:, 3] * x + t[:, 4] * y + t[:, 5]) / Z
            out.append(np.stack([(u + 1) * wt / 2 - 0.5, (v + 1) * ht / 2 - 0.5], axis=-1))
    return np.stack(out, axis=1)


def corner_error(theta, theta_true, wt, ht):
    """largest displacement of the four frame corners from theta_true, court pixels: (B,)"""
    d = corner_px(theta, wt, ht) - corner_px(theta_true, wt, ht)
    return np.sqrt((d ** 2).sum(axis=-1)).max(axis=1)


def theta_margin_px(theta, wt, ht, ulps=64):
    """the court-pixel size of `ulps` float32 ulps of every entry of theta (theta8 = 1): see the module docstring"""
    t = np.asarray(theta, dtype=np.float64).reshape(9)
    t = t / t[8]
    d = ulps * 2.0 ** -24 * np.abs(t)
    worst = 0.0
    for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        Wd = abs(t[6] * x + t[7] * y + 1.0)
        X, Y = abs(t[0] * x + t[1] * y + t[2]), abs(t[3] * x + t[4] * y + t[5])
        dW = d[6] + d[7]
        mx = ((d[0] + d[1] + d[2]) / Wd + X * dW / Wd ** 2) * wt / 2
        my = ((d[3] + d[4] + d[5]) / Wd + Y * dW / Wd ** 2) * ht / 2
        worst = max(worst, float(np.hypot(mx, my)))
    return worst
