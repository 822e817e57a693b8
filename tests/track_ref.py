"""numpy restatement (test infrastructure only) of the inter-frame tracking rule stated in include/sfh_amd.h above the
sfh_track_* entries.  Nothing here imports the library.

Staging, as on the device and as tests/refine_ref.py: the coordinates, the bilinear weights, the bilinear value and the two tap
differences are float32, one rounding per operation (the fused multiply-adds of the rule are formed as the fp64 expression
rounded once: the product of two float32 is exact in fp64); everything behind them is float64, written in the kernel's
operation order.  The step runs on Python floats (IEEE double, no contraction); candidates are rounded to float32.

BOUNDS.  None is fitted to a kernel's output.

planes.  Exact: an integer sum below 2^24 and one IEEE division.  The device must give the same bits.

sums_bound(A, n).  Device and restatement share every operation of a per-pixel term, the float64 ones included (the header
  fixes their order: q, c, ic, rho, omega, J_k, (omega J_i) J_j), so a term is the SAME number on both sides; what differs is
  the order in which the n terms of a pair are added: (n - 1) additions of 2^-53 on partial sums of at most A = sum |term|, each
  side.  |got - ref| <= (2 n + 32) 2^-53 A - the refinement's bound, whose 32 is kept although no term differs here - times
  K2 = 1.01 for the second order.  A == 0 demands exact +0.0.  n itself is a sum of ones below 2^53: exact.

align_margin(err_ref, M_true, W, H).  A whole alignment on the device follows the restatement's trajectory as long as every accept /
  reject decision agrees; the sums differ within sums_bound, i.e. ~1e-12 relative, which the solve amplifies by the condition
  of the damped system and the float32 rounding of the candidate then mostly swallows.  Where a candidate lands on the other
  side of a float32 boundary the trajectories part by one ulp of M and rejoin at the same minimum to within the
  minimiser's own resolution.  The uvfit section's margin is used unchanged: device end error <= 1.25 x the restatement's + 64
  float32 ulps of M expressed in full-resolution pixels (uvfit_ref.theta_margin_px of M* on the raster (W-1) x (H-1), whose
  derivation stands in that module).  The comparison is honest only while the restatement itself converges: the host test
  asserts its end error < 0.1 px on every case.
"""
import math

import numpy as np

from chol8_ref import chol8_solve
from uvfit_ref import theta_margin_px
from refine_ref import F32, E53, K2, _fma32, axis as refine_axis, candidate, coords

SUMS, COST, N = 46, 44, 45
TILE = 64


def slabs(hl, wl):
    return -(-wl // TILE) * -(-hl // TILE)


# ------------------------------------------------------------------------------------------------ planes
def luma(frames, bgr=False):
    """frames (B,H,W,3) uint8 -> (B,H,W) int64: (19595 r + 38470 g + 7471 b + 32768) >> 16"""
    fr = np.asarray(frames).astype(np.int64)
    r, g, b = (fr[..., 2], fr[..., 1], fr[..., 0]) if bgr else (fr[..., 0], fr[..., 1], fr[..., 2])
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def planes(frames, f, bgr=False):
    """(B,H,W,3) uint8 -> (B,H/f,W/f) float32, exact"""
    y = luma(frames, bgr)
    B, H, W = y.shape
    S = y.reshape(B, H // f, f, W // f, f).sum(axis=(2, 4))
    return (S.astype(F32) / F32(255 * f * f)).astype(F32)


# ------------------------------------------------------------------------------------------------ coordinates
def track_axis(f, n):
    """(k, o) as float32: k = (n - 1) / (2 f), o = (f - 1) / (2 f), evaluated in fp64, rounded once"""
    return F32((n - 1) / (2.0 * f)), F32((f - 1) / (2.0 * f))


def grid(f, H, W):
    ax, cx = refine_axis(f, W, W)
    ay, cy = refine_axis(f, H, H)
    return _fma32(ax, np.arange(W // f, dtype=F32), cx), _fma32(ay, np.arange(H // f, dtype=F32), cy)


def pixel_terms(M, prev, cur, H, W, f, delta):
    """M (9,) float32, prev / cur (hl,wl) float32 planes of level f.  -> dict: counts (hl,wl) bool, r, rho, omega (hl,wl)
    float64, J (8,hl,wl) float64, px, py (hl,wl) float32; values where counts is False are meaningless"""
    prev, cur = np.asarray(prev, dtype=F32), np.asarray(cur, dtype=F32)
    hl, wl = cur.shape
    assert prev.shape == cur.shape == (H // f, W // f)
    xn, yn = grid(f, H, W)
    X, Y, Z, s, live, xb, yb = (a[0] for a in coords(np.asarray(M, dtype=F32).reshape(1, 9), xn, yn))
    kx, ox = track_axis(f, W)
    ky, oy = track_axis(f, H)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        px = _fma32(((s * X).astype(F32) + one).astype(F32), kx, -ox)
        py = _fma32(((s * Y).astype(F32) + one).astype(F32), ky, -oy)
        x0, y0 = np.floor(px), np.floor(py)
        counts = live & (x0 >= 0) & ((x0 + one).astype(F32) <= F32(wl - 1)) & (y0 >= 0) & ((y0 + one).astype(F32) <= F32(hl - 1))
        ix, iy = np.where(counts, x0, 0).astype(np.int64), np.where(counts, y0, 0).astype(np.int64)
        t00, t01, t10, t11 = prev[iy, ix], prev[iy, ix + 1], prev[iy + 1, ix], prev[iy + 1, ix + 1]
        wx1, wy1 = (px - x0).astype(F32), (py - y0).astype(F32)
        wx0, wy0 = (one - wx1).astype(F32), (one - wy1).astype(F32)
        val = (t00 * (wy0 * wx0).astype(F32)).astype(F32)
        for t, w in ((t01, (wy0 * wx1).astype(F32)), (t10, (wy1 * wx0).astype(F32)), (t11, (wy1 * wx1).astype(F32))):
            val = (val + (t * w).astype(F32)).astype(F32)
        duf = ((wy0 * (t01 - t00).astype(F32)).astype(F32) + (wy1 * (t11 - t10).astype(F32)).astype(F32)).astype(F32)
        dvf = ((wx0 * (t10 - t00).astype(F32)).astype(F32) + (wx1 * (t11 - t01).astype(F32)).astype(F32)).astype(F32)
        assert val.dtype == F32 and duf.dtype == F32 and dvf.dtype == F32 and px.dtype == F32
        r = val.astype(np.float64) - cur.astype(np.float64)
        du, dv = duf.astype(np.float64) * float(kx), dvf.astype(np.float64) * float(ky)
        d2 = float(delta) * float(delta)
        r2 = r * r
        c = 1.0 + r2 / d2
        ic = 1.0 / c
        rho, om = r2 * ic, ic * ic
        ds, dx, dy = s.astype(np.float64), xb.astype(np.float64), yb.astype(np.float64)
        gu, gv = -(X.astype(np.float64) * ds) * ds, -(Y.astype(np.float64) * ds) * ds
        a0, a1 = ds * dx, ds * dy
        J = np.stack([du * a0, du * a1, du * ds, dv * a0, dv * a1, dv * ds,
                      du * (gu * dx) + dv * (gv * dx), du * (gu * dy) + dv * (gv * dy)])
    return {"counts": counts, "r": r, "rho": rho, "omega": om, "J": J, "px": px, "py": py}


def sums(M, prev, cur, H, W, f, delta, want_A=True):
    """the 46 sums of one pair and A = the sums of the absolute terms: (S (46,), A (46,))"""
    q = pixel_terms(M, prev, cur, H, W, f, delta)
    k = q["counts"]
    S, A = np.zeros(SUMS), np.zeros(SUMS)
    if not k.any():
        return S, A
    J, r = q["J"][:, k], q["r"][k]
    om = q["omega"][k]
    e = 0
    for i in range(8):
        wj = om * J[i]
        for j in range(i, 8):
            t = wj * J[j]
            S[e] = t.sum()
            A[e] = np.abs(t).sum() if want_A else 0.0
            e += 1
        t = wj * r
        S[36 + i], A[36 + i] = t.sum(), (np.abs(t).sum() if want_A else 0.0)
    S[COST] = A[COST] = q["rho"][k].sum()
    S[N] = A[N] = float(k.sum())
    return S, A


def sums_bound(A, n):
    return K2 * (2 * n + 32) * E53 * np.asarray(A, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ step
def lm_solve(S, lam):
    S = [float(v) for v in S]
    L = [[0.0] * 8 for _ in range(8)]
    e = 0
    for i in range(8):
        for j in range(i, 8):
            L[j][i] = S[e] + lam * S[e] if i == j else S[e]
            e += 1
    g = [-S[36 + i] for i in range(8)]
    ok = chol8_solve(L, g, True)
    return g, ok


def _mean(S):
    with np.errstate(all="ignore"):
        return float(np.float64(S[COST]) / np.float64(S[N]))


class StepState:
    """the per-pair state of sfh_track_step, one pair, across the levels of a schedule"""

    def __init__(self):
        self.M = self.S = None
        self.lam, self.piv, self.dead, self.accepted = 1e-3, False, False, 0

    def step(self, S, M_eval, first, last, level, nmin):
        """-> (M_next (9,) float32, tie (9,) bool)"""
        S = np.asarray(S, dtype=np.float64)
        take = True
        if first:
            self.lam, self.accepted, self.mean_first = 1e-3, 0, _mean(S)
            self.dead = bool((level > 0 and self.dead) or not np.isfinite(S).all() or not S[N] >= nmin)
        else:
            take = bool(not self.dead and self.piv and S[N] >= nmin and _mean(S) < _mean(self.S))
            if not self.dead:
                self.lam = self.lam / 10.0 if take else self.lam * 10.0
            self.accepted += int(take)
        if take:
            self.M, self.S = np.asarray(M_eval, dtype=F32).reshape(9).copy(), S.copy()
        self.delta, self.piv = lm_solve(self.S, self.lam)
        if last or self.dead:
            return self.M.copy(), np.zeros(9, dtype=bool)
        return candidate(self.M, self.delta, self.piv)

    def stats(self):
        return self.mean_first, _mean(self.S), float(self.S[N])

    def ok(self, max_cost):
        m = _mean(self.S)
        return int(not self.dead and bool(np.isfinite(self.M).all()) and (not max_cost > 0.0 or m <= max_cost))


def nmin_of(min_overlap, hl, wl):
    return float(math.ceil(min_overlap * hl * wl))


def align(prev_u8, cur_u8, M0=None, factors=(8, 4, 2), iters=6, delta=0.06, min_overlap=0.25, max_cost=None, bgr=False):
    """the whole schedule for one pair of (H,W,3) uint8 frames -> dict M (9,) float32, stats (L,3), accepted (L,), ok"""
    H, W = cur_u8.shape[:2]
    cur = np.asarray(M0 if M0 is not None else np.eye(3), dtype=F32).reshape(9).copy()
    L = len(factors)
    out = {"stats": np.zeros((L, 3)), "accepted": np.zeros(L, dtype=np.int32)}
    st = StepState()
    for li, f in enumerate(factors):
        pp, pc = planes(prev_u8[None], f, bgr)[0], planes(cur_u8[None], f, bgr)[0]
        nmin = nmin_of(min_overlap, H // f, W // f)
        ev = lambda m: sums(m, pp, pc, H, W, f, delta, want_A=False)[0]
        cand, _ = st.step(ev(cur), cur, True, iters == 0, li, nmin)
        for it in range(iters):
            cand, _ = st.step(ev(cand), cand, False, it == iters - 1, li, nmin)
        cur = cand
        out["stats"][li] = st.stats()
        out["accepted"][li] = st.accepted
    out["M"], out["ok"] = cur, st.ok(max_cost if max_cost is not None else 0.0)
    return out


# ------------------------------------------------------------------------------------------------ propagate
def _adj(m):
    t = [float(v) for v in m]
    a = [t[4] * t[8] - t[5] * t[7], t[2] * t[7] - t[1] * t[8], t[1] * t[5] - t[2] * t[4],
         t[5] * t[6] - t[3] * t[8], t[0] * t[8] - t[2] * t[6], t[2] * t[3] - t[0] * t[5],
         t[3] * t[7] - t[4] * t[6], t[1] * t[6] - t[0] * t[7], t[0] * t[4] - t[1] * t[3]]
    return a, (t[0] * a[0] + t[1] * a[3]) + t[2] * a[6]


def _mul(P, m):
    return [(P[i * 3] * m[j] + P[i * 3 + 1] * m[3 + j]) + P[i * 3 + 2] * m[6 + j] for i in range(3) for j in range(3)]


def propagate(theta, M, link, score=None, max_score=0.0, max_gap=30):
    """theta, M (F,9) float32, link (F,) -> (theta_out (F,9) float32, source (F,) int32)"""
    theta = np.asarray(theta, dtype=F32).reshape(-1, 9)
    M = np.asarray(M, dtype=F32).reshape(-1, 9)
    F = theta.shape[0]
    link = np.asarray(link).reshape(F)

    def good(t):
        with np.errstate(all="ignore"):
            det = np.float64(_adj(np.asarray(theta[t], dtype=np.float64))[1])
        return bool(np.isfinite(det) and det != 0 and (score is None or F32(score[t]) <= F32(max_score)))

    out, src = theta.copy(), np.arange(F, dtype=np.int32)
    for t in range(F):
        if good(t):
            continue
        back = fwd = -1
        for d in range(1, max_gap + 1):
            k = t - d
            if k < 0 or link[k + 1] == 0:
                break
            if good(k):
                back = k
                break
        for d in range(1, max_gap + 1):
            k = t + d
            if k >= F or link[k] == 0:
                break
            if good(k):
                fwd = k
                break
        use_back = back >= 0 and (fwd < 0 or t - back <= fwd - t)
        k = back if use_back else fwd
        out[t], src[t] = np.nan, -1
        if k < 0:
            continue
        with np.errstate(all="ignore"):
            P = [np.float64(v) for v in theta[k]]
            if use_back:
                for j in range(k + 1, t + 1):
                    P = _mul(P, [np.float64(v) for v in M[j]])
            else:
                for j in range(k, t, -1):
                    P = _mul(P, [np.float64(v) for v in _adj([np.float64(v) for v in M[j]])[0]])
            if np.isfinite(P[8]) and P[8] != 0:
                out[t] = [F32(P[i] / P[8]) for i in range(8)] + [F32(1.0)]
                src[t] = k
    return out, src


# ------------------------------------------------------------------------------------------------ geometry of a result
def corner_px(M, W, H):
    """the four frame corners (xn, yn = +-1) under M in full-resolution pixels, fp64: (4,2)"""
    t = np.asarray(M, dtype=np.float64).reshape(9)
    out = []
    for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        Z = t[6] * x + t[7] * y + t[8]
        u, v = (t[0] * x + t[1] * y + t[2]) / Z, (t[3] * x + t[4] * y + t[5]) / Z
        out.append(((u + 1) * (W - 1) / 2, (v + 1) * (H - 1) / 2))
    return np.asarray(out)


def corner_error(M, M_true, W, H):
    """largest displacement of the four frame corners from M_true, full-resolution pixels"""
    with np.errstate(all="ignore"):
        d = corner_px(M, W, H) - corner_px(M_true, W, H)
        return float(np.sqrt((d ** 2).sum(axis=-1)).max())


def align_margin(err_ref, M_true, W, H):
    return 1.25 * err_ref + theta_margin_px(M_true, W - 1, H - 1)
