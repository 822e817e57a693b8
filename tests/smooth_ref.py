"""numpy restatement (test infrastructure only) of the temporal smoothing rule stated in include/sfh_amd.h above
sfh_track_smooth, operation for operation: csrc/smooth_core.h's functions by name, the kernel's lane layout, and butterfly(),
which reproduces wave_sum_all (csrc/common.h).  Everything is np.float64, one rounding per operation; the adjugate and the
product are track_ref's, the GOOD rule is sfh_track_propagate's.  Nothing here imports the library.

Every operation of the rule is stated and its order fixed, so the device is held to this file bit for bit: no bound."""
import numpy as np

from chol8_ref import chol8_solve
from track_ref import F32, _adj, _mul

F64 = np.float64
CTRL = np.array([[-1, 0.2], [1, 0.2], [1, 1], [-1, 1]], dtype=F32)
MAX_RADIUS = 31


def butterfly(v):
    """the xor butterfly 32 .. 1 over 64 lanes: every lane ends with the same bits; -> that sum"""
    v = np.asarray(v, dtype=F64).copy()
    assert v.shape == (64,)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ o]
    assert (v.view(np.uint64) == v.view(np.uint64)[0]).all() or np.isnan(v).all()
    return v[0]


def good(theta, score, max_score, t):
    with np.errstate(all="ignore"):
        det = F64(_adj(np.asarray(theta[t], dtype=F64))[1])
    return bool(np.isfinite(det) and det != 0 and (score is None or F32(score[t]) <= F32(max_score)))


def linked(theta, score, max_score, link, k, t):
    if k < 0 or k >= len(theta) or not good(theta, score, max_score, k):
        return False
    return all(link[j] != 0 for j in range(min(k, t) + 1, max(k, t) + 1))


def chain(theta, M, k, t):
    """theta_k seen from frame t: nine np.float64, not normalised"""
    with np.errstate(all="ignore"):
        P = [F64(v) for v in theta[k]]
        for j in range(k + 1, t + 1):
            P = _mul(P, [F64(v) for v in M[j]])
        for j in range(k, t, -1):
            P = _mul(P, [F64(v) for v in _adj([F64(v) for v in M[j]])[0]])
    return P


def project(P, ctrl=CTRL):
    """-> (member, q (8,) float64)"""
    q, pos, neg = np.zeros(8), 0, 0
    with np.errstate(all="ignore"):
        for c in range(4):
            x, y = F64(ctrl[c][0]), F64(ctrl[c][1])
            X = (P[0] * x + P[1] * y) + P[2]
            Y = (P[3] * x + P[4] * y) + P[5]
            W = (P[6] * x + P[7] * y) + P[8]
            q[2 * c], q[2 * c + 1] = X / W, Y / W
            pos, neg = pos + int(W > 0), neg + int(W < 0)
    return bool(np.isfinite(q).all() and (pos == 4 or neg == 4)), q


def triangle(R, dist):
    return F64(R + 1 - dist) / F64(R + 1)


def r2_of(q, c):
    s = F64(0.0)
    with np.errstate(all="ignore"):
        for i in range(8):
            e = F64(q[i]) - F64(c[i])
            s = s + e * e
    return s


def omega(r2, d2):
    with np.errstate(all="ignore"):
        ic = F64(1.0) / (F64(1.0) + F64(r2) / F64(d2))
        return ic * ic


def refit(c, ctrl=CTRL, ok=True):
    """-> (h: 8 floats, ok)"""
    A, b = [], []
    with np.errstate(all="ignore"):
        for p in range(4):
            x, y, u, v = float(F64(ctrl[p][0])), float(F64(ctrl[p][1])), float(c[2 * p]), float(c[2 * p + 1])
            A += [[x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y)], [0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y)]]
            b += [u, v]
        N, h = [[0.0] * 8 for _ in range(8)], [0.0] * 8
        for i in range(8):
            for j in range(i + 1):
                s = 0.0
                for r in range(8):
                    s += A[r][i] * A[r][j]
                N[i][j] = s
            s = 0.0
            for r in range(8):
                s += A[r][i] * b[r]
            h[i] = s
    ok = chol8_solve(N, h, ok)
    return h, ok


def smooth_frame(theta, M, link, t, score=None, max_score=0.0, back=12, ahead=12, iters=3, delta=0.05, min_members=1, ctrl=CTRL):
    """one frame, the kernel's lanes -> (theta_out (9,) float32, members, stats (3,) float64)"""
    d2 = F64(delta) * F64(delta)
    mem, q, g = np.zeros(64, dtype=bool), np.zeros((64, 8)), np.zeros(64)
    for lane in range(back + ahead + 1):
        k = t - back + lane
        if linked(theta, score, max_score, link, k, t):
            mem[lane], q[lane] = project(chain(theta, M, k, t), ctrl)
        g[lane] = triangle(back if k < t else ahead, abs(t - k))
    n = int(mem.sum())
    ref = -1
    for d in range(MAX_RADIUS + 1):
        if ref >= 0:
            break
        if d <= back and mem[back - d]:
            ref = back - d
        elif back + d < 64 and mem[back + d]:
            ref = back + d
    ref = max(ref, 0)
    c0 = q[ref].copy()
    with np.errstate(all="ignore"):
        dq = q - c0
        c = c0.copy()
        gw = np.zeros(64)
        for p in range(iters + 1):
            om = np.ones(64) if p == 0 else np.array([omega(r2_of(q[l], c), d2) for l in range(64)])
            gw = np.where(mem, g * om, 0.0)
            sw = butterfly(gw)
            c = np.array([c0[i] + butterfly(np.where(mem, gw * dq[:, i], 0.0)) / sw for i in range(8)])
        r2 = np.array([r2_of(q[l], c) for l in range(64)])
        srr = butterfly(np.where(mem, gw * r2, 0.0))
        own = np.sqrt(r2[back]) if mem[back] else F64(np.nan)
        ok = n >= min_members and bool(np.isfinite(c).all())
        h, ok = refit(c, ctrl, ok)
        if not ok:
            return np.full(9, np.nan, dtype=F32), n, np.full(3, np.nan)
        return np.array([F32(v) for v in h] + [F32(1.0)], dtype=F32), n, np.array([sw, np.sqrt(srr / sw), own])


def smooth(theta, M, link, score=None, max_score=0.0, back=12, ahead=12, iters=3, delta=0.05, min_members=1, ctrl=CTRL):
    """theta, M (F,9) float32, link (F,) -> (theta_out (F,9) float32, members (F,) int32, stats (F,3) float64)"""
    theta = np.asarray(theta, dtype=F32).reshape(-1, 9)
    M = np.asarray(M, dtype=F32).reshape(-1, 9)
    F = theta.shape[0]
    link = np.asarray(link).reshape(F)
    ctrl = np.asarray(ctrl, dtype=F32).reshape(4, 2)
    out, mem, stats = np.zeros((F, 9), dtype=F32), np.zeros(F, dtype=np.int32), np.zeros((F, 3))
    for t in range(F):
        out[t], mem[t], stats[t] = smooth_frame(theta, M, link, t, score, max_score, back, ahead, iters, delta, min_members, ctrl)
    return out, mem, stats


# ------------------------------------------------------------------------------------------------ exact inputs
# Where every member sees the same points the rule returns c = c0 exactly, but the refit is an fp64 solve, not an identity: its
# normal matrix has condition ~ 55 (A's is 7.4) and an entry is ~ 100 rounded operations away from its inputs, so h is within
# 55 * 100 * 2^-53 < 2^-40 of the true theta's entries (all O(1) here).  After fl32 a non-zero entry is then the true one or its
# neighbour (1 ulp), and an entry that is truly 0 comes back as a number below 2^-40: "ulps" mean nothing at 0.
EXACT_ULPS, EXACT_ZERO = 1, 2.0 ** -40


def exact_gap(out, true):
    """(largest distance in fp32 ulps over the entries where `true` is not 0, largest |out| over those where it is)"""
    out, true = np.ascontiguousarray(out, dtype=F32), np.ascontiguousarray(true, dtype=F32)
    assert np.isfinite(out).all()
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (out, true))
    ia, ib = (np.where(v < 0, -(v & 0x7FFFFFFF), v) for v in (ia, ib))
    nz = true != 0
    return int(np.abs(ia - ib)[nz].max()), float(np.abs(out[~nz]).max()) if (~nz).any() else 0.0


# ------------------------------------------------------------------------------------------------ the noisy clip
def corners(theta, ctrl=CTRL, scale=(640.0, 360.0)):
    """the control points under theta in court pixels of a raster `scale` wide and high: (4,2) fp64"""
    t = np.asarray(theta, dtype=F64).reshape(3, 3)
    p = np.concatenate([np.asarray(ctrl, dtype=F64), np.ones((4, 1))], axis=1) @ t.T
    with np.errstate(all="ignore"):
        return p[:, :2] / p[:, 2:] * (np.asarray(scale) / 2)


def corner_error(theta, true, **kw):
    """largest displacement of the four control points from `true`, court pixels"""
    with np.errstate(all="ignore"):
        d = corners(theta, **kw) - corners(true, **kw)
        e = np.sqrt((d ** 2).sum(axis=-1)).max()
    return float(e) if np.isfinite(e) else float("inf")


def noisy_clip(F=60, seed=7, theta_noise=0.004, m_noise=2e-4, garbage=17, gap=(30, 34), cut=45):
    """a pan / zoom clip with a known theta*_t = theta*_{t-1} M*_t: theta carries noise of theta_noise per entry, M of m_noise;
    frame `garbage` holds a usable but wrong theta (no score says so), frames gap[0] .. gap[1]-1 hold none (zeros), link[cut]
    is 0.  -> dict theta, M (F,9) float32, link (F,) int32, true (F,9) float64, good (F,) bool (frames with a noisy theta)"""
    rng = np.random.default_rng(seed)
    true = [np.array([[0.62, 0.05, 0.04], [-0.04, 0.58, -0.03], [0.05, -0.03, 1.0]])]
    Ms = [np.eye(3)]
    for t in range(1, F):
        s, a = 1.0 + 0.004 * np.sin(t / 7.0), 0.002 * np.cos(t / 9.0)
        m = np.array([[s, -a, 0.012 * np.cos(t / 11.0)], [a, s, 0.006 * np.sin(t / 5.0)], [0.001 * np.sin(t / 13.0), -0.0008, 1.0]])
        Ms.append(m)
        true.append(true[-1] @ m)
    true = np.stack([(m / m[2, 2]).reshape(9) for m in true])
    theta = (true + theta_noise * rng.standard_normal((F, 9))).astype(F32)
    theta[:, 8] = 1.0
    M = (np.stack([m.reshape(9) for m in Ms]) + m_noise * rng.standard_normal((F, 9))).astype(F32)
    M[:, 8] = 1.0
    M[0] = np.nan                                            # not read
    link = np.ones(F, dtype=np.int32)
    link[0], link[cut] = 0, 0
    isgood = np.ones(F, dtype=bool)
    theta[garbage] = [1.3, 0.4, -0.2, 0.3, 0.7, 0.5, 0.1, 0.2, 1.0]
    theta[gap[0]:gap[1]] = 0.0
    isgood[garbage] = False
    isgood[gap[0]:gap[1]] = False
    return {"theta": theta, "M": M, "link": link, "true": true, "good": isgood, "garbage": garbage, "gap": gap, "cut": cut}
