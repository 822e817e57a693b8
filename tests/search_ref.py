"""numpy restatement (test infrastructure only) of the coarse shift search stated in include/sfh_amd.h above
sfh_track_search, operation for operation: csrc/search_core.h's functions by name, the cost kernel's lane layout, and
smooth_ref.butterfly for wave_sum_all (csrc/common.h).  Everything behind the fp32 planes is np.float64, one rounding per
operation.  Nothing here imports the library.

Every operation of the rule is stated and its order fixed, so the device is held to this file bit for bit: no bound.  The
lane sums add +0.0 where a pixel is not counted: rho is never negative, so a sum that starts at +0.0 keeps its bits."""
import math

import numpy as np

import track_ref as T
from smooth_ref import butterfly

F32, F64 = np.float32, np.float64
MAX_RADIUS = 32


def candidates(rx, ry):
    return (2 * rx + 1) * (2 * ry + 1)


def index(dx, dy, rx, ry):
    return (dy + ry) * (2 * rx + 1) + (dx + rx)


def candidate(c, rx, ry):
    """-> (dx, dy)"""
    w = 2 * rx + 1
    return c % w - rx, c // w - ry


def count(hl, wl, dx, dy):
    return float(max(0, hl - abs(dy)) * max(0, wl - abs(dx)))


def rho(prev, cur, d2):
    """float32 arrays -> float64"""
    with np.errstate(all="ignore"):
        r = np.asarray(prev, dtype=F32).astype(F64) - np.asarray(cur, dtype=F32).astype(F64)
        r2 = r * r
        c = 1.0 + r2 / F64(d2)
        ic = 1.0 / c
        return r2 * ic


def mean_of(prev, cur, dx, dy, d2):
    """the mean cost of one candidate on two (hl, wl) float32 planes, in the kernel's summation order"""
    hl, wl = cur.shape
    chunks = -(-wl // 64)
    full = np.zeros((hl, chunks * 64))                        # +0.0 where a pixel is not counted
    i0, i1 = max(0, -dy), min(hl, hl - dy)
    j0, j1 = max(0, -dx), min(wl, wl - dx)
    if i1 > i0 and j1 > j0:
        full[i0:i1, j0:j1] = rho(prev[i0 + dy:i1 + dy, j0 + dx:j1 + dx], cur[i0:i1, j0:j1], d2)
    acc = np.zeros(64)
    with np.errstate(all="ignore"):
        for I in range(hl):
            for k in range(chunks):
                acc = acc + full[I, k * 64:(k + 1) * 64]      # lane l: J = l + 64 k
        return F64(butterfly(acc)) / F64(count(hl, wl, dx, dy))


def table(planes, ia, ib, rx, ry, delta):
    """planes (nframes, hl, wl) float32 -> the table of means (P, candidates) float64"""
    planes = np.asarray(planes, dtype=F32)
    d2 = F64(delta) * F64(delta)
    out = np.full((len(ia), candidates(rx, ry)), np.nan)
    for p, (a, b) in enumerate(zip(ia, ib)):
        if not (0 <= a < len(planes) and 0 <= b < len(planes)):
            continue
        for c in range(out.shape[1]):
            dx, dy = candidate(c, rx, ry)
            out[p, c] = mean_of(planes[a], planes[b], dx, dy, d2)
    return out


def key(mean, n, nmin, dx, dy):
    """search_key: (ok, mean, dx, dy)"""
    return (bool(n >= nmin and np.isfinite(mean)), float(mean), dx, dy)


def before(a, b):
    """search_before"""
    if not a[0] or not b[0]:
        return a[0] and not b[0]
    if a[1] != b[1]:
        return a[1] < b[1]
    da, db = a[2] * a[2] + a[3] * a[3], b[2] * b[2] + b[3] * b[3]
    if da != db:
        return da < db
    if a[3] != b[3]:
        return a[3] < b[3]
    return a[2] < b[2]


def offset(d, f, n):
    return F32(F64(d * 2 * f) / F64(n - 1))


def m0_of(f, W, H, dx, dy):
    return np.array([1, 0, offset(dx, f, W), 0, 1, offset(dy, f, H), 0, 0, 1], dtype=F32)


def choose(row, hl, wl, rx, ry, nmin, f, W, H):
    """one pair's row of the table -> dict shift (2,) int32, found, m0 (9,) float32, sstats (3,) float64, runner_up: the
    second smallest admissible mean (NaN if there is none) - for the argmin condition of the tests"""
    best, means = (False, 0.0, 0, 0), []
    for c in range(candidates(rx, ry)):
        dx, dy = candidate(c, rx, ry)
        k = key(row[c], count(hl, wl, dx, dy), nmin, dx, dy)
        if k[0]:
            means.append(k[1])
        if before(k, best):
            best = k
    zero = key(row[index(0, 0, rx, ry)], count(hl, wl, 0, 0), nmin, 0, 0)
    dx, dy = (best[2], best[3]) if best[0] else (0, 0)
    means.sort()
    return {"shift": np.array([dx, dy], dtype=np.int32), "found": int(best[0]), "m0": m0_of(f, W, H, dx, dy),
            "sstats": np.array([best[1] if best[0] else np.nan, zero[1] if (best[0] and zero[0]) else np.nan,
                                count(hl, wl, dx, dy) if best[0] else 0.0]),
            "runner_up": means[1] if len(means) > 1 else float("nan")}


def search(planes, ia, ib, H, W, f, rx, ry, delta, nmin):
    """sfh_track_search -> (table (P,C), shift (P,2) int32, found (P,) int32, m0 (P,9) float32, sstats (P,3), runner_up (P,))"""
    hl, wl = H // f, W // f
    tab = table(planes, ia, ib, rx, ry, delta)
    rows = [choose(tab[p], hl, wl, rx, ry, nmin, f, W, H) for p in range(len(ia))]
    return (tab, np.stack([r["shift"] for r in rows]), np.array([r["found"] for r in rows], dtype=np.int32),
            np.stack([r["m0"] for r in rows]), np.stack([r["sstats"] for r in rows]), np.array([r["runner_up"] for r in rows]))


def margin(best, runner_up):
    """the relative gap between the best and the second smallest admissible mean (inf where there is no second)"""
    if not np.isfinite(runner_up):
        return float("inf")
    return float(abs(runner_up - best) / max(abs(runner_up), abs(best))) if runner_up != best else 0.0


def searched_align(prev_u8, cur_u8, radius, factors=(8, 4, 2), iters=6, delta=0.06, min_overlap=0.25, bgr=False):
    """FrameAligner(search=radius) on one pair of (H,W,3) uint8 frames: the search on the planes of factors[0], then
    track_ref.align from its m0 -> align's dict + shift, found, sstats, runner_up, m0"""
    H, W = cur_u8.shape[:2]
    f = factors[0]
    pl = T.planes(np.stack([prev_u8, cur_u8]), f, bgr)
    nmin = T.nmin_of(min_overlap, H // f, W // f)
    tab, shift, found, m0, sstats, ru = search(pl, [0], [1], H, W, f, radius[0], radius[1], delta, nmin)
    out = T.align(prev_u8, cur_u8, M0=m0[0], factors=factors, iters=iters, delta=delta, min_overlap=min_overlap, bgr=bgr)
    out.update(shift=shift[0], found=int(found[0]), sstats=sstats[0], runner_up=float(ru[0]), m0=m0[0])
    return out


def nmin_of(min_overlap, hl, wl):
    return float(math.ceil(min_overlap * hl * wl))
