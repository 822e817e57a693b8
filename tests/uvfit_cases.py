"""The cases of the UV homography fit's tests (tests/test_uvfit_host.py, tests/test_gpu_uvfit.py): court raster, thetas, uv
maps, logits, contamination - plain numpy, deterministic, no library."""
import json
import os

import numpy as np

import uvfit_ref as R

F32 = np.float32
WT, HT = 320, 180                       # the court raster the labels are rendered from
H, W = 72, 128                          # the whole-fit grid
GRIDS = [(2, 2), (18, 32), (65, 67), (72, 128), (72, 136)]

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=F32)
ZOOM = np.array([0.55, 0.02, 0.1, -0.015, 0.6, -0.05, 0, 0, 1], dtype=F32)
PERSPECTIVE = np.array([0.7, 0.05, 0.05, -0.03, 0.75, 0.02, 0.12, -0.18, 1], dtype=F32)
TRUE = {"identity": IDENTITY, "zoom": ZOOM, "perspective": PERSPECTIVE}


def u_tables(wt=WT, ht=HT):
    """preparation.uv_tables without offsets, restated: generate_uv_template's float32 linspace times 65535, rounded - and its
    window [0, n - 1), which leaves the last column and row 0"""
    out = []
    for n in (wt, ht):
        t = np.rint(np.linspace(1.0 / n, 1, num=n, dtype=F32).astype(np.float64) * 65535).astype(np.uint16)
        t[n - 1] = 0
        out.append(t)
    return tuple(out)


def court_point(theta, h, w, Hg, Wg):
    """the normalised court point of every pixel centre under theta, fp64: (cxn, cyn) (h,w)"""
    t = np.asarray(theta, dtype=np.float64).reshape(9)
    xs, ys = R.grid(Hg, Wg, h, w)
    x, y = np.meshgrid(xs, ys)
    with np.errstate(all="ignore"):
        Wd = t[6] * x + t[7] * y + t[8]
        return (t[0] * x + t[1] * y + t[2]) / Wd, (t[3] * x + t[4] * y + t[5]) / Wd


def exact_uv(theta, h, w, Hg=None, Wg=None, wt=WT, ht=HT):
    """uv (2,h,w) float32 computed in fp64 from theta and rounded; 0 where the pixel does not show the court"""
    cxn, cyn = court_point(theta, h, w, Hg or h, Wg or w)
    u, v = (cxn + (1 + 1.0 / wt)) / 2, (cyn + (1 + 1.0 / ht)) / 2
    with np.errstate(invalid="ignore"):
        ok = (u > 1.0 / wt) & (u <= 1) & (v > 1.0 / ht) & (v <= 1)
    return np.stack([np.where(ok, u, 0), np.where(ok, v, 0)]).astype(F32)


def label_uv(theta, h, w, Hg=None, Wg=None, wt=WT, ht=HT):
    """uv (2,h,w) float32 as a label holds it: the nearest court pixel of the tap rule px = (c + 1) wt / 2 - 0.5, its table value
    / 65535 (the rule of preparation.split_uv); 0 outside the court"""
    cxn, cyn = court_point(theta, h, w, Hg or h, Wg or w)
    ut, vt = u_tables(wt, ht)
    with np.errstate(invalid="ignore"):
        ix, iy = np.rint((cxn + 1) * wt / 2 - 0.5), np.rint((cyn + 1) * ht / 2 - 0.5)
        ok = (ix >= 0) & (ix < wt) & (iy >= 0) & (iy < ht)
    ix, iy = np.where(ok, ix, 0).astype(np.int64), np.where(ok, iy, 0).astype(np.int64)
    u = np.where(ok, ut[ix], 0) / 65535.0
    v = np.where(ok, vt[iy], 0) / 65535.0
    return np.stack([u, v]).astype(F32)


def contaminate(uv, share, seed):
    """`share` of the pixels replaced by uniform random (u, v)"""
    g = np.random.default_rng(seed)
    out = np.array(uv, dtype=F32, copy=True)
    hit = g.random(out.shape[-2:]) < share
    rnd = g.random(out.shape).astype(F32)
    out[..., hit] = rnd[..., hit]
    return out


def shifted(theta, px=9.0, wt=WT, ht=HT):
    """theta moved by `px` court pixels (a translation of 0.8 px, 0.6 px of it along the two axes): the corner error of the
    result against theta is px where the last row is (0, 0, 1)"""
    t = np.array(theta, dtype=np.float64)
    t[2] += 0.8 * px * 2 / wt
    t[5] += 0.6 * px * 2 / ht
    return t.astype(F32)


def logits(nc, uv, seed):
    """(nc,h,w) float32: class 0 where uv is 0 and on every seventh column, else 1 + (i + j) % (nc - 1), by a margin of 4 over
    N(0, 1) noise; plus three kinds of special pixels on row 1: a tie between classes 0 and 1 (the first wins: background), a
    NaN at class 0 (stays the answer: background), a NaN at class 2 (skipped)"""
    g = np.random.default_rng(seed)
    h, w = uv.shape[-2:]
    i, j = np.mgrid[0:h, 0:w]
    cls = np.where((uv[0] == 0) | (j % 7 == 0), 0, 1 + (i + j) % (nc - 1))
    lg = g.normal(0, 1, (nc, h, w)).astype(F32)
    lg[cls, i, j] += F32(4.0)
    if h > 1 and w >= 6:
        lg[:, 1, 1] = F32(-1.0)
        lg[0, 1, 1] = lg[1, 1, 1] = F32(2.5)
        lg[0, 1, 3] = np.nan
        lg[2 % nc, 1, 5] = np.nan
    return lg


def horizon_theta(h, Hg, row):
    """Wd = 0 exactly on row `row` of an h-row grid: theta7 = 1, theta8 = -y[row]"""
    _, ys = R.grid(Hg, 8, h, 8)
    t = ZOOM.copy()
    t[6], t[7], t[8] = 0.0, 1.0, -F32(ys[row])
    return t


def kernel_thetas(h, Hg):
    """the theta cases of the accumulate test: (names, (5,9) float32); `none` is the caller's"""
    scaled = (PERSPECTIVE.astype(np.float64) * 1.7).astype(F32)          # the STN's theta8 is not 1
    return (("identity", "zoom", "perspective-x1.7", "horizon", "nan"),
            np.stack([IDENTITY, ZOOM, scaled, horizon_theta(h, Hg, h // 2), np.full(9, np.nan, dtype=F32)]))


ACC_PARAMS = [(g, B, nc, twice) for g in GRIDS for B in (1, 3) for nc in (None, 4, 7) for twice in (False, True)]


def acc_id(p):
    (h, w), B, nc, twice = p
    return f"{h}x{w}-b{B}-{'nologits' if nc is None else 'nc%d' % nc}-{'grid2x' if twice else 'grid1x'}"


def accumulate_case(p):
    """the inputs of one accumulate case: uv (B,2,h,w) - frame 0 rendered from ZOOM (two pixels of row 0 moved onto the gate's
    thresholds), frame 1 all zero, frame 2 rendered from
    PERSPECTIVE with NaN in every 11th u and every 13th v -, logits (B,nc,h,w) or None, the grid theta addresses, and the
    theta cases"""
    (h, w), B, nc, twice = p
    Hg, Wg = (2 * h, 2 * w) if twice else (h, w)
    frames = [label_uv(ZOOM, h, w, Hg, Wg)]
    if w >= 6:                          # exactly on the gate's thresholds: u > u_min and v > v_min are strict, both fail
        u_min, v_min, _, _ = R.constants(WT, HT)
        frames[0][0, 0, 2], frames[0][1, 0, 4] = u_min, v_min
    if B == 3:
        holes = label_uv(PERSPECTIVE, h, w, Hg, Wg)
        flat = holes.reshape(2, -1)
        flat[0, ::11] = np.nan
        flat[1, ::13] = np.nan
        frames += [np.zeros((2, h, w), dtype=F32), holes]
    uv = np.stack(frames)
    lg = None if nc is None else np.stack([logits(nc, uv[b], 100 + b) for b in range(B)])
    names, thetas = kernel_thetas(h, Hg)
    return {"uv": uv, "logits": lg, "H": Hg, "W": Wg, "names": ("none",) + names,
            "thetas": [None] + [np.repeat(t[None], B, axis=0) for t in thetas]}


def whole_cases():
    """the whole-fit cases at 72 x 128: (name, true theta, uv kind, contamination share, with theta0)"""
    out = [(f"{kind}-{name}", name, kind, 0.0, False) for kind in ("exact", "label") for name in TRUE]
    out += [(f"label-{name}-{int(100 * share)}pct-{'theta0' if t0 else 'cold'}", name, "label", share, t0)
            for name in ("identity", "zoom") for share in (0.1, 0.3) for t0 in (False, True)]
    return out


def whole_inputs(case):
    """-> uv (1,2,H,W), theta0 (1,9) or None, the true theta"""
    _, name, kind, share, t0 = case
    true = TRUE[name]
    uv = (exact_uv if kind == "exact" else label_uv)(true, H, W)
    if share:
        uv = contaminate(uv, share, 5)
    return uv[None], (shifted(true)[None] if t0 else None), true


# ------------------------------------------------------------------------------------------------ the parity file
def record(path, rows):
    """merge `rows` (dicts with "test" and "case") into the jsonl file at `path`, one row per (test, case), sorted"""
    have = {}
    try:
        with open(path) as f:
            for line in f:
                r = json.loads(line)
                have[(r["test"], r["case"])] = r
    except (OSError, ValueError):
        pass
    for r in rows:
        have[(r["test"], r["case"])] = r
        print(json.dumps(r))
    try:
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            for key in sorted(have):
                f.write(json.dumps(have[key]) + "\n")
        os.replace(tmp, path)
    except OSError:          # a read-only checkout: the figures are still printed
        pass
