"""Case table of the coarse-shift-search tests (tests/test_search_host.py, tests/test_gpu_search.py): the fast pans of the
whole-alignment comparison and the plane sets of the kernel comparison, each with the restatement's result computed once and
shared.  Plain numpy; nothing here imports the library."""
import functools

import numpy as np

import search_ref as S
import track_cases as K
import track_ref as T

F32 = np.float32
RADIUS = (8, 4)                      # plane pixels of factors[0] = 8 on the 256 x 144 frames: a reach of 64 x 32 frame pixels
OCCLUDE_SEED = 23


def _compose(a, b):
    m = np.asarray(a, dtype=np.float64).reshape(3, 3) @ np.asarray(b, dtype=np.float64).reshape(3, 3)
    return (m / m[2, 2]).reshape(9).astype(F32)


PAN_CASES = {                                             # name -> M*: pans the plain alignment does not reach
    "pan31": K.pan(31.3, -6.4),
    "pan47": K.pan(47.2, 9.7),
    "pan60": K.pan(-60.6, -20.3),
}
COMPOSED = "zoompan47"
WIDE_CASES = {**PAN_CASES, COMPOSED: _compose(K.zoom_rot(1.03, 1.4), K.pan(47.2, 9.7))}
PAN_IDS = [f"{n}-{k}" for n in PAN_CASES for k in ("clean", "occluded")]
WIDE_IDS = [f"{n}-{k}" for n in WIDE_CASES for k in ("clean", "occluded")]


@functools.lru_cache(maxsize=None)
def wide_pair(case):
    """'<name>-clean' | '<name>-occluded' -> (prev (H,W,3) uint8, cur (H,W,3) uint8, M* (9,) float32)"""
    name, kind = case.split("-")
    M = WIDE_CASES[name]
    cur = K.frame(M)
    if kind == "occluded":
        cur = K.occlude(cur, seed=OCCLUDE_SEED)
    return K.frame(), cur, M


def pair_of(case):
    return K.align_pair(case) if case in K.ALIGN_IDS else wide_pair(case)


@functools.lru_cache(maxsize=None)
def searched_ref(case):
    """the restatement's searched alignment of a case of K.ALIGN_IDS or WIDE_IDS, computed once and shared:
    search_ref.searched_align's dict + err, start (px) and start_searched (px): the corner error of the search's m0"""
    prev, cur, M = pair_of(case)
    out = S.searched_align(prev, cur, RADIUS, factors=K.FACTORS, iters=K.ITERS, delta=K.DELTA, min_overlap=K.MIN_OVERLAP)
    out["err"] = T.corner_error(out["M"], M, K.W, K.H)
    out["start"] = T.corner_error(K.IDENTITY, M, K.W, K.H)
    out["start_searched"] = T.corner_error(out["m0"], M, K.W, K.H)
    return out


@functools.lru_cache(maxsize=None)
def plain_ref(case):
    """the restatement's alignment of a wide case from the identity: what the search is for"""
    prev, cur, M = wide_pair(case)
    out = T.align(prev, cur, factors=K.FACTORS, iters=K.ITERS, delta=K.DELTA, min_overlap=K.MIN_OVERLAP)
    out["err"] = T.corner_error(out["M"], M, K.W, K.H)
    return out


# ------------------------------------------------------------------------------------------------ kernel tests
def _random(rng, n, hl, wl):
    """planes as sfh_track_planes writes them at f = 1: k / 255, a smooth ramp under the noise so that shifts differ"""
    y, x = np.mgrid[0:hl, 0:wl]
    base = 96 + 60 * np.sin(0.9 * x + 0.3) * np.cos(0.7 * y) + 1.5 * x - 0.8 * y
    k = np.clip(np.rint(base[None] + rng.integers(-40, 41, (n, hl, wl))), 0, 255)
    return (k.astype(F32) / F32(255)).astype(F32)


def _dyadic(rng, hl, wl, sx, sy):
    """two planes of multiples of 1/256 with prev[I + sy][J + sx] == cur[I][J] wherever both exist: the mean cost at (sx, sy)
    is exactly +0.0, and no other shift repeats the pattern"""
    cur = (rng.integers(0, 256, (hl, wl)).astype(F32) / F32(256)).astype(F32)
    prev = (rng.integers(0, 256, (hl, wl)).astype(F32) / F32(256)).astype(F32)
    i0, i1, j0, j1 = max(0, -sy), min(hl, hl - sy), max(0, -sx), min(wl, wl - sx)
    prev[i0 + sy:i1 + sy, j0 + sx:j1 + sx] = cur[i0:i1, j0:j1]
    return np.stack([prev, cur, prev])


# (hl, wl), (rx, ry), f: the raw entry sees frames of H = hl f, W = wl f
GEOMETRIES = {"2x2-r1": ((2, 2), (1, 1), 1), "2x2-r3": ((2, 2), (3, 3), 1), "7x9": ((7, 9), (2, 3), 1), "18x32": ((18, 32), (8, 4), 8),
              "65x67": ((65, 67), (2, 2), 1), "7x9-r0": ((7, 9), (0, 0), 2)}
PAIRS_1 = ((0,), (1,))
PAIRS_3 = ((0, 0, 1), (1, 1, 0))                  # a repeated pair and the reversed one
PAIRS_BAD = ((2, 0, 1), (0, 3, -1))               # with three frames: the indices 3 and -1 are outside
CONTENTS = ("random", "flat", "dyadic", "nan", "nmin")


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """'<geometry>/<contents>/<pairs>' -> dict: planes (3,hl,wl) float32, ia, ib, H, W, f, rx, ry, delta, nmin, contents"""
    geo, contents, pairs = name.split("/")
    (hl, wl), (rx, ry), f = (45, 80), (16, 8), 8
    if geo != "45x80":
        (hl, wl), (rx, ry), f = GEOMETRIES[geo]
    rng = np.random.default_rng(sum(ord(ch) for ch in geo + contents))
    nmin = 1.0 if geo.startswith("2x2") else S.nmin_of(K.MIN_OVERLAP, hl, wl)
    if contents == "flat":
        planes = np.full((3, hl, wl), F32(0.375), dtype=F32)
    elif contents == "dyadic":
        planes = _dyadic(rng, hl, wl, min(rx, 1, wl - 1), -min(ry, 2, hl - 1))
    else:
        planes = _random(rng, 3, hl, wl)
    if contents == "nan":
        planes[0, 0, 0] = np.nan              # frame 0 is the previous one of the pair (0, 1): the shifts with dx <= 0 and dy <= 0 count it
    if contents == "nmin":
        nmin = float(hl * wl + 1)
    ia, ib = {"p1": PAIRS_1, "p3": PAIRS_3, "bad": PAIRS_BAD}[pairs]
    return dict(planes=planes, ia=np.array(ia, dtype=np.int32), ib=np.array(ib, dtype=np.int32), H=hl * f, W=wl * f, f=f, rx=rx, ry=ry,
                delta=K.DELTA, nmin=nmin, contents=contents, hl=hl, wl=wl)


KERNEL_IDS = ([f"{g}/{c}/{p}" for g in GEOMETRIES for c, p in (("random", "p1"), ("random", "p3"), ("flat", "p1"), ("dyadic", "p3"))]
              + ["7x9/nan/p3", "18x32/nan/p1", "7x9/nmin/p1", "18x32/random/bad", "65x67/random/bad", "45x80/random/p1"])


@functools.lru_cache(maxsize=None)
def kernel_ref(name):
    """search_ref.search of a kernel case, computed once and shared: (table, shift, found, m0, sstats, runner_up)"""
    c = kernel_case(name)
    return S.search(c["planes"], c["ia"], c["ib"], c["H"], c["W"], c["f"], c["rx"], c["ry"], c["delta"], c["nmin"])
