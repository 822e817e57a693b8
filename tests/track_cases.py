"""Case table of the tracking tests (tests/test_track_host.py, tests/test_gpu_track.py): the synthetic scenes of the recovery
table, the M kinds of the kernel tests and the clips of the propagation tests.  Plain numpy; nothing here imports the library.

Scenes.  An analytic texture - a sum of 24 sinusoids with a fixed seed, defined on the whole plane of normalised frame
coordinates - is sampled at M* x for the current frame and at x for the previous one, then quantised to uint8 (r = g = b, so
the luma is the value itself).  Both frames are exact samples of one continuous scene: there is no resampling bias, and M* is
the minimiser up to quantisation.  "Players": opaque random rectangles covering 20 % of the current frame only."""
import functools

import numpy as np

import track_ref as T

F32 = np.float32
H, W = 144, 256                            # frames of the whole-alignment cases
FACTORS, ITERS, DELTA, MIN_OVERLAP = (8, 4, 2), 6, 0.06, 0.25


def _waves(seed=5, n=24):
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.6, 7.0, n)                       # cycles over the frame's width
    ang = rng.uniform(0.0, np.pi, n)
    ph = rng.uniform(0.0, 2 * np.pi, n)
    amp = 1.0 / np.sqrt(k)
    return k * np.pi * np.cos(ang), k * np.pi * np.sin(ang) * (H / W), ph, amp / np.sqrt((amp ** 2).sum() / 2)


def texture(x, y):
    """the scene at normalised coordinates (any shape), fp64 in [0, 1]: mean 0.5, standard deviation 0.2, clipped (the clip is
    part of the scene: both frames sample it)"""
    wx, wy, ph, amp = _waves()
    v = np.zeros(np.broadcast(x, y).shape)
    for a, b, p, c in zip(wx, wy, ph, amp):
        v = v + c * np.sin(a * x + b * y + p)
    return np.clip(0.5 + 0.2 * v, 0.0, 1.0)


def frame(M=None, h=H, w=W):
    """(h,w,3) uint8: the scene sampled at M x over the full-resolution grid 2 j / (w-1) - 1"""
    x, y = np.meshgrid(2.0 * np.arange(w) / (w - 1) - 1.0, 2.0 * np.arange(h) / (h - 1) - 1.0)
    if M is not None:
        m = np.asarray(M, dtype=np.float64).reshape(9)
        Z = m[6] * x + m[7] * y + m[8]
        x, y = (m[0] * x + m[1] * y + m[2]) / Z, (m[3] * x + m[4] * y + m[5]) / Z
    g = np.clip(np.rint(texture(x, y) * 255.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def occlude(fr, seed, cover=0.2):
    """opaque random rectangles until `cover` of the frame is covered"""
    rng = np.random.default_rng(seed)
    out, mask = fr.copy(), np.zeros(fr.shape[:2], dtype=bool)
    h, w = mask.shape
    while mask.mean() < cover:
        rh, rw = int(rng.integers(h // 8, h // 3)), int(rng.integers(w // 16, w // 8))
        y0, x0 = int(rng.integers(0, h - rh)), int(rng.integers(0, w - rw))
        shade = int(rng.integers(0, 20)) if rng.integers(0, 2) else int(rng.integers(236, 256))
        out[y0:y0 + rh, x0:x0 + rw] = shade
        mask[y0:y0 + rh, x0:x0 + rw] = True
    return out


def pan(dx, dy, w=W, h=H):
    """M* of a translation by (dx, dy) full-resolution pixels"""
    return np.array([1, 0, 2.0 * dx / (w - 1), 0, 1, 2.0 * dy / (h - 1), 0, 0, 1], dtype=F32)


def zoom_rot(scale, deg):
    c, s = scale * np.cos(np.deg2rad(deg)), scale * np.sin(np.deg2rad(deg))
    a = (H - 1) / (W - 1)                                # a rotation of the pixel raster, in normalised coordinates
    return np.array([c, -s * a, 0.004, s / a, c, -0.003, 0, 0, 1], dtype=F32)


IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=F32)
ALIGN_CASES = {                                           # name -> M*; every alignment starts from the identity
    "identity": IDENTITY,
    "pan3": pan(3.0, 1.1),
    "pan6": pan(5.9, -2.3),        # not a whole-pixel pan: that would make the two frames the same samples
    "pan12": pan(12.0, 3.0),
    "zoomrot": zoom_rot(1.03, 1.4),
    "perspective": np.array([1.0, 0.004, 0.006, -0.003, 1.0, 0.004, 0.012, -0.009, 1.0], dtype=F32),
}
ALIGN_IDS = [f"{n}-{k}" for n in ALIGN_CASES for k in ("clean", "occluded")]


@functools.lru_cache(maxsize=None)
def align_pair(case):
    """'<name>-clean' | '<name>-occluded' -> (prev (H,W,3) uint8, cur (H,W,3) uint8, M* (9,) float32)"""
    name, kind = case.split("-")
    M = ALIGN_CASES[name]
    cur = frame(M)
    if kind == "occluded":
        cur = occlude(cur, seed=17 + list(ALIGN_CASES).index(name))
    return frame(), cur, M


@functools.lru_cache(maxsize=None)
def align_ref(case):
    """the restatement's whole alignment of a case, computed once and shared: track_ref.align's dict + err (px)"""
    prev, cur, M = align_pair(case)
    out = T.align(prev, cur, factors=FACTORS, iters=ITERS, delta=DELTA, min_overlap=MIN_OVERLAP)
    out["err"] = T.corner_error(out["M"], M, W, H)
    out["start"] = T.corner_error(IDENTITY, M, W, H)
    return out


# ------------------------------------------------------------------------------------------------ kernel tests
GRIDS = ((2, 2), (18, 32), (65, 67), (72, 128), (72, 136))        # plane sizes (hl, wl) of the accumulate test, level f = 1


def plane_frames(hl, wl, n=3, seed=3):
    """n random-textured uint8 frames of hl x wl (level 1: a plane pixel per frame pixel): smooth enough to have gradients"""
    rng = np.random.default_rng(seed + hl * 1000 + wl)
    out = []
    for k in range(n):
        fr = frame(pan(1.7 * k, -0.9 * k, wl, hl), hl, wl).astype(np.int64)
        fr = fr + rng.integers(-6, 7, fr.shape[:2])[..., None]
        out.append(np.clip(fr, 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.stack(out))


def kernel_Ms(yn, row):
    """the M kinds of the accumulate test, (7,9) float32: identity; pan; zoom; perspective; horizon (Z = 0 exactly on grid
    row `row`: m6 = 0, m8 = -fl32(m7 yn[row])); all-NaN; a shift that leaves n = 0"""
    m7 = F32(0.9)
    return np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1],
                     [1, 0, 0.031, 0, 1, -0.043, 0, 0, 1],
                     [0.93, 0, 0.01, 0, 0.91, -0.02, 0, 0, 1],
                     [0.97, 0.02, 0.01, -0.015, 1.02, 0.01, 0.04, -0.05, 1],
                     [0.8, 0.0, 0.1, 0.0, 0.7, 0.0, 0.0, m7, -F32(m7 * F32(yn[row]))],
                     [np.nan] * 9,
                     [1, 0, 50.0, 0, 1, 50.0, 0, 0, 1]], dtype=F32)


KERNEL_M_IDS = ("identity", "pan", "zoom", "perspective", "horizon", "nan", "outside")


# ------------------------------------------------------------------------------------------------ propagation
def dyadic_clip(F=8):
    """theta_t = theta_0 M_1 .. M_t with dyadic translations: every product is exact, so the rule can be checked bit for bit.
    -> (theta (F,9), M (F,9)) float32; M[0] is garbage (it is not read)"""
    M = np.tile(IDENTITY, (F, 1))
    M[:, 2] = [np.nan] + [2.0 ** -k for k in range(3, 3 + F - 1)]
    M[:, 5] = [np.nan] + [-(2.0 ** -k) for k in range(4, 4 + F - 1)]
    theta = np.zeros((F, 9), dtype=F32)
    theta[0] = [0.5, 0, 0.25, 0, 0.5, -0.125, 0, 0, 1]
    for t in range(1, F):
        theta[t] = np.asarray(T._mul([float(v) for v in theta[t - 1]], [float(v) for v in M[t]]), dtype=F32)
    return theta, M
