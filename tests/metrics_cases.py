"""Case tables of the registration-metric tests (tests/test_metrics_host.py, tests/test_gpu_metrics.py): inputs as numpy
arrays, made from fixed seeds; counts that can be derived by hand are carried as ``expect`` beside the inputs, so that the
restatement (tests/metrics_ref.py) is not its own judge."""
import zlib

import numpy as np

F32 = np.float32
IGNORE = -100

# H x W: one pixel; odd sizes (the scalar path); more than one workgroup turn; a tail behind a full tile with H W % 4 == 0
# (the 16-byte path); one full frame
SHAPES = [(1, 1), (5, 7), (23, 41), (65, 64), (360, 640)]
BATCHES = (1, 3)
CLASSES = (2, 4, 7, 8)
KINDS = (0, 1, 2, 3)
SPECIAL_SHAPES = [(23, 41), (65, 64)]


def rng(name):
    return np.random.default_rng(zlib.crc32(str(name).encode()))


def batches_of(shape):
    return (1,) if shape == (360, 640) else BATCHES


# ------------------------------------------------------------------------------------------------ confusion
def warp_values(ids, nc):
    """class ids -> the warp mask's fp32 values k / nc"""
    return (ids.astype(F32) / F32(nc)).astype(F32)


def pred_of_ids(ids, kind, nc, r):
    """a prediction of ``kind`` whose class is ``ids`` everywhere: ids themselves, logits with a clear maximum, or k / nc"""
    if kind == 0:
        return ids.astype(np.int32)
    if kind == 1:
        return ids.astype(np.uint8)
    if kind == 3:
        return warp_values(ids, nc)
    B, H, W = ids.shape
    L = r.standard_normal((B, nc, H, W)).astype(F32)
    np.put_along_axis(L, ids[:, None], L.max(axis=1, keepdims=True) + F32(1), axis=1)
    return L


def random_case(shape, B, nc, kind):
    r = rng(("conf", shape, B, nc, kind))
    H, W = shape
    gt = r.integers(0, nc, (B, H, W)).astype(np.int64)
    gt[r.random((B, H, W)) < 0.1] = IGNORE
    if kind == 2:
        pred = (r.standard_normal((B, nc, H, W)) * 3).astype(F32)          # the class is the argmax rule's
    else:
        pred = pred_of_ids(r.integers(0, nc, (B, H, W)), kind, nc, r)
    return pred, gt


def rounds_up_value():
    """(v, k, nc): a warp value v < k / nc (as real numbers) whose fp32 product v * nc rounds UP to the integer k: trunc gives k,
    a product in higher precision would give k - 1.  Among nc = 2 .. 8 only 5/6 has such a neighbour (0.8333333)."""
    for nc in range(2, 9):
        for k in range(1, nc):
            v = np.nextafter(F32(k) / F32(nc), F32(2))
            for _ in range(6):
                if float(v) * nc < k and F32(v * F32(nc)) == F32(k):
                    return v, k, nc
                v = np.nextafter(v, F32(0))
    raise AssertionError("no such value")


def special_cases(shape):
    """name -> (pred, kind, nc, gt, flag expected); each a case of its own"""
    H, W = shape
    out = {}
    n = H * W
    for nc in (4, 8):
        r = rng(("special", shape, nc))
        ids = r.integers(0, nc, (2, H, W))
        gt = r.integers(0, nc, (2, H, W)).astype(np.int64)
        out[f"all-ignored-nc{nc}"] = (pred_of_ids(ids, 2, nc, r), 2, nc, np.full((2, H, W), IGNORE, dtype=np.int64), 0)
        scattered = gt.copy()
        scattered[r.random(gt.shape) < 0.3] = IGNORE
        out[f"scattered-ignored-nc{nc}"] = (pred_of_ids(ids, 0, nc, r), 0, nc, scattered, 0)
        one = np.full((2, H, W), 1, dtype=np.int64)          # every pixel on one key: the worst case for contention
        for kind in KINDS:
            out[f"single-class-nc{nc}-kind{kind}"] = (pred_of_ids(one, kind, nc, r), kind, nc, one.copy(), 0)
        # pixel i holds key i % nc^2: every wave sees every key, the worst case for the distinct-key loop
        key = (np.arange(2 * n) % (nc * nc)).reshape(2, H, W)
        for kind in (1, 2):
            out[f"checkerboard-nc{nc}-kind{kind}"] = (pred_of_ids(key % nc, kind, nc, r), kind, nc, (key // nc).astype(np.int64), 0)
        # integer-valued logits: exact two-way ties (first index wins) and all-way ties (class 0)
        L = r.integers(-2, 3, (2, nc, H, W)).astype(F32)
        L[:, :, ::3] = F32(1)
        out[f"ties-nc{nc}"] = (L, 2, nc, gt, 0)
    nc = 4
    r = rng(("special4", shape))
    gt = r.integers(0, nc, (1, H, W)).astype(np.int64)
    L = r.standard_normal((1, nc, H, W)).astype(F32)
    rows = np.array([[1, np.nan, 3, .5], [1, 2, np.inf, 0], [np.nan, 5, 6, 7], [-np.inf, -np.inf, -np.inf, -np.inf]], dtype=F32)
    flat = L.reshape(nc, n)
    for i in range(n):
        if i % 5 < 4:
            flat[:, i] = rows[i % 5]
    out["nonfinite-logits"] = (L, 2, nc, gt, 0)
    v, k, ncu = rounds_up_value()
    gu = r.integers(0, ncu, (1, H, W)).astype(np.int64)
    w = warp_values(r.integers(0, ncu, (1, H, W)), ncu)
    w.reshape(-1)[::2] = v
    out["warp-rounds-up"] = (w, 3, ncu, gu, 0)
    ids = r.integers(0, nc, (1, H, W))
    bad_gt = gt.copy()
    bad_gt.reshape(-1)[0] = nc
    bad_gt.reshape(-1)[-1] = -1
    out["flag-1"] = (pred_of_ids(ids, 0, nc, r), 0, nc, bad_gt, 1)
    bad_ids = ids.astype(np.int32)
    bad_ids.reshape(-1)[n // 2] = nc
    out["flag-2-int32"] = (bad_ids, 0, nc, gt, 2)
    bad_u8 = ids.astype(np.uint8)
    bad_u8.reshape(-1)[n // 2] = 200
    out["flag-2-uint8"] = (bad_u8, 1, nc, gt, 2)
    bad_w = warp_values(ids, nc)
    bad_w.reshape(-1)[n // 2] = np.nan
    bad_w.reshape(-1)[0] = F32(1.0)                          # class nc
    out["flag-2-warp"] = (bad_w, 3, nc, gt, 2)
    out["flag-3"] = (bad_w, 3, nc, bad_gt, 3)
    return out


SPECIAL_NAMES = sorted(special_cases((2, 2)))


# ------------------------------------------------------------------------------------------------ region
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=F32)
HALF = np.array([.5, 0, 0, 0, .5, 0, 0, 0, 1], dtype=F32)
# entries with a few bits: theta adj(theta) is det * identity without a rounding, so the whole-court image is the court exactly
DYADIC = np.array([1, .25, .125, .125, 1, -.25, .25, .125, 1], dtype=F32)
RANK2 = np.array([1, 2, 3, 2, 4, 6, 0, 0, 1], dtype=F32)
ALL_NAN = np.full(9, np.nan, dtype=F32)
# adj's last row is (0, -3, 1): W = 1 - 3 yn changes sign at yn = 1/3 inside the canvas.  Sign-blind, the rows yn >= 1/2 are
# counted (|yn| <= 3 yn - 1); a W > 0 rule would stop at yn <= 1/4.
HORIZON = np.array([1, 0, 0, 0, 1, 0, 0, 3, 1], dtype=F32)

RASTERS = [(2, 2), (8, 8), (80, 45), (320, 180)]            # (wc, hc)


def perspective(name, amount=0.15):
    r = rng(("theta", name))
    t = np.eye(3) + r.uniform(-amount, amount, (3, 3))
    t[2, 2] = 1.0
    return t.reshape(9).astype(F32)


def margins(raster):
    return [(0, 0), (1, 1), (raster[0] // 2, raster[1] // 2)]


def region_batches():
    """(theta_pred, theta_gt) of B = 1 and B = 3, a different theta per frame"""
    a, b, c = perspective("a"), perspective("b"), perspective("c", 0.4)
    return [(np.stack([a]), np.stack([b])),
            (np.stack([a, c, HORIZON]), np.stack([IDENTITY, b, a]))]


def hand_cases():
    """(name, mode, (wc, hc), (mx, my), theta_pred, theta_gt, [nA, nB, nAB]) with the counts derived by hand"""
    out = []
    for wc, hc in RASTERS:
        out.append((f"identity-part-{wc}x{hc}", 0, (wc, hc), (0, 0), IDENTITY, IDENTITY, [wc * hc] * 3))
        for m in margins((wc, hc))[1:]:
            out.append((f"identity-whole-{wc}x{hc}-m{m[0]}", 1, (wc, hc), m, IDENTITY, IDENTITY, [wc * hc] * 3))
    # adj(diag(.5, .5, 1)) = diag(.5, .5, .25): |2x - (wc-1)| <= (wc-1) / 2.  320: x = 80 .. 239 (160); 180: y = 45 .. 134 (90)
    out.append(("half-320x180", 0, (320, 180), (0, 0), HALF, IDENTITY, [14400, 57600, 14400]))
    # 321: |2x - 320| <= 160, x = 80 .. 240 (161); 181: |2y - 180| <= 90, y = 45 .. 135 (91): the boundary lies ON pixel
    # centres, so these counts hold only with the inclusive <=
    out.append(("half-321x181", 0, (321, 181), (0, 0), HALF, IDENTITY, [161 * 91, 321 * 181, 161 * 91]))
    for bad, name in ((RANK2, "rank-deficient"), (ALL_NAN, "all-nan")):
        out.append((f"{name}-part", 0, (80, 45), (0, 0), bad, IDENTITY, [0, 3600, 0]))
        out.append((f"{name}-whole", 1, (80, 45), (40, 22), bad, IDENTITY, [0, 3600, 0]))
        out.append((f"{name}-gt-whole", 1, (80, 45), (40, 22), IDENTITY, bad, [0, 3600, 0]))
    return out


# ------------------------------------------------------------------------------------------------ points
def court_points(n_side=(7, 5)):
    """odd multiples of 1/8 and 1/6-free dyadic values inside the court: no point at the origin, exact in a few bits"""
    xs = (2 * np.arange(n_side[0]) - (n_side[0] - 1)) / 8.0 + 1 / 16.0
    ys = (2 * np.arange(n_side[1]) - (n_side[1] - 1)) / 8.0 + 1 / 16.0
    return np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2).astype(np.float64)


def many_points(n=150):
    """more points than a wave has lanes, some outside the court"""
    return rng("many-points").uniform(-1.2, 1.2, (n, 2))


def translation(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty, 0, 0, 1], dtype=F32)


def random_pairs(B, name, amount=0.2):
    return (np.stack([perspective((name, "p", i), amount) for i in range(B)]),
            np.stack([perspective((name, "g", i), amount) for i in range(B)]))
