"""Images and size pairs for the resize tests (tests/test_resample_host.py, tests/test_gpu_resample.py).  Everything is
generated from fixed seeds.  Sizes are HEIGHT x WIDTH, as array shapes are."""
import numpy as np

# (source H, W) -> (destination H, W): the host test's shapes
HOST_SHAPES = (((720, 1280), (360, 640)), ((1080, 1920), (360, 640)), ((187, 333), (360, 640)), ((37, 50), (16, 17)),
               ((1, 1), (5, 7)), ((9, 200), (9, 64)), ((64, 9), (3, 9)), ((360, 640), (720, 1280)), ((100, 100), (1, 1)),
               ((3, 5000), (2, 3)), ((720, 1280), (361, 641)), ((45, 80), (360, 640)))
TEMPLATE_SHAPE = ((1819, 3421), (360, 640))           # the NCAA template's size: L only (bicubic needs 23 taps per column)
# the pairs on which the closed form floor((i + 0.5) in / out) is not Pillow's NEAREST rule
NEAREST_NAMED = ((1000, 999), (88, 361), (1068, 99), (2312, 692), (786, 157), (1152, 412))
NEAREST_IMAGE_PAIRS = (((187, 333), (360, 640)), ((360, 640), (187, 333)), ((1000, 1000), (999, 999)))


def noise(shape, seed=0, dtype=np.uint8):
    hi = 256 if dtype == np.uint8 else 65536
    return np.random.default_rng(20261018 + seed).integers(0, hi, shape).astype(dtype)


def checker(h=64, w=64, period=3, channels=None):
    """0/255 squares of `period` pixels: bicubic overshoots below 0 and above 255 at every edge"""
    yy, xx = np.mgrid[0:h, 0:w]
    g = ((((yy // period) + (xx // period)) & 1) * 255).astype(np.uint8)
    return g if channels is None else np.ascontiguousarray(np.stack([g, 255 - g, np.roll(g, 1, 1)][:channels], axis=-1))


def ramp(h, w, channels=None):
    yy, xx = np.mgrid[0:h, 0:w]
    g = ((xx * 7 + yy * 3) % 256).astype(np.uint8)
    return g if channels is None else np.ascontiguousarray(np.stack([g, g[::-1], g[:, ::-1]][:channels], axis=-1))


def host_cases():
    """name -> (uint8 array (H,W) or (H,W,3), destination (H, W))"""
    c = {}
    for k, (src, dst) in enumerate(HOST_SHAPES):
        c[f"noise_{src[0]}x{src[1]}_to_{dst[0]}x{dst[1]}_L"] = (noise(src, k), dst)
        c[f"noise_{src[0]}x{src[1]}_to_{dst[0]}x{dst[1]}_RGB"] = (noise(src + (3,), 100 + k), dst)
    src, dst = TEMPLATE_SHAPE
    c[f"noise_{src[0]}x{src[1]}_to_{dst[0]}x{dst[1]}_L"] = (noise(src, 50), dst)
    c["constant_L"] = (np.full((37, 50), 77, np.uint8), (16, 17))
    c["constant_RGB"] = (np.broadcast_to(np.array([10, 200, 255], np.uint8), (37, 50, 3)).copy(), (90, 100))
    c["ramp_L"] = (ramp(37, 50), (16, 17))
    c["ramp_RGB"] = (ramp(37, 50, 3), (90, 100))
    c["checker_L"] = (checker(), (90, 100))
    c["checker_RGB"] = (checker(channels=3), (90, 100))
    return c


def axis_pairs():
    """every (in, out) a host case resizes along one axis"""
    pairs = set()
    for src, dst in HOST_SHAPES + (TEMPLATE_SHAPE, ((64, 64), (90, 100)), ((37, 50), (90, 100))):
        pairs.add((src[0], dst[0]))
        pairs.add((src[1], dst[1]))
    return sorted(p for p in pairs if p[0] != p[1])


def nearest_pairs(count=300):
    rng = np.random.default_rng(20261019)
    return [tuple(int(v) for v in rng.integers(1, 2501, 2)) for _ in range(count)] + list(NEAREST_NAMED)


def variant(img, k):
    """image k of a batch made from one case: rolled by k pixels along x and 2k rows along y, plus k"""
    return np.ascontiguousarray(np.roll(img, (2 * k, k), axis=(0, 1)) + np.uint8(k))
