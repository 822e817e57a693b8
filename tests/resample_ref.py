"""numpy restatement of Pillow's 8-bit image resize (test infrastructure only): ``Image.resize(size, filter)`` of L and RGB images
for BOX, BILINEAR and BICUBIC (libImaging/Resample.c) and the NEAREST index rule (libImaging/Geometry.c, ImagingScaleAffine).
tests/test_resample_host.py pins it to the installed Pillow byte for byte; the device kernels are then pinned to it.

Per axis (precompute_coeffs + normalize_coeffs_8bpc), all in fp64: scale = in / out, fs = max(scale, 1), sup = support * fs; per
output index xx: c = (xx + 0.5) * scale, xmin = max(int(c - sup + 0.5), 0), n = min(int(c + sup + 0.5), in) - xmin,
w_x = f((x + xmin - c + 0.5) * (1 / fs)) - Pillow multiplies by the reciprocal, it does not divide -, the weights summed in index
order and divided by the sum unless that is 0, then k = int(w * 2^22 +- 0.5) truncated towards zero.  A pass is
clamp((2^21 + sum pixel * k) >> 22, 0, 255) in 32-bit int with an arithmetic shift; the horizontal pass runs first and only when
the widths differ, the vertical one only when the heights differ, the intermediate image is uint8.
"""
import math

import numpy as np

BOX, BILINEAR, BICUBIC = 4, 2, 3          # Pillow's numbering (Image.Resampling)
FILTERS = {"box": BOX, "bilinear": BILINEAR, "bicubic": BICUBIC}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0}
PRECISION_BITS = 32 - 8 - 2
NEAREST_PIL, NEAREST_CV2 = 0, 1


def _filter(filt, x):
    if filt == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    x = abs(x)
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(insize, outsize, filt):
    """-> (bounds int32 (out, 2) = (xmin, n), coef int32 (out, ksize) zero padded, ksize)"""
    scale = insize / outsize
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((outsize, 2), np.int32)
    coef = np.zeros((outsize, ksize), np.int32)
    for xx in range(outsize):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), insize) - xmin
        w = [_filter(filt, (x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coef[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return bounds, coef, ksize


def _pass(img, bounds, coef, axis):
    """one pass along `axis` (0 rows, 1 columns) of an (H,W,C) uint8 array"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t in range(n):
            acc = acc + src[xmin + t] * int(coef[xx, t])
        assert np.all(np.abs(acc) < 2 ** 31)          # Pillow accumulates in 32-bit int: no overflow to restate
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize(img, size, filt=BICUBIC):
    """Image.fromarray(img).resize(size, filt) on a uint8 (H,W) or (H,W,3) array; size = (W, H)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    wd, hd = int(size[0]), int(size[1])
    a = img.reshape(img.shape[0], img.shape[1], -1)
    if a.shape[1] != wd:
        b, k, _ = coeffs(a.shape[1], wd, filt)
        a = _pass(a, b, k, 1)
    if a.shape[0] != hd:
        b, k, _ = coeffs(a.shape[0], hd, filt)
        a = _pass(a, b, k, 0)
    return a.reshape((hd, wd) + img.shape[2:]).copy()


def nearest_index(insize, outsize, rule=NEAREST_PIL):
    """source index of every output index: Pillow's running fp64 sum, or OpenCV's INTER_NEAREST closed form"""
    idx = np.empty(outsize, np.int32)
    if rule == NEAREST_PIL:
        a = insize / outsize
        x = a * 0.5
        for i in range(outsize):
            idx[i] = min(int(x), insize - 1)
            x += a
    else:
        ifx = 1.0 / (outsize / insize)
        for i in range(outsize):
            idx[i] = min(int(math.floor(i * ifx)), insize - 1)
    return idx


def nearest_index_closed_form(insize, outsize):
    """floor((i + 0.5) * in / out): NOT Pillow's rule (it differs on e.g. 1000 -> 999); kept so that a test can say so"""
    a = insize / outsize
    return np.minimum(np.floor((np.arange(outsize) + 0.5) * a).astype(np.int32), insize - 1)


def resize_nearest(img, size, rule=NEAREST_PIL):
    """nearest resize of an (H,W[,C]) array to size = (W, H)"""
    img = np.asarray(img)
    sx = nearest_index(img.shape[1], int(size[0]), rule)
    sy = nearest_index(img.shape[0], int(size[1]), rule)
    return np.ascontiguousarray(img[sy][:, sx])
