"""Files for the JPEG decoder tests (tests/test_jpegdec_host.py, tests/test_gpu_jpegdec.py): name -> bytes of a JFIF file.
Everything comes from the fixed-seed images of tests/jpegenc_cases.py, written by PIL (libjpeg) with the options named in the
case, or by the encoder's restatement tests/jpegenc_ref.py (``ref_``).  A file with a restart interval has more than 8 segments,
so RST7 -> RST0 is reached.  Sizes in names are HEIGHT x WIDTH."""
import functools
import io

import numpy as np
from PIL import Image

import jpegenc_cases as EC
import jpegenc_ref as ER

SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (37, 50), (24, 16), (16, 24), (160, 48), (333, 187), (16, 1280))
QUALITIES = (25, 50, 75, 90, 95, 100)


def pil_file(img, quality=90, subsampling=None, optimize=False, dri=None):
    """dri: None | "rows" (restart_marker_rows=1) | "blocks" (restart_marker_blocks=1)"""
    kw = {"quality": quality, "optimize": optimize}
    if img.ndim == 3:
        kw["subsampling"] = 2 if subsampling is None else subsampling
    if dri == "rows":
        kw["restart_marker_rows"] = 1
    elif dri == "blocks":
        kw["restart_marker_blocks"] = 1
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data, bgr=False):
    """PIL's pixels of a file: (H,W,3) RGB (BGR) or (H,W)"""
    im = Image.open(io.BytesIO(bytes(data)))
    a = np.asarray(im)
    return np.ascontiguousarray(a[:, :, ::-1]) if bgr and a.ndim == 3 else a


def _mcus(H, W, kind):
    m = 16 if kind == "420" else 8
    return -(-H // m), -(-W // m)


@functools.lru_cache(maxsize=None)
def small_files():
    """the small cases (at most 333 x 187 pixels, and 16 x 1280): name -> bytes"""
    src = EC.small_cases()
    f = {}
    for H, W in SIZES:
        rgb, gray = src[f"noise_{H}x{W}_rgb"][0], src[f"noise_{H}x{W}_gray"][0]
        f[f"noise_{H}x{W}_420"] = pil_file(rgb)
        f[f"noise_{H}x{W}_444"] = pil_file(rgb, subsampling=0)
        f[f"noise_{H}x{W}_gray"] = pil_file(gray)
        for kind, img, sub in (("420", rgb, 2), ("444", rgb, 0), ("gray", gray, None)):
            rows, cols = _mcus(H, W, kind)
            if rows > 8:
                f[f"noise_{H}x{W}_{kind}_rows"] = pil_file(img, subsampling=sub, dri="rows", optimize=kind == "gray")
            if rows * cols > 8:
                f[f"noise_{H}x{W}_{kind}_blocks"] = pil_file(img, subsampling=sub, dri="blocks", optimize=kind == "420" and H * W < 20000)
    rgb, gray = src["noise_37x50_rgb"][0], src["noise_37x50_gray"][0]
    for q in QUALITIES:
        f[f"noise_37x50_q{q}_420_opt"] = pil_file(rgb, q, optimize=True)
        f[f"noise_37x50_q{q}_444_blocks"] = pil_file(rgb, q, subsampling=0, dri="blocks")
        f[f"noise_37x50_q{q}_gray_opt_blocks"] = pil_file(gray, q, optimize=True, dri="blocks")
    for name in ("constant", "hramp", "vramp", "blocks0_255_q100"):
        q = 100 if name.endswith("q100") else 90
        f[f"{name}_420"] = pil_file(src[name + "_rgb"][0], q)
        f[f"{name}_444_opt_blocks"] = pil_file(src[name + "_rgb"][0], q, subsampling=0, optimize=True, dri="blocks")
        f[f"{name}_gray_blocks"] = pil_file(src[name + "_gray"][0], q, dri="blocks")
    f["noise_333x187_q100_420"] = pil_file(src["noise_333x187_rgb"][0], 100)       # > 256 subsequences, many stuffed 0xFF
    # the encoder restatement's own files: a restart interval of one MCU row
    for name in ("noise_160x48_rgb", "noise_160x48_gray", "noise_333x187_rgb", "noise_333x187_gray"):
        f["ref_" + name] = ER.ref_encode(src[name][0], 90)
    return f


@functools.lru_cache(maxsize=None)
def template_files():
    """the four court templates over noise, as the overlay's statistics are: name -> bytes"""
    f = {}
    # (quality, subsampling, optimised tables, restart interval); PIL's optimising writer needs the whole file in its buffer of
    # max(64 KiB, W * H) bytes, which noise above about 1 byte per pixel does not fit
    how = ((90, 2, False, None), (90, 0, False, "rows"), (90, 2, False, "rows"), (75, 2, True, None))
    for name, (q, sub, opt, dri) in zip(EC.TEMPLATES, how):
        img = np.ascontiguousarray(EC.template_over_noise(name)[:, :, ::-1])
        f[f"template_{name}"] = pil_file(img, q, subsampling=sub, optimize=opt, dri=dri)
    return f


def big_file(H, W, dri=None):
    """a court template blended over noise, tiled / cropped to H x W, quality 90, 4:2:0"""
    t = EC.template_over_noise("ncaa_nc4_1280x720")
    reps = (-(-H // t.shape[0]), -(-W // t.shape[1]), 1)
    return pil_file(np.ascontiguousarray(np.tile(t, reps)[:H, :W]), 90, dri=dri)


def has_dri(data):
    return b"\xff\xdd\x00\x04" in bytes(data)[:1024]
