"""Images for the JPEG encoder tests (tests/test_jpegenc_host.py, tests/test_gpu_jpegenc.py): name -> (uint8 array (H,W) or
(H,W,3), quality).  Everything is generated from fixed seeds; the four court templates are the packaged ones.  Sizes in names
are HEIGHT x WIDTH."""
import os

import numpy as np

from conftest import ROOT

TEMPLATES = ("ncaa_nc4_1280x720", "ncaa_nc4_640x360", "pitch_v3_nc4_1280x720", "pitch_v3_nc4_640x360")
# edge replication in both directions and odd chroma widths; half an MCU; one full-width interval; RSTm wrapping past 7
SHAPES = ((1, 1), (8, 8), (16, 16), (17, 33), (37, 50), (333, 187), (24, 16), (16, 24), (16, 1280), (16, 1920), (160, 48))
QUALITIES = (25, 50, 75, 90, 95, 100)


def _both(c, name, gray, quality=90):
    """a gray case and its colour version (three differently shifted copies as channels)"""
    c[name + "_gray"] = (np.ascontiguousarray(gray), quality)
    c[name + "_rgb"] = (np.ascontiguousarray(np.stack([gray, np.roll(gray, 3, 1), np.roll(gray, 5, 0)], axis=-1)), quality)


def small_cases():
    rng = np.random.default_rng(20261018)
    c = {}
    for H, W in SHAPES:
        c[f"noise_{H}x{W}_gray"] = (rng.integers(0, 256, (H, W), dtype=np.uint8), 90)
        c[f"noise_{H}x{W}_rgb"] = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 90)
    for q in QUALITIES:
        if q != 90:
            c[f"noise_37x50_q{q}_gray"] = (c["noise_37x50_gray"][0], q)
            c[f"noise_37x50_q{q}_rgb"] = (c["noise_37x50_rgb"][0], q)
    H, W = 37, 50
    yy, xx = np.mgrid[0:H, 0:W]
    c["constant_gray"] = (np.full((H, W), 77, np.uint8), 90)
    c["constant_rgb"] = (np.broadcast_to(np.array([10, 200, 90], np.uint8), (H, W, 3)).copy(), 90)
    _both(c, "hramp", (xx * 255 // (W - 1)).astype(np.uint8))
    _both(c, "vramp", (yy * 255 // (H - 1)).astype(np.uint8))
    # 8x8 blocks alternating 0 and 255 at quality 100: on the block grid in the upper half (flat blocks, DC differences of
    # category 11), shifted by half a block in the lower half (a full step inside every block: AC category 10, the largest)
    y2, x2 = np.mgrid[0:48, 0:80]
    blocks = ((((y2 // 8) + (x2 // 8)) & 1) * 255).astype(np.uint8)
    blocks[24:] = np.roll(blocks[24:], 4, axis=1)
    _both(c, "blocks0_255_q100", blocks, 100)
    # a one-pixel checkerboard at quality 25: high-frequency coefficients behind runs of zeros (of at most 15 here)
    _both(c, "checker_q25", (((yy + xx) & 1) * 255).astype(np.uint8), 25)
    # single cosines at quality 25, which leave ONE coefficient per block at zig-zag position 20, 40 and 63: ZRL once, twice and
    # three times in a block (the checkerboard's own runs depend on what quantisation leaves of its 16 odd-odd frequencies)
    x8 = np.arange(8)
    for z, (u, v) in ((20, (5, 0)), (40, (3, 5)), (63, (7, 7))):
        basis = np.outer(np.cos((2 * x8 + 1) * u * np.pi / 16), np.cos((2 * x8 + 1) * v * np.pi / 16))
        tile = np.clip(np.rint(128 + 120 * basis / np.abs(basis).max()), 0, 255).astype(np.uint8)
        _both(c, f"cosine_zz{z}_q25", np.tile(tile, (2, 4)), 25)
    # coefficient 63 survives (no EOB): cos(7 pi (2x+1)/16) cos(7 pi (2y+1)/16) at full amplitude, quality 100
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.clip(np.rint(128 + 127 * np.sign(np.outer(k, k))), 0, 255).astype(np.uint8)
    _both(c, "last_ac_q100", np.tile(tile, (3, 5)), 100)
    return c


def template_over_noise(name, seed=0):
    """the overlay's statistics: the court template coloured with the table of format_masks("rgb"), its bytes written as given,
    and blended over a noise frame by OverlayRenderer's rule: a black mask pixel keeps the frame, any other becomes
    (colour + frame) >> 1 per channel"""
    from sfh_amd.outputs import _palette_bytes
    ids = np.load(os.path.join(ROOT, "sports-field-homography_amd", "data", f"court_ids_{name}.npy"))
    ids = ids.reshape(ids.shape[-2:]).astype(np.uint8)
    frame = np.random.default_rng(100 + seed).integers(0, 256, ids.shape + (3,), dtype=np.uint8)
    col = _palette_bytes(4)[ids]
    out = np.where(col.any(axis=2, keepdims=True), (frame.astype(np.uint16) + col) >> 1, frame)
    return np.ascontiguousarray(out.astype(np.uint8))


def template_cases():
    return {f"template_{n}": (template_over_noise(n), 90) for n in TEMPLATES}


def variant(img, k):
    """image k of a batch made from one case: rolled by k pixels along x and k rows along y"""
    return np.ascontiguousarray(np.roll(img, (k, k), axis=(0, 1)))
