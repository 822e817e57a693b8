"""The pieces png_pack_kernel and jpeg_pack_kernel share (csrc/codec_pack.h: the compact base, the wave's slot copy, the closing
sizes / offsets writes) and BatchEncoder's partial-batch slice, on the MI355X against the numpy restatements, byte for byte."""
import functools

import numpy as np
import pytest
import torch

import jpegenc_ref as JR
import pngenc_ref as PR

pytestmark = pytest.mark.gpu

BATCH, PART, FILL, QUALITY = 6, 4, 0xA5, 90
SHAPES = {"png": (23, 37), "jpeg": (37, 50)}          # H, W of 3-channel images
SEED = 1              # chosen on the restatement alone: with it the six bases of both codecs cover all residues mod 4


def _images(H, W):
    """six blocky images under noise whose amplitude and number of rows grow with the index, so that the files differ in size
    (PNG's run tokens gain nothing on a noisy row, whatever the amplitude)"""
    rng = np.random.default_rng(SEED)
    imgs = []
    for k in range(BATCH):
        a = np.zeros((H, W, 3), np.int64)
        for _ in range(5):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            a[y:y + int(rng.integers(2, H)), x:x + int(rng.integers(2, W))] = rng.integers(0, 256, 3)
        a[:4 * k] += rng.integers(-4 * k, 4 * k + 1, a[:4 * k].shape)
        imgs.append(np.clip(a, 0, 255).astype(np.uint8))
    return np.stack(imgs)


@functools.lru_cache(maxsize=None)
def _case(codec):
    """-> (images, the restatement's files), computed once"""
    imgs = _images(*SHAPES[codec])
    encode = PR.ref_encode if codec == "png" else functools.partial(JR.ref_encode, quality=QUALITY)
    return imgs, [np.frombuffer(encode(im), np.uint8) for im in imgs]


def _encoder(codec, compact):
    H, W = SHAPES[codec]
    if codec == "png":
        from sfh_amd.pngenc import PngEncoder
        return PngEncoder(H, W, 3, BATCH, compact=compact)
    from sfh_amd.jpegenc import JpegEncoder
    return JpegEncoder(H, W, 3, BATCH, quality=QUALITY, compact=compact)


@pytest.mark.parametrize("compact", (True, False))
@pytest.mark.parametrize("codec", ("png", "jpeg"))
def test_pack_places_every_file_and_nothing_else(codec, compact):
    imgs, refs = _case(codec)
    lens = np.array([r.size for r in refs], np.int64)
    # the slot copy's head-byte branch must see every alignment of a destination: on the restatement alone
    assert {int(v) % 4 for v in np.cumsum(lens) - lens} == {0, 1, 2, 3}, (np.cumsum(lens) - lens).tolist()
    enc = _encoder(codec, compact)
    dev = torch.from_numpy(imgs).cuda()
    for b in (BATCH, PART):                                                     # the whole batch, then the partial-batch slice
        out = enc.new_output()
        out.data.fill_(FILL)
        got = enc.encode(dev[:b].contiguous(), out=out)
        assert got.data.data_ptr() == out.data.data_ptr() and isinstance(got, type(out))
        sizes, off, data = got.sizes.cpu().numpy(), got.offsets.cpu().numpy(), out.data.cpu().numpy()
        assert sizes.shape == (b,) and off.shape == (b + 1,)
        assert sizes.tolist() == lens[:b].tolist()
        if compact:
            want_off = np.concatenate([[0], np.cumsum(lens[:b])])
        else:
            want_off = np.arange(b + 1, dtype=np.int64) * enc.capacity
        assert off.tolist() == want_off.tolist()
        outside = np.ones(data.size, bool)
        for k in range(b):
            lo = int(want_off[k])
            assert np.array_equal(data[lo:lo + lens[k]], refs[k]), f"{codec} compact={compact} batch {b} file {k}"
            outside[lo:lo + lens[k]] = False
        assert (data[outside] == FILL).all(), f"{codec} compact={compact} batch {b}: {int((data[outside] != FILL).sum())} bytes " \
                                              "outside the files were written"
