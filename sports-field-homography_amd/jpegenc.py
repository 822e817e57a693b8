"""Baseline JPEG files made on the device: ``(B,H,W,3)`` / ``(B,H,W)`` uint8 tensors -> encoded bytes, in two launches on the
caller's current stream (``csrc/jpegenc.hip``), with no synchronisation and no stock torch kernel.

    enc = JpegEncoder(720, 1280, channels=3, batch=16, quality=90)
    batch = enc.encode(overlay_u8)                # JpegBatch: .data, .offsets, .sizes on the device
    files = batch.to_host()                       # list of 1-D uint8 arrays, what outputs.encode_jpeg returns

The files are the ones libjpeg writes - byte for byte those of PIL's ``save(.., "JPEG", quality=q, subsampling=2,
restart_marker_rows=1)`` (gray without ``subsampling``), which tests/test_jpegenc_host.py pins through the numpy restatement
``tests/jpegenc_ref.py``: JFIF 1.01 header, Annex K quantisation tables scaled by libjpeg's quality rule, 4:2:0, the "islow"
integer DCT, Annex K Huffman tables, a restart interval of one MCU row.  ``cv2.imwrite(path, img, [IMWRITE_JPEG_QUALITY, q])``
(the reference's predict.py:394) is the same libjpeg with the same defaults and no restart markers: its file decodes to the
same pixels.

``sfh_jpeg_encode`` has one workgroup per (image, MCU row) - a restart interval is byte aligned and predicts its DC values
from 0, so MCU rows are independent; ``sfh_jpeg_pack`` one per image.  In compact mode (the default) the files lie back to
back in ``data``, as ``pngenc``'s do.

Stated deviations: restart markers are added, so a file is larger than ``cv2.imwrite``'s by the 6-byte DRI segment and 2 bytes
plus at most 7 padding bits per MCU row; the Huffman tables are Annex K's, not optimised; there is no 4:4:4, no 4:2:2 and no
progressive mode; the decoder is ``sfh_amd.jpegdec``.  JPEG is for photographs: masks and labels hold class ids and stay PNG.
"""

import torch

from . import _lib
from ._codec import BatchEncoder, JpegBatch, as_image_batch, image_files_from_batch, ptr, stream  # noqa: F401 (re-exported)

MAX_WIDTH = _lib.ABI.defines["SFH_JPEG_MAX_WIDTH"]


def jpeg_capacity(H, W, C):
    """upper bound of the size of one encoded H x W x C image (every coefficient at its longest code, every byte stuffed): it
    sizes every buffer, and the encoder never writes past it"""
    H, W, C = int(H), int(W), int(C)
    if C not in (1, 3):
        raise ValueError(f"jpeg_capacity: {C} channels (1 gray, 3 colour)")
    if H < 1 or W < 1 or W > MAX_WIDTH or H > 65535:
        raise ValueError(f"jpeg_capacity: image {W}x{H}x{C} (at most {MAX_WIDTH} wide and 65535 high)")
    cap = _lib.load().sfh_jpeg_capacity(H, W, C)
    if cap < 0:
        _lib.check(-1, "jpeg_capacity")
    return int(cap)


def _check_quality(quality, who):
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"{who}: quality {quality!r} (an integer 1 .. 100)")
    return int(quality)


class JpegEncoder(BatchEncoder):
    """Encoder of batches of up to ``batch`` H x W images of ``channels`` (1 | 3) channels at one quality; owns the scratch,
    output, sizes and offsets buffers (``encode`` reuses them: a JpegBatch is valid until the next call without ``out``).  bgr:
    3-channel tensors are BGR in memory (cv2's convention, like ``PngEncoder``); False for RGB tensors."""
    batch_type = JpegBatch

    capacity_of = staticmethod(jpeg_capacity)

    def __init__(self, H, W, channels=3, batch=1, quality=90, bgr=True, compact=True, device="cuda", _window_dwords=0):
        if int(batch) >= 1:                       # the batch refusal comes first, as in every encoder
            self.quality = _check_quality(quality, "JpegEncoder")
        self._window = int(_window_dwords)        # tests only: a smaller LDS bit window, to reach the multi-pass branch
        super().__init__(H, W, channels, batch, bgr, compact, device)
        self.intervals = -(-self.H // (16 if self.C == 3 else 8))
        self._last = 0                            # images of the last encode

    def scratch_bytes_of(self, lib):
        return lib.sfh_jpeg_scratch_bytes(self.B, self.H, self.W, self.C)

    def _launch(self, images_u8, b, out, dev):
        lib = _lib.load()
        _lib.check(lib.sfh_jpeg_encode(ptr(images_u8), b, self.H, self.W, self.C, int(self.bgr), self.quality,
                                       ptr(self.scratch), self.scratch_bytes, self._window, stream(dev)), "jpeg_encode")
        _lib.check(lib.sfh_jpeg_pack(ptr(self.scratch), self.scratch_bytes, b, self.H, self.W, self.C, self.quality,
                                     int(self.compact), ptr(out.data), out.data.numel(), ptr(out.offsets), ptr(out.sizes),
                                     stream(dev)), "jpeg_pack")
        self._last = b

    def passes(self):
        """-> int64 array (b, intervals): through how many LDS bit windows every restart interval of the last ``encode`` was
        emitted (1 unless its bit stream is longer than the window; no rows before the first ``encode``).  Synchronises; a
        diagnostic."""
        n = self._last * self.intervals
        return self.scratch[:8 * n].view(torch.int32).cpu().numpy().reshape(self._last, self.intervals, 2)[:, :, 1].astype("int64")


def encode_jpeg_device(img_or_batch, quality=90, bgr=True):
    """One-off: a uint8 GPU tensor (H,W) or (H,W,3) -> one 1-D uint8 numpy array; a batch -> a list of them (the shapes are read
    as ``pngenc.encode_png_device`` reads them).  Synchronises (it returns host bytes)."""
    t, C, single = as_image_batch(img_or_batch, "encode_jpeg_device")
    enc = JpegEncoder(t.shape[1], t.shape[2], C, t.shape[0], quality=quality, bgr=bgr, device=t.device)
    files = enc.encode(t.contiguous()).to_host()
    return files[0] if single else files


def jpeg_files_from_batch(images, channels, where="host", quality=90):
    """the JPEG leg of the host drivers' ``image_format=`` switch (visualize, rectify_game): a batch (B,H,W[,3]) of uint8 BGR
    images, a GPU tensor or a host array -> list of B JPEG files as 1-D uint8 arrays.  "host": ``outputs.encode_jpeg`` (PIL)
    of the downloaded images; "device": encoded on the GPU, only the files are downloaded.  The two give the same bytes."""
    import numpy as np
    quality = _check_quality(quality, "jpeg_files_from_batch")
    if where == "host":
        from .outputs import encode_jpeg
        host = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        return [encode_jpeg(img, quality) for img in host]
    if where != "device":
        raise ValueError(f'png={where!r} ("host" or "device")')
    if not isinstance(images, torch.Tensor) or images.device.type != "cuda":
        raise RuntimeError('png="device" needs the images on the GPU - the HIP path has no CPU fallback')
    enc = JpegEncoder(images.shape[1], images.shape[2], channels, images.shape[0], quality=quality, device=images.device)
    return enc.encode(images.contiguous()).to_host()
