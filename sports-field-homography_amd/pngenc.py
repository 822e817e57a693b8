"""PNG files made on the device: ``(B,H,W)`` / ``(B,H,W,3)`` uint8 tensors -> encoded bytes, in two launches on the caller's
current stream (``csrc/pngenc.hip``), with no synchronisation and no stock torch kernel.

    enc = PngEncoder(720, 1280, channels=1, batch=16)
    batch = enc.encode(masks_u8)                  # PngBatch: .data, .offsets, .sizes on the device
    files = batch.to_host()                       # list of 1-D uint8 arrays, what outputs.encode_png returns

The files are standard PNGs (PIL, OpenCV, the reference's ``viz_preds.py`` and ``outputs.decode_png`` read them), built only
from pieces every inflater accepts; the exact rule is restated in ``tests/pngenc_ref.py`` and the device output equals it byte
for byte: 8-bit gray or RGB, filter 1 (Sub) on every scanline, strips of at most 16 rows / 32768 bytes, each strip one
fixed-Huffman deflate block of run tokens (or a stored block when that is shorter) in its own IDAT chunk.

``sfh_png_encode`` has one workgroup per (image, strip); ``sfh_png_pack`` one per image.  In compact mode (the default) the
files lie back to back in ``data``: every pack workgroup sums the byte counts of the images before its own from the strip
records the first launch left, so the scan over the B image totals needs neither a third launch nor a first block that the
others wait for.

Stated deviation: the files are 1.3-2.2x the size of ``outputs.encode_png``'s (zlib level 1) on label maps and raw-sized
(+ 0.4-0.8 %) on photographs and noise - dynamic Huffman tables and matches beyond distance 1 are not built.
"""
import numpy as np
import torch

from . import _lib
from ._codec import BatchEncoder, PngBatch, as_image_batch, ptr, split_files, stream  # noqa: F401 (re-exported)

MAX_ROW = _lib.ABI.defines["SFH_PNG_MAX_ROW"]


def png_capacity(H, W, C):
    """upper bound of the size of one encoded H x W x C image: it sizes every buffer, and the encoder never writes past it"""
    H, W, C = int(H), int(W), int(C)
    if C not in (1, 3):
        raise ValueError(f"png_capacity: {C} channels (1 gray, 3 colour)")
    if H < 1 or W < 1 or 1 + W * C > MAX_ROW:
        raise ValueError(f"png_capacity: image {W}x{H}x{C} (a scanline of 1 + W*C bytes may have at most {MAX_ROW})")
    cap = _lib.load().sfh_png_capacity(H, W, C)
    if cap < 0:
        _lib.check(-1, "png_capacity")
    return int(cap)


class PngEncoder(BatchEncoder):
    """Encoder of batches of up to ``batch`` H x W images of ``channels`` (1 | 3) channels; owns the scratch, output, sizes and
    offsets buffers (``encode`` reuses them: a PngBatch is valid until the next call without ``out``).  bgr: 3-channel
    tensors are BGR in memory (cv2's convention, like ``outputs.encode_png``); False for RGB tensors."""

    capacity_of = staticmethod(png_capacity)

    def __init__(self, H, W, channels=1, batch=1, bgr=True, compact=True, device="cuda"):
        super().__init__(H, W, channels, batch, bgr, compact, device)

    def scratch_bytes_of(self, lib):
        return lib.sfh_png_scratch_bytes(self.B, self.H, self.W, self.C)

    def _launch(self, images_u8, b, out, dev):
        lib = _lib.load()
        _lib.check(lib.sfh_png_encode(ptr(images_u8), b, self.H, self.W, self.C, int(self.bgr), ptr(self.scratch),
                                      self.scratch_bytes, stream(dev)), "png_encode")
        _lib.check(lib.sfh_png_pack(ptr(self.scratch), self.scratch_bytes, b, self.H, self.W, self.C, int(self.compact),
                                    ptr(out.data), out.data.numel(), ptr(out.offsets), ptr(out.sizes), stream(dev)), "png_pack")


def encode_png_device(img_or_batch, bgr=True):
    """One-off: a uint8 GPU tensor (H,W) or (H,W,3) -> one 1-D uint8 numpy array; a batch -> a list of them.  A 3-D tensor
    whose last dimension is 3 is ONE colour image, any other 3-D tensor a batch of gray images, a 4-D tensor (B,H,W,1|3) a
    batch.  Synchronises (it returns host bytes)."""
    t, C, single = as_image_batch(img_or_batch, "encode_png_device")
    enc = PngEncoder(t.shape[1], t.shape[2], C, t.shape[0], bgr=bgr, device=t.device)
    files = enc.encode(t.contiguous()).to_host()
    return files[0] if single else files


def files_from_batch(images, channels, png="host"):
    """The ``png=`` switch of the host drivers (visualize, prepare_dataset, rectify_game): a batch (B,H,W[,3]) of uint8 images,
    a GPU tensor or a host array -> list of B PNG files as 1-D uint8 arrays.  "host": ``outputs.encode_png`` of the downloaded
    images (today's bytes); "device": encoded on the GPU, only the files are downloaded."""
    if png == "host":
        from .outputs import encode_png
        host = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        return [encode_png(img) for img in host]
    if png != "device":
        raise ValueError(f'png={png!r} ("host" or "device")')
    if not isinstance(images, torch.Tensor) or images.device.type != "cuda":
        raise RuntimeError('png="device" needs the images on the GPU - the HIP path has no CPU fallback')
    enc = PngEncoder(images.shape[1], images.shape[2], channels, images.shape[0], device=images.device)
    return enc.encode(images.contiguous()).to_host()
