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
import ctypes

import numpy as np
import torch

from . import _lib

MAX_ROW = 32768


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


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


def split_files(data, offsets, sizes):
    """host bytes (1-D uint8 array), offsets (B+1) and sizes (B) -> list of B 1-D uint8 arrays (copies)"""
    return [np.array(data[int(o):int(o) + int(n)], dtype=np.uint8) for o, n in zip(offsets[:-1], sizes)]


class PngBatch:
    """the encoded files of one batch on the device: ``data`` uint8, file b = data[offsets[b] : offsets[b] + sizes[b]]"""

    def __init__(self, data, offsets, sizes):
        self.data, self.offsets, self.sizes = data, offsets, sizes

    def to_host(self):
        """-> list of B 1-D uint8 numpy arrays (the type ``outputs.encode_png`` returns); synchronises"""
        off = self.offsets.cpu().numpy()
        sizes = self.sizes.cpu().numpy()
        data = self.data[:int(off[-1])].cpu().numpy()
        return split_files(data, off, sizes)


class BatchEncoder:
    """what the device encoders (PngEncoder, sfh_amd.jpegenc.JpegEncoder) share: the output buffers and the refusals of
    ``encode``'s argument.  A subclass sets H, W, C, B, capacity, device and ``batch_type``."""
    batch_type = PngBatch

    def new_output(self):
        return self.batch_type(torch.empty(self.B * self.capacity, dtype=torch.uint8, device=self.device),
                               torch.empty(self.B + 1, dtype=torch.int64, device=self.device),
                               torch.empty(self.B, dtype=torch.int32, device=self.device))

    def _checked(self, images):
        """-> the number of images.  What is wrong with the tensor itself (type, dtype, shape, contiguity) is a ValueError
        wherever the tensor lies; a well-formed tensor that is not on the GPU is the RuntimeError of every HIP path."""
        who = type(self).__name__
        if not isinstance(images, torch.Tensor):
            raise ValueError(f"{who}: expected a tensor, got {type(images).__name__}")
        if images.dtype != torch.uint8:
            raise ValueError(f"{who}: dtype {images.dtype} (uint8 only)")
        want = (self.H, self.W) if self.C == 1 else (self.H, self.W, 3)
        shape = tuple(images.shape)
        if self.C == 1 and len(shape) == 4 and shape[3] == 1:
            shape = shape[:3]
        if len(shape) != len(want) + 1 or shape[1:] != want or not 1 <= shape[0] <= self.B:
            raise ValueError(f"{who}: expected (b,{','.join(map(str, want))}) with b <= {self.B}, got {tuple(images.shape)}")
        if not images.is_contiguous():
            raise ValueError(f"{who}: expected a contiguous tensor")
        if images.device.type != "cuda":
            raise RuntimeError(f"{who}: device {images.device} - the HIP path has no CPU fallback")
        return shape[0]


def as_image_batch(t, who):
    """how the one-off entry points read a tensor -> (batch tensor, channels, whether it was ONE image): a 2-D tensor and a 3-D
    tensor whose last dimension is 3 are one image, any other 3-D tensor a batch of gray images, a 4-D tensor (B,H,W,1|3) a
    batch"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{who}: dtype {t.dtype} (uint8 only)")
    single = t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)
    batch = t[None] if single else t
    if batch.dim() == 3:
        return batch, 1, single
    if batch.dim() == 4 and batch.shape[3] in (1, 3):
        return batch, int(batch.shape[3]), single
    raise ValueError(f"{who}: shape {tuple(t.shape)}")


class PngEncoder(BatchEncoder):
    """Encoder of batches of up to ``batch`` H x W images of ``channels`` (1 | 3) channels; owns the scratch, output, sizes and
    offsets buffers (``encode`` reuses them: a PngBatch is valid until the next call without ``out``).  bgr: 3-channel
    tensors are BGR in memory (cv2's convention, like ``outputs.encode_png``); False for RGB tensors."""

    def __init__(self, H, W, channels=1, batch=1, bgr=True, compact=True, device="cuda"):
        self.H, self.W, self.C, self.B = int(H), int(W), int(channels), int(batch)
        if self.B < 1:
            raise ValueError(f"PngEncoder: batch {batch}")
        self.capacity = png_capacity(self.H, self.W, self.C)
        self.bgr, self.compact = bool(bgr), bool(compact)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PngEncoder: device {self.device} - the HIP path has no CPU fallback")
        self.scratch_bytes = int(_lib.load().sfh_png_scratch_bytes(self.B, self.H, self.W, self.C))
        if self.scratch_bytes < 0 or self.capacity * self.B >= 2 ** 31:
            raise ValueError(f"PngEncoder: {self.B} images of {self.W}x{self.H}x{self.C}: encoded batch of 2 GiB or more")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self.out = self.new_output()

    def encode(self, images_u8, out=None):
        """images_u8: uint8 (b,H,W[,3]) on the GPU, b <= batch -> PngBatch (of b files: offsets[:b+1], sizes[:b])"""
        b = self._checked(images_u8)
        out = self.out if out is None else out
        lib = _lib.load()
        dev = images_u8.device
        with torch.cuda.device(dev):
            _lib.check(lib.sfh_png_encode(_ptr(images_u8), b, self.H, self.W, self.C, int(self.bgr), _ptr(self.scratch),
                                          self.scratch_bytes, _stream(dev)), "png_encode")
            _lib.check(lib.sfh_png_pack(_ptr(self.scratch), self.scratch_bytes, b, self.H, self.W, self.C, int(self.compact),
                                        _ptr(out.data), out.data.numel(), _ptr(out.offsets), _ptr(out.sizes), _stream(dev)),
                       "png_pack")
        if b == self.B:
            return out
        return PngBatch(out.data, out.offsets[:b + 1], out.sizes[:b])


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
