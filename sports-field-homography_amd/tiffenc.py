"""8- and 16-bit TIFF files made on the device - the UV labels as the reference's ``BasicDataset(use_uv=True)`` reads them:
``(B,H,W)`` / ``(B,H,W,3)`` uint8 or uint16 tensors -> encoded bytes, in two launches on the caller's current stream
(``csrc/tiffenc.hip``, core ``csrc/tiff_core.h``), with no synchronisation and no stock torch kernel.

    enc = TiffEncoder(720, 1280, channels=3, bits=16, batch=16)
    batch = enc.encode(uv_u16)                    # TiffBatch: .data, .offsets, .sizes on the device
    files = batch.to_host()                       # list of 1-D uint8 arrays, what outputs.encode_tiff returns

The files equal ``outputs.encode_tiff``'s byte for byte - the written-down rule: little endian, strips of about 8 KB directly
behind the header, LZW (greedy, as libtiff writes it: a strip whose dictionary never fills is libtiff's strip) with predictor 2,
the IFD last.  bgr=True (the default, ``pngenc``'s meaning) stores three samples reversed: a label (id, u, v) is stored (v, u,
id), which ``cv2.imread(path, -1)`` returns as (id, u, v) with the id in channel 0, where the reference takes it.

``sfh_tiff_encode`` has one wave per (image, strip); ``sfh_tiff_pack`` one workgroup per image, the files back to back in
``data``.  The LZW of a strip is serial: the wave forms the strip's bytes in parallel, 4 KB at a time, and walks them as one.
"""
import numpy as np
import torch

from . import _lib
from ._codec import BatchEncoder, TiffBatch, as_image_batch, ptr, stream
from .outputs import tiff_strip_rows

_COMPRESSION = {"none": 1, "lzw": 5}


class TiffEncoder(BatchEncoder):
    """Encoder of batches of up to ``batch`` H x W images of ``channels`` (1 | 3) samples of ``bits`` (8 | 16) bits; owns the
    scratch, output, sizes and offsets buffers (``encode`` reuses them: a TiffBatch is valid until the next call without
    ``out``).  compression "lzw" | "none"; predictor 1 | 2 (LZW only, as in libtiff: an uncompressed file is written undifferenced
    with Predictor 1); rows_per_strip: None for max(1, 8192 // bytes per row).  bgr: 3-channel tensors are stored reversed."""
    batch_type = TiffBatch

    def __init__(self, H, W, channels=3, bits=16, batch=1, bgr=True, compression="lzw", predictor=2, rows_per_strip=None,
                 device="cuda"):
        if int(bits) not in (8, 16) or int(channels) not in (1, 3) or int(H) < 1 or int(W) < 1:
            raise ValueError(f"TiffEncoder: image {W}x{H}x{channels} of {bits} bits (1 or 3 channels of 8 or 16 bits)")
        if compression not in _COMPRESSION:
            raise ValueError(f'TiffEncoder: compression={compression!r} ("lzw" or "none")')
        if predictor not in (1, 2):
            raise ValueError(f"TiffEncoder: predictor={predictor!r} (1 or 2)")
        self.bits = int(bits)
        self.SAMPLE = torch.uint8 if self.bits == 8 else torch.uint16
        self.compression = _COMPRESSION[compression]
        self.predictor = int(predictor) if compression == "lzw" else 1
        self.rows_per_strip = tiff_strip_rows(H, W, channels, self.bits, rows_per_strip)
        super().__init__(H, W, channels, batch, bgr, True, device)

    def capacity_of(self, H, W, C):
        cap = _lib.load().sfh_tiff_capacity(H, W, C, self.bits, self.compression, self.rows_per_strip)
        if cap < 0:
            _lib.check(-1, "tiff_capacity")
        return int(cap)

    def scratch_bytes_of(self, lib):
        return lib.sfh_tiff_scratch_bytes(self.B, self.H, self.W, self.C, self.bits, self.compression, self.rows_per_strip)

    def _launch(self, images, b, out, dev):
        lib = _lib.load()
        _lib.check(lib.sfh_tiff_encode(ptr(images), b, self.H, self.W, self.C, self.bits, int(self.bgr), self.compression,
                                       self.predictor, self.rows_per_strip, ptr(self.scratch), self.scratch_bytes, stream(dev)),
                   "tiff_encode")
        _lib.check(lib.sfh_tiff_pack(ptr(self.scratch), self.scratch_bytes, b, self.H, self.W, self.C, self.bits,
                                     self.compression, self.predictor, self.rows_per_strip, 1, ptr(out.data), out.data.numel(),
                                     ptr(out.offsets), ptr(out.sizes), stream(dev)), "tiff_pack")


def encode_tiff_device(img_or_batch, bgr=True, compression="lzw", predictor=2, rows_per_strip=None):
    """One-off: a uint8 / uint16 GPU tensor (H,W) or (H,W,3) -> one 1-D uint8 numpy array; a batch -> a list of them (a 3-D
    tensor whose last dimension is 3 is ONE colour image, as in ``encode_png_device``).  Synchronises (it returns host bytes)."""
    t, C, single = as_image_batch(img_or_batch, "encode_tiff_device", (torch.uint8, torch.uint16))
    enc = TiffEncoder(t.shape[1], t.shape[2], C, 8 * t.element_size(), t.shape[0], bgr=bgr, compression=compression,
                      predictor=predictor, rows_per_strip=rows_per_strip, device=t.device)
    files = enc.encode(t.contiguous()).to_host()
    return files[0] if single else files


def files_from_batch(images, tif="host"):
    """The ``tif=`` switch of ``prepare_dataset``: a batch (B,H,W,3) of uint16 UV labels, a GPU tensor or a host array -> list of
    B TIFF files as 1-D uint8 arrays.  "host": ``outputs.encode_tiff`` of the downloaded labels; "device": encoded on the GPU in
    one ``TiffEncoder.encode``, only the files are downloaded."""
    if tif == "host":
        from .outputs import encode_tiff
        host = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        return [encode_tiff(img) for img in host]
    if tif != "device":
        raise ValueError(f'tif={tif!r} ("host" or "device")')
    if not isinstance(images, torch.Tensor) or images.device.type != "cuda":
        raise RuntimeError('tif="device" needs the labels on the GPU - the HIP path has no CPU fallback')
    enc = TiffEncoder(images.shape[1], images.shape[2], images.shape[3] if images.dim() == 4 else 1, 8 * images.element_size(),
                      images.shape[0], device=images.device)
    return enc.encode(images.contiguous()).to_host()
