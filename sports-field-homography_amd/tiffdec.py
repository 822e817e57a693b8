"""8- and 16-bit TIFF files decoded on the device - the UV labels as the reference's ``BasicDataset(use_uv=True)`` reads them
(``cv2.imread(path, -1)`` of ``<name>.tif``): a batch of files as bytes -> ``(B,H,W)`` / ``(B,H,W,3)`` uint8 or uint16 images on
the caller's current stream (``csrc/tiffdec.hip``, core ``csrc/tiff_core.h``), with no pixel on the host, no stock torch kernel
and no allocation inside a call.

    dec = TiffDecoder(720, 1280, channels=3, bits=16, batch=16)
    uv = dec.decode(files)                        # files: list of bytes / 1-D uint8 arrays, or a tiffenc.TiffBatch
    assert not dec.status.any()                   # synchronises; an image with a status comes back as zeros

The pixels are those of ``outputs.decode_tiff``, the written-down rule, which tests/test_tiff_host.py holds to libtiff's own
strips and to Pillow.  bgr=True (the default, ``pngdec``'s meaning) returns the file's three samples reversed, as OpenCV does:
a label stored (v, u, id) comes back (id, u, v), the layout ``LabelMaker`` produces and ``split_uv`` consumes.

The host reads the header and the first IFD and checks every offset against the file (``sfh_tiff_parse``); parses, strip tables
and files travel in one pinned staging buffer and one non-blocking copy.  On the device one wave decodes one strip
(``tiff_lzw_kernel``, a grid over (image, strip): a 1280x720 label has about 720 strips), then a kernel per 8 rows undoes the
predictor as a prefix sum per channel, swaps ``MM`` samples, orders the channels and writes the image.

Admitted: classic TIFF, the first IFD, ``II`` and ``MM``, strips with any RowsPerStrip, chunky, FillOrder 1, unsigned samples of 8
or 16 bits, 1 (BlackIsZero) or 3 (RGB) per pixel, compression 1 and 5 (TIFF 6.0 LZW; a strip may lack its EOI), predictor 1 and 2
(ignored in an uncompressed file, as libtiff does), SHORT or LONG strip tables.  Refused on the host with nothing launched -
``NotImplementedError`` naming the feature, ``ValueError`` for a malformed file: ``REASONS``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._codec import BatchDecoder, TiffBatch, as_bytes_array, ptr, refuse, stream
from .outputs import TIFF_REASONS as REASONS

STATUS_BITS = {1: "a code above the next free code", 2: "a first code after Clear that is not a literal",
               4: "output short of or beyond the strip's rows", 8: "the bits end early"}


TiffInfo = _lib.ABI.structs["sfh_tiff_info"]
assert ctypes.sizeof(TiffInfo) == 64


def tiff_file_capacity(H, W, C, bits=16):
    """the default ``max_file_bytes``: the image uncompressed or in worst-case LZW strips of one row each, the tables of one
    strip per row, and 64 KB of other tags - a file with more metadata needs the argument"""
    raw = int(H) * int(W) * int(C) * (int(bits) // 8)
    return raw + raw // 2 + 16 * int(H) + 65536


def parse_tiff(data):
    """the host parse of one file as a dict (no device needed): width, height, channels, bits, compression, predictor (1 for an
    uncompressed file), big_endian, rows_per_strip, photometric and strips = [(offset, byte count, first row, rows)].  Raises
    what ``TiffDecoder.decode`` raises for a refused file."""
    a = as_bytes_array(data, "parse_tiff")
    lib = _lib.load()
    info = TiffInfo()
    src = a.ctypes.data_as(ctypes.c_void_p)
    if lib.sfh_tiff_parse(src, a.size, ctypes.byref(info), None, 0) != 0:
        refuse(REASONS, info.reason, "parse_tiff")
    strips = np.zeros((info.nstrips, 4), dtype=np.int32)
    if lib.sfh_tiff_parse(src, a.size, ctypes.byref(info), strips.ctypes.data_as(ctypes.c_void_p), info.nstrips) != 0:
        refuse(REASONS, info.reason, "parse_tiff")
    out = {k: getattr(info, k) for k in ("width", "height", "channels", "bits", "compression", "predictor", "rows_per_strip",
                                         "photometric")}
    out["big_endian"] = bool(info.big_endian)
    out["strips"] = [tuple(int(v) for v in s) for s in strips]
    return out


class TiffDecoder(BatchDecoder):
    """Decoder of batches of up to ``batch`` TIFF files of H x W pixels, ``channels`` (1 | 3) samples of ``bits`` (8 | 16) bits;
    owns the pinned staging buffer, its device copy, the scratch, the images and the per-image results - every buffer is
    allocated once, and the images ``decode`` returns without ``out`` are valid until the next call.  The files of a batch may
    differ in byte order, compression, predictor and strips.  bgr: 3-channel images come out with the file's samples reversed
    (cv2's convention); False for the file's order.

    ``decode_staged``: 3 launches on the current stream.  ``status`` bits: 1 (a code above the next free code), 2 (a first code
    after Clear that is not a literal), 4 (output short of or beyond a strip's rows * W * C * bytes), 8 (the bits end early)."""
    NAME, REASONS, batch_type = "tiff", REASONS, TiffBatch
    CHANNELS, LIMITS = (1, 3), "1 or 3 channels"
    MIN_FILE_BYTES, CORRUPT = 8, "LZW"

    def __init__(self, H, W, channels=3, bits=16, batch=1, bgr=True, max_file_bytes=None, device="cuda"):
        if int(bits) not in (8, 16):
            raise ValueError(f"TiffDecoder: {bits} bits (8 or 16)")
        self.bits = int(bits)
        self.SAMPLE = torch.uint8 if self.bits == 8 else torch.uint16
        self._sizes_detail = f" of {self.bits} bits"
        super().__init__(H, W, channels, batch, bgr, max_file_bytes, device)

    def default_max_file_bytes(self, H, W, C):
        return tiff_file_capacity(H, W, C, self.bits)

    def _sizes(self, lib):
        return (lib.sfh_tiff_dec_staging_bytes(self.B, self.H, self.W, self.C, self.bits, self.max_file_bytes),
                lib.sfh_tiff_dec_scratch_bytes(self.B, self.H, self.W, self.C, self.bits))

    def _stage(self, lib, ptrs, sizes, n, reason, index):
        return lib.sfh_tiff_dec_stage(ptrs, sizes, n, self.H, self.W, self.C, self.bits, self.max_file_bytes, ptr(self.staging),
                                      self.staging_bytes, reason, index)

    def _launch(self, lib, n, out, dev):
        _lib.check(lib.sfh_tiff_decode(ptr(self.staging), ptr(self.staged), self.staging_bytes, n, self.H, self.W, self.C,
                                       self.bits, int(self.bgr), self.max_file_bytes, ptr(self.scratch), self.scratch_bytes,
                                       ptr(out), ptr(self._status), stream(dev)), "tiff_decode")


def decode_tiff_device(file_or_files, bgr=True, device="cuda"):
    """One-off: one file (bytes or a 1-D uint8 array) -> a uint8 / uint16 GPU tensor (H,W) or (H,W,3); a list of files or a
    TiffBatch -> (B,H,W[,3]).  The size, the channels and the bits are read from the first file.  Raises RuntimeError when an image
    has a status."""
    who = "decode_tiff_device"
    single = isinstance(file_or_files, (bytes, bytearray, memoryview, np.ndarray))
    if single:
        files = [file_or_files]
    else:
        files = file_or_files.to_host() if isinstance(file_or_files, TiffBatch) else list(file_or_files)
    if not files:
        raise ValueError(f"{who}: no files")
    head = parse_tiff(files[0])
    dec = TiffDecoder(head["height"], head["width"], head["channels"], head["bits"], len(files), bgr=bgr,
                      max_file_bytes=max(max(len(f) for f in files), TiffDecoder.MIN_FILE_BYTES), device=device)
    images = dec.decode(files)
    if dec.status.any():
        raise RuntimeError(f"{who}: corrupt LZW data, status {dec.status.tolist()}")
    return images[0] if single else images
