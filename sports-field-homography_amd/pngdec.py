"""Standard PNG files decoded on the device: a batch of PNG files as bytes -> ``(B,H,W)`` / ``(B,H,W,3|4)`` uint8 images on the
caller's current stream (``csrc/pngdec.hip``, decode core ``csrc/pngdec_core.h``), with no pixel on the host, no stock torch
kernel and no allocation inside a call.

    dec = PngDecoder(720, 1280, channels=1, batch=16)
    masks = dec.decode(files)                     # files: list of bytes / 1-D uint8 arrays, or a pngenc.PngBatch
    assert not dec.status.any()                   # synchronises; an image with a status comes back as zeros

The pixels are those of ``outputs.decode_png`` (gray as (H,W); RGB / RGBA as BGR(A) with ``bgr=True``, as stored otherwise -
then they are ``np.array(PIL.Image.open(f))``), which tests/test_pngdec_host.py pins to PIL.

The host checks the signature and every chunk's CRC-32, reads IHDR and the zlib header and lists the IDAT bodies
(``sfh_png_parse``); parses, range tables and files travel in one pinned staging buffer and one non-blocking copy.  On the device
the SERIAL leg - one wave per image inflates the joined IDAT bodies into the filtered stream, through a 48 KB LDS ring - is right
for every admitted file.  The SEGMENTED leg is tried first on files with 2 .. 1024 IDAT chunks: every chunk is decoded as a
deflate sequence of its own, and the image is accepted only if the device finds that every chunk ended exactly at its last byte
on a block boundary, only the last saw BFINAL, no match reached before its chunk's first byte, the byte counts sum to
H (1 + W C) and the Adler-32 of the result is the file's.  Files of ``sfh_amd.pngenc`` (one chunk per strip) and streams cut
at Z_FULL_FLUSH points pass; anything else takes the serial leg.  Then the Adler-32 check and one of two unfilter kernels
(None / Sub rows as prefix sums; the other filters as a skewed wavefront over bands of 64 rows).

Admitted: non-interlaced 8-bit files of colour type 0, 2 and 6, all five scanline filters, any number of IDAT chunks cut
anywhere, stored, fixed and dynamic blocks, ancillary chunks (skipped).  Refused on the host with nothing launched -
``NotImplementedError`` naming the feature for a well-formed file that needs something not built, ``ValueError`` for a malformed
one: other bit depths, palette and gray + alpha files, Adam7, APNG, another size or channel count than the decoder's, a file above
``max_file_bytes``, a chunk CRC mismatch, IDAT chunks missing or not consecutive, a missing IEND, a zlib header that is not
CM 8 / window <= 32 KB / no preset dictionary.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._codec import BatchDecoder, PngBatch, as_bytes_array, ptr, refuse, stream

REASONS = {1: "the bytes end inside the header", 2: "no PNG signature: not a PNG file", 3: "a chunk CRC mismatch",
           4: "a missing or malformed IHDR chunk", 5: "IDAT chunks that are not consecutive", 6: "no IDAT chunk",
           7: "no IEND chunk: the chunks end early", 8: "a zlib header that is not deflate with a window of at most 32 KB",
           9: "a zlib preset dictionary", 10: "an unknown critical chunk",
           11: "size or channels other than the decoder's", 12: "a file longer than the decoder's max_file_bytes",
           100: "a bit depth other than 8", 101: "a palette image", 102: "a gray + alpha image", 103: "Adam7 interlacing",
           104: "APNG"}

STATUS_BITS = {1: "an over-subscribed or incomplete code-length set", 2: "an invalid symbol, distance code or block type",
               4: "a distance beyond the bytes produced", 8: "a stored block with LEN != ~NLEN",
               16: "output short of or beyond H (1 + W C)", 32: "the bits end early", 64: "a filter byte above 4",
               128: "an Adler-32 mismatch"}


PngInfo = _lib.ABI.structs["sfh_png_info"]
assert ctypes.sizeof(PngInfo) == 64


def png_file_capacity(H, W, C):
    """the default ``max_file_bytes``: the filtered stream in stored blocks (5 bytes per 65535), chunk framing and 64 KB of
    ancillary chunks - every file a deflater makes of an H x W x C image fits, a file with more metadata needs the argument"""
    raw = int(H) * (1 + int(W) * int(C))
    return raw + 5 * (raw // 65535 + 1) + 12 * (raw // 8192 + 4) + 6 + 33 + 65536


def parse_png(data):
    """the host parse of one file as a dict (no device needed): size, channels, bit depth, colour type, the zlib header's two
    bytes, the Adler-32 that ends the joined IDAT bodies, their byte count and the bodies [(first byte, end byte)].  Every
    chunk's CRC-32 is verified.  Raises what ``PngDecoder.decode`` raises for a refused file."""
    a = as_bytes_array(data, "parse_png")
    lib = _lib.load()
    info = PngInfo()
    src = a.ctypes.data_as(ctypes.c_void_p)
    if lib.sfh_png_parse(src, a.size, ctypes.byref(info), None, 0) != 0:
        refuse(REASONS, info.reason, "parse_png")
    ranges = np.zeros((info.nidat, 2), dtype=np.int32)
    if lib.sfh_png_parse(src, a.size, ctypes.byref(info), ranges.ctypes.data_as(ctypes.c_void_p), info.nidat) != 0:
        refuse(REASONS, info.reason, "parse_png")
    return {"width": info.width, "height": info.height, "channels": info.channels, "bit_depth": info.bit_depth,
            "color_type": info.color_type, "interlace": info.interlace, "nidat": info.nidat, "idat_bytes": info.idat_bytes,
            "cmf": info.cmf, "flg": info.flg, "adler": int(info.adler), "idat": [(int(a0), int(a1)) for a0, a1 in ranges]}


class PngDecoder(BatchDecoder):
    """Decoder of batches of up to ``batch`` PNG files of H x W pixels and ``channels`` (1 | 3 | 4) channels; owns the pinned
    staging buffer, its device copy, the scratch, the images and the per-image results - every buffer is allocated once, and the
    images ``decode`` returns without ``out`` are valid until the next call.  bgr: 3- and 4-channel images come out BGR(A) in
    memory (cv2's convention, like ``outputs.decode_png``); False for the file's order.

    ``stage`` verifies every chunk's CRC-32.  ``decode_staged``: one small memset and 5 launches on the current stream, 10 when
    a file of the batch has more than one IDAT chunk.  ``status`` bits: 1 (an over-subscribed or incomplete code-length set, or
    none for end-of-block), 2 (symbols 286 / 287, distance codes 30 / 31, bits that are no code, block type 3), 4 (a distance
    beyond the bytes produced), 8 (a stored block with LEN != ~NLEN), 16 (output short of or beyond H (1 + W C)), 32 (the bits
    end early), 64 (a filter byte above 4), 128 (an Adler-32 mismatch)."""
    NAME, REASONS, batch_type = "png", REASONS, PngBatch
    CHANNELS, LIMITS = (1, 3, 4), "1, 3 or 4 channels"
    MIN_FILE_BYTES, CORRUPT = 8, "compressed"
    default_max_file_bytes = staticmethod(png_file_capacity)

    def __init__(self, H, W, channels=1, batch=1, bgr=True, max_file_bytes=None, device="cuda", _serial_only=False):
        self.serial_only = bool(_serial_only)              # tests: the serial leg on files the segmented leg would take
        super().__init__(H, W, channels, batch, bgr, max_file_bytes, device)
        self._segmented = torch.zeros(self.B, dtype=torch.int32, device=self.device)

    def _sizes(self, lib):
        return (lib.sfh_png_dec_staging_bytes(self.B, self.H, self.W, self.C, self.max_file_bytes),
                lib.sfh_png_dec_scratch_bytes(self.B, self.H, self.W, self.C))

    def _stage(self, lib, ptrs, sizes, n, reason, index):
        return lib.sfh_png_dec_stage(ptrs, sizes, n, self.H, self.W, self.C, self.max_file_bytes, ptr(self.staging),
                                     self.staging_bytes, reason, index)

    def _launch(self, lib, n, out, dev):
        _lib.check(lib.sfh_png_decode(ptr(self.staging), ptr(self.staged), self.staging_bytes, n, self.H, self.W, self.C,
                                      int(self.bgr), self.max_file_bytes, int(self.serial_only), ptr(self.scratch),
                                      self.scratch_bytes, ptr(out), ptr(self._status), ptr(self._segmented), stream(dev)),
                   "png_decode")

    @staticmethod
    def _head(f):
        head = parse_png(f)
        return head["height"], head["width"], head["channels"]

    def segmented(self):
        """bool (b) of the last call: whether the image's filtered stream came from the segmented leg.  Synchronises."""
        return self._segmented[:self._n].cpu().numpy().astype(bool)


def decode_png_device(file_or_files, bgr=True, device="cuda"):
    """One-off: one file (bytes or a 1-D uint8 array) -> a uint8 GPU tensor (H,W) or (H,W,3|4); a list of files or a PngBatch
    -> (B,H,W[,C]).  The size and the channels are read from the first file.  Raises RuntimeError when an image has a status."""
    return PngDecoder.decode_once("decode_png_device", file_or_files, bgr=bgr, device=device)


def masks_from_files(files, device):
    """the ``masks_decode="device"`` / ``decode="device"`` switch of the host drivers (visualize, read_dataset): PNG files of
    gray id masks of one size -> uint8 (B,H,W) on the GPU, in one PngDecoder.decode"""
    files = list(files)
    masks = decode_png_device(files, device=device)
    if masks.dim() != 3:
        raise ValueError("the mask files must hold gray id masks of one size")
    return masks


def frames_from_files(files, device, bgr=True):
    """the ``frames_format="png"`` switch of the host drivers (visualize, rectify_game): an iterable of file bytes -> uint8
    frames (B,H,W,3) on the GPU"""
    files = list(files)
    try:
        frames = decode_png_device(files, bgr=bgr, device=device)
    except (ValueError, NotImplementedError) as e:
        raise type(e)(f"frames_format='png': {e}") from e
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames_format='png': the drivers need 3-channel frames, these files are gray or RGBA")
    return frames
