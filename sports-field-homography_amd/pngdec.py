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
from .pngenc import PngBatch, _ptr, _stream

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


class PngInfo(ctypes.Structure):
    """mirror of sfh_png_info (include/sfh_amd.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "channels", "bit_depth", "color_type", "interlace", "nidat",
                                              "idat_bytes", "cmf", "flg")] + [("adler", ctypes.c_uint32)] + [
        (n, ctypes.c_int32) for n in ("reason", "file_pos", "file_bytes", "range_pos", "joined_pos")]


assert ctypes.sizeof(PngInfo) == 64


def _refuse(reason, who, index=None):
    what = REASONS.get(int(reason), f"reason {reason}")
    where = "" if index is None or index < 0 else f" (file {index})"
    if reason >= 100:
        raise NotImplementedError(f"{who}: {what} is not built{where}")
    raise ValueError(f"{who}: {what}{where}")


def _as_bytes_array(f, who):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return np.frombuffer(f, dtype=np.uint8)
    a = np.asarray(f)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError(f"{who}: a file is bytes or a 1-D uint8 array, not {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def png_file_capacity(H, W, C):
    """the default ``max_file_bytes``: the filtered stream in stored blocks (5 bytes per 65535), chunk framing and 64 KB of
    ancillary chunks - every file a deflater makes of an H x W x C image fits, a file with more metadata needs the argument"""
    raw = int(H) * (1 + int(W) * int(C))
    return raw + 5 * (raw // 65535 + 1) + 12 * (raw // 8192 + 4) + 6 + 33 + 65536


def parse_png(data):
    """the host parse of one file as a dict (no device needed): size, channels, bit depth, colour type, the zlib header's two
    bytes, the Adler-32 that ends the joined IDAT bodies, their byte count and the bodies [(first byte, end byte)].  Every
    chunk's CRC-32 is verified.  Raises what ``PngDecoder.decode`` raises for a refused file."""
    a = _as_bytes_array(data, "parse_png")
    lib = _lib.load()
    info = PngInfo()
    src = a.ctypes.data_as(ctypes.c_void_p)
    if lib.sfh_png_parse(src, a.size, ctypes.byref(info), None, 0) != 0:
        _refuse(info.reason, "parse_png")
    ranges = np.zeros((info.nidat, 2), dtype=np.int32)
    if lib.sfh_png_parse(src, a.size, ctypes.byref(info), ranges.ctypes.data_as(ctypes.c_void_p), info.nidat) != 0:
        _refuse(info.reason, "parse_png")
    return {"width": info.width, "height": info.height, "channels": info.channels, "bit_depth": info.bit_depth,
            "color_type": info.color_type, "interlace": info.interlace, "nidat": info.nidat, "idat_bytes": info.idat_bytes,
            "cmf": info.cmf, "flg": info.flg, "adler": int(info.adler), "idat": [(int(a0), int(a1)) for a0, a1 in ranges]}


class PngDecoder:
    """Decoder of batches of up to ``batch`` PNG files of H x W pixels and ``channels`` (1 | 3 | 4) channels; owns the pinned
    staging buffer, its device copy, the scratch, the images and the per-image results - every buffer is allocated once, and the
    images ``decode`` returns without ``out`` are valid until the next call.  bgr: 3- and 4-channel images come out BGR(A) in
    memory (cv2's convention, like ``outputs.decode_png``); False for the file's order."""

    def __init__(self, H, W, channels=1, batch=1, bgr=True, max_file_bytes=None, device="cuda", _serial_only=False):
        self.H, self.W, self.C, self.B = int(H), int(W), int(channels), int(batch)
        if self.B < 1:
            raise ValueError(f"PngDecoder: batch {batch}")
        if self.C not in (1, 3, 4) or self.H < 1 or self.W < 1:
            raise ValueError(f"PngDecoder: image {self.W}x{self.H}x{self.C} (1, 3 or 4 channels)")
        self.max_file_bytes = png_file_capacity(self.H, self.W, self.C) if max_file_bytes is None else int(max_file_bytes)
        self.bgr = bool(bgr)
        self.serial_only = bool(_serial_only)              # tests: the serial leg on files the segmented leg would take
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PngDecoder: device {self.device} - the HIP path has no CPU fallback")
        lib = _lib.load()
        self.staging_bytes = int(lib.sfh_png_dec_staging_bytes(self.B, self.H, self.W, self.C, self.max_file_bytes))
        self.scratch_bytes = int(lib.sfh_png_dec_scratch_bytes(self.B, self.H, self.W, self.C))
        if self.staging_bytes < 0 or self.scratch_bytes < 0:
            raise ValueError(f"PngDecoder: {self.B} files of {self.W}x{self.H}x{self.C}, at most {self.max_file_bytes} bytes each: "
                             "refused, or buffers of 2 GiB or more")
        self.staging = torch.empty(self.staging_bytes, dtype=torch.uint8).pin_memory()
        self.staged = torch.empty(self.staging_bytes, dtype=torch.uint8, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self.out = torch.empty(self._shape(self.B), dtype=torch.uint8, device=self.device)
        self._status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._segmented = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._uploaded = None                     # event behind the last copy out of the staging buffer
        self._used = self._n = 0

    def _shape(self, n):
        return (n, self.H, self.W) + ((self.C,) if self.C > 1 else ())

    def stage(self, files):
        """host only: parse the files (every chunk CRC verified) and pack them into the pinned staging buffer -> number of files.
        Waits for the copy of the previous batch out of that buffer; raises for a refused file, with nothing launched."""
        if isinstance(files, PngBatch):
            files = files.to_host()
        files = [_as_bytes_array(f, "PngDecoder") for f in files]
        n = len(files)
        if not 1 <= n <= self.B:
            raise ValueError(f"PngDecoder: {n} files (1 .. {self.B})")
        if self._uploaded is not None:
            self._uploaded.synchronize()
            self._uploaded = None
        ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in files])
        sizes = (ctypes.c_int64 * n)(*[f.size for f in files])
        reason, index = ctypes.c_int32(0), ctypes.c_int32(-1)
        used = _lib.load().sfh_png_dec_stage(ptrs, sizes, n, self.H, self.W, self.C, self.max_file_bytes,
                                             ctypes.c_void_p(self.staging.data_ptr()), self.staging_bytes, ctypes.byref(reason),
                                             ctypes.byref(index))
        if used < 0:
            self._n = 0
            if reason.value:
                _refuse(reason.value, "PngDecoder", index.value)
            _lib.check(-1, "png_dec_stage")
        self._used, self._n = int(used), n
        return n

    def upload(self):
        """the staged batch -> the device, one non-blocking copy on the current stream"""
        if self._n == 0:
            raise RuntimeError("PngDecoder.upload: stage() a batch first")
        self.staged[:self._used].copy_(self.staging[:self._used], non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))

    def _checked_out(self, out, n):
        want = self._shape(n)
        if not isinstance(out, torch.Tensor):
            raise ValueError(f"PngDecoder: out: expected a tensor, got {type(out).__name__}")
        if out.dtype != torch.uint8:
            raise ValueError(f"PngDecoder: out: dtype {out.dtype} (uint8 only)")
        if tuple(out.shape[1:]) != want[1:] or out.dim() != len(want) or out.shape[0] < n:
            raise ValueError(f"PngDecoder: out: expected ({n}+,{','.join(map(str, want[1:]))}), got {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError("PngDecoder: out: expected a contiguous tensor")
        if out.device != self.staged.device:
            raise RuntimeError(f"PngDecoder: out on {out.device}, the decoder on {self.staged.device}")
        return out

    def decode_staged(self, out=None):
        """the uploaded batch -> images (n,H,W[,C]): one small memset and 5 launches on the current stream, 10 when a file of
        the batch has more than one IDAT chunk"""
        n = self._n
        if n == 0:
            raise RuntimeError("PngDecoder.decode_staged: stage() and upload() a batch first")
        out = self.out if out is None else self._checked_out(out, n)
        dev = self.device
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sfh_png_decode(ctypes.c_void_p(self.staging.data_ptr()), _ptr(self.staged), self.staging_bytes, n,
                                                  self.H, self.W, self.C, int(self.bgr), self.max_file_bytes, int(self.serial_only),
                                                  _ptr(self.scratch), self.scratch_bytes, _ptr(out), _ptr(self._status),
                                                  _ptr(self._segmented), _stream(dev)), "png_decode")
        return out[:n]

    def decode(self, files, out=None):
        """files: a list of b <= batch files (bytes or 1-D uint8 arrays) or a PngBatch -> uint8 (b,H,W[,C]) images on the GPU.
        out: a contiguous uint8 tensor of that shape (or with more images) to decode into.  Everything wrong with the files'
        chunks or with ``out`` raises before anything is launched."""
        if out is not None:
            n = len(files.sizes) if isinstance(files, PngBatch) else len(files)
            self._checked_out(out, n)
        self.stage(files)
        self.upload()
        return self.decode_staged(out)

    @property
    def status(self):
        """int32 (b) of the last call: 0, or the OR of 1 (an over-subscribed or incomplete code-length set, or none for
        end-of-block), 2 (symbols 286 / 287, distance codes 30 / 31, bits that are no code, block type 3), 4 (a distance beyond
        the bytes produced), 8 (a stored block with LEN != ~NLEN), 16 (output short of or beyond H (1 + W C)), 32 (the bits end
        early), 64 (a filter byte above 4), 128 (an Adler-32 mismatch) - such an image came back as zeros.  Synchronises."""
        return self._status[:self._n].cpu().numpy()

    def segmented(self):
        """bool (b) of the last call: whether the image's filtered stream came from the segmented leg.  Synchronises."""
        return self._segmented[:self._n].cpu().numpy().astype(bool)


def _file_list(file_or_files):
    single = isinstance(file_or_files, (bytes, bytearray, memoryview, np.ndarray))
    if single:
        return [file_or_files], True
    return (file_or_files.to_host() if isinstance(file_or_files, PngBatch) else list(file_or_files)), False


def decode_png_device(file_or_files, bgr=True, device="cuda"):
    """One-off: one file (bytes or a 1-D uint8 array) -> a uint8 GPU tensor (H,W) or (H,W,3|4); a list of files or a PngBatch
    -> (B,H,W[,C]).  The size and the channels are read from the first file.  Raises RuntimeError when an image has a status."""
    files, single = _file_list(file_or_files)
    if not files:
        raise ValueError("decode_png_device: no files")
    head = parse_png(files[0])
    dec = PngDecoder(head["height"], head["width"], head["channels"], len(files), bgr=bgr,
                     max_file_bytes=max(max(len(f) for f in files), 8), device=device)
    images = dec.decode(files)
    if dec.status.any():
        raise RuntimeError(f"decode_png_device: corrupt compressed data, status {dec.status.tolist()}")
    return images[0] if single else images


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
