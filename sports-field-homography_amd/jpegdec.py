"""Baseline JPEG files decoded on the device: a batch of JFIF files as bytes -> ``(B,H,W,3)`` / ``(B,H,W)`` uint8 frames on the
caller's current stream (``csrc/jpegdec.hip``, decode core ``csrc/jpegdec_core.h``), with no stock torch kernel and no
allocation inside a call.

    dec = JpegDecoder(720, 1280, channels=3, batch=16)
    frames = dec.decode(files)                    # files: list of bytes / 1-D uint8 arrays, or a jpegenc.JpegBatch
    assert not dec.status.any()                   # synchronises; an image with a status comes back as zeros

The pixels are the ones libjpeg gives - byte for byte those of ``PIL.Image.open`` (jidctint's "islow" IDCT, the triangle h2v2
upsampler, the 16-bit fixed-point YCbCr -> RGB tables), which tests/test_jpegdec_host.py pins through the numpy restatement
``tests/jpegdec_ref.py``.

The host parses the markers (``sfh_jpeg_parse``) and packs parses, segment tables and files into one pinned staging buffer that
travels in one non-blocking copy.  ``sfh_jpeg_entropy_decode`` has one workgroup per (image, segment between restart markers):
the segment's bits are cut into subsequences, a bounded fixed-point iteration over their exit states finds every subsequence's
true entry state, a last pass scatters the coefficients.  ``sfh_jpeg_decode_pixels``: status, IDCT, upsampling and colour.

Admitted: SOF0, 8 bits, one interleaved scan, gray or YCbCr at 4:2:0 or 4:4:4, any 8-bit quantisation and any Huffman tables
(optimised ones included), any restart interval, APPn / COM segments, fill bytes before markers.  Refused on the host with
nothing launched - ``NotImplementedError`` naming the feature for a well-formed file that needs something not built,
``ValueError`` for a malformed header: progressive and arithmetic coding, 12-bit samples, 16-bit quantisation tables, 2 or 4
components, RGB, 4:2:2 / 4:4:0 / 4:1:1, several scans, DNL, another size than the decoder's, a file above ``max_file_bytes``.
All files of one call share H, W and sampling; their tables may differ.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .jpegenc import JpegBatch, jpeg_capacity
from .pngenc import _ptr, _stream

REASONS = {1: "the bytes end inside the header", 2: "no SOI marker: not a JPEG file", 3: "a marker out of place",
           4: "a malformed SOF0 segment", 5: "a malformed or missing DQT / DHT table", 6: "a malformed SOS segment",
           7: "restart markers out of sequence or not matching the restart interval",
           8: "size, channels or sampling other than the decoder's (or the batch's first file's)",
           9: "a file longer than the decoder's max_file_bytes",
           100: "progressive coding", 101: "arithmetic coding", 102: "12-bit samples", 103: "16-bit quantisation tables",
           104: "2 or 4 components (CMYK / YCCK)", 105: "RGB components", 106: "sampling other than 4:2:0 / 4:4:4 (4:2:2, 4:4:0, 4:1:1)",
           107: "a non-interleaved file (several scans)", 108: "DNL / height 0", 109: "extended sequential, lossless or hierarchical frames"}


class HuffTab(ctypes.Structure):
    _fields_ = [("look", ctypes.c_uint16 * 256), ("maxcode", ctypes.c_int32 * 18), ("valoff", ctypes.c_int32 * 18),
                ("vals", ctypes.c_uint8 * 256)]


class JpegInfo(ctypes.Structure):
    """mirror of sfh_jpeg_info (include/sfh_amd.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "ncomp", "hsamp", "vsamp", "mcus_x", "mcus_y", "blocks_per_mcu",
                                              "restart_interval", "nsegments", "scan_begin", "scan_end", "reason")] + [
        ("qsel", ctypes.c_int32 * 3), ("dcsel", ctypes.c_int32 * 3), ("acsel", ctypes.c_int32 * 3),
        ("file_pos", ctypes.c_int32), ("file_bytes", ctypes.c_int32), ("seg_pos", ctypes.c_int32), ("nsub", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2), ("quant", (ctypes.c_uint16 * 64) * 4), ("dc", HuffTab * 4), ("ac", HuffTab * 4)]


assert ctypes.sizeof(JpegInfo) == 7920


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


def _tab(t):
    return {"look": np.array(t.look, dtype=np.int64), "maxcode": np.array(t.maxcode, dtype=np.int64),
            "valoff": np.array(t.valoff, dtype=np.int64), "vals": np.array(t.vals, dtype=np.int64)}


def parse_jpeg(data):
    """the host parse of one file as a dict (no device needed): sizes, sampling, table selectors, the quantisation tables in
    natural order, the Huffman tables in the lookup form the kernel reads, the scan's byte range, the restart interval and the
    segments [(first byte, end byte, first MCU)].  Raises what ``JpegDecoder.decode`` raises for a refused file."""
    a = _as_bytes_array(data, "parse_jpeg")
    lib = _lib.load()
    info = JpegInfo()
    src = a.ctypes.data_as(ctypes.c_void_p)
    if lib.sfh_jpeg_parse(src, a.size, ctypes.byref(info), None, 0) != 0:
        _refuse(info.reason, "parse_jpeg")
    segs = np.zeros((info.nsegments, 4), dtype=np.int32)
    if lib.sfh_jpeg_parse(src, a.size, ctypes.byref(info), segs.ctypes.data_as(ctypes.c_void_p), info.nsegments) != 0:
        _refuse(info.reason, "parse_jpeg")
    nc = info.ncomp
    used = lambda sel: sorted(set(sel[:nc]))
    return {"width": info.width, "height": info.height, "ncomp": nc, "hsamp": info.hsamp, "vsamp": info.vsamp,
            "mcus_x": info.mcus_x, "mcus_y": info.mcus_y, "blocks_per_mcu": info.blocks_per_mcu,
            "restart_interval": info.restart_interval, "nsegments": info.nsegments, "scan_begin": info.scan_begin,
            "scan_end": info.scan_end, "qsel": list(info.qsel[:nc]), "dcsel": list(info.dcsel[:nc]), "acsel": list(info.acsel[:nc]),
            "quant": {q: np.array(info.quant[q], dtype=np.int64) for q in used(info.qsel)},
            "dc": {k: _tab(info.dc[k]) for k in used(info.dcsel)}, "ac": {k: _tab(info.ac[k]) for k in used(info.acsel)},
            "segments": [tuple(int(v) for v in s[:3]) for s in segs]}


class JpegDecoder:
    """Decoder of batches of up to ``batch`` JFIF files of H x W pixels and ``channels`` (1 | 3) channels; owns the pinned staging
    buffer, its device copy, the scratch, the frames, ``status`` and the round counts - every buffer is allocated once, and the
    frames ``decode`` returns without ``out`` are valid until the next call.  bgr: 3-channel frames come out BGR in memory
    (cv2's convention, like the rest of the package); False for RGB."""

    def __init__(self, H, W, channels=3, batch=1, bgr=True, max_file_bytes=None, device="cuda", _subseq_bits=0):
        self.H, self.W, self.C, self.B = int(H), int(W), int(channels), int(batch)
        if self.B < 1:
            raise ValueError(f"JpegDecoder: batch {batch}")
        if self.C not in (1, 3) or self.H < 1 or self.W < 1 or self.H > 65535 or self.W > 65535:
            raise ValueError(f"JpegDecoder: image {self.W}x{self.H}x{self.C} (1 or 3 channels, at most 65535 a side)")
        self.max_file_bytes = jpeg_capacity(self.H, self.W, self.C) if max_file_bytes is None else int(max_file_bytes)
        self.bgr = bool(bgr)
        self.subseq_bits = int(_subseq_bits) if _subseq_bits else 1024    # tests: smaller ones reach many rounds on small files
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"JpegDecoder: device {self.device} - the HIP path has no CPU fallback")
        lib = _lib.load()
        self.staging_bytes = int(lib.sfh_jpeg_dec_staging_bytes(self.B, self.H, self.W, self.C, self.max_file_bytes))
        self.scratch_bytes = int(lib.sfh_jpeg_dec_scratch_bytes(self.B, self.H, self.W, self.C, self.max_file_bytes, self.subseq_bits))
        if self.staging_bytes < 0 or self.scratch_bytes < 0:
            raise ValueError(f"JpegDecoder: {self.B} files of {self.W}x{self.H}x{self.C}, at most {self.max_file_bytes} bytes each, "
                             f"subsequences of {self.subseq_bits} bits (a multiple of 32): refused, or buffers of 2 GiB or more")
        self.staging = torch.empty(self.staging_bytes, dtype=torch.uint8).pin_memory()
        self.staged = torch.empty(self.staging_bytes, dtype=torch.uint8, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        shape = (self.B, self.H, self.W) + ((3,) if self.C == 3 else ())
        self.out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._rounds = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._uploaded = None                     # event behind the last copy out of the staging buffer
        self._used = self._n = 0
        self._hsamp = 1

    # ---- the three steps of decode(), apart for callers that upload on a stream of their own (FramePipeline.submit_jpeg)

    def stage(self, files):
        """host only: parse the files and pack them into the pinned staging buffer -> number of files.  Waits for the copy of
        the previous batch out of that buffer; raises for a refused file, with nothing launched."""
        if isinstance(files, JpegBatch):
            files = files.to_host()
        files = [_as_bytes_array(f, "JpegDecoder") for f in files]
        n = len(files)
        if not 1 <= n <= self.B:
            raise ValueError(f"JpegDecoder: {n} files (1 .. {self.B})")
        if self._uploaded is not None:
            self._uploaded.synchronize()
            self._uploaded = None
        ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in files])
        sizes = (ctypes.c_int64 * n)(*[f.size for f in files])
        reason, index = ctypes.c_int32(0), ctypes.c_int32(-1)
        used = _lib.load().sfh_jpeg_dec_stage(ptrs, sizes, n, self.H, self.W, self.C, self.max_file_bytes, self.subseq_bits,
                                              ctypes.c_void_p(self.staging.data_ptr()), self.staging_bytes, ctypes.byref(reason),
                                              ctypes.byref(index))
        if used < 0:
            self._n = 0
            if reason.value:
                _refuse(reason.value, "JpegDecoder", index.value)
            _lib.check(-1, "jpeg_dec_stage")
        self._used, self._n = int(used), n
        self._hsamp = int(self.staging[20:24].view(torch.int32)[0])
        return n

    def upload(self):
        """the staged batch -> the device, one non-blocking copy on the current stream"""
        if self._n == 0:
            raise RuntimeError("JpegDecoder.upload: stage() a batch first")
        self.staged[:self._used].copy_(self.staging[:self._used], non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))

    def _checked_out(self, out, n):
        want = (n, self.H, self.W) + ((3,) if self.C == 3 else ())
        if not isinstance(out, torch.Tensor):
            raise ValueError(f"JpegDecoder: out: expected a tensor, got {type(out).__name__}")
        if out.dtype != torch.uint8:
            raise ValueError(f"JpegDecoder: out: dtype {out.dtype} (uint8 only)")
        if tuple(out.shape[1:]) != want[1:] or out.dim() != len(want) or out.shape[0] < n:
            raise ValueError(f"JpegDecoder: out: expected ({n}+,{','.join(map(str, want[1:]))}), got {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError("JpegDecoder: out: expected a contiguous tensor")
        if out.device != self.staged.device:
            raise RuntimeError(f"JpegDecoder: out on {out.device}, the decoder on {self.staged.device}")
        return out

    def decode_staged(self, out=None):
        """the uploaded batch -> frames (n,H,W[,3]), five launches and one memset on the current stream"""
        n = self._n
        if n == 0:
            raise RuntimeError("JpegDecoder.decode_staged: stage() and upload() a batch first")
        out = self.out if out is None else self._checked_out(out, n)
        lib = _lib.load()
        dev = self.device
        with torch.cuda.device(dev):
            _lib.check(lib.sfh_jpeg_entropy_decode(ctypes.c_void_p(self.staging.data_ptr()), _ptr(self.staged), self.staging_bytes, n,
                                                   self.H, self.W, self.C, self.max_file_bytes, self.subseq_bits, _ptr(self.scratch),
                                                   self.scratch_bytes, _stream(dev)), "jpeg_entropy_decode")
            _lib.check(lib.sfh_jpeg_decode_pixels(_ptr(self.staged), n, self.H, self.W, self.C, self._hsamp, int(self.bgr),
                                                  self.max_file_bytes, self.subseq_bits, _ptr(self.scratch), self.scratch_bytes,
                                                  _ptr(out), _ptr(self._status), _ptr(self._rounds), _stream(dev)),
                       "jpeg_decode_pixels")
        return out[:n]

    def decode(self, files, out=None):
        """files: a list of b <= batch files (bytes or 1-D uint8 arrays) or a JpegBatch -> uint8 (b,H,W[,3]) frames on the GPU.
        out: a contiguous uint8 tensor of that shape (or with more images) to decode into.  Everything wrong with the files'
        headers or with ``out`` raises before anything is launched."""
        if out is not None:
            n = len(files.sizes) if isinstance(files, JpegBatch) else len(files)
            self._checked_out(out, n)
        self.stage(files)
        self.upload()
        return self.decode_staged(out)

    @property
    def status(self):
        """int32 (b) of the last call: 0, or the OR of 1 (no such code), 2 (a run past coefficient 63), 4 (the bits end early),
        8 (blocks left over) over the image's segments - such an image came back as zeros.  Synchronises."""
        return self._status[:self._n].cpu().numpy()

    def rounds(self):
        """the largest number of rounds the fixed-point iteration took in a segment of the last call.  Synchronises."""
        return int(self._rounds[:self._n].max().item()) if self._n else 0


def decode_jpeg_device(file_or_files, bgr=True, device="cuda"):
    """One-off: one file (bytes or a 1-D uint8 array) -> a uint8 GPU tensor (H,W,3) or (H,W); a list of files or a JpegBatch
    -> (B,H,W[,3]).  The size and the channels are read from the first file.  Raises RuntimeError when an image has a status."""
    single = isinstance(file_or_files, (bytes, bytearray, memoryview, np.ndarray))
    files = [file_or_files] if single else (file_or_files.to_host() if isinstance(file_or_files, JpegBatch) else list(file_or_files))
    if not files:
        raise ValueError("decode_jpeg_device: no files")
    head = parse_jpeg(files[0])
    dec = JpegDecoder(head["height"], head["width"], head["ncomp"], len(files), bgr=bgr,
                      max_file_bytes=max(max(len(f) for f in files), 4), device=device)
    frames = dec.decode(files)
    if dec.status.any():
        raise RuntimeError(f"decode_jpeg_device: corrupt entropy-coded data, status {dec.status.tolist()}")
    return frames[0] if single else frames


def frames_from_files(files, device, bgr=True):
    """the ``frames_format="jpeg"`` switch of the host drivers (visualize, rectify_game): an iterable of file bytes -> uint8
    frames (B,H,W,3) on the GPU"""
    files = list(files)
    frames = decode_jpeg_device(files, bgr=bgr, device=device)
    if frames.dim() != 4:
        raise ValueError("frames_format='jpeg': the drivers need 3-channel frames, these files are gray")
    return frames
