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
from ._codec import BatchDecoder, JpegBatch, as_bytes_array, ptr, refuse, stream
from .jpegenc import jpeg_capacity

REASONS = {1: "the bytes end inside the header", 2: "no SOI marker: not a JPEG file", 3: "a marker out of place",
           4: "a malformed SOF0 segment", 5: "a malformed or missing DQT / DHT table", 6: "a malformed SOS segment",
           7: "restart markers out of sequence or not matching the restart interval",
           8: "size, channels or sampling other than the decoder's (or the batch's first file's)",
           9: "a file longer than the decoder's max_file_bytes",
           100: "progressive coding", 101: "arithmetic coding", 102: "12-bit samples", 103: "16-bit quantisation tables",
           104: "2 or 4 components (CMYK / YCCK)", 105: "RGB components", 106: "sampling other than 4:2:0 / 4:4:4 (4:2:2, 4:4:0, 4:1:1)",
           107: "a non-interleaved file (several scans)", 108: "DNL / height 0", 109: "extended sequential, lossless or hierarchical frames"}


HuffTab = _lib.ABI.structs["sfh_jpeg_hufftab"]
JpegInfo = _lib.ABI.structs["sfh_jpeg_info"]
assert ctypes.sizeof(JpegInfo) == 7920


def _tab(t):
    return {"look": np.array(t.look, dtype=np.int64), "maxcode": np.array(t.maxcode, dtype=np.int64),
            "valoff": np.array(t.valoff, dtype=np.int64), "vals": np.array(t.vals, dtype=np.int64)}


def parse_jpeg(data):
    """the host parse of one file as a dict (no device needed): sizes, sampling, table selectors, the quantisation tables in
    natural order, the Huffman tables in the lookup form the kernel reads, the scan's byte range, the restart interval and the
    segments [(first byte, end byte, first MCU)].  Raises what ``JpegDecoder.decode`` raises for a refused file."""
    a = as_bytes_array(data, "parse_jpeg")
    lib = _lib.load()
    info = JpegInfo()
    src = a.ctypes.data_as(ctypes.c_void_p)
    if lib.sfh_jpeg_parse(src, a.size, ctypes.byref(info), None, 0) != 0:
        refuse(REASONS, info.reason, "parse_jpeg")
    segs = np.zeros((info.nsegments, 4), dtype=np.int32)
    if lib.sfh_jpeg_parse(src, a.size, ctypes.byref(info), segs.ctypes.data_as(ctypes.c_void_p), info.nsegments) != 0:
        refuse(REASONS, info.reason, "parse_jpeg")
    nc = info.ncomp
    used = lambda sel: sorted(set(sel[:nc]))
    return {"width": info.width, "height": info.height, "ncomp": nc, "hsamp": info.hsamp, "vsamp": info.vsamp,
            "mcus_x": info.mcus_x, "mcus_y": info.mcus_y, "blocks_per_mcu": info.blocks_per_mcu,
            "restart_interval": info.restart_interval, "nsegments": info.nsegments, "scan_begin": info.scan_begin,
            "scan_end": info.scan_end, "qsel": list(info.qsel[:nc]), "dcsel": list(info.dcsel[:nc]), "acsel": list(info.acsel[:nc]),
            "quant": {q: np.array(info.quant[q], dtype=np.int64) for q in used(info.qsel)},
            "dc": {k: _tab(info.dc[k]) for k in used(info.dcsel)}, "ac": {k: _tab(info.ac[k]) for k in used(info.acsel)},
            "segments": [tuple(int(v) for v in s[:3]) for s in segs]}


HEAD_HSAMP = 5        # word of the staging buffer's head {magic, batch, largest segment count, subsequence bits, bytes, hsamp}


class JpegDecoder(BatchDecoder):
    """Decoder of batches of up to ``batch`` JFIF files of H x W pixels and ``channels`` (1 | 3) channels; owns the pinned staging
    buffer, its device copy, the scratch, the frames, ``status`` and the round counts - every buffer is allocated once, and the
    frames ``decode`` returns without ``out`` are valid until the next call.  bgr: 3-channel frames come out BGR in memory
    (cv2's convention, like the rest of the package); False for RGB.

    ``decode_staged``: five launches and one memset on the current stream.  ``status`` bits, over the image's segments: 1 (no
    such code), 2 (a run past coefficient 63), 4 (the bits end early), 8 (blocks left over)."""
    NAME, REASONS, batch_type = "jpeg", REASONS, JpegBatch
    CHANNELS, LIMITS, MAX_SIDE = (1, 3), "1 or 3 channels, at most 65535 a side", 65535
    MIN_FILE_BYTES, CORRUPT = 4, "entropy-coded"
    default_max_file_bytes = staticmethod(jpeg_capacity)

    def __init__(self, H, W, channels=3, batch=1, bgr=True, max_file_bytes=None, device="cuda", _subseq_bits=0):
        self.subseq_bits = int(_subseq_bits) if _subseq_bits else 1024    # tests: smaller ones reach many rounds on small files
        self._sizes_detail = f", subsequences of {self.subseq_bits} bits (a multiple of 32)"
        super().__init__(H, W, channels, batch, bgr, max_file_bytes, device)
        self._rounds = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._hsamp = 1

    def _sizes(self, lib):
        return (lib.sfh_jpeg_dec_staging_bytes(self.B, self.H, self.W, self.C, self.max_file_bytes),
                lib.sfh_jpeg_dec_scratch_bytes(self.B, self.H, self.W, self.C, self.max_file_bytes, self.subseq_bits))

    def _stage(self, lib, ptrs, sizes, n, reason, index):
        return lib.sfh_jpeg_dec_stage(ptrs, sizes, n, self.H, self.W, self.C, self.max_file_bytes, self.subseq_bits,
                                      ptr(self.staging), self.staging_bytes, reason, index)

    def stage(self, files):
        n = super().stage(files)
        self._hsamp = int(self.staging[:4 * (HEAD_HSAMP + 1)].view(torch.int32)[HEAD_HSAMP])
        return n

    def _launch(self, lib, n, out, dev):
        _lib.check(lib.sfh_jpeg_entropy_decode(ptr(self.staging), ptr(self.staged), self.staging_bytes, n, self.H, self.W, self.C,
                                               self.max_file_bytes, self.subseq_bits, ptr(self.scratch), self.scratch_bytes,
                                               stream(dev)), "jpeg_entropy_decode")
        _lib.check(lib.sfh_jpeg_decode_pixels(ptr(self.staged), n, self.H, self.W, self.C, self._hsamp, int(self.bgr),
                                              self.max_file_bytes, self.subseq_bits, ptr(self.scratch), self.scratch_bytes,
                                              ptr(out), ptr(self._status), ptr(self._rounds), stream(dev)), "jpeg_decode_pixels")

    @staticmethod
    def _head(f):
        head = parse_jpeg(f)
        return head["height"], head["width"], head["ncomp"]

    def rounds(self):
        """the largest number of rounds the fixed-point iteration took in a segment of the last call.  Synchronises."""
        return int(self._rounds[:self._n].max().item()) if self._n else 0


def decode_jpeg_device(file_or_files, bgr=True, device="cuda"):
    """One-off: one file (bytes or a 1-D uint8 array) -> a uint8 GPU tensor (H,W,3) or (H,W); a list of files or a JpegBatch
    -> (B,H,W[,3]).  The size and the channels are read from the first file.  Raises RuntimeError when an image has a status."""
    return JpegDecoder.decode_once("decode_jpeg_device", file_or_files, bgr=bgr, device=device)


def frames_from_files(files, device, bgr=True):
    """the ``frames_format="jpeg"`` switch of the host drivers (visualize, rectify_game): an iterable of file bytes -> uint8
    frames (B,H,W,3) on the GPU"""
    files = list(files)
    frames = decode_jpeg_device(files, bgr=bgr, device=device)
    if frames.dim() != 4:
        raise ValueError("frames_format='jpeg': the drivers need 3-channel frames, these files are gray")
    return frames
