"""The frame the four image codecs (pngenc, jpegenc, pngdec, jpegdec) share; DESIGN.md, "The codecs' common frame".

Encoder side: ``BatchEncoder`` - images -> fixed-stride slots + a meta record per slot (launch 1) -> the files packed into a
``PngBatch`` / ``JpegBatch`` (launch 2).  Decoder side: ``BatchDecoder`` - the host parses the files into ONE pinned staging
buffer (``stage``), one non-blocking copy takes it to the device (``upload``), the launches read it there (``decode_staged``);
every image has a status word.  A codec module supplies its names, its refusal reasons and its ctypes calls.  The TIFF codec
(tiffenc, tiffdec) stands on the same frame; its samples are uint8 or uint16 (``SAMPLE``).
"""
import ctypes

import numpy as np
import torch

from . import _lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream(dev):
    """the caller's current stream on ``dev`` (``ops._stream()`` is the thread-local stream stack of the network, another thing)"""
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


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


class JpegBatch(PngBatch):
    """the encoded files of one batch on the device: ``data`` uint8, file b = data[offsets[b] : offsets[b] + sizes[b]];
    ``to_host()`` -> list of B 1-D uint8 numpy arrays (synchronises)"""


class TiffBatch(PngBatch):
    """the encoded files of one batch on the device: ``data`` uint8, file b = data[offsets[b] : offsets[b] + sizes[b]];
    ``to_host()`` -> list of B 1-D uint8 numpy arrays (synchronises)"""


def _dtype_name(dtype):
    return str(dtype).split(".")[-1]


def as_image_batch(t, who, dtypes=(torch.uint8,)):
    """how the one-off entry points read a tensor -> (batch tensor, channels, whether it was ONE image): a 2-D tensor and a 3-D
    tensor whose last dimension is 3 are one image, any other 3-D tensor a batch of gray images, a 4-D tensor (B,H,W,1|3) a
    batch"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: expected a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise ValueError(f"{who}: dtype {t.dtype} ({' or '.join(_dtype_name(d) for d in dtypes)} only)")
    single = t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)
    batch = t[None] if single else t
    if batch.dim() == 3:
        return batch, 1, single
    if batch.dim() == 4 and batch.shape[3] in (1, 3):
        return batch, int(batch.shape[3]), single
    raise ValueError(f"{who}: shape {tuple(t.shape)}")


def _cuda_device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: device {device} - the HIP path has no CPU fallback")
    return device


class BatchEncoder:
    """what the device encoders (PngEncoder, JpegEncoder) share: the constructor, the scratch and output buffers, the refusals
    of ``encode``'s argument and the partial-batch slice.  A subclass sets ``batch_type``, ``capacity_of(H, W, C)`` and
    ``scratch_bytes_of(lib)``, and launches in ``_launch(images, b, out, dev)``.  ``SAMPLE``: the dtype of the images' samples
    (TiffEncoder sets it per instance: uint8 or uint16)."""
    batch_type = PngBatch
    SAMPLE = torch.uint8

    def __init__(self, H, W, channels, batch, bgr, compact, device):
        who = type(self).__name__
        self.H, self.W, self.C, self.B = int(H), int(W), int(channels), int(batch)
        if self.B < 1:
            raise ValueError(f"{who}: batch {batch}")
        self.capacity = self.capacity_of(self.H, self.W, self.C)
        self.bgr, self.compact = bool(bgr), bool(compact)
        self.device = _cuda_device(device, who)
        self.scratch_bytes = int(self.scratch_bytes_of(_lib.load()))
        # a PNG scratch is below 1.7 capacity * B, so the 4 GiB bound only ever refuses a JPEG batch
        if self.scratch_bytes < 0 or self.scratch_bytes >= 2 ** 32 or self.capacity * self.B >= 2 ** 31:
            raise ValueError(f"{who}: {self.B} images of {self.W}x{self.H}x{self.C}: encoded batch of 2 GiB or more")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self.out = self.new_output()

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
        if images.dtype != self.SAMPLE:
            raise ValueError(f"{who}: dtype {images.dtype} ({_dtype_name(self.SAMPLE)} only)")
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

    def encode(self, images_u8, out=None):
        """images_u8: uint8 (b,H,W[,3]) on the GPU, b <= batch -> ``batch_type`` (of b files: offsets[:b+1], sizes[:b]); two
        launches on the current stream"""
        b = self._checked(images_u8)
        out = self.out if out is None else out
        dev = images_u8.device
        with torch.cuda.device(dev):
            self._launch(images_u8, b, out, dev)
        if b == self.B:
            return out
        return self.batch_type(out.data, out.offsets[:b + 1], out.sizes[:b])


def refuse(reasons, reason, who, index=None):
    """a host refusal (the codec's REASONS) as an exception: codes from 100 on name a feature that is not built"""
    what = reasons.get(int(reason), f"reason {reason}")
    where = "" if index is None or index < 0 else f" (file {index})"
    if reason >= 100:
        raise NotImplementedError(f"{who}: {what} is not built{where}")
    raise ValueError(f"{who}: {what}{where}")


def as_bytes_array(f, who):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return np.frombuffer(f, dtype=np.uint8)
    a = np.asarray(f)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError(f"{who}: a file is bytes or a 1-D uint8 array, not {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


class BatchDecoder:
    """what the device decoders (PngDecoder, JpegDecoder) share: the constructor's refusals, the pinned staging buffer, its
    device copy, the scratch, the images and the status words - every buffer is allocated once - and the three steps of
    ``decode``, apart for callers that upload on a stream of their own (FramePipeline.submit_jpeg).

    A subclass sets ``NAME`` (of its C entry points), ``REASONS``, ``CHANNELS``, ``LIMITS`` (the words of the shape refusal),
    ``MAX_SIDE``, ``batch_type`` (the device file batch ``decode`` takes), ``default_max_file_bytes(H, W, C)``, ``_sizes(lib)``
    -> (staging bytes, scratch bytes), ``_stage(lib, ptrs, sizes, n, reason, index)`` -> staged bytes, ``_launch(lib, n, out,
    dev)``, and for ``decode_once`` ``MIN_FILE_BYTES``, ``CORRUPT`` and ``_head(file)`` -> (H, W, channels).  ``SAMPLE``: the
    dtype of the images' samples (TiffDecoder sets it per instance: uint8 or uint16)."""
    MAX_SIDE = None
    SAMPLE = torch.uint8
    _sizes_detail = ""

    def __init__(self, H, W, channels, batch, bgr, max_file_bytes, device):
        who = type(self).__name__
        self.H, self.W, self.C, self.B = int(H), int(W), int(channels), int(batch)
        if self.B < 1:
            raise ValueError(f"{who}: batch {batch}")
        side = self.MAX_SIDE
        if self.C not in self.CHANNELS or self.H < 1 or self.W < 1 or (side and (self.H > side or self.W > side)):
            raise ValueError(f"{who}: image {self.W}x{self.H}x{self.C} ({self.LIMITS})")
        self.max_file_bytes = self.default_max_file_bytes(self.H, self.W, self.C) if max_file_bytes is None else int(max_file_bytes)
        self.bgr = bool(bgr)
        self.device = _cuda_device(device, who)
        self.staging_bytes, self.scratch_bytes = (int(v) for v in self._sizes(_lib.load()))
        if self.staging_bytes < 0 or self.scratch_bytes < 0:
            raise ValueError(f"{who}: {self.B} files of {self.W}x{self.H}x{self.C}, at most {self.max_file_bytes} bytes each"
                             f"{self._sizes_detail}: refused, or buffers of 2 GiB or more")
        self.staging = torch.empty(self.staging_bytes, dtype=torch.uint8).pin_memory()
        self.staged = torch.empty(self.staging_bytes, dtype=torch.uint8, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self.out = torch.empty(self._shape(self.B), dtype=self.SAMPLE, device=self.device)
        self._status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._uploaded = None                     # event behind the last copy out of the staging buffer
        self._used = self._n = 0

    def _shape(self, n):
        return (n, self.H, self.W) + ((self.C,) if self.C > 1 else ())

    def stage(self, files):
        """host only: parse the files and pack them into the pinned staging buffer -> number of files.  Waits for the copy of
        the previous batch out of that buffer; raises for a refused file, with nothing launched."""
        who = type(self).__name__
        if isinstance(files, self.batch_type):
            files = files.to_host()
        files = [as_bytes_array(f, who) for f in files]
        n = len(files)
        if not 1 <= n <= self.B:
            raise ValueError(f"{who}: {n} files (1 .. {self.B})")
        if self._uploaded is not None:
            self._uploaded.synchronize()
            self._uploaded = None
        ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in files])
        sizes = (ctypes.c_int64 * n)(*[f.size for f in files])
        reason, index = ctypes.c_int32(0), ctypes.c_int32(-1)
        used = self._stage(_lib.load(), ptrs, sizes, n, ctypes.byref(reason), ctypes.byref(index))
        if used < 0:
            self._n = 0
            if reason.value:
                refuse(self.REASONS, reason.value, who, index.value)
            _lib.check(-1, f"{self.NAME}_dec_stage")
        self._used, self._n = int(used), n
        return n

    def upload(self):
        """the staged batch -> the device, one non-blocking copy on the current stream"""
        if self._n == 0:
            raise RuntimeError(f"{type(self).__name__}.upload: stage() a batch first")
        self.staged[:self._used].copy_(self.staging[:self._used], non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))

    def _checked_out(self, out, n):
        who = type(self).__name__
        want = self._shape(n)
        if not isinstance(out, torch.Tensor):
            raise ValueError(f"{who}: out: expected a tensor, got {type(out).__name__}")
        if out.dtype != self.SAMPLE:
            raise ValueError(f"{who}: out: dtype {out.dtype} ({_dtype_name(self.SAMPLE)} only)")
        if tuple(out.shape[1:]) != want[1:] or out.dim() != len(want) or out.shape[0] < n:
            raise ValueError(f"{who}: out: expected ({n}+,{','.join(map(str, want[1:]))}), got {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError(f"{who}: out: expected a contiguous tensor")
        if out.device != self.staged.device:
            raise RuntimeError(f"{who}: out on {out.device}, the decoder on {self.staged.device}")
        return out

    def decode_staged(self, out=None):
        """the uploaded batch -> images (n,H,W[,C]): the codec's launches on the current stream"""
        n = self._n
        if n == 0:
            raise RuntimeError(f"{type(self).__name__}.decode_staged: stage() and upload() a batch first")
        out = self.out if out is None else self._checked_out(out, n)
        with torch.cuda.device(self.device):
            self._launch(_lib.load(), n, out, self.device)
        return out[:n]

    def decode(self, files, out=None):
        """files: a list of b <= batch files (bytes or 1-D uint8 arrays) or a ``batch_type`` -> uint8 (b,H,W[,C]) images on the
        GPU.  out: a contiguous uint8 tensor of that shape (or with more images) to decode into.  Everything wrong with the
        files' headers or with ``out`` raises before anything is launched."""
        if out is not None:
            n = len(files.sizes) if isinstance(files, self.batch_type) else len(files)
            self._checked_out(out, n)
        self.stage(files)
        self.upload()
        return self.decode_staged(out)

    @property
    def status(self):
        """int32 (b) of the last call: 0, or the OR of the codec's status bits (the class's docstring) - such an image came
        back as zeros.  Synchronises."""
        return self._status[:self._n].cpu().numpy()


    @classmethod
    def decode_once(cls, who, file_or_files, **kw):
        """the one-off decode: one file (bytes or a 1-D uint8 array) -> one image; a list of files or a ``batch_type`` ->
        (B,H,W[,C]).  The size and the channels are read from the first file.  Raises RuntimeError when an image has a status."""
        single = isinstance(file_or_files, (bytes, bytearray, memoryview, np.ndarray))
        if single:
            files = [file_or_files]
        else:
            files = file_or_files.to_host() if isinstance(file_or_files, cls.batch_type) else list(file_or_files)
        if not files:
            raise ValueError(f"{who}: no files")
        H, W, C = cls._head(files[0])
        dec = cls(H, W, C, len(files), max_file_bytes=max(max(len(f) for f in files), cls.MIN_FILE_BYTES), **kw)
        images = dec.decode(files)
        if dec.status.any():
            raise RuntimeError(f"{who}: corrupt {cls.CORRUPT} data, status {dec.status.tolist()}")
        return images[0] if single else images


def frames_from_files(files, device, frames_format, bgr=True):
    """the ``frames_format=`` switch of the host drivers (visualize, rectify_game): an iterable of "jpeg" or "png" file
    bytes -> uint8 frames (B,H,W,3) on the GPU"""
    from . import jpegdec, pngdec
    legs = {"jpeg": jpegdec, "png": pngdec}
    if frames_format not in legs:
        raise ValueError(f'frames_format={frames_format!r} ("jpeg" or "png")')
    return legs[frames_format].frames_from_files(files, device, bgr=bgr)


def image_files_from_batch(images, channels, where="host", image_format="png", jpeg_quality=90):
    """the ``image_format=`` / ``png=`` switches of the host drivers together -> (list of B files, file extension)"""
    from . import jpegenc, pngenc
    if image_format == "png":
        return pngenc.files_from_batch(images, channels, where), "png"
    if image_format == "jpeg":
        return jpegenc.jpeg_files_from_batch(images, channels, where, jpeg_quality), "jpeg"     # the reference's extension
    raise ValueError(f'image_format={image_format!r} ("png" or "jpeg")')
