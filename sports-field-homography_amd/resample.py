"""Pillow's image resize on the device: the step between "decoded image" and "tensor the model takes" on the reference's
image-directory path (``BasicDataset``, utils/dataset.py:146-185; ``test.py``; ``predict.py --img_dir``), which resizes with PIL
and not with OpenCV.

    r = Resampler((720, 1280), (360, 640))        # (H, W) -> (H, W), bicubic: Image.resize(size)'s default filter
    x = r.to_input(frames_u8)                     # uint8 (B,720,1280,3) on the GPU -> float32 (B,3,360,640) = resized bytes / 255
    small = r.resize(frames_u8)                   # -> uint8 (B,360,640,3): the bytes Image.resize gives
    masks = resize_nearest(mask_u8, (360, 640), rule="pil")       # Image.resize(.., Image.NEAREST)
    uv = resize_nearest(uv_u16, (360, 640), rule="cv2")           # cv2.resize(.., interpolation=cv2.INTER_NEAREST)

The bytes are Pillow's, which tests/test_resample_host.py pins through the numpy restatement ``tests/resample_ref.py``: per axis a
table of 22-bit fixed-point coefficients computed in fp64 on the host (``sfh_resample_tab``, cached on the device per size pair), a
horizontal pass into a uint8 intermediate that lives in LDS, then a vertical pass, integer arithmetic throughout
(``csrc/resample.hip``).  One launch per call, on the caller's current stream, with no synchronisation, no atomics and no stock
torch kernel.

Stated deviations: BOX, BILINEAR and BICUBIC only (LANCZOS and HAMMING take their coefficients from libm's sin / cos, which cannot
be pinned to the byte); no ``box=`` and no ``reducing_gap``; the filters take uint8 L / RGB images only; files are not decoded on
the device; an output index may have at most ``MAX_TAPS`` coefficients (bicubic: downscales up to 16x) - a size pair beyond that is
refused with ``NotImplementedError`` and nothing is launched.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._codec import ptr as _ptr, stream as _stream

FILTERS = {f: _lib.ABI.defines["SFH_FILTER_" + f.upper()] for f in ("box", "bilinear", "bicubic")}     # Pillow's numbering
NEAREST_RULES = {r: _lib.ABI.defines["SFH_NEAREST_" + r.upper()] for r in ("pil", "cv2")}
MAX_TAPS = _lib.ABI.defines["SFH_RESAMPLE_MAX_TAPS"]

_TABS = {}
_NEAREST_TABS = {}


def _filter_code(name):
    if name not in FILTERS:
        raise ValueError(f"filter {name!r} (one of {sorted(FILTERS)}; LANCZOS and HAMMING are not on the HIP path)")
    return FILTERS[name]


def axis_table(insize, outsize, filter="bicubic"):
    """host arrays of one axis: (bounds int32 (out, 2) = (xmin, n), coef int32 (out, ksize), ksize) - sfh_resample_tab, no device"""
    insize, outsize, code = int(insize), int(outsize), _filter_code(filter)
    if insize < 1 or outsize < 1:
        raise ValueError(f"resample table {insize} -> {outsize}: sizes must be positive")
    lib = _lib.load()
    scale = max(insize / outsize, 1.0)
    ksize = int(np.ceil({4: 0.5, 2: 1.0, 3: 2.0}[code] * scale)) * 2 + 1
    bounds = np.zeros((outsize, 2), np.int32)
    coef = np.zeros((outsize, ksize), np.int32)
    got = lib.sfh_resample_tab(insize, outsize, code, bounds.ctypes.data_as(ctypes.c_void_p), coef.ctypes.data_as(ctypes.c_void_p),
                               coef.size)
    if got != ksize:
        raise ValueError(f"no resample table for {insize} -> {outsize} ({filter})")
    return bounds, coef, ksize


def _check_taps(insize, outsize, filter, bounds):
    taps = int(bounds[:, 1].max())
    if taps > MAX_TAPS:
        raise NotImplementedError(f"GPU resize {insize} -> {outsize} ({filter}) needs {taps} coefficients per output index; the "
                                  f"HIP path is bounded at {MAX_TAPS} (SFH_RESAMPLE_MAX_TAPS)")
    return taps


def _axis_tab(insize, outsize, filter, device):
    """device copies of one axis' table, cached per (size pair, filter, device): (bounds, coef, ksize, taps, tile_rows)"""
    key = (insize, outsize, filter, str(device))
    t = _TABS.get(key)
    if t is None:
        bounds, coef, ksize = axis_table(insize, outsize, filter)
        taps = _check_taps(insize, outsize, filter, bounds)
        rows = _lib.load().sfh_resample_tile_rows(insize, outsize, FILTERS[filter])
        if rows < 1:
            raise NotImplementedError(f"GPU resize {insize} -> {outsize} ({filter}): beyond the bound of {MAX_TAPS} coefficients")
        t = _TABS[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coef).to(device), ksize, taps, rows)
    return t


def nearest_table(insize, outsize, rule="pil"):
    """host int32 array (out): the source index of every output index (sfh_nearest_tab, no device).  "pil": Image.resize(..,
    NEAREST)'s running fp64 sum; "cv2": cv2.INTER_NEAREST's min(floor(i * (1 / (out / in))), in - 1)"""
    if rule not in NEAREST_RULES:
        raise ValueError(f'rule {rule!r} ("pil" or "cv2")')
    insize, outsize = int(insize), int(outsize)
    if insize < 1 or outsize < 1:
        raise ValueError(f"nearest table {insize} -> {outsize}: sizes must be positive")
    idx = np.zeros(outsize, np.int32)
    if _lib.load().sfh_nearest_tab(insize, outsize, NEAREST_RULES[rule], idx.ctypes.data_as(ctypes.c_void_p), outsize) != outsize:
        raise ValueError(f"no nearest table for {insize} -> {outsize}")
    return idx


def _nearest_tab(insize, outsize, rule, device):
    key = (insize, outsize, rule, str(device))
    t = _NEAREST_TABS.get(key)
    if t is None:
        t = _NEAREST_TABS[key] = torch.from_numpy(nearest_table(insize, outsize, rule)).to(device)
    return t


def _hw(hw, what):
    try:
        h, w = int(hw[0]), int(hw[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"{what}: expected (H, W), got {hw!r}") from None
    if len(hw) != 2 or h < 1 or w < 1:
        raise ValueError(f"{what}: expected positive (H, W), got {hw!r}")
    return h, w


class Resampler:
    """``Image.resize((W, H), filter)`` for batches of uint8 frames of one size: src_hw = (H, W) of the frames, dst_hw = (H, W)
    of the result, channels 1 (L) or 3 (RGB; the channel order does not matter to the filter).  The tables are built here -
    on the host, nothing is launched - and uploaded at the first call."""

    def __init__(self, src_hw, dst_hw, channels=3, filter="bicubic"):
        self.src_hw, self.dst_hw = _hw(src_hw, "src_hw"), _hw(dst_hw, "dst_hw")
        self.C = int(channels)
        if self.C not in (1, 3):
            raise ValueError(f"Resampler: {channels} channels (1 or 3)")
        self.filter = filter
        _filter_code(filter)
        # refuse a size pair beyond the bound now, not at the first batch
        for i, o in zip(self.src_hw, self.dst_hw):
            if i != o:
                _check_taps(i, o, filter, axis_table(i, o, filter)[0])

    def _checked(self, frames):
        (hs, ws), C = self.src_hw, self.C
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise ValueError(f"Resampler: expected a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
        if frames.device.type != "cuda":
            raise ValueError(f"Resampler: tensor on {frames.device} - the HIP path needs a GPU tensor (there is no CPU fallback)")
        shape = tuple(frames.shape)
        if not (shape[1:] == (hs, ws, C) and len(shape) == 4) and not (C == 1 and len(shape) == 3 and shape[1:] == (hs, ws)):
            raise ValueError(f"Resampler: expected (B,{hs},{ws},{C}), got {shape}")
        if shape[0] < 1 or shape[0] > 65535:
            raise ValueError(f"Resampler: batch {shape[0]} (1 .. 65535)")
        if not frames.is_contiguous():
            raise ValueError("Resampler: expected a contiguous tensor (a strided, transposed or expanded view is refused)")
        return shape[0]

    def _run(self, frames, want_u8, want_f32):
        B = self._checked(frames)
        (hs, ws), (hd, wd), C = self.src_hw, self.dst_hw, self.C
        dev = frames.device
        u8 = torch.empty((B, hd, wd, C) if frames.dim() == 4 else (B, hd, wd), dtype=torch.uint8, device=dev) if want_u8 else None
        f32 = torch.empty((B, C, hd, wd), dtype=torch.float32, device=dev) if want_f32 else None
        with torch.cuda.device(dev):
            xb = xk = yb = yk = None
            xs = xt = ys = yt = 0
            rows = 16
            if ws != wd:
                xb, xk, xs, xt, _ = _axis_tab(ws, wd, self.filter, dev)
            if hs != hd:
                yb, yk, ys, yt, rows = _axis_tab(hs, hd, self.filter, dev)
            _lib.check(_lib.load().sfh_resample_u8(_ptr(frames), _ptr(u8), _ptr(f32), B, C, hs, ws, hd, wd, _ptr(xb), _ptr(xk), xs, xt,
                                                   _ptr(yb), _ptr(yk), ys, yt, rows, _stream(dev)), "resample_u8")
        return u8, f32

    def resize(self, frames_u8):
        """uint8 (B,H,W,C) (or (B,H,W) with channels=1) on the GPU -> uint8 of the same layout at dst_hw: Image.resize's bytes"""
        return self._run(frames_u8, True, False)[0]

    def to_input(self, frames_u8):
        """-> float32 (B,C,H,W) = resized bytes / 255: what ``ops.frames_u8_to_input`` makes of ``resize``'s result, bit for bit"""
        return self._run(frames_u8, False, True)[1]

    def both(self, frames_u8):
        """-> (uint8 frames, float32 input) from one launch"""
        return self._run(frames_u8, True, True)


_RESAMPLERS = {}


def resampler(src_hw, dst_hw, channels=3, filter="bicubic"):
    """the Resampler of a size pair, built once per process"""
    key = (tuple(src_hw), tuple(dst_hw), int(channels), filter)
    r = _RESAMPLERS.get(key)
    if r is None:
        r = _RESAMPLERS[key] = Resampler(src_hw, dst_hw, channels, filter)
    return r


def resize_nearest(t, dst_hw, rule="pil"):
    """nearest resize of a batch on the GPU: t uint8 (B,H,W) | (B,H,W,1) | (B,H,W,3) or uint16 (B,H,W,3) (the UV label) -> the same
    layout at dst_hw = (H, W).  rule "pil": Image.resize(.., Image.NEAREST) (preprocess_mask); "cv2": cv2.INTER_NEAREST
    (preprocess_uv_mask).  One launch."""
    if rule not in NEAREST_RULES:
        raise ValueError(f'resize_nearest: rule {rule!r} ("pil" or "cv2")')
    hd, wd = _hw(dst_hw, "dst_hw")
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"resize_nearest: expected a uint8 or uint16 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.device.type != "cuda":
        raise ValueError(f"resize_nearest: tensor on {t.device} - the HIP path needs a GPU tensor (there is no CPU fallback)")
    if t.dim() not in (3, 4) or t.numel() == 0:
        raise ValueError(f"resize_nearest: expected (B,H,W) or (B,H,W,C), got {tuple(t.shape)}")
    C = 1 if t.dim() == 3 else int(t.shape[3])
    if (t.dtype == torch.uint8 and C not in (1, 3)) or (t.dtype == torch.uint16 and (C != 3 or t.dim() != 4)):
        raise ValueError(f"resize_nearest: {t.dtype} with {C} channels (uint8 with 1 or 3 channels, uint16 with 3)")
    if not t.is_contiguous():
        raise ValueError("resize_nearest: expected a contiguous tensor")
    B, hs, ws = (int(v) for v in t.shape[:3])
    if B > 65535 or hd > 65535:
        raise ValueError(f"resize_nearest: batch {B} and {hd} rows (at most 65535 each)")
    dev = t.device
    out = torch.empty((B, hd, wd) + tuple(t.shape[3:]), dtype=t.dtype, device=dev)
    with torch.cuda.device(dev):
        yi, xi = _nearest_tab(hs, hd, rule, dev), _nearest_tab(ws, wd, rule, dev)
        _lib.check(_lib.load().sfh_resize_gather(_ptr(t), _ptr(out), B, C, t.element_size(), hs, ws, hd, wd, _ptr(yi), _ptr(xi),
                                                 _stream(dev)), "resize_gather")
    return out


def _one_call(frames_u8, size, filter):
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() not in (3, 4):
        raise ValueError("expected a uint8 (B,H,W,C) or (B,H,W) tensor on the GPU")
    C = 1 if frames_u8.dim() == 3 else int(frames_u8.shape[3])
    return resampler(tuple(int(v) for v in frames_u8.shape[1:3]), (int(size[1]), int(size[0])), C, filter)


def pil_resize_device(frames_u8, size, filter="bicubic"):
    """``[Image.fromarray(f).resize(size, filter) for f in frames]`` on the GPU; size = (W, H) as PIL takes it"""
    return _one_call(frames_u8, size, filter).resize(frames_u8)


def pil_resize_to_input(frames_u8, size, filter="bicubic"):
    """``BasicDataset.preprocess_img`` (utils/dataset.py:146-161) for a batch on the GPU: resize to size = (W, H), HWC -> CHW,
    / 255 -> float32 (B,C,H,W)"""
    return _one_call(frames_u8, size, filter).to_input(frames_u8)
