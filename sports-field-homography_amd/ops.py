"""Host-side helpers around the C-ABI library: the launch stream, engine-build kernels (fill, |w| reductions, small vector
ops), the split activation formats and the thin layout / resize / POI / CE wrappers; all arithmetic is in ``libsfh_amd.so``."""
import ctypes
import math
import struct
import threading

import numpy as np
import torch

from . import _lib


# the HIP stream of the engine run() on this THREAD's stack (torch.cuda.current_stream() costs ~9 us per launch);
# thread-local: another thread's run() - another model, device or torch.cuda.stream() context - has its own
_STREAM_TLS = threading.local()


def _stream():
    stack = getattr(_STREAM_TLS, "stack", None)
    if stack:
        return stack[-1]
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _stream_scope:
    """Resolve the current HIP stream once for all launches of one engine run (of the calling thread)."""

    def __enter__(self):
        stack = getattr(_STREAM_TLS, "stack", None)
        if stack is None:
            stack = _STREAM_TLS.stack = []
        stack.append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def __exit__(self, *exc):
        _STREAM_TLS.stack.pop()
        return False


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float32 tensor, got {t.dtype} "
                         f"contiguous={t.is_contiguous()}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP path needs a GPU tensor "
                           "(there is no CPU fallback)")
    return t


# ---- engine-build helpers (csrc/hostprep.hip): the work around packing a checkpoint on this library's own kernels
def filled(shape, dtype, device, value=0):
    """torch.full / torch.zeros for 4-byte element types on this library's fill kernel"""
    t = torch.empty(shape, dtype=dtype, device=device)
    if t.element_size() != 4:
        raise ValueError("filled: 4-byte element types only")
    if t.numel():
        word = struct.unpack("<I", struct.pack("<f" if dtype.is_floating_point else "<i", value))[0]
        with torch.cuda.device(t.device):
            _lib.check(_lib.load().sfh_fill_words(_ptr(t), t.numel(), word, _stream()), "fill_words")
    return t


_ABSMAX_TABLES = {}


def absminmax_words(tensors):
    """device int32 tensor of 2 words per tensor (sfh_multi_absminmax: bits of max |x|, 0x7FFFFFFF - bits of min |x|), no
    read-back - for consumers that stay on the device (sfh_grad_scale)"""
    dev = tensors[0].device
    for t in tensors:
        _f32c(t, "absminmax operand")
    # the (address, size) table lives on the device; a blocking upload would synchronise the caller's stream, so the table of
    # a recurring set of tensors (a training step's gradient seeds come back at the same addresses) is uploaded once
    key = (str(dev),) + tuple((t.data_ptr(), t.numel()) for t in tensors)
    dtab = _ABSMAX_TABLES.get(key)
    if dtab is None:
        tab = np.array([(t.data_ptr(), t.numel()) for t in tensors], dtype=np.int64)
        dtab = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(dev)
        if len(_ABSMAX_TABLES) >= 16:
            _ABSMAX_TABLES.pop(next(iter(_ABSMAX_TABLES)))
        _ABSMAX_TABLES[key] = dtab
    words = filled((2 * len(tensors),), torch.int32, dev)
    _lib.check(_lib.load().sfh_multi_absminmax(_ptr(dtab), len(tensors), _ptr(words), _stream()), "multi_absminmax")
    return words


def absminmax(tensors):
    """[(max |x|, min |x|)] of float32 device tensors - ONE launch over all of them (sfh_multi_absminmax) and ONE
    read-back, where torch would run an abs + a reduction + a host sync per tensor.  A non-finite element gives inf / nan."""
    if not tensors:
        return []
    w = absminmax_words(tensors).cpu().numpy().view(np.uint32)
    mx = w[0::2].copy().view(np.float32)
    mn = (np.uint32(0x7FFFFFFF) - w[1::2]).astype(np.uint32).view(np.float32)
    return [(float(a), float(b)) for a, b in zip(mx, mn)]


def h2_weight_exp(wmax, top=14):
    """exponent e with max |w| * 2^e in [2^(top-1), 2^top) (include/sfh_amd.h, H2 weights); 0 for an all-zero tensor"""
    if not math.isfinite(wmax):
        raise ValueError("conv weight holds non-finite values")
    return max(-100, min(100, top - math.frexp(wmax)[1])) if wmax > 0 else 0


def resolve_wexp(w, wexp=None):
    """H2 exponent of weight tensor w: `wexp` from a caller that has the maximum already (one batched read-back for many
    layers), else one device read-back here; within the +-100 the packing kernels take"""
    return max(-100, min(100, int(wexp if wexp is not None else h2_weight_exp(absminmax([w])[0][0]))))


def weight_exps(tensors):
    """{data_ptr: h2_weight_exp} of float32 weight tensors: ONE |w| reduction over all of them and one read-back"""
    return {w.data_ptr(): h2_weight_exp(mx) for w, (mx, _) in zip(tensors, absminmax(tensors))}


def vec_op(a, b=None, op="scale", factor=1.0, out=None):
    """out = a * factor ("scale"), a / b ("div") or a * b * factor ("mul") on the HIP helper kernel; b is indexed modulo
    its length (a tiled operand); out may be a itself.  Small float32 vectors: a layer's folded scale / shift."""
    code = {"scale": 0, "div": 1, "mul": 2}[op]
    a = _f32c(a, "vec_op operand")
    if out is None:
        out = torch.empty_like(a)
    if b is not None:
        b = _f32c(b, "vec_op operand")
    _lib.check(_lib.load().sfh_vec_op(code, _ptr(a), _ptr(b) if b is not None else None, a.numel(), b.numel() if b is not None else 0,
                              float(factor), _ptr(out), _stream()), "vec_op")
    return out


def snapshot(t):
    """a private copy of a small float32 tensor (engines keep NO live reference to a parameter: load_state_dict writes
    parameters in place, and an engine that finishes batches in flight must still see the weights it was built from)"""
    return vec_op(_f32c(t.detach(), "snapshot operand"))


def rows_all_equal(t):
    """do all t[k] hold the bits of t[0]?  (4-byte elements, contiguous; one launch, one word read back)"""
    if t.shape[0] <= 1:
        return True
    if not t.is_contiguous() or t.element_size() != 4 or not t.is_cuda:
        raise ValueError("rows_all_equal: expected a contiguous GPU tensor of 4-byte elements")
    flag = filled((1,), torch.int32, t.device)
    _lib.check(_lib.load().sfh_rows_differ(_ptr(t), t[0].numel(), t.shape[0], _ptr(flag), _stream()), "rows_differ")
    return int(flag.cpu()[0]) == 0


def stn_input_assemble(logits, frame, uv, cs):
    """(B,H,W,cs) NHWC = cat((logits, frame, uv), 1) zero-padded (any of the three may be None): the ResNet-STN input of
    the modes the fused OutConv epilogue does not cover (models/reconstructor.py:174-183,214)"""
    srcs = [_f32c(t.contiguous(), "stn input source") if t is not None else None for t in (logits, frame, uv)]
    ref = next(t for t in srcs if t is not None)
    B, _, H, W = ref.shape
    for t in srcs:
        if t is not None and (t.shape[0], t.shape[2], t.shape[3]) != (B, H, W):
            raise ValueError("stn_input_assemble: sources of different batch / size")
    out = torch.empty((B, H, W, cs), dtype=torch.float32, device=ref.device)
    ch = [t.shape[1] if t is not None else 0 for t in srcs]
    _lib.check(_lib.load().sfh_stn_input_assemble(_ptr(srcs[0]), ch[0], _ptr(srcs[1]), ch[1], _ptr(srcs[2]), ch[2], B, H, W, cs,
                                                  _ptr(out), _stream()), "stn_input_assemble")
    return out


def slice_in_channels(w, c0, c1):
    """w[:, c0:c1] of an OIHW weight as a contiguous tensor (sfh_copy2d_words)"""
    w = _f32c(w.detach(), "conv weight")
    cout, cin, kh, kw = w.shape
    out = torch.empty((cout, c1 - c0, kh, kw), dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().sfh_copy2d_words(ctypes.c_void_p(w.data_ptr() + 4 * c0 * kh * kw), cin * kh * kw, _ptr(out),
                                    (c1 - c0) * kh * kw, (c1 - c0) * kh * kw, cout, _stream()), "copy2d_words")
    return out


# Split ("plane") activation formats of include/sfh_amd.h, identified by the tensor dtype:
#   "s3": (B,H,C/32,3,4,W,8) bfloat16 - three bf16 planes, exact fp32 value            (precision "bf16x6")
#   "h2": (B,H,C/32,2,4,W,8) float16  - two fp16 planes of v * 2^2, 22 significand bits (precision "f16x3")
_SPLIT = {"s3": (torch.bfloat16, 3, _lib.FMT_S3), "h2": (torch.float16, 2, _lib.FMT_H2)}
_SPLIT_DTYPES = {torch.bfloat16: "s3", torch.float16: "h2"}
PRECISIONS = {"bf16x6": "s3", "f16x3": "h2", "fp32": None}


def _fmt_of(t):
    """"s3" / "h2" for a split tensor, None for fp32 NHWC"""
    return _SPLIT_DTYPES.get(t.dtype)


def _fmt_code(t):
    f = _fmt_of(t)
    return _SPLIT[f][2] if f else _lib.FMT_F32


def _chan(t):
    """channels per pixel of an activation tensor: fp32 NHWC (B,H,W,C) or split (B,H,C/32,planes,4,W,8)"""
    return t.shape[2] * 32 if t.dtype in _SPLIT_DTYPES else t.shape[3]


def _hw(t):
    """(H, W) of an activation tensor in either format"""
    return (t.shape[1], t.shape[5]) if t.dtype in _SPLIT_DTYPES else (t.shape[1], t.shape[2])


def split_shape(fmt, b, h, w, c):
    if c % 32:
        raise ValueError(f"split-format tensors need a multiple of 32 channels, got {c}")
    return (b, h, c // 32, _SPLIT[fmt][1], 4, w, 8)


def s3_empty(b, h, w, c, device):
    """uninitialised split-bf16 activation tensor for c channels (c multiple of 32)"""
    return torch.empty(split_shape("s3", b, h, w, c), dtype=torch.bfloat16, device=device)


def _split_to_f32_into(t, out, exp=_lib.H2_ACT_EXP):
    """exp: exponent of an H2 tensor (ignored for S3)"""
    lib = _lib.load()
    B = t.shape[0]
    H, W = _hw(t)
    C = _chan(t)
    if tuple(out.shape) != (B, H, W, C) or out.dtype != torch.float32:
        raise ValueError(f"split_to_f32: destination {tuple(out.shape)} does not match {(B, H, W, C)}")
    if _fmt_of(t) == "h2":
        _lib.check(lib.sfh_h2_to_f32(_ptr(t), _ptr(out), B * H, W, C, int(exp), _stream()), "h2_to_f32")
    else:
        _lib.check(lib.sfh_s3_to_f32(_ptr(t), _ptr(out), B * H, W, C, _stream()), "s3_to_f32")
    return out


def _f32_to_split_into(t, out, overflow=None, exp=_lib.H2_ACT_EXP, range_word=None):
    """H2 destinations: exp = the tensor's exponent, overflow / range_word: optional device words (OR 1 on
    saturation / atomic max of |v * 2^exp|, see H2Ranges)"""
    lib = _lib.load()
    B, H, W, C = t.shape
    if (out.shape[0],) + _hw(out) + (_chan(out),) != (B, H, W, C):
        raise ValueError(f"f32_to_split: destination {tuple(out.shape)} does not match {(B, H, W, C)}")
    if _fmt_of(out) == "h2":
        _lib.check(lib.sfh_f32_to_h2(_ptr(t), _ptr(out), B * H, W, C, int(exp), _ptr(overflow),
                                     ctypes.c_void_p(range_word) if range_word else None, _stream()), "f32_to_h2")
    else:
        _lib.check(lib.sfh_f32_to_s3(_ptr(t), _ptr(out), B * H, W, C, _stream()), "f32_to_s3")
    return out


def s3_to_f32(t, exp=_lib.H2_ACT_EXP):
    """split tensor (S3: (B,H,C/32,3,4,W,8) bf16, exact sum of the planes; H2: (B,H,C/32,2,4,W,8) fp16 carrying
    v * 2^exp) -> (B,H,W,C) float32."""
    out = torch.empty((t.shape[0],) + _hw(t) + (_chan(t),), dtype=torch.float32, device=t.device)
    return _split_to_f32_into(t, out, exp)


def split_empty(fmt, b, h, w, c, device):
    """uninitialised split-format activation tensor ("s3" or "h2") for c channels (c multiple of 32)"""
    return torch.empty(split_shape(fmt, b, h, w, c), dtype=_SPLIT[fmt][0], device=device)


def f32_to_split(t, fmt, overflow=None, exp=_lib.H2_ACT_EXP):
    """(B,H,W,C) float32 -> split tensor of format "s3" or "h2" (h2: carrying v * 2^exp) """
    t = _f32c(t, "nhwc tensor")
    return _f32_to_split_into(t, split_empty(fmt, *t.shape, t.device), overflow, exp)


def f32_to_h2(t, overflow=None, exp=_lib.H2_ACT_EXP, range_word=None):
    """(B,H,W,C) float32 -> (B,H,C/32,2,4,W,8) fp16 two-plane tensor of v * 2^exp (include/sfh_amd.h, SFH_FMT_H2);
    range_word: an int32 tensor whose first word receives the largest bit pattern of |v * 2^exp|."""
    t = _f32c(t, "nhwc tensor")
    return _f32_to_split_into(t, split_empty("h2", *t.shape, t.device), overflow, exp,
                              range_word.data_ptr() if range_word is not None else None)


def f32_to_s3(t):
    """(B,H,W,C) float32 -> (B,H,C/32,3,4,W,8) bf16 split tensor."""
    return f32_to_split(t, "s3")


_AREA_TABS = {}


def _area_tab(ssize, dsize, device):
    """device copies of one axis' INTER_AREA table (sfh_resize_area_tab: OpenCV's computeResizeAreaTab), cached per size pair"""
    key = (ssize, dsize, str(device))
    t = _AREA_TABS.get(key)
    if t is None:
        cap = 2 * dsize + ssize
        ofs, si, al = np.zeros(dsize + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        n = _lib.load().sfh_resize_area_tab(ssize, dsize, ofs.ctypes.data_as(ctypes.c_void_p), si.ctypes.data_as(ctypes.c_void_p),
                                    al.ctypes.data_as(ctypes.c_void_p), cap)
        if n < 0:
            raise ValueError(f"no INTER_AREA table for {ssize} -> {dsize}")
        t = _AREA_TABS[key] = tuple(torch.from_numpy(a).to(device) for a in (ofs, si[:max(n, 1)].copy(), al[:max(n, 1)].copy()))
    return t


def frames_u8_to_input(frames_u8, target_size=None, resize="area"):
    """uint8 (B,H,W,C) decoded frames on the GPU -> float32 (B,C,H,W) in [0,1], bit-identical to the
    reference dataset's `img.transpose((2,0,1)) / 255` (utils/dataset.py:154-159).  target_size = (W, H):
    like VideoDataset.preprocess_img (utils/dataset.py:310-330) frames WIDER than the target are resized first with
    cv2.INTER_AREA's rules: the integer factors 2 .. 16 take OpenCV's block-average fast paths (1280x720 -> 640x360 is the
    2x2 special case, 1920x1080 -> 640x360 the 3x3 one), any other downscale (both factors >= 1, e.g. 1920x1080 -> 1024x576
    or 1600x900 -> 640x360) the generic area tables (round 5).  Frames narrower than the target (the reference switches to
    INTER_LINEAR there) are not on the HIP path.
    resize="pil": frames of another size are resized with Pillow's rule instead - `pil_img.resize(target_size)`, bicubic with
    antialiasing, BasicDataset.preprocess_img's (utils/dataset.py:146-161) - for any size pair within sfh_amd.resample's tap
    bound, upscales included."""
    if resize not in ("area", "pil"):
        raise ValueError(f'frames_u8_to_input: resize={resize!r} ("area" or "pil")')
    lib = _lib.load()
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_cuda:
        raise ValueError("expected a uint8 (B,H,W,C) tensor on the GPU")
    if resize == "pil" and target_size is not None and (int(target_size[0]), int(target_size[1])) != tuple(frames_u8.shape[2:0:-1]):
        from . import resample
        return resample.pil_resize_to_input(frames_u8.contiguous(), target_size)
    f = frames_u8.contiguous()
    B, H, W, C = f.shape
    if target_size is not None and (int(target_size[0]), int(target_size[1])) != (W, H):
        tw, th = int(target_size[0]), int(target_size[1])
        if tw <= 0 or th <= 0 or W <= tw or H < th:      # (W > tw: the reference's own test for INTER_AREA, utils/dataset.py:314)
            raise NotImplementedError(f"GPU frame resize {W}x{H} -> {tw}x{th}: only downscales (cv2.INTER_AREA, the reference's choice "
                                      "for frames wider than the target) are on the HIP path; resize on the host as utils/dataset.py does")
        out = torch.empty((B, C, th, tw), dtype=torch.float32, device=f.device)
        k = W // tw
        if 2 <= k <= 16 and (k * tw, k * th) == (W, H):
            _lib.check(lib.sfh_u8hwc_areak_to_f32nchw(_ptr(f), _ptr(out), B, C, th, tw, k, _stream()), "u8hwc_areak_to_f32nchw")
            return out
        if (tw * (W // tw), th * (H // th)) == (W, H):
            # integer factors that differ per axis, or beyond 16: OpenCV's resizeAreaFast_ with a kx x ky block
            kx, ky = W // tw, H // th
            if kx > 64 or ky > 64:
                raise NotImplementedError(f"GPU frame resize {W}x{H} -> {tw}x{th}: integer factors beyond 64 are not on the HIP path")
            _lib.check(lib.sfh_u8hwc_areaxy_to_f32nchw(_ptr(f), _ptr(out), B, C, th, tw, kx, ky, _stream()), "u8hwc_areaxy_to_f32nchw")
            return out
        xo, xs, xa = _area_tab(W, tw, f.device)
        yo, ys, yb = _area_tab(H, th, f.device)
        _lib.check(lib.sfh_u8hwc_area_to_f32nchw(_ptr(f), _ptr(out), B, C, H, W, th, tw, _ptr(xo), _ptr(xs), _ptr(xa), _ptr(yo),
                                                 _ptr(ys), _ptr(yb), _stream()), "u8hwc_area_to_f32nchw")
        return out
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=f.device)
    _lib.check(lib.sfh_u8hwc_to_f32nchw(_ptr(f), _ptr(out), B, C, H, W, _stream()), "u8hwc_to_f32nchw")
    return out


def resize_nchw(t, size_hw, mode, align_corners=False):
    """F.interpolate(t, size=size_hw, mode=mode[, align_corners]) for NCHW float32 tensors."""
    t = _f32c(t.contiguous(), "nchw tensor")
    B, C, hs, ws = t.shape
    hd, wd = size_hw
    out = torch.empty((B, C, hd, wd), dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().sfh_resize_nchw(_ptr(t), _ptr(out), B * C, hs, ws, hd, wd, 1 if mode == "bilinear" else 0,
                                   1 if align_corners else 0, _stream()), "resize_nchw")
    return out


def nhwc_to_nchw(t, channels=None, exp=_lib.H2_ACT_EXP):
    if t.dtype in _SPLIT_DTYPES:
        t = s3_to_f32(t, exp)
    B, H, W, cs = t.shape
    C = cs if channels is None else channels
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().sfh_nhwc_to_nchw(_ptr(t), _ptr(out), B, C, H, W, cs, _stream()), "nhwc_to_nchw")
    return out


def nchw_to_nhwc(t, cs=None):
    t = _f32c(t, "nchw tensor")
    B, C, H, W = t.shape
    cs = cs or -(-C // 4) * 4
    out = torch.empty((B, H, W, cs), dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().sfh_nchw_to_nhwc(_ptr(t), _ptr(out), B, C, H, W, cs, _stream()), "nchw_to_nhwc")
    return out


def poi_project(theta, poi, normalize=True):
    theta = _f32c(theta.reshape(-1, 3, 3).contiguous(), "theta")
    B = theta.shape[0]
    if poi.shape[0] < B:
        raise ValueError(f"batch {B} exceeds the court POI batch {poi.shape[0]}")
    p = _f32c(poi[:B].contiguous(), "court_poi")
    out = torch.empty_like(p)
    _lib.check(_lib.load().sfh_poi_project_fwd(_ptr(theta), _ptr(p), B, p.shape[1], 1 if normalize else 0,
                                       _ptr(out), _stream()), "poi_project")
    return out


def consistency_ce(logits, mask_i32):
    lib = _lib.load()
    logits = _f32c(logits, "logits")
    B, nc, H, W = logits.shape
    if mask_i32.dtype != torch.int32 or not mask_i32.is_contiguous():
        raise ValueError("warp mask must be a contiguous int32 tensor")
    hm, wm = mask_i32.shape[1], mask_i32.shape[2]
    partial = torch.empty(lib.sfh_ce_workspace_floats(B, H, W), dtype=torch.float32, device=logits.device)
    score = torch.empty(B, dtype=torch.float32, device=logits.device)
    _lib.check(lib.sfh_consistency_ce_fwd(_ptr(logits), _ptr(mask_i32), B, nc, H, W, hm, wm, _ptr(partial),
                                          _ptr(score), _stream()), "consistency_ce")
    return score
