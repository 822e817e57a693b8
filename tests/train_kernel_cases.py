"""Inputs shared by tests/test_train_kernel_host.py (CPU) and tests/test_gpu_train_kernels.py (GPU): the smallest shapes at
which each plain training kernel of csrc/train_bn.hip and csrc/train_heads.hip can still go wrong.  Everything is drawn
from seeded generators, so both files see the same numbers; the cases are cached, and nobody writes into them."""
import functools
import zlib

import numpy as np
import torch

import train_kernel_ref as R

EPS, MOMENTUM = 1e-5, 0.1

# (npix, C) of the per-channel reductions: bn_stats, bn_bwd_reduce, colsum
REDUCTIONS = [
    (1, 4),          # a single pixel
    (5, 4),          # fewer pixels than lanes
    (257, 4),        # two blocks
    (300, 12),       # 3 quads: 85 lanes, thread 255 idle
    (1000, 64),      # the four-pixel unrolled loop and its tail in one block
    (777, 96),       # a quad count that does not divide 256
    (129, 1024),     # one lane per quad
    (70, 1036),      # a second channel chunk of 3 quads
    (70, 2048),      # two full channel chunks
    (262401, 4),     # grid saturated at 1024 blocks; a 4 MB tensor
]
REDUCTION_DATA = ["randn", "offset"]      # offset: 100 + 0.01 randn, the cancellation case
COLSUM_SLICE = (300, 32, 96, 32)          # (npix, C, cs, c_off): a channel slice inside a wider tensor

FINALIZE_C = [1, 3, 256, 257]
FINALIZE_NPIX = [1, 2, 4096, 14745600]
PARTIAL_ROWS = [1, 3, 4, 5, 15, 16, 17, 127, 128, 129, 257]
PARTIAL_C = [1, 33, 64, 65, 130]
PARTIAL_ROW_PIXELS = 64                   # pixels behind one row of a partial-sum table

APPLY_SHAPES = [(1, 1, 1, 4), (2, 3, 5, 12), (3, 7, 37, 96), (1, 2, 3, 2048)]
SPLIT_SHAPES = [(3, 7, 37, 96), (1, 5, 3, 32)]          # C % 32 == 0: the launches that also write the split copy
BWD_MODES = ["linear", "y", "recompute"]                # relu = 0; relu with y given; relu with y == NULL
BWD_OUTPUTS = [(0, 0), (1, 1), (1, 0), (0, 1)]          # (dres wanted, acc_f32 wanted)

POOL_SHAPES = [(1, 2, 2, 4), (2, 5, 7, 12), (3, 8, 6, 64), (1, 3, 2, 1028)]
POOL_DATA = ["randn", "halves", "constant", "zeros", "nan"]      # nan: the forward only

# (B, H, W, cin, nc)
OUTCONV_SHAPES = [
    (1, 1, 1, 4, 1),         # a single pixel
    (2, 9, 13, 12, 3),       # 3 quads per pixel
    (1, 33, 32, 64, 4),      # 1056 pixels: a second block of 32
    (2, 37, 29, 64, 5),      # 2146 pixels: the second block spans two frames
    (3, 19, 23, 256, 8),     # 4 lanes, 256 pixels per thread: the 64-term flush
]
OUTCONV_NO_DX = (2, 9, 13, 12, 3)         # run once more with dx == NULL (sfh_outconv_bwd only)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ident(shape):
    return "x".join(map(str, shape))


# ------------------------------------------------------------------------------------------------ BatchNorm
def _activations(g, npix, C, kind):
    """z (npix, C) fp32: channel 1 constant (variance exactly 0), channel 2 all zero, the others randn with a per-channel
    scale and shift, or 100 + 0.01 randn"""
    z = torch.randn(npix, C, generator=g)
    if kind == "offset":
        z = 100.0 + 0.01 * z
    else:
        z = z * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    z[:, 1] = 100.25 if kind == "offset" else 0.7
    z[:, 2] = 0.0
    return z.contiguous()


@functools.lru_cache(maxsize=None)
def bn_case(npix, C, kind="randn", W=0):
    """One BatchNorm layer's tensors over (npix, C): z, its batch statistics as the kernels would leave them (mi = the fp32
    [mean | invstd] of bn_finalize_ref on bn_stats_ref), gamma and beta (beta = 0 on the constant and the zero channel: there
    the pre-activation is an exact zero), a residual, the forward outputs y (fp32, the rounded reference, with the
    residual) and dy."""
    g = _gen("bn", npix, C, kind)
    z = _activations(g, npix, C, kind)
    s, A = R.bn_stats_ref(z)
    fin = R.bn_finalize_ref(s.astype(np.float64), npix, EPS, MOMENTUM)
    mi = torch.from_numpy(np.concatenate([fin["mean"], fin["invstd"]]).astype(np.float32))
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[1:3] = 0.0
    residual = torch.randn(npix, C, generator=g)
    dy = torch.randn(npix, C, generator=g)
    y_res = torch.from_numpy(R.bn_apply_ref(z, mi, gamma, beta, residual, 1)["y"].astype(np.float32))
    return {"id": f"{npix}x{C}-{kind}", "npix": npix, "C": C, "W": W, "z": z, "mi": mi, "gamma": gamma, "beta": beta,
            "residual": residual, "dy": dy, "y_res": y_res, "stats": (s, A),
            "acc_pre": 0.5 * torch.randn(2, C, generator=g).double()}


def bwd_inputs(c, mode):
    """(y, relu) of a backward mode: the layer with a residual hands its y over, the one without lets the kernel recompute"""
    return {"linear": (None, 0), "y": (c["y_res"], 1), "recompute": (None, 1)}[mode]


def shape_case(shape, kind="randn"):
    B, H, W, C = shape
    return bn_case(B * H * W, C, kind, W)


# ------------------------------------------------------------------------------------------------ finalize
@functools.lru_cache(maxsize=None)
def finalize_case(C, npix):
    """acc (2, C) fp64 of a layer with means of both signs (every fourth near 100) and variances in [0, 2] (every fifth
    exactly 0); with npix == 1 the sums are those of one pixel.  Channel 0 is built so that acc1 / n - mean^2 rounds below
    zero in fp64 (checked here), which the kernel has to clamp.  Running statistics as a trained layer has them."""
    g = _gen("finalize", C, npix)
    mean = 3.0 * torch.randn(C, generator=g).double() + torch.where(torch.arange(C) % 4 == 3, 100.0, 0.0)
    var = 2.0 * torch.rand(C, generator=g).double() * (torch.arange(C) % 5 != 4)
    if npix == 1:
        var = var * 0
    acc = torch.stack([mean * npix, (var + mean * mean) * npix]).numpy()
    m = acc[0, 0] / npix
    a1 = np.nextafter(m * m * npix, -np.inf) * (1.0 - 2.0 ** -50)
    assert a1 / npix - m * m < 0.0
    acc[1, 0] = a1
    return {"acc": torch.from_numpy(acc), "running_mean": torch.randn(C, generator=g),
            "running_var": 0.5 + torch.rand(C, generator=g)}


@functools.lru_cache(maxsize=None)
def partials_case(rows, C):
    """(rows, 2, C) fp64: row r holds [sum z | sum z^2] of its own 64 pixels, as a conv epilogue leaves them"""
    g = _gen("partials", rows, C)
    z = (torch.randn(rows, PARTIAL_ROW_PIXELS, C, generator=g) * (0.5 + torch.rand(C, generator=g))
         + 2.0 * torch.randn(C, generator=g)).double()
    return {"partial": torch.stack([z.sum(dim=1), (z * z).sum(dim=1)], dim=1).contiguous(), "npix": rows * PARTIAL_ROW_PIXELS,
            "running_mean": torch.randn(C, generator=g), "running_var": 0.5 + torch.rand(C, generator=g),
            "acc_pre": 0.5 * torch.randn(2 * C, generator=g).double()}


# ------------------------------------------------------------------------------------------------ max-pool
@functools.lru_cache(maxsize=None)
def pool_case(shape, kind):
    """x, dy (fp32) and the earlier content of dx for the accumulating launch"""
    B, H, W, C = shape
    g = _gen("pool", shape, kind)
    x = torch.randn(B, H, W, C, generator=g)
    if kind == "halves":
        x = torch.round(2.0 * x) / 2.0                                   # ties in most windows
    elif kind == "constant":
        x = torch.full_like(x, 0.75)                                     # every window is all ties
    elif kind == "zeros":
        x = torch.where(torch.rand(x.shape, generator=g) < 0.5, -0.0, 0.0) * torch.ones_like(x)    # mixed +0 / -0
    elif kind == "nan":
        x[0, 0, 1, 0] = float("nan")                                     # second in scan order
        x[-1, H // 2 * 2 - 1, W // 2 * 2 - 1, C - 1] = float("nan")      # the last element of the last window
    return {"x": x, "dy": torch.randn(B, H // 2, W // 2, C, generator=g), "pre": torch.randn(B, H, W, C, generator=g)}


# ------------------------------------------------------------------------------------------------ OutConv backward
@functools.lru_cache(maxsize=None)
def outconv_case(shape):
    """x (B,H,W,cin) - for the BatchNorm form the conv output z it is recomputed from, with mi, gamma, beta -, w (nc,cin),
    dl (B,nc,H,W) and the earlier contents of the three accumulators"""
    B, H, W, cin, nc = shape
    g = _gen("outconv", shape)
    c = bn_case(B * H * W, cin, "randn")
    return {"z": c["z"].reshape(B, H, W, cin), "mi": c["mi"], "gamma": c["gamma"], "beta": c["beta"],
            "x": torch.relu(torch.randn(B, H, W, cin, generator=g)), "w": 0.2 * torch.randn(nc, cin, generator=g),
            "dl": torch.randn(B, nc, H, W, generator=g) / (B * H * W),
            "acc_w": 0.5 * torch.randn(nc, cin, generator=g).double(), "acc_b": 0.5 * torch.randn(nc, generator=g).double(),
            "acc_bn": 0.5 * torch.randn(2, cin, generator=g).double()}
