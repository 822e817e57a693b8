"""One SHA-256 per (kernel, case) of every order-fixed output of the BatchNorm family of csrc/train_bn.hip (with the
fused OutConv and first-layer backward-filter of train_heads.hip and train_wgrad.hip), on the shapes of
tests/train_kernel_cases.py and of the two sibling tests of tests/test_gpu_train_kernels.py.  Two builds of the library
compute the same bits exactly when the two listings are equal line for line:

    python profiles/train_kernel_digest.py > new.txt
    SFH_AMD_LIB=<other libsfh_amd.so> python profiles/train_kernel_digest.py > other.txt       (a fresh process each)

Atomically summed outputs (the fp64 accumulators, multi-tile weight gradients) have a free order and are not listed; the
bound tests hold them.  profiles/ab_bn_math.txt keeps the listing of the commit that introduced csrc/bn_math.h,
profiles/ab_train_split.txt that of the commit that split csrc/train.hip into those files."""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import train_kernel_cases as cases  # noqa: E402
import train_kernel_ref as R  # noqa: E402
from sfh_amd import _lib  # noqa: E402
from sfh_amd import engine as E  # noqa: E402
from sfh_amd.engine import _ptr, _stream  # noqa: E402

lib = _lib.load()
EPS, MOM = cases.EPS, cases.MOMENTUM
WGRAD_ONE_TILE = [(1, 8, 8), (1, 4, 16), (1, 2, 32), (1, 3, 5)]
WGRAD_M = [12, 72]


def emit(kernel, case, **outs):
    torch.cuda.synchronize()
    for name, t in outs.items():
        print(f"{kernel} {case} {name} {hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()}")


def ok(rc):
    _lib.check(rc, "train_kernel_digest")


def zeros(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def dev(c, *names):
    return [c[k].cuda() for k in names]


def bwd_acc(c, mode):
    y, relu = cases.bwd_inputs(c, mode)
    s, _ = R.bn_bwd_reduce_ref(c["dy"], y, c["z"], c["mi"], c["gamma"], c["beta"], relu)
    return torch.from_numpy(s.astype(np.float64).reshape(-1)).cuda()


def planes(fmt, B, H, W, C):
    return zeros(E.split_shape(fmt, B, H, W, C), E._SPLIT[fmt][0]), zeros((1,), torch.int32)


def bn_apply():
    for shape, with_res, relu in itertools.product(cases.APPLY_SHAPES, (False, True), (0, 1)):
        c = cases.shape_case(shape)
        z, mi, gam, bet, res = dev(c, "z", "mi", "gamma", "beta", "residual")
        y = zeros((c["npix"], c["C"]))
        ok(lib.sfh_bn_apply(_ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), _ptr(res) if with_res else None, relu, c["npix"], c["C"],
                            _ptr(y), None, 0, 0, None, _stream()))
        emit("bn_apply", f"{cases.ident(shape)}-res{int(with_res)}-relu{relu}", y=y)
    for shape, with_res, fmt in itertools.product(cases.SPLIT_SHAPES, (False, True), ("s3", "h2")):
        B, H, W, C = shape
        c = cases.shape_case(shape)
        z, mi, gam, bet, res = dev(c, "z", "mi", "gamma", "beta", "residual")
        y, (pl, over) = zeros(shape), planes(fmt, *shape)
        ok(lib.sfh_bn_apply(_ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), _ptr(res) if with_res else None, 1, c["npix"], C, _ptr(y),
                            _ptr(pl), W, E._SPLIT[fmt][2], _ptr(over), _stream()))
        emit("bn_apply_split", f"{cases.ident(shape)}-res{int(with_res)}-{fmt}", y=y, planes=pl, overflow=over)


def bn_bwd_apply():
    for shape, mode in itertools.product(cases.APPLY_SHAPES + cases.SPLIT_SHAPES, cases.BWD_MODES):
        B, H, W, C = shape
        c = cases.shape_case(shape)
        y, relu = cases.bwd_inputs(c, mode)
        dy, z, mi, gam, bet = dev(c, "dy", "z", "mi", "gamma", "beta")
        yg, acc = (y.cuda() if y is not None else None), bwd_acc(c, mode)
        args = (_ptr(dy), _ptr(yg), _ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), _ptr(acc), relu, c["npix"], C)
        dz, dres, a32 = zeros(shape), zeros(shape), zeros((2 * C,))
        ok(lib.sfh_bn_bwd_apply(*args, _ptr(dz), _ptr(dres), None, 0, 0, None, _ptr(a32), _stream()))
        emit("bn_bwd_apply", f"{cases.ident(shape)}-{mode}", dz=dz, dres=dres, acc_f32=a32)
        if shape not in cases.SPLIT_SHAPES:
            continue
        for fmt in ("s3", "h2"):
            dz, dres, a32, (pl, over) = zeros(shape), zeros(shape), zeros((2 * C,)), planes(fmt, *shape)
            ok(lib.sfh_bn_bwd_apply(*args, _ptr(dz), _ptr(dres), _ptr(pl), W, E._SPLIT[fmt][2], _ptr(over), _ptr(a32), _stream()))
            emit("bn_bwd_apply_split", f"{cases.ident(shape)}-{mode}-{fmt}", dz=dz, dres=dres, planes=pl, acc_f32=a32, overflow=over)


def pool():
    for shape, fmt in itertools.product(cases.SPLIT_SHAPES, ("s3", "h2")):
        B, H, W, C = shape
        c = cases.shape_case(shape)
        z, mi, gam, bet = dev(c, "z", "mi", "gamma", "beta")
        (ypl, over), (ppl, _) = planes(fmt, B, H, W, C), planes(fmt, B, H // 2, W // 2, C)
        ok(lib.sfh_bn_apply_pool(_ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), B, H, W, C, _ptr(ypl), _ptr(ppl), E._SPLIT[fmt][2],
                                 _ptr(over), _stream()))
        emit("bn_apply_pool", f"{cases.ident(shape)}-{fmt}", y_planes=ypl, pool_planes=ppl, overflow=over)
    for shape, accumulate in itertools.product([s for s in cases.APPLY_SHAPES + cases.SPLIT_SHAPES if s[1] >= 2 and s[2] >= 2], (0, 1)):
        B, H, W, C = shape
        c = cases.shape_case(shape)
        z, mi, gam, bet = dev(c, "z", "mi", "gamma", "beta")
        g = torch.Generator().manual_seed(H * 1000 + W)
        dp = torch.randn(B, H // 2, W // 2, C, generator=g).cuda()
        dx = torch.randn(B, H, W, C, generator=g).cuda() if accumulate else zeros(shape)
        acc = zeros((2, C), torch.float64)
        ok(lib.sfh_pool2_bwd_bn_reduce(_ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), _ptr(dp), B, H, W, C, accumulate, _ptr(dx),
                                       _ptr(acc), _stream()))
        emit("pool2_bwd_bn_reduce", f"{cases.ident(shape)}-acc{accumulate}", dx=dx)


def outconv():
    for shape in cases.OUTCONV_SHAPES:
        B, H, W, cin, nc = shape
        c = cases.outconv_case(shape)
        x, z, mi, gam, bet, w, dl = dev(c, "x", "z", "mi", "gamma", "beta", "w", "dl")
        for bn in (False, True):
            dx, aw, ab, abn = zeros((B * H * W, cin)), zeros((nc, cin), torch.float64), zeros((nc,), torch.float64), zeros((2, cin), torch.float64)
            if bn:
                ok(lib.sfh_outconv_bwd_bn(_ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), cin, _ptr(w), _ptr(dl), nc, B, H, W, _ptr(dx),
                                          _ptr(aw), _ptr(ab), _ptr(abn), _stream()))
            else:
                ok(lib.sfh_outconv_bwd(_ptr(x), cin, _ptr(w), _ptr(dl), nc, B, H, W, _ptr(dx), _ptr(aw), _ptr(ab), _stream()))
            emit("outconv_bwd_bn" if bn else "outconv_bwd", cases.ident(shape), dx=dx)


def finalize():
    for C, npix in itertools.product(cases.FINALIZE_C, cases.FINALIZE_NPIX):
        c = cases.finalize_case(C, npix)
        acc, rm, rv = dev(c, "acc", "running_mean", "running_var")
        mi, cnt = zeros((2 * C,)), zeros((1,), torch.int64)
        ok(lib.sfh_bn_finalize(_ptr(acc), npix, C, EPS, MOM, _ptr(rm), _ptr(rv), _ptr(mi), _ptr(cnt), _stream()))
        emit("bn_finalize", f"C{C}-n{npix}", mean_invstd=mi, running_mean=rm, running_var=rv, counter=cnt)
    for rows, C in itertools.product(cases.PARTIAL_ROWS, cases.PARTIAL_C):
        c = cases.partials_case(rows, C)
        p, rm, rv = dev(c, "partial", "running_mean", "running_var")
        mi, cnt = zeros((2 * C,)), zeros((1,), torch.int64)
        ok(lib.sfh_bn_finalize_partials(_ptr(p), rows, c["npix"], C, EPS, MOM, _ptr(rm), _ptr(rv), _ptr(mi), _ptr(cnt), _stream()))
        emit("bn_finalize_partials", f"{rows}x{C}", mean_invstd=mi, running_mean=rm, running_var=rv, counter=cnt)


def wgrad_c4_bn():
    for (B, H, W), M in itertools.product(WGRAD_ONE_TILE, WGRAD_M):
        c = cases.bn_case(B * H * W, M, "randn")
        dy, z, mi, gam, bet = dev(c, "dy", "z", "mi", "gamma", "beta")
        acc = bwd_acc(c, "recompute")
        x = torch.randn(B, H, W, 4, generator=torch.Generator().manual_seed(1000 * B * H * W + M))
        x[..., 3] = 0.0
        xg, raw = x.cuda(), zeros((M, 9, 4))
        ok(lib.sfh_conv_wgrad_c4_bn(_ptr(dy), _ptr(z), _ptr(mi), _ptr(gam), _ptr(bet), _ptr(acc), M, _ptr(xg), 3, B, H, W, _ptr(raw),
                                    4, _stream()))
        emit("conv_wgrad_c4_bn", f"{B}x{H}x{W}-M{M}", raw=raw)


if __name__ == "__main__":
    for part in (bn_apply, bn_bwd_apply, pool, outconv, finalize, wgrad_c4_bn):
        part()
