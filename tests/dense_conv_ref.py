"""fp64 CPU references (test infrastructure only) for the dense convolution launches: sfh_conv_fwd (csrc/conv_mfma.hip),
sfh_conv_s3_fwd in its S3 and H2 source formats (csrc/conv_s3.hip), sfh_conv_small_fwd (csrc/conv_small.hip), the same
kernels as backward-data through pack modes 1, 3 and 4, and the backward-filter pair sfh_conv_wgrad (csrc/train_wgrad.hip) and
sfh_conv_wgrad_s3 (csrc/wgrad_s3.hip).  Plain numpy / torch-CPU; nothing here imports the library.

Tensors are NHWC numpy arrays as the kernels see them.  Every reference returns its value and the absolute sum
``A = sum |term|`` its bound is built from; every bound is a count of roundings read off the kernel (u = 2^-24, factor 1.01
for the second-order terms), none is fitted to a kernel's output, and each adds the fp64 reference's own error (the same
count at 2^-53).  A count that cannot be read off the source - how one MFMA instruction rounds inside itself - is taken at
its worst case: sequential, one rounding per product and per addition.

n * u rule (Jeannerod and Rump 2013, as in tests/train_kernel_ref.py): a sum of n fp32 products accumulated in ANY order,
contracted or not, errs by at most n * u * sum |a_i b_i|; a sum of n EXACT terms by at most (n - 1) * u * sum |t_i|.

The three arithmetics (K = the real terms of one output; zero-padded channels and taps add exact zeros):

fp32   conv_mfma_kernel / wgrad_kernel: v_mfma_f32_16x16x4f32 chains, one rounding per product and per addition.
       |d acc| <= 1.01 * K * u * A.

S3     three bf16 planes per operand, v = p0 + p1 + p2 EXACTLY (include/sfh_amd.h), |p1| <= 2^-8 (1 + 2^-8) |v|,
       |p2| <= 2^-16 |v|.  A bf16 x bf16 product has 16 significand bits: exact in fp32, so only additions round.  The
       stage loop keeps w0x2 + w1x1 + w2x0 + w0x1 + w1x0 + w0x0 and drops w1x2 + w2x1 + w2x2 <= (2 * 2^-24 * (1 + 2^-8) +
       2^-32) |w x| <= 2.02 u |w x|.  The 6 K retained terms meet in at most 6 K - 1 additions and sum in absolute value to at
       most (1 + 2^-7 + 2^-15)^2 A <= 1.016 A:   |d acc| <= 1.01 * u * (6 K * 1.016 + 2.02) * A.

H2     two fp16 planes of U = v * 2^e: p0 = f16(U), p1 = f16(U - p0).  The header's statement of the format, used as it
       stands: |U - p0 - p1| <= 2^-22 |U| while |U| >= 2^-3, <= 2^-25 below that - h2_rep() returns this d(v) in real units,
       and l(v) = 2^-11 |v| + 2^-24 2^-e >= |p1| 2^-e.  fp16 x fp16 products (22 bits) are exact in fp32.  With the
       operands a, b:  representation  R = sum (d_a |b| + |a| d_b + d_a d_b),  the one dropped product  D = sum l_a l_b,
       the 3 K retained terms sum in absolute value to at most Ahat = sum (|a| + 2 l_a)(|b| + 2 l_b):
       |d acc| <= 1.01 * (R + D) + 1.01 * 3 K * u * Ahat.
       The exponents are powers of two folded into the epilogue scale: exact, they do not enter.

Epilogue (csrc/conv_epilogue.h), y = [relu](acc * scale + shift [+ residual]): the product and the sum round once each (or
once together), the residual enters by at most three additions (an S3 residual is added plane by plane), an H2 residual
carries its own representation error d(r), ReLU is 1-Lipschitz:
       |dy| <= |scale| * |d acc| + 1.01 u (|acc scale| + |pre|) + 3.03 u (|pre| + |r|) + 1.01 d(r).
An H2 destination stores the H2 split of the computed y: + d(|y| + |dy|) at the destination's exponent; an S3 destination
is exact.  The pooled second output is the maximum of four stored values: its bound is the maximum of their bounds.
The H2 range word (sfh_conv_desc.h2_range) is the largest |y * 2^e| over the tensor's elements - lanes of a workgroup tile
that lie past the frame or on the shared zero rows between frames store nothing and do not enter it -: it must lie within
the element bound of max |y| 2^e, and the overflow word stays 0 while nothing saturates.

Backward-filter, raw[m][tap][n] = raw0 + sum_p dz[p][m] * x[p + tap][n] over P pixels (the header above sfh_conv_wgrad): a
workgroup accumulates its pixels in MFMA chains from an exact zero, then W workgroups add their sums onto raw atomically
in free order - W roundings, each relative to a running value of at most |raw0| + A.  No cross-lane additions in either
kernel.  With T = 1, 6 or 3 retained terms per product:
       |d raw| <= 1.01 u ((T P + W) Ahat + W |raw0|)  [+ 1.01 (R + D) for H2, + 2.02 u A for S3],
W is bounded by the number of 64-pixel tiles (both launchers clamp their split count to it).  An element all of whose
terms are zero keeps raw0 exactly: adding an exact zero rounds nothing.

Deviations that are rules, not defects:
  * pool0 takes the maximum with sfh_max_nan, which propagates NaN where F.max_pool2d's CPU kernel may not; no case here
    feeds a NaN into a pooled window.
  * -0 does not survive the S3 round trip as -0: plane 1 of -0 is +0 and -0 + 0 = +0.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
E53 = 2.0 ** -53
H2_ACT_EXP = 2      # SFH_H2_ACT_EXP
NPROD = {"f32": 1, "s3": 6, "h2": 3}


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _t(w):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float64)))


def out_size(n, ksize, stride):
    """padding ksize // 2 before, (ksize - 1) // 2 after: 3 -> 1 / 1, 1 -> 0 / 0, 4 -> 2 / 1"""
    return (n + ksize // 2 + (ksize - 1) // 2 - ksize) // stride + 1


# ------------------------------------------------------------------------------------------------ the split formats
def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def split_s3(v):
    """plane0 = bf16(v), plane1 = bf16(v - plane0), plane2 = bf16(v - plane0 - plane1), the subtractions in fp32"""
    f32 = np.float32
    v = np.asarray(v, dtype=f32)
    p0 = _bf16(v)
    r1 = (v - p0).astype(f32)
    p1 = _bf16(r1)
    return p0, p1, _bf16((r1 - p1).astype(f32))


def split_h2(v, e):
    """u = v * 2^e saturated to +-65504, plane0 = f16(u), plane1 = f16(u - plane0), as fp32 arrays (the numpy statement of
    the H2 split of include/sfh_amd.h; tests/test_dense_conv_host.py holds h2_rep() to it)"""
    f32 = np.float32
    u = np.clip(np.asarray(v, dtype=f32) * f32(2.0 ** e), f32(-65504.0), f32(65504.0)).astype(f32)
    p0 = u.astype(np.float16).astype(f32)
    return p0, (u - p0).astype(f32).astype(np.float16).astype(f32)


# ------------------------------------------------------------------------------------------------ the linear maps
def assemble(x0, c0, x1=None, c1=0, pad1=(0, 0), pool0=False):
    """the conv input frame: channels [0, c0) of x0 - MaxPool2d(2) (floor) applied first with pool0 - beside channels
    [0, c1) of x1 placed at pad1 = (top, left) inside the frame, zero elsewhere -> (B,H,W,c0+c1) float64"""
    a = np.asarray(x0, dtype=np.float64)[..., :c0]
    if pool0:
        a = _nhwc(F.max_pool2d(_nchw(a), 2))
    if x1 is None:
        return a
    B, H, W, _ = a.shape
    b = np.asarray(x1, dtype=np.float64)[..., :c1]
    full = np.zeros((B, H, W, c1))
    full[:, pad1[0]:pad1[0] + b.shape[1], pad1[1]:pad1[1] + b.shape[2]] = b
    return np.concatenate([a, full], axis=3)


def conv_op(ksize, stride=1):
    """-> op(x NHWC, w OIHW) = nn.Conv2d(ksize, stride, bias=False) with the kernels' padding, NHWC float64"""
    pb, pa = ksize // 2, (ksize - 1) // 2

    def op(x, w):
        return _nhwc(F.conv2d(F.pad(_nchw(x), (pb, pa, pb, pa)), _t(w), None, stride))
    return op


def stem_op(x, w):
    """nn.Conv2d(cin, cout, 7, stride 2, padding 3, bias=False): what pack mode 2 + sfh_space_to_depth2 + a ksize-4 launch
    compute (models/resnet.py:172)"""
    return _nhwc(F.conv2d(_nchw(x), _t(w), None, 2, 3))


def up_op(x, w):
    """nn.ConvTranspose2d(cin, cout, 2, stride 2) as the launch sees it: a 1x1 conv to 4 * cout VIRTUAL channels,
    (dy * 2 + dx) * cout + co; w IOHW (cin, cout, 2, 2) -> (B,H,W,4*cout)"""
    w = np.asarray(w, dtype=np.float64)
    wv = np.transpose(w, (2, 3, 1, 0)).reshape(4 * w.shape[1], w.shape[0], 1, 1)
    return _nhwc(F.conv2d(_nchw(x), _t(wv)))


def up2_op(H, W):
    """-> op(x (B,h0,w0,C), w OIHW (4*cout, C, 2, 2)) = the 2x2 up-scatter conv of sfh_conv_s3_fwd (ksize 2, include/sfh_amd.h:
    SFH_OUT_UPSCATTER2) on the H x W conv frame, x zero-extended to it (h0 in {H, H-1}): virtual channel (dy*2+dx)*cout + co
    of pixel (y, x) = sum_{c,ky,kx} x[y + dy - 1 + ky][x + dx - 1 + kx][c] * w[(dy*2+dx)*cout + co][c][ky][kx], zero outside
    -> (B,H,W,4*cout)"""
    def op(x, w):
        x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
        c = w.shape[0] // 4
        P = np.zeros((x.shape[0], H + 2, W + 2, x.shape[3]))
        P[:, 1:1 + x.shape[1], 1:1 + x.shape[2]] = x
        outs = [_nhwc(F.conv2d(_nchw(P[:, (q >> 1):(q >> 1) + H + 1, (q & 1):(q & 1) + W + 1]), _t(w[q * c:(q + 1) * c])))
                for q in range(4)]
        return np.concatenate(outs, axis=3)
    return op


def upscatter(yv):
    """SFH_OUT_UPSCATTER2: virtual channel (dy * 2 + dx) * cout + co of pixel (y, x) -> channel co of (2y + dy, 2x + dx)"""
    B, H, W, C4 = yv.shape
    c = C4 // 4
    out = np.zeros((B, 2 * H, 2 * W, c), dtype=yv.dtype)
    for q in range(4):
        out[:, q >> 1::2, q & 1::2] = yv[..., q * c:(q + 1) * c]
    return out


def bwd_data_op(ksize, H, W):
    """-> op(dz NHWC, w OIHW (cout, cin, k, k)) = the gradient of the stride-1 conv with respect to its input (pack mode 3),
    through fp64 autograd"""
    def op(dz, w):
        w = _t(w)
        x = torch.zeros((dz.shape[0], w.shape[1], H, W), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(F.pad(x, (ksize // 2, (ksize - 1) // 2) * 2), w)
        return _nhwc(torch.autograd.grad(y, x, _nchw(dz))[0].detach())
    return op


def up_bwd_data_op(dy, w):
    """the gradient of nn.ConvTranspose2d(cin, cout, 2, stride 2) with respect to its input (pack mode 4 behind
    sfh_space_to_depth2): dy (B,2h,2w,cout), w IOHW (cin, cout, 2, 2) -> (B,h,w,cin), through fp64 autograd"""
    w = _t(w)
    B, H2, W2, _ = dy.shape
    x = torch.zeros((B, w.shape[0], H2 // 2, W2 // 2), dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, None, 2)
    return _nhwc(torch.autograd.grad(y, x, _nchw(dy))[0].detach())


def wgrad_op(ksize, pad=(0, 0), frame=None):
    """-> op(dz (B,H,W,M), x (B,xh,xw,N)) = raw (M, ksize^2, N) float64, the sum in the header above sfh_conv_wgrad:
    raw[m][ky*k+kx][n] = sum_{b,y,x} dz[b][y][x][m] * xin[b][y + ky - p][x + kx - p][n], xin = x at pad = (top, left) inside the
    H x W frame, zero elsewhere, p = ksize // 2.  Written out as stated, not through autograd (tests/test_dense_conv_host.py
    holds it to autograd)."""
    p = ksize // 2

    def op(dz, x):
        dz, x = np.asarray(dz, dtype=np.float64), np.asarray(x, dtype=np.float64)
        B, H, W, M = dz.shape
        N = x.shape[3]
        xin = np.zeros((B, H + ksize - 1, W + ksize - 1, N))
        xin[:, p + pad[0]:p + pad[0] + x.shape[1], p + pad[1]:p + pad[1] + x.shape[2]] = x
        raw = np.zeros((M, ksize * ksize, N))
        for ky in range(ksize):
            for kx in range(ksize):
                raw[:, ky * ksize + kx] = np.einsum("bhwm,bhwn->mn", dz, xin[:, ky:ky + H, kx:kx + W])
        return raw
    return op


# ------------------------------------------------------------------------------------------------ the bounds
def h2_rep(v, e):
    """H2 tensor with exponent e -> (d, l): d = the header's representation error of v (2^-22 |v| while |v| 2^e >= 2^-3, else
    2^-25 2^-e), l >= |p1| 2^-e, both in real units"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    d = np.where(a * 2.0 ** e >= 2.0 ** -3, a * 2.0 ** -22, 2.0 ** (-25 - e))
    return d * (a > 0), (a * 2.0 ** -11 + 2.0 ** (-24 - e)) * (a > 0)


def bilinear(op, a, b, K, arith, ea=H2_ACT_EXP, eb=H2_ACT_EXP):
    """op bilinear in (a, b), each output a sum of at most K real terms -> (value, A = op(|a|, |b|), accumulator bound) for
    the arithmetic 'f32', 's3' or 'h2' (ea, eb: the exponents of the two H2 operands; a zero is exact in every format)"""
    val = op(a, b)
    aa, ab = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    A = op(aa, ab)
    own = K * E53 * A
    if arith == "f32":
        return val, A, 1.01 * K * U * A + own
    if arith == "s3":
        return val, A, 1.01 * U * (6 * K * 1.016 + 2.02) * A + own
    assert arith == "h2"
    da, la = h2_rep(a, ea)
    db, lb = h2_rep(b, eb)
    R = np.maximum(op(aa + da, ab + db) - A, 0.0) + 4 * own      # (the subtraction's own fp64 cancellation)
    D = op(la, lb)
    Ahat = op(aa + 2 * la, ab + 2 * lb)
    return val, A, 1.01 * (R + D) + 1.01 * 3 * K * U * Ahat + own


def epilogue(acc, eacc, scale, shift, residual=None, relu=False, res_h2_exp=None, dst_h2_exp=None):
    """y = [relu](acc * scale + shift [+ residual]) per channel -> (y, bound); eacc = the accumulator bound; res_h2_exp /
    dst_h2_exp: the exponent of an H2 residual / destination (None: another format)"""
    scale, shift = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    pre = acc * scale + shift
    # scale == 0: 0 * acc + shift = shift exactly; shift == 0: the addition rounds nothing
    bound = np.abs(scale) * eacc + (1.01 * U + 2 * E53) * (np.abs(acc * scale) + np.abs(pre) * (shift != 0)) * (scale != 0)
    y = pre
    if residual is not None:
        r = np.asarray(residual, dtype=np.float64)
        y = pre + r
        bound = bound + 3.03 * U * (np.abs(pre) + np.abs(r)) * (r != 0) + 2 * E53 * np.abs(y)
        if res_h2_exp is not None:
            bound = bound + 1.01 * h2_rep(r, res_h2_exp)[0]
    if relu:
        y = np.maximum(y, 0.0)
    if dst_h2_exp is not None:
        bound = bound + h2_rep(np.abs(y) + bound, dst_h2_exp)[0] * (np.abs(y) + bound > 0)
    return y, bound


def pooled(y, bound):
    """MaxPool2d(2) (floor) of y and the bound that goes with it (|max a - max b| <= max |a - b|)"""
    mp = lambda a: _nhwc(F.max_pool2d(_nchw(a), 2))
    return mp(y), mp(bound)


def wgrad_tiles(B, H, W):
    """64-pixel tiles of the backward-filter launchers (2x32, 4x16 or 8x8, the fewest; both kernels): the ceiling of the
    number of workgroups that add to one raw element"""
    return B * min(-(-H // th) * -(-W // tw) for th, tw in ((2, 32), (4, 16), (8, 8)))


def wgrad(dz, x, raw0, ksize, arith, pad=(0, 0)):
    """-> (raw = raw0 + the sum, bound); raw0 (M, ksize^2, N) is the slice of the starting raw this launch adds to"""
    B, H, W, _ = dz.shape
    P, Wg = B * H * W, wgrad_tiles(B, H, W)
    op = wgrad_op(ksize, pad)
    val, A, _ = bilinear(op, dz, x, P, "f32")
    r0 = np.abs(np.asarray(raw0, dtype=np.float64))
    if arith == "f32":
        bound = (1.01 * U + E53) * ((P + Wg) * A + Wg * r0 * (A > 0))
    elif arith == "s3":
        bound = (1.01 * U + E53) * ((6 * P + Wg) * 1.016 * A + 2.02 * A + Wg * r0 * (A > 0))
    else:
        _, _, eh = bilinear(op, dz, x, P, "h2")        # R + D + 3 P u Ahat
        Ahat = op(np.abs(dz) + 2 * h2_rep(dz, H2_ACT_EXP)[1], np.abs(x) + 2 * h2_rep(x, H2_ACT_EXP)[1])
        bound = eh + (1.01 * U + E53) * (Wg * Ahat + Wg * r0 * (A > 0))
    return val + np.asarray(raw0, dtype=np.float64), bound


def ratio(got, ref, bound):
    """max |got - ref| / bound; an entry with a zero bound must be exact"""
    err = np.abs(np.asarray(got).astype(np.longdouble) - np.asarray(ref).astype(np.longdouble)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert not np.isnan(err).any(), "NaN in the output"
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference leaves no room"
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


# ------------------------------------------------------------------------------------------------ exact copies
def shifted_copy(src, c_src, cout, o, ky, kx, ksize, stride):
    """what a weight with a single 1 at (o, c_src, ky, kx) must produce from the assembled frame src (B,H,W,C):
    dst[b, oy, ox, o] = src[b, oy * stride + ky - p, ox * stride + kx - p, c_src], p = ksize // 2, zero where that pixel lies in
    the padding and in every other channel"""
    B, H, W, _ = src.shape
    p = ksize // 2
    Ho, Wo = out_size(H, ksize, stride), out_size(W, ksize, stride)
    out = np.zeros((B, Ho, Wo, cout), dtype=np.float64)
    for oy in range(Ho):
        sy = oy * stride + ky - p
        if not 0 <= sy < H:
            continue
        for ox in range(Wo):
            sx = ox * stride + kx - p
            if 0 <= sx < W:
                out[:, oy, ox, o] = src[:, sy, sx, c_src]
    return out


def scattered_copy(dz, o, cin, c, ky, kx, ksize):
    """the transpose of shifted_copy at stride 1 (backward-data of the impulse weight): dx[b, y + ky - p, x + kx - p, c] =
    dz[b, y, x, o]"""
    B, H, W, _ = dz.shape
    p = ksize // 2
    out = np.zeros((B, H, W, cin), dtype=np.float64)
    for y in range(H):
        sy = y + ky - p
        if not 0 <= sy < H:
            continue
        for x in range(W):
            sx = x + kx - p
            if 0 <= sx < W:
                out[:, sy, sx, c] = dz[:, y, x, o]
    return out
