"""fp64 CPU references (test infrastructure only) for the specialised convolution launches: sfh_conv_upfused_fwd and the two
launches it replaces (csrc/conv_upfused.hip; sfh_conv_s3_fwd with shift_border / acc_init), sfh_conv3x3_c4h2_fwd,
sfh_conv3x3_c4_fwd, sfh_frame_to_h2, sfh_conv_inc_fused_fwd and sfh_stem7x7_fwd.  Plain numpy / torch-CPU; nothing here
imports the library.  The linear maps, the three arithmetics' accumulator bounds, the epilogue's bound and the exact copies
are tests/dense_conv_ref.py's, used as they stand with its conventions (u = 2^-24, factor 1.01, the n * u rule, worst case
where an MFMA's inner order is unknown); this file adds only what those launches have beyond a dense conv.

The fused Up block (header of csrc/conv_upfused.hip; the same arithmetic in one launch or in two):
    accA = the 2x2 up-scatter conv of the low-resolution x, K_A = 4 c1 real terms, H2 arithmetic     |d accA| <= eA
    v    = accA * up_scale + shift_border[class of the output pixel]: the product and the sum round once each
           |dv| <= |up_scale| eA + 1.01 u (|accA up_scale| + |v|)                          (the epilogue's rule)
    acc  = v + the 3x3 conv of the skip tensor, K_B = 9 c0 real terms: the accumulators START from v (registers, or
           acc_init read back from an fp32 tensor, which stores v exactly), so the 3 K_B retained products are added onto a
           value of at most |v| + |dv|: by the n * u rule on the 3 K_B + 1 terms
           |d acc| <= |dv| + eB + 1.01 * 3 K_B u (|v| + |dv|)          (eB = the skip conv's own count, which already
           holds 3 K_B u Ahat_B and the representation terms R + D)
    out  = relu(acc * scale + shift) stored as H2: dense_conv_ref.epilogue with dst_h2_exp.
  All exponents (both sources', both weight buffers') are powers of two folded into up_scale, shift_border and scale by the
  caller: exact, they do not enter.

The fused first DoubleConv (csrc/conv_inc_fused.hip): mid = H2(relu(conv1(x) * s1 + h1)) at the intermediate's exponent, with
    bound_mid = the first conv's bound (H2 operands, 3 K_1 retained products, K_1 = 9 c0) + its epilogue + the H2 destination
    term, exactly what dense_conv_ref.epilogue(dst_h2_exp = e_mid) returns.  The second conv reads the STORED mid: its own
    count is taken at the reference mid, and the intermediate's error enters linearly through the retained products,
    |d acc2| <= own(mid, w2) + (1 + 1.01 * 3 K_2 u) conv(bound_mid, |w2| + 2 l(w2))      (l: dense_conv_ref.h2_rep),
    ReLU is 1-Lipschitz.  Halo pixels of mid outside the frame are the second conv's zero padding.

sfh_frame_to_h2: no arithmetic beyond the split itself - both planes are dense_conv_ref.split_h2's, bit for bit.
    A value beyond the fp16 range at the tensor's exponent saturates to +-65504 (Inf included); a NaN becomes -65504
    (fmaxf(NaN, -65504) = -65504); both raise `overflow`, and `range` receives the bit pattern of |x * 2^e| BEFORE saturation
    (an Inf reads 0x7F800000, a NaN above it).  The fp32 NHWC4 copy keeps the input's bits.

The stem (csrc/stem.hip) splits its fp32 source itself: S3 (split_arith 0 or SFH_FMT_S3) is exact, H2 carries the
representation error of h2_rep at h2_exp_src - dense_conv_ref.bilinear's 's3' / 'h2' models with K = 49 c0."""
import numpy as np

import dense_conv_ref as R
from dense_conv_ref import (E53, U, bilinear, conv_op, epilogue, h2_rep, pooled, ratio, shifted_copy, split_h2, stem_op,  # noqa: F401
                            up2_op, upscatter)


def border_class(n, up):
    """class of output row / column 0 .. n-1 against an up-sampled extent `up` (include/sfh_amd.h, sfh_compose_up_weights):
    0 the first, 2 the last of the up-sampled tensor, 3 the padded one behind it, 1 everything else"""
    i = np.arange(n)
    return np.where(i == 0, 0, np.where(i == up - 1, 2, np.where(i >= up, 3, 1)))


def up_tables(case, us, sb):
    """up_scale and shift_border as the output pixel sees them -> (us_d, sb_d), both (H,W,cout): output (y, x) takes virtual
    cout ((y & 1) * 2 + (x & 1)) * cout + co and border class 4 * class(y) + class(x)"""
    H, W, C = case.H, case.W, case.cout
    q = (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)
    cls = 4 * border_class(H, 2 * case.h1)[:, None] + border_class(W, 2 * case.w1)[None, :]
    cov = q[..., None] * C + np.arange(C)
    return np.asarray(us, np.float64)[cov], np.asarray(sb, np.float64)[cls[..., None], cov]


def upfused(case, inp, scale, shift, relu, wexp_up, wexp_sk):
    """the fp64 value and bound of the fused Up block's first conv -> dict accA, v, ev (the seed and its bound, destination
    layout), accB, acc, A (largest absolute partial sum), y, bound"""
    Hc, Wc = case.h1 + (case.H - 2 * case.h1), case.w1 + (case.W - 2 * case.w1)
    low, skip = inp["low"][..., :case.c1], inp["skip"][..., :case.c0]
    a, Aa, ea = bilinear(up2_op(Hc, Wc), low, inp["wq"], 4 * case.c1, "h2", case.e_src, wexp_up)
    crop = lambda t: upscatter(t)[:, :case.H, :case.W]
    accA, AA, eA = crop(a), crop(Aa), crop(ea)
    us_d, sb_d = up_tables(case, inp["us"], inp["sb"])
    pA = accA * us_d
    v = pA + sb_d
    ev = np.abs(us_d) * eA + (1.01 * U + 2 * E53) * (np.abs(pA) + np.abs(v) * (sb_d != 0)) * (us_d != 0)
    accB, AB, eB = bilinear(conv_op(3), skip, inp["w"], 9 * case.c0, "h2", case.e_src, wexp_sk)
    acc = v + accB
    eacc = ev + eB + 1.01 * 3 * 9 * case.c0 * U * (np.abs(v) + ev) * (AB > 0) + 2 * E53 * np.abs(acc)
    y, bound = epilogue(acc, eacc, scale, shift, None, relu, dst_h2_exp=case.e_dst)
    return dict(accA=accA, v=v, ev=ev, accB=accB, acc=acc, A=AA * np.abs(us_d) + np.abs(sb_d) + AB, y=y, bound=bound)


def up_shifted_copy(case, low, c, ov, ky, kx):
    """what the composed conv's weight with a single 1 at (virtual cout ov, c, ky, kx) must leave in the destination (up_scale
    1, a zero border table): quadrant q = ov // cout = (py, px), channel co = ov % cout of output (2Y + py, 2X + px) =
    low[Y + py - 1 + ky][X + px - 1 + kx][c], zero where that pixel lies outside the low-resolution tensor -> (B,H,W,cout)"""
    q, co = divmod(ov, case.cout)
    py, px = q >> 1, q & 1
    out = np.zeros((case.B, case.H, case.W, case.cout))
    for y in range(py, case.H, 2):
        sy = (y >> 1) + py - 1 + ky
        if not 0 <= sy < case.h1:
            continue
        for x in range(px, case.W, 2):
            sx = (x >> 1) + px - 1 + kx
            if 0 <= sx < case.w1:
                out[:, y, x, co] = low[:, sy, sx, c]
    return out


def first_layer(case, inp, scale, shift, relu, wexp):
    """sfh_conv3x3_c4h2_fwd (H2 operands at e_src / wexp) or sfh_conv3x3_c4_fwd (fp32) -> dict acc, A, y, bound"""
    ar = "h2" if case.kern == "c4h2" else "f32"
    acc, A, eacc = bilinear(conv_op(3), inp["x"], inp["w"], 9 * case.c0, ar, case.e_src, wexp)
    y, bound = epilogue(acc, eacc, scale, shift, None, relu, dst_h2_exp=case.e_dst if case.dst == "h2" else None)
    return dict(acc=acc, A=A, y=y, bound=bound)


def inc_fused(case, inp, scale, shift, relu, wexp1, wexp2):
    """the fp64 DoubleConv with the intermediate's H2 rounding carried through -> dict mid, bound_mid, acc, A, y, bound and, with
    case.pool, pool / pool_bound"""
    a1, A1, e1 = bilinear(conv_op(3), inp["x"], inp["w1"], 9 * case.c0, "h2", case.e_frame, wexp1)
    mid, bmid = epilogue(a1, e1, inp["s1"], inp["h1"], None, bool(case.relu), dst_h2_exp=case.e_mid)
    K2 = 9 * 64
    a2, A2, own = bilinear(conv_op(3), mid, inp["w2"], K2, "h2", case.e_mid, wexp2)
    w2 = np.abs(np.asarray(inp["w2"], np.float64))
    carried = conv_op(3)(bmid, w2 + 2 * h2_rep(w2, wexp2)[1]) * (1 + 1.01 * 3 * K2 * U)
    y, bound = epilogue(a2, own + carried, scale, shift, None, relu, dst_h2_exp=case.e_dst)
    out = dict(a1=a1, A1=A1, mid=mid, bound_mid=bmid, acc=a2, A=A2, y=y, bound=bound)
    if case.pool:
        out["pool"], out["pool_bound"] = pooled(y, bound)
    return out


def stem(case, inp, scale, shift, relu, wexp):
    """sfh_stem7x7_fwd: the 7x7 stride-2 conv over channels [0, c0) in the S3 or the H2 arithmetic -> dict acc, A, y, bound"""
    ar = "h2" if case.arith == 2 else "s3"
    acc, A, eacc = bilinear(stem_op, inp["x"][..., :case.c0], inp["w"], 49 * case.c0, ar, case.e_src, wexp)
    y, bound = epilogue(acc, eacc, scale, shift, None, relu)
    return dict(acc=acc, A=A, y=y, bound=bound)


def range_word_limits(y, bound, e):
    """an H2 destination's range word lies within the element bound of max |y| 2^e"""
    return float((np.abs(y) - bound).max()) * 2.0 ** e, float((np.abs(y) + bound).max()) * 2.0 ** e


def frame_to_h2(x, e):
    """(B,C,H,W) float32 -> (planes (B,H,W,2,4) as fp32 values of the fp16 planes, nhwc4 (B,H,W,4) float32, range word bits,
    overflow) per the header: channels >= C are +0"""
    B, C, H, W = x.shape
    nhwc = np.zeros((B, H, W, 4), np.float32)
    nhwc[..., :C] = np.transpose(x, (0, 2, 3, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        u = (nhwc * np.float32(2.0 ** e)).astype(np.float32)
        p0, p1 = split_h2(np.where(np.isnan(nhwc), np.float32(-np.inf), nhwc), e)
    bits = (u.view(np.uint32) & 0x7FFFFFFF)
    word = int(bits.max())
    return np.stack([p0, p1], axis=3), nhwc, word, int(word > 0x477FE000)
