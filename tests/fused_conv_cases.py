"""The cases of the specialised convolution launches, shared by tests/test_fused_conv_host.py (numpy restatements) and
tests/test_gpu_fused_conv.py (the kernels): sfh_conv_upfused_fwd and the two launches it replaces (csrc/conv_upfused.hip,
csrc/conv_s3.hip with shift_border / acc_init), sfh_conv3x3_c4h2_fwd / sfh_conv3x3_c4_fwd / sfh_frame_to_h2
(csrc/conv_c4h2.hip, csrc/conv_mfma.hip), sfh_conv_inc_fused_fwd (csrc/conv_inc_fused.hip) and sfh_stem7x7_fwd
(csrc/stem.hip).  Plain numpy; nothing here imports the library.  Names come from the kernels' own constants (tiles, stage
widths, stored channels), as in tests/dense_conv_cases.py, whose generators and plane-walk constants are used as they are."""
from collections import namedtuple

import numpy as np

import dense_conv_cases as K

GUARD = K.GUARD
UP_TILE = (16, 32)                      # conv_upfused.hip: TH x TW output pixels, a wave = one output parity class
C4_TILE = (8, 32)                       # conv_c4h2.hip / conv3x3_c4_kernel / conv_inc_fused.hip, flat row space
STEM_TILE = {8: (8, 32), 16: (8, 16)}   # stem.hip: output pixels of the 8- and the 16-channel instance, per image
SCALES = np.array([-1.0, -0.5, 0.25, 0.5, 1.0, 2.0], dtype=np.float32)


def _rng(name, salt):
    return K._rng(name, salt)


def _randn_split(r, shape):
    """randn * exp(randn): what a split operand is tested with"""
    return (r.standard_normal(shape) * np.exp(r.standard_normal(shape))).astype(np.float32)


def _ints(r, shape, hi):
    return r.integers(-hi, hi + 1, shape).astype(np.float32)


def _median_shift(acc, scale, frac):
    """minus the per-channel median of acc * scale, rounded down to an integer, + frac: about half of the activated outputs
    fall below zero and none lies within rounding of it"""
    C = acc.shape[-1]
    return (np.floor(-np.median((acc * scale.astype(np.float64)).reshape(-1, C), axis=0)) + frac).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the fused Up block
# skip (B,H,W,cs0 = c0 + 32) and low (B,h1,w1,cs1 = c1 + 32) H2 at e_src, dst (B,H,W,cout + 32) H2 at e_dst; H in {2 h1,
# 2 h1 + 1}, W alike.  The extra stage of both sources holds non-zero junk, the extra words of dst must keep the sentinel.
Up = namedtuple("Up", "name B H W h1 w1 c0 c1 cout relu e_src e_dst")
# one under / one over the 16 x 32 tile each way; the padded row / column (class 3) on either axis alone; degenerate maps
UP_FRAMES = [(16, 32, 8, 16), (15, 31, 7, 15), (17, 33, 8, 16), (18, 34, 9, 17), (16, 33, 8, 16), (17, 32, 8, 16),
             (2, 2, 1, 1), (3, 3, 1, 1), (2, 35, 1, 17), (19, 2, 9, 1)]


def _up_cases():
    out = []
    for i, (H, W, h1, w1) in enumerate(UP_FRAMES):
        out.append(Up(f"up_{H}x{W}", 2 if i < 4 else 1, H, W, h1, w1, (32, 96)[i % 2], (32, 64)[(i // 2) % 2],
                      (64, 128)[i % 4 in (1, 2)], int(i % 3 == 0), (2, 0)[i % 2], (2, 0, 1)[i % 3]))
    # 12 tiles: 4 dead workgroups per cout block in the grid padded to 8; source, destination and both weight exponents differ
    out.append(Up("up_17x33_b3", 3, 17, 33, 8, 16, 96, 64, 128, 1, 1, 3))
    assert len({c.name for c in out}) == len(out)
    return out


UP = _up_cases()
UP_IMPULSE = [Up("up_imp_18x34", 2, 18, 34, 9, 17, 96, 64, 128, 0, 2, 2), Up("up_imp_17x33", 1, 17, 33, 8, 16, 64, 32, 64, 0, 0, 2)]
UP_WALK = [Up("up_walk_17x33", 2, 17, 33, 8, 16, 64, 64, 128, 0, 2, 2), Up("up_walk_18x34_e0", 1, 18, 34, 9, 17, 64, 64, 128, 0, 0, 0)]


def up_frame(case):
    """the conv frame of the composed 2x2 conv: the low-resolution source plus the padded row / column"""
    return case.h1 + (case.H - 2 * case.h1), case.w1 + (case.W - 2 * case.w1)


def up_inputs(case, kind):
    """-> dict skip, low, w (cout,c0,3,3), wq (4*cout,c1,2,2: four independent quadrant blocks), us (4*cout: up_scale),
    sb (16,4*cout: a full random border table, every class its own value).  'randn': split-operand inputs, us from SCALES, sb
    standard normal.  'int': |x| <= 3, |w| <= 2, us in {-2,-1,1,2}, sb integers: v = accA * us + sb and v + accB are integers"""
    r = _rng(case.name, 11 if kind == "randn" else 12)
    sk, lo = (case.B, case.H, case.W, case.c0 + 32), (case.B, case.h1, case.w1, case.c1 + 32)
    ws, wqs = (case.cout, case.c0, 3, 3), (4 * case.cout, case.c1, 2, 2)
    if kind == "int":
        d = dict(skip=_ints(r, sk, 3), low=_ints(r, lo, 3), w=_ints(r, ws, 2), wq=_ints(r, wqs, 2),
                 us=r.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), 4 * case.cout),
                 sb=_ints(r, (16, 4 * case.cout), 40))
    else:
        d = dict(skip=_randn_split(r, sk), low=_randn_split(r, lo),
                 w=(r.standard_normal(ws) / np.sqrt(9 * case.c0)).astype(np.float32),
                 wq=(r.standard_normal(wqs) / np.sqrt(4 * case.c1)).astype(np.float32),
                 us=r.choice(SCALES, 4 * case.cout), sb=r.standard_normal((16, 4 * case.cout)).astype(np.float32))
    d["skip"][..., case.c0:] = 1000.0 + np.arange(32, dtype=np.float32)
    d["low"][..., case.c1:] = 500.0 + np.arange(32, dtype=np.float32)
    return d


def up_epilogue(case, acc, kind):
    """scale / shift of the skip-half conv's epilogue over acc = v + accB (B,H,W,cout).  'randn': SCALES with channel 1 at 0.
    'int': {-2,-1,-0.5,0.5,1,2} with channel 1 at 0 and shifts of an integer + 0.25: acc * scale is a multiple of 0.5, so
    |pre-ReLU| >= 0.25 everywhere and every step is exact"""
    r = _rng(case.name, 13)
    if kind == "int":
        scale = r.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], dtype=np.float32), case.cout)
    else:
        scale = r.choice(SCALES, case.cout)
    scale[1] = 0.0
    shift = _median_shift(acc, scale, 0.25 if kind == "int" else 0.5)
    return scale, shift


def up_impulses(case):
    """yields (half, w, wq, o, c, ky, kx): a single 1 at every tap - 'up': all 4 taps of all 4 quadrants (o = the virtual cout),
    'skip': all 9 taps - for the first and last (cout, channel) of the first and last cout block and K stage; the other half's
    weights are zero"""
    ws, wqs = (case.cout, case.c0, 3, 3), (4 * case.cout, case.c1, 2, 2)
    co = sorted({0, 63, case.cout - 64, case.cout - 1})
    for o, c in sorted({(co[0], 0), (co[1], case.c1 - 1), (co[-2], 31 % case.c1), (co[-1], case.c1 - 32)}):
        for q in range(4):
            for t in range(4):
                wq = np.zeros(wqs, np.float32)
                wq[q * case.cout + o, c, t >> 1, t & 1] = 1.0
                yield "up", np.zeros(ws, np.float32), wq, q * case.cout + o, c, t >> 1, t & 1
    for o, c in sorted({(co[0], 0), (co[1], case.c0 - 1), (co[-2], 31), (co[-1], case.c0 - 32)}):
        for t in range(9):
            w = np.zeros(ws, np.float32)
            w[o, c, t // 3, t % 3] = 1.0
            yield "skip", w, np.zeros(wqs, np.float32), o, c, t // 3, t % 3


# ------------------------------------------------------------------------------------------------ the first layer
# kern 'c4h2' (sfh_conv3x3_c4h2_fwd: FH2 frame source at e_src, H2 arithmetic) or 'c4' (sfh_conv3x3_c4_fwd: fp32 NHWC4, fp32
# arithmetic); dst 'f32', 'h2' or 's3' (what each launcher accepts), dst_cs = cout + 32
C4 = namedtuple("C4", "name kern B H W c0 cout dst e_src e_dst")
# one under / one over the 8 x 32 tile; three frames inside one tile; degenerate maps; odd rows per frame
C4_FRAMES = [(1, 7, 31), (1, 9, 33), (3, 5, 6), (2, 1, 1), (2, 1, 37), (2, 9, 1), (2, 45, 80)]
C4_DST = {"c4h2": ("h2", "f32"), "c4": ("f32", "s3", "h2")}


def _c4_cases():
    out, n = [], 0
    for kern in ("c4h2", "c4"):
        for (B, H, W) in C4_FRAMES:
            for dst in C4_DST[kern]:
                out.append(C4(f"{kern}_{B}x{H}x{W}_{dst}", kern, B, H, W, (1, 3, 4)[n % 3], (64, 128)[(n // 3) % 2], dst,
                              (2, 0, -3)[n % 3] if kern == "c4h2" else 0, (2, 0)[n % 2]))
                n += 1
    return out


C4S = _c4_cases()
C4_IMPULSE = [C4(f"{k}_imp", k, 2, 9, 33, 4, 128, "f32", 2 if k == "c4h2" else 0, 2) for k in ("c4h2", "c4")] + \
             [C4("c4h2_imp_3frames", "c4h2", 3, 5, 6, 3, 64, "h2", 0, 2)]
C4_WALK = [C4("c4h2_walk", "c4h2", 2, 9, 33, 4, 128, "f32", 2, 2), C4("c4h2_walk_e0", "c4h2", 3, 5, 6, 3, 64, "h2", 0, 2)]


def c4_inputs(case, kind):
    """-> dict x (B,H,W,c0) NHWC real channels (the test stores them as 4, the rest zero), w (cout,c0,3,3)"""
    r = _rng(case.name, 21 if kind == "randn" else 22)
    xs, ws = (case.B, case.H, case.W, case.c0), (case.cout, case.c0, 3, 3)
    if kind == "int":
        return dict(x=_ints(r, xs, 3), w=_ints(r, ws, 2))
    x = _randn_split(r, xs) if case.kern == "c4h2" else r.standard_normal(xs).astype(np.float32)
    return dict(x=x, w=(r.standard_normal(ws) / np.sqrt(9 * case.c0)).astype(np.float32))


def plain_epilogue(name, acc, kind, unit=1.0):
    """scale / shift of a launch without residual over acc (..., C).  'randn': K.epilogue_inputs' choices - SCALES with channel
    1 at 0, a shift of minus the median + 0.5.  'int' (acc a multiple of `unit`, 1 or 0.5): scales s with s * unit a multiple of
    0.5, channel 1 at 0, shifts of an integer + 0.25: |pre-ReLU| >= 0.25 everywhere and every step is exact"""
    C = acc.shape[-1]
    r = _rng(name, 23)
    if kind == "int":
        pick = np.array([s for s in (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0) if (s * unit * 2.0) % 1.0 == 0.0], dtype=np.float32)
        scale = r.choice(pick, C)
    else:
        scale = r.choice(SCALES, C)
    scale[1] = 0.0
    return scale, _median_shift(acc, scale, 0.25 if kind == "int" else 0.5)


def impulse_oc(cout, cin):
    """the first and last (cout, channel) of the first and last cout block"""
    return sorted({(0, 0), (63 % cout, cin - 1), (cout - 64, cin // 2), (cout - 1, cin - 1), (cout - 1, 0)})


# ------------------------------------------------------------------------------------------------ sfh_frame_to_h2
F2H = namedtuple("F2H", "name B C H W e")
# pixel counts 1, 255, 257 (one under / over the 256-thread block) and 2 * 45 * 80
F2HS = [F2H(f"f2h_{B}x{C}x{H}x{W}_e{e}", B, C, H, W, e)
        for n, (B, H, W) in enumerate(((1, 1, 1), (1, 15, 17), (1, 1, 257), (2, 45, 80)))
        for C in (1, 3, 4) for e in ((-3, 0, 2) if n == 1 else ((-3, 0, 2)[(n + C) % 3],))]


def f2h_input(case):
    """(B,C,H,W) over 30 binades, all inside the fp16 range at the case's exponent, with +-0 and a plane-1 subnormal"""
    r = _rng(case.name, 31)
    shape = (case.B, case.C, case.H, case.W)
    x = (r.standard_normal(shape) * np.exp(r.uniform(-12, 8, shape))).astype(np.float32)
    x = np.clip(x, -60000.0 * 2.0 ** -case.e, 60000.0 * 2.0 ** -case.e).astype(np.float32)
    flat = x.reshape(-1)
    for i, v in enumerate((0.0, -0.0, 2.0 ** -30, 1.0)[:flat.size]):
        flat[i] = v
    return x


# ------------------------------------------------------------------------------------------------ the fused first DoubleConv
# the frames of the first layer; c0 in {3, 4}; pool: dst_pool (floor of odd sizes); rev: reverse_tiles
Inc = namedtuple("Inc", "name B H W c0 pool rev e_frame e_mid e_dst relu")


def _inc_cases():
    out = []
    for n, (B, H, W) in enumerate(C4_FRAMES):
        out.append(Inc(f"inc_{B}x{H}x{W}", B, H, W, (3, 4)[n % 2], 0, n % 3 == 1, (2, 0, 1)[n % 3], (2, 1, 3)[n % 3], (2, 0)[n % 2], 1))
    out.append(Inc("inc_2x45x80_pool", 2, 45, 80, 3, 1, 0, 2, 2, 2, 1))
    out.append(Inc("inc_1x9x33_pool_rev", 1, 9, 33, 4, 1, 1, 1, 0, 3, 1))
    out.append(Inc("inc_2x45x80_rev", 2, 45, 80, 4, 0, 1, 0, 2, 1, 1))
    return out


INC = _inc_cases()
INC_IMPULSE = [Inc("inc_imp", 2, 9, 33, 4, 1, 0, 2, 2, 2, 0), Inc("inc_imp_3frames", 3, 5, 6, 3, 0, 1, 0, 0, 2, 0)]
INC_WALK = [Inc("inc_walk", 2, 9, 33, 4, 0, 0, 2, 2, 2, 0), Inc("inc_walk_e0", 3, 5, 6, 3, 0, 0, 0, 0, 0, 0)]


def inc_inputs(case, kind):
    """-> dict x (B,H,W,c0), w1 (64,c0,3,3), w2 (64,64,3,3), s1 / h1 (the first conv's scale / shift).  'int': |x| <= 3,
    |w1| <= 2, s1 in {1, 2} and h1 an integer + 0.5: the intermediate's pre-ReLU value is an integer + 0.5 (never within
    rounding of zero), the intermediate a multiple of 0.5 of at most 9 * 4 * 6 * 2 + 4.5 (exact in its first fp16 plane at
    every exponent used); |w2| <= 1: the second accumulator is a multiple of 0.5"""
    r = _rng(case.name, 41 if kind == "randn" else 42)
    xs, w1s, w2s = (case.B, case.H, case.W, case.c0), (64, case.c0, 3, 3), (64, 64, 3, 3)
    if kind == "int":
        return dict(x=_ints(r, xs, 3), w1=_ints(r, w1s, 2), w2=_ints(r, w2s, 1),
                    s1=r.choice(np.array([1.0, 2.0], dtype=np.float32), 64), h1=_ints(r, (64,), 4) + np.float32(0.5))
    return dict(x=_randn_split(r, xs), w1=(r.standard_normal(w1s) / np.sqrt(9 * case.c0)).astype(np.float32),
                w2=(r.standard_normal(w2s) / np.sqrt(9 * 64)).astype(np.float32), s1=r.choice(SCALES, 64),
                h1=(0.5 * r.standard_normal(64)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the stem
# arith: 0 (split_arith 0 = S3), 1 (SFH_FMT_S3), 2 (SFH_FMT_H2, at e_src); cs0 8: the narrow instance, 12 / 16: the wide one
Stem = namedtuple("Stem", "name B H W c0 cs0 arith e_src dst_cs relu")


def _stem_cases():
    out, n = [], 0
    frames = {8: [], 16: []}
    for cs, sizes in ((8, ((7, 31), (9, 33))), (16, ((7, 15), (9, 17)))):
        for ho, wo in sizes:              # one under / over the tile, from an odd and from an even input size
            frames[cs] += [(2 * ho - 1, 2 * wo - 1), (2 * ho, 2 * wo)]
        frames[cs] += [(1, 1), (1, 37), (9, 1)]
    chans = {8: ((1, 8), (5, 8), (8, 8)), 16: ((9, 12), (12, 12), (13, 16), (16, 16))}
    for cs in (8, 16):
        for (H, W) in frames[cs]:
            for arith, e in ((0, 0), (1, 0), (2, 0), (2, 2)):
                c0, cs0 = chans[cs][n % len(chans[cs])]
                out.append(Stem(f"stem{cs}_{H}x{W}_a{arith}e{e}", 3, H, W, c0, cs0, arith, e, (64, 96)[n % 2], (n // 2) % 2))
                n += 1
    return out


STEM = _stem_cases()
STEM_IMPULSE = [Stem("stem8_imp", 2, 17, 65, 5, 8, 2, 2, 64, 0), Stem("stem8_imp_s3", 2, 18, 66, 8, 8, 1, 0, 64, 0),
                Stem("stem16_imp", 2, 17, 33, 9, 12, 2, 0, 64, 0), Stem("stem16_imp_s3", 2, 18, 34, 13, 16, 0, 0, 64, 0)]
STEM_WALK = [Stem("stem8_walk_s3", 2, 17, 65, 8, 8, 1, 0, 64, 0), Stem("stem8_walk_h2", 2, 18, 66, 5, 8, 2, 2, 64, 0),
             Stem("stem16_walk_s3", 2, 17, 33, 12, 12, 0, 0, 64, 0), Stem("stem16_walk_h2", 2, 18, 34, 16, 16, 2, 0, 64, 0)]


def stem_fmt(case):
    return "h2" if case.arith == 2 else "s3"


def stem_out_hw(case):
    return (case.H - 1) // 2 + 1, (case.W - 1) // 2 + 1


def stem_inputs(case, kind):
    """-> dict x (B,H,W,cs0) with the stored channels beyond c0 zero (as sfh_nchw_to_nhwc leaves them), w (64,c0,7,7)"""
    r = _rng(case.name, 51 if kind == "randn" else 52)
    xs, ws = (case.B, case.H, case.W, case.cs0), (64, case.c0, 7, 7)
    if kind == "int":
        x, w = _ints(r, xs, 3), _ints(r, ws, 2)
    else:
        x, w = _randn_split(r, xs), (r.standard_normal(ws) / np.sqrt(49 * case.c0)).astype(np.float32)
    x[..., case.c0:] = 0.0
    return dict(x=x, w=w)
