"""The cases of the dense convolution launches, shared by tests/test_dense_conv_host.py (numpy restatements) and
tests/test_gpu_dense_conv.py (the kernels).  Plain numpy; nothing here imports the library.  Names come from the kernels'
own constants (tile ids of include/sfh_amd.h, stage widths, pack modes), not from the workload."""
from collections import namedtuple

import numpy as np

GUARD = 64          # elements behind every output buffer that no kernel may touch
H2_ACT_EXP = 2
# SFH_TILE_* -> (TH, TW) at stride 1; the fp32 kernel halves TH at stride 2, the split kernel keeps it (tiles 3, 4 only)
TILES = {0: (8, 32), 1: (16, 16), 2: (32, 8), 3: (8, 16), 4: (16, 8)}
SMALL_TILE = (12, 20)   # sfh_conv_small_fwd

# kern: 'f32' (sfh_conv_fwd), 's3' / 'h2' (sfh_conv_s3_fwd), 'small' (sfh_conv_small_fwd, H2).  H, W: the conv frame.
# mode: the pack mode (0 conv, 1 transposed + up-scatter, 2 the 7x7 s2 stem as ksize 4, 3 / 4 backward-data).
# c1 > 0: a second source of (H - 1) x (W - 1) at pad1.  aux: the pack argument of modes 2, 3, 4.
# flags: pool0, dst_pool, res (residual of the destination's format), res_f32 (fp32 residual beside a split destination),
#        split (destination in the sources' format), rev (reverse_tiles), wg128 (wg_couts = 128), junk (cs0 = c0 + 32 / + 16)
Fwd = namedtuple("Fwd", "name kern B H W ks stride tile c0 c1 pad1 cout dst_cs mode aux flags")


def fwd(name, kern, B, H, W, ks=3, stride=1, tile=0, c0=None, c1=0, pad1=(0, 0), cout=64, dst_cs=None, mode=0, aux=0,
        flags=()):
    if c0 is None:
        c0 = 16 if kern == "f32" else 32
    creal = cout // 4 if (mode == 1 or ks == 2) else cout    # up-scatter: cout counts the four quadrants' virtual channels
    return Fwd(name, kern, B, H, W, ks, stride, tile, c0, c1, pad1, cout, dst_cs or creal, mode, aux, frozenset(flags))


def is_up(case):
    """SFH_OUT_UPSCATTER2: the transposed conv (pack mode 1, ksize 1) or the 2x2 up-scatter conv (pack mode 0, ksize 2)"""
    return case.mode == 1 or case.ks == 2


def dst_hw(case):
    """rows and columns of the destination; 'short' (ksize 2): the source is one row and column short of the conv frame and
    the destination one short of 2H x 2W (up_dst_h / up_dst_w)"""
    ho, wo = out_hw(case)
    if not is_up(case):
        return ho, wo
    s = 1 if "short" in case.flags else 0
    return 2 * ho - s, 2 * wo - s


def arith(case):
    return "h2" if case.kern == "small" else case.kern


def tile_hw(kern, tile, stride):
    th, tw = SMALL_TILE if kern == "small" else TILES[tile]
    return (th // 2 if (stride == 2 and kern == "f32") else th), tw


def out_hw(case):
    n = lambda v: (v + case.ks // 2 + (case.ks - 1) // 2 - case.ks) // case.stride + 1
    return n(case.H), n(case.W)


def cs0(case):
    """stored channels of source 0: c0, rounded up to the launcher's rule for the fp32 kernel (below 16, or a multiple of
    16); 'junk' adds a whole stage of channels the conv must ignore"""
    cs = case.c0
    if case.kern == "f32" and cs > 16:
        cs = -(-cs // 16) * 16
    if "junk" in case.flags:
        cs += 16 if case.kern == "f32" else 32
    return cs


def K_terms(case):
    """real terms of one output"""
    if case.mode == 2:
        return 49 * case.aux
    return case.ks * case.ks * (case.c0 + case.c1)


def _fwd_cases():
    out = []
    # --- one under and one over every tile shape, at both strides
    for kern, tiles in (("f32", (0, 1, 2)), ("s3", (0, 1, 2, 3, 4)), ("h2", (0, 1, 2, 3, 4))):
        for t in tiles:
            for s in (1, 2):
                if s == 2 and kern != "f32" and t < 3:
                    continue            # the split kernel takes stride 2 on the half-size tiles only
                th, tw = tile_hw(kern, t, s)
                for d in (-1, 1):
                    ho, wo = th + d, tw + d
                    H, W = (ho, wo) if s == 1 else (2 * ho - 1, 2 * wo)
                    out.append(fwd(f"{kern}_tile{t}_s{s}_{ho}x{wo}", kern, 1, H, W, stride=s, tile=t))
    out += [fwd(f"small_{h}x{w}", "small", 1, h, w) for h, w in ((11, 19), (13, 21))]
    # --- degenerate maps; three frames inside one tile of the flattened row space; stride 2 on odd and even frames
    for kern in ("f32", "s3", "h2", "small"):
        out += [fwd(f"{kern}_map{h}x{w}", kern, 2, h, w) for h, w in ((1, 1), (1, 37), (9, 1))]
        out.append(fwd(f"{kern}_3frames_H5", kern, 3, 5, 6))
        out.append(fwd(f"{kern}_2x45x80", kern, 2, 45, 80, c0=64 if kern != "f32" else 48))
    for kern, t in (("f32", 0), ("f32", 2), ("s3", 3), ("h2", 4)):
        out += [fwd(f"{kern}_s2_{h}x{w}_tile{t}", kern, 2, h, w, stride=2, tile=t) for h, w in ((23, 41), (24, 40))]
        out.append(fwd(f"{kern}_k1_s2_tile{t}", kern, 2, 23, 41, ks=1, stride=2, tile=t, c0=32))
    # --- channels
    for c in (8, 12, 16, 24, 48, 64):          # cs0 < 16; whole stages; 24: a remainder of the 16-wide stage of ksize 3
        out.append(fwd(f"f32_c{c}", "f32", 2, 7, 9, c0=c))
    out.append(fwd("f32_k1_c48", "f32", 2, 7, 9, ks=1, c0=48))      # a remainder of the 32-wide stage of ksize 1
    out.append(fwd("f32_k1_c64", "f32", 2, 7, 9, ks=1, c0=64))
    out.append(fwd("f32_k4_c16", "f32", 2, 7, 9, ks=4, c0=16))      # pack mode 0 at ksize 4: padding 2 before, 1 after
    for kern in ("s3", "h2"):
        out.append(fwd(f"{kern}_c96", kern, 2, 7, 9, c0=96))        # three K stages
        out.append(fwd(f"{kern}_k1_c96", kern, 2, 7, 9, ks=1, c0=96))
    out.append(fwd("small_c96", "small", 2, 7, 9, c0=96))
    for kern in ("f32", "s3", "h2", "small"):
        out.append(fwd(f"{kern}_junk", kern, 2, 7, 9, flags=("junk",)))
        for co in (128, 192):
            out.append(fwd(f"{kern}_cout{co}", kern, 1, 7, 9, cout=co))
        out.append(fwd(f"{kern}_dstcs", kern, 2, 7, 9, dst_cs=96))
        if kern != "f32":
            out.append(fwd(f"{kern}_dstcs_split", kern, 2, 7, 9, dst_cs=96, flags=("split",)))
    for kern, c0, c1 in (("f32", 64, 64), ("s3", 64, 32), ("h2", 64, 32)):
        for pad in ((0, 0), (0, 1), (1, 0), (1, 1)):
            out.append(fwd(f"{kern}_two_pad{pad[0]}{pad[1]}", kern, 2, 7, 9, c0=c0, c1=c1, pad1=pad))
    out.append(fwd("h2_wg128", "h2", 2, 9, 33, c0=128, cout=256, flags=("wg128",)))
    out.append(fwd("h2_wg64_same", "h2", 2, 9, 33, c0=128, cout=256))
    # --- modes
    out.append(fwd("f32_pool0", "f32", 2, 7, 9, c0=16, flags=("pool0",)))
    out.append(fwd("f32_res_relu", "f32", 2, 7, 9, flags=("res",)))
    for kern in ("s3", "h2"):
        for t in (0, 2):       # 1x16 pixel groups pool across tile rows, 2x8 groups inside a lane pair
            out.append(fwd(f"{kern}_dst_pool_tile{t}", kern, 2, 9, 11, tile=t, flags=("dst_pool",)))
            out.append(fwd(f"{kern}_dst_pool_split_tile{t}", kern, 2, 9, 11, tile=t, flags=("dst_pool", "split")))
        out.append(fwd(f"{kern}_res_f32dst", kern, 2, 7, 9, flags=("res",)))
        out.append(fwd(f"{kern}_res_split", kern, 2, 7, 9, flags=("res", "split")))
        out.append(fwd(f"{kern}_res_f32_beside_split", kern, 2, 7, 9, flags=("res_f32", "split")))
        out.append(fwd(f"{kern}_rev", kern, 2, 19, 35, flags=("rev",)))
    out.append(fwd("small_res_split", "small", 2, 13, 21, flags=("res", "split")))
    out.append(fwd("small_res_f32dst", "small", 2, 13, 21, flags=("res",)))
    for kern in ("f32", "s3", "h2"):
        out.append(fwd(f"{kern}_mode1_up", kern, 2, 5, 7, ks=1, c0=64, cout=256, mode=1))
        for aux in (7, 8):
            out.append(fwd(f"{kern}_mode2_aux{aux}", kern, 2, 6, 9, ks=4, c0=32, mode=2, aux=aux))
        out.append(fwd(f"{kern}_mode3_k3", kern, 2, 7, 9, c0=64, mode=3, aux=40))
        out.append(fwd(f"{kern}_mode3_k1", kern, 2, 7, 9, ks=1, c0=64, mode=3, aux=40))
        out.append(fwd(f"{kern}_mode4", kern, 2, 5, 7, ks=1, c0=64, mode=4, aux=16))
    # the 2x2 up-scatter conv of sfh_conv_s3_fwd (pack mode 0, ksize 2, four quadrants): plain, and with the source one row
    # and column short of the frame and the destination one short of 2H x 2W (up_dst_h / up_dst_w)
    for kern in ("s3", "h2"):
        out.append(fwd(f"{kern}_k2_up", kern, 2, 5, 7, ks=2, c0=32, cout=256))
        out.append(fwd(f"{kern}_k2_up_short", kern, 2, 5, 7, ks=2, c0=64, cout=256, flags=("short",)))
        out.append(fwd(f"{kern}_k2_up_short_tile2", kern, 2, 9, 5, ks=2, tile=2, c0=32, cout=256, flags=("short",)))
        out.append(fwd(f"{kern}_k2_up_short_split_resf32", kern, 2, 5, 7, ks=2, c0=32, cout=256,
                       flags=("short", "split", "res_f32")))
    assert len({c.name for c in out}) == len(out)
    return out


FWD = _fwd_cases()
# where the impulse family runs: a tile seam in both directions, two frames, a stride-2 map, two sources, three couts
# blocks and K stages; the small-map kernel; backward-data
IMPULSE = [fwd("f32_imp", "f32", 2, 9, 33, c0=32, cout=192), fwd("f32_imp_s2", "f32", 1, 10, 35, stride=2, c0=16),
           fwd("f32_imp_two", "f32", 1, 6, 7, c0=16, c1=16, pad1=(1, 0)),
           fwd("f32_imp_k4", "f32", 1, 9, 33, ks=4, c0=16),
           fwd("s3_imp", "s3", 2, 9, 33, c0=96, cout=192), fwd("s3_imp_s2", "s3", 1, 10, 35, stride=2, tile=3),
           fwd("h2_imp", "h2", 2, 9, 33, c0=96, cout=192), fwd("h2_imp_two", "h2", 1, 6, 7, c0=32, c1=32, pad1=(0, 1)),
           fwd("h2_imp_s2", "h2", 1, 10, 35, stride=2, tile=4), fwd("small_imp", "small", 2, 13, 21, c0=64, cout=128)]
IMPULSE_BWD = [fwd(f"{k}_imp_mode3", k, 2, 9, 17, c0=64, mode=3, aux=40, tile=1) for k in ("f32", "s3", "h2")]
IMPULSE_UP2 = [fwd(f"{k}_imp_k2_short", k, 2, 9, 17, ks=2, tile=1, c0=64, cout=256, flags=("short",)) for k in ("s3", "h2")]
# backward-data impulses beyond pack mode 3 at 3x3: mode 3 at 1x1, and modes 1 and 4 (expected values: the reference, exact on integers)
IMPULSE_BWD_REF = [fwd(f"{k}_imp_{n}", k, 2, 5, 7, **kw) for k in ("f32", "s3", "h2") for n, kw in
                   (("mode3_k1", dict(ks=1, c0=64, mode=3, aux=40)), ("mode1", dict(ks=1, c0=64, cout=256, mode=1)),
                    ("mode4", dict(ks=1, c0=64, mode=4, aux=16)))]
PLANE_WALK = [fwd("s3_walk", "s3", 2, 9, 33, c0=64, cout=128), fwd("h2_walk", "h2", 2, 9, 33, c0=64, cout=128),
              fwd("small_walk", "small", 2, 13, 21, c0=64, cout=128), fwd("s3_walk_s2", "s3", 1, 10, 35, stride=2, tile=3)]

# backward-filter: kern 'f32' (sfh_conv_wgrad), 's3' / 'h2' (sfh_conv_wgrad_s3); N1 > 0: a second source of
# (H - 1) x (W - 1) at pad, written to raw at n_off = N; raw_n = N + N1 + 32
Wg = namedtuple("Wg", "name kern B H W ks M N N1 pad")


def _wg_cases():
    out = []
    for kern in ("f32", "s3", "h2"):
        for ks in ((1, 3, 4) if kern == "f32" else (1, 3)):
            n = 32 if ks == 4 else 96
            out.append(Wg(f"{kern}_k{ks}_M64", kern, 2, 5, 37, ks, 64, 32, 0, (0, 0)))       # 2x32 tiles
            out.append(Wg(f"{kern}_k{ks}_M192", kern, 2, 11, 9, ks, 192, n, 0, (0, 0)))       # 4x16 / 8x8 tiles
            if ks != 4:
                for pad in ((0, 0), (1, 1), (0, 1), (1, 0)):
                    out.append(Wg(f"{kern}_k{ks}_two_pad{pad[0]}{pad[1]}", kern, 1, 9, 17, ks, 64, 32, 32, pad))
        out.append(Wg(f"{kern}_k3_1x1", kern, 1, 1, 1, 3, 64, 32, 0, (0, 0)))
        out.append(Wg(f"{kern}_k3_3frames", kern, 3, 5, 6, 3, 64, 32, 0, (0, 0)))
    return out


WGRAD = _wg_cases()


def _rng(name, salt):
    return np.random.default_rng([salt] + [ord(ch) for ch in name])


def wexp_for(w):
    """the exponent sfh_pack_h2_weights expects: max |w| * 2^wexp in [2^13, 2^14)"""
    m = float(np.abs(w).max())
    return 13 - int(np.floor(np.log2(m))) if m > 0 else 0


# ------------------------------------------------------------------------------------------------ inputs
def weight_shape(case):
    if case.mode == 1:
        return (case.c0, case.cout // 4, 2, 2)              # IOHW
    if case.mode == 2:
        return (case.cout, case.aux, 7, 7)
    if case.mode == 3:
        return (case.c0, case.aux, case.ks, case.ks)        # the layer's OIHW: cout = c0 of the launch, cin = aux
    if case.mode == 4:
        return (case.cout, case.aux, 2, 2)                  # IOHW of the transposed conv: cin = cout of the launch
    return (case.cout, case.c0 + case.c1, case.ks, case.ks)


def source_shapes(case):
    """-> (shape of what the test generates for source 0, shape of source 1 or None).  Mode 2: the un-shuffled frame
    (B,2H-1,2W-1,aux rounded up to c0/4 stored); mode 4: dY (B,2H,2W,aux) - both go through sfh_space_to_depth2."""
    B, H, W = case.B, case.H, case.W
    if case.mode == 2:
        return (B, 2 * H - 1, 2 * W - 1, case.c0 // 4), None
    if case.mode == 4:
        return (B, 2 * H, 2 * W, case.aux), None
    if "short" in case.flags:
        return (B, H - 1, W - 1, cs0(case)), None
    s0 = (B, 2 * H + 1, 2 * W + 1, cs0(case)) if "pool0" in case.flags else (B, H, W, cs0(case))
    return s0, ((B, H - 1, W - 1, case.c1) if case.c1 else None)


def _fill(case, kind, shape, r, k):
    if kind == "int":
        return r.integers(-3, 4, shape).astype(np.float32)
    x = r.standard_normal(shape)
    if arith(case) != "f32" and kind == "randn":
        x = x * np.exp(r.standard_normal(shape))
    return x.astype(np.float32)


def fwd_inputs(case, kind):
    """kind 'randn' (randn * exp(randn) for the split formats) or 'int' (|x| <= 3, |w| <= 2: every product and partial sum an
    integer below 2^24 - at most 9 * 160 terms of at most 6 - in every format's first plane)
    -> dict x0, x1, w, res (B,Ho,Wo,cout real), scale, shift.  Stored channels beyond c0 hold non-zero junk."""
    r = _rng(case.name, 1 if kind == "randn" else 2)
    s0, s1 = source_shapes(case)
    x0 = _fill(case, kind, s0, r, 0)
    if case.mode == 2:
        x0[..., case.aux:] = 0.0            # the stem's padded channels are zero by construction (sfh_nchw_to_nhwc)
    elif case.mode == 0 and s0[3] > case.c0:
        x0[..., case.c0:] = 1000.0 + np.arange(s0[3] - case.c0, dtype=np.float32)
    x1 = _fill(case, kind, s1, r, 1) if s1 else None
    ws = weight_shape(case)
    if kind == "int":
        w = r.integers(-2, 3, ws).astype(np.float32)
    else:
        w = (r.standard_normal(ws) / np.sqrt(max(K_terms(case), 1))).astype(np.float32)
    creal = case.cout // 4 if is_up(case) else case.cout
    oshape = (case.B,) + dst_hw(case) + (creal,)
    res = _fill(case, "int" if kind == "int" else "plain", oshape, r, 2)
    return dict(x0=x0, x1=x1, w=w, res=res)


def epilogue_inputs(case, acc):
    """scales from {-1, -0.5, 0.25, 0.5, 1, 2} with channel 1 at exactly 0, and a shift that puts about half of the activated
    outputs below zero (minus the per-channel median of acc * scale, rounded to an integer + 0.5).  On the integer inputs
    every step of the epilogue is then exact in fp32 - the ReLU decision is never within rounding of zero, and the output
    must equal the fp64 value bit for bit -> (scale, shift) float32 per VIRTUAL channel"""
    C = acc.shape[-1]
    r = _rng(case.name, 3)
    scale = r.choice(np.array([-1.0, -0.5, 0.25, 0.5, 1.0, 2.0], dtype=np.float32), C)
    scale[1] = 0.0
    shift = -np.median((acc * scale.astype(np.float64)).reshape(-1, C), axis=0)
    shift = (np.floor(shift) + 0.5).astype(np.float32)
    shift[1] = np.float32(0.25)
    return scale, shift


def pixel_coded(shape):
    """1 + (y * W + x) mod 2039 in every channel: an integer below 2^11 (one fp16 / two bf16 planes hold it)"""
    B, H, W, C = shape
    pix = (np.arange(H * W).reshape(1, H, W, 1) % 2039 + 1).astype(np.float32)
    return np.broadcast_to(pix, shape).copy()


def channel_coded(shape):
    """1 + c at every pixel"""
    return np.broadcast_to(np.arange(1, shape[3] + 1, dtype=np.float32), shape).copy()


def impulse_weights(case):
    """yields (w, o, c, ky, kx): a single 1 at every tap, for the first and last (o, c) of the first and last cout block and
    K stage (the last channel of source 0, the first and last of source 1)"""
    ws = weight_shape(case)
    O, C = ws[0], ws[1]
    last0 = case.c0 - 1 if case.mode == 0 else C - 1        # the last channel of source 0
    for o, c in sorted({(0, 0), (O - 1, C - 1), (0, last0), (O - 1, (last0 + 1) % C), (63 % O, C - 1), (64 % O, 0)}):
        for ky in range(case.ks):
            for kx in range(case.ks):
                w = np.zeros(ws, dtype=np.float32)
                w[o, c, ky, kx] = 1.0
                yield w, o, c, ky, kx


# ------------------------------------------------------------------------------------------------ the plane walk
# S3: v = s * 2^a * (1 + 2^-9 + 2^-18): bf16 keeps 8 significand bits, so plane 0 = 2^a, plane 1 = 2^(a-9), plane 2 = 2^(a-18).
# With a weight of the same structure the full product is 2^(a+b) * (1 + 2^-8 + 3 * 2^-18 + 2^-26 + 2^-36); the six retained
# products sum to 2^(a+b) * (1 + 2^-8 + 3 * 2^-18) - 19 bits, an fp32 number - and the dropped 2^-26 + 2^-36 lies below half an
# ulp (2^-24): the fp64 product rounds to exactly the retained sum.  The smallest retained product is 2^-18 = 32 ulps.
# H2: U = v * 2^e = s * 2^a * (1 + 2^-13), 1 <= 2^a <= 2^4: fp16 keeps 11 bits, plane 0 = 2^a, plane 1 = 2^(a-13) (a normal fp16
# number); the weight 2^b * (1 + 2^-13) alike.  Full product 2^(a+b) * (1 + 2^-12 + 2^-26), retained 1 + 2^-12, dropped 2^-26
# below half an ulp; either cross product is 2^-13 = 1024 ulps.
WALK = {"s3": (1.0 + 2.0 ** -9 + 2.0 ** -18, 1.0 + 2.0 ** -8 + 3 * 2.0 ** -18), "h2": (1.0 + 2.0 ** -13, 1.0 + 2.0 ** -12)}


def walk_values(shape, fmt, salt, exp=H2_ACT_EXP):
    """a tensor of plane-walk values: sign * 2^a * m with a from 0 .. 4 (S3: -2 .. 2) varying with the position; for H2 the
    STORED value v * 2^exp has its leading bit at 2^0 .. 2^4"""
    r = np.random.default_rng([7, salt])
    a = r.integers(0, 5, shape).astype(np.float64) - (2 if fmt == "s3" else exp)
    s = r.choice(np.array([-1.0, 1.0]), shape)
    return (s * 2.0 ** a * WALK[fmt][0]).astype(np.float32)


def walk_weight(fmt):
    """the one non-zero weight: -(1 + ...) * 2^-1 (any power of two does: the H2 packing scales it to 2^13)"""
    return np.float32(-0.5 * WALK[fmt][0])


# ------------------------------------------------------------------------------------------------ backward-filter inputs
def wg_inputs(case, kind):
    """-> dz (B,H,W,M), x0 (B,H,W,N), x1 (B,H-1,W-1,N1) or None, raw0 (M, ks^2, N + N1 + 32) non-zero.  'int': |dz|, |x| <= 3,
    |raw0| <= 5: at most 3 * 55 * 9 + 5 per element, exact in every format"""
    r = _rng(case.name, 4 if kind == "randn" else 5)
    B, H, W = case.B, case.H, case.W
    shapes = [(B, H, W, case.M), (B, H, W, case.N), (B, H - 1, W - 1, case.N1) if case.N1 else None,
              (case.M, case.ks * case.ks, case.N + case.N1 + 32)]
    if kind == "int":
        f = lambda s, hi=3: r.integers(-hi, hi + 1, s).astype(np.float32)
        dz, x0, x1, raw0 = f(shapes[0]), f(shapes[1]), (f(shapes[2]) if shapes[2] else None), f(shapes[3], 5)
    else:
        f = lambda s: r.standard_normal(s).astype(np.float32)
        g = (lambda s: (r.standard_normal(s) * np.exp(r.standard_normal(s))).astype(np.float32)) if case.kern != "f32" else f
        dz, x0, x1, raw0 = f(shapes[0]), g(shapes[1]), (f(shapes[2]) if shapes[2] else None), f(shapes[3])
    raw0[raw0 == 0] = 1.0
    return dz, x0, x1, raw0


# ------------------------------------------------------------------------------------------------ expected values
def reference(case, inp, scale=None, shift=None, relu=False, exps=(H2_ACT_EXP, H2_ACT_EXP, H2_ACT_EXP)):
    """the fp64 value and bound of one forward launch, from tests/dense_conv_ref.py alone.  exps = the exponents of the H2
    sources, destination and residual -> dict: acc, A (per virtual channel), y, bound (destination layout), pool, pool_bound"""
    import dense_conv_ref as R
    ar, K = arith(case), K_terms(case)
    e_src, e_dst, e_res = exps
    w = inp["w"]
    if case.ks == 2:
        a, op = inp["x0"][..., :case.c0], R.up2_op(case.H, case.W)
    elif case.mode == 0:
        a = R.assemble(inp["x0"], case.c0, inp["x1"], case.c1, case.pad1, "pool0" in case.flags)
        op = R.conv_op(case.ks, case.stride)
    elif case.mode == 1:
        a, op = R.assemble(inp["x0"], case.c0), R.up_op
    elif case.mode == 2:
        a, op = inp["x0"][..., :case.aux], R.stem_op
    elif case.mode == 3:
        a, op = inp["x0"][..., :case.c0], R.bwd_data_op(case.ks, case.H, case.W)
    else:
        a, op = inp["x0"], R.up_bwd_data_op
    acc, A, eacc = R.bilinear(op, a, w, K, ar, e_src, wexp_for(w))
    if acc.shape[3] < case.cout:       # mode 3: the padded output channels
        grow = lambda t: np.concatenate([t, np.zeros(t.shape[:3] + (case.cout - t.shape[3],))], axis=3)
        acc, A, eacc = grow(acc), grow(A), grow(eacc)
    scale = np.ones(case.cout, np.float32) if scale is None else scale
    shift = np.zeros(case.cout, np.float32) if shift is None else shift
    split = "split" in case.flags
    res = inp["res"] if ("res" in case.flags or "res_f32" in case.flags) else None
    if is_up(case) and res is not None:      # the residual has the destination's geometry: bring it to the virtual channels
        dh, dw = dst_hw(case)
        full = np.zeros((acc.shape[0], 2 * acc.shape[1], 2 * acc.shape[2], acc.shape[3] // 4))
        full[:, :dh, :dw] = res
        res = np.concatenate([full[:, q >> 1::2, q & 1::2] for q in range(4)], axis=3)
    y, bound = R.epilogue(acc, eacc, scale, shift, res, relu,
                          res_h2_exp=e_res if (ar == "h2" and split and "res" in case.flags) else None,
                          dst_h2_exp=e_dst if (ar == "h2" and split) else None)
    if is_up(case):
        dh, dw = dst_hw(case)
        y, bound = R.upscatter(y)[:, :dh, :dw], R.upscatter(bound)[:, :dh, :dw]
    out = dict(acc=acc, A=A, y=y, bound=bound)
    if "dst_pool" in case.flags:
        out["pool"], out["pool_bound"] = R.pooled(y, bound)
    return out
