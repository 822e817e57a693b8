"""The cases of the grouped 3x3 convolution (csrc/conv_grouped.hip), shared by tests/test_grouped_conv_host.py (the
stand-alone host program, which walks the kernels' index functions) and tests/test_gpu_grouped_conv.py (the kernels).
Plain numpy; nothing here imports the library.  A case is (B, H, W, G, cg, stride)."""
import numpy as np

# the workgroup tile of output pixels the kernels use (csrc/conv_grouped_core.h: GC_TW, gc_tile_h)
TW = 16
GUARD = 64      # floats behind every output buffer that no kernel may touch


def tile_h(stride):
    return 8 if stride == 1 else 4


def wgrad_lanes(cg):
    """threads that share one raw element inside a workgroup (gc_wgrad_lanes)"""
    return 256 // (32 * (min(cg, 32) // 4))


def wgrad_plan(case):
    """-> (N = B * Ho * Wo, roundings a term meets inside a workgroup, workgroups that add to one raw element): the numbers
    grouped_conv_ref.wgrad_bound takes.  Inside a workgroup: 1 product + the thread's chain over its share of the tile's
    pixels (the first addition, onto 0, is exact) + the lanes' partial sums."""
    B, H, W, G, cg, s = case
    ho, wo = (H - 1) // s + 1, (W - 1) // s + 1
    lanes, th = wgrad_lanes(cg), tile_h(s)
    per_thread = -(-(th * TW) // lanes)
    return B * ho * wo, 1 + (per_thread - 1) + (lanes - 1), B * -(-ho // th) * -(-wo // TW)


def _cases():
    out = []
    for cg in (4, 8, 16, 32, 64):                       # every admitted cg at the models' 32 groups
        out += [(2, 7, 5, 32, cg, s) for s in (1, 2)]
    out += [(2, 23, 41, 1, 64, s) for s in (1, 2)]      # one group: a dense conv (also compared with PackedConv)
    out += [(1, 9, 200, 3, 4, 1)]                       # 12 channels: no multiple of 32, no power of two
    out += [(1, 1, 1, 2, 4, 1), (1, 1, 1, 2, 4, 2), (1, 2, 1, 2, 4, 1), (1, 2, 1, 2, 4, 2),      # degenerate maps
            (1, 1, 37, 2, 4, 1), (1, 1, 37, 2, 4, 2)]
    out += [(1, 23, 41, 2, 8, 2), (1, 24, 40, 2, 8, 2)]  # stride 2: odd sizes; last row / column read by no centre tap
    for s in (1, 2):                                     # tile edges: th - 1, th, th + 1 rows x tw - 1, tw, tw + 1 columns
        th = tile_h(s)
        for dh, dw in ((-1, -1), (0, 0), (1, 1), (-1, 1), (1, -1)):
            ho, wo = th + dh, TW + dw
            out.append((1, ho if s == 1 else 2 * ho - (dh & 1), wo if s == 1 else 2 * wo - 1 + (dw & 1), 2, 4, s))
    out += [(3, 5, 6, 2, 4, 1), (3, 5, 6, 2, 16, 2)]     # frames that end inside one workgroup's pixel range
    out += [(2, 90, 160, 32, 4, 1)]                      # more workgroups than the chip holds at once
    return out


CASES = _cases()
DENSE = [c for c in CASES if c[3] == 1]
# where the impulse family runs: 32 groups at both strides, the 12-channel case, one group of 64
IMPULSE = [(2, 7, 5, 32, 4, 1), (2, 7, 5, 32, 4, 2), (1, 9, 200, 3, 4, 1), (1, 5, 6, 2, 64, 2), (1, 24, 40, 2, 8, 2)]


def case_id(c):
    return "B{}_{}x{}_G{}_cg{}_s{}".format(*c)


def out_hw(case):
    _, H, W, _, _, s = case
    return (H - 1) // s + 1, (W - 1) // s + 1


def _rng(case, salt):
    return np.random.default_rng([salt, *case])


def randn_inputs(case):
    """-> x (B,H,W,C), w (C,cg,3,3), dz (B,Ho,Wo,C), raw0 (C,9,cg) float32, all non-zero"""
    B, H, W, G, cg, s = case
    C, (ho, wo) = G * cg, out_hw(case)
    r = _rng(case, 1)
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)
    return f(B, H, W, C), f(C, cg, 3, 3) * np.float32(1.0 / np.sqrt(9 * cg)), f(B, ho, wo, C), f(C, 9, cg)


def int_inputs(case):
    """the same tensors as small integers: every product and every partial sum is an integer below 2^24 (|x|, |dz| <= 3,
    |w| <= 2; forward: 576 terms of at most 6; backward-filter: at most 28,800 pixels of at most 9, + |raw0| <= 5), exact in
    fp32 in any order - the kernels must give the fp64 value bit for bit"""
    B, H, W, G, cg, s = case
    C, (ho, wo) = G * cg, out_hw(case)
    r = _rng(case, 2)
    i = lambda lo, hi, *shape: r.integers(lo, hi + 1, shape).astype(np.float32)
    return i(-3, 3, B, H, W, C), i(-2, 2, C, cg, 3, 3), i(-3, 3, B, ho, wo, C), i(-5, 5, C, 9, cg)


def epilogue_inputs(case, acc):
    """scale in [-1, 1] with channel 1 at exactly 0, and a shift that puts about half of the activated outputs below zero
    (minus the per-channel median of acc * scale) -> (scale, shift) float32"""
    C = case[3] * case[4]
    r = _rng(case, 3)
    scale = r.uniform(-1.0, 1.0, C).astype(np.float32)
    scale[1] = 0.0
    shift = (-np.median((acc * scale.astype(np.float64)).reshape(-1, C), axis=0)).astype(np.float32)
    shift[1] = np.float32(0.25)
    return scale, shift


def impulse_source(shape):
    """channel + 1024 * pixel (pixel = the index inside the frame + the frame's first index): integers below 2^24"""
    B, H, W, C = shape
    assert B * H * W * 1024 + C < 2 ** 24
    pix = np.arange(B * H * W, dtype=np.float32).reshape(B, H, W, 1)
    return (pix * np.float32(1024.0) + np.arange(C, dtype=np.float32)).astype(np.float32)


def impulse_weights(case):
    """yields (w, g, o, c, ky, kx): a single 1 at every tap, for the first and last (o, c) of the first and last group"""
    _, _, _, G, cg, _ = case
    for g in sorted({0, G - 1}):
        for o, c in sorted({(0, 0), (cg - 1, cg - 1), (0, cg - 1)}):
            for ky in range(3):
                for kx in range(3):
                    w = np.zeros((G * cg, cg, 3, 3), dtype=np.float32)
                    w[g * cg + o, c, ky, kx] = 1.0
                    yield w, g, o, c, ky, kx
