"""Shared cases and inputs (test infrastructure only) of tests/test_pointwise_host.py and tests/test_gpu_pointwise.py: the
smallest shapes at which the forward kernels of csrc/pointwise.hip can go wrong.  numpy only; every input is fp32 (int32 for
the masks) and reproducible from the case's id.  Nothing here imports the library.  tests/test_pointwise_host.py checks the
tables themselves: every edge the kernels have is present."""
import zlib

import numpy as np

F32 = np.float32
NAN = F32(np.nan)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def randn(name, shape):
    return _rng(name).standard_normal(shape).astype(F32)


def r4(c):
    return (c + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ layout movers
LAYOUT_CHANNELS = (1, 3, 4, 5, 7, 8)
# pixel counts 1, 255, 256, 257 (one block of 256 threads and its neighbours) and 3 x 91: frame boundaries inside a block
LAYOUT_SHAPES = ((1, 1, 1), (1, 15, 17), (1, 16, 16), (1, 1, 257), (3, 7, 13))


def layout_strides(C):
    return (r4(C), r4(C) + 4)


S2D_SIZES = ((1, 1), (2, 2), (3, 5), (6, 4), (7, 7))
S2D_STRIDES = (4, 8, 12)
S2D_BATCHES = (1, 2)

MAXPOOL_SIZES = ((1, 1), (1, 7), (2, 2), (5, 6), (7, 5), (23, 41))
MAXPOOL_CHANNELS = (4, 12, 64)
MAXPOOL_KINDS = ("rand", "neginf", "nan")


def maxpool_nan_positions(H, W):
    """(channel, y, x) of the NaNs of the 'nan' kind: an even / even pixel is the middle tap of a window, an odd / odd one the
    last tap of one window and the first of the next, the last pixel of the map closes the list"""
    pos = [(0, 0, 0), (2, H - 1, W - 1)]
    if H > 1 and W > 1:
        pos.append((1, 1, 1))
    if H > 3 and W > 3:
        pos += [(3, 3, 3), (0, 2, 2)]
    return pos


def maxpool_input(H, W, C, kind):
    x = randn(f"maxpool-{H}x{W}x{C}-{kind}", (2, H, W, C))
    if kind == "neginf":
        x[:, :, :, 1] = -np.inf                  # a whole plane
        x[0, :, :, 2] = -np.inf
        x[1, 0, 0, 3] = -np.inf
    elif kind == "nan":
        for c, y, xx in maxpool_nan_positions(H, W):
            x[:, y, xx, c] = NAN
    return x


# nearest and bilinear resize: (in, out) per axis.  26 -> 22 and 62 -> 14: pairs where floor(fl32(o * fl32(in / out))) differs
# from the exact floor(o * in / out) - a search over all in, out < 2048 finds many (the first is 62 -> 14 at o = 7; 26 -> 22 at
# o = 11 is the smallest source); tests/test_pointwise_host.py holds both against torch.
SIZE_PAIRS = ((1, 1), (1, 5), (5, 1), (7, 3), (3, 7), (45, 90), (45, 91), (90, 45), (61, 97), (26, 22), (62, 14))
BILINEAR_EXTRA = ((23, 24), (41, 42))            # the GPU stand-in for 360 x 640 -> 361 x 641, which the host test runs
RESIZE_PLANES = (1, 6)


def resize_geometries(extra=False):
    """(hs, ws, hd, wd): pair i along the rows with pair i + 1 along the columns, so that every pair is used on both axes"""
    n = len(SIZE_PAIRS)
    g = [(SIZE_PAIRS[i][0], SIZE_PAIRS[(i + 1) % n][0], SIZE_PAIRS[i][1], SIZE_PAIRS[(i + 1) % n][1]) for i in range(n)]
    if extra:
        g.append((BILINEAR_EXTRA[0][0], BILINEAR_EXTRA[1][0], BILINEAR_EXTRA[0][1], BILINEAR_EXTRA[1][1]))
    return g


def resize_input(geom, planes):
    return randn(f"resize-{geom}-{planes}", (planes, geom[0], geom[1]))


UP2_SIZES = ((1, 1), (1, 4), (3, 1), (2, 2), (5, 7), (10, 9))
UP2_CHANNELS = (4, 12, 64)
UP2_BATCHES = (1, 2)


# ------------------------------------------------------------------------------------------------ sfh_fold_bn
FOLD_N = (1, 9, 64, 300)
FOLD_REPEAT = (1, 4)
FOLD_VARS = (0.0, 1e-12, 1.0, 1e6)
FOLD_EPS = 1e-5


def fold_inputs(n, off=0):
    """gamma, beta, mean, var, conv_bias of n channels; var walks FOLD_VARS from `off`; channel 0 has mean == conv_bias (the
    difference is exactly 0) and channel 1 (n > 1) the fp32 neighbour of it (a cancellation down to one ulp)"""
    r = _rng(f"fold-{n}-{off}")
    x = {k: r.standard_normal(n).astype(F32) for k in ("gamma", "beta", "mean", "cb")}
    x["var"] = np.array([FOLD_VARS[(i + off) % 4] for i in range(n)], dtype=F32)
    x["mean"][0] = x["cb"][0]
    if n > 1:
        x["mean"][1] = np.nextafter(x["cb"][1], F32(np.inf))
    return x


# ------------------------------------------------------------------------------------------------ sfh_outconv_fwd
def _oc(cid, nc, cin, shape, out="both", stn=None, seed=0):
    return dict(id=cid, nc=nc, cin=cin, shape=shape, out=out, stn=stn, seed=seed)


OUTCONV_STN = ((4, 8, 4), (4, 8, 8), (5, 8, 4), (7, 12, 4), (8, 12, 4), (8, 16, 4), (2, 16, 8))      # (nc, stn_cs, frame_cs)
OUTCONV_PIXELS = ((1, 1, 1), (1, 1, 127), (1, 8, 16), (1, 3, 43), (1, 7, 19))                          # 1, 127, 128, 129, 133
OUTCONV_FRAMES = (3, 7, 13)          # 273 pixels: frame boundaries and an odd tail inside 128-pixel blocks


def outconv_cases():
    out = [_oc(f"nc{nc}", nc, 64, OUTCONV_FRAMES) for nc in range(1, 9)]
    for i, cin in enumerate((8, 24, 72)):
        for nc in (4, 8):
            out.append(_oc(f"cin{cin}-nc{nc}", nc, cin, OUTCONV_PIXELS[1 + i]))
    out += [_oc(f"cin1024-nc{nc}", nc, 1024, (1, 10, 13)) for nc in (4, 8)]       # nc 8: 32 KB of LDS; 130 pixels
    out += [_oc(f"pix{b * h * w}", 4, 64, (b, h, w)) for b, h, w in OUTCONV_PIXELS]
    out += [_oc("logits-only", 4, 64, OUTCONV_FRAMES, out="logits"), _oc("argmax-only", 4, 64, OUTCONV_FRAMES, out="argmax")]
    out += [_oc(f"stn-nc{nc}-cs{scs}-f{fcs}", nc, 64, OUTCONV_FRAMES, stn=(scs, fcs)) for nc, scs, fcs in OUTCONV_STN]
    return out


def outconv_inputs(c):
    B, H, W = c["shape"]
    r = _rng(f"outconv-{c['id']}-{c['seed']}")
    x = dict(x=r.standard_normal((B, H, W, c["cin"])).astype(F32), w=r.standard_normal((c["nc"], c["cin"])).astype(F32),
             bias=r.standard_normal(c["nc"]).astype(F32), frame=None)
    if c["stn"]:
        x["frame"] = r.standard_normal((B, H, W, c["stn"][1])).astype(F32)
    return x


def outconv_tie_inputs():
    """integer-valued x, w and bias (every product and sum exact in fp32), nc 4, cin 8, 1 x 5 x 31 pixels: classes 1 and 2
    share their weights and bias (a two-way tie at every pixel, on top at many), and the first five pixels are zero, where all
    four logits equal the common bias (an all-way tie)"""
    r = _rng("outconv-ties")
    x = r.randint(-3, 4, size=(1, 5, 31, 8)).astype(F32)
    x[0, 0, :5] = 0
    w = r.randint(-4, 5, size=(4, 8)).astype(F32)
    w[2] = w[1]
    return dict(x=x, w=w, bias=np.full(4, 2.0, dtype=F32), frame=None)


# logits rows reached through the bias (x = 0): the kernel's answer under its strict `>` scan
OUTCONV_NONFINITE = (((1.0, np.nan, 3.0, 0.5), 2), ((1.0, 2.0, np.inf, 0.0), 2), ((np.nan, 1.0, 2.0, 3.0), 0),
                     ((1.0, 2.0, 3.0, np.nan), 2), ((-np.inf,) * 4, 0), ((np.inf, np.inf, 1.0, 0.0), 0),
                     ((np.nan,) * 4, 0), ((1.0, -np.inf, np.nan, 5.0), 3))


# ------------------------------------------------------------------------------------------------ sfh_consistency_ce_fwd
def _ce(cid, nc, shape, mask=None, kind="randn"):
    return dict(id=cid, nc=nc, shape=shape, mask=mask or shape[1:], kind=kind)


CE_SIZES = ((1, 1), (15, 17), (23, 89), (32, 64), (3, 683), (77, 133), (257, 512))   # H W = 1, 255, 2047, 2048, 2049, 5 * 2048 + 1 and 131584: 65 partials per frame
CE_MASK_RESIZES = (((45, 56), (90, 112)), ((45, 56), (91, 113)), ((90, 112), (45, 56)), ((1, 1), (7, 9)))


def ce_cases():
    out = [_ce(f"nc{nc}", nc, (3, 7, 13)) for nc in range(2, 9)]
    for i, (h, w) in enumerate(CE_SIZES):
        out.append(_ce(f"hw{h * w}", 2 + (i + 1) % 7, (3 if i & 1 else 1, h, w)))
    out[-1] = _ce("hw131584-65partials", 2, (3, 257, 512))
    out += [_ce(kind, 4, (2, 3, 5), kind=kind) for kind in ("spread200", "equal", "big")]
    out += [_ce(f"mask{m[0]}x{m[1]}-to-{s[0]}x{s[1]}", 4, (3,) + s, mask=m) for m, s in CE_MASK_RESIZES]
    return out


def ce_inputs(c):
    B, H, W = c["shape"]
    nc = c["nc"]
    r = _rng(f"ce-{c['id']}")
    logits = (2.0 * r.standard_normal((B, nc, H, W))).astype(F32)
    if c["kind"] == "spread200":
        top = r.randint(0, nc, size=(B, 1, H, W))
        logits = (r.standard_normal((B, nc, H, W)) - 100.0 + 200.0 * (np.arange(nc)[None, :, None, None] == top)).astype(F32)
    elif c["kind"] == "equal":
        logits[:] = 1.5
    elif c["kind"] == "big":
        logits[:, 1] = 1e4
    mask = r.randint(0, nc, size=(B,) + tuple(c["mask"])).astype(np.int32)
    return logits, mask


# ------------------------------------------------------------------------------------------------ sfh_avgpool_linear_fwd
AVG_HW = ((1, 1), (1, 3), (2, 2), (3, 4), (1, 13), (4, 4), (17, 1), (1, 29), (12, 20))     # 1, 3, 4, 12, 13, 16, 17, 29, 240
AVG_C = (4, 64, 65, 100, 512, 2048)
AVG_NOUT = (1, 3, 4, 5, 9)


def avgpool_cases():
    """every H W with C, nout and the batch going round; C = 2048 meets H W = 240"""
    out = []
    for i, (h, w) in enumerate(AVG_HW):
        out.append(dict(id=f"hw{h * w}", shape=(3 if i & 1 else 1, h, w, AVG_C[(i + 3) % 6]), nout=AVG_NOUT[i % 5]))
    out += [dict(id=f"c{c}", shape=(3, 1, 13, c), nout=9) for c in (4, 64)]
    return out


def avgpool_inputs(c):
    """x = 1000 + noise: a wrong divisor or a dropped pixel is a thousand bounds away"""
    r = _rng(f"avgpool-{c['id']}")
    C = c["shape"][3]
    return dict(x=(1000.0 + r.standard_normal(c["shape"])).astype(F32), w=(r.standard_normal((c["nout"], C)) / 8).astype(F32),
                b=r.standard_normal(c["nout"]).astype(F32))


# ------------------------------------------------------------------------------------------------ sfh_compose_up_weights
COMPOSE_CASES = ((16, 0, 16, 16), (32, 16, 48, 16), (48, 80, 16, 48), (80, 16, 48, 48), (80, 0, 16, 16))   # (c1, c0, cout, cx)


def compose_inputs(c1, c0, cout, cx, dtype=F32, name=None):
    r = _rng(name or f"compose-{(c1, c0, cout, cx)}")
    g = lambda *s: r.standard_normal(s).astype(dtype)
    return dict(wconv=g(cout, c0 + c1, 3, 3), wt=g(cx, c1, 2, 2), bt=g(c1), scale4=g(4 * cout), shift4=g(4 * cout))
