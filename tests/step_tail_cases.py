"""Shared cases and inputs (test infrastructure only) of tests/test_step_tail_host.py and tests/test_gpu_step_tail.py: the
smallest shapes at which the loss, optimizer, copy and scale kernels of a training step can go wrong.  numpy only; every
input is fp32 (int64 for the masks) and reproducible from the case's id.  Nothing here imports the library."""
import zlib

import numpy as np

F32 = np.float32


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _nb(x, up):
    """the fp32 neighbour of x above (up) or below"""
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


# ------------------------------------------------------------------------------------------------ sfh_train_losses
def _loss_case(cid, nc, shape, lam=(2.0, 0.5, 1.0), rec_mse=0, focal=0, warp=True, dwarp=True, kind="randn"):
    return dict(id=cid, nc=nc, shape=shape, lam=lam, rec_mse=rec_mse, focal=focal, warp=warp, dwarp=dwarp, kind=kind)


def loss_cases():
    """coverage and geometry: every nc at 3x7x13 (a 256-thread block spans frame boundaries, HW = 91 is no multiple of 64)
    with the four focal_flags and both pointwise criteria going round; all eight combinations at nc = 4; 1x1x1; 2x16x16 (one
    block per frame, exactly); each lambda zero in turn; no warp; no dwarp; the range cases.  The grid-stride case stands
    alone (LOSS_LARGE)."""
    out = []
    for nc in range(2, 9):
        out.append(_loss_case(f"nc{nc}", nc, (3, 7, 13), rec_mse=nc & 1, focal=nc & 3))
    for focal in range(4):
        for mse in (0, 1):
            out.append(_loss_case(f"nc4-f{focal}-m{mse}", 4, (3, 7, 13), rec_mse=mse, focal=focal))
    out.append(_loss_case("one-pixel", 3, (1, 1, 1)))
    out.append(_loss_case("one-pixel-focal", 8, (1, 1, 1), focal=3))
    out.append(_loss_case("block-per-frame", 5, (2, 16, 16), focal=2))
    out.append(_loss_case("no-seg", 4, (3, 7, 13), lam=(0.0, 0.5, 1.0)))
    out.append(_loss_case("no-rec", 4, (3, 7, 13), lam=(2.0, 0.0, 1.0)))
    out.append(_loss_case("no-cons", 4, (3, 7, 13), lam=(2.0, 0.5, 0.0), focal=1))
    out.append(_loss_case("no-warp", 6, (3, 7, 13), lam=(2.0, 0.0, 0.0), warp=False, dwarp=False))
    out.append(_loss_case("no-dwarp", 7, (3, 7, 13), dwarp=False))
    for kind in ("spread200", "equal", "big"):
        for focal in (0, 3):
            out.append(_loss_case(f"{kind}-f{focal}", 4, (2, 3, 5), focal=focal, kind=kind))
    out.append(_loss_case("spread200-nc8-f3", 8, (2, 3, 5), focal=3, kind="spread200"))
    return out


LOSS_LARGE = _loss_case("grid-stride", 4, (2, 512, 513))     # 525312 pixels > 2048 blocks x 256: the loop's second trip


def boundary_warps(nc):
    """the warp values at which the consistency target decides: fl32(k / nc) for k = 0 .. nc with both neighbours, 1 and its
    neighbour below, a small negative value and -0"""
    v = []
    for k in range(nc + 1):
        x = F32(k) / F32(nc)
        v += [_nb(x, False), x, _nb(x, True)]
    v += [F32(1.0), _nb(1.0, False), F32(-1e-3), F32(-0.0)]
    return np.array(v, dtype=F32)


def loss_decision_cases():
    """per nc: the boundary warps as one row of pixels, consistency term only (CE and focal), so that d logits shows the
    chosen class alone.  And the SmoothL1 / MSE decision points at nc = 4, reconstruction term only."""
    out = []
    for nc in range(2, 9):
        n = len(boundary_warps(nc))
        for focal in (0, 2):
            out.append(_loss_case(f"tc-nc{nc}-f{focal}", nc, (1, 1, n), lam=(0.0, 0.0, 1.0), focal=focal, kind="tc"))
    for mse in (0, 1):
        out.append(_loss_case(f"pw-m{mse}", 4, (1, 1, len(_PW_WARP)), lam=(0.0, 1.0, 0.0), rec_mse=mse, kind="pw"))
    return out


# (gt, warp): d = warp - gt / 4 at +-1, their neighbours, 0, inside and beyond 1 (warp up to 2.5)
_PW = [(0, 1.0), (0, _nb(1.0, True)), (0, _nb(1.0, False)), (0, -1.0), (0, _nb(-1.0, True)), (0, _nb(-1.0, False)),
       (2, 1.5), (2, _nb(1.5, True)), (2, _nb(1.5, False)), (2, -0.5), (2, _nb(-0.5, True)), (2, _nb(-0.5, False)),
       (0, 0.0), (3, 0.75), (1, 0.3), (0, 2.5), (3, 2.5), (3, -0.75), (1, -0.0)]
_PW_WARP = np.array([w for _, w in _PW], dtype=F32)
_PW_GT = np.array([g for g, _ in _PW], dtype=np.int64)


def loss_inputs(c):
    """logits (B,nc,H,W) fp32, gt (B,H,W) int64, weight (B,) fp32, warp (B,H,W) fp32 or None, pre (3,) fp64"""
    r = _rng("loss-" + c["id"])
    B, H, W = c["shape"]
    nc = c["nc"]
    logits = (3.0 * r.standard_normal((B, nc, H, W))).astype(F32)
    gt = r.randint(0, nc, size=(B, H, W)).astype(np.int64)
    gt.flat[-1] = nc - 1
    weight = (0.5 + r.random_sample(B)).astype(F32)
    if B > 1:
        weight[1] = 0.0                                         # a frame that does not count
    warp = r.random_sample((B, H, W)).astype(F32)
    kind = c["kind"]
    if kind == "spread200":                                     # the small exponentials underflow; focal takes log(1e-8)
        top = r.randint(0, nc, size=(B, 1, H, W))
        logits = (r.standard_normal((B, nc, H, W)) - 100.0 + 200.0 * (np.arange(nc)[None, :, None, None] == top)).astype(F32)
    elif kind == "equal":
        logits[:] = 1.5
    elif kind == "big":
        logits[:, 1] = 1e4
    elif kind == "tc":
        warp = boundary_warps(nc).reshape(B, H, W)
    elif kind == "pw":
        warp, gt = _PW_WARP.reshape(B, H, W).copy(), _PW_GT.reshape(B, H, W).copy()
    return dict(logits=logits, gt=gt, weight=weight, warp=warp if c["warp"] else None, pre=np.array([0.75, -1.5, 3.25]))


def loss_exact_inputs(nc):
    """B * H * W, the lambdas and the weights powers of two, all logits equal, warp dyadic: d logits = coef * (1 / nc - onehot),
    d warp and loss3[1] are exact in fp32 / fp64 for nc = 2, 4, 8"""
    r = _rng(f"loss-exact-{nc}")
    B, H, W = 2, 4, 8
    logits = np.full((B, nc, H, W), 0.75, dtype=F32)
    gt = r.randint(0, nc, size=(B, H, W)).astype(np.int64)
    weight = np.array([1.0, 0.5], dtype=F32)
    warp = (r.randint(0, 17, size=(B, H, W)) / 8.0).astype(F32)           # multiples of 1/8 in [0, 2]: both SmoothL1 branches
    return dict(logits=logits, gt=gt, weight=weight, warp=warp, pre=np.array([0.0, 3.5, 0.0]), shape=(B, H, W))


# ------------------------------------------------------------------------------------------------ sfh_reproj_loss
REPROJ_BATCHES = [1, 63, 64, 65, 130]       # one thread per frame, 64 per block
REPROJ_NPTS = [1, 33]


def reproj_inputs(batch, npts, kind="rand"):
    """poi, gt (B,N,2), nonzeros (B,N), num_nonzero (B,) clamped to 1 as the dataset does.  A point with nz = 0, a frame with
    none (batch > 2), a point with dist == 0; kind 'none': no point counts anywhere."""
    r = _rng(f"reproj-{batch}-{npts}-{kind}")
    poi = r.random_sample((batch, npts, 2)).astype(F32)
    gt = r.random_sample((batch, npts, 2)).astype(F32)
    nz = (r.random_sample((batch, npts)) < 0.8).astype(F32)
    nz[0, 0] = 1.0
    gt[0, 0] = poi[0, 0]                                       # dist == 0 on a counted point
    if npts > 1:
        nz[0, 1] = 0.0
    if batch > 2:
        nz[2] = 0.0
    if kind == "none":
        nz[:] = 0.0
    nn = np.maximum(nz.sum(axis=1), 1.0).astype(F32)
    return dict(poi=poi, gt=gt, nz=nz, nn=nn, lam=8.0)


def reproj_exact_inputs():
    """integer coordinate differences that form Pythagorean triples, lambda, num_nonzero and batch powers of two: every dist
    and the loss are exact.  d poi = -(nz sc / dist) * dx is exact only where dist is a power of two - no triple has such a
    hypotenuse - so the last two points of every frame differ along one axis only ((0, 4) and (8, 0)): those are exact."""
    tri = [(3, 4), (5, 12), (8, 15), (6, 8), (-20, 21), (7, -24), (0, 4), (8, 0)]
    B, N = 4, len(tri)
    r = _rng("reproj-exact")
    poi = r.randint(-8, 9, size=(B, N, 2)).astype(F32)
    gt = poi + np.array(tri, dtype=F32)[None]
    nz = np.ones((B, N), dtype=F32)
    return dict(poi=poi, gt=gt, nz=nz, nn=np.full(B, float(N), dtype=F32), lam=2.0, exact_points=slice(6, 8))


# ------------------------------------------------------------------------------------------------ sfh_uv_loss
UV_CASES = [((1, 2, 21, 34), 1), ((12, 2, 9, 12), 12), ((1, 1, 1, 1), 1), ((3, 2, 5, 3), 3)]
UV_LARGE = ((1, 2, 257, 511), 1)            # 262654 elements > 1024 blocks x 256


def uv_inputs(shape, nweights):
    """uv in [-1, 2) against gt in [0, 1): both SmoothL1 branches; the first elements sit at d = +-1, their neighbours and 0"""
    r = _rng(f"uv-{shape}")
    uv = (r.random_sample(shape) * 3 - 1).astype(F32)
    gt = r.random_sample(shape).astype(F32)
    edge = [1.5, _nb(1.5, True), _nb(1.5, False), -0.5, _nb(-0.5, True), _nb(-0.5, False), 0.5]
    n = min(len(edge), uv.size)
    if uv.size > 1:
        uv.flat[:n], gt.flat[:n] = np.array(edge[:n], dtype=F32), F32(0.5)
    weight = (0.5 + r.random_sample(nweights)).astype(F32)
    return dict(uv=uv, gt=gt, weight=weight, lam=2.0)


# ------------------------------------------------------------------------------------------------ optimizers
OPT_SIZES = [1, 255, 256, 257, 65536, 65537, 70001]     # 65537: a second chunk of one element at offset 65536
CHUNK = 65536
DEFAULTS = dict(lr=1e-4, wd=1e-8, mu=0.9, alpha=0.99, eps=1e-8, clip=0.1, gscale=1.0, b1=0.9, b2=0.999)   # TrainStep's
SENTINEL_STATE = 777.25


def chunk_table(sizes):
    """(tensor, count, offset) rows exactly as TrainStep._init_optimizer builds them, as the bytes the kernel reads"""
    chunks = [(i, min(CHUNK, n - off), off) for i, n in enumerate(sizes) for off in range(0, n, CHUNK)]
    ch = np.zeros(len(chunks), dtype=np.dtype([("t", "<i4"), ("c", "<i4"), ("o", "<i8")]))
    for j, c in enumerate(chunks):
        ch[j] = c
    return ch.view(np.uint8).reshape(-1).copy(), len(chunks)


def _hp(**kw):
    h = dict(DEFAULTS)
    h.update(kw)
    return h


# id -> (kind, hyperparameters, gradient flavour)
OPT_CASES = {
    "rmsprop-defaults": ("rmsprop", _hp(), "randn"),
    "sgd-defaults": ("sgd", _hp(lr=1e-2), "randn"),
    "adam-defaults": ("adam", _hp(lr=1e-3), "randn"),
    "rmsprop-mu0": ("rmsprop", _hp(mu=0.0), "randn"),
    "sgd-mu0": ("sgd", _hp(mu=0.0, lr=1e-2), "randn"),
    "rmsprop-noclip": ("rmsprop", _hp(clip=0.0, lr=1e-3, wd=1e-4), "randn"),
    "sgd-noclip": ("sgd", _hp(clip=-1.0, lr=1e-2, wd=1e-4), "randn"),
    "adam-noclip": ("adam", _hp(clip=0.0, lr=1e-3, wd=1e-4), "randn"),
    "rmsprop-gscale": ("rmsprop", _hp(gscale=0.5, wd=1e-4), "randn"),
    "adam-gscale-wd0": ("adam", _hp(gscale=0.5, wd=0.0), "randn"),
    "sgd-wd0": ("sgd", _hp(wd=0.0), "randn"),
    "rmsprop-edges": ("rmsprop", _hp(clip=0.125, gscale=0.5, wd=1e-4, lr=1e-3), "edges"),
    "sgd-edges": ("sgd", _hp(clip=0.125, gscale=0.5, wd=1e-4, lr=1e-2), "edges"),
    "adam-edges": ("adam", _hp(clip=0.125, gscale=0.5, wd=1e-4, lr=1e-3), "edges"),
}
# powers of two throughout: every product, square root and quotient of the rule is exact
OPT_EXACT = {
    "rmsprop-exact": ("rmsprop", dict(lr=0.25, wd=0.0, mu=0.5, alpha=0.5, eps=0.125, clip=0.0, gscale=1.0), 3),
    "sgd-exact": ("sgd", dict(lr=0.25, wd=0.5, mu=0.5, clip=0.0, gscale=1.0), 3),
    "adam-exact": ("adam", dict(lr=0.25, wd=0.0, b1=0.5, b2=0.75, eps=0.125, clip=0.0, gscale=1.0), 1),
}


def clip_edges(hp):
    """gradients exactly at +-clip / gscale and one ulp beyond, 0, -0, +-inf (-> +-clip) and NaN (stays NaN, as clamp_)"""
    c = F32(hp["clip"]) / F32(hp["gscale"])
    return np.array([c, -c, _nb(c, True), _nb(-c, False), _nb(c, False), 0.0, -0.0, np.inf, -np.inf, np.nan], dtype=F32)


def opt_inputs(cid, sizes=OPT_SIZES, steps=3):
    """start state p, sq, buf per tensor and the gradients of `steps` steps.  A state tensor the rule never touches (buf at
    mu = 0, sq for SGD) starts as a sentinel and must come back bit-identical."""
    kind, hp, flavour = OPT_CASES[cid]
    r = _rng("opt-" + cid)
    p = [r.standard_normal(n).astype(F32) for n in sizes]
    sq = [(r.random_sample(n) * 0.01).astype(F32) for n in sizes]
    buf = [(r.standard_normal(n) * 0.05).astype(F32) for n in sizes]
    if kind == "sgd":
        sq = [np.full(n, SENTINEL_STATE, dtype=F32) for n in sizes]
    if kind != "adam" and not hp["mu"] > 0:
        buf = [np.full(n, SENTINEL_STATE, dtype=F32) for n in sizes]
    grads = []
    for it in range(steps):
        gs = [(r.standard_normal(n) * (0.3 if it else 0.05)).astype(F32) for n in sizes]
        if flavour == "edges":
            e = clip_edges(hp)
            i = sizes.index(257) if 257 in sizes else 0
            if it == 0:
                gs[i][:len(e)] = e[:len(gs[i])]
            else:                                   # the NaN element of step 1 has poisoned its weight: keep the rest finite
                gs[i][:len(e) - 1] = e[:len(e) - 1][:len(gs[i])]
        grads.append(gs)
    return dict(kind=kind, hp=hp, p=p, sq=sq, buf=buf, grads=grads, sizes=list(sizes))


def opt_exact_inputs(cid, sizes=(1, 257, 65537)):
    kind, hp, steps = OPT_EXACT[cid]
    r = _rng("opt-" + cid)
    g_mag = F32(0.125)
    p = [(r.randint(-64, 65, size=n) / 16.0).astype(F32) for n in sizes]
    grads = [[(g_mag * r.choice([-1.0, 1.0], size=n)).astype(F32) for n in sizes] for _ in range(steps)]
    if kind == "rmsprop":      # sq0 = g^2 keeps sq' = g^2: sqrt = |g| = eps, avg = 2 |g|, step = +-1/2
        sq = [np.full(n, g_mag * g_mag, dtype=F32) for n in sizes]
        buf = [(r.randint(-8, 9, size=n) / 4.0).astype(F32) for n in sizes]
    elif kind == "sgd":
        sq = [np.full(n, SENTINEL_STATE, dtype=F32) for n in sizes]
        buf = [(r.randint(-8, 9, size=n) / 4.0).astype(F32) for n in sizes]
    else:                      # adam at step 1 from zero moments: m' = g / 2, v' = g^2 / 4, sqrt(v') / sqrt(1/4) = |g| = eps
        sq = [np.zeros(n, dtype=F32) for n in sizes]
        buf = [np.zeros(n, dtype=F32) for n in sizes]
    return dict(kind=kind, hp=hp, p=p, sq=sq, buf=buf, grads=grads, sizes=list(sizes))


# ------------------------------------------------------------------------------------------------ sfh_multi_copy
def copy_sources():
    """[(name, storage (1-D fp32 / int32 array), element offset, logical shape, element strides, is_int)]: a contiguous tensor,
    the weight-gradient view (M, N, k, k) of an [m][tap][n] buffer, a view with a storage offset, one element, 65537 words, and
    an int32 tensor whose words include NaN payloads and -0"""
    r = _rng("copy")
    M, N, k = 5, 4, 3      # (small enough that a gather with two indices swapped stays inside the 64-element slack)
    out = [("contiguous", r.standard_normal(6 * 35).astype(F32), 0, (2, 3, 5, 7), (105, 35, 7, 1), False),
           ("wgrad-view", r.standard_normal(M * k * k * N).astype(F32), 0, (M, N, k, k), (k * k * N, 1, k * N, N), False),
           ("offset-view", r.standard_normal(100).astype(F32), 17, (4, 9), (18, 2), False),
           ("one", r.standard_normal(1).astype(F32), 0, (1,), (1,), False),
           ("two-chunks", r.standard_normal(65537).astype(F32), 0, (65537,), (1,), False)]
    words = r.randint(-2 ** 31, 2 ** 31, size=300, dtype=np.int64).astype(np.int32)
    words[:4] = np.array([0x7FC00001, 0xFFFFFFFF, 0x80000000, 0x7F800001], dtype=np.uint32).view(np.int32)
    out.append(("int32", words, 0, (3, 100), (100, 1), True))
    return out


COPY_SCALES = [0.25, 3.0]


# ------------------------------------------------------------------------------------------------ sfh_grad_scale
def _bits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def grad_scale_cases():
    """(id, head maxima (bit patterns), theta maximum or None, shift, overflow word before)"""
    b = _bits
    below = lambda x: b(np.nextafter(F32(x), F32(0)))
    out = []
    for shift in (-3, 0, 6):
        out.append((f"heads-s{shift}", [b(0.3), b(1.7), b(0.02)], None, shift, 0))
        out.append((f"theta-s{shift}", [], b(3e-5), shift, 0))
        out.append((f"both-s{shift}", [b(0.3), b(1.7)], b(0.4), shift, 0))
        out.append((f"pow2-s{shift}", [b(0.25), b(2.0 ** -5)], None, shift, 0))             # the frexpf edge: 2^e exactly
        out.append((f"pow2-below-s{shift}", [below(0.25), b(2.0 ** -5)], None, shift, 0))   # and one ulp below it
    out.append(("theta-pow2", [], b(2.0 ** -20), 0, 0))
    out.append(("theta-pow2-below", [], below(2.0 ** -20), 0, 0))
    out.append(("theta-raise", [b(1.5)], b(2.0 ** -21 * 1.25), 0, 0))          # theta * S < 2^-16, the heads allow the raise
    out.append(("theta-raise-edge", [b(1.0)], b(2.0 ** -18), 0, 0))            # theta * S = 2^-17; S2 puts it at 2^-16 exactly
    out.append(("theta-at-limit", [b(1.0)], b(2.0 ** -17), 0, 0))              # theta * S = 2^-16: not below, S stays
    out.append(("theta-no-room", [b(1.5)], b(2.0 ** -40), 0, 1))               # heads would pass 2^6: bit 4, S unchanged; bit 1 kept
    out.append(("theta-room-edge", [b(1.0)], b(2.0 ** -22), 0, 0))             # head * S2 = 2^6 exactly: refused
    out.append(("theta-room-edge-below", [below(1.0)], b(2.0 ** -22), 0, 0))   # just below 2^6: raised
    out.append(("nan-head", [b(0.5), 0x7FC00000], b(0.1), 0, 8))
    out.append(("inf-theta", [b(0.5)], 0x7F800000, 0, 0))
    out.append(("inf-only-theta", [], 0x7F800000, 0, 4))
    out.append(("zeros", [0, 0], 0, 0, 0))
    out.append(("zero-heads-theta", [0], b(0.5), 0, 0))
    return out


def grad_scale_words(heads, theta):
    """the word table of sfh_multi_absminmax: two words per tensor, the first = the bits of max |x|"""
    hb = list(heads) + ([theta] if theta is not None else [])
    w = np.zeros(2 * len(hb) + 2, dtype=np.uint32)
    w[0:2 * len(hb):2] = hb
    w[1::2] = 0x12345678              # the second word of a pair is not read
    return w


# ------------------------------------------------------------------------------------------------ resize backward
UP2_SHAPES = [(2, 8, 5, 7), (1, 4, 1, 3), (2, 4, 2, 2), (1, 8, 11, 20), (1, 4, 1, 1), (1, 12, 3, 5)]      # (B, C, H, W) of dx
# (hs, ws, hd, wd): the existing test's, an identity, an exact 2x and an exact 1/2
NEAREST_SHAPES = [(48, 80, 64, 96), (64, 96, 48, 80), (7, 9, 23, 31), (5, 5, 5, 5), (30, 17, 11, 40), (6, 7, 12, 14), (12, 14, 6, 7)]
NEAREST_PLANES = 6


def up2_dy(shape, integer=False):
    B, C, H, W = shape
    r = _rng(f"up2-{shape}-{integer}")
    if integer:
        return r.randint(-8, 9, size=(B, 2 * H, 2 * W, C)).astype(F32)
    return r.standard_normal((B, 2 * H, 2 * W, C)).astype(F32)


def nearest_dy(shape, integer=False):
    hs, ws, hd, wd = shape
    r = _rng(f"nearest-{shape}-{integer}")
    if integer:
        return r.randint(-8, 9, size=(NEAREST_PLANES, hd, wd)).astype(F32)
    return r.standard_normal((NEAREST_PLANES, hd, wd)).astype(F32)
