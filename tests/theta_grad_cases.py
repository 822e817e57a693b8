"""Inputs shared by tests/test_theta_grad_host.py (CPU) and tests/test_gpu_theta_gradient.py (GPU): the warp and POI
backward-theta cases.  Everything is drawn from seeded generators, so both files see the same numbers."""
import zlib

import numpy as np
import torch

from sfh_amd import synth

FRAMES = [(2, 2), (80, 45), (257, 5), (259, 9), (640, 6)]                 # (w, h)
TEMPLATES = ["court", "noise", "t3x2", "t1x1"]
THETAS = ["identity", "real0", "real1", "zoom_out", "outside", "z_cross", "z_row0"]
COMBOS = [(1, True), (3, False), (17, True), (1, False), (3, True), (17, False)]   # (batch, shared_template)
ONE_HOTS = ["first", "last", "row_end_256", "y4_x255"]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def template(name, B, seed=0):
    """(B,1,ht,wt) fp32, a different template in every frame"""
    g = _gen("tmpl", name, B, seed)
    if name == "court":                                                    # the 160x90 court slice, shifted per frame
        c = synth.load_court_template("ncaa_nc4_640x360", 4, 1)[:, :, ::4, ::4]
        return torch.cat([torch.roll(c, shifts=(3 * b, 7 * b), dims=(2, 3)) for b in range(B)]).contiguous()
    ht, wt = {"noise": (97, 61), "t3x2": (2, 3), "t1x1": (1, 1)}[name]
    return torch.randn(B, 1, ht, wt, generator=g)


def thetas(kind, B, seed=0):
    """(B,9) fp32; frame 0 is the plain matrix, the other frames carry a little noise in the first two rows"""
    g = _gen("theta", kind, B, seed)
    base = {
        "identity": np.eye(3),
        "real0": synth.REALISTIC_THETAS[0] / synth.REALISTIC_THETAS[0][2, 2],
        "real1": synth.REALISTIC_THETAS[1],                                # as printed: theta[2][2] = 13.25
        "zoom_out": np.diag([3.0, 3.0, 1.0]),                              # frame -> [-3, 3]^2: most taps outside
        "outside": np.array([[1.0, 0, 5.0], [0, 1.0, 0], [0, 0, 1.0]]),    # u in [4, 6]: nothing inside
        "z_cross": np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0.3, 0.1]]),  # Z = xn + 0.3 yn + 0.1 changes sign in the frame
        "zoom_in": np.array([[0.7, 0.05, 0.1], [-0.04, 0.8, -0.05], [0.02, 0.03, 1.0]]),   # the whole frame inside (one-hots)
        "z_row0": np.array([[1.0, 0.1, 0], [0, 1.0, 0.05], [0, 0, 0]]),    # Z = 0 everywhere: s = 1
    }[kind]
    th = torch.tensor(np.asarray(base, dtype=np.float32)).reshape(1, 3, 3).repeat(B, 1, 1)
    noise = 0.01 * torch.randn(B, 3, 3, generator=g)
    noise[0] = 0.0
    noise[:, 2] = 0.0
    return (th + noise).reshape(B, 9).contiguous()


def combo_for(fi, ti, tpl):
    return COMBOS[(fi + ti + 2 * tpl) % len(COMBOS)]


def warp_randn_cases(frame, kind):
    """the four templates at one (frame, theta kind); batch and sharing rotate (test_theta_grad_host checks the coverage)"""
    w, h = frame
    fi, ti = FRAMES.index(frame), THETAS.index(kind)
    for tpl, name in enumerate(TEMPLATES):
        B, shared = combo_for(fi, ti, tpl)
        g = _gen("dout", frame, kind, name)
        yield {"id": f"{w}x{h}-{kind}-{name}-B{B}-{'shared' if shared else 'own'}", "theta": thetas(kind, B),
               "tmpl": template(name, B), "h": h, "w": w, "dout": torch.randn(B, h, w, generator=g), "shared": shared,
               "kind": kind, "tmpl_name": name}


def one_hot_position(name, h, w):
    y, x = {"first": (0, 0), "last": (h - 1, w - 1), "row_end_256": (h - 1, 256), "y4_x255": (4, 255)}[name]
    return (y, x) if (y < h and x < w) else None


def warp_one_hot_cases(frame):
    """dout is one pixel of the last of three frames: the reference is a single term, so an index error cannot hide"""
    w, h = frame
    B = 3
    for pos_name in ONE_HOTS:
        pos = one_hot_position(pos_name, h, w)
        if pos is None:
            continue
        for kind in ("identity", "zoom_in"):
            for name in ("court", "noise"):
                dout = torch.zeros(B, h, w)
                dout[B - 1, pos[0], pos[1]] = 1.5
                yield {"id": f"{w}x{h}-{kind}-{name}-onehot-{pos_name}", "theta": thetas(kind, B), "tmpl": template(name, B),
                       "h": h, "w": w, "dout": dout, "shared": False, "kind": kind, "tmpl_name": name}


# ------------------------------------------------------------------------------------------------ poi
POI_BATCHES = [1, 64, 65, 130]


def poi_points(npts, B):
    """(B,npts,2): the 33 pitch points, or one point per frame"""
    if npts == 33:
        return synth.load_court_poi("pitch", B)
    g = _gen("poi", npts, B)
    return (torch.rand(B, npts, 2, generator=g) * 1.8 - 0.9).contiguous()


def poi_case(B, npts, seed=0):
    """theta: the realistic pair with per-frame noise; frame B // 2 is replaced by a theta whose inverse has Z = 0 (to
    about 1e-15: the |Z| <= 1e-8 branch) at its first point and Z of both signs over the other points."""
    g = _gen("poi_theta", B, npts, seed)
    poi = poi_points(npts, B)
    idx = torch.arange(B) % 2
    th = torch.tensor(synth.REALISTIC_THETAS)[idx] + 0.01 * torch.randn(B, 3, 3, generator=g)
    th = th / th[:, 2:3, 2:3]
    zb = B // 2
    px, py = float(poi[zb, 0, 0]), float(poi[zb, 0, 1])
    m6 = np.float32(-1.0 / px)
    m7 = np.float32(-(1.0 + float(m6) * px) / py)
    th[zb] = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [-float(m6), -float(m7), 1.0]])      # its inverse is exact
    dout = torch.randn(B, npts, 2, generator=g)
    return {"theta": th.reshape(B, 9).contiguous(), "poi": poi, "dout": dout, "zero_frame": zb}


# ------------------------------------------------------------------------------------------------ max-pool
MAXPOOL_SHAPES = [(1, 1, 1, 4), (2, 2, 3, 4), (3, 7, 9, 8), (1, 8, 8, 64), (2, 45, 80, 64), (1, 6, 130, 12)]   # (B,H,W,C)
MAXPOOL_INPUTS = ["randn", "relu_q", "const"]


def maxpool_case(shape, kind):
    """x (B,H,W,C): randn (no ties), relu(randn) rounded to multiples of 0.25 (ties in most windows), or a constant (all ties);
    dy (B,Ho,Wo,C) integer-valued in [-8, 8]: the up-to-four-term sums of the backward are exact."""
    B, H, W, C = shape
    g = _gen("maxpool", shape, kind)
    x = torch.randn(B, H, W, C, generator=g)
    if kind == "relu_q":
        x = torch.round(torch.relu(x) * 4.0) / 4.0
    elif kind == "const":
        x = torch.full((B, H, W, C), 0.75)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randint(-8, 9, (B, Ho, Wo, C), generator=g).float()
    return x, dy


# ------------------------------------------------------------------------------------------------ avg-pool + linear
AVGPOOL_SHAPES = [(1, 1, 1, 4, 9), (3, 3, 5, 512, 9), (2, 12, 20, 2048, 9), (17, 2, 2, 260, 9), (2, 3, 3, 8, 1),
                  (2, 3, 3, 8, 256)]                                                                          # (B,H,W,C,nout)


def avgpool_case(shape):
    B, H, W, C, nout = shape
    g = _gen("avgpool", shape)
    return {"x": torch.randn(B, H, W, C, generator=g), "w": torch.randn(nout, C, generator=g),
            "d": torch.randn(B, nout, generator=g),
            # the accumulators' earlier contents: fp32-representable, so that the fp64 sums of acc_b are exact
            "acc_w": torch.randn(nout, C, generator=g).double(), "acc_b": torch.randn(nout, generator=g).double()}


# ------------------------------------------------------------------------------------------------ stem backward-data
STEM_SHAPES = [(1, 1, 1), (1, 5, 63), (2, 6, 65), (1, 4, 129), (3, 9, 200), (11, 8, 130)]                     # (B,H,W)
STEM_CHANNELS = [(1, 0, 1), (4, 0, 7), (3, 3, 7), (5, 0, 5), (8, 2, 12)]                                      # (nc,c_off,cin)


def stem_case(shape, chans, integer):
    """dz (B,Ho,Wo,64), w (64,cin,7,7), and the earlier contents of dlogits (B,nc,H,W), which the kernel adds to"""
    B, H, W = shape
    nc, c_off, cin = chans
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = _gen("stem", shape, chans, integer)
    if integer:
        draw = lambda *s: torch.randint(-2, 3, s, generator=g).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
    return {"dz": draw(B, Ho, Wo, 64), "w": draw(64, cin, 7, 7), "pre": draw(B, nc, H, W)}
