"""fp64 CPU references (test infrastructure only) for the seven non-convolution kernels of the theta-gradient chain:

  sfh_homography_warp_bwd_theta, sfh_poi_project_bwd_theta, sfh_maxpool3x3s2_bwd, sfh_avgpool_linear_bwd,
  sfh_stem_bwd_data, sfh_zero_stuff2, sfh_slice_add

Plain numpy / torch-CPU; nothing here imports a kernel.  The two theta references start from the forward's pinned fp32
coordinates (oracle/warp_ref.py - the forward kernels are held bit for bit to those) and do everything behind them in fp64.
Besides each sum they return ``A``, the sum of the absolute values of the terms that were added: the derived error bounds
of tests/test_gpu_theta_gradient.py are multiples of it.  tests/test_theta_grad_host.py holds the references themselves
against torch autograd.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import warp_ref

U24, U23, U40, U50 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -40, 2.0 ** -50


# ------------------------------------------------------------------------------------------------ warp
def warp_coords_f32(theta, h, w):
    """X, Y, Z, s, xn, yn as fp32 numpy arrays (B,h,w) in the pinned order of warp_ref._homography_apply, and live = |Z| > eps."""
    B = theta.shape[0]
    t = theta.reshape(B, 9).to(torch.float32)
    tt = [t[:, k].reshape(B, 1, 1) for k in range(9)]
    xn = warp_ref.normalized_axis(w).reshape(1, 1, w).expand(B, h, w)
    yn = warp_ref.normalized_axis(h).reshape(1, h, 1).expand(B, h, w)
    X = (tt[0] * xn + tt[1] * yn) + tt[2]
    Y = (tt[3] * xn + tt[4] * yn) + tt[5]
    Z = (tt[6] * xn + tt[7] * yn) + tt[8]
    one = torch.ones_like(Z)
    live = torch.abs(Z) > warp_ref.EPS
    s = torch.where(live, one / (Z + warp_ref.EPS), one)
    return X, Y, Z, s, xn, yn, live


def _taps(tm, x0, y0):
    """zero-padded taps of tm (B,ht,wt) fp64 at integral-valued fp64 (x0, y0) (B,h,w)"""
    B, ht, wt = tm.shape
    ok = (x0 >= 0) & (x0 <= wt - 1) & (y0 >= 0) & (y0 <= ht - 1)
    ix = np.clip(x0, 0, wt - 1).astype(np.int64)
    iy = np.clip(y0, 0, ht - 1).astype(np.int64)
    bb = np.arange(B).reshape(B, 1, 1)
    return np.where(ok, tm[bb, iy, ix], 0.0)


def theta_terms(gu, gv, X, Y, s, xn, yn, live):
    """per-pixel terms (B,9,h,w) of the nine sums, from d loss / d u and d loss / d v (u = X s, v = Y s), all fp64"""
    gX, gY = gu * s, gv * s
    gZ = np.where(live, -(gu * X + gv * Y) * s * s, 0.0)
    return np.stack([gX * xn, gX * yn, gX, gY * xn, gY * yn, gY, gZ * xn, gZ * yn, gZ], axis=1)


def warp_bwd_theta_ref(theta, tmpl, h, w, dout, shared, weights="fp64"):
    """d loss / d theta (B,9) of out = grid_sample(tmpl, grid(theta), bilinear, zeros, align_corners=False), from dout (B,h,w).

    theta (B,9)|(B,3,3)|(B,1,3,3) fp32, tmpl (B|1,1,ht,wt) fp32 (shared: frame 0 serves every frame).  Returns (sum, A), both
    fp64 (B,9).  weights="fp32" restates the kernel's one fp32 stage - the bilinear weights and the two tap-difference
    combinations rounded operation by operation - and is what the derived bound is checked against on the CPU."""
    B = theta.shape[0]
    ht, wt = tmpl.shape[-2], tmpl.shape[-1]
    X, Y, Z, s, xn, yn, live = warp_coords_f32(theta, h, w)
    px = warp_ref.unnormalize(s * X, wt).numpy()
    py = warp_ref.unnormalize(s * Y, ht).numpy()
    assert np.isfinite(px).all() and np.isfinite(py).all(), "the reference covers finite sampling coordinates only"
    tm = tmpl.reshape(-1, ht, wt).numpy()
    tm = np.broadcast_to(tm[:1], (B, ht, wt)) if shared else tm
    assert tm.shape[0] == B
    X, Y, s, xn, yn = (a.numpy().astype(np.float64) for a in (X, Y, s, xn, yn))
    live = live.numpy()
    g = dout.reshape(B, h, w).numpy().astype(np.float64)
    x0, y0 = np.floor(px), np.floor(py)            # fp32, integral-valued
    v = [_taps(tm.astype(np.float64), x0.astype(np.float64) + dx, y0.astype(np.float64) + dy)
         for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    if weights == "fp64":
        wx1 = px.astype(np.float64) - x0
        wy1 = py.astype(np.float64) - y0
        wx0, wy0 = 1.0 - wx1, 1.0 - wy1
        du = wy0 * (v[1] - v[0]) + wy1 * (v[3] - v[2])
        dv = wx0 * (v[2] - v[0]) + wx1 * (v[3] - v[1])
    else:
        assert weights == "fp32"
        f = [a.astype(np.float32) for a in v]
        one = np.float32(1.0)
        wx1, wy1 = px - x0, py - y0
        wx0, wy0 = one - wx1, one - wy1
        du = (wy0 * (f[1] - f[0]) + wy1 * (f[3] - f[2])).astype(np.float64)
        dv = (wx0 * (f[2] - f[0]) + wx1 * (f[3] - f[1])).astype(np.float64)
        assert du.dtype == np.float64 and wy0.dtype == np.float32
    terms = theta_terms(g * du * (0.5 * wt), g * dv * (0.5 * ht), X, Y, s, xn, yn, live)
    return terms.sum(axis=(2, 3)), np.abs(terms).sum(axis=(2, 3))


def warp_bound(ref, A):
    """|got - ref| <= 8 * 2^-24 * A + 2^-23 * |ref|: at most four fp32 roundings in each of gu and gv in front of the fp64
    chain (weight complement, two products, one sum), doubled, plus the fp32 cast of the result."""
    return 8.0 * U24 * A + U23 * np.abs(ref)


# ------------------------------------------------------------------------------------------------ poi
def inverse_h33_f32(theta):
    """fp64 adjugate inverse in inverse_h33's operation order (csrc/warp_coords.h), each entry rounded once to fp32: (B,9)"""
    m = theta.reshape(-1, 9).to(torch.float32).numpy().astype(np.float64).T
    c00 = m[4] * m[8] - m[5] * m[7]
    c01 = m[5] * m[6] - m[3] * m[8]
    c02 = m[3] * m[7] - m[4] * m[6]
    det = m[0] * c00 + m[1] * c01 + m[2] * c02
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        idet = 1.0 / det
        M = np.stack([c00 * idet, (m[2] * m[7] - m[1] * m[8]) * idet, (m[1] * m[5] - m[2] * m[4]) * idet,
                      c01 * idet, (m[0] * m[8] - m[2] * m[6]) * idet, (m[2] * m[3] - m[0] * m[5]) * idet,
                      c02 * idet, (m[1] * m[6] - m[0] * m[7]) * idet, (m[0] * m[4] - m[1] * m[3]) * idet], axis=1)
        return M.astype(np.float32)


def poi_bwd_theta_ref(theta, poi, dout, normalize):
    """d loss / d theta (B,9) of out = hom(M p) (/ 2 + 0.5 if normalize), M = fp32(inverse(theta)), from dout (B,N,2).

    dM in fp64 (Kornia's rule: s = 1/(Z + 1e-8), constant 1 where |Z| <= 1e-8), d theta = -M^T dM M^T.  Returns (sum, A)."""
    B = theta.shape[0]
    M = inverse_h33_f32(theta).astype(np.float64).reshape(B, 3, 3)
    p = poi[:B].numpy().astype(np.float64)
    d = dout.numpy().astype(np.float64) * (0.5 if normalize else 1.0)
    px, py = p[..., 0], p[..., 1]
    r = [M[:, i, 0:1] * px + M[:, i, 1:2] * py + M[:, i, 2:3] for i in range(3)]
    X, Y, Z = r
    live = np.abs(Z) > 1e-8
    with np.errstate(divide="ignore"):
        s = np.where(live, 1.0 / (Z + 1e-8), 1.0)
    gu, gv = d[..., 0], d[..., 1]
    gX, gY = gu * s, gv * s
    gZ = np.where(live, -(gu * X + gv * Y) * s * s, 0.0)
    terms = np.stack([gX * px, gX * py, gX, gY * px, gY * py, gY, gZ * px, gZ * py, gZ], axis=1)   # (B,9,N)
    dM = terms.sum(axis=2).reshape(B, 3, 3)
    AM = np.abs(terms).sum(axis=2).reshape(B, 3, 3)
    Mt = M.transpose(0, 2, 1)
    ref = -(Mt @ dM @ Mt)
    A = np.abs(Mt) @ AM @ np.abs(Mt)
    return ref.reshape(B, 9), A.reshape(B, 9)


def poi_bound(ref, A):
    """the kernel is fp64 with the same rounded M: the fp32 cast of the result plus fp64 summation slack"""
    return U23 * np.abs(ref) + U40 * A


# ------------------------------------------------------------------------------------------------ max-pool 3x3 s2 p1
def maxpool3x3s2_bwd_ref(x_nhwc, dy_nhwc):
    """fp64 autograd through F.max_pool2d(x, 3, 2, 1); x (B,H,W,C), dy (B,Ho,Wo,C) -> dx (B,H,W,C) fp64"""
    x = x_nhwc.permute(0, 3, 1, 2).double().contiguous().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    y.backward(dy_nhwc.permute(0, 3, 1, 2).double().contiguous())
    return x.grad.permute(0, 2, 3, 1).contiguous()


def pool_out(n):
    return (n + 2 - 3) // 2 + 1


# ------------------------------------------------------------------------------------------------ avg-pool + linear
def avgpool_linear_bwd_ref(x, w, d):
    """AdaptiveAvgPool2d(1) + Linear backward in closed form.  x (B,H,W,C), w (nout,C), d (B,nout), all fp32 tensors.
    Returns dict of fp64 arrays: dx (B,C) (the same for every pixel), acc_w (nout,C), acc_b (nout) - the increments - and the
    absolute sums the bounds are built from: a_dx = sum_j |d_j w_jc| / HW, a_w = sum_b |d_bj| mean_p |x_bpc|, a_b = sum_b |d_bj|."""
    B, H, W, C = x.shape
    HW = H * W
    x64 = x.numpy().astype(np.float64).reshape(B, HW, C)
    w64, d64 = w.numpy().astype(np.float64), d.numpy().astype(np.float64)
    mean = x64.mean(axis=1)                                  # (B,C)
    amean = np.abs(x64).mean(axis=1)
    return {
        "dx": (d64 @ w64) / HW,
        "a_dx": (np.abs(d64) @ np.abs(w64)) / HW,
        "acc_w": d64.T @ mean,
        "a_w": np.abs(d64).T @ amean,
        "acc_b": np.asarray(d64.astype(np.longdouble).sum(axis=0), dtype=np.float64),
        "a_b": np.abs(d64).sum(axis=0),
    }


# ------------------------------------------------------------------------------------------------ stem backward-data
def stem_out(n):
    return (n + 6 - 7) // 2 + 1


def stem_bwd_data_ref(dz_nhwc, w, c_off, nc, H, W):
    """fp64 autograd through conv2d(x, w, stride=2, padding=3) for the input channels c_off .. c_off+nc.
    dz (B,Ho,Wo,64), w (64,cin,7,7) -> (d x (B,nc,H,W), sum |dz * w| (B,nc,H,W)), fp64."""
    B = dz_nhwc.shape[0]
    dz = dz_nhwc.permute(0, 3, 1, 2).double().contiguous()
    ws = w[:, c_off:c_off + nc].double().contiguous()
    out = []
    for a, b in ((dz, ws), (dz.abs(), ws.abs())):
        x = torch.zeros(B, nc, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, b, stride=2, padding=3).backward(a)
        out.append(x.grad.numpy())
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ movers
def zero_stuff2_ref(src, H, W):
    """dst (B,H,W,C): dst[:, 2j, 2i] = src[:, j, i], zero elsewhere"""
    B, ho, wo, C = src.shape
    dst = torch.zeros(B, H, W, C, dtype=src.dtype)
    dst[:, 0:2 * ho:2, 0:2 * wo:2] = src
    return dst


def slice_add_ref(src, c_off, oy, ox, dst, accumulate):
    """dst[b,y,x,:] (+)= src[b, y+oy, x+ox, c_off:c_off+C], zero out of range (the comment of slice_add_kernel)"""
    B, Hs, Ws, _ = src.shape
    _, h, w, C = dst.shape
    v = torch.zeros_like(dst)
    y0, y1 = max(0, -oy), min(h, Hs - oy)
    x0, x1 = max(0, -ox), min(w, Ws - ox)
    if y1 > y0 and x1 > x0:
        v[:, y0:y1, x0:x1] = src[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox, c_off:c_off + C]
    return dst + v if accumulate else v
