"""fp64 CPU references (test infrastructure only) for the grouped 3x3 convolution of csrc/conv_grouped.hip and for the
ResNet-STN around it.  Plain numpy / torch-CPU; nothing here imports the library.

Tensors are NHWC numpy arrays as the kernels see them: x (B,H,W,C), w OIHW (C,cg,3,3) with G = C // cg groups, dz
(B,Ho,Wo,C), Ho = (H - 1) // stride + 1.  Every reference returns its value and the absolute sum ``A = sum |term|`` the
bound is built from; every bound is a count of fp32 roundings (u = 2^-24), none is fitted to a kernel's output, and each
adds the fp64 reference's own error (the same count at 2^-53).

n * u rule (Jeannerod and Rump 2013, as in tests/train_kernel_ref.py): a sum of n fp32 products accumulated in ANY order,
contracted or not, errs by at most n * u * sum |a_i b_i|; the factor 1.01 covers the second-order terms.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
E53 = 2.0 ** -53


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _w(w):
    return torch.from_numpy(np.asarray(w, dtype=np.float64))


def out_size(n, stride):
    return (n - 1) // stride + 1


def conv(x, w, stride):
    """-> (acc (B,Ho,Wo,C), A = sum |x * w|) of nn.Conv2d(C, C, 3, stride, 1, groups=C // cg, bias=False)"""
    g = x.shape[3] // w.shape[1]
    acc = F.conv2d(_nchw(x), _w(w), None, stride, 1, 1, g)
    A = F.conv2d(_nchw(np.abs(x)), _w(np.abs(w)), None, stride, 1, 1, g)
    return _nhwc(acc), _nhwc(A)


def conv_bound(A, cg):
    """K = 9 * cg products and adds per output in some order: 1.01 * K * u * A, plus the reference's K * 2^-53 * A"""
    K = 9 * cg
    return (1.01 * K * U + K * E53) * A


def epilogue(acc, A, cg, scale, shift, relu):
    """y = [relu](acc * scale + shift) per channel -> (y, bound = conv_bound + 1.01 * u * (2 |acc * scale| + |y|)).  The
    kernel rounds the product and the sum once each: |dy| <= |scale| * d(acc) + u * |acc * scale| + u * |acc * scale +
    shift|; |scale| <= 1 (asserted) keeps the first term within conv_bound.  Behind a ReLU that closes (y = 0) the last term
    matters only where the computed value came out positive, and is then itself no larger than the error before it -
    second order, inside the factor 1.01."""
    scale, shift = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    assert np.abs(scale).max() <= 1.0
    pre = acc * scale + shift
    y = np.maximum(pre, 0.0) if relu else pre
    return y, conv_bound(A, cg) + 1.01 * U * (2 * np.abs(acc * scale) + np.abs(y))


def bwd_data(dz, w, stride, H, W):
    """-> (dx (B,H,W,C), A) = the gradient of conv() with respect to x for the output gradient dz, through autograd"""
    g = dz.shape[3] // w.shape[1]

    def run(d, ww):
        x = torch.zeros((d.shape[0], d.shape[3], H, W), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, _w(ww), None, stride, 1, 1, g)
        return _nhwc(torch.autograd.grad(y, x, _nchw(d))[0])
    return run(dz, w), run(np.abs(dz), np.abs(w))


def wgrad(dz, x, cg, stride):
    """-> (dw OIHW (C,cg,3,3), A) = the gradient of conv() with respect to w, through autograd"""
    C = x.shape[3]

    def run(d, xx):
        w = torch.zeros((C, cg, 3, 3), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(_nchw(xx), w, None, stride, 1, 1, C // cg)
        return torch.autograd.grad(y, w, _nchw(d))[0].numpy()
    return run(dz, x), run(np.abs(dz), np.abs(x))


def wgrad_bound(A, raw0, n_pixels, n_inner, n_workgroups):
    """The kernel's accumulation plan (csrc/conv_grouped_core.h), all fp32: one rounding per product; inside a workgroup a
    term passes at most n_inner - 1 further additions (its thread's chain, which starts from an exact 0, then the lanes'
    partial sums); each of the n_workgroups workgroups adds its sum to raw with one atomic, whose rounding is relative to the
    running value, at most |raw0| + A.  So |d raw| <= u * ((n_inner + n_workgroups) * A + n_workgroups * |raw0|).  Adding an
    exact zero rounds nothing, and the N = n_pixels products of an element meet in at most N - 1 non-trivial additions
    among themselves: the count in front of A never exceeds N plus the one addition onto a non-zero raw0.
    The reference's own error: the same counts at 2^-53."""
    nA = min(n_inner + n_workgroups, n_pixels + 1)
    return (1.01 * U + E53) * (nA * A + n_workgroups * np.abs(raw0) * (A > 0))


def raw_to_oihw(raw, cg):
    """the kernel's raw (C, 9, cg) -> OIHW (C, cg, 3, 3)"""
    C = raw.shape[0]
    return np.transpose(raw.reshape(C, 3, 3, cg), (0, 3, 1, 2))


def shifted_copy(src, c_src, c_dst, ky, kx, stride):
    """what a weight with a single 1 at (o, c, ky, kx) must produce: dst[b, oy, ox, c_dst] = src[b, oy * stride + ky - 1,
    ox * stride + kx - 1, c_src], zero where that pixel lies in the padding, zero in every other channel"""
    B, H, W, C = src.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    out = np.zeros((B, Ho, Wo, C), dtype=src.dtype)
    for oy in range(Ho):
        sy = oy * stride + ky - 1
        if not 0 <= sy < H:
            continue
        for ox in range(Wo):
            sx = ox * stride + kx - 1
            if 0 <= sx < W:
                out[:, oy, ox, c_dst] = src[:, sy, sx, c_src]
    return out


def scattered_copy(dz, c_src, c_dst, ky, kx, stride, H, W):
    """the transpose of shifted_copy (backward-data of the same impulse weight): dx[b, oy * stride + ky - 1,
    ox * stride + kx - 1, c_dst] = dz[b, oy, ox, c_src]"""
    B, Ho, Wo, C = dz.shape
    out = np.zeros((B, H, W, C), dtype=dz.dtype)
    for oy in range(Ho):
        sy = oy * stride + ky - 1
        if not 0 <= sy < H:
            continue
        for ox in range(Wo):
            sx = ox * stride + kx - 1
            if 0 <= sx < W:
                out[:, sy, sx, c_dst] = dz[:, oy, ox, c_src]
    return out


# ------------------------------------------------------------------------------------------------ the ResNet-STN
def _bn(x, sd, p, training):
    if training:
        return F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], True, 0.1, 1e-5)
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.1, 1e-5)


def _gconv(x, w, stride=1, padding=0):
    """conv without bias; the number of groups is read off the weight's shape"""
    return F.conv2d(x, w, None, stride, padding, 1, x.shape[1] // w.shape[1])


def _relu(x, masks, key):
    """ReLU - or, with masks ({key: bool tensor of x's shape}), the decisions of another pass imposed: x where the mask is set,
    0 elsewhere.  A pre-activation within rounding distance of zero may fall either way in an fp32-grade pass, and the
    element's whole gradient goes with the decision; under equal decisions the gradients differ by rounding alone."""
    return F.relu(x) if masks is None else x * masks[key].to(x.dtype)


def bottleneck(x, sd, p, stride, training=False, masks=None):
    """models/resnet.py:120-140 with the grouped conv2 of the ResNeXt depths; mask keys p.t1, p.t, p.out"""
    out = _relu(_bn(_gconv(x, sd[p + ".conv1.weight"]), sd, p + ".bn1", training), masks, p + ".t1")
    out = _relu(_bn(_gconv(out, sd[p + ".conv2.weight"], stride, 1), sd, p + ".bn2", training), masks, p + ".t")
    out = _bn(_gconv(out, sd[p + ".conv3.weight"]), sd, p + ".bn3", training)
    if p + ".downsample.0.weight" in sd:
        x = _bn(_gconv(x, sd[p + ".downsample.0.weight"], stride), sd, p + ".downsample.1", training)
    return _relu(out + x, masks, p + ".out")


def resnet_stn(y, sd, p="resnet_reg", training=False, masks=None):
    """models/resnet.py:235-254 for the Bottleneck depths of its table (plain, wide, ResNeXt), in the dtype of y and sd: stem
    7x7 s2, maxpool 3 s2 p1, the stages as far as sd has blocks, avgpool, Linear -> (B,1,3,3).  p = "" for a bare ResNetSTN
    state dict.  masks: see _relu; keys p.stem and the blocks'."""
    p = p + "." if p else ""
    x = _relu(_bn(F.conv2d(y, sd[p + "conv0.weight"], None, 2, 3), sd, p + "bn1", training), masks, p + "stem")
    x = F.max_pool2d(x, 3, 2, 1)
    for li in range(1, 5):
        bi = 0
        while f"{p}layer{li}.{bi}.conv1.weight" in sd:
            bp = f"{p}layer{li}.{bi}"
            stride = 2 if (li > 1 and bi == 0) else 1
            x = bottleneck(x, sd, bp, stride, training, masks)
            bi += 1
    x = torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)
    return F.linear(x, sd[p + "reg.weight"], sd[p + "reg.bias"]).view(-1, 1, 3, 3)


def transform_poi(theta, court_poi):
    """models/reconstructor.py:120-130 in the dtype of theta: the points through inverse(theta) with Kornia's
    de-homogenisation (1 / (z + 1e-8) where |z| > 1e-8), then / 2 + 0.5"""
    t = torch.inverse(theta.reshape(-1, 3, 3))
    p = court_poi[:t.shape[0]].to(t.dtype)
    x, y = p[..., 0], p[..., 1]
    r = [t[:, i, j].reshape(-1, 1) for i in range(3) for j in range(3)]
    X, Y, Z = (r[0] * x + r[1] * y) + r[2], (r[3] * x + r[4] * y) + r[5], (r[6] * x + r[7] * y) + r[8]
    s = torch.where(Z.abs() > 1e-8, 1.0 / (Z + 1e-8), torch.ones_like(Z))
    return torch.stack([s * X, s * Y], dim=-1) / 2.0 + 0.5
