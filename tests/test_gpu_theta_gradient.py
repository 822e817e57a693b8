"""The seven non-convolution HIP kernels of the theta-gradient chain, one by one, against the fp64 CPU references of
tests/theta_grad_ref.py (which tests/test_theta_grad_host.py holds against torch autograd):

  sfh_homography_warp_bwd_theta, sfh_poi_project_bwd_theta, sfh_maxpool3x3s2_bwd, sfh_avgpool_linear_bwd,
  sfh_stem_bwd_data, sfh_zero_stuff2, sfh_slice_add

Every output buffer a test hands to a kernel ends in a guard of 64 sentinel elements that must come back untouched; an
output the kernel overwrites is pre-filled with NaN, one it accumulates into with non-zero values that the reference adds.
Every bound is derived (see each test) and built from the reference's own absolute sums; none is fitted to a kernel's output.
Each test prints its largest error / bound ratio (``pytest -s``).

Out of scope: NaN inputs of the max-pool backward.  The kernel's routing of a NaN differs from torch's and is not pinned here.
"""
import math

import numpy as np
import pytest
import torch

import theta_grad_cases as cases
import theta_grad_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 777.25
NAN = float("nan")


@pytest.fixture(scope="module")
def T():
    from sfh_amd import training
    return training


@pytest.fixture(scope="module")
def K():
    """(lib, _ptr, _stream): the raw C entry points"""
    from sfh_amd import _lib
    from sfh_amd.engine import _ptr, _stream
    return _lib.load(), _ptr, _stream


class Guarded:
    """a device buffer of ``shape`` followed by GUARD sentinel elements; ``fill`` is a scalar or a CPU tensor"""

    def __init__(self, shape, dtype, fill):
        self.n = math.prod(shape)
        self.buf = torch.empty(self.n + GUARD, dtype=dtype, device="cuda")
        self.buf[self.n:] = SENTINEL
        self.t = self.buf[:self.n].view(*shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.to(dtype))
        else:
            self.t.fill_(fill)

    def result(self):
        """the payload on the CPU, after checking that the guard is intact"""
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == SENTINEL).all()), "the kernel wrote behind its output"
        return self.t.cpu()


def _ratio(err, bound):
    """max err / bound; an entry with a zero bound must be exact"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert not np.isnan(err).any(), "NaN in the output"
    assert (err[bound == 0] == 0).all(), "non-zero error where the reference leaves no room"
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


# ------------------------------------------------------------------------------------------------ warp backward
def _check_warp(T, K, c):
    lib, _ptr, _stream = K
    B, h, w = c["theta"].shape[0], c["h"], c["w"]
    ht, wt = c["tmpl"].shape[2:]
    ref, A = R.warp_bwd_theta_ref(c["theta"], c["tmpl"], h, w, c["dout"], c["shared"])
    bound = R.warp_bound(ref, A)
    th, tm, dout = c["theta"].cuda(), c["tmpl"].cuda(), c["dout"].cuda()
    got = T.warp_backward_theta(th, tm, h, w, dout, c["shared"]).cpu().double().numpy()
    again = T.warp_backward_theta(th, tm, h, w, dout, c["shared"]).cpu().double().numpy()
    r = _ratio(np.abs(got - ref), bound)
    assert r <= 1.0, (c["id"], r)
    # two calls: the order of the fp64 atomics is free, so the same bound and not bit equality
    assert _ratio(np.abs(got - again), bound) <= 1.0, c["id"]
    if c["kind"] == "outside":
        assert (got == 0).all(), c["id"]
    if c["kind"] == "z_row0":
        assert (got[:, 6:] == 0).all(), c["id"]
    # the raw entry point accumulates into fp64 sums: earlier contents stay, nothing is written behind them
    pre = torch.randn(B * 9, generator=torch.Generator().manual_seed(B)).double() * 0.5
    acc = Guarded((B * 9,), torch.float64, pre)
    rc = lib.sfh_homography_warp_bwd_theta(_ptr(th), _ptr(tm), 0 if c["shared"] else ht * wt, ht, wt, B, h, w, _ptr(dout),
                                           _ptr(acc.t), _stream())
    assert rc == 0
    after = acc.result().numpy().reshape(B, 9)
    want = pre.numpy().reshape(B, 9) + ref
    slack = 2.0 ** -52 * np.abs(pre.numpy().reshape(B, 9)) * (A > 0)     # fp64 roundings of adding onto the earlier contents
    assert _ratio(np.abs(after - want), bound + slack) <= 1.0, c["id"]
    return r


@pytest.mark.parametrize("kind", cases.THETAS)
@pytest.mark.parametrize("frame", cases.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_warp_bwd_theta(T, K, frame, kind):
    """d loss / d theta of the bilinear warp, dout = randn, the four templates (160x90 court slice, 61x97 noise, 3x2, 1x1) with
    batch 1 / 3 / 17 and shared or per-frame templates in rotation (every frame size meets every combination).  Frames: 2x2
    (the minimum), 80x45, 257x5 (one pixel in the second 256-pixel block, ragged 4-row band), 259x9 (a quad broken at the row
    end), 640x6.  Thetas: identity (half-out taps at px = -0.5), the realistic pair, zoomed out, wholly outside (exactly
    zero), z changing sign inside the frame, a zero last row (Z = 0, s = 1: entries 6-8 exactly zero).
    Bound per entry: |got - ref| <= 8 * 2^-24 * A + 2^-23 * |ref| - at most four fp32 roundings in each of gu and gv in front of
    the fp64 chain, doubled, plus the fp32 cast of the result (test_theta_grad_host shows a correct kernel stays inside)."""
    worst = max(_check_warp(T, K, c) for c in cases.warp_randn_cases(frame, kind))
    print(f"RATIO warp_bwd_theta {frame[0]}x{frame[1]} {kind}: {worst:.3f}")


@pytest.mark.parametrize("frame", cases.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_warp_bwd_theta_one_hot(T, K, frame):
    """dout is one pixel - (0,0), (h-1,w-1), (h-1,256), (4,255), where the frame has it - of the last of three frames with
    their own templates: the reference is that pixel's single term, so a wrong pixel, row, frame or template shows."""
    worst = max(_check_warp(T, K, c) for c in cases.warp_one_hot_cases(frame))
    print(f"RATIO warp_bwd_theta one-hot {frame[0]}x{frame[1]}: {worst:.3f}")


# ------------------------------------------------------------------------------------------------ poi backward
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("npts", [1, 33])
@pytest.mark.parametrize("B", cases.POI_BATCHES)
def test_poi_bwd_theta(T, K, B, npts, normalize):
    """One thread per frame, 64 per block: batch 1, 64, 65, 130; one point and the 33 pitch points; the realistic thetas with
    per-frame noise and one frame whose Z is zero at a point (the |Z| <= 1e-8 branch) and of both signs over the others.
    Bound: 2^-23 * |ref| + 2^-40 * A - the kernel is fp64 with the same rounded M; what is left is the fp32 cast."""
    lib, _ptr, _stream = K
    c = cases.poi_case(B, npts)
    ref, A = R.poi_bwd_theta_ref(c["theta"], c["poi"], c["dout"], normalize)
    th, poi, dout = c["theta"].cuda(), c["poi"].cuda(), c["dout"].cuda()
    out = Guarded((B, 9), torch.float32, NAN)
    assert lib.sfh_poi_project_bwd_theta(_ptr(th), _ptr(poi), B, npts, 1 if normalize else 0, _ptr(dout), _ptr(out.t),
                                         _stream()) == 0
    got = out.result()
    r = _ratio(np.abs(got.double().numpy() - ref), R.poi_bound(ref, A))
    print(f"RATIO poi_bwd_theta B{B} n{npts} norm{int(normalize)}: {r:.3f}")
    assert r <= 1.0
    assert torch.equal(T.poi_backward_theta(th, poi, dout, normalize).cpu(), got)     # the wrapper is the same launch


# ------------------------------------------------------------------------------------------------ max-pool backward
@pytest.mark.parametrize("kind", cases.MAXPOOL_INPUTS)
@pytest.mark.parametrize("shape", cases.MAXPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool3x3s2_bwd(K, shape, kind):
    """MaxPool2d(3, 2, 1) backward against fp64 autograd: randn (no ties), relu(randn) in multiples of 0.25 (ties), a constant
    (all ties: the first-maximum-in-scan-order rule decides every pixel).  dy is integer-valued in [-8, 8], so the sums of up
    to four terms are exact and the result must equal the reference bit for bit."""
    lib, _ptr, _stream = K
    B, H, W, C = shape
    x, dy = cases.maxpool_case(shape, kind)
    want = R.maxpool3x3s2_bwd_ref(x, dy).float()
    dx = Guarded(shape, torch.float32, NAN)
    xg, dyg = x.cuda(), dy.cuda()
    assert lib.sfh_maxpool3x3s2_bwd(_ptr(xg), _ptr(dyg), _ptr(dx.t), B, H, W, C, _stream()) == 0
    assert torch.equal(dx.result(), want)


# ------------------------------------------------------------------------------------------------ avg-pool + linear backward
@pytest.mark.parametrize("shape", cases.AVGPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_linear_bwd(K, shape):
    """AdaptiveAvgPool2d(1) + Linear backward against its closed forms; acc_w and acc_b arrive loaded.  The kernel's serial
    fp32 sums are bounded by the n * u rule on the reference's absolute sums:
      dx    (nout + 1) * 2^-24 * sum_j |d_j w_jc| / HW      (nout products and adds, the scaling)
      acc_w (HW + 1) * 2^-24 * sum_b |d_bj| mean_p |x_bpc|  (the HW-term mean and its scaling; the rest is fp64)
      acc_b 2^-50 * sum_b |d_bj|                            (fp64 sums of fp32 values)"""
    lib, _ptr, _stream = K
    B, H, W, C, nout = shape
    c = cases.avgpool_case(shape)
    r = R.avgpool_linear_bwd_ref(c["x"], c["w"], c["d"])
    dx = Guarded((B, H, W, C), torch.float32, NAN)
    acc_w = Guarded((nout, C), torch.float64, c["acc_w"])
    acc_b = Guarded((nout,), torch.float64, c["acc_b"])
    xg, wg, dg = c["x"].cuda(), c["w"].cuda(), c["d"].cuda()
    assert lib.sfh_avgpool_linear_bwd(_ptr(xg), _ptr(wg), _ptr(dg), B, H, W, C, nout, _ptr(dx.t), _ptr(acc_w.t),
                                      _ptr(acc_b.t), _stream()) == 0
    got_dx = dx.result().double().numpy()
    e_dx = np.abs(got_dx - r["dx"][:, None, None, :])
    r_dx = _ratio(e_dx, np.broadcast_to(((nout + 1) * R.U24 * r["a_dx"])[:, None, None, :], e_dx.shape))
    r_w = _ratio(np.abs(acc_w.result().numpy() - (c["acc_w"].numpy() + r["acc_w"])), (H * W + 1) * R.U24 * r["a_w"])
    r_b = _ratio(np.abs(acc_b.result().numpy() - (c["acc_b"].numpy() + r["acc_b"])), R.U50 * r["a_b"])
    print(f"RATIO avgpool_linear_bwd {shape}: dx {r_dx:.3f} acc_w {r_w:.3f} acc_b {r_b:.3f}")
    assert r_dx <= 1.0 and r_w <= 1.0 and r_b <= 1.0


# ------------------------------------------------------------------------------------------------ stem backward-data
@pytest.mark.parametrize("integer", [True, False], ids=["int", "randn"])
@pytest.mark.parametrize("chans", cases.STEM_CHANNELS, ids=lambda c: "nc%d-off%d-cin%d" % c)
@pytest.mark.parametrize("shape", cases.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_bwd_data(K, shape, chans, integer):
    """Backward-data of the 7x7 stride-2 stem into the logits channels against fp64 autograd through conv2d; dlogits arrives
    loaded (the kernel adds).  Shapes: 1x1; 5x63; 6x65 (x + 64 < W for one column); 4x129 (one column in the second 128-tile);
    9x200 x 3 (18 tiles on 24 workgroups) and 8x130 x 11 (44 tiles) for the XCD-contiguous workgroup order.  nc 5 and 8 are the
    second instantiation (100 KB of LDS).  Integer dz, w and dlogits in [-2, 2]: every partial sum is exact in fp32, so bit
    equality.  randn: (1024 + 1) * 2^-24 * sum |dz w| per output - up to 64 x 16 serial fp32 terms and the final add."""
    lib, _ptr, _stream = K
    B, H, W = shape
    nc, c_off, cin = chans
    c = cases.stem_case(shape, chans, integer)
    ref, aref = R.stem_bwd_data_ref(c["dz"], c["w"], c_off, nc, H, W)
    want = c["pre"].double().numpy() + ref
    out = Guarded((B, nc, H, W), torch.float32, c["pre"])
    dz, w = c["dz"].cuda(), c["w"].cuda()
    assert lib.sfh_stem_bwd_data(_ptr(dz), _ptr(w), cin, c_off, nc, B, H, W, _ptr(out.t), _stream()) == 0
    got = out.result()
    if integer:
        assert torch.equal(got, torch.from_numpy(want).float())
    else:
        r = _ratio(np.abs(got.double().numpy() - want), 1025 * R.U24 * aref)
        print(f"RATIO stem_bwd_data {shape} {chans}: {r:.3f}")
        assert r <= 1.0


# ------------------------------------------------------------------------------------------------ movers
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1, 4), (2, 3, 5, 5, 10, 8), (3, 4, 7, 8, 13, 64), (1, 2, 2, 6, 7, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_zero_stuff2(K, shape):
    """dst[2j, 2i] = src[j, i], zero elsewhere: H = 2 ho - 1, H = 2 ho and H > 2 ho (the same for W); bit equality"""
    lib, _ptr, _stream = K
    B, ho, wo, H, W, C = shape
    src = torch.randn(B, ho, wo, C, generator=torch.Generator().manual_seed(H * W))
    dst = Guarded((B, H, W, C), torch.float32, NAN)
    sg = src.cuda()
    assert lib.sfh_zero_stuff2(_ptr(sg), _ptr(dst.t), B, ho, wo, H, W, C, _stream()) == 0
    assert torch.equal(dst.result(), R.zero_stuff2_ref(src, H, W))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("off", [(0, 0), (-1, -2), (2, 3)], ids=lambda o: f"oy{o[0]}ox{o[1]}")
@pytest.mark.parametrize("c_off", [0, 64])
def test_slice_add(K, c_off, off, accumulate):
    """dst[b,y,x,:] (+)= src[b, y+oy, x+ox, c_off:c_off+C], zero out of range: src (2,8,34,128) -> dst (2,11,37,64); one fp32
    add per element at the most, so bit equality"""
    lib, _ptr, _stream = K
    g = torch.Generator().manual_seed(17)
    src = torch.randn(2, 8, 34, 128, generator=g)
    pre = torch.randn(2, 11, 37, 64, generator=g)
    dst = Guarded(pre.shape, torch.float32, pre if accumulate else NAN)
    sg = src.cuda()
    assert lib.sfh_slice_add(_ptr(sg), 8, 34, 128, c_off, off[0], off[1], _ptr(dst.t), 2, 11, 37, 64, accumulate,
                             _stream()) == 0
    assert torch.equal(dst.result(), R.slice_add_ref(src, c_off, off[0], off[1], pre, accumulate))


@pytest.mark.parametrize("n", [4, 260, 9])
def test_add_small(T, K, n):
    """training._add_small: the (1,1,1,n) form of slice_add that sums the theta gradients; n = 9 takes its padded path"""
    lib = K[0]
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ag = Guarded((n,), torch.float32, a)
    got = T._add_small(lib, ag.t, b.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), a + b)
    if n % 4 == 0:
        assert torch.equal(ag.result(), a + b)      # in place
    else:
        assert torch.equal(ag.result(), a)          # the padded path returns a new tensor
