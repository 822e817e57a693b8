"""CPU tests that hold the fp64 references of tests/theta_grad_ref.py themselves: each is compared with torch autograd, the
max-pool tie rule the HIP kernel relies on is stated, and the derived warp bound is shown to admit a correct kernel on every
case tests/test_gpu_theta_gradient.py runs.  No GPU, no kernel: reference against reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import warp_ref

import theta_grad_cases as cases
import theta_grad_ref as R

# Measured on the CPU (torch 2.10), reference against reference, as max |ref - autograd| / A over the cases of the test that
# uses it; each test asserts at four times its value.
WARP_END_TO_END_MEASURED = 5.65e-4
POI_END_TO_END_MEASURED = 1.2e-7


def _all_warp_cases(frames=cases.FRAMES):
    for frame in frames:
        for kind in cases.THETAS:
            yield from cases.warp_randn_cases(frame, kind)
        yield from cases.warp_one_hot_cases(frame)


def _frame_template(c):
    B = c["theta"].shape[0]
    return c["tmpl"][:1].expand(B, -1, -1, -1) if c["shared"] else c["tmpl"]


# ------------------------------------------------------------------------------------------------ warp
def test_warp_case_coverage():
    """every frame meets every (template, batch, sharing); the one-hot positions exist where the issue places them"""
    for frame in cases.FRAMES:
        seen = set()
        for kind in cases.THETAS:
            for c in cases.warp_randn_cases(frame, kind):
                seen.add((tuple(c["tmpl"].shape[2:]), c["theta"].shape[0], c["shared"]))
        assert len(seen) == len(cases.TEMPLATES) * len(cases.COMBOS), frame
    assert cases.one_hot_position("row_end_256", 5, 257) == (4, 256)
    assert cases.one_hot_position("y4_x255", 9, 259) == (4, 255)
    assert cases.one_hot_position("y4_x255", 2, 2) is None
    tm = cases.template("court", 3)
    assert tm.shape == (3, 1, 90, 160) and not torch.equal(tm[0], tm[1]) and not torch.equal(tm[1], tm[2])
    tm = cases.template("noise", 3)
    assert tm.shape == (3, 1, 97, 61) and not torch.equal(tm[0], tm[1])


def test_warp_coords_are_the_oracles():
    """the reference starts from the coordinates the forward is pinned to: s * X, s * Y are warp_ref.warp_grid bit for bit"""
    for kind in cases.THETAS:
        th = cases.thetas(kind, 3)
        X, Y, Z, s, xn, yn, live = R.warp_coords_f32(th, 9, 259)
        grid = warp_ref.warp_grid(th, 9, 259)
        assert torch.equal(s * X, grid[..., 0]) and torch.equal(s * Y, grid[..., 1])
    Z = R.warp_coords_f32(cases.thetas("z_cross", 1), 45, 80)[2]
    assert (Z > 0).any() and (Z < 0).any()
    X, Y, Z, s, xn, yn, live = R.warp_coords_f32(cases.thetas("z_row0", 3), 5, 257)
    assert (Z == 0).all() and (s == 1).all() and not live.any()


@pytest.mark.parametrize("frame", cases.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_warp_ref_vs_grid_sample_autograd(frame):
    """grid -> output leg, every case of the GPU test at this frame size: fp64 autograd through F.grid_sample(bilinear, zeros,
    align_corners=False) gives the same d loss / d (u, v) as the reference's four zero-padded taps, within 2^-40 * A after
    the common chain to theta.  The grid handed to grid_sample is the fp64 pre-image of the pinned fp32 pixel coordinate
    (u = (2 px + 1) / wt - 1), so that both sample at the same point."""
    masked = total = checked = 0
    for c in _all_warp_cases([frame]):
        B, h, w = c["theta"].shape[0], c["h"], c["w"]
        ht, wt = c["tmpl"].shape[2:]
        X, Y, Z, s, xn, yn, live = R.warp_coords_f32(c["theta"], h, w)
        px = warp_ref.unnormalize(s * X, wt).double()
        py = warp_ref.unnormalize(s * Y, ht).double()
        # on an exact integer d out / d px jumps and rounding decides which side autograd takes: those pixels are left out
        # of both sides (their dout is zeroed); everywhere else the two floors agree
        on_edge = ((px == px.floor()) & (px > -1) & (px < wt)) | ((py == py.floor()) & (py > -1) & (py < ht))
        dout = c["dout"] * (~on_edge)
        masked += int(on_edge.sum())
        total += on_edge.numel()
        grid = torch.stack([(2.0 * px + 1.0) / wt - 1.0, (2.0 * py + 1.0) / ht - 1.0], dim=-1).requires_grad_(True)
        out = F.grid_sample(_frame_template(c).double(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out.backward(dout.double().reshape(B, 1, h, w))
        gu, gv = grid.grad[..., 0].numpy(), grid.grad[..., 1].numpy()
        f64 = [a.numpy().astype(np.float64) for a in (X, Y, s, xn, yn)]
        want = R.theta_terms(gu, gv, *f64, live.numpy()).sum(axis=(2, 3))
        ref, A = R.warp_bwd_theta_ref(c["theta"], c["tmpl"], h, w, dout, c["shared"])
        assert (np.abs(ref - want) <= R.U40 * A).all(), c["id"]
        checked += int((A > 0).any())
    print(f"grid_sample leg: {masked} of {total} pixels on a cell edge left out; {checked} cases with a non-zero gradient")
    assert masked < 0.05 * total and checked >= 20


def _smooth_template(B, ht, wt):
    """a low-frequency sinusoid, one period across the template, shifted per frame"""
    y = torch.arange(ht, dtype=torch.float64).reshape(1, 1, ht, 1) / ht
    x = torch.arange(wt, dtype=torch.float64).reshape(1, 1, 1, wt) / wt
    b = torch.arange(B, dtype=torch.float64).reshape(B, 1, 1, 1)
    return (0.5 + 0.3 * torch.sin(2 * np.pi * (x + 0.1 * b)) * torch.cos(2 * np.pi * 0.7 * y + 0.3 * b)).float()


def _warp_all_fp64_autograd(theta, tmpl, h, w, dout, shared):
    B = theta.shape[0]
    th = theta.double().reshape(B, 9).clone().requires_grad_(True)
    xn = ((torch.arange(w, dtype=torch.float64) / (w - 1) - 0.5) * 2).reshape(1, 1, w).expand(B, h, w)
    yn = ((torch.arange(h, dtype=torch.float64) / (h - 1) - 0.5) * 2).reshape(1, h, 1).expand(B, h, w)
    t = [th[:, k].reshape(B, 1, 1) for k in range(9)]
    X, Y, Z = t[0] * xn + t[1] * yn + t[2], t[3] * xn + t[4] * yn + t[5], t[6] * xn + t[7] * yn + t[8]
    s = torch.where(Z.abs() > warp_ref.EPS, 1.0 / (Z + warp_ref.EPS), torch.ones_like(Z))
    tm = tmpl.double()
    tm = tm[:1].expand(B, -1, -1, -1) if shared else tm
    out = F.grid_sample(tm, torch.stack([s * X, s * Y], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=False)
    out.backward(dout.double().reshape(B, 1, h, w))
    return th.grad.numpy()


def test_warp_ref_vs_all_fp64_autograd():
    """End to end, theta included, against a chain that is fp64 throughout (coordinates too), on a smooth template and the
    benign thetas (identity and the realistic pair), every frame size, both template sizes, shared and per-frame.  The two
    differ by the fp32 rounding of the coordinates, which cannot be derived: measured max |ref - autograd| / A = 5.64e-4 (the
    identity at 257x5 on the 160-wide template, where pixel coordinates land exactly on template columns and the bilinear
    slope changes cell; 5.5e-5 at 80x45, below 3e-5 everywhere else).  Asserted at four times that."""
    worst = 0.0
    for (w, h) in cases.FRAMES:
        for kind in ("identity", "real0", "real1"):
            for (ht, wt) in ((90, 160), (97, 61)):
                for B, shared in ((3, False), (1, True)):
                    th, tm = cases.thetas(kind, B), _smooth_template(B, ht, wt)
                    dout = torch.randn(B, h, w, generator=torch.Generator().manual_seed(5))
                    ref, A = R.warp_bwd_theta_ref(th, tm, h, w, dout, shared)
                    diff = np.abs(ref - _warp_all_fp64_autograd(th, tm, h, w, dout, shared))
                    assert (A > 0).all() or w == 2          # (the realistic thetas put the corners of a 2x2 frame outside)
                    assert (diff[A == 0] == 0).all()
                    worst = max(worst, (diff[A > 0] / A[A > 0]).max(initial=0.0))
    print(f"warp reference vs all-fp64 autograd: max |diff| / A = {worst:.3e}")
    assert worst <= 4.0 * WARP_END_TO_END_MEASURED


@pytest.mark.parametrize("frame", cases.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_warp_bound_admits_the_fp32_weight_stage(frame):
    """The bound of the GPU test, 8 * 2^-24 * A + 2^-23 * |ref|, on every one of its cases at this frame size: the reference with its bilinear
    weights and tap combinations in individually rounded fp32 (the kernel's one fp32 stage, restated) and the result cast to
    fp32 stays inside it - so the bound alone cannot fail a correct kernel.  Also the exact properties the GPU test asserts."""
    worst = 0.0
    for c in _all_warp_cases([frame]):
        args = (c["theta"], c["tmpl"], c["h"], c["w"], c["dout"], c["shared"])
        ref, A = R.warp_bwd_theta_ref(*args)
        got = R.warp_bwd_theta_ref(*args, weights="fp32")[0].astype(np.float32).astype(np.float64)
        err, bound = np.abs(got - ref), R.warp_bound(ref, A)
        assert (err <= bound).all(), c["id"]
        worst = max(worst, (err[bound > 0] / bound[bound > 0]).max(initial=0.0))
        if c["kind"] == "outside":
            assert (ref == 0).all() and (A == 0).all(), c["id"]
        elif c["kind"] == "z_row0":
            assert (ref[:, 6:] == 0).all() and (A[:, 6:] == 0).all(), c["id"]
            assert (A[:, :6] > 0).any() or c["tmpl_name"] != "noise", c["id"]
        elif c["tmpl_name"] == "noise" and (c["w"] > 2 or c["kind"] in ("identity", "z_cross", "zoom_in")):
            assert (A[-1, :6] > 0).any(), c["id"]                    # a case that exercises nothing would pass any kernel
    print(f"fp32-weight restatement: max error / bound = {worst:.3f}")
    assert 0.0 < worst < 1.0


def test_warp_one_hot_reference_is_one_term():
    """a one-hot dout leaves exactly one pixel's term: |sum| = A entry by entry, and only the frame that holds the pixel"""
    for c in cases.warp_one_hot_cases((259, 9)):
        ref, A = R.warp_bwd_theta_ref(c["theta"], c["tmpl"], c["h"], c["w"], c["dout"], c["shared"])
        assert (np.abs(ref) == A).all() and (A[:-1] == 0).all(), c["id"]


# ------------------------------------------------------------------------------------------------ poi
def test_poi_inverse_is_the_forwards():
    """M of the reference is the fp32 matrix the forward's point transform uses: inverse(theta) in fp64, rounded once"""
    c = cases.poi_case(65, 33)
    M = R.inverse_h33_f32(c["theta"])
    want = torch.linalg.inv(c["theta"].double().reshape(-1, 3, 3)).reshape(-1, 9).numpy()
    assert (np.abs(M - want) <= 2.0 ** -23 * np.abs(want) + 1e-12).all()
    zb = c["zero_frame"]
    Z = M[zb, 6].astype(np.float64) * float(c["poi"][zb, 0, 0]) + M[zb, 7].astype(np.float64) * float(c["poi"][zb, 0, 1]) + M[zb, 8]
    assert abs(Z) <= 1e-8                                  # the |Z| <= 1e-8 branch, at the first point of that frame
    Zall = M[zb, 6] * c["poi"][zb, :, 0].numpy() + M[zb, 7] * c["poi"][zb, :, 1].numpy() + M[zb, 8]
    assert (Zall > 1e-3).any() and (Zall < -1e-3).any()    # and both signs over the 33 points


def test_poi_ref_vs_fp64_autograd():
    """Against fp64 autograd through torch.linalg.inv and Kornia's de-homogenisation (warp_ref.transform_points' rule), every
    batch size, 1 and 33 points, normalised or not; the frame built for the |Z| <= 1e-8 branch is left out (its branch is
    decided by rounding).  The gap is the fp32 rounding of M: measured max |ref - autograd| / A = 1.19e-7; asserted at four
    times that."""
    worst = 0.0
    for B in cases.POI_BATCHES:
        for npts in (1, 33):
            for normalize in (True, False):
                c = cases.poi_case(B, npts)
                keep = [b for b in range(B) if b != c["zero_frame"]]
                if not keep:
                    continue
                th, poi, d = c["theta"][keep], c["poi"][keep], c["dout"][keep]
                ref, A = R.poi_bwd_theta_ref(th, poi, d, normalize)
                t = th.double().reshape(-1, 3, 3).clone().requires_grad_(True)
                M, p = torch.linalg.inv(t), poi.double()
                X, Y, Z = (M[:, i, 0:1] * p[..., 0] + M[:, i, 1:2] * p[..., 1] + M[:, i, 2:3] for i in range(3))
                s = torch.where(Z.abs() > warp_ref.EPS, 1.0 / (Z + warp_ref.EPS), torch.ones_like(Z))
                out = torch.stack([s * X, s * Y], dim=-1)
                (out / 2.0 + 0.5 if normalize else out).backward(d.double())
                worst = max(worst, (np.abs(ref - t.grad.numpy().reshape(-1, 9)) / A).max())
    print(f"poi reference vs fp64 autograd: max |diff| / A = {worst:.3e}")
    assert worst <= 4.0 * POI_END_TO_END_MEASURED


def test_poi_dead_branch_frame():
    """in the frame built for it, the first point contributes d X and d Y with s = 1 and nothing to d Z"""
    c = cases.poi_case(3, 1)
    zb = c["zero_frame"]
    ref, A = R.poi_bwd_theta_ref(c["theta"], c["poi"], c["dout"], True)
    M = R.inverse_h33_f32(c["theta"]).astype(np.float64).reshape(-1, 3, 3)[zb]
    gu, gv = 0.5 * c["dout"][zb, 0].double().numpy()
    px, py = c["poi"][zb, 0].double().numpy()
    dM = np.array([[gu * px, gu * py, gu], [gv * px, gv * py, gv], [0, 0, 0]])
    assert np.allclose(ref[zb].reshape(3, 3), -(M.T @ dM @ M.T), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ max-pool tie rule
def _first_max_routing(x, dy):
    """MaxPool2d(3, 2, 1) backward with the gradient of a window going to its first maximum in row-major scan order"""
    B, H, W, C = x.shape
    dx = np.zeros((B, H, W, C))
    bb, cc = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for yo in range(dy.shape[1]):
        for xo in range(dy.shape[2]):
            ys = [y for y in range(2 * yo - 1, 2 * yo + 2) if 0 <= y < H]
            xs = [x_ for x_ in range(2 * xo - 1, 2 * xo + 2) if 0 <= x_ < W]
            win = x[:, ys][:, :, xs].reshape(B, len(ys) * len(xs), C)
            k = np.argmax(win, axis=1)                      # numpy: the first of equal maxima
            np.add.at(dx, (bb, np.asarray(ys)[k // len(xs)], np.asarray(xs)[k % len(xs)], cc), dy[:, yo, xo])
    return dx


@pytest.mark.parametrize("shape", cases.MAXPOOL_SHAPES)
def test_maxpool_reference_routes_ties_to_the_first_maximum(shape):
    """The property maxpool3x3s2_bwd_kernel relies on: torch's fp64 max_pool2d backward sends a window's gradient to the first
    maximum in row-major scan order.  On the all-ties input that is the first in-range element of each window.  A torch
    upgrade that changed the rule shows here, not on the GPU."""
    for kind in cases.MAXPOOL_INPUTS:
        x, dy = cases.maxpool_case(shape, kind)
        ref = R.maxpool3x3s2_bwd_ref(x, dy).numpy()
        assert np.array_equal(ref, _first_max_routing(x.numpy().astype(np.float64), dy.numpy().astype(np.float64))), kind
        if kind == "const":
            B, H, W, C = shape
            want = np.zeros((B, H, W, C))
            for yo in range(dy.shape[1]):
                for xo in range(dy.shape[2]):
                    want[:, max(2 * yo - 1, 0), max(2 * xo - 1, 0)] += dy[:, yo, xo].numpy()
            assert np.array_equal(ref, want)
        if kind == "relu_q" and R.pool_out(shape[1]) * R.pool_out(shape[2]) > 1:
            print(f"max-pool {shape} relu_q: {_tie_fraction(x):.2f} of the windows hold a tie at their maximum")


def _tie_fraction(x):
    """fraction of (window, channel) pairs whose maximum occurs more than once"""
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    win = F.unfold(xp, 3, stride=2).reshape(x.shape[0], x.shape[3], 9, -1)
    return ((win == win.max(dim=2, keepdim=True).values).sum(dim=2) > 1).float().mean().item()


# ------------------------------------------------------------------------------------------------ the other references
def test_avgpool_linear_reference_vs_autograd():
    c = cases.avgpool_case((3, 3, 5, 512, 9))
    x = c["x"].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    b = torch.zeros(9, dtype=torch.float64, requires_grad=True)
    (x.mean(dim=(1, 2)) @ w.T + b).backward(c["d"].double())
    r = R.avgpool_linear_bwd_ref(c["x"], c["w"], c["d"])
    assert np.allclose(x.grad.numpy(), np.broadcast_to(r["dx"][:, None, None, :], x.shape), rtol=1e-12, atol=1e-15)
    assert np.allclose(w.grad.numpy(), r["acc_w"], rtol=1e-12, atol=1e-15)
    assert np.allclose(b.grad.numpy(), r["acc_b"], rtol=1e-14, atol=0)
    assert (r["a_dx"] >= np.abs(r["dx"])).all() and (r["a_w"] >= np.abs(r["acc_w"])).all()


@pytest.mark.parametrize("shape", cases.AVGPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_linear_bounds_admit_serial_fp32(shape):
    """the kernel's arithmetic restated - serial fp32 sums, scaling by fl(1 / HW) - stays inside the bounds of the GPU test"""
    B, H, W, C, nout = shape
    HW = H * W
    c = cases.avgpool_case(shape)
    r = R.avgpool_linear_bwd_ref(c["x"], c["w"], c["d"])
    x, w, d = c["x"].numpy().reshape(B, HW, C), c["w"].numpy(), c["d"].numpy()
    inv = np.float32(1.0) / np.float32(HW)
    s = np.zeros((B, C), np.float32)
    for i in range(HW):
        s = s + x[:, i]
    mean = s * inv
    df = np.zeros((B, C), np.float32)
    for j in range(nout):
        df = df + d[:, j:j + 1] * w[j][None]
    df = df * inv
    assert df.dtype == np.float32 and mean.dtype == np.float32
    acc_w = d.astype(np.float64).T @ mean.astype(np.float64)
    assert (np.abs(df - r["dx"]) <= (nout + 1) * R.U24 * r["a_dx"]).all()
    assert (np.abs(acc_w - r["acc_w"]) <= (HW + 1) * R.U24 * r["a_w"]).all()


def test_stem_reference_is_the_transposed_sum():
    """dlogits[b][c][y][x] = sum dz[b][Y][X][co] w[co][c][ky][kx] over 2Y + ky - 3 = y, 2X + kx - 3 = x, written out"""
    c = cases.stem_case((2, 6, 65), (3, 3, 7), integer=True)
    ref, aref = R.stem_bwd_data_ref(c["dz"], c["w"], 3, 3, 6, 65)
    dz, w = c["dz"].double().numpy(), c["w"].double().numpy()
    want = np.zeros((2, 3, 6, 65))
    for Y in range(dz.shape[1]):
        for X in range(dz.shape[2]):
            for ky in range(7):
                for kx in range(7):
                    y, x = 2 * Y + ky - 3, 2 * X + kx - 3
                    if 0 <= y < 6 and 0 <= x < 65:
                        want[:, :, y, x] += dz[:, Y, X] @ w[:, 3:6, ky, kx]
    assert np.array_equal(ref, want)
    assert (aref >= np.abs(ref)).all()


def test_mover_references():
    src = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(2, 3, 4, 8) + 1.0
    z = R.zero_stuff2_ref(src[..., :4].contiguous(), 6, 9)
    assert z.shape == (2, 6, 9, 4) and z.sum() == src[..., :4].sum()
    assert torch.equal(z[:, 4, 6], src[:, 2, 3, :4]) and (z[:, 1::2] == 0).all() and (z[:, :, 1::2] == 0).all()
    assert (z[:, :, 8:] == 0).all()
    dst = torch.full((2, 5, 5, 4), 100.0)
    got = R.slice_add_ref(src, 4, -1, 2, dst, 1)
    for y in range(5):
        for x in range(5):
            sy, sx = y - 1, x + 2
            inside = 0 <= sy < 3 and 0 <= sx < 4
            want = 100.0 + (src[:, sy, sx, 4:8] if inside else 0.0)
            assert torch.equal(got[:, y, x], want * torch.ones(2, 4))
    assert torch.equal(R.slice_add_ref(src, 4, -1, 2, dst, 0), got - 100.0)
