"""CPU checks of the homography refinement (include/sfh_amd.h, "Homography refinement against the segmentation"):

- tests/refine_ref.py, the numpy restatement, against itself: its J^T r against central differences of its own cost, the
  coordinate rule against the closed form, the planes on hand-made blocks;
- the convergence table of the two scenes of tests/refine_cases.py (printed): the restatement ends below 0.5 template
  pixels on all sixteen starts;
- the refusals of the C entries that need no device, through ctypes, and ThetaRefiner's ValueErrors on CPU tensors.
No sanitizer runs on code loaded into Python."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import refine_cases as K
import refine_ref as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def test_planes_on_hand_made_blocks():
    ids = np.array([[0, 1, 1, 2], [3, 1, 0, 2], [5, 5, 6, 7], [5, 4, 7, 7]])
    for nc in (4, 7, 8):
        t = (np.minimum(ids, nc - 1).astype(F32) / F32(nc))[None]
        p1, p2, p4 = (R.template_planes(t, nc, f) for f in (1, 2, 4))
        assert p1.shape == (1, 4, 4, R.channels(nc)) and p4.shape == (1, 1, 1, R.channels(nc))
        m = np.minimum(ids, nc - 1)
        for c in range(1, nc):
            assert np.array_equal(p1[0, :, :, c - 1], (m == c).astype(F32))
            assert p2[0, 0, 0, c - 1] == F32((m[:2, :2] == c).sum() / 4.0) and p4[0, 0, 0, c - 1] == F32((m == c).sum() / 16.0)
        assert not p1[..., nc - 1:].any() and not p4[..., nc - 1:].any()          # pad channels
    lg = np.zeros((1, 4, 2, 2), dtype=F32)
    lg[0, 2] = 80.0
    p, b = R.evidence_planes(lg, 2)
    assert p.shape == (1, 1, 1, 4) and abs(p[0, 0, 0, 1] - 1.0) < 1e-12 and p[0, 0, 0, 0] < 1e-30
    assert (b[..., :3] > 0).all() and not b[..., 3].any()
    eq, _ = R.evidence_planes(np.zeros((1, 4, 2, 2), dtype=F32), 1)
    assert np.array_equal(eq[0, 0, 0], [0.25, 0.25, 0.25, 0.0])
    f32 = R.evidence_planes_f32(lg, 2)
    assert f32[0, 0, 0, 1] == 1.0 and f32[0, 0, 0, 3] == 0.0


@pytest.mark.parametrize("f,n,nl", [(1, 128, 128), (1, 128, 64), (2, 128, 128), (4, 128, 64), (1, 72, 72), (2, 72, 36), (1, 640, 640)])
def test_axis_rule_against_the_closed_form(f, n, nl):
    """ax, cx are the fp64 expressions rounded once (checked against exact rationals to an fp64 rounding or two), and the
    points they give are the centres of the averaged pixels in create_meshgrid's convention: logits pixel l sits at
    (l + 1/2) n / nl - 1/2 of the warp grid, grid point x at 2 x / (n - 1) - 1."""
    ax, cx = R.axis(f, n, nl)
    exa = Fraction(2 * f * n, nl * (n - 1))
    exc = (Fraction(f * n, nl) - 1) / (n - 1) - 1
    assert abs(Fraction(float(ax)) - exa) <= Fraction(2) ** -24 * abs(exa) * (1 + Fraction(1, 2 ** 20))
    assert abs(Fraction(float(cx)) - exc) <= Fraction(2) ** -24 * abs(exc) * (1 + Fraction(1, 2 ** 20))
    for j in (0, 1, nl // f - 1):
        centre = (Fraction(f * j) + Fraction(f - 1, 2) + Fraction(1, 2)) * n / nl - Fraction(1, 2)
        assert exa * j + exc == 2 * centre / (n - 1) - 1
    if f == 1 and nl == n:
        assert cx == F32(-1.0) and abs(float(ax) - 2.0 / (n - 1)) <= 2.0 ** -24 * 2.0 / (n - 1)
        xn, _ = R.grid(1, n, n, n, n)
        from oracle import warp_ref
        assert np.abs(xn - warp_ref.normalized_axis(n).numpy()).max() <= 2 * 2.0 ** -24     # near, not required bit-equal
    from sfh_amd import _lib
    out = (ctypes.c_float * 2)()
    assert _lib.load().sfh_refine_axis(f, n, nl, ctypes.cast(out, ctypes.c_void_p)) == 0
    assert (F32(out[0]), F32(out[1])) == (ax, cx)


def _smooth_planes(h, w, cp, seed, n=1):
    """planes whose bilinear interpolant is nearly smooth: sums of waves much longer than a cell"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w, cp), dtype=F32)
    for c in range(cp - 1):
        for _ in range(3):
            kx, ky, ph = g.uniform(0.02, 0.06), g.uniform(0.02, 0.06), g.uniform(0, 6.28)
            out[..., c] += (0.15 * np.sin(kx * x + ky * y + ph)).astype(F32)
        out[..., c] += F32(0.5)
    return out


def test_jacobian_against_central_differences():
    """J^T r of the restatement against (cost(theta + h e_i) - cost(theta - h e_i)) / 4h of its own cost, on smooth planes.
    Allowance, per parameter i with G_i = sum |du r a_i| + |dv r b_i| (the absolute J^T r sum, A of sums()):
      - the float32 stage of the cost: a value carries at most 7 roundings (refine_ref's count: three weights and products,
        three additions), so cost moves by at most sum 2 |r| 7 u |val| per evaluation; two evaluations over 4 h;
      - the interpolant is piecewise bilinear: a pixel that crosses a cell border within +-h sees its derivative jump by the
        planes' second difference (waves of k <= 0.06 per cell, amplitude 0.45: <= 0.45 * 0.06^2 * 2 per cell against first
        differences of 0.45 * 0.06), a relative 0.12 on the fraction h |dp/dtheta| <= h * 80 of the pixels, plus the
        h^2 truncation of a cubic-free interpolant's products (below that): 0.12 * 80 h G_i, doubled."""
    Hh, Ww, he, we = 72, 128, 36, 64
    tp, ev = _smooth_planes(45, 80, 4, 1), _smooth_planes(he, we, 4, 2)
    theta = np.array([[0.7, 0.05, 0.02, -0.04, 0.65, 0.03, 0.04, -0.03, 1.0]], dtype=F32)
    S, A = R.sums(theta, tp, ev, Hh, Ww, 2)
    q = R.pixel_terms(theta, tp, ev, Hh, Ww, 2)
    h = 2.0 ** -12
    noise = 2 * 7 * R.U * float(np.sqrt(q["Arr"]).sum()) * 2.0      # |r| <= sqrt(sum r^2) per pixel, |val| <= 1
    for i in range(8):
        d = np.zeros(9, dtype=F32)
        d[i] = h
        cp, cm = (R.eval_cost(theta + s * d, tp, ev, Hh, Ww, 2)[0] for s in (1, -1))
        hh = float((theta + d)[0, i]) - float((theta - d)[0, i])                # the step actually taken in float32
        fd = (cp - cm) / (2 * hh)
        tol = 2 * noise / (2 * hh) + 2 * 0.12 * 80 * h * A[0, 36 + i]
        print(f"RATIO jacobian[{i}]: {abs(fd - S[0, 36 + i]) / tol:.3g}  (J^T r {S[0, 36 + i]:.6g}, fd {fd:.6g})")
        assert abs(fd - S[0, 36 + i]) <= tol
    # J^T J is the Gauss-Newton matrix of the same J: positive semi-definite, and the layout is the upper triangle by rows
    M = np.zeros((8, 8))
    M[np.triu_indices(8)] = S[0, :36]
    M = M + np.triu(M, 1).T
    assert np.linalg.eigvalsh(M).min() >= -1e-9 * np.abs(M).max() and (S[0, :36] <= A[0, :36] * (1 + 1e-12)).all()


def test_lm_solve_solves_its_system():
    g = np.random.default_rng(5)
    J = g.normal(size=(40, 8))
    r = g.normal(size=40)
    S = np.concatenate([(J.T @ J)[np.triu_indices(8)], J.T @ r, [r @ r]])
    for lam in (0.0, 1e-3, 10.0):
        d, ok = R.lm_solve(S, lam)
        Mx = J.T @ J + lam * np.diag(np.diag(J.T @ J))
        assert ok and np.allclose(Mx @ np.array(d), -(J.T @ r), rtol=1e-9, atol=1e-9)
    assert R.lm_solve(np.zeros(45), 1e-3)[1] is False
    S[44] = np.nan
    st = R.StepState()
    st.step(np.where(np.isnan(S), 1.0, S), np.arange(9, dtype=F32), True, False)
    cand, _ = st.step(S, np.ones(9, dtype=F32), False, False)              # a NaN cost rejects
    assert st.accepted == 0 and st.lam == 1e-2 and np.array_equal(st.theta, np.arange(9, dtype=F32))


# ------------------------------------------------------------------------------------------------ convergence
@pytest.fixture(scope="module")
def table():
    rows = {}
    for name in ("exact", "noisy"):
        sc = K.scene(name)
        tps = [R.template_planes(sc["tmpl"][:, 0], 4, f) for f in (4, 2, 1)]
        evs = [R.evidence_planes_f32(sc["logits"], f) for f in (4, 2, 1)]
        out = R.refine(sc["starts"], tps, evs, K.H, K.W)
        rows[name] = (sc, out)
    return rows


def test_convergence_table(table):
    """the restatement ends below 0.5 template pixels on all sixteen starts"""
    for name, (sc, out) in table.items():
        e0 = R.corner_error(sc["starts"], sc["theta_true"], K.WT, K.HT)
        e1 = R.corner_error(out["theta"], sc["theta_true"], K.WT, K.HT)
        for k in range(len(e0)):
            print(f"CONVERGENCE {name} start {k}: {e0[k]:6.2f} px -> {e1[k]:.3f} px, finest level's cost "
                  f"{out['cost'][k, -1, 0]:.4f} -> {out['cost'][k, -1, 1]:.4f}, accepted {out['accepted'][k].tolist()}")
        assert np.allclose(e0, sc["offsets"], atol=1e-3)
        assert (e1 < 0.5).all(), (name, e1)
        assert (out["cost"][:, :, 1] <= out["cost"][:, :, 0]).all()


def test_dead_frame_and_zero_iterations():
    """all-background evidence and the template outside: the singular system rejects every step"""
    tmpl = K.template(4)[:, 0]
    lg = np.zeros((1, 4, K.H, K.W), dtype=F32)
    lg[:, 0] = 8.0
    theta = np.array([[1.0, 0, 50.0, 0, 1.0, 50.0, 0, 0, 1.0]], dtype=F32)
    tps = [R.template_planes(tmpl, 4, f) for f in (4, 2, 1)]
    evs = [R.evidence_planes_f32(lg, f) for f in (4, 2, 1)]
    out = R.refine(theta, tps, evs, K.H, K.W)
    assert np.array_equal(out["theta"], theta) and not out["accepted"].any() and np.array_equal(out["cost"][..., 0], out["cost"][..., 1])
    out0 = R.refine(K.scene("exact")["starts"][:1], tps, evs, K.H, K.W, iters=0)
    assert np.array_equal(out0["theta"], K.scene("exact")["starts"][:1]) and not out0["accepted"].any()


# ------------------------------------------------------------------------------------------------ the C interface, no device
_HOST = (ctypes.c_double * 4096)()


def test_refusals_without_a_device():
    """every refusal returns -1 before anything could be launched (the pointers are host memory)"""
    from sfh_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p((ctypes.addressof(_HOST) + 15) & ~15)          # 16-byte aligned, as the plane loads ask
    assert lib.sfh_refine_workspace_bytes(3, 72, 128) == 2 * 2 * 3 * 45 * 8 == R.slabs(72, 128) * 3 * 45 * 8
    assert lib.sfh_refine_workspace_bytes(3, 18, 32) == 1 * 3 * 45 * 8 and lib.sfh_refine_workspace_bytes(16, 360, 640) == 60 * 16 * 360
    assert lib.sfh_refine_workspace_bytes(0, 8, 8) == -1 and lib.sfh_refine_workspace_bytes(1, 0, 8) == -1
    assert lib.sfh_refine_workspace_bytes(65536, 8, 8) == -1
    for nc in (1, 9):
        assert lib.sfh_refine_template_planes(p, 1, 8, 8, nc, 1, p, None) == -1 and b"nc" in lib.sfh_last_error()
        assert lib.sfh_refine_evidence_planes(p, 1, nc, 8, 8, 1, p, None) == -1 and b"nc" in lib.sfh_last_error()
        assert lib.sfh_refine_accumulate(p, p, 0, 8, 8, p, 1, nc, 8, 8, 8, 8, 1, p, 1 << 30, None) == -1 and b"nc" in lib.sfh_last_error()
    assert lib.sfh_refine_template_planes(p, 1, 9, 8, 4, 2, p, None) == -1 and b"divide" in lib.sfh_last_error()
    assert lib.sfh_refine_evidence_planes(p, 1, 4, 8, 9, 2, p, None) == -1 and b"divide" in lib.sfh_last_error()
    assert lib.sfh_refine_accumulate(p, p, 0, 8, 8, p, 1, 4, 8, 6, 8, 8, 4, p, 1 << 30, None) == -1 and b"divide" in lib.sfh_last_error()
    assert lib.sfh_refine_template_planes(None, 1, 8, 8, 4, 1, p, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_refine_evidence_planes(p, 1, 4, 8, 8, 1, None, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_refine_accumulate(None, p, 0, 8, 8, p, 1, 4, 8, 8, 8, 8, 1, p, 1 << 30, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_refine_step(None, 1, 1, 1, 0, p, p, p, p, p, p, p, p, 0, 1, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_refine_step(p, 0, 1, 1, 0, p, p, p, p, p, p, p, p, 0, 1, None) == -1
    assert lib.sfh_refine_step(p, 1, 1, 1, 0, p, p, p, p, p, p, p, p, 3, 3, None) == -1
    assert lib.sfh_refine_axis(1, 8, 8, None) == -1
    p4 = ctypes.c_void_p(p.value + 4)                            # the planes are read with 16-byte loads
    assert lib.sfh_refine_accumulate(p, p4, 0, 8, 8, p, 1, 4, 8, 8, 8, 8, 1, p, 1 << 30, None) == -1 and b"aligned" in lib.sfh_last_error()
    assert lib.sfh_refine_accumulate(p, p, 0, 8, 8, p4, 1, 4, 8, 8, 8, 8, 1, p, 1 << 30, None) == -1 and b"aligned" in lib.sfh_last_error()
    assert lib.sfh_refine_accumulate(p, p, 258, 8, 8, p, 2, 4, 8, 8, 8, 8, 1, p, 1 << 30, None) == -1 and b"stride" in lib.sfh_last_error()
    assert lib.sfh_refine_accumulate(p, p, 252, 8, 8, p, 2, 4, 8, 8, 8, 8, 1, p, 1 << 30, None) == -1 and b"stride" in lib.sfh_last_error()
    need = lib.sfh_refine_workspace_bytes(3, 36, 64)
    args = (p, p, 0, 180, 320, p, 3, 4, 72, 128, 72, 128, 2)
    for ws, nbytes in ((None, need), (p, need - 1)):
        assert lib.sfh_refine_accumulate(*args, ws, nbytes, None) == -1
        msg = lib.sfh_last_error().decode()
        assert "workspace" in msg and str(need) in msg and (str(need - 1) in msg or ws is None), msg


def test_refiner_value_errors_on_cpu_tensors():
    from sfh_amd.refine import ThetaRefiner
    court = torch.from_numpy(K.template(4))
    for bad in (dict(mask_classes=1), dict(mask_classes=9), dict(iters=-1), dict(factors=(7,)), dict(factors=(0,)), dict(grid_size=(1, 72))):
        with pytest.raises(ValueError):
            ThetaRefiner(court, **{**dict(mask_classes=4, grid_size=(K.W, K.H)), **bad})
    for t in (court[0], court.double(), court.expand(1, 2, -1, -1)):
        with pytest.raises(ValueError):
            ThetaRefiner(t, mask_classes=4, grid_size=(K.W, K.H))
    r = ThetaRefiner(court, mask_classes=4, grid_size=(K.W, K.H))
    th, lg = torch.eye(3).reshape(1, 1, 3, 3).repeat(2, 1, 1, 1), torch.zeros(2, 4, K.H, K.W)
    with pytest.raises(ValueError, match="CUDA"):
        r(th, lg)
    for a, b, what in ((th.double(), lg, "float32"), (th, lg.half(), "float32"), (th[:1], lg, "theta must be"),
                       (th.reshape(2, 9), lg, "theta must be"), (th, lg[:, :3], "logits must be"), (th, lg[0], "logits must be"),
                       (th, lg[:, :, :70], "does not divide"), (th, lg[:, :, :, :126], "does not divide")):
        with pytest.raises(ValueError, match=what):
            r(a, b)
    import pickle
    r2 = pickle.loads(pickle.dumps(r))
    assert (r2.mask_classes, r2.grid_size, r2.factors, r2.iters) == (4, (K.W, K.H), (4, 2, 1), 5) and r2._tmpl is None and r2._work == {}
    assert torch.equal(r2.court_img, court)
