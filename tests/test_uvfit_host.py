"""CPU checks of the UV homography fit (include/sfh_amd.h, "Homography fit from the UV head"):

- tests/uvfit_ref.py, the numpy restatement, against itself: the 8 x 8 system assembled from the 24 moments against A^T w A,
  A^T w b built row by row; the coordinate convention against the oracle's tap indices and preparation.uv_tables;
- the recovery and contamination figures of the restatement, written to profiles/uvfit_parity.jsonl (test "host_recovery";
  the figures are the measurement - nothing absolute is asserted beyond "every solve succeeded");
- the tie condition of every case the GPU tests compare an inlier count on;
- UVFit's ValueErrors on CPU tensors and the refusals of the C entries that need no device, through ctypes.
No sanitizer runs on code loaded into Python."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import prep_ref
import uvfit_cases as K
import uvfit_ref as R
from conftest import ROOT

F32 = np.float32
PARITY = os.path.join(ROOT, "profiles", "uvfit_parity.jsonl")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("weighted", [False, True])
def test_assembly_against_rows(weighted):
    """the system assembled from the 24 moments equals A^T w A and A^T w b built row by row in fp64, on random gated pixels"""
    g = np.random.default_rng(7)
    h, w = 18, 32
    uv = g.uniform(0.05, 1.0, (1, 2, h, w)).astype(F32)
    uv[0, :, g.random((h, w)) < 0.3] = 0                               # not gated
    theta = K.PERSPECTIVE[None] if weighted else None
    q = R.pixel_terms(uv, None, theta, h, w, K.WT, K.HT)
    S, A, n = R.sums(uv, None, theta, h, w, K.WT, K.HT)
    keep = q["gate"][0]
    x, y, cx, cy, om = (q[k][0][keep] for k in ("x", "y", "cx", "cy", "om"))
    z, one = np.zeros_like(x), np.ones_like(x)
    rows = np.concatenate([np.stack([x, y, one, z, z, z, -cx * x, -cx * y], 1), np.stack([z, z, z, x, y, one, -cy * x, -cy * y], 1)])
    rhs, ww = np.concatenate([cx, cy]), np.concatenate([om, om])
    M, b = (rows * ww[:, None]).T @ rows, (rows * ww[:, None]).T @ rhs
    As, gs = R.assemble(S[0])
    scale = np.abs(M).max()
    assert n[0] == keep.sum() == S[0, 24] and 100 < n[0] < h * w
    assert np.abs(np.array(As) - M).max() <= 1e-12 * scale and np.abs(np.array(gs) - b).max() <= 1e-12 * scale
    assert abs(S[0, 23] - (ww * rhs * rhs).sum()) <= 1e-12 * S[0, 23]
    hv, ok = R.solve(S[0])
    assert ok and np.abs(M @ np.array(hv) - b).max() <= 1e-9 * scale
    # the cost of the solution by the step's expression is the weighted residual sum of squares
    _, status, stats, _ = R.step(S[0], 0, False, None, 0)
    h32 = np.array([F32(v) for v in hv], dtype=np.float64)
    rss = (ww * (rows @ h32 - rhs) ** 2).sum()
    assert status == 1 and abs(stats[3] - rss) <= 1e-9 * max(rss, S[0, 23] * 1e-3)


@pytest.mark.parametrize("name", list(K.TRUE))
@pytest.mark.parametrize("hw", [(72, 128), (72, 136)])
def test_coordinate_convention(name, hw):
    """A label pixel holds the table value of the oracle's nearest tap (prep_ref.tap_indices over preparation.uv_tables); the
    rule's cx = 2 u - (1 + 1 / wt) then is the CENTRE of that court pixel in the tap rule's own coordinates, px = (cx + 1) wt / 2
    - 0.5 = ix up to the 16-bit quantisation of the label (wt / 2 / 65535 px and a float32 rounding of u), and the rule's frame
    coordinates are the warp grid's: the court point of the pixel under the true theta lies within the nearest tap's half
    pixel of it.  The align-corners reading 2 (u wt - 1) / (wt - 1) - 1 is off by up to a pixel at the raster's ends."""
    from sfh_amd import preparation
    h, w = hw
    theta = K.TRUE[name]
    ut, vt = preparation.uv_tables((K.WT, K.HT))
    assert np.array_equal(ut, K.u_tables()[0]) and np.array_equal(vt, K.u_tables()[1])
    ix, iy, ok = (a[0] for a in prep_ref.tap_indices(torch.from_numpy(theta).reshape(1, 3, 3), (K.HT, K.WT), h, w))
    label = preparation.split_uv(np.stack([np.zeros((h, w), np.uint16), np.where(ok, ut[ix], 0).astype(np.uint16),
                                           np.where(ok, vt[iy], 0).astype(np.uint16)], axis=-1))[1]
    q = R.pixel_terms(label[None], None, theta[None], h, w, K.WT, K.HT)
    ok = ok & (ix < K.WT - 1) & (iy < K.HT - 1)        # generate_uv_template's window leaves the last column and row 0
    assert np.array_equal(q["gate"][0], ok) and ok.sum() > 0.9 * h * w
    px, py = (q["cx"][0] + 1) * K.WT / 2 - 0.5, (q["cy"][0] + 1) * K.HT / 2 - 0.5
    quant = 0.5 * K.WT / 65535 + K.WT * 2.0 ** -24
    assert np.abs(px - ix)[ok].max() <= quant and np.abs(py - iy)[ok].max() <= quant
    # the residual of a label under its own theta is the nearest tap's rounding: at most half a pixel per axis (+ float32 slack)
    r = np.sqrt(q["r2"][0][ok])
    assert r.max() <= np.sqrt(0.5) + 1e-3
    wrong = (2 * (label[0].astype(np.float64) * K.WT - 1) / (K.WT - 1) - 1 + 1) * K.WT / 2 - 0.5
    print(f"CONVENTION {name} {w}x{h}: residual rms {np.sqrt((r ** 2).mean()):.3f} px, max {r.max():.3f}; align-corners "
          f"reading off by up to {np.abs(wrong - ix)[ok].max():.2f} px")
    # the numpy label of the cases is the oracle's label except where the fp32 walk and fp64 disagree on a half-pixel boundary
    # (under the identity the whole last row and column sit on one, px = 319.5 and py = 179.5: not compared there)
    mine = K.label_uv(theta, h, w)
    assert name == "identity" or (mine != label).any(axis=0).mean() < 0.01


def test_recovery_and_contamination_figures():
    """the figures the README quotes, recomputed: corner error of the restatement against the true theta, court pixels"""
    rows = []
    for case in K.whole_cases():
        uv, t0, true = K.whole_inputs(case)
        out = R.fit(uv, None, t0, K.H, K.W, K.WT, K.HT)
        err = float(R.corner_error(out["theta"], true, K.WT, K.HT)[0])
        rows.append({"test": "host_recovery", "case": case[0], "err_px": err, "status": int(out["status"][0]),
                     "n": out["stats"][0, 0], "inliers": out["stats"][0, 1], "rms_px": out["stats"][0, 2]})
        assert out["status"][0] == 5 and np.isfinite(err)
    # a second frame size, and the stated limit: a strong perspective, 30 % contamination, no theta0 - the outliers are about a
    # third of the gated pixels and four passes are not enough; recorded, not asserted
    for name, true in K.TRUE.items():
        out = R.fit(K.label_uv(true, 72, 136)[None], None, None, 72, 136, K.WT, K.HT)
        rows.append({"test": "host_recovery", "case": f"label-{name}-72x136", "status": int(out["status"][0]),
                     "err_px": float(R.corner_error(out["theta"], true, K.WT, K.HT)[0])})
    strong = np.array([0.8, 0.1, 0.0, -0.05, 0.9, 0.0, 0.35, -0.3, 1.0], dtype=F32)
    uv = K.contaminate(K.label_uv(strong, K.H, K.W), 0.3, 5)[None]
    for iters in (4, 9):
        out = R.fit(uv, None, None, K.H, K.W, K.WT, K.HT, iters=iters)
        rows.append({"test": "host_recovery", "case": f"stated-limit-strong-perspective-30pct-cold-{iters + 1}-solves",
                     "err_px": float(R.corner_error(out["theta"], strong, K.WT, K.HT)[0]), "status": int(out["status"][0]),
                     "n": out["stats"][0, 0], "inliers": out["stats"][0, 1]})
    K.record(PARITY, rows)


def test_tie_condition():
    """in every case with a theta on which the GPU tests compare the inlier count, no gated pixel of the restatement has r2
    within a relative 1e-9 of delta^2: the count cannot legitimately differ - by choice of inputs, not by tolerance"""
    seen = 0
    for p in K.ACC_PARAMS:
        c = K.accumulate_case(p)
        for name, th in zip(c["names"], c["thetas"]):
            if th is not None and name != "nan":
                assert R.near_delta(c["uv"], c["logits"], th, c["H"], c["W"], K.WT, K.HT) == 0, (K.acc_id(p), name)
                seen += 1
    for case in K.whole_cases():
        uv, t0, _ = K.whole_inputs(case)
        out = R.fit(uv, None, t0, K.H, K.W, K.WT, K.HT)
        assert R.near_delta(uv, None, out["theta"], K.H, K.W, K.WT, K.HT) == 0, case[0]
    assert seen == len(K.ACC_PARAMS) * 4


def test_dead_frames_of_the_restatement():
    """n = 3, one row, all zero: status 0 and the three dead-frame thetas; a frame that fails later keeps its last solve"""
    uv = np.zeros((1, 2, 18, 32), dtype=F32)
    for th0 in (None, K.ZOOM[None]):
        out = R.fit(uv, None, th0, 18, 32, K.WT, K.HT)
        assert out["status"][0] == 0 and out["stats"][0, 0] == 0
        assert np.isnan(out["theta"]).all() if th0 is None else np.array_equal(out["theta"], th0)
    row = K.exact_uv(K.ZOOM, 18, 32)
    row[:, :9] = 0
    row[:, 10:] = 0
    three = np.zeros_like(row)
    three[:, 9, 4:7] = row[:, 9, 4:7]
    out = R.fit(three[None], None, None, 18, 32, K.WT, K.HT)
    assert out["status"][0] == 0 and out["stats"][0, 0] == 3 and np.isnan(out["theta"]).all()
    # one row of pixels: the system is singular in exact arithmetic, but its rounded pivots need not be <= 0 - the pivot rule
    # catches what rounding leaves singular, no more (the README says so); what is held is that device and restatement agree
    out = R.fit(row[None], None, None, 18, 32, K.WT, K.HT)
    print(f"ONE ROW: status {out['status'][0]}, stats {out['stats'][0].tolist()}")
    assert out["stats"][0, 0] == 32 and 0 <= out["status"][0] <= 5
    S, _, _ = R.sums(K.exact_uv(K.ZOOM, 18, 32)[None], None, None, 18, 32, K.WT, K.HT)
    t1, s1, _, _ = R.step(S[0], 0, False, None, 0)
    bad = S[0].copy()
    bad[7] = np.inf
    t2, s2, _, _ = R.step(bad, 1, False, t1, s1)
    t3, s3, _, _ = R.step(S[0], 2, False, t2, s2)                      # dead: a good system is not solved any more
    assert (s1, s2, s3) == (1, 1, 1) and np.array_equal(t1, t2) and np.array_equal(t2, t3)


# ------------------------------------------------------------------------------------------------ the Python layer, no device
def test_uvfit_value_errors_on_cpu_tensors():
    from sfh_amd.uvfit import UVFit
    for bad in (dict(court_size=(1, 180)), dict(grid_size=(128, 1)), dict(iters=-1), dict(delta=0.0), dict(delta=float("nan")),
                dict(mask_classes=1), dict(mask_classes=9)):
        with pytest.raises(ValueError):
            UVFit(**{**dict(court_size=(K.WT, K.HT), grid_size=(K.W, K.H)), **bad})
    f = UVFit((K.WT, K.HT), (K.W, K.H), mask_classes=4)
    uv, lg, th = torch.zeros(2, 2, K.H, K.W), torch.zeros(2, 4, K.H, K.W), torch.eye(3).reshape(1, 1, 3, 3).repeat(2, 1, 1, 1)
    with pytest.raises(ValueError, match="CUDA"):
        f(uv, lg, th)
    for a, b, c, what in ((uv[0], None, None, "uv must be"), (uv[:, :1], None, None, "uv must be"), (uv.double(), None, None, "float32"),
                          (uv, lg[:, :3], None, "logits must be"), (uv, lg[:1], None, "logits must be"), (uv, lg.half(), None, "float32"),
                          (uv, None, th[:1], "theta0 must be"), (uv, None, th.reshape(2, 9), "theta0 must be"),
                          (uv, None, th.double(), "float32"), (uv[:, :, :1], None, None, "both >= 2")):
        with pytest.raises(ValueError, match=what):
            f(a, b, c)
    with pytest.raises(ValueError, match="without mask_classes"):
        UVFit((K.WT, K.HT), (K.W, K.H))(uv, lg)
    f2 = pickle.loads(pickle.dumps(f))
    assert (f2.court_size, f2.grid_size, f2.mask_classes, f2.iters, f2.delta, f2._work) == ((K.WT, K.HT), (K.W, K.H), 4, 4, 2.0, {})
    u_min, v_min, kx, ky = f.constants()
    assert (F32(u_min), F32(v_min), kx, ky) == R.constants(K.WT, K.HT)


def test_uv_fitter_setter_refuses():
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    from sfh_amd.uvfit import UVFit
    court, poi = synth.load_court_template(batch_size=1), synth.load_court_poi(batch_size=1)
    fit = UVFit((K.WT, K.HT), (640, 360), mask_classes=4)
    for kw in (dict(), dict(use_unet=False, resnet_input="img")):
        net = Reconstructor(court, poi, **kw)
        assert net.uv_fitter is None
        with pytest.raises(ValueError, match="UV head"):
            net.uv_fitter = fit
        net.uv_fitter = None
    net = Reconstructor(court, poi, unet_uv=True)
    with pytest.raises(ValueError, match="UVFit"):
        net.uv_fitter = 3
    net.uv_fitter = fit
    assert net.uv_fitter is fit and "uv_fitter" not in net.state_dict()
    assert pickle.loads(pickle.dumps(net)).uv_fitter.court_size == (K.WT, K.HT)


# ------------------------------------------------------------------------------------------------ the C interface, no device
_HOST = (ctypes.c_double * 4096)()


def test_refusals_without_a_device():
    """every refusal returns -1 before anything could be launched (the pointers are host memory)"""
    from sfh_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(ctypes.addressof(_HOST))
    assert _lib.ABI.defines["SFH_UVFIT_SUMS"] == R.SUMS == 27
    assert lib.sfh_uvfit_workspace_bytes(3, 72, 136) == 3 * 2 * 3 * 27 * 8 == R.slabs(72, 136) * 3 * 27 * 8
    assert lib.sfh_uvfit_workspace_bytes(1, 2, 2) == 27 * 8 and lib.sfh_uvfit_workspace_bytes(16, 360, 640) == 60 * 16 * 27 * 8
    assert lib.sfh_uvfit_workspace_bytes(1, 65535 * 64, 2) == 65535 * 27 * 8
    for args in ((0, 8, 8), (65536, 8, 8), (1, 1, 8), (1, 8, 1), (1, 65535 * 64 + 1, 2)):      # the last: 65536 tile rows
        assert lib.sfh_uvfit_workspace_bytes(*args) == -1
    u_min, v_min, kx, ky = 0.5 / 320, 0.5 / 180, 1 + 1 / 320, 1 + 1 / 180
    big = 1 << 30

    def acc(uv=p, lg=p, nc=4, th=p, B=1, h=8, w=8, Hg=8, Wg=8, wt=320, ht=180, delta=2.0, ws=p, nbytes=big):
        return lib.sfh_uvfit_accumulate(uv, lg, nc, th, B, h, w, Hg, Wg, wt, ht, u_min, v_min, kx, ky, delta, ws, nbytes, None)

    assert acc(uv=None) == -1 and b"null" in lib.sfh_last_error()
    for nc in (1, 9):
        assert acc(nc=nc) == -1 and b"nc" in lib.sfh_last_error()
    for kw in (dict(h=1), dict(w=1), dict(Hg=1), dict(Wg=1), dict(wt=1), dict(ht=1)):
        assert acc(**kw) == -1 and b"geometry" in lib.sfh_last_error(), kw
    for d in (0.0, -1.0, float("nan")):
        assert acc(delta=d) == -1 and b"delta" in lib.sfh_last_error()
    for B in (0, 65536):
        assert acc(B=B) == -1 and b"batch" in lib.sfh_last_error()
    need = lib.sfh_uvfit_workspace_bytes(3, 72, 128)
    for ws, nbytes in ((None, need), (p, need - 1)):
        assert acc(B=3, h=72, w=128, Hg=72, Wg=128, ws=ws, nbytes=nbytes) == -1
        msg = lib.sfh_last_error().decode()
        assert "workspace" in msg and str(need) in msg and (str(need - 1) in msg or ws is None), msg

    def step(part=p, slabs=1, B=1, k=0, last=0, te=p, tn=p, status=p, stats=p):
        return lib.sfh_uvfit_step(part, slabs, B, k, last, te, tn, status, stats, None)

    for kw in (dict(part=None), dict(tn=None), dict(status=None), dict(stats=None)):
        assert step(**kw) == -1 and b"null" in lib.sfh_last_error(), kw
    assert step(te=None, k=1) == -1 and b"theta_eval" in lib.sfh_last_error()
    assert step(te=None, last=1) == -1 and b"theta_eval" in lib.sfh_last_error()
    for kw in (dict(slabs=0), dict(B=0), dict(B=65536), dict(k=-1)):
        assert step(**kw) == -1 and b"geometry" in lib.sfh_last_error(), kw
