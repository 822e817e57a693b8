"""GPU checks of sfh_amd.preparation (csrc/prepare.hip): the rendered labels against the model's own nearest warp and the
oracle, byte for byte; the batched fit against the numpy restatement tests/prep_ref.py; rgb -> ids; the way into
BatchAugment / TrainStep / eval_reconstructor.  Figures of the fit comparison go to profiles/prep_parity.jsonl."""
import json
import os

import numpy as np
import pytest
import torch

import prep_fixtures as F
import prep_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
WH = np.array([1280.0, 720.0])
PARITY = os.path.join(ROOT, "profiles", "prep_parity.jsonl")
_rows = []


def _P():
    from sfh_amd import preparation as P
    return P


def _record(row):
    _rows.append(row)
    print(json.dumps(row))
    try:
        with open(PARITY, "w") as f:
            for r in _rows:
                f.write(json.dumps(r) + "\n")
    except OSError:          # a read-only checkout: the figures are still printed
        pass


def _render_thetas(B):
    """golden / published theta, the identity, a theta putting the whole court outside the frame, a theta whose z crosses
    zero inside the frame, then mild perturbations; float32 (B,3,3)"""
    th = [t for t in F.fixture_thetas()[:4]]
    th.append(np.eye(3))
    th.append(np.array([[1.0, 0, 50.0], [0, 1.0, 50.0], [0, 0, 1.0]]))          # court coordinates 49 .. 51: all outside
    th.append(np.array([[1.0, 0.1, 0.0], [0.0, 1.0, 0.1], [1.5, 0.3, 0.2]]))    # z = 1.5 x + 0.3 y + 0.2 changes sign
    g = np.random.default_rng(23)
    while len(th) < B:
        th.append(np.eye(3) + g.normal(0, 0.06, (3, 3)))
    return torch.from_numpy(np.stack(th[:B]).astype(np.float32))


@pytest.mark.parametrize("size", [(640, 360), (1280, 720)])
@pytest.mark.parametrize("court", ["ncaa_nc4", "pitch_v3_nc4"])
@pytest.mark.parametrize("B", [1, 16, 17])
def test_render_is_the_models_nearest_warp(size, court, B):
    from oracle import warp_ref
    from sfh_amd import engine as E
    P = _P()
    W, H = size
    ids = F.court_ids(f"{court}_{W}x{H}" if (W, H) == (1280, 720) and B == 17 else f"{court}_640x360")
    lm = P.LabelMaker(ids, F.court_poi("pitch"), size, 4, uv=True)
    theta = _render_thetas(7)[6:7] if B == 1 else _render_thetas(B)      # batch 1: the z-crossing one
    out = lm.render(theta.cuda())
    again = lm.render(theta.cuda())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = lm.render(theta.cuda())
    s.synchronize()
    torch.cuda.synchronize()
    mask, uv = out["mask"].cpu(), out["uv"].cpu()
    for o in (again, other):
        assert torch.equal(o["mask"].cpu(), mask) and torch.equal(o["uv"].cpu().view(torch.int16), uv.view(torch.int16))
    tmpl = torch.from_numpy(ids.astype(np.float32) / 4.0)[None, None]
    _, wi = E.homography_warp(theta.cuda().reshape(B, 1, 3, 3), tmpl.cuda(), H, W, True, scale=4.0, want_f32=False,
                              want_i32=True, shared_template=True)
    model = wi.cpu().to(torch.uint8)
    assert int((model != mask).sum()) == 0
    want = (warp_ref.homography_warp(theta, tmpl.expand(B, 1, -1, -1), H, W, "nearest") * 4.0).to(torch.uint8)
    assert int((want != mask).sum()) == 0
    uvn = uv.numpy()
    assert np.array_equal(uvn[..., 0], mask.numpy())
    ix, iy, ok = R.tap_indices(theta, ids.shape, H, W)
    assert np.array_equal(uvn[..., 1], np.where(ok, lm.u_tab[ix], 0))
    assert np.array_equal(uvn[..., 2], np.where(ok, lm.v_tab[iy], 0))
    if B >= 7:
        assert not mask[5].any() and mask[4].any() and mask[6].any()       # all outside / identity / z-crossing


def _geometry_px(theta_c2f, theta_true, court):
    return float(np.abs(F.project_c2f(theta_c2f, court) * WH - F.project(theta_true, court) * WH).max())


@pytest.mark.parametrize("court_name", ["pitch", "ncaa"])
@pytest.mark.parametrize("refine", [0, 10])
def test_fit_exact_data(court_name, refine):
    P = _P()
    court, th = F.court_poi(court_name), F.fixture_thetas()
    th = np.concatenate([th, th[:3]])
    manual, n_short = F.exact_annotations(court, th, seed=3 + refine, n_short=3)
    ign = P.FOOTBALL_PITCH_IGNORE_POINTS
    lm = P.LabelMaker(F.court_ids(), court, (640, 360), 4, ignore_pts=ign, refine=refine)
    got = {k: v.cpu().numpy() for k, v in lm.fit(manual).items()}
    ref = R.fit_batch(court, manual, ignore_pts=ign, refine=refine)
    assert np.array_equal(got["status"], ref["status"]) and int((got["status"] == 0).sum()) == n_short
    assert np.array_equal(got["num_nonzero"], ref["num_nonzero"])
    assert np.array_equal(got["poi"][..., 2], ref["poi"][..., 2])
    for k in ("theta", "theta_c2f", "poi", "reproj_mse"):
        assert not got[k][got["status"] == 0].any(), k
    for b in np.flatnonzero(got["status"] == 1):
        e_gpu, e_ref = _geometry_px(got["theta_c2f"][b], th[b], court), _geometry_px(ref["theta_c2f"][b], th[b], court)
        ulp = EPS * float(np.abs(F.project(th[b], court) * WH).max())       # one fp64 ulp of the coordinate
        _record({"test": "fit_exact", "court": court_name, "refine": refine, "frame": int(b),
                 "points": int(R.usable_points(manual[b]).sum()), "gpu_err_px": e_gpu, "ref_err_px": e_ref, "ulp_px": ulp})
        assert e_gpu <= 2 * e_ref + ulp, (b, e_gpu, e_ref)


def _cost(theta_c2f, court, manual):
    """the one evaluation of the geometric cost (normalised frame coordinates, plain numpy sum)"""
    use = R.usable_points(manual)
    h = np.asarray(theta_c2f).reshape(9)
    x, y = court[use, 0], court[use, 1]
    w = h[6] * x + h[7] * y + h[8]
    rx = (h[0] * x + h[1] * y + h[2]) / w - (manual[use, 0] * 2 - 1)
    ry = (h[3] * x + h[4] * y + h[5]) / w - (manual[use, 1] * 2 - 1)
    return float(np.sum(rx * rx + ry * ry)), int(use.sum())


@pytest.mark.parametrize("noise_px", [1.0, 3.0])
def test_fit_noisy_clicks(noise_px):
    P = _P()
    court, th = F.court_poi("ncaa"), F.fixture_thetas()
    manual, _ = F.exact_annotations(court, th, seed=int(noise_px) + 40, n_short=0, noise_px=noise_px)
    lm = P.LabelMaker(F.court_ids(), court, (640, 360), 4)
    g0 = {k: v.cpu().numpy() for k, v in lm.fit(manual, refine=0).items()}
    g1 = {k: v.cpu().numpy() for k, v in lm.fit(manual, refine=10).items()}
    r0 = R.fit_batch(court, manual, refine=0)
    r1 = R.fit_batch(court, manual, refine=10)
    assert g0["status"].all() and g1["status"].all()
    for b in range(th.shape[0]):
        # refine = 0: no cheap extended-precision reference here, so the exact-data bound (2 x the restatement's error + an
        # ulp) is scaled by the condition figure the restatement reports: the distance between the two DLTs may be at most
        # 64 eps lambda_max / lambda_2 of the coordinate (the perturbation bound of tests/test_prep_host.py), twice
        eig = np.sort(r0["eig"][b])
        span = float(np.abs(F.project(th[b], court) * WH).max())
        bound = 2 * 64 * EPS * (eig[-1] / (eig[1] - eig[0])) * span + EPS * span
        d = float(np.abs(F.project_c2f(g0["theta_c2f"][b], court) * WH - F.project_c2f(r0["theta_c2f"][b], court) * WH).max())
        c_g0, n = _cost(g0["theta_c2f"][b], court, manual[b])
        c_g1, _ = _cost(g1["theta_c2f"][b], court, manual[b])
        c_r1, _ = _cost(r1["theta_c2f"][b], court, manual[b])
        # rounding of the evaluation: 2n squared terms of about 16 roundings each, summed (n more): relative
        margin = (2 * n + 16) * EPS * max(c_g0, c_r1)
        _record({"test": "fit_noisy", "noise_px": noise_px, "frame": b, "points": n, "dlt_gpu_vs_ref_px": d,
                 "dlt_bound_px": bound, "dlt_reference": "condition-scaled exact-data bound", "cost_dlt_gpu": c_g0,
                 "cost_refined_gpu": c_g1, "cost_refined_ref": c_r1, "margin": margin})
        assert d <= bound, (b, d, bound)
        assert c_g1 <= c_g0 + margin, (b, c_g1, c_g0)
        assert c_g1 <= c_r1 + margin, (b, c_g1, c_r1)


def test_fit_outputs_are_consistent():
    P = _P()
    court, th = F.court_poi("pitch"), F.fixture_thetas()
    manual, _ = F.exact_annotations(court, th, seed=77, n_short=0, noise_px=2.0)
    norm = (1280.0, 720.0)
    lm = P.LabelMaker(F.court_ids(), court, (640, 360), 4, ignore_pts=P.FOOTBALL_PITCH_IGNORE_POINTS, norm_size=norm)
    a = lm.fit(manual)
    b2 = lm.fit(torch.from_numpy(manual).cuda())
    got = {k: v.cpu().numpy() for k, v in a.items()}
    for k in a:                                                  # bit-reproducible run to run
        assert np.array_equal(got[k], b2[k].cpu().numpy()), k
    N = court.shape[0]
    for b in range(th.shape[0]):
        c2f, t = got["theta_c2f"][b], got["theta"][b]
        assert c2f[2, 2] == 1.0 and t[2, 2] == 1.0
        prod = t @ c2f
        kappa = np.linalg.cond(c2f)
        assert np.abs(prod / prod[2, 2] - np.eye(3)).max() <= 64 * EPS * kappa
        assert np.array_equal(got["theta_f32"][b], t.astype(np.float32))
        # transform_poi's rule in fp64 on the returned matrix: the same operations, so a few ulp of the coordinate
        want = R.project_poi(c2f, court)
        assert np.abs(got["poi"][b, :, :2] - want).max() <= 8 * EPS * max(1.0, np.abs(want).max())
        # through inverse(theta), as the model does; Kornia's 1e-8 in the divisor is not scale-free, so the inverse is brought
        # to the label's own scale (last entry 1) first
        minv = np.linalg.inv(t)
        via_inv = R.project_poi(minv / minv[2, 2], court)
        assert np.abs(got["poi"][b, :, :2] - via_inv).max() <= 64 * EPS * kappa * max(1.0, np.abs(want).max())
        flags = got["poi"][b, :, 2]
        assert np.array_equal(flags.astype(bool), R.nonzero_flags(manual[b], P.FOOTBALL_PITCH_IGNORE_POINTS))
        pn, mn = got["poi"][b, :, :2] * np.asarray(norm), manual[b] * np.asarray(norm)      # calculate_reprojection_rmse's order
        d = np.sqrt(((pn - mn) ** 2).sum(1))
        rm = float((d * flags).sum() / flags.sum())
        # a distance is a difference of coordinates in pixels: its rounding is an ulp of the COORDINATE (4: two products, the
        # difference, the root), then the N-term sum and the division
        coord = float(np.abs(pn[flags.astype(bool)]).max())
        assert abs(got["reproj_mse"][b] - rm) <= 4 * EPS * coord + 4 * N * EPS * rm
        assert got["num_nonzero"][b] == int(flags.sum())


@pytest.mark.parametrize("nc", [4, 7, 8])
def test_rgb_to_ids(nc):
    from sfh_amd import outputs as O
    P = _P()
    g = np.random.default_rng(nc)
    ids = torch.from_numpy(g.integers(0, nc, (3, 45, 67), dtype=np.uint8)).cuda()       # 9045 pixels: a scalar tail
    rgb = O.format_masks(ids, "rgb", nc)
    assert torch.equal(P.rgb_to_ids(rgb, nc), ids)
    rnd = g.integers(0, 256, (2, 33, 50, 3), dtype=np.uint8)
    pal = O._palette_bytes(8)
    pick = g.random((2, 33, 50)) < 0.5
    rnd[pick] = pal[g.integers(0, 8, int(pick.sum()))]
    got = P.rgb_to_ids(torch.from_numpy(rnd).cuda(), nc).cpu().numpy()
    assert np.array_equal(got, R.rgb_to_ids(rnd, nc))


def test_labels_feed_augment_train_and_eval():
    """annotations from golden theta -> LabelMaker.make -> to_batch -> BatchAugment -> TrainStep.step, and one
    eval_reconstructor batch: no conversion in between, finite losses, labels unchanged by the trip"""
    from sfh_amd import augment as A, synth, training as T
    from sfh_amd.evaluation import eval_reconstructor
    from sfh_amd.reconstructor import Reconstructor
    from conftest import GOLDEN
    P = _P()
    W, H = 128, 96
    court, th = F.court_poi("pitch"), F.fixture_thetas()[:5]
    manual, n_short = F.exact_annotations(court, th, seed=13, n_short=1)
    ids = F.court_ids("pitch_v3_nc4_640x360")
    lm = P.LabelMaker(ids, court, (W, H), 4)
    labels = lm.make(manual)
    frames = torch.from_numpy(synth.synth_frames_u8(5, H, W, seed=3)).cuda()
    batch, dropped = P.to_batch(labels, frames, names=[f"f{k}" for k in range(5)])
    assert dropped == ["f4"] and len(dropped) == n_short and batch["name"] == ["f0", "f1", "f2", "f3"]
    B = 4
    keep = {k: v.clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
    tmpl = torch.from_numpy(ids.astype(np.float32) / 4.0)[None, None].repeat(B, 1, 1, 1).cuda()
    cpoi = synth.load_court_poi("pitch", B).cuda()
    net = Reconstructor(tmpl, cpoi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 47))
    net.cuda().train()
    ts = T.TrainStep(net, lr=1e-4)
    aug = A.BatchAugment({'apperance': {'jitter': {}}, 'geometric': {'hflip': 0.5, 'poi_flip_map':
                          os.path.join(GOLDEN, "pitch-poi-flip-mapping.json")}}, target_size=(W, H))
    g = torch.Generator().manual_seed(5)
    out = aug(batch["frames_u8"], batch["mask_u8"], poi=batch["poi"], nonzeros=batch["nonzeros"], generator=g)
    losses = ts.step(out["image"], {**batch, **out})
    assert bool(torch.isfinite(losses).all()), losses
    res = eval_reconstructor(net, [batch], "cuda", (W, H))
    assert all(np.isfinite(v) for k, v in res.items() if k.startswith("val_")), res
    for k, v in keep.items():
        assert torch.equal(batch[k], v), k
    # the mask the model is trained against is the model's own nearest warp of the label theta
    from sfh_amd import engine as E
    _, wi = E.homography_warp(batch["theta"].reshape(B, 1, 3, 3), tmpl, H, W, True, scale=4.0, want_f32=False,
                              want_i32=True, shared_template=False)
    assert torch.equal(wi.to(torch.int64), batch["mask"])
