"""GPU checks of the homography refinement (csrc/refine.hip, sfh_amd.refine) against the numpy restatement
tests/refine_ref.py: the four kernels one by one, then the whole schedule, then the hook in Reconstructor.predict().
Every output sits behind 64-element guards, overwritten outputs are pre-filled with NaN, and every comparison prints
``RATIO name: error / bound`` and asserts it <= 1.  The rows of the convergence comparison go to profiles/refine_parity.jsonl."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import det_ref
import refine_cases as K
import refine_ref as R
import step_tail_ref as ST
from conftest import ROOT

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64
PARITY = os.path.join(ROOT, "profiles", "refine_parity.jsonl")
_rows = []


def _lib():
    from sfh_amd import _lib as L
    return L, L.load()


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _st():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """a device buffer of `shape` between two guards of 64 elements, all NaN (integers: a sentinel) before the run"""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.fill = float("nan") if dtype.is_floating_point else -7777
        self.full = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + n].view(shape)

    def intact(self):
        g = torch.cat([self.full[:GUARD], self.full[-GUARD:]]).cpu()
        return bool(torch.isnan(g).all()) if g.dtype.is_floating_point else bool((g == self.fill).all())

    def untouched(self):
        f = self.full.cpu()
        return bool(torch.isnan(f).all()) if f.dtype.is_floating_point else bool((f == self.fill).all())


def _record(row):
    _rows.append(row)
    print(json.dumps(row))
    try:
        with open(PARITY, "w") as f:
            for r in _rows:
                f.write(json.dumps(r) + "\n")
    except OSError:          # a read-only checkout: the figures are still printed
        pass


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ 1. template planes
@pytest.mark.parametrize("n", [1, 3], ids=["shared", "per-frame"])
@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("nc", [4, 7, 8])
def test_template_planes(nc, f, n):
    L, lib = _lib()
    tmpl = K.template(nc, n)
    want = R.template_planes(tmpl[:, 0], nc, f)
    out = Guarded(want.shape)
    L.check(lib.sfh_refine_template_planes(_p(torch.from_numpy(tmpl).cuda()), n, K.HT, K.WT, nc, f, _p(out.t), _st()), "planes")
    got = out.t.cpu().numpy()
    assert out.intact() and np.array_equal(_bits(got), _bits(want))
    assert not got[..., nc - 1:].any() and got[..., :nc - 1].any(axis=(0, 1, 2)).all()
    print(f"RATIO template_planes nc={nc} f={f} n={n}: 0 (bit-equal, {got.size} values)")


# ------------------------------------------------------------------------------------------------ 2. evidence planes
def _logits(nc, h=K.H, w=K.W, seed=3):
    """frame 0: randn * 4; frame 1: +-80, which saturate; frame 2: equal logits"""
    g = np.random.default_rng(seed)
    lg = np.zeros((3, nc, h, w), dtype=F32)
    lg[0] = g.normal(0, 4, (nc, h, w))
    lg[1] = np.where(g.random((nc, h, w)) < 0.5, 80.0, -80.0)
    lg[2] = F32(1.25)
    return lg


@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("nc", [4, 7, 8])
def test_evidence_planes(nc, f):
    L, lib = _lib()
    lg = _logits(nc)
    want, bound = R.evidence_planes(lg, f)
    out = Guarded(want.shape)
    L.check(lib.sfh_refine_evidence_planes(_p(torch.from_numpy(lg).cuda()), 3, nc, K.H, K.W, f, _p(out.t), _st()), "evidence")
    got = out.t.cpu().numpy()
    assert out.intact() and not got[..., nc - 1:].any()
    for b, kind in enumerate(("randn", "saturated", "equal")):
        ratio = ST.ratio(got[b], want[b], bound[b])
        print(f"RATIO evidence_planes nc={nc} f={f} {kind}: {ratio:.3g}")
        assert ratio <= 1.0
    assert np.abs(got[2, ..., :nc - 1] - 1.0 / nc).max() <= 4 * R.U


# ------------------------------------------------------------------------------------------------ 3. accumulate
#            nc  hl   wl   H    W    f      evidence grid
ACC_CASES = [(4, 72, 128, 72, 128, 1),    # 72 x 128: whole workgroups in x, a last one of 8 rows in y
             (4, 72, 128, 72, 128, 4),    # 18 x 32: one workgroup, partly filled in both directions
             (4, 40, 72, 40, 72, 2),      # 20 x 36 from a 40 x 72 frame: neither direction fills its last workgroup
             (4, 72, 136, 72, 136, 1),    # 72 x 136: three workgroups across, the last of 8 columns, above a row of 8 rows
             (4, 36, 64, 72, 128, 1),     # logits at half the warp grid: the ax / cx rule
             (7, 72, 128, 72, 128, 2)]    # CP = 8: the pad channels of both operands meet


def _accumulate(lib, L, theta, tp, bstride, ht, wt, ev, B, nc, hl, wl, H, W, f, ws, nbytes):
    return lib.sfh_refine_accumulate(_p(theta), _p(tp), bstride, ht, wt, _p(ev), B, nc, hl, wl, H, W, f, _p(ws), nbytes, _st())


@pytest.mark.parametrize("case", ACC_CASES, ids=[f"nc{c[0]}-{c[2]}x{c[1]}-f{c[5]}" for c in ACC_CASES])
def test_accumulate(case):
    nc, hl, wl, H, W, f = case
    L, lib = _lib()
    he, we = hl // f, wl // f
    _, yn = R.grid(f, H, W, hl, wl)
    thetas = K.kernel_thetas(yn, he // 2 + 1)
    B = thetas.shape[0]
    tmpl = K.template(nc)
    tp = R.template_planes(tmpl[:, 0], nc, f)
    lg = np.random.default_rng(nc + f).normal(0, 3, (B, nc, hl, wl)).astype(F32)
    ev = R.evidence_planes_f32(lg, f)
    ref, A = R.sums(thetas, tp, ev, H, W, f)
    bound = R.sums_bound(A, he * we)

    nslab = R.slabs(he, we)
    need = lib.sfh_refine_workspace_bytes(B, he, we)
    assert need == nslab * B * R.SUMS * 8
    d_theta, d_tp, d_ev = (torch.from_numpy(a).cuda() for a in (thetas, tp, ev))
    args = (d_theta, d_tp, 0, K.HT, K.WT, d_ev, B, nc, hl, wl, H, W, f)

    ws = Guarded((nslab, B, R.SUMS), torch.float64)
    assert _accumulate(lib, L, *args, ws.t, need - 1) == -1 and b"workspace" in lib.sfh_last_error()
    torch.cuda.synchronize()
    assert ws.untouched()                                         # one byte short: nothing written
    L.check(_accumulate(lib, L, *args, ws.t, need), "accumulate")
    part = ws.t.cpu().numpy()
    assert ws.intact() and np.isfinite(part).all()                # every slab element written
    got = np.stack([det_ref.det_sum(np.zeros(R.SUMS), part[:, b]) for b in range(B)])
    for b, kind in enumerate(("near-identity", "partly-outside", "outside", "z0-row", "z-sign-change")):
        ratio = ST.ratio(got[b], ref[b], bound[b])
        print(f"RATIO accumulate {case} {kind}: {ratio:.3g}")
        assert ratio <= 1.0, (kind, got[b], ref[b])
    # entirely outside: every tap is zero - the 44 derivative sums are exactly 0 and the cost is sum E^2
    assert not got[2, :44].any() and not ref[2, :44].any()
    e2 = float((ev[2].astype(np.float64) ** 2).sum())
    assert abs(ref[2, 44] - e2) <= 1e-12 * e2 and abs(got[2, 44] - e2) <= bound[2, 44] + 1e-12 * e2
    # the Z = 0 row: the `live` rule - s = 1 and no Z-derivative on that row (the restatement's own a, b say so)
    q = R.pixel_terms(thetas[3:4], tp, ev[3:4], H, W, f)
    row = he // 2 + 1
    assert not q["a"][6:, 0, row].any() and not q["b"][6:, 0, row].any() and (q["a"][2, 0, row] == 1.0).all()
    assert q["a"][6:, 0, row - 1].any()

    # a second call, and a call on a side stream beside a busy stream: the same bits
    ws2 = Guarded((nslab, B, R.SUMS), torch.float64)
    L.check(_accumulate(lib, L, *args, ws2.t, need), "accumulate")
    busy = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    ws3 = Guarded((nslab, B, R.SUMS), torch.float64)
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        L.check(_accumulate(lib, L, *args, ws3.t, need), "accumulate")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ws2.t.cpu().numpy()), _bits(part)) and np.array_equal(_bits(ws3.t.cpu().numpy()), _bits(part))


def test_accumulate_per_frame_templates():
    """three templates, three frames: frame b reads its own planes through the batch stride"""
    L, lib = _lib()
    nc, f, B = 4, 2, 3
    tmpl = K.template(nc, B)
    tp = R.template_planes(tmpl[:, 0], nc, f)
    thetas = np.repeat(K.THETA_TRUE[None], B, axis=0)
    ev = R.evidence_planes_f32(K.onehot_logits(thetas, tmpl, nc, 8.0), f)
    ref, A = R.sums(thetas, tp, ev, K.H, K.W, f)
    need = lib.sfh_refine_workspace_bytes(B, K.H // f, K.W // f)
    ws = Guarded((need // 8,), torch.float64)
    d_theta, d_tp, d_ev = (torch.from_numpy(a).cuda() for a in (thetas, tp, ev))
    L.check(lib.sfh_refine_accumulate(_p(d_theta), _p(d_tp), tp[0].size, K.HT, K.WT, _p(d_ev), B, nc, K.H, K.W, K.H, K.W, f,
                                      _p(ws.t), need, _st()), "acc")
    part = ws.t.cpu().numpy().reshape(-1, B, R.SUMS)
    got = np.stack([det_ref.det_sum(np.zeros(R.SUMS), part[:, b]) for b in range(B)])
    ratio = ST.ratio(got, ref, R.sums_bound(A, (K.H // f) * (K.W // f)))
    print(f"RATIO accumulate per-frame templates: {ratio:.3g}")
    assert ws.intact() and ratio <= 1.0 and not np.array_equal(ref[0], ref[1])


# ------------------------------------------------------------------------------------------------ 4. step
def _system(g, kind, nslab):
    """partial slabs (nslab, 45) float64 of one frame"""
    J = g.normal(size=(60, 8))
    r = g.normal(size=60)
    S = np.concatenate([(J.T @ J)[np.triu_indices(8)], J.T @ r, [r @ r]])
    if kind == "singular":
        S[:] = 0.0
        S[44] = 3.0
    if kind == "nan":
        S[44] = np.nan
    if kind == "cancelling":      # +G early, -G last, G = 1e6 |S|: the chain's bits depend on the order, its value stays near S
        w = g.random((nslab - 2, 1))
        parts, G = S[None] * (w / w.sum()), 1e6 * np.abs(S) + 1.0
        return np.concatenate([parts[:10], G[None], parts[10:], -G[None]])
    w = g.random((nslab, 1))
    return S[None] * (w / w.sum())


def test_step():
    """two calls on slabs written here: first = 1 adopts, first = 0 decides.  Frames: SPD (a lower cost: accepted), SPD (a
    higher cost: rejected), cancelling slabs, a singular system, a NaN cost on the second call."""
    L, lib = _lib()
    g = np.random.default_rng(17)
    kinds = ("spd", "spd", "cancelling", "singular", "spd")
    B, nslab = len(kinds), 37
    p1 = np.stack([_system(g, k, nslab) for k in kinds], axis=1)                     # (nslab, B, 45)
    p2 = np.stack([_system(g, k, nslab) for k in ("spd", "spd", "spd", "spd", "nan")], axis=1)
    c1 = np.stack([det_ref.det_sum(np.zeros(R.SUMS), p1[:, b]) for b in range(B)])[:, 44]
    p2[-1, 0, 44] += 0.5 * c1[0] - det_ref.det_sum(np.zeros(R.SUMS), p2[:, 0])[44]      # frame 0: about half the cost
    p2[-1, 1, 44] += 2.0 * c1[1] - det_ref.det_sum(np.zeros(R.SUMS), p2[:, 1])[44]      # frame 1: twice
    p2[-1, 2, 44] += 0.5 * c1[2] - det_ref.det_sum(np.zeros(R.SUMS), p2[:, 2])[44]
    theta0 = (np.eye(3).reshape(1, 9) + g.normal(0, 0.1, (B, 9))).astype(F32)

    acc, sums, lam = Guarded((B, 9)), Guarded((B, R.SUMS), torch.float64), Guarded((B,), torch.float64)
    ok, nxt = Guarded((B,), torch.int32), Guarded((B, 9))
    cost, accepted = Guarded((B, 2, 2), torch.float64), Guarded((B, 2), torch.int32)
    d_theta = torch.from_numpy(theta0).cuda()

    def call(part, first, last, t_eval):
        L.check(lib.sfh_refine_step(_p(torch.from_numpy(part).cuda()), nslab, B, first, last, _p(t_eval), _p(acc.t), _p(sums.t),
                                    _p(lam.t), _p(ok.t), _p(nxt.t), _p(cost.t), _p(accepted.t), 1, 2, _st()), "step")
        torch.cuda.synchronize()
        return {k: v.t.cpu().numpy().copy() for k, v in (("acc", acc), ("sums", sums), ("lam", lam), ("ok", ok), ("next", nxt),
                                                          ("cost", cost), ("accepted", accepted))}

    states = [R.StepState() for _ in range(B)]
    ties = 0
    for part, first, t_eval in ((p1, 1, d_theta), (p2, 0, None)):
        t_eval = nxt.t.clone() if t_eval is None else t_eval
        ev_np = t_eval.cpu().numpy()
        got = call(part, first, 0, t_eval)
        for b in range(B):
            S = det_ref.det_sum(np.zeros(R.SUMS), part[:, b])
            cand, tie = states[b].step(S, ev_np[b], bool(first), False)
            st = states[b]
            # the fixed-order sum: bit-equal to the ascending chain (NaN meets NaN)
            assert np.array_equal(_bits(got["sums"][b]), _bits(st.S)), (b, first)
            assert got["lam"][b] == st.lam and bool(got["ok"][b]) == st.ok and got["accepted"][b, 1] == st.accepted
            assert np.array_equal(_bits(got["acc"][b]), _bits(st.theta))
            assert got["cost"][b, 1, 1] == st.S[44] and got["cost"][b, 1, 0] == st.cost_first
            same = _bits(got["next"][b]) == _bits(cand)
            off = np.abs(_bits(got["next"][b]).astype(np.int64) - _bits(cand).astype(np.int64))
            assert (same | (tie & (off <= 1))).all(), (b, got["next"][b], cand)
            ties += int((~same).sum())
    print(f"RATIO step: 0 (decisions, lambda, counters and sums equal; {ties} candidates off by one ulp at a flagged tie)")
    assert [s.accepted for s in states] == [1, 0, 1, 0, 0] and [s.ok for s in states] == [True, True, True, False, True]
    assert states[3].lam == 1e-2 and states[0].lam == 1e-4 and states[4].lam == 1e-2
    # level 0 of cost / accepted was not this call's: still NaN / sentinel; every guard intact
    assert np.isnan(cost.t.cpu().numpy()[:, 0]).all() and (accepted.t.cpu().numpy()[:, 0] == -7777).all()
    assert all(x.intact() for x in (acc, sums, lam, ok, nxt, cost, accepted))
    got = call(p2, 0, 1, nxt.t.clone())                                   # last: theta_next is the accepted theta
    assert np.array_equal(_bits(got["next"]), _bits(got["acc"]))


# ------------------------------------------------------------------------------------------------ 5. the whole refinement
def _refiner(tmpl, nc=4, **kw):
    from sfh_amd.refine import ThetaRefiner
    return ThetaRefiner(torch.from_numpy(tmpl).cuda(), mask_classes=nc, grid_size=(K.W, K.H), **kw)


@pytest.mark.parametrize("name", ["exact", "noisy"])
def test_whole_refinement(name):
    sc = K.scene(name)
    n = len(sc["starts"])
    fs = (4, 2, 1)
    tps = [R.template_planes(sc["tmpl"][:, 0], 4, f) for f in fs]
    evs = [R.evidence_planes_f32(sc["logits"], f) for f in fs]
    ref = R.refine(sc["starts"], tps, evs, K.H, K.W)
    r = _refiner(sc["tmpl"])
    out = r(torch.from_numpy(sc["starts"]).cuda().view(n, 1, 3, 3), torch.from_numpy(sc["logits"]).cuda())
    again = r(torch.from_numpy(sc["starts"]).cuda().view(n, 1, 3, 3), torch.from_numpy(sc["logits"]).cuda())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert all(torch.equal(out[k], again[k]) for k in out)
    assert got["theta"].shape == (n, 1, 3, 3) and got["cost"].shape == (n, 3, 2) and got["accepted"].shape == (n, 3)
    # the accept rule, exactly: the last cost of every level is at most its first
    assert (got["cost"][:, :, 1] <= got["cost"][:, :, 0]).all()
    e_gpu = R.corner_error(got["theta"], sc["theta_true"], K.WT, K.HT)
    e_ref = R.corner_error(ref["theta"], sc["theta_true"], K.WT, K.HT)
    ulp = float(np.spacing(F32(max(K.WT, K.HT))))                          # one fp32 ulp of the coordinate
    # one host evaluation of the finest level's cost for both sides (refine_ref.eval_cost on the restatement's planes), as
    # test_gpu_prep._cost does; the margin is the rounding of that evaluation alone (refine_ref.cost_margin)
    c_gpu = R.eval_cost(got["theta"].reshape(n, 9), tps[-1], evs[-1], K.H, K.W, 1)
    c_ref = R.eval_cost(ref["theta"], tps[-1], evs[-1], K.H, K.W, 1)
    cmax = float(c_ref.max())
    limit = cmax + float(c_ref.max() - c_ref.min()) + R.cost_margin(K.H * K.W, cmax)
    for k in range(n):
        _record({"test": "whole_refinement", "scene": name, "start": k, "start_px": float(sc["offsets"][k]),
                 "gpu_err_px": float(e_gpu[k]), "ref_err_px": float(e_ref[k]), "ulp_px": ulp,
                 "cost_gpu": float(c_gpu[k]), "cost_ref": float(c_ref[k]), "cost_limit": limit,
                 "cost_reported_gpu": float(got["cost"][k, -1, 1]), "cost_reported_ref": float(ref["cost"][k, -1, 1]),
                 "accepted_gpu": got["accepted"][k].tolist(), "accepted_ref": ref["accepted"][k].tolist()})
        print(f"RATIO whole_refinement {name} start {k}: corner {e_gpu[k] / (2 * e_ref[k] + ulp):.3g}, "
              f"cost {c_gpu[k] / limit:.6g}")
        assert e_gpu[k] <= 2 * e_ref[k] + ulp, (k, e_gpu[k], e_ref[k])
        assert c_gpu[k] <= limit, (k, c_gpu[k], limit)


# ------------------------------------------------------------------------------------------------ 6. / 7. the quiet cases
def test_dead_frame():
    """all-background evidence, the template entirely outside: theta bit for bit, nothing accepted, the cost unchanged"""
    tmpl = K.template(4)
    lg = np.zeros((K.B, 4, K.H, K.W), dtype=F32)
    lg[:, 0] = 8.0
    theta = np.repeat(np.array([[1.0, 0, 50.0, 0, 1.0, 50.0, 0, 0, 1.0]], dtype=F32), K.B, axis=0)
    out = _refiner(tmpl)(torch.from_numpy(theta).cuda().view(K.B, 1, 3, 3), torch.from_numpy(lg).cuda())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(_bits(got["theta"].reshape(K.B, 9)), _bits(theta)) and not got["accepted"].any()
    assert np.array_equal(got["cost"][..., 0], got["cost"][..., 1]) and (got["cost"] > 0).all()


def test_zero_iterations():
    """iters = 0: of the three outputs only `cost` carries anything - theta is the input bit for bit (a fresh tensor; the input
    itself is not written), `accepted` is all zero, and the first and last cost of a level are one number: the cost of the
    input at that level, which falls within the evidence planes' rounding of the restatement's"""
    sc = K.scene("exact")
    start = sc["starts"][:K.B]
    th = torch.from_numpy(start).cuda().view(K.B, 1, 3, 3)
    lg = torch.from_numpy(sc["logits"][:K.B]).cuda()
    out = _refiner(sc["tmpl"], iters=0)(th, lg)
    assert out["theta"].data_ptr() != th.data_ptr() and torch.equal(out["theta"], th)
    assert np.array_equal(_bits(th.cpu().numpy().reshape(K.B, 9)), _bits(start))
    assert np.array_equal(lg.cpu().numpy(), sc["logits"][:K.B])
    assert out["accepted"].shape == (K.B, 3) and not out["accepted"].any().item()
    c = out["cost"].cpu().numpy()
    assert np.array_equal(c[..., 0], c[..., 1]) and np.isfinite(c).all()
    for li, f in enumerate((4, 2, 1)):
        want = R.eval_cost(start, R.template_planes(sc["tmpl"][:, 0], 4, f), R.evidence_planes_f32(sc["logits"][:K.B], f), K.H, K.W, f)
        _, eb = R.evidence_planes(sc["logits"][:K.B], f)
        # the device's planes and numpy's differ by d <= 2 * evidence bound per element: |C(E + d) - C(E)| <= 2 sqrt(C) |d| + |d|^2
        dn = 2.0 * np.sqrt((eb ** 2).sum(axis=(1, 2, 3)))
        tol = 2.0 * np.sqrt(want) * dn + dn * dn + R.cost_margin((K.H // f) * (K.W // f), 1.0) * want
        print(f"RATIO zero_iterations level {f}: {float((np.abs(c[:, li, 0] - want) / tol).max()):.3g}")
        assert (np.abs(c[:, li, 0] - want) <= tol).all()


def test_refiner_caches_and_refuses():
    sc = K.scene("exact")
    r = _refiner(sc["tmpl"])
    th, lg = torch.from_numpy(sc["starts"][:K.B]).cuda().view(K.B, 1, 3, 3), torch.from_numpy(sc["logits"][:K.B]).cuda()
    r(th, lg)
    planes, work = r._tmpl[2], dict(r._work)
    torch.cuda.synchronize()
    before = torch.cuda.memory_reserved()
    r(th, lg)
    assert r._tmpl[2] is planes and r._work == work and len(work) == 1 and torch.cuda.memory_reserved() == before
    # template planes built on one stream, used at once on another: the second call waits for the build through an event
    want = {k: v.clone() for k, v in r(th, lg).items()}
    fresh, side = _refiner(sc["tmpl"]), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = fresh(th, lg)
    second = fresh(th, lg)                                        # the caller's stream, no synchronisation in between
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], want[k]) and torch.equal(second[k], want[k]) for k in want) and len(fresh._work) == 2
    per_frame = _refiner(K.template(4, 2))
    with pytest.raises(ValueError, match="exceeds"):
        per_frame(th, lg)
    with pytest.raises(ValueError, match="CUDA"):
        r(th.cpu(), lg)


# ------------------------------------------------------------------------------------------------ 8. the hook
def _model():
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    court = torch.from_numpy(K.template(4)).expand(K.B, 1, -1, -1).contiguous().cuda()      # one template, replicated
    poi = synth.load_court_poi("pitch", K.B).cuda()
    net = Reconstructor(court, poi, target_size=(K.W, K.H), unet_size=(K.W, K.H), warp_size=(K.W, K.H), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    return net.cuda().eval(), synth.smooth_frames(K.B, K.H, K.W, seed=19).cuda()


def test_hook_off_changes_nothing():
    """refiner = None against a model on which the attribute does not exist"""
    a, x = _model()
    b, _ = _model()
    del b.__dict__["refiner"]
    with torch.no_grad():
        oa, ob = a.predict(x, consistency=True, project_poi=True), b.predict(x, consistency=True, project_poi=True)
        pa = a.predict_async(x, consistency=True, project_poi=True).result()
    assert set(oa) == set(ob) == set(pa) == {"logits", "theta", "warp_mask", "consist_score", "poi"}
    assert all(torch.equal(oa[k], ob[k]) and torch.equal(oa[k], pa[k]) for k in oa)


def test_hook_on():
    from sfh_amd import engine as E
    from sfh_amd.refine import ThetaRefiner
    plain, x = _model()
    net, _ = _model()
    net.refiner = ThetaRefiner(net.court_img, mask_classes=4, grid_size=net.warp_size)
    with torch.no_grad():
        want = plain.predict(x, consistency=True, project_poi=True)
        out = net.predict(x, consistency=True, project_poi=True)
        assert set(out) == set(want) | {"theta_stn"}
        assert torch.equal(out["theta_stn"], want["theta"]) and torch.equal(out["logits"], want["logits"])
        ref = net.refiner(out["theta_stn"], out["logits"])["theta"]
        assert torch.equal(out["theta"], ref)
        wm, score = E.warp_consistency(ref, net.court_img.contiguous(), out["logits"], 4.0, shared_template=True,
                                       warp_hw=(K.H, K.W))
        assert torch.equal(out["warp_mask"], wm) and torch.equal(out["consist_score"], score)
        assert torch.equal(out["poi"], plain.transform_poi(ref, plain.court_poi))
        again = net.predict_async(x, consistency=True, project_poi=True).result()
        assert all(torch.equal(again[k], out[k]) for k in out)
        net.graph_replay = True                              # replay falls through to predict()
        for _ in range(2):
            rep = net.predict(x, consistency=True, project_poi=True)
            assert all(torch.equal(rep[k], out[k]) for k in out)
        assert not net.__dict__.get("_replay")
        net.graph_replay = False
        clone = pickle.loads(pickle.dumps(net))
        assert clone.refiner._tmpl is None and clone.refiner._work == {} and clone.refiner.factors == (4, 2, 1)
        back = clone.cuda().eval().predict(x, consistency=True, project_poi=True)
        assert all(torch.equal(back[k], out[k]) for k in out)
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    no_unet = Reconstructor(net.court_img, net.court_poi, target_size=(K.W, K.H), unet_size=(K.W, K.H), warp_size=(K.W, K.H),
                            warp_with_nearest=True, use_unet=False, resnet_input="img")
    no_unet.load_state_dict(synth.synth_state_dict(no_unet.state_dict(), 19))
    no_unet.cuda().eval()
    no_unet.refiner = net.refiner
    with torch.no_grad(), pytest.raises(ValueError, match="evidence"):      # no UNet, no evidence
        no_unet.predict(x)
