"""GPU checks of the UV homography fit (csrc/uvfit.hip, sfh_amd.uvfit) against the numpy restatement tests/uvfit_ref.py: the
two kernels one by one, then the whole schedule, then the hooks in Reconstructor.predict() and metrics.evaluate_registration.
Every output and the workspace sit behind 64-element guards, overwritten outputs are pre-filled with NaN (integers: a
sentinel), and every comparison prints ``RATIO name: error / bound`` and asserts it <= 1.  The rows of the whole-fit
comparison go to profiles/uvfit_parity.jsonl (test "whole_fit")."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import det_ref
import step_tail_ref as ST
import uvfit_cases as K
import uvfit_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64
PARITY = os.path.join(ROOT, "profiles", "uvfit_parity.jsonl")


def _lib():
    from sfh_amd import _lib as L
    return L, L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _consts():
    u_min, v_min, kx, ky = R.constants(K.WT, K.HT)
    return float(u_min), float(v_min), kx, ky


def _accumulate(lib, uv, lg, nc, th, B, h, w, Hg, Wg, ws, nbytes, delta=2.0):
    return lib.sfh_uvfit_accumulate(_p(uv), _p(lg), nc, _p(th), B, h, w, Hg, Wg, K.WT, K.HT, *_consts(), delta, _p(ws), nbytes, _st())


def _total(part, B):
    """the ascending chain over the slabs, per frame: (B,27)"""
    return np.stack([det_ref.det_sum(np.zeros(R.SUMS), part[:, b]) for b in range(B)])


# ------------------------------------------------------------------------------------------------ 1. accumulate
@pytest.mark.parametrize("p", K.ACC_PARAMS, ids=[K.acc_id(p) for p in K.ACC_PARAMS])
def test_accumulate(p):
    (h, w), B, nc, _ = p
    L, lib = _lib()
    c = K.accumulate_case(p)
    Hg, Wg = c["H"], c["W"]
    nslab = R.slabs(h, w)
    need = lib.sfh_uvfit_workspace_bytes(B, h, w)
    assert need == nslab * B * R.SUMS * 8
    d_uv, d_lg = _dev(c["uv"]), _dev(c["logits"])
    gate = R.gate(c["uv"], c["logits"], K.WT, K.HT)
    n_ref = gate.reshape(B, -1).sum(axis=1)
    if w >= 6:      # the two pixels ON the thresholds are out, by the strict comparison alone (a >= gate would count them)
        ge = (c["uv"][0, 0] >= R.constants(K.WT, K.HT)[0]) & (c["uv"][0, 1] >= R.constants(K.WT, K.HT)[1])
        assert not gate[0, 0, 2] and not gate[0, 0, 4] and ge[0, 2] and ge[0, 4]
    for name, th in zip(c["names"], c["thetas"]):
        d_th = _dev(th)
        args = (d_uv, d_lg, nc or 0, d_th, B, h, w, Hg, Wg)
        ws = Guarded((nslab, B, R.SUMS), torch.float64)
        if name == "none":
            assert _accumulate(lib, *args, ws.t, need - 1) == -1 and b"workspace" in lib.sfh_last_error()
            torch.cuda.synchronize()
            assert ws.untouched()                                     # one byte short: nothing written
        L.check(_accumulate(lib, *args, ws.t, need), "accumulate")
        part = ws.t.cpu().numpy()
        assert ws.intact() and not np.isnan(part).any()               # every slab element written
        got = _total(part, B)
        ref, A, n = R.sums(c["uv"], c["logits"], th, Hg, Wg, K.WT, K.HT)
        bound = R.sums_bound(A, n)
        bound[:, 24:26] = 0.0                                         # the integer sums: equal
        assert np.array_equal(n, n_ref) and np.array_equal(got[:, 24], n_ref.astype(np.float64)) and np.array_equal(got[:, 25], ref[:, 25])
        ratio = ST.ratio(got, ref, bound)
        print(f"RATIO accumulate {K.acc_id(p)} theta={name}: {ratio:.3g}  (n {n.tolist()}, inliers {ref[:, 25].tolist()})")
        assert ratio <= 1.0, (name, got, ref)
        if name in ("none", "nan"):                                   # no theta: 25 and 26 are 0; a NaN theta: the moments too
            assert not got[:, 25:].any()
        if name == "nan":
            assert not got[:, :24].any() and not np.signbit(got[:, :24]).any()
        if B == 3:                                                    # the all-zero frame: n = 0, every sum exactly +0.0
            assert not part[:, 1].any() and not np.signbit(part[:, 1]).any()
        if name == "zoom":
            # a second call, and a call on a side stream beside a busy stream: the same bits
            ws2, ws3 = Guarded((nslab, B, R.SUMS), torch.float64), Guarded((nslab, B, R.SUMS), torch.float64)
            L.check(_accumulate(lib, *args, ws2.t, need), "accumulate")
            busy = torch.randn(1024, 1024, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            for _ in range(4):
                busy = busy @ busy * 1e-3
            with torch.cuda.stream(side):
                L.check(_accumulate(lib, *args, ws3.t, need), "accumulate")
            torch.cuda.synchronize()
            assert np.array_equal(_bits(ws2.t.cpu().numpy()), _bits(part)) and np.array_equal(_bits(ws3.t.cpu().numpy()), _bits(part))
            assert ws2.intact() and ws3.intact()
    if (h, w) == (2, 2) and nc is None:
        assert n_ref[0] == 4                                          # four pixels: the exactly determined system


# ------------------------------------------------------------------------------------------------ 2. step
def test_step():
    """The device's own partials (72 x 136, six slabs) are fed to the restatement of the step.  Frames: 0 a solved SPD system;
    1 all gated pixels on one row (rank-deficient); 2 n = 3; 3 a pixel with u = +inf (a non-finite sum); 4 SPD with cancelling
    slabs (+G onto slab 0, -G onto the last, G = 1e6 |S|); 5 SPD on pass 0, a NaN sum on pass 1 (dead with its last solved
    theta).  Three calls: pass 0 without and with a theta0 (the first two dead-frame thetas), pass 1, last."""
    L, lib = _lib()
    h, w, B = 72, 136, 6
    full = K.exact_uv(K.ZOOM, h, w)
    row, three, inf = np.zeros_like(full), np.zeros_like(full), full.copy()
    row[:, 40] = full[:, 40]
    three[:, 40, 70:73] = full[:, 40, 70:73]
    inf[0, 10, 10] = np.inf
    uv = np.stack([full, row, three, inf, K.exact_uv(K.PERSPECTIVE, h, w), full])
    d_uv = _dev(uv)
    nslab = R.slabs(h, w)
    need = lib.sfh_uvfit_workspace_bytes(B, h, w)
    theta0 = np.repeat(K.shifted(K.ZOOM)[None], B, axis=0)

    def partials(th, edit):
        ws = Guarded((nslab, B, R.SUMS), torch.float64)
        L.check(_accumulate(lib, d_uv, None, 0, th, B, h, w, h, w, ws.t, need), "accumulate")
        part = ws.t.cpu().numpy().copy()
        assert ws.intact()
        edit(part)
        return part

    def cancel(part):
        G = 1e6 * np.abs(part[:, 4].sum(axis=0)) + 1.0
        part[0, 4] += G
        part[-1, 4] -= G

    def call(part, k, last, t_eval):
        nxt, status, stats = Guarded((B, 9)), Guarded((B,), torch.int32), Guarded((B, 4), torch.float64)
        if k > 0:
            status.t.copy_(call.status)
        L.check(lib.sfh_uvfit_step(_p(_dev(part)), nslab, B, k, last, _p(t_eval), _p(nxt.t), _p(status.t), _p(stats.t), _st()), "step")
        torch.cuda.synchronize()
        assert nxt.intact() and status.intact() and stats.intact()
        call.status = status.t.clone()
        return nxt.t.cpu().numpy().copy(), status.t.cpu().numpy().copy(), stats.t.cpu().numpy().copy()

    ties = 0

    def compare(got, part, k, last, t_eval, status_in):
        nonlocal ties
        for b in range(B):
            S = det_ref.det_sum(np.zeros(R.SUMS), part[:, b])
            tn, st, stats, tie = R.step(S, k, last, None if t_eval is None else t_eval[b], status_in[b])
            assert got[1][b] == st, (k, b, got[1][b], st)
            assert np.array_equal(_bits(got[0][b]), _bits(tn)), (k, b, got[0][b], tn)
            assert np.array_equal(got[2][b], stats, equal_nan=True), (k, b, got[2][b], stats)
            ties += int(tie.sum())
        return got

    for th0 in (None, theta0):
        p0 = partials(_dev(th0), cancel)
        g0 = compare(call(p0, 0, 0, _dev(th0)), p0, 0, False, th0, np.zeros(B, dtype=np.int32))
        # frame 3: without a theta the infinite cx reaches the sums; under theta0 its r2 is infinite, omega = 0, and it solves
        assert g0[1].tolist()[0] == 1 and g0[1].tolist()[2:] == [0, 0 if th0 is None else 1, 1, 1]
        for b in (2, 3) if th0 is None else (2,):                     # dead at once: nine NaNs, or theta0
            assert np.isnan(g0[0][b]).all() if th0 is None else np.array_equal(_bits(g0[0][b]), _bits(th0[b]))
        assert (g0[0][[0, 4, 5], 8] == 1.0).all() and g0[2][:4, 0].tolist() == [h * w, w, 3, h * w]

    def poison(part):
        part[2, 5, 7] = np.nan

    cand = _dev(g0[0])
    p1 = partials(cand, poison)
    g1 = compare(call(p1, 1, 0, cand), p1, 1, False, g0[0], g0[1])
    assert g1[1][0] == 2 and g1[1][5] == 1 and np.array_equal(_bits(g1[0][5]), _bits(g0[0][5]))      # dead: the last solved theta
    assert g1[1][2] == 0 and np.array_equal(_bits(g1[0][2]), _bits(g0[0][2]))                        # n = 3 stays theta0
    cand = _dev(g1[0])
    p2 = partials(cand, lambda part: None)
    g2 = compare(call(p2, 2, 1, cand), p2, 2, True, g1[0], g1[1])
    assert np.array_equal(_bits(g2[0]), _bits(g1[0])) and np.array_equal(g2[1], g1[1])               # last: nothing solved
    assert g2[2][0, 1] == g2[2][0, 0] and g2[2][0, 2] < 1e-3                                         # exact uv: all inliers
    print(f"RATIO step: 0 (status, theta_next bits and stats equal on 4 calls x {B} frames; {ties} solutions flagged near an "
          f"fp32 rounding boundary)")
    assert ties == 0


# ------------------------------------------------------------------------------------------------ 3. the whole fit
def _fitter(**kw):
    from sfh_amd.uvfit import UVFit
    return UVFit((K.WT, K.HT), (K.W, K.H), **kw)


_LABELS = {}


def _device_label(name):
    """the label of LabelMaker.render on the device, through split_uv: uv (2,H,W) float32"""
    if name not in _LABELS:
        from sfh_amd import preparation, synth
        i, j = np.mgrid[0:K.HT, 0:K.WT]
        ids = ((i // 30 + j // 40) % 4).astype(np.uint8)
        poi = synth.load_court_poi("pitch", 1)[0, :, :2]
        maker = preparation.LabelMaker(ids, poi, (K.W, K.H), 4, uv=True)
        out = maker.render(_dev(K.TRUE[name].reshape(1, 3, 3)), uv=True)
        _LABELS[name] = preparation.split_uv(out["uv"])[1][0].cpu().numpy()
    return _LABELS[name]


@pytest.mark.parametrize("case", K.whole_cases(), ids=[c[0] for c in K.whole_cases()])
def test_whole_fit(case):
    """device against restatement on the same inputs: status and the integer statistics equal; the device's corner error at most
    1.25 x the restatement's plus the court-pixel size of 64 fp32 ulps of theta (uvfit_ref.theta_margin_px) - the margin for the
    one-ulp differences in theta_k that the summation order may cause between passes.  The restatement's own figure is the
    measurement; no absolute threshold."""
    uv, t0, true = K.whole_inputs(case)
    if case[2] == "label":
        uv = _device_label(case[1])
        if case[3]:
            uv = K.contaminate(uv, case[3], 5)
        uv = uv[None]
    ref = R.fit(uv, None, t0, K.H, K.W, K.WT, K.HT)
    assert R.near_delta(uv, None, ref["theta"], K.H, K.W, K.WT, K.HT) == 0       # the tie condition, on the device's label too
    fit = _fitter()
    theta, stats, status = fit(_dev(uv), None, None if t0 is None else _dev(t0).view(1, 1, 3, 3))
    again = fit(_dev(uv), None, None if t0 is None else _dev(t0).view(1, 1, 3, 3))
    torch.cuda.synchronize()
    assert torch.equal(theta, again[0]) and torch.equal(stats, again[1]) and torch.equal(status, again[2])
    assert theta.shape == (1, 1, 3, 3) and stats.shape == (1, 4) and status.shape == (1,)
    th, sg, sr = theta.cpu().numpy().reshape(1, 9), stats.cpu().numpy(), ref["stats"]
    assert status.cpu().numpy().tolist() == ref["status"].tolist() == [5]
    assert sg[0, 0] == sr[0, 0] and sg[0, 1] == sr[0, 1]
    e_gpu = float(R.corner_error(th, true, K.WT, K.HT)[0])
    e_ref = float(R.corner_error(ref["theta"], true, K.WT, K.HT)[0])
    margin = R.theta_margin_px(true, K.WT, K.HT)
    K.record(PARITY, [{"test": "whole_fit", "case": case[0], "gpu_err_px": e_gpu, "ref_err_px": e_ref, "margin_px": margin,
                       "n": sg[0, 0], "inliers": sg[0, 1], "rms_px_gpu": sg[0, 2], "rms_px_ref": sr[0, 2],
                       "theta_equal_bits": bool(np.array_equal(_bits(th), _bits(ref["theta"])))}])
    print(f"RATIO whole_fit {case[0]}: {e_gpu / (1.25 * e_ref + margin):.3g}")
    assert e_gpu <= 1.25 * e_ref + margin, (e_gpu, e_ref, margin)
    # the robust rms moves by no more than the residuals do (r / sqrt(1 + r^2 / d^2) has slope <= 1): the same margin
    assert abs(sg[0, 2] - sr[0, 2]) <= margin


def test_dead_frame_beside_live_ones():
    uv = np.stack([K.exact_uv(K.ZOOM, K.H, K.W), np.zeros((2, K.H, K.W), dtype=F32), K.label_uv(K.PERSPECTIVE, K.H, K.W)])
    t0 = np.stack([K.shifted(K.ZOOM), K.IDENTITY, K.shifted(K.PERSPECTIVE)])
    ref = R.fit(uv, None, t0, K.H, K.W, K.WT, K.HT)
    theta, stats, status = _fitter()(_dev(uv), None, _dev(t0).view(3, 1, 3, 3))
    assert status.tolist() == ref["status"].tolist() == [5, 0, 5]
    th = theta.cpu().numpy().reshape(3, 9)
    assert np.array_equal(_bits(th[1]), _bits(K.IDENTITY)) and stats[1, 0].item() == 0 and np.isnan(stats[1, 2].item())
    cold = _fitter()(_dev(uv))
    assert cold[2].tolist() == [5, 0, 5] and torch.isnan(cold[0][1]).all() and torch.isfinite(cold[0][[0, 2]]).all()
    e = R.corner_error(th[[0, 2]], np.stack([K.ZOOM, K.PERSPECTIVE]), K.WT, K.HT)
    e_ref = R.corner_error(ref["theta"][[0, 2]], np.stack([K.ZOOM, K.PERSPECTIVE]), K.WT, K.HT)
    for k, true in enumerate((K.ZOOM, K.PERSPECTIVE)):
        assert e[k] <= 1.25 * e_ref[k] + R.theta_margin_px(true, K.WT, K.HT)


def test_zero_iterations_empty_batch_and_gate():
    uv = K.label_uv(K.ZOOM, K.H, K.W)[None]
    lg = K.logits(4, uv[0], 3)[None]
    for logits in (None, lg):
        ref = R.fit(uv, logits, None, K.H, K.W, K.WT, K.HT, iters=0)
        theta, stats, status = _fitter(iters=0, mask_classes=4)(_dev(uv), _dev(logits))
        assert status.tolist() == [1] and stats[0, 0].item() == ref["stats"][0, 0] and stats[0, 1].item() == ref["stats"][0, 1]
        assert np.array_equal(_bits(theta.cpu().numpy().reshape(1, 9)), _bits(ref["theta"]))      # one solve on equal-weight sums
    assert ref["stats"][0, 0] < 0.9 * K.H * K.W                                                    # the class gate removed pixels
    e = _fitter(mask_classes=4)(torch.empty((0, 2, K.H, K.W), device="cuda"), torch.empty((0, 4, K.H, K.W), device="cuda"))
    assert e[0].shape == (0, 1, 3, 3) and e[1].shape == (0, 4) and e[2].shape == (0,)
    assert (e[0].dtype, e[1].dtype, e[2].dtype) == (torch.float32, torch.float64, torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        _fitter()(torch.from_numpy(uv))


def test_caches_and_streams():
    uv, t0 = _dev(K.label_uv(K.PERSPECTIVE, K.H, K.W)[None]), _dev(K.shifted(K.PERSPECTIVE)).view(1, 1, 3, 3)
    f = _fitter()
    want = f(uv, None, t0)
    work = dict(f._work)
    torch.cuda.synchronize()
    before = torch.cuda.memory_reserved()
    again = f(uv, None, t0)
    assert f._work == work and len(work) == 1 and torch.cuda.memory_reserved() == before
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = f(uv, None, t0)
    torch.cuda.synchronize()
    assert len(f._work) == 2 and all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(want, again, other))
    clone = pickle.loads(pickle.dumps(f))
    assert clone._work == {} and all(torch.equal(a, b) for a, b in zip(want, clone(uv, None, t0)))


# ------------------------------------------------------------------------------------------------ 4. the hooks
HW = (64, 96)


def _model(**kw):
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    H, W = HW
    B = 2
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :H, :W].contiguous().cuda()
    poi = synth.load_court_poi("pitch", B).cuda()
    net = Reconstructor(court, poi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H), warp_with_nearest=True, **kw)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 57))
    return net.cuda().eval(), synth.smooth_frames(B, H, W, seed=57).cuda()


def _hook_fitter(net):
    from sfh_amd.uvfit import UVFit
    return UVFit((K.WT, K.HT), net.warp_size, mask_classes=4)


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


PLAIN_KEYS = {"logits", "theta", "warp_mask", "consist_score", "poi"}


def test_hook_off_changes_nothing():
    """uv_fitter = None against a model on which the attribute does not exist"""
    a, x = _model(unet_uv=True)
    b, _ = _model(unet_uv=True)
    del b.__dict__["_uv_fitter"]
    with torch.no_grad():
        oa, ob = a.predict(x, consistency=True, project_poi=True), b.predict(x, consistency=True, project_poi=True)
        pa = a.predict_async(x, consistency=True, project_poi=True).result()
    assert set(oa) == PLAIN_KEYS and _same(oa, ob) and _same(oa, pa)


def test_hook_on():
    plain, x = _model(unet_uv=True)
    net, _ = _model(unet_uv=True)
    net.uv_fitter = _hook_fitter(net)
    with torch.no_grad():
        want = plain.predict(x, consistency=True, project_poi=True)
        out = net.predict(x, consistency=True, project_poi=True)
        assert set(out) == PLAIN_KEYS | {"theta_uv", "uv_fit"}
        assert _same(want, {k: out[k] for k in want})                         # the other outputs are untouched
        # By hand on eval-mode forward()'s uv.  ONE launch legitimately differs between the two paths: forward() of a unet_uv
        # model takes its logits from sfh_outconv_fwd, predict() - with or without a fitter - from the fused head epilogue of
        # the last conv, which adds the 64 products in another order; the logits (and the theta behind them) agree to rounding,
        # not to the bit, so the gate and the start are predict()'s own.  uv is sfh_outconv_fwd over the same stored y in both.
        fw = net(x)
        assert (fw["logits"] - out["logits"]).abs().max().item() <= 1e-4 * max(1.0, out["logits"].abs().max().item())
        hand = _hook_fitter(net)(fw["uv"], out["logits"], out["theta"])
        assert torch.equal(out["theta_uv"].view(torch.int32), hand[0].view(torch.int32))
        assert torch.equal(out["uv_fit"].view(torch.int64), hand[1].view(torch.int64))
        assert out["theta_uv"].shape == (2, 1, 3, 3) and out["uv_fit"].shape == (2, 4) and out["uv_fit"].dtype == torch.float64
        assert _same(net.predict_async(x, consistency=True, project_poi=True).result(), out)      # runs synchronously: same dict
        net.graph_replay = True                                                # replay falls through to predict()
        for _ in range(2):
            assert _same(net.predict(x, consistency=True, project_poi=True), out)
        assert not net.__dict__.get("_replay")
        net.graph_replay = False
        empty = net.predict(x[:0], consistency=True, project_poi=True)
        assert set(empty) == set(out) and all(empty[k].shape[1:] == out[k].shape[1:] and empty[k].dtype == out[k].dtype for k in out)
        clone = pickle.loads(pickle.dumps(net))
        assert clone.uv_fitter._work == {} and _same(clone.cuda().eval().predict(x, consistency=True, project_poi=True), out)
    no_uv, _ = _model()
    with pytest.raises(ValueError, match="UV head"):
        no_uv.uv_fitter = net.uv_fitter


@pytest.mark.parametrize("variant", ["bf16x6", "fp32", "bilinear"])
def test_hook_on_other_head_configurations(variant):
    """A fitter on an img+mask model keeps the fused head and lets the last conv also store its output (sfh_conv_desc.
    head_skip_dst = 0).  The same two properties as test_hook_on - every other output bit-equal to the plain model's, uv the
    one forward() computes - in the other operand formats (three-plane bf16, fp32 MFMA) and on the bilinear Up variant, whose
    last block runs the plain two-source DoubleConv launch instead of the fused Up kernel."""
    kw = dict(unet_uv=True, unet_bilinear=True) if variant == "bilinear" else dict(unet_uv=True)
    plain, x = _model(**kw)
    net, _ = _model(**kw)
    if variant != "bilinear":
        plain.precision = net.precision = variant
    net.uv_fitter = _hook_fitter(net)
    with torch.no_grad():
        want = plain.predict(x, consistency=True, project_poi=True)
        out = net.predict(x, consistency=True, project_poi=True)
        assert set(out) == PLAIN_KEYS | {"theta_uv", "uv_fit"} and _same(want, {k: out[k] for k in want})
        hand = _hook_fitter(net)(net(x)["uv"], out["logits"], out["theta"])
        assert torch.equal(out["theta_uv"].view(torch.int32), hand[0].view(torch.int32))
        assert torch.equal(out["uv_fit"].view(torch.int64), hand[1].view(torch.int64))


def test_uv_input_model():
    """unet_uv=True, resnet_input='img+mask+uv': predict() runs, with the reference's keys (no 'uv'); theta is eval-mode
    forward()'s bit for bit (the same launches: unfused head, sfh_stn_input_assemble, the same ResNet engine); warp_mask and
    consist_score follow from theta by the existing rule; predict_async and replay run predict() (they say so), and
    FramePipeline, which goes through predict_async, returns predict()'s theta"""
    from sfh_amd import engine as E
    from sfh_amd import synth
    from sfh_amd.pipeline import FramePipeline
    net, x = _model(unet_uv=True, resnet_input="img+mask+uv")
    H, W = HW
    with torch.no_grad():
        out = net.predict(x, consistency=True, project_poi=True)
        fw = net(x)
        assert set(out) == PLAIN_KEYS and set(fw) == {"logits", "uv", "theta", "poi", "warp_mask"}
        assert torch.equal(out["theta"].view(torch.int32), fw["theta"].view(torch.int32)) and torch.isfinite(out["theta"]).all()
        assert torch.equal(out["logits"], fw["logits"]) and torch.equal(out["poi"], fw["poi"])
        wm, score = E.warp_consistency(out["theta"], net.court_img.contiguous(), out["logits"], 4.0, shared_template=True,
                                       warp_hw=(H, W))
        assert torch.equal(out["warp_mask"], wm) and torch.equal(out["consist_score"], score)
        assert _same(net.predict_async(x, consistency=True, project_poi=True).result(), out)
        net.graph_replay = True
        for _ in range(2):
            assert _same(net.predict(x, consistency=True, project_poi=True), out)
        assert _same(net.predict_replay(x, consistency=True, project_poi=True), out) and not net.__dict__.get("_replay")
        net.graph_replay = False
        empty = net.predict(x[:0], consistency=True, project_poi=True)
        assert set(empty) == set(out)
        frames = [torch.from_numpy(synth.synth_frames_u8(2, H, W, seed=70 + k)).pin_memory() for k in range(3)]
        got = list(FramePipeline(net, 2, (H, W), req_outputs=("theta", "warp_mask")).run(iter(frames)))
        for fr, res in zip(frames, got):
            ref = net.predict(E.frames_u8_to_input(fr.cuda()), consistency=True)
            assert np.array_equal(res["theta"], ref["theta"].cpu().numpy())
        net.uv_fitter = _hook_fitter(net)                                      # the fitter on the model family that feeds on uv
        both = net.predict(x, consistency=True, project_poi=True)
        assert set(both) == PLAIN_KEYS | {"theta_uv", "uv_fit"} and _same(out, {k: both[k] for k in out})


def test_evaluate_registration_scores_theta_uv():
    from sfh_amd import metrics as M
    from sfh_amd import synth
    H, W = HW
    net, _ = _model(unet_uv=True)
    g = np.random.default_rng(11)
    loader = []
    for i, B in enumerate((2, 1)):
        th = np.eye(3, dtype=F32)[None].repeat(B, 0) + g.normal(0, 0.05, (B, 3, 3)).astype(F32)
        th[:, 2, 2] = 1
        loader.append({"image": synth.smooth_frames(B, H, W, seed=90 + i), "mask": torch.from_numpy(g.integers(0, 4, (B, H, W))),
                       "theta": torch.from_numpy(th), "name": [f"b{i}-{k}" for k in range(B)]})
    plain = M.evaluate_registration(net, loader, "cuda", lattice=(7, 5))
    assert "theta_uv" not in plain and "frames_uv" not in plain
    net.uv_fitter = _hook_fitter(net)
    res = M.evaluate_registration(net, loader, "cuda", lattice=(7, 5))
    assert net.training and res["theta_uv"]["frames"] == res["theta"]["frames"] == 3 and "theta_stn" not in res
    direct = M.RegistrationMetrics(4, (W, H), (W, H), net.court_poi[0, :, :2], lattice=(7, 5))
    net.eval()
    with torch.no_grad():
        for b in loader:
            p = net.predict(b["image"].cuda(), consistency=False)
            direct.add(p["theta_uv"], b["theta"].cuda(), b["mask"].cuda(), logits=p["logits"], names=b["name"])
    want = direct.table()
    assert set(want) == set(res["frames_uv"])
    for col in want:
        a, b = res["frames_uv"][col], want[col]
        assert a.tolist() == b.tolist() if a.dtype == object else np.array_equal(a, b, equal_nan=True), col
    for col in plain["frames"]:                                               # nothing changes for theta itself
        a, b = res["frames"][col], plain["frames"][col]
        assert a.tolist() == b.tolist() if a.dtype == object else np.array_equal(a, b, equal_nan=True), col
