"""CPU checks of the inter-frame tracking (no device): the numpy restatement tests/track_ref.py against hand cases, the
condition that keeps the GPU comparison honest (the restatement alone converges on every whole-alignment case), the
propagation rule on dyadic translations, the host arithmetic of csrc/det_core.h and csrc/track_core.h in a stand-alone
sanitizer build, and every refusal of sfh_amd.track and of the sfh_track_* entries."""
import ctypes
import pickle
import subprocess

import numpy as np
import pytest
import torch

import host_program
import track_cases as K
import track_ref as T

F32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_planes_by_hand():
    fr = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    fr[0, :2, :2] = (255, 0, 0)
    fr[0, :2, 2:] = (0, 255, 0)
    fr[0, 2:, :2] = (0, 0, 255)
    fr[0, 2:, 2:] = (255, 255, 255)
    # (19595 * 255 + 32768) >> 16 = 76, 38470 -> 150, 7471 -> 29, white -> 255
    assert T.luma(fr)[0, ::2, ::2].tolist() == [[76, 150], [29, 255]] and T.luma(fr, bgr=True)[0, ::2, ::2].tolist() == [[29, 150], [76, 255]]
    p2 = T.planes(fr, 2)
    assert p2.dtype == F32 and np.array_equal(p2[0], (np.array([[76, 150], [29, 255]], dtype=F32) * 4 / F32(1020)).astype(F32))
    assert T.planes(fr, 4)[0, 0, 0] == F32(F32(4 * (76 + 150 + 29 + 255)) / F32(255 * 16))
    assert T.planes(np.full((1, 8, 8, 3), 255, np.uint8), 4).tolist() == [[[1.0, 1.0], [1.0, 1.0]]]


def test_identity_counts_the_interior_and_costs_nothing():
    """33 x 65 at level 1: 2 / (n - 1) is dyadic, so xn, u + 1 and px = J are exact - the counted pixels are those whose four
    taps exist, (hl - 1) (wl - 1), every weight is 1 or 0 and every residual is exactly 0"""
    h, w = 33, 65
    p = T.planes(K.plane_frames(h, w)[:1], 1)[0]
    q = T.pixel_terms(K.IDENTITY, p, p, h, w, 1, 0.06)
    assert np.array_equal(q["px"], np.broadcast_to(np.arange(w, dtype=F32), (h, w)))
    assert np.array_equal(q["py"], np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w)))
    S, A = T.sums(K.IDENTITY, p, p, h, w, 1, 0.06)
    assert S[T.N] == (h - 1) * (w - 1) and q["counts"][:-1, :-1].all() and not q["counts"][-1].any() and not q["counts"][:, -1].any()
    assert S[T.COST] == 0.0 and not S[36:44].any() and S[:36].any()
    # at the levels of the schedule px = J holds up to rounding: within 2^-16 of a plane pixel at 144 x 256
    for f in K.FACTORS:
        pf = T.planes(K.frame()[None], f)[0]
        q = T.pixel_terms(K.IDENTITY, pf, pf, K.H, K.W, f, 0.06)
        assert np.abs(q["px"] - np.arange(K.W // f, dtype=F32)).max() <= 2.0 ** -16
        assert np.abs(q["py"] - np.arange(K.H // f, dtype=F32)[:, None]).max() <= 2.0 ** -16


def test_whole_pixel_translation_has_zero_residual_on_the_overlap():
    """33 x 65, level 1, the current plane = the previous one moved by (+3, -2) pixels: M = the dyadic pan (6 / 64, -4 / 32) puts
    px = J + 3, py = I - 2 exactly, the residual is exactly 0 and n = (wl - 1 - 3) (hl - 1 - 2) ... by hand: columns 0 .. wl-5,
    rows 2 .. hl-1"""
    h, w = 33, 65
    prev = T.planes(K.plane_frames(h, w)[:1], 1)[0]
    cur = np.zeros_like(prev)
    cur[2:, :w - 3] = prev[:h - 2, 3:]
    M = K.pan(3.0, -2.0, w, h)
    assert float(M[2]) == 6.0 / 64 and float(M[5]) == -4.0 / 32
    q = T.pixel_terms(M, prev, cur, h, w, 1, 0.06)
    assert np.array_equal(q["px"][0], np.arange(w, dtype=F32) + 3) and np.array_equal(q["py"][:, 0], np.arange(h, dtype=F32) - 2)
    want = np.zeros((h, w), dtype=bool)
    want[2:, :w - 4] = True                      # x0 + 1 = J + 4 <= wl - 1; y0 = I - 2 >= 0 (and I - 1 <= hl - 1 always)
    assert np.array_equal(q["counts"], want)
    S, _ = T.sums(M, prev, cur, h, w, 1, 0.06)
    assert S[T.N] == (h - 2) * (w - 4) and S[T.COST] == 0.0 and not S[36:44].any()
    assert not q["r"][want].any()


def test_horizon_nan_and_outside_count_nothing():
    h, w = 18, 32
    fr = K.plane_frames(h, w)
    p0, p1 = T.planes(fr[:1], 1)[0], T.planes(fr[1:2], 1)[0]
    _, yn = T.grid(1, h, w)
    Ms = K.kernel_Ms(yn, h // 2 + 1)
    q = T.pixel_terms(Ms[4], p0, p1, h, w, 1, 0.06)
    assert not q["counts"][h // 2 + 1].any() and q["counts"].any()
    for k in (5, 6):
        S, A = T.sums(Ms[k], p0, p1, h, w, 1, 0.06)
        assert not S.any() and not A.any() and not np.signbit(S).any()


def test_weight_is_geman_mcclure():
    h, w = 18, 32
    fr = K.plane_frames(h, w)
    p0, p1 = T.planes(fr[:1], 1)[0], T.planes(fr[1:2], 1)[0]
    q = T.pixel_terms(K.IDENTITY, p0, p1, h, w, 1, 0.06)
    k = q["counts"]
    r, c = q["r"][k], 1.0 + q["r"][k] ** 2 / 0.06 ** 2
    assert np.allclose(q["rho"][k], r * r / c, rtol=1e-14) and np.allclose(q["omega"][k], 1 / c ** 2, rtol=1e-14)
    assert (q["rho"][k] < 0.06 ** 2).all()          # the cost of a pixel saturates at delta^2


# ------------------------------------------------------------------------------------------------ the honest-comparison condition
@pytest.mark.parametrize("case", K.ALIGN_IDS)
def test_restatement_converges(case):
    """the restatement alone ends below 0.1 px on every whole-alignment case: what the device is compared against is a
    converged alignment, not a shared failure"""
    r = K.align_ref(case)
    print(f"RECOVERY {case}: start {r['start']:.2f} px -> {r['err']:.4f} px, accepted {r['accepted'].tolist()}, "
          f"mean cost {r['stats'][-1, 0]:.3g} -> {r['stats'][-1, 1]:.3g}, n {r['stats'][:, 2].tolist()}")
    assert r["ok"] == 1 and r["err"] < 0.1
    assert (r["stats"][:, 1] <= r["stats"][:, 0]).all() or case.startswith("identity")
    assert (r["stats"][:, 2] >= [T.nmin_of(K.MIN_OVERLAP, K.H // f, K.W // f) for f in K.FACTORS]).all()


def test_dead_pair_and_max_cost():
    prev, cur, _ = K.align_pair("pan3-clean")
    far = np.array([1, 0, 50.0, 0, 1, 50.0, 0, 0, 1], dtype=F32)
    out = T.align(prev, cur, M0=far)
    assert out["ok"] == 0 and np.array_equal(out["M"], far) and not out["accepted"].any() and not out["stats"][:, 2].any()
    assert np.isnan(out["stats"][:, :2]).all()
    # a cut: unrelated frames align to something, at a mean cost that max_cost tells from a pan's
    cut = K.frame(K.pan(90.0, 40.0))[::-1, ::-1].copy()
    good, bad = K.align_ref("pan3-clean"), T.align(prev, cut, max_cost=1e-4)
    assert good["stats"][-1, 1] < 1e-5 < 1e-4 < bad["stats"][-1, 1] and bad["ok"] == 0
    assert T.align(prev, cur, max_cost=1e-4)["ok"] == 1
    out0 = T.align(prev, cur, iters=0)
    assert np.array_equal(out0["M"], K.IDENTITY) and not out0["accepted"].any() and out0["ok"] == 1


# ------------------------------------------------------------------------------------------------ propagation
def test_propagate_rule():
    theta, M = K.dyadic_clip(8)
    link = np.ones(8, dtype=np.int32)
    score = np.zeros(8, dtype=F32)
    bad = theta.copy()
    bad[3] = 0.0                                        # singular
    score[4] = np.nan                                   # NaN score
    bad[4] = theta[4] + F32(0.3)                        # garbage, but usable: only the score says so
    out, src = T.propagate(bad, M, link, score, 0.1)
    assert src.tolist() == [0, 1, 2, 2, 5, 5, 6, 7]
    # dyadic: the carried theta is the true one, bit for bit, back (3 from 2) and forward (4 from 5)
    assert np.array_equal(_bits(out), _bits(theta))
    # a tie goes back: frame 3 of bad 3 alone sits between 2 and 4
    b2 = theta.copy()
    b2[3] = np.nan
    out, src = T.propagate(b2, M, link)
    assert src[3] == 2 and np.array_equal(_bits(out), _bits(theta))
    # a broken link stops the walk: link[3] = 0 cuts (2, 3), so 3 comes from 4
    l2 = link.copy()
    l2[3] = 0
    out, src = T.propagate(b2, M, l2)
    assert src[3] == 4 and np.array_equal(_bits(out), _bits(theta))
    l2[4] = 0
    out, src = T.propagate(b2, M, l2)
    assert src[3] == -1 and np.isnan(out[3]).all() and np.array_equal(_bits(out[[0, 1, 2, 4, 5, 6, 7]]), _bits(theta[[0, 1, 2, 4, 5, 6, 7]]))
    # max_gap: frames 2..5 bad, gap 1 reaches 2 and 5 only
    b3 = theta.copy()
    b3[2:6] = np.inf
    out, src = T.propagate(b3, M, link, max_gap=1)
    assert src.tolist() == [0, 1, 1, -1, -1, 6, 6, 7] and np.array_equal(_bits(out[[2, 5]]), _bits(theta[[2, 5]]))
    out, src = T.propagate(b3, M, link, max_gap=2)
    assert src.tolist() == [0, 1, 1, 1, 6, 6, 6, 7] and np.array_equal(_bits(out), _bits(theta))
    out, src = T.propagate(b3, M, link, max_gap=0)
    assert src.tolist() == [0, 1, -1, -1, -1, -1, 6, 7]
    # no good frame at all
    out, src = T.propagate(np.zeros_like(theta), M, link)
    assert (src == -1).all() and np.isnan(out).all()
    # entry 0 of M and link is never read
    M[0], link[0] = np.nan, 0
    assert np.array_equal(_bits(T.propagate(b2, M, link)[0]), _bits(theta))


# ------------------------------------------------------------------------------------------------ the host arithmetic, sanitized
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program.build_host_program(tmp_path_factory, "track")


def test_host_program_plan_and_axis(host_exe):
    plans = [(1, 2, 2), (3, 18, 32), (3, 65, 67), (16, 180, 320), (1, 72, 136), (0, 8, 8), (65536, 8, 8), (1, 1, 8), (1, 8, 1),
             (65535, 64, 64), (2, 64 * 65535, 2), (2, 64 * 65535 + 1, 2)]
    axes = [(f, n) for f in (1, 2, 4, 8, 16, 3, 17, 0) for n in (8, 16, 144, 256, 360, 640, 33, 2)]
    text = "".join(f"plan {p} {h} {w}\n" for p, h, w in plans) + "".join(f"axis {f} {n}\n" for f, n in axes)
    r = subprocess.run([host_exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for (p, h, w), line in zip(plans, lines):
        ok = 1 <= p <= 65535 and h >= 2 and w >= 2 and -(-h // 64) <= 65535
        want = (1, T.slabs(h, w), T.SUMS * p, 8, T.slabs(h, w) * T.SUMS * p * 8) if ok else (0, 0, 0, 0, -1)
        assert tuple(int(v) for v in line.split()) == want, (p, h, w, line)
    for (f, n), line in zip(axes, lines[len(plans):]):
        ok = 1 <= f <= 16 and n % f == 0 and n >= f
        k, o = T.track_axis(f, n) if ok else (F32(0), F32(0))
        assert line.split() == [str(int(ok)), f"{int(_bits(np.array([k]))[0]):08x}", f"{int(_bits(np.array([o]))[0]):08x}"], (f, n, line)


# ------------------------------------------------------------------------------------------------ the C interface, no device
_HOST = (ctypes.c_double * 4096)()


def test_refusals_without_a_device():
    """every refusal returns -1 before anything could be launched (the pointers are host memory)"""
    from sfh_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(ctypes.addressof(_HOST))
    assert _lib.ABI.defines["SFH_TRACK_SUMS"] == T.SUMS == 46
    assert lib.sfh_track_workspace_bytes(3, 72, 136) == 2 * 3 * 3 * 46 * 8 == T.slabs(72, 136) * 3 * 46 * 8
    assert lib.sfh_track_workspace_bytes(16, 180, 320) == 15 * 16 * 46 * 8
    for bad in ((0, 8, 8), (65536, 8, 8), (1, 1, 8), (1, 8, 1)):
        assert lib.sfh_track_workspace_bytes(*bad) == -1
    a = (ctypes.c_float * 2)()
    for f, n in ((8, 256), (2, 144), (1, 33)):
        assert lib.sfh_track_axis(f, n, a) == 0 and (F32(a[0]), F32(a[1])) == T.track_axis(f, n)
    assert lib.sfh_track_axis(1, 8, None) == -1 and b"null" in lib.sfh_last_error()
    for f, n in ((0, 8), (17, 34), (3, 8), (8, 4)):
        assert lib.sfh_track_axis(f, n, a) == -1 and b"level" in lib.sfh_last_error()
    assert lib.sfh_track_planes(None, 1, 8, 8, 1, 0, p, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_track_planes(p, 0, 8, 8, 1, 0, p, None) == -1
    for f, H, W in ((3, 8, 8), (2, 9, 8), (2, 8, 9), (17, 34, 34)):
        assert lib.sfh_track_planes(p, 1, H, W, f, 0, p, None) == -1 and b"divide" in lib.sfh_last_error()
        assert lib.sfh_track_accumulate(p, p, 2, p, p, 1, H, W, f, 0.06, p, 1 << 30, None) == -1 and b"divide" in lib.sfh_last_error()
    assert lib.sfh_track_accumulate(None, p, 2, p, p, 1, 8, 8, 1, 0.06, p, 1 << 30, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_track_accumulate(p, p, 2, None, p, 1, 8, 8, 1, 0.06, p, 1 << 30, None) == -1 and b"null" in lib.sfh_last_error()
    assert lib.sfh_track_accumulate(p, p, 0, p, p, 1, 8, 8, 1, 0.06, p, 1 << 30, None) == -1
    for d in (0.0, -1.0, float("nan"), float("inf"), 1e-200):
        assert lib.sfh_track_accumulate(p, p, 2, p, p, 1, 8, 8, 1, d, p, 1 << 30, None) == -1 and b"delta" in lib.sfh_last_error()
    assert lib.sfh_track_accumulate(p, p, 2, p, p, 1, 8, 16, 8, 0.06, p, 1 << 30, None) == -1 and b"planes 2x1" in lib.sfh_last_error()
    for pairs in (0, 65536):
        assert lib.sfh_track_accumulate(p, p, 2, p, p, pairs, 8, 8, 1, 0.06, p, 1 << 30, None) == -1 and b"pairs" in lib.sfh_last_error()
    need = lib.sfh_track_workspace_bytes(3, 36, 64)
    for ws, nbytes in ((None, need), (p, need - 1)):
        assert lib.sfh_track_accumulate(p, p, 4, p, p, 3, 72, 128, 2, 0.06, ws, nbytes, None) == -1
        msg = lib.sfh_last_error().decode()
        assert "workspace" in msg and str(need) in msg, msg
    ok = (p, 1, 1, 1, 0, p, p, p, p, p, p, p, p, p, p, 0, 1, 4.0, 0.0, None)
    for k in (0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14):
        args = list(ok)
        args[k] = None
        assert lib.sfh_track_step(*args) == -1 and b"null" in lib.sfh_last_error()
    for k, v in ((1, 0), (2, 0), (2, 65536), (15, 1), (15, -1), (16, 0), (17, -1.0), (17, float("nan")), (18, float("nan"))):
        args = list(ok)
        args[k] = v
        assert lib.sfh_track_step(*args) == -1, (k, v)
    assert lib.sfh_track_propagate(None, None, 0.0, p, p, 4, 30, p, p, None) == -1 and b"null" in lib.sfh_last_error()
    q = ctypes.c_void_p(p.value + 4096)
    assert lib.sfh_track_propagate(p, None, 0.0, p, p, 0, 30, q, p, None) == -1
    assert lib.sfh_track_propagate(p, None, 0.0, p, p, 4, -1, q, p, None) == -1 and b"max_gap" in lib.sfh_last_error()
    assert lib.sfh_track_propagate(p, None, 0.0, p, p, 4, 30, p, p, None) == -1 and b"overlaps" in lib.sfh_last_error()


def test_value_errors_on_the_host():
    from sfh_amd.track import FrameAligner, propagate_theta
    for bad in (dict(factors=(3,)), dict(factors=(0,)), dict(factors=(32,)), dict(factors=(16,), frame_size=(16, 32)), dict(iters=-1),
                dict(delta=0.0), dict(delta=-1.0), dict(delta=float("nan")), dict(min_overlap=0.0), dict(min_overlap=1.5),
                dict(max_cost=0.0), dict(frame_size=(1, 8))):
        with pytest.raises(ValueError):
            FrameAligner(**{**dict(frame_size=(K.W, K.H)), **bad})
    al = FrameAligner(frame_size=(K.W, K.H), max_cost=0.01, bgr=True)
    fr = torch.zeros((2, K.H, K.W, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        al(fr)
    with pytest.raises(ValueError, match="tensor"):
        al(fr.numpy())
    al2 = pickle.loads(pickle.dumps(al))
    assert (al2.frame_size, al2.factors, al2.iters, al2.delta, al2.min_overlap, al2.max_cost, al2.bgr) == (
        (K.W, K.H), (8, 4, 2), 6, 0.06, 0.25, 0.01, True) and al2._work == {}
    th = torch.eye(3).reshape(1, 1, 3, 3).repeat(4, 1, 1, 1)
    with pytest.raises(ValueError, match="CUDA"):
        propagate_theta(th, th[1:].clone(), torch.ones(3, dtype=torch.int32))
