"""CPU checks of the temporal smoothing of theta (no device): the numpy restatement tests/smooth_ref.py by its properties, the
conditions that keep the GPU comparison honest (the restatement alone improves the noisy clip), csrc/smooth_core.h in a
stand-alone sanitizer build held to the restatement bit for bit, and every refusal of sfh_amd.track.smooth_theta and of
sfh_track_smooth."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import host_program
import smooth_ref as S
import track_cases as K
from conftest import ROOT

F32 = np.float32
PARITY = os.path.join(ROOT, "profiles", "smooth_parity.jsonl")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _close(out, true):
    """S.exact_gap within its bound; -> the gap for the record"""
    gap = S.exact_gap(out, true)
    assert gap[0] <= S.EXACT_ULPS and gap[1] <= S.EXACT_ZERO, gap
    return gap


# ------------------------------------------------------------------------------------------------ the restatement's properties
def test_butterfly_is_the_xor_tree():
    rng = np.random.default_rng(1)
    v = rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64)
    # by hand: level by level, lane l takes lane l ^ o
    w = v.copy()
    for o in (32, 16, 8, 4, 2, 1):
        w = np.array([w[l] + w[l ^ o] for l in range(64)])
    assert _bits(np.array([S.butterfly(v)]))[0] == _bits(w[:1])[0] and len(set(_bits(w).tolist())) == 1
    assert S.butterfly(np.zeros(64)) == 0.0 and not np.signbit(S.butterfly(np.zeros(64)))
    one = np.zeros(64)
    one[37] = 0.1
    assert S.butterfly(one) == 0.1
    assert abs(S.butterfly(v) - float(np.sum(v.astype(np.longdouble)))) <= 64 * 2.0 ** -53 * np.abs(v).sum()


def test_exact_members_return_the_reference_member_exactly():
    """dyadic clip: every member sees the same points, d_k = 0, so c = c0 whatever the weights; the refit then lands within
    a few fp32 ulps of the true theta"""
    theta, M = K.dyadic_clip(8)
    link = np.ones(8, dtype=np.int32)
    for back, ahead in ((0, 0), (1, 0), (0, 1), (2, 2), (31, 31)):
        out, mem, stats = S.smooth(theta, M, link, back=back, ahead=ahead)
        assert mem.tolist() == [min(t, back) + 1 + min(7 - t, ahead) for t in range(8)]
        assert not stats[:, 1].any() and not stats[:, 2].any()
        for t in range(8):
            g = [S.triangle(back, t - k) for k in range(max(0, t - back), t + 1)] + [S.triangle(ahead, k - t) for k in range(t + 1, min(7, t + ahead) + 1)]
            assert abs(stats[t, 0] - sum(g)) <= 1e-12
        print(f"EXACT back {back} ahead {ahead}: {_close(out, theta)} (fp32 ulps, largest |entry| where the true one is 0)")


def test_members_by_hand():
    theta, M = K.dyadic_clip(8)
    link = np.ones(8, dtype=np.int32)
    bad = theta.copy()
    bad[3], bad[5] = 0.0, np.nan
    score = np.zeros(8, dtype=F32)
    score[6] = np.nan
    out, mem, stats = S.smooth(bad, M, link, score=score, max_score=0.1, back=2, ahead=2)
    # good: 0 1 2 4 7
    assert mem.tolist() == [3, 3, 4, 3, 2, 2, 2, 1]
    assert np.isnan(stats[[3, 5, 6], 2]).all() and not np.isnan(stats[[0, 1, 2, 4, 7], 2]).any()
    _close(out, theta)                                  # the bad frames are filled with the true theta
    cut = link.copy()
    cut[3] = 0                                                       # (2, 3) is cut
    out, mem, _ = S.smooth(bad, M, cut, score=score, max_score=0.1, back=2, ahead=2)
    assert mem.tolist() == [3, 3, 3, 1, 1, 2, 2, 1]
    cut[5] = 0
    out, mem, _ = S.smooth(bad, M, cut, score=score, max_score=0.1, back=2, ahead=2)
    assert mem.tolist() == [3, 3, 3, 1, 1, 1, 1, 1] and np.isnan(out).sum() == 0
    out, mem, stats = S.smooth(bad, M, cut, score=score, max_score=0.1, back=2, ahead=2, min_members=3)
    assert np.isnan(out[3:]).all() and np.isnan(stats[3:]).all() and not np.isnan(out[:3]).any() and mem.tolist() == [3, 3, 3, 1, 1, 1, 1, 1]
    out, mem, stats = S.smooth(np.zeros_like(theta), M, link)
    assert not mem.any() and np.isnan(out).all() and np.isnan(stats).all()


def test_tie_goes_back_and_mixed_sign_is_dropped():
    theta, M = K.dyadic_clip(8)
    link = np.ones(8, dtype=np.int32)
    th = theta.copy()
    th[3] = np.nan
    th[2], th[4] = theta[2] + F32(0.3), theta[4] - F32(0.17)         # two members at distance 1 that disagree widely
    th[[0, 1, 5, 6, 7]] = 0.0
    out, mem, stats = S.smooth(th, M, link, back=1, ahead=2, iters=0)       # weights 1/2 back and 2/3 forward, both at distance 1
    assert mem[3] == 2
    ok2, q2 = S.project(S.chain(th, M, 2, 3))
    ok4, q4 = S.project(S.chain(th, M, 4, 3))
    assert ok2 and ok4
    g2, g4 = S.triangle(1, 1), S.triangle(2, 1)
    c = q2 + (g4 * (q4 - q2)) / (g2 + g4)                            # c0 = q2, the back member: the same mean as from q4 up to
    c_fwd = q4 + (g2 * (q2 - q4)) / (g2 + g4)                        # rounding, and the rounding is what shows the tie
    assert not np.array_equal(c, c_fwd) and np.abs(c - c_fwd).max() < 1e-15
    assert np.array_equal(_bits(out[3]), _bits(np.array([F32(v) for v in S.refit(c)[0]] + [F32(1)], dtype=F32)))
    # a member whose W changes sign over the control points: the horizon row y = 0.6 crosses them
    hor = np.array([0.5, 0, 0.1, 0, 0.5, 0, 0, 1.0, -0.6], dtype=F32)
    assert S.good([hor], None, 0.0, 0) and not S.project([np.float64(v) for v in hor])[0]
    th2 = theta.copy()
    th2[4] = hor
    out, mem, _ = S.smooth(th2, M, link, back=1, ahead=1)
    assert mem.tolist() == [2, 3, 3, 2, 2, 2, 3, 2]
    _close(out, theta)


# ------------------------------------------------------------------------------------------------ the conditions on the inputs
def test_the_restatement_improves_the_noisy_clip():
    """what the device is compared against does what the feature is for: at radius 12 with three re-weightings the median error
    of the good frames falls below 0.6 of the inputs', the garbage frame ends below the inputs' median, and with iters = 0
    (the plain mean) it does not"""
    clip = S.noisy_clip()
    err = lambda th: np.array([S.corner_error(th[t], clip["true"][t]) for t in range(len(th))])
    e_in = err(clip["theta"])
    med_in = float(np.median(e_in[clip["good"]]))
    rows = []
    for radius, iters in ((12, 3), (12, 0), (6, 3), (31, 3)):
        out, mem, stats = S.smooth(clip["theta"], clip["M"], clip["link"], back=radius, ahead=radius, iters=iters)
        e = err(out)
        row = {"what": "restatement on the noisy clip", "radius": radius, "iters": iters, "median_in_px": round(med_in, 4),
               "median_out_px": round(float(np.median(e[clip["good"]])), 4), "garbage_in_px": round(float(e_in[clip["garbage"]]), 2),
               "garbage_out_px": round(float(e[clip["garbage"]]), 4),
               "gap_out_px": [round(float(v), 4) for v in e[clip["gap"][0]:clip["gap"][1]]],
               "garbage_deviation": round(float(stats[clip["garbage"], 2]), 4),
               "median_deviation": round(float(np.nanmedian(stats[clip["good"], 2])), 4)}
        rows.append(row)
        print("SMOOTH", json.dumps(row))
    r3, r0 = rows[0], rows[1]
    assert r3["median_out_px"] < 0.6 * med_in
    assert r3["garbage_out_px"] < med_in
    assert not r0["garbage_out_px"] < med_in
    assert np.isfinite(r3["gap_out_px"]).all()
    try:
        kept = [json.loads(ln) for ln in open(PARITY)] if os.path.exists(PARITY) else []
        with open(PARITY, "w") as f:
            for r in rows + [r for r in kept if r.get("what") != rows[0]["what"]]:
                f.write(json.dumps(r) + "\n")
    except OSError:          # a read-only checkout: the figures are still printed
        pass


# ------------------------------------------------------------------------------------------------ smooth_core.h, sanitized
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program.build_host_program(tmp_path_factory, "smooth")


def _w(v):
    return f"{int(_bits(np.array([v], dtype=F32))[0]):08x}"


def _d(v):
    return f"{int(_bits(np.array([v], dtype=np.float64))[0]):016x}"


def _clip_text(theta, M, link, score, max_score, ctrl):
    use = score is not None
    sc = score if use else np.zeros(len(theta), dtype=F32)
    head = f"clip {len(theta)} {int(use)} {_w(max_score)} " + " ".join(_w(v) for v in np.asarray(ctrl, dtype=F32).reshape(8)) + "\n"
    return head + "".join(" ".join(_w(v) for v in theta[t]) + " " + " ".join(_w(v) for v in M[t]) + f" {int(link[t])} {_w(sc[t])}\n"
                          for t in range(len(theta)))


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [ln.split() for ln in r.stdout.strip().split("\n")]


def test_host_program_members_and_chains(host_exe):
    """every (k, t) of three clips: linked, member, the nine entries of the chain and the eight projected values"""
    theta, M = K.dyadic_clip(8)
    bad = theta.copy()
    bad[3], bad[5] = 0.0, np.inf
    bad[6] = [0.5, 0, 0.1, 0, 0.5, 0, 0, 1.0, -0.6]                  # mixed-sign W over the control points
    score = np.zeros(8, dtype=F32)
    score[1] = np.nan
    cut = np.ones(8, dtype=np.int32)
    cut[2] = 0
    noisy = S.noisy_clip(F=20, garbage=5, gap=(9, 11), cut=14)
    n = 0
    for th, m, link, sc, ms, ctrl in ((bad, M, cut, score, 0.1, S.CTRL), (theta, M, np.ones(8, np.int32), None, 0.0, S.CTRL),
                                      (noisy["theta"], noisy["M"], noisy["link"], None, 0.0, S.CTRL * F32(0.5))):
        F = len(th)
        pairs = [(k, t) for t in range(F) for k in range(-1, F + 1)]
        lines = _run(host_exe, _clip_text(th, m, link, sc, ms, ctrl) + "".join(f"member {k} {t}\n" for k, t in pairs))
        assert len(lines) == len(pairs)
        for (k, t), ln in zip(pairs, lines):
            linked = S.linked(th, sc, ms, link, k, t)
            assert int(ln[0]) == int(linked), (k, t)
            if not linked:
                assert ln[1] == "0"
                continue
            P = S.chain(th, m, k, t)
            member, q = S.project(P, ctrl)
            assert int(ln[1]) == int(member), (k, t)
            assert ln[2:11] == [_d(v) for v in P], (k, t)
            if member:
                assert ln[11:19] == [_d(v) for v in q], (k, t)
            n += 1
    assert not S.project(S.chain(bad, M, 6, 6))[0] and S.linked(bad, score, 0.1, cut, 6, 6)
    print(f"HOST members and chains: {n} linked pairs bit-equal")


def test_host_program_weights_and_refits(host_exe):
    rng = np.random.default_rng(11)
    clip = S.noisy_clip(F=12, garbage=3, gap=(5, 6), cut=9)
    qs = [S.project(S.chain(clip["theta"], clip["M"], t, t))[1] for t in (0, 1, 2, 3, 4)]
    text, want = _clip_text(clip["theta"], clip["M"], clip["link"], None, 0.0, S.CTRL), []
    d2 = np.float64(0.05) * np.float64(0.05)
    for R, dist in ((0, 0), (12, 0), (12, 1), (12, 12), (31, 17), (5, 3)):
        q, c = qs[dist % 5], qs[(dist + 1) % 5]
        text += f"weight {R} {dist} " + " ".join(_d(v) for v in q) + " " + " ".join(_d(v) for v in c) + f" {_d(d2)}\n"
        r2 = S.r2_of(q, c)
        want.append([_d(S.triangle(R, dist)), _d(r2), _d(S.omega(r2, d2))])
    cs = qs + [qs[0] + 1e-3 * rng.standard_normal(8) for _ in range(8)]
    cs.append(np.zeros(8))                                           # all four points in one place: a pivot fails
    cs.append(np.array([0.3, 0.1, np.nan, 0.2, 0.1, 0.5, 0.6, 0.7]))  # a NaN fails every comparison of a pivot
    for c in cs:
        text += "refit 1 " + " ".join(_d(v) for v in c) + "\n"
    text += "refit 0 " + " ".join(_d(v) for v in qs[0]) + "\n"
    lines = _run(host_exe, text)
    assert lines[:len(want)] == want
    solved = 0
    for c, ln in zip(cs + [qs[0]], lines[len(want):]):
        h, ok = S.refit(c, S.CTRL, ln is not lines[-1])
        assert int(ln[0]) == int(ok)
        if ok:
            assert ln[1:] == [_d(v) for v in h]
            solved += 1
    assert solved == len(cs) - 2 and lines[-1][0] == "0"
    # a round trip: the refit of a theta's own points is that theta
    for t in (0, 1, 2):
        h, ok = S.refit(qs[t])
        assert ok and np.abs(np.array(h) - clip["theta"][t][:8].astype(np.float64)).max() < 1e-13
    print(f"HOST weights and refits: {len(want)} weights, {solved} refits bit-equal, 3 failed solves agree")


# ------------------------------------------------------------------------------------------------ refusals
_HOST = (ctypes.c_double * 4096)()


def test_refusals_without_a_device():
    """every refusal returns -1 before anything could be launched (the pointers are host memory)"""
    from sfh_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(ctypes.addressof(_HOST))
    q = ctypes.c_void_p(p.value + 4096)
    ok = [p, None, 0.0, p, p, 4, 12, 12, 3, 0.05, 1, None, q, p, p, None]
    for k, v, word in ((5, -1, b"frames"), (6, -1, b"back"), (6, 32, b"back"), (7, -1, b"ahead"), (7, 32, b"ahead"), (8, -1, b"iters"),
                       (9, 0.0, b"delta"), (9, -1.0, b"delta"), (9, float("nan"), b"delta"), (9, float("inf"), b"delta"), (9, 1e-200, b"delta"),
                       (10, 0, b"min_members"), (0, None, b"null"), (3, None, b"null"), (4, None, b"null"), (12, None, b"null"),
                       (13, None, b"null"), (14, None, b"null"), (12, p, b"overlaps"), (12, ctypes.c_void_p(p.value + 35 * 4), b"overlaps")):
        args = list(ok)
        args[k] = v
        assert lib.sfh_track_smooth(*args) == -1 and word in lib.sfh_last_error(), (k, v, lib.sfh_last_error())
    args = list(ok)
    args[5] = 0                                                      # an empty clip: nothing to launch, nothing refused
    assert lib.sfh_track_smooth(*args) == 0


def test_value_errors_on_the_host():
    from sfh_amd.track import smooth_theta, track_game
    th = torch.eye(3).reshape(1, 1, 3, 3).repeat(4, 1, 1, 1)
    M, ok = th[1:].clone(), torch.ones(3, dtype=torch.int32)
    for bad in (dict(radius=-1), dict(radius=32), dict(radius=(1, 32)), dict(radius=(1, 2, 3)), dict(iters=-1), dict(delta=0.0),
                dict(delta=float("nan")), dict(delta=float("inf")), dict(min_members=0), dict(ctrl=np.zeros((3, 2))),
                dict(ctrl=np.full((4, 2), np.nan))):
        with pytest.raises(ValueError, match="smooth_theta"):
            smooth_theta(th, M, ok, **bad)
    with pytest.raises(ValueError, match="CUDA"):                    # propagate_theta's own
        smooth_theta(th, M, ok)
    with pytest.raises(ValueError, match="CUDA"):
        smooth_theta(th.numpy(), M, ok)
    import inspect
    sig = inspect.signature(track_game).parameters
    assert sig["smooth_radius"].default is None and sig["smooth_iters"].default == 3 and sig["smooth_delta"].default == 0.05
    assert sig["smooth_min_members"].default == 1
