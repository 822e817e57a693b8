"""GPU checks of the temporal smoothing of theta (track_smooth_kernel in csrc/track.hip, sfh_amd.track.smooth_theta) against
the numpy restatement tests/smooth_ref.py.  Every operation of the rule is stated and its order fixed, so members, theta_out
and stats are held to the restatement BIT FOR BIT (a NaN against a NaN): there is no bound in this file.  Outputs sit behind
64-element guards and are pre-filled with NaN (integers: a sentinel).  The figures of the noisy clip go to
profiles/smooth_parity.jsonl next to the restatement's own (tests/test_smooth_host.py)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import smooth_ref as S
import track_cases as K
from conftest import ROOT
from test_gpu_track import THETA0, Guarded, _aligner, _bits, _clip, _cuda, _lib, _p, _st

pytestmark = pytest.mark.gpu
F32 = np.float32
PARITY = os.path.join(ROOT, "profiles", "smooth_parity.jsonl")
WHAT = "device against the restatement, noisy clip"


def _same(a, b):
    """bit-equal, a NaN matching a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _smooth(theta, M, link, score=None, max_score=0.0, back=12, ahead=12, iters=3, delta=0.05, min_members=1, ctrl=None):
    L, lib = _lib()
    F = theta.shape[0]
    out, mem, stats = Guarded((F, 9)), Guarded((F,), torch.int32), Guarded((F, 3), torch.float64)
    d_theta, d_M, d_link = _cuda(theta), _cuda(M), _cuda(np.asarray(link, dtype=np.int32))     # held until the launch has run
    d_score = _cuda(score) if score is not None else None
    pts = np.ascontiguousarray(ctrl, dtype=F32) if ctrl is not None else None
    L.check(lib.sfh_track_smooth(_p(d_theta), _p(d_score) if d_score is not None else None, max_score, _p(d_M), _p(d_link), F, back, ahead,
                                 iters, delta, min_members, pts.ctypes.data if pts is not None else None, _p(out.t), _p(mem.t),
                                 _p(stats.t), _st()), "smooth")
    torch.cuda.synchronize()
    assert out.intact() and mem.intact() and stats.intact()
    return out.t.cpu().numpy(), mem.t.cpu().numpy(), stats.t.cpu().numpy()


def _against_the_restatement(name, theta, M, link, **kw):
    got = _smooth(theta, M, link, **kw)
    ref = S.smooth(theta, M, link, **{**kw, "ctrl": kw["ctrl"] if kw.get("ctrl") is not None else S.CTRL})
    assert got[1].tolist() == ref[1].tolist(), name
    assert _same(got[0], ref[0]), (name, got[0], ref[0])
    assert _same(got[2], ref[2]), (name, got[2], ref[2])
    return got


# ------------------------------------------------------------------------------------------------ 0. existence
def test_the_feature_exists():
    import sfh_amd.track as tr
    L, lib = _lib()
    assert "sfh_track_smooth" in L.SIGNATURES and hasattr(lib, "sfh_track_smooth")
    assert callable(tr.smooth_theta)
    import inspect
    assert "smooth_radius" in inspect.signature(tr.track_game).parameters


# ------------------------------------------------------------------------------------------------ 1. the rule
WINDOWS = ((0, 0), (1, 0), (0, 1), (2, 2), (31, 31))


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"{w[0]}-{w[1]}")
def test_windows_on_exact_inputs(window):
    """the dyadic clip, every frame good: bit-equal to the restatement; against fl32 of the true theta the gap is reported"""
    back, ahead = window
    theta, M = K.dyadic_clip(8)
    for F in (8, 2, 1):
        out, mem, stats = _against_the_restatement(f"F={F}", theta[:F], M[:F], np.ones(F, np.int32), back=back, ahead=ahead)
        assert mem.tolist() == [min(t, back) + 1 + min(F - 1 - t, ahead) for t in range(F)]
        gap = S.exact_gap(out, theta[:F])
        print(f"EXACT back {back} ahead {ahead} F {F}: {gap[0]} fp32 ulps where the true entry is not 0, |entry| <= {gap[1]:.3g} where it is; "
              f"bit-equal to the true theta: {bool(np.array_equal(_bits(out), _bits(theta[:F])))}")
        assert gap[0] <= S.EXACT_ULPS and gap[1] <= S.EXACT_ZERO
        assert not stats[:, 1:].any()                                # the members agree exactly: no spread, no deviation


def _rule_cases():
    theta, M = K.dyadic_clip(8)
    ones = np.ones(8, dtype=np.int32)
    bad = theta.copy()
    bad[2], bad[4], bad[5] = 0.0, np.nan, theta[5]
    bad[5, 3] = np.inf
    nan_score = np.zeros(8, dtype=F32)
    nan_score[6] = np.nan
    nan_score[1] = 0.5
    cut1, cut2 = ones.copy(), ones.copy()
    cut1[3] = 0
    cut2[3] = cut2[5] = 0
    tie = theta.copy()
    tie[3] = np.nan
    tie[2], tie[4] = theta[2] + F32(0.3), theta[4] - F32(0.17)
    tie[[0, 1, 5, 6, 7]] = 0.0
    hor = theta.copy()
    hor[4] = [0.5, 0, 0.1, 0, 0.5, 0, 0, 1.0, -0.6]                  # W changes sign over the control points
    noisy = (theta + F32(0.01) * np.random.default_rng(3).standard_normal(theta.shape).astype(F32)).astype(F32)
    noisy[:, 8] = 1.0
    return {
        "zero-nan-inf": (bad, M, ones, dict(back=2, ahead=2), [2, 3, 3, 2, 2, 3, 2, 2]),      # good: 0 1 3 6 7
        "zero-nan-inf-causal": (bad, M, ones, dict(back=3, ahead=0), [1, 2, 2, 3, 2, 1, 2, 2]),
        "nan-score": (noisy, M, ones, dict(back=2, ahead=2, score=nan_score, max_score=0.1), [2, 3, 4, 4, 4, 4, 3, 2]),      # good: 0 2 3 4 5 7
        "one-cut": (noisy, M, cut1, dict(back=2, ahead=2), [3, 3, 3, 3, 4, 5, 4, 3]),       # (2, 3) is cut
        "two-cuts": (noisy, M, cut2, dict(back=31, ahead=31), [3, 3, 3, 2, 2, 3, 3, 3]),
        "tie": (tie, M, ones, dict(back=1, ahead=2, iters=0), None),
        "tie-reweighted": (tie, M, ones, dict(back=1, ahead=2, iters=3), None),
        "min-members-1": (bad, M, ones, dict(back=2, ahead=2, min_members=1), None),
        "min-members-3": (bad, M, ones, dict(back=2, ahead=2, min_members=3), None),
        "mixed-sign": (hor, M, ones, dict(back=1, ahead=1), [2, 3, 3, 2, 2, 2, 3, 2]),
        "all-bad": (np.zeros_like(theta), M, ones, dict(back=2, ahead=2), [0] * 8),
        "other-ctrl": (noisy, M, ones, dict(back=2, ahead=1, ctrl=np.array([[-0.5, -0.25], [0.75, 0], [0.5, 0.5], [-1, 0.75]], dtype=F32)), None),
        "asymmetric-noisy": (noisy, M, ones, dict(back=3, ahead=1, iters=2, delta=0.01), None),
    }


RULE_CASES = _rule_cases()


@pytest.mark.parametrize("case", list(RULE_CASES))
def test_rule(case):
    theta, M, link, kw, want_members = RULE_CASES[case]
    out, mem, stats = _against_the_restatement(case, theta, M, link, **kw)
    if want_members is not None:
        assert mem.tolist() == want_members
    produced = ~np.isnan(out).any(axis=1)
    assert np.array_equal(produced, mem >= kw.get("min_members", 1)) and np.array_equal(np.isnan(stats[:, 0]), ~produced)
    assert (out[produced, 8] == 1.0).all()
    if case == "all-bad":
        assert np.isnan(out).all() and np.isnan(stats).all()
    if case == "min-members-3":
        assert produced.any() and not produced.all()
    if case == "tie":                                                # the back member is the reference: test_smooth_host.py's hand case
        q2, q4 = S.project(S.chain(theta, M, 2, 3))[1], S.project(S.chain(theta, M, 4, 3))[1]
        g2, g4 = S.triangle(1, 1), S.triangle(2, 1)
        c = q2 + (g4 * (q4 - q2)) / (g2 + g4)
        assert mem[3] == 2 and np.array_equal(_bits(out[3]), _bits(np.array([F32(v) for v in S.refit(c)[0]] + [F32(1)], dtype=F32)))
    if case in ("zero-nan-inf", "mixed-sign"):                       # the good frames are exact, so the filled ones are the true thetas
        true = K.dyadic_clip(8)[0]
        gap = S.exact_gap(out, true)
        assert gap[0] <= S.EXACT_ULPS and gap[1] <= S.EXACT_ZERO


# ------------------------------------------------------------------------------------------------ 2. the noisy clip
@functools.lru_cache(maxsize=None)
def _noisy_ref(radius, iters):
    clip = S.noisy_clip()
    return S.smooth(clip["theta"], clip["M"], clip["link"], back=radius, ahead=radius, iters=iters)


def _record(row):
    print(json.dumps(row))
    try:
        kept = [json.loads(ln) for ln in open(PARITY)] if os.path.exists(PARITY) else []
        same = lambda r: r.get("what") == WHAT and (r["radius"], r["iters"]) == (row["radius"], row["iters"])
        with open(PARITY, "w") as f:
            for r in [r for r in kept if not same(r)] + [row]:
                f.write(json.dumps(r) + "\n")
    except OSError:          # a read-only checkout: the figures are still printed
        pass


@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("radius", [6, 12])
def test_noisy_clip(radius, iters):
    """60 frames, one garbage theta, a four-frame gap, a cut (smooth_ref.noisy_clip): the device gives the restatement's bits"""
    clip = S.noisy_clip()
    out, mem, stats = _smooth(clip["theta"], clip["M"], clip["link"], back=radius, ahead=radius, iters=iters)
    ref, ref_mem, ref_stats = _noisy_ref(radius, iters)
    diff_theta = int((_bits(out) != _bits(ref)).sum() - (np.isnan(out) & np.isnan(ref) & (_bits(out) != _bits(ref))).sum())
    diff_stats = int((_bits(stats) != _bits(ref_stats)).sum() - (np.isnan(stats) & np.isnan(ref_stats) & (_bits(stats) != _bits(ref_stats))).sum())
    err = np.array([S.corner_error(out[t], clip["true"][t]) for t in range(len(out))])
    e_in = np.array([S.corner_error(clip["theta"][t], clip["true"][t]) for t in range(len(out))])
    _record({"what": WHAT, "radius": radius, "iters": iters, "frames": len(out), "members_equal": bool(np.array_equal(mem, ref_mem)),
             "theta_words_differing": diff_theta, "stats_words_differing": diff_stats,
             "median_in_px": round(float(np.median(e_in[clip["good"]])), 4), "median_out_px": round(float(np.median(err[clip["good"]])), 4),
             "garbage_out_px": round(float(err[clip["garbage"]]), 4)})
    assert np.array_equal(mem, ref_mem) and _same(out, ref) and _same(stats, ref_stats)
    assert not np.isnan(out).any()                                   # every frame is produced, the gap included


# ------------------------------------------------------------------------------------------------ 3. the Python layer
def _clip_tensors():
    clip = S.noisy_clip()
    return clip, _cuda(clip["theta"]).reshape(-1, 1, 3, 3), _cuda(clip["M"]).reshape(-1, 1, 3, 3), _cuda(clip["link"])


def test_smooth_theta_forms_and_repeatability():
    from sfh_amd.track import smooth_theta
    clip, theta, M, link = _clip_tensors()
    ref, ref_mem, ref_stats = _noisy_ref(12, 3)
    th, stats, mem = smooth_theta(theta, M, link)
    assert th.shape == theta.shape and stats.shape == (60, 3) and stats.dtype == torch.float64 and mem.dtype == torch.int32
    assert _same(th.cpu().numpy().reshape(60, 9), ref) and _same(stats.cpu().numpy(), ref_stats) and mem.cpu().tolist() == ref_mem.tolist()
    # a second call, the F - 1 row form, the (F,3,3) form and a side stream: the same bits
    th2, stats2, mem2 = smooth_theta(theta, M, link, radius=(12, 12), iters=3, delta=0.05, ctrl=S.CTRL, min_members=1)
    th3, stats3, mem3 = smooth_theta(theta.reshape(60, 3, 3), M[1:].contiguous(), link[1:].contiguous())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        th4, stats4, mem4 = smooth_theta(theta, M, link)
    side.synchronize()
    assert th3.shape == (60, 3, 3)
    for a, b, c in ((th2, stats2, mem2), (th3, stats3, mem3), (th4, stats4, mem4)):
        assert _same(a.cpu().numpy().reshape(60, 9), ref) and _same(b.cpu().numpy(), ref_stats) and torch.equal(c, mem)
    # the causal form, a score gate, other settings: the restatement's bits through the Python layer
    score = np.full(60, 0.01, dtype=F32)
    score[clip["garbage"]] = 0.5
    th5, stats5, mem5 = smooth_theta(theta, M, link, score=_cuda(score), max_score=0.1, radius=(6, 0), iters=1, delta=0.02, min_members=2)
    r5 = S.smooth(clip["theta"], clip["M"], clip["link"], score=score, max_score=0.1, back=6, ahead=0, iters=1, delta=0.02, min_members=2)
    assert _same(th5.cpu().numpy().reshape(60, 9), r5[0]) and _same(stats5.cpu().numpy(), r5[2]) and mem5.cpu().tolist() == r5[1].tolist()
    assert np.isnan(r5[0]).any() and not np.isnan(r5[0]).all()
    empty = smooth_theta(theta[:0], M[:0], link[:0])
    assert empty[0].shape == (0, 1, 3, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)
    for bad in (dict(M=M[:3]), dict(ok=link.long()), dict(score=_cuda(score[:5]), max_score=0.1), dict(theta=theta.double()), dict(radius=32),
                dict(theta=theta.cpu())):
        kw = {**dict(theta=theta, M=M, ok=link), **bad}
        with pytest.raises(ValueError):
            smooth_theta(kw.pop("theta"), kw.pop("M"), kw.pop("ok"), **kw)


def test_track_game_smoothed_round_trip(tmp_path):
    from sfh_amd import outputs as O
    from sfh_amd.mapping import CourtMapping
    from sfh_amd.track import smooth_theta, track_game
    frames, _ = _clip(6)
    names = [f"frame_{k:04d}" for k in range(6)]
    theta = np.tile(THETA0, (6, 1)).reshape(6, 1, 3, 3)
    theta[2] = np.array([1.3, 0.4, -0.2, 0.3, 0.7, 0.5, 0.1, 0.2, 1.0], dtype=F32).reshape(1, 3, 3)
    scores = [0.01, 0.02, 0.5, 0.01, 0.6, 0.01]
    with O.CourtJsonWriter(str(tmp_path), "clip", "test-model") as wr:
        for k, n in enumerate(names):
            wr.add(n, scores[k], theta[k])
    dst = str(tmp_path / "out" / "clip_smoothed_court.json")
    assert track_game(wr.path, list(frames), dst, max_score=0.1, batch=4, names=names, smooth_radius=(2, 1), smooth_iters=2,
                      smooth_delta=0.04, smooth_min_members=2) == dst
    cm = CourtMapping(dst)
    text = open(dst).read()
    raw = json.loads(text)
    assert cm.names == names and cm.model == "test-model" and np.allclose(cm.scores, scores)
    M, _, _, ok = _aligner()(_cuda(frames))
    th, stats, mem = smooth_theta(_cuda(theta.astype(F32)), M, ok, score=_cuda(np.array(scores, dtype=F32)), max_score=0.1, radius=(2, 1),
                                  iters=2, delta=0.04, min_members=2)
    th, stats, mem = th.cpu().numpy().reshape(6, 9), stats.cpu().numpy(), mem.cpu().numpy()
    assert _same(cm.theta.reshape(6, 9), th)
    produced = ~np.isnan(th).any(axis=1)
    assert produced.any() and [raw[n]["source"] for n in names] == [k if produced[k] else -1 for k in range(6)]
    assert [raw[n]["members"] for n in names] == mem.tolist()
    for key, col in (("spread", 1), ("deviation", 2)):
        for k, n in enumerate(names):
            v = raw[n][key]
            assert (v is None and np.isnan(stats[k, col])) or v == stats[k, col]
    assert raw[names[2]]["deviation"] is None and "null" in text     # frame 2 fails the gate: it is no member of its own window
