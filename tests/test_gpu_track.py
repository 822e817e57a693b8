"""GPU checks of the inter-frame tracking (csrc/track.hip, sfh_amd.track) against the numpy restatement tests/track_ref.py:
the kernels one by one, then the whole alignment, the batching forms, the propagation and the clip driver.  Every output of
an entry sits behind 64-element guards, overwritten outputs are pre-filled with NaN (integers: a sentinel), and every
comparison prints ``RATIO name: error / bound`` and asserts it <= 1.  The rows of the whole-alignment comparison go to
profiles/track_parity.jsonl."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import det_ref
import step_tail_ref as ST
import track_cases as K
import track_ref as T
from conftest import ROOT

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64
PARITY = os.path.join(ROOT, "profiles", "track_parity.jsonl")
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
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 0. existence
def test_the_feature_exists():
    import sfh_amd.track as tr
    L, lib = _lib()
    for n in ("sfh_track_axis", "sfh_track_planes", "sfh_track_workspace_bytes", "sfh_track_accumulate", "sfh_track_step",
              "sfh_track_propagate"):
        assert n in L.SIGNATURES and hasattr(lib, n)
    assert tr.SUMS == 46 and callable(tr.FrameAligner) and callable(tr.propagate_theta) and callable(tr.track_game)


# ------------------------------------------------------------------------------------------------ 1. planes
@pytest.mark.parametrize("bgr", [0, 1])
@pytest.mark.parametrize("size", [(8, 8), (72, 136), (144, 256)], ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_planes(f, size, bgr):
    L, lib = _lib()
    H, W = size
    fr = np.random.default_rng(f * 100 + H + bgr).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    fr[2], fr[3] = 0, 255
    want = T.planes(fr, f, bool(bgr))
    out = Guarded(want.shape)
    d_fr = _cuda(fr)
    L.check(lib.sfh_track_planes(_p(d_fr), 4, H, W, f, bgr, _p(out.t), _st()), "planes")
    got = out.t.cpu().numpy()
    assert out.intact() and np.array_equal(_bits(got), _bits(want))
    assert not got[2].any() and (got[3] == 1.0).all()
    if H > 8:
        assert not np.array_equal(want, T.planes(fr, f, not bgr))            # the flag matters
    print(f"RATIO planes f={f} {W}x{H} bgr={bgr}: 0 (bit-equal, {got.size} values)")


# ------------------------------------------------------------------------------------------------ 2. accumulate
def _accumulate(lib, M, planes, n, ia, ib, P, H, W, f, delta, ws, nbytes):
    return lib.sfh_track_accumulate(_p(M), _p(planes), n, _p(ia), _p(ib), P, H, W, f, delta, _p(ws), nbytes, _st())


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("grid", K.GRIDS, ids=lambda g: f"{g[1]}x{g[0]}")
def test_accumulate(grid, P):
    """level 1 on frames of the grid's own size.  P = 3: the pair (0, 1), the same pair again and its reverse (1, 0) - or, for
    the kinds that follow, (2, 0): any pairing of the batch's frames"""
    L, lib = _lib()
    hl, wl = grid
    fr = K.plane_frames(hl, wl)
    pl = T.planes(fr, 1)
    _, yn = T.grid(1, hl, wl)
    Ms = K.kernel_Ms(yn, min(hl - 1, hl // 2 + 1))
    nslab, need = T.slabs(hl, wl), lib.sfh_track_workspace_bytes(P, hl, wl)
    assert need == nslab * P * T.SUMS * 8
    d_pl = Guarded(pl.shape)
    d_fr = _cuda(fr)
    L.check(lib.sfh_track_planes(_p(d_fr), 3, hl, wl, 1, 0, _p(d_pl.t), _st()), "planes")
    assert np.array_equal(_bits(d_pl.t.cpu().numpy()), _bits(pl))
    groups = [[k] for k in range(7)] if P == 1 else [[0, 0, 0], [1, 2, 3], [4, 5, 6]]
    pairs = [(0, 1)] if P == 1 else [(0, 1), (0, 1), (1, 0)]
    worst = 0.0
    for gi, kinds in enumerate(groups):
        pr = pairs if gi % 2 == 0 else [(2, 0)] + pairs[1:]
        ia, ib = (_cuda(np.array(v, dtype=np.int32)) for v in zip(*pr))
        d_M = _cuda(Ms[kinds])
        args = (d_M, d_pl.t, 3, ia, ib, P, hl, wl, 1, K.DELTA)
        ws = Guarded((nslab, P, T.SUMS), torch.float64)
        if gi == 0:
            assert _accumulate(lib, *args, ws.t, need - 1) == -1 and b"workspace" in lib.sfh_last_error()
            torch.cuda.synchronize()
            assert ws.untouched()                                     # one byte short: nothing written
        L.check(_accumulate(lib, *args, ws.t, need), "accumulate")
        part = ws.t.cpu().numpy()
        assert ws.intact() and np.isfinite(part).all()                # every slab element written
        for p, (kind, (a, b)) in enumerate(zip(kinds, pr)):
            ref, A = T.sums(Ms[kind], pl[a], pl[b], hl, wl, 1, K.DELTA)
            got = det_ref.det_sum(np.zeros(T.SUMS), part[:, p])
            n = ref[T.N]
            assert got[T.N] == n, (K.KERNEL_M_IDS[kind], got[T.N], n)                  # the counted pixels: exact
            ratio = ST.ratio(got[:45], ref[:45], T.sums_bound(A[:45], n))
            worst = max(worst, ratio)
            print(f"RATIO accumulate {wl}x{hl} P={P} {K.KERNEL_M_IDS[kind]} pair {(a, b)}: {ratio:.3g} (n = {int(n)})")
            assert ratio <= 1.0, (K.KERNEL_M_IDS[kind], got, ref)
            if kind in (5, 6):                                        # NaN M, and the shift that leaves nothing: exactly +0.0
                assert n == 0 and not _bits(part[:, p]).any()
            if kind == 0 and hl > 2:
                assert n > 0.8 * (hl - 1) * (wl - 1)
        if P == 3 and gi == 0:                                        # the repeated pair: the same bits; the reversed one: not
            assert np.array_equal(_bits(part[:, 0]), _bits(part[:, 1])) and not np.array_equal(part[:, 1], part[:, 2])
        if gi == 0:
            # a second call, and a call on a side stream beside a busy stream: the same bits
            ws2, ws3 = Guarded((nslab, P, T.SUMS), torch.float64), Guarded((nslab, P, T.SUMS), torch.float64)
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
    assert worst <= 1.0


def test_accumulate_refuses_nothing_for_a_bad_index_but_counts_nothing():
    """an index outside the frames cannot be refused without a read-back: the pair counts no pixel"""
    L, lib = _lib()
    hl, wl = 18, 32
    pl = _cuda(T.planes(K.plane_frames(hl, wl), 1))
    need = lib.sfh_track_workspace_bytes(2, hl, wl)
    ws = Guarded((1, 2, T.SUMS), torch.float64)
    ia, ib = _cuda(np.array([0, 3], dtype=np.int32)), _cuda(np.array([1, -1], dtype=np.int32))
    L.check(_accumulate(lib, _cuda(np.stack([K.IDENTITY] * 2)), pl, 3, ia, ib, 2, hl, wl, 1, K.DELTA, ws.t, need), "accumulate")
    part = ws.t.cpu().numpy()
    assert ws.intact() and part[0, 0, T.N] > 0 and not _bits(part[0, 1]).any()


# ------------------------------------------------------------------------------------------------ 3. step
def test_step():
    """on the device's own partials of seven copies of one pair (72 x 136, level 1: six slabs), edited on the host where a
    case needs it.  Pairs: 0 accepted; 1 rejected on its mean cost although its cost sum fell; 2 rejected on n < nmin although the mean cost fell; 3 singular; 4 a
    NaN cost; 5 dead on its first evaluation; 6 as 0, for the max_cost gate."""
    L, lib = _lib()
    hl, wl, P, Lv = 72, 136, 7, 2
    pl = _cuda(T.planes(K.plane_frames(hl, wl), 1))
    nslab, need = T.slabs(hl, wl), lib.sfh_track_workspace_bytes(P, hl, wl)
    ia, ib = _cuda(np.zeros(P, dtype=np.int32)), _cuda(np.ones(P, dtype=np.int32))
    nmin = T.nmin_of(0.5, hl, wl)

    def partials(d_M):
        ws = Guarded((nslab, P, T.SUMS), torch.float64)
        L.check(_accumulate(lib, d_M, pl, 3, ia, ib, P, hl, wl, 1, K.DELTA, ws.t, need), "accumulate")
        return ws.t.cpu().numpy().copy()

    acc, sums, lam = Guarded((P, 9)), Guarded((P, T.SUMS), torch.float64), Guarded((P,), torch.float64)
    piv, dead, nxt, ok = Guarded((P,), torch.int32), Guarded((P,), torch.int32), Guarded((P, 9)), Guarded((P,), torch.int32)
    stats, accepted = Guarded((P, Lv, 3), torch.float64), Guarded((P, Lv), torch.int32)
    bufs = dict(acc=acc, sums=sums, lam=lam, piv=piv, dead=dead, next=nxt, ok=ok, stats=stats, accepted=accepted)

    def call(part, first, last, m_eval, level, max_cost):
        d_part = _cuda(part)
        L.check(lib.sfh_track_step(_p(d_part), nslab, P, first, last, _p(m_eval), _p(acc.t), _p(sums.t), _p(lam.t), _p(piv.t),
                                   _p(dead.t), _p(nxt.t), _p(stats.t), _p(accepted.t), _p(ok.t), level, Lv, nmin, max_cost, _st()), "step")
        torch.cuda.synchronize()
        return {k: v.t.cpu().numpy().copy() for k, v in bufs.items()}

    states = [T.StepState() for _ in range(P)]
    ties = 0

    def compare(got, part, first, last, m_eval, level, max_cost):
        nonlocal ties
        for p in range(P):
            S = det_ref.det_sum(np.zeros(T.SUMS), part[:, p])
            st = states[p]
            cand, tie = st.step(S, m_eval[p], bool(first), bool(last), level, nmin)
            assert np.array_equal(_bits(got["sums"][p]), _bits(st.S)), (p, first)        # the ascending chain, NaN meets NaN
            assert got["lam"][p] == st.lam and bool(got["piv"][p]) == st.piv and bool(got["dead"][p]) == st.dead, (p, first)
            assert got["accepted"][p, level] == st.accepted and got["ok"][p] == st.ok(max_cost), (p, first)
            assert np.array_equal(_bits(got["acc"][p]), _bits(st.M))
            assert np.array_equal(_bits(got["stats"][p, level]), _bits(np.array(st.stats()))), (p, got["stats"][p, level], st.stats())
            same = _bits(got["next"][p]) == _bits(cand)
            off = np.abs(_bits(got["next"][p]).astype(np.int64) - _bits(cand).astype(np.int64))
            assert (same | (tie & (off <= 1))).all(), (p, got["next"][p], cand)
            ties += int((~same).sum())

    M0 = np.stack([K.IDENTITY] * P)
    d_M0 = _cuda(M0)
    p1 = partials(d_M0)
    p1[:, 3, :36] = 0.0                                      # pair 3: a singular system
    p1[:, 5, T.N] *= 0.125                                   # pair 5: too few pixels on its first evaluation
    got = call(p1, 1, 0, d_M0, 0, 0.0)
    compare(got, p1, 1, 0, M0, 0, 0.0)
    assert [s.dead for s in states] == [False] * 5 + [True, False] and [s.piv for s in states] == [True] * 3 + [False] + [True] * 3
    assert np.array_equal(_bits(got["next"][[3, 5]]), _bits(M0[[3, 5]])) and got["ok"].tolist() == [1, 1, 1, 1, 1, 0, 1]
    assert not np.array_equal(got["next"][0], M0[0])

    cand = got["next"].copy()
    d_cand = _cuda(cand)
    p2 = partials(d_cand)
    mean1 = float(states[0].stats()[1])
    S2 = det_ref.det_sum(np.zeros(T.SUMS), p2[:, 0])
    scale = 0.5 * mean1 / (S2[T.COST] / S2[T.N])             # pairs 0, 6: half the accepted mean cost
    p2[:, 0, T.COST] *= scale
    p2[:, 6, T.COST] *= scale
    S1, S21 = det_ref.det_sum(np.zeros(T.SUMS), p1[:, 1]), det_ref.det_sum(np.zeros(T.SUMS), p2[:, 1])
    p2[:, 1, T.COST] *= 0.9 * S1[T.COST] / S21[T.COST]       # pair 1: the cost SUM falls to 0.9, on 0.6 of the pixels (still
    p2[:, 1, T.N] *= 0.6                                     # >= nmin): the MEAN rises to ~1.5 - rejected
    p2[:, 2, T.COST] *= 0.125 * scale                        # pair 2: the mean cost halves, on a quarter of the pixels
    p2[:, 2, T.N] *= 0.25
    p2[0, 4, T.COST] = np.nan                                # pair 4
    for max_cost, want_ok in ((0.0, [1, 1, 1, 1, 1, 0, 1]), (0.75 * mean1, [1, 0, 0, 0, 0, 0, 1])):
        snap = {k: v.full.clone() for k, v in bufs.items()}
        keep = [(s.M, s.S, s.lam, s.piv, s.dead, s.accepted) for s in states]
        got = call(p2, 0, 0, d_cand, 0, max_cost)
        compare(got, p2, 0, 0, cand, 0, max_cost)
        assert got["ok"].tolist() == want_ok, (max_cost, got["ok"])
        assert [s.accepted for s in states] == [1, 0, 0, 0, 0, 0, 1]
        assert [s.lam for s in states] == [1e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-3, 1e-4]
        if max_cost == 0.0:                                  # the same step again under the other gate: state put back
            for k, v in bufs.items():
                v.full.copy_(snap[k])
            for s, (M, S, lm, pv, dd, ac) in zip(states, keep):
                s.M, s.S, s.lam, s.piv, s.dead, s.accepted = M, S, lm, pv, dd, ac
    # level 0 only was written; every guard intact
    assert np.isnan(stats.t.cpu().numpy()[:, 1]).all() and (accepted.t.cpu().numpy()[:, 1] == -7777).all()
    assert all(x.intact() for x in bufs.values())
    # the first step of the next level on unedited partials: the dead pair stays dead by its flag alone; last: M_next = M_acc
    m_eval = got["next"].copy()
    p3 = partials(_cuda(m_eval))
    got = call(p3, 1, 1, _cuda(m_eval), 1, 0.0)
    compare(got, p3, 1, 1, m_eval, 1, 0.0)
    assert got["dead"].tolist() == [0, 0, 0, 0, 0, 1, 0] and np.array_equal(_bits(got["next"]), _bits(got["acc"]))
    assert np.array_equal(_bits(got["acc"][5]), _bits(M0[5]))
    print(f"RATIO step: 0 (decisions, lambda, counters, flags, statistics and sums equal; {ties} candidates off by one ulp at a "
          "flagged tie)")


# ------------------------------------------------------------------------------------------------ 4. the whole alignment
def _aligner(**kw):
    from sfh_amd.track import FrameAligner
    return FrameAligner(**{**dict(frame_size=(K.W, K.H), factors=K.FACTORS, iters=K.ITERS, delta=K.DELTA, min_overlap=K.MIN_OVERLAP), **kw})


@functools.lru_cache(maxsize=None)
def _device_alignments():
    """every case in one call: frame 0 the previous frame, frames 1.. the cases' current frames, pairs (0, k)"""
    frames = np.stack([K.align_pair(K.ALIGN_IDS[0])[0]] + [K.align_pair(c)[1] for c in K.ALIGN_IDS])
    n = len(K.ALIGN_IDS)
    out = _aligner()(_cuda(frames), pairs=([0] * n, list(range(1, n + 1))))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("case", K.ALIGN_IDS)
def test_whole_alignment(case):
    k = K.ALIGN_IDS.index(case)
    M, stats, accepted, ok = _device_alignments()
    ref, M_true = K.align_ref(case), K.align_pair(case)[2]
    assert M.shape == (len(K.ALIGN_IDS), 1, 3, 3) and stats.shape == (len(K.ALIGN_IDS), 3, 3)
    err = T.corner_error(M[k].reshape(9), M_true, K.W, K.H)
    bound = T.align_margin(ref["err"], M_true, K.W, K.H)
    _record({"case": case, "start_px": round(ref["start"], 4), "err_ref_px": ref["err"], "err_device_px": err, "bound_px": bound,
             "accepted_ref": ref["accepted"].tolist(), "accepted_device": accepted[k].tolist(), "ok": int(ok[k]),
             "mean_cost_device": stats[k, -1, 1], "mean_cost_ref": ref["stats"][-1, 1],
             "same_bits": bool(np.array_equal(_bits(M[k].reshape(9)), _bits(ref["M"])))})
    print(f"RATIO whole_alignment {case}: {err / bound:.3g} (device {err:.4f} px, restatement {ref['err']:.4f} px)")
    assert err <= bound
    assert accepted[k].tolist() == ref["accepted"].tolist() and ok[k] == ref["ok"] == 1
    assert np.array_equal(stats[k, :, 2], ref["stats"][:, 2])
    if _rows[-1]["same_bits"]:                               # the same trajectory: the costs differ by the order of their sums alone
        assert np.allclose(stats[k, :, :2], ref["stats"][:, :2], rtol=1e-9, atol=0.0)


# ------------------------------------------------------------------------------------------------ 5. prev= and pairs=
def _clip(n=6):
    """n frames of one camera move: frame t sees the scene through C_t = M*_1 .. M*_t -> (frames, C (n,9) float64, M* (n,9))"""
    steps = [K.IDENTITY, K.pan(2.5, -1.0), K.ALIGN_CASES["perspective"], K.pan(-3.0, 1.5), K.ALIGN_CASES["zoomrot"], K.pan(1.0, 2.0)]
    C, frames, Ms = np.eye(3), [], []
    for t in range(n):
        m = np.asarray(steps[t % len(steps)], dtype=np.float64).reshape(3, 3) if t else np.eye(3)
        C = C @ m
        Ms.append(m.reshape(9))
        frames.append(K.frame(C.reshape(9)))
    return np.stack(frames), np.stack(Ms).astype(F32)


def test_prev_and_pairs_are_the_same_alignment():
    frames, _ = _clip(4)
    d = _cuda(frames)
    al = _aligner()
    whole = [t.cpu().numpy() for t in al(d)]
    assert whole[0].shape == (3, 1, 3, 3) and whole[1].shape == (3, 3, 3) and whole[2].shape == (3, 3) and whole[3].shape == (3,)
    with_prev = [t.cpu().numpy() for t in al(d[1:], prev=d[:1])]
    by_pairs = [t.cpu().numpy() for t in al(d, pairs=(torch.tensor([0, 1, 2]), np.array([1, 2, 3])))]
    started = [t.cpu().numpy() for t in al(d, pairs=([0, 1, 2], [1, 2, 3]), m0=torch.eye(3, device="cuda").reshape(1, 1, 3, 3).repeat(3, 1, 1, 1))]
    for other in (with_prev, by_pairs, started):
        for a, b in zip(whole, other):
            assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    assert whole[3].tolist() == [1, 1, 1] and (whole[2] > 0).any()
    # a second call reuses the buffers: the same bits; one frame alone and an empty batch give empty outputs
    again = [t.cpu().numpy() for t in al(d)]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(whole, again)) and len(al._work) == 1      # four frames, three pairs: one set of buffers
    for empty in (al(d[:1]), al(d[:0])):
        assert [tuple(t.shape) for t in empty] == [(0, 1, 3, 3), (0, 3, 3), (0, 3), (0,)]
    assert al(d[:1], prev=d[1:2])[0].shape == (1, 1, 3, 3)
    for bad, what in ((dict(pairs=([0, 4], [1, 2])), "outside"), (dict(pairs=([0, -1], [1, 2])), "outside"), (dict(pairs=([0], [1, 2])), "indices"),
                      (dict(pairs=([0.5], [1.0])), "integer"), (dict(prev=d[:2]), "one frame"), (dict(prev=d[:1], pairs=([0], [1])), "exclude"),
                      (dict(m0=torch.eye(3, device="cuda")), "m0"), (dict(m0=torch.zeros(3, 1, 3, 3)), "m0")):
        with pytest.raises(ValueError, match=what):
            al(d, **bad)
    for fr, what in ((d[:, :, :, :2], "uint8"), (d.float(), "uint8"), (d[0], "uint8"), (d[:, ::2], "frame_size"), (d[:, :, ::2], "frame_size"),
                     (d.permute(0, 2, 1, 3), "frame_size"), (d.transpose(1, 2).contiguous().transpose(1, 2), "contiguous")):
        with pytest.raises(ValueError, match=what):
            al(fr)


# ------------------------------------------------------------------------------------------------ 6. propagate
def _propagate(lib, L, theta, M, link, score, max_score, max_gap):
    F = theta.shape[0]
    out, src = Guarded((F, 9)), Guarded((F,), torch.int32)
    d_theta, d_M, d_link = _cuda(theta), _cuda(M), _cuda(np.asarray(link, dtype=np.int32))     # held until the launch has run
    d_score = _cuda(score) if score is not None else None
    L.check(lib.sfh_track_propagate(_p(d_theta), _p(d_score) if d_score is not None else None, max_score, _p(d_M), _p(d_link), F, max_gap,
                                    _p(out.t), _p(src.t), _st()), "propagate")
    torch.cuda.synchronize()
    assert out.intact() and src.intact()
    return out.t.cpu().numpy(), src.t.cpu().numpy()


def test_propagate_rule():
    """the host cases, on the device: bit-equal to the restatement (and, dyadic, to the true thetas)"""
    L, lib = _lib()
    theta, M = K.dyadic_clip(8)
    ones = np.ones(8, dtype=np.int32)
    nan_score = np.zeros(8, dtype=F32)
    nan_score[4] = np.nan
    b1 = theta.copy()
    b1[3], b1[4] = 0.0, theta[4] + F32(0.3)
    b2 = theta.copy()
    b2[3] = np.nan
    b3 = theta.copy()
    b3[2:6] = np.inf
    cut1, cut2 = ones.copy(), ones.copy()
    cut1[3] = 0
    cut2[3] = cut2[4] = 0
    n = 0
    for th, link, score, max_score, gap, want_src in (
            (b1, ones, nan_score, 0.1, 30, [0, 1, 2, 2, 5, 5, 6, 7]), (b2, ones, None, 0.0, 30, [0, 1, 2, 2, 4, 5, 6, 7]),
            (b2, cut1, None, 0.0, 30, [0, 1, 2, 4, 4, 5, 6, 7]), (b2, cut2, None, 0.0, 30, [0, 1, 2, -1, 4, 5, 6, 7]),
            (b3, ones, None, 0.0, 1, [0, 1, 1, -1, -1, 6, 6, 7]), (b3, ones, None, 0.0, 2, [0, 1, 1, 1, 6, 6, 6, 7]),
            (b3, ones, None, 0.0, 0, [0, 1, -1, -1, -1, -1, 6, 7]), (np.zeros_like(theta), ones, None, 0.0, 30, [-1] * 8),
            (theta, ones, np.full(8, 0.2, dtype=F32), 0.1, 30, [-1] * 8), (theta[:1], ones[:1], None, 0.0, 30, [0])):
        got, src = _propagate(lib, L, th, M[:len(th)], link, score, max_score, gap)
        ref, ref_src = T.propagate(th, M[:len(th)], link, score, max_score, gap)
        assert src.tolist() == ref_src.tolist() == want_src
        assert np.array_equal(_bits(got), _bits(ref))
        carried = np.array(want_src) >= 0
        assert np.array_equal(_bits(got[carried]), _bits(theta[:len(th)][carried])) and np.isnan(got[~carried]).all()
        n += 1
    print(f"RATIO propagate rule: 0 (bit-equal, {n} cases)")


THETA0 = np.array([0.62, 0.05, 0.04, -0.04, 0.58, -0.03, 0.05, -0.03, 1.0], dtype=F32)


def test_propagate_a_clip():
    """six frames of one camera move with a known theta*_t = theta*_0 M*_1 .. M*_t; frames 2 and 3 carry a garbage theta and a
    score above the gate.  The device's aligner and propagation against the restatement's, in corner pixels of theta"""
    from sfh_amd.track import propagate_theta
    frames, Mstar = _clip(6)
    true = [THETA0.astype(np.float64).reshape(3, 3)]
    for t in range(1, 6):
        true.append(true[-1] @ Mstar[t].astype(np.float64).reshape(3, 3))
    true = np.stack([(m / m[2, 2]).reshape(9) for m in true]).astype(F32)
    theta, score = true.copy(), np.full(6, 0.01, dtype=F32)
    theta[2] = [1.3, 0.4, -0.2, 0.3, 0.7, 0.5, 0.1, 0.2, 1.0]
    theta[3] = theta[2][::-1].copy()
    theta[3][8] = 1.0
    score[2:4] = 0.5
    M, stats, accepted, ok = _aligner()(_cuda(frames))
    th2, src = propagate_theta(_cuda(theta).reshape(6, 1, 3, 3), M, ok, score=_cuda(score), max_score=0.1, max_gap=30)
    assert th2.shape == (6, 1, 3, 3) and src.dtype == torch.int32
    th2, src = th2.cpu().numpy().reshape(6, 9), src.cpu().numpy()
    refs = [T.align(frames[t - 1], frames[t], factors=K.FACTORS, iters=K.ITERS, delta=K.DELTA, min_overlap=K.MIN_OVERLAP) for t in range(1, 6)]
    M_ref = np.stack([K.IDENTITY] + [r["M"] for r in refs])
    ref, ref_src = T.propagate(theta, M_ref, np.array([0] + [r["ok"] for r in refs]), score, 0.1, 30)
    assert src.tolist() == ref_src.tolist() == [0, 1, 1, 4, 4, 5] and ok.cpu().tolist() == [1] * 5
    good = [0, 1, 4, 5]
    assert np.array_equal(_bits(th2[good]), _bits(theta[good]))
    for t in (2, 3):
        e_ref, e_dev = T.corner_error(ref[t], true[t], K.W, K.H), T.corner_error(th2[t], true[t], K.W, K.H)
        bound = T.align_margin(e_ref, true[t], K.W, K.H)
        print(f"RATIO propagate clip frame {t}: {e_dev / bound:.3g} (device {e_dev:.4f} px, restatement {e_ref:.4f} px, "
              f"garbage theta {T.corner_error(theta[t], true[t], K.W, K.H):.1f} px)")
        assert e_dev <= bound and e_ref < 0.1
    # the same through the F-row form, row 0 unread
    M_f = torch.cat([torch.full((1, 1, 3, 3), float("nan"), device="cuda"), M])
    ok_f = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), ok])
    th3, src3 = propagate_theta(_cuda(theta).reshape(6, 3, 3), M_f, ok_f, score=_cuda(score), max_score=0.1)
    assert th3.shape == (6, 3, 3) and np.array_equal(_bits(th3.cpu().numpy().reshape(6, 9)), _bits(th2)) and src3.cpu().tolist() == src.tolist()
    for bad in (dict(M=M[:3]), dict(ok=ok.long()), dict(score=_cuda(score[:5])), dict(max_gap=-1), dict(theta=_cuda(theta).double().reshape(6, 1, 3, 3))):
        kw = {**dict(theta=_cuda(theta).reshape(6, 1, 3, 3), M=M, ok=ok, score=_cuda(score), max_score=0.1, max_gap=30), **bad}
        with pytest.raises(ValueError):
            propagate_theta(kw.pop("theta"), kw.pop("M"), kw.pop("ok"), **kw)


# ------------------------------------------------------------------------------------------------ 7. the clip driver
def test_track_game_round_trip(tmp_path):
    from sfh_amd import outputs as O
    from sfh_amd.mapping import CourtMapping
    from sfh_amd.track import propagate_theta, track_game
    frames, Mstar = _clip(6)
    names = [f"frame_{k:04d}" for k in range(6)]
    theta = np.tile(THETA0, (6, 1)).reshape(6, 1, 3, 3)
    theta[2] = np.array([1.3, 0.4, -0.2, 0.3, 0.7, 0.5, 0.1, 0.2, 1.0], dtype=F32).reshape(1, 3, 3)
    scores = [0.01, 0.02, 0.5, 0.01, 0.6, 0.01]
    with O.CourtJsonWriter(str(tmp_path), "clip", "test-model") as wr:
        for k, n in enumerate(names):
            wr.add(n, scores[k], theta[k])
    dst = str(tmp_path / "out" / "clip_tracked_court.json")
    assert track_game(wr.path, list(frames), dst, max_score=0.1, batch=4, names=names) == dst          # batches of 4 + 2: prev carries over
    cm = CourtMapping(dst)
    raw = json.load(open(dst))
    assert cm.names == names and cm.model == "test-model" and np.allclose(cm.scores, scores)
    src = [raw[n]["source"] for n in names]
    assert src == [0, 1, 1, 3, 3, 5]
    # what the driver wrote is what the two calls give on the whole clip at once
    M, _, _, ok = _aligner()(_cuda(frames))
    th2, src2 = propagate_theta(_cuda(theta.astype(F32)), M, ok, score=_cuda(np.array(scores, dtype=F32)), max_score=0.1)
    assert src2.cpu().tolist() == src and np.array_equal(_bits(cm.theta.reshape(6, 9)), _bits(th2.cpu().numpy().reshape(6, 9)))
    assert np.array_equal(cm.theta[[0, 1, 3, 5]], theta[[0, 1, 3, 5], 0]) and not np.array_equal(cm.theta[2], theta[2, 0])
    with pytest.raises(ValueError, match="not aligned"):
        track_game(wr.path, list(frames), dst, names=names[::-1])
    with pytest.raises(ValueError, match="5 frames"):
        track_game(wr.path, list(frames[:5]), dst)
