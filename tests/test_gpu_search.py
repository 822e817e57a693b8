"""GPU checks of the coarse shift search of the tracker (csrc/track.hip: sfh_track_search; sfh_amd.track.FrameAligner(search=))
against the numpy restatement tests/search_ref.py.  The summation order is part of the rule, so the table of means, shift,
found, m0 and sstats are held to the restatement bit for bit (a NaN meets a NaN: its sign and payload are not part of the
rule); the whole alignment behind the search is held by tests/test_gpu_track.py's criterion, track_ref.align_margin.  Every
output sits behind 64-element guards and is pre-filled with NaN (integers: a sentinel).  The conditions that keep these
comparisons honest are asserted on the restatement alone in tests/test_search_host.py.  The rows of the whole-alignment
comparison go to profiles/search_parity.jsonl."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import search_cases as C
import search_ref as S
import track_cases as K
import track_ref as T
from conftest import ROOT

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64
PARITY = os.path.join(ROOT, "profiles", "search_parity.jsonl")
WHAT = "device, searched alignment"
_rows = []


def _lib():
    from sfh_amd import _lib as L
    assert "sfh_track_search" in L.SIGNATURES, "the coarse shift search is not in include/sfh_amd.h"
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    """bit-equal, a NaN meeting a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]))


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


class Outputs:
    def __init__(self, P, ncand):
        self.ws = Guarded((P, ncand), torch.float64)
        self.shift, self.found = Guarded((P, 2), torch.int32), Guarded((P,), torch.int32)
        self.m0, self.sstats = Guarded((P, 9)), Guarded((P, 3), torch.float64)

    def all(self):
        return (self.ws, self.shift, self.found, self.m0, self.sstats)

    def host(self):
        return [g.t.cpu().numpy() for g in self.all()]


def _search(lib, c, d_planes, d_ia, d_ib, out, ws_bytes=None, **over):
    a = {**c, **over}
    P = len(c["ia"])
    need = lib.sfh_track_search_workspace_bytes(P, a["rx"], a["ry"])
    return lib.sfh_track_search(_p(d_planes), a["planes"].shape[0], _p(d_ia), _p(d_ib), P, a["H"], a["W"], a["f"], a["rx"], a["ry"],
                                a["delta"], a["nmin"], _p(out.ws.t), need if ws_bytes is None else ws_bytes, _p(out.shift.t),
                                _p(out.found.t), _p(out.m0.t), _p(out.sstats.t), _st())


def _run_case(name):
    L, lib = _lib()
    c = C.kernel_case(name)
    P, ncand = len(c["ia"]), S.candidates(c["rx"], c["ry"])
    assert lib.sfh_track_search_workspace_bytes(P, c["rx"], c["ry"]) == P * ncand * 8
    dev = (_cuda(c["planes"]), _cuda(c["ia"]), _cuda(c["ib"]))
    out = Outputs(P, ncand)
    L.check(_search(lib, c, *dev, out), "track_search")
    torch.cuda.synchronize()
    return L, lib, c, dev, out


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", C.KERNEL_IDS)
def test_search_kernels(name):
    L, lib, c, dev, out = _run_case(name)
    tab, shift, found, m0, sstats, _ = C.kernel_ref(name)
    got = out.host()
    assert all(g.intact() for g in out.all())
    bad = int((~(np.isnan(got[0]) & np.isnan(tab)) & (_bits(got[0]) != _bits(tab))).sum())
    print(f"RATIO search {name}: {bad} of {tab.size} means differ; shift {got[1].tolist()} found {got[2].tolist()}")
    assert _same(got[0], tab), (name, bad)
    assert _same(got[1], shift) and _same(got[2], found) and _same(got[3], m0) and _same(got[4], sstats), (name, got[1:], shift, found, sstats)
    assert not np.isnan(got[3]).any()                                # every word of every output was written
    if c["contents"] == "flat":
        assert got[1].tolist() == [[0, 0]] * len(found) and not got[0][np.isfinite(got[0])].any()
    if c["contents"] == "dyadic":
        assert not _bits(got[4][:, 0]).any()                          # exactly +0.0 at the true shift
    if c["contents"] == "nmin":
        assert not got[2].any() and np.array_equal(got[3], np.tile(K.IDENTITY, (len(found), 1)))
    if name.endswith("p3"):                                           # the repeated pair: the same bits; the reversed one: not
        assert _same(got[0][0], got[0][1]) and _same(got[1][0], got[1][1])
        if c["contents"] == "random" and tab.shape[1] > 1:            # (0, 0) alone: rho is even in r, the reversed pair costs the same
            assert not _same(got[0][1], got[0][2])


def test_second_call_and_side_stream_give_the_same_bits():
    name = "18x32/random/p3"
    L, lib, c, dev, out = _run_case(name)
    first = out.host()
    out2, out3 = Outputs(3, S.candidates(c["rx"], c["ry"])), Outputs(3, S.candidates(c["rx"], c["ry"]))
    L.check(_search(lib, c, *dev, out2), "track_search")
    busy = torch.randn(1024, 1024, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(4):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        L.check(_search(lib, c, *dev, out3), "track_search")
    torch.cuda.synchronize()
    for other in (out2, out3):
        assert all(g.intact() for g in other.all()) and all(_same(a, b) for a, b in zip(first, other.host()))
    assert _same(first[0], C.kernel_ref(name)[0])


def test_refusals_launch_nothing():
    """one case per line of the header's list; the outputs and the workspace keep their fill"""
    L, lib = _lib()
    name = "18x32/random/p3"
    c = C.kernel_case(name)
    dev = (_cuda(c["planes"]), _cuda(c["ia"]), _cuda(c["ib"]))
    out = Outputs(3, S.candidates(c["rx"], c["ry"]))
    need = lib.sfh_track_search_workspace_bytes(3, c["rx"], c["ry"])
    for over, word in ((dict(f=0), b"level"), (dict(f=17), b"level"), (dict(f=7), b"level"), (dict(H=8, W=256), b"2x2"),
                       (dict(rx=33), b"radius"), (dict(ry=-1), b"radius"), (dict(delta=0.0), b"delta"), (dict(delta=float("inf")), b"delta"),
                       (dict(delta=float("nan")), b"delta"), (dict(nmin=0.0), b"nmin"), (dict(nmin=float("nan")), b"nmin")):
        assert _search(lib, c, *dev, out, ws_bytes=need if "rx" not in over and "ry" not in over else 1 << 20, **over) == -1
        assert word in lib.sfh_last_error(), (over, lib.sfh_last_error())
    assert _search(lib, c, *dev, out, ws_bytes=need - 1) == -1 and b"workspace" in lib.sfh_last_error()
    args = [_p(dev[0]), 3, _p(dev[1]), _p(dev[2]), 3, c["H"], c["W"], c["f"], c["rx"], c["ry"], c["delta"], c["nmin"], _p(out.ws.t), need,
            _p(out.shift.t), _p(out.found.t), _p(out.m0.t), _p(out.sstats.t), _st()]
    for k in (0, 2, 3, 12, 14, 15, 16, 17):
        a = list(args)
        a[k] = None
        assert lib.sfh_track_search(*a) == -1 and (b"null" in lib.sfh_last_error() or b"workspace" in lib.sfh_last_error())
    for pairs in (0, 65536):
        a = list(args)
        a[4] = pairs
        assert lib.sfh_track_search(*a) == -1 and b"pairs" in lib.sfh_last_error()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.all())
    L.check(lib.sfh_track_search(*args), "track_search")              # and the unedited call runs
    torch.cuda.synchronize()
    assert _same(out.host()[0], C.kernel_ref(name)[0])


# ------------------------------------------------------------------------------------------------ 2. the public layer
def _aligner(**kw):
    from sfh_amd.track import FrameAligner
    return FrameAligner(**{**dict(frame_size=(K.W, K.H), factors=K.FACTORS, iters=K.ITERS, delta=K.DELTA, min_overlap=K.MIN_OVERLAP), **kw})


@functools.lru_cache(maxsize=None)
def _device_pans():
    """every pan case in one call: frame 0 the previous frame, frames 1.. the cases' current frames, pairs (0, k)"""
    frames = _cuda(np.stack([C.wide_pair(C.PAN_IDS[0])[0]] + [C.wide_pair(c)[1] for c in C.PAN_IDS]))
    n = len(C.PAN_IDS)
    pairs = ([0] * n, list(range(1, n + 1)))
    al = _aligner(search=C.RADIUS)
    searched = al(frames, pairs=pairs)
    coarse = al.coarse_shift(frames, pairs=pairs)
    started = _aligner()(frames, pairs=pairs, m0=coarse[0])            # the plain aligner from the search's start
    plain = _aligner()(frames, pairs=pairs)
    torch.cuda.synchronize()
    assert len(al._work) == 1                                        # one set of buffers serves both calls
    return [[t.cpu().numpy() for t in out] for out in (searched, coarse, started, plain)]


def _record(row):
    _rows.append(row)
    print("SEARCH", json.dumps(row))
    try:
        kept = [json.loads(ln) for ln in open(PARITY)] if os.path.exists(PARITY) else []
        with open(PARITY, "w") as f:
            for r in [r for r in kept if r.get("what") != WHAT] + _rows:
                f.write(json.dumps(r) + "\n")
    except OSError:          # a read-only checkout: the figures are still printed
        pass


@pytest.mark.parametrize("case", C.PAN_IDS)
def test_searched_alignment(case):
    k = C.PAN_IDS.index(case)
    searched, coarse, started, plain = _device_pans()
    ref, M_true = C.searched_ref(case), C.wide_pair(case)[2]
    n = len(C.PAN_IDS)
    assert coarse[0].shape == (n, 1, 3, 3) and coarse[1].shape == (n, 2) and coarse[2].shape == (n,) and coarse[3].shape == (n, 3)
    assert coarse[0].dtype == F32 and coarse[1].dtype == np.int32 and coarse[2].dtype == np.int32 and coarse[3].dtype == np.float64
    # coarse_shift is the restatement's search, bit for bit
    assert _same(coarse[1][k], ref["shift"]) and coarse[2][k] == ref["found"] == 1
    assert _same(coarse[0][k].reshape(9), ref["m0"]) and _same(coarse[3][k], ref["sstats"])
    # FrameAligner(search=) is the plain aligner started at coarse_shift's m0: the same four outputs
    for a, b in zip(searched, started):
        assert a.dtype == b.dtype and _same(a[k], b[k])
    M, stats, accepted, ok = searched
    err = T.corner_error(M[k].reshape(9), M_true, K.W, K.H)
    err_plain = T.corner_error(plain[0][k].reshape(9), M_true, K.W, K.H)
    bound = T.align_margin(ref["err"], M_true, K.W, K.H)
    _record({"what": WHAT, "case": case, "radius": list(C.RADIUS), "shift": coarse[1][k].tolist(), "err_ref_px": ref["err"], "err_device_px": err,
             "bound_px": bound, "plain_err_device_px": err_plain, "accepted_ref": ref["accepted"].tolist(), "accepted_device": accepted[k].tolist(),
             "ok": int(ok[k]), "same_bits": bool(_same(M[k].reshape(9), ref["M"]))})
    print(f"RATIO searched_alignment {case}: {err / bound:.3g} (device {err:.4f} px, restatement {ref['err']:.4f} px, plain device {err_plain:.1f} px)")
    assert err <= bound and ok[k] == ref["ok"] == 1
    assert accepted[k].tolist() == ref["accepted"].tolist() and np.array_equal(stats[k, :, 2], ref["stats"][:, 2])
    assert err_plain > 10.0                                          # what the search is for


def test_search_none_changes_no_bit():
    frames = _cuda(np.stack([K.align_pair(K.ALIGN_IDS[0])[0]] + [K.align_pair(c)[1] for c in K.ALIGN_IDS[2:6]]))
    without = [t.cpu().numpy() for t in _aligner()(frames)]
    none = [t.cpu().numpy() for t in _aligner(search=None)(frames)]
    with_prev = [t.cpu().numpy() for t in _aligner(search=None)(frames[1:], prev=frames[:1])]
    for other in (none, with_prev):
        for a, b in zip(without, other):
            assert a.dtype == b.dtype and _same(a, b)
    # with a search: prev= and pairs= are the same alignment too, and a second call reuses the buffers
    al = _aligner(search=C.RADIUS)
    whole = [t.cpu().numpy() for t in al(frames)]
    again = [t.cpu().numpy() for t in al(frames)]
    prev = [t.cpu().numpy() for t in al(frames[1:], prev=frames[:1])]
    by_pairs = [t.cpu().numpy() for t in al(frames, pairs=([0, 1, 2, 3], [1, 2, 3, 4]))]
    for other in (again, prev, by_pairs):
        assert all(_same(a, b) for a, b in zip(whole, other))
    cs = [t.cpu().numpy() for t in al.coarse_shift(frames)]
    cs_prev = [t.cpu().numpy() for t in al.coarse_shift(frames[1:], prev=frames[:1])]
    assert all(_same(a, b) for a, b in zip(cs, cs_prev)) and cs[2].tolist() == [1] * 4
    for empty in (al.coarse_shift(frames[:1]), al.coarse_shift(frames[:0])):
        assert [tuple(t.shape) for t in empty] == [(0, 1, 3, 3), (0, 2), (0,), (0, 3)]
    assert [tuple(t.shape) for t in al(frames[:1])] == [(0, 1, 3, 3), (0, 3, 3), (0, 3), (0,)]


def test_value_errors():
    frames = _cuda(np.stack([K.frame(), K.frame(K.pan(3.0, 1.0))]))
    al = _aligner(search=C.RADIUS)
    with pytest.raises(ValueError, match="search and m0"):
        al(frames, m0=torch.eye(3, device="cuda").reshape(1, 1, 3, 3))
    with pytest.raises(ValueError, match="coarse_shift needs search"):
        _aligner().coarse_shift(frames)
    with pytest.raises(ValueError, match="exclude"):
        al.coarse_shift(frames, prev=frames[:1], pairs=([0], [1]))
    with pytest.raises(ValueError, match="outside"):
        al.coarse_shift(frames, pairs=([0], [2]))
    with pytest.raises(ValueError, match="uint8"):
        al.coarse_shift(frames.float())
    for bad in ((8,), (33, 0), (0, -1), (8.0, 4)):
        with pytest.raises(ValueError, match="search"):
            _aligner(search=bad)
    with pytest.raises(ValueError, match="factors is empty"):
        _aligner(factors=(), search=(1, 1))


def test_track_game_round_trip_with_search(tmp_path):
    """a clip with one fast pan in it: the driver with search= writes what FrameAligner(search=) and propagate_theta give on the
    whole clip, and the frame behind the fast pan gets the theta the motion implies"""
    from sfh_amd import outputs as O
    from sfh_amd.mapping import CourtMapping
    from sfh_amd.track import propagate_theta, track_game
    steps = [K.IDENTITY, K.pan(2.5, -1.0), C.PAN_CASES["pan47"], K.pan(-3.0, 1.5), K.pan(1.0, 2.0)]
    Cm, frames = np.eye(3), []
    for m in steps:
        Cm = Cm @ np.asarray(m, dtype=np.float64).reshape(3, 3)
        frames.append(K.frame(Cm.reshape(9)))
    frames = np.stack(frames)
    theta0 = np.array([0.62, 0.05, 0.04, -0.04, 0.58, -0.03, 0.05, -0.03, 1.0], dtype=F32)
    true = [theta0.astype(np.float64).reshape(3, 3)]
    for m in steps[1:]:
        true.append(true[-1] @ np.asarray(m, dtype=np.float64).reshape(3, 3))
    true = np.stack([(m / m[2, 2]).reshape(9) for m in true]).astype(F32)
    names = [f"frame_{k:04d}" for k in range(5)]
    theta = true.copy().reshape(5, 1, 3, 3)
    theta[2] = np.array([1.3, 0.4, -0.2, 0.3, 0.7, 0.5, 0.1, 0.2, 1.0], dtype=F32).reshape(1, 3, 3)
    scores = [0.01, 0.02, 0.5, 0.01, 0.01]
    with O.CourtJsonWriter(str(tmp_path), "clip", "test-model") as wr:
        for k, n in enumerate(names):
            wr.add(n, scores[k], theta[k])
    dst = str(tmp_path / "out" / "clip_tracked_court.json")
    assert track_game(wr.path, list(frames), dst, max_score=0.1, batch=3, names=names, search=C.RADIUS) == dst
    cm = CourtMapping(dst)
    raw = json.load(open(dst))
    assert cm.names == names and [raw[n]["source"] for n in names] == [0, 1, 1, 3, 4]
    M, _, _, ok = _aligner(search=C.RADIUS)(_cuda(frames))
    th2, src = propagate_theta(_cuda(theta), M, ok, score=_cuda(np.array(scores, dtype=F32)), max_score=0.1)
    assert src.cpu().tolist() == [0, 1, 1, 3, 4] and _same(cm.theta.reshape(5, 9), th2.cpu().numpy().reshape(5, 9))
    # frame 2 against the restatement's searched alignment of its pair, by test_gpu_track.py's criterion for a carried theta
    ref = S.searched_align(frames[1], frames[2], C.RADIUS, factors=K.FACTORS, iters=K.ITERS, delta=K.DELTA, min_overlap=K.MIN_OVERLAP)
    M_ref = np.stack([K.IDENTITY, K.IDENTITY, ref["M"], K.IDENTITY, K.IDENTITY])
    th_ref, _ = T.propagate(theta.reshape(5, 9), M_ref, np.array([0, 1, ref["ok"], 1, 1]), np.array(scores, dtype=F32), 0.1, 30)
    e_ref, e_dev = T.corner_error(th_ref[2], true[2], K.W, K.H), T.corner_error(cm.theta[2].reshape(9), true[2], K.W, K.H)
    bound = T.align_margin(e_ref, true[2], K.W, K.H)
    plain = str(tmp_path / "out" / "clip_plain_court.json")
    track_game(wr.path, list(frames), plain, max_score=0.1, batch=3, names=names)
    e_plain = T.corner_error(CourtMapping(plain).theta[2].reshape(9), true[2], K.W, K.H)
    print(f"RATIO track_game frame 2 behind a 47 px pan: {e_dev / bound:.3g} (device {e_dev:.4f} px, restatement {e_ref:.4f} px, "
          f"without the search {e_plain:.1f} px of theta's corners)")
    assert e_dev <= bound and e_ref < 0.1
    # without the search M is off by more than 10 px (tests/test_search_host.py); theta0 scales a frame pixel by more than 0.5
    assert e_plain > 5.0
