"""Inter-frame homography tracking: what relates frame t of a clip to frame t - 1, and theta carried across it.

    al = FrameAligner(frame_size=(640, 360), factors=(8, 4, 2), iters=6, delta=0.06, min_overlap=0.25, max_cost=None)
    M, stats, accepted, ok = al(frames_u8)                       # consecutive pairs of the batch: B - 1 of them
    M, ... = al(frames_u8, prev=last_frame_of_previous_batch)    # B pairs: a clip processed in batches loses no pair
    M, ... = al(frames_u8, pairs=(ia, ib), m0=M_start)           # arbitrary pairs (previous ia[p], current ib[p]), caller's start
    theta2, source = propagate_theta(theta, M, ok, score=score, max_score=0.1, max_gap=30)
    theta_s, stats, members = smooth_theta(theta, M, ok, score=score, max_score=0.1, radius=12)   # radius=(12, 0): causal
    al = FrameAligner(frame_size=(640, 360), search=(16, 8))     # a coarse shift search gives every pair its start
    m0, shift, found, sstats = al.coarse_shift(frames_u8)        # the search alone

M (P,1,3,3) float32 maps the normalised coordinates of the current frame of a pair to those of its previous frame, so
theta_t = theta_{t-1} M_t.  stats (P,L,3) float64 = [first mean cost, last mean cost, counted pixels] per level, accepted
(P,L) int32, ok (P,) int32: 0 marks a cut or a failed alignment.  Direct photometric alignment on luma planes, coarse to fine,
``iters`` robust Levenberg-Marquardt steps per level.  The rule is stated once in include/sfh_amd.h above the ``sfh_track_*``
entries; csrc/track.hip runs it, tests/track_ref.py restates it in numpy.  The reference project has no counterpart.

``smooth_theta`` combines, per frame, the thetas of the good frames within ``radius`` carried to that frame across M: a robust
mean of estimates of one quantity, so it has no lag; it also outvotes an isolated bad theta and fills gaps.  The rule stands
above ``sfh_track_smooth``; tests/smooth_ref.py restates it.

``search=(rx, ry)`` widens the capture range: before the descent every whole-pixel shift (dx, dy), |dx| <= rx, |dy| <= ry, of the
coarsest plane (``factors[0]``; the reach in frame pixels is ``rx * factors[0]``) is scored by the tracker's own robust mean
cost, and the best one is the start.  The rule stands above ``sfh_track_search``; tests/search_ref.py restates it.  Two more
launches per call; with ``search=None`` every launch and every bit is as without the argument.

A call launches on the caller's current stream, synchronises nothing and reads nothing back (``pairs=`` given as host
sequences are checked on the host; given as device tensors they are read back once for that check): 1 launch per level for
the planes (2 with ``prev``) and 2 * (iters + 1) per level for the steps.  Planes, workspaces and state are held once per
(frames, pairs, size, stream); after the first call of a shape only the four outputs are new tensors.
"""
import json
import math
import os

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

SUMS = _lib.ABI.defines["SFH_TRACK_SUMS"]


def _frames_checked(fr, what, H, W):
    if not torch.is_tensor(fr):
        raise ValueError(f"FrameAligner: {what} must be a tensor")
    if not fr.is_cuda:
        raise ValueError(f"FrameAligner: {what} must be a CUDA tensor (there is no CPU path)")
    if fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[3] != 3:
        raise ValueError(f"FrameAligner: {what} must be uint8 (B,H,W,3), got {fr.dtype} {tuple(fr.shape)}")
    if fr.shape[1] != H or fr.shape[2] != W:
        raise ValueError(f"FrameAligner: {what} of {fr.shape[2]}x{fr.shape[1]}, frame_size is {W}x{H}")
    if not fr.is_contiguous():
        raise ValueError(f"FrameAligner: {what} must be contiguous")


class FrameAligner:
    def __init__(self, frame_size=(640, 360), factors=(8, 4, 2), iters=6, delta=0.06, min_overlap=0.25, max_cost=None, bgr=False,
                 search=None):
        """frame_size (W, H); factors: the pyramid, coarse to fine, each in 1..16 dividing W and H; delta: the scale of the
        Geman-McClure weight in luma units (0..1); min_overlap: the share of a level's pixels that must be counted;
        max_cost: a mean cost above it clears ``ok`` (None: no such gate); search: None, or (rx, ry), each in 0..32 - the
        radius of the coarse shift search in pixels of the plane of ``factors[0]``"""
        W, H = int(frame_size[0]), int(frame_size[1])
        factors, iters, delta, min_overlap = tuple(int(f) for f in factors), int(iters), float(delta), float(min_overlap)
        if W < 2 or H < 2:
            raise ValueError(f"FrameAligner: frame_size {frame_size}")
        for f in factors:
            if not 1 <= f <= 16 or H % f or W % f or H < 2 * f or W < 2 * f:
                raise ValueError(f"FrameAligner: level {f} (1..16) does not divide the frame {W}x{H}")
        if iters < 0:
            raise ValueError(f"FrameAligner: iters={iters} (>= 0)")
        if not delta > 0.0 or not math.isfinite(delta):
            raise ValueError(f"FrameAligner: delta={delta} (> 0)")
        if not 0.0 < min_overlap <= 1.0:
            raise ValueError(f"FrameAligner: min_overlap={min_overlap} (0 < . <= 1)")
        if max_cost is not None and not float(max_cost) > 0.0:
            raise ValueError(f"FrameAligner: max_cost={max_cost} (> 0, or None)")
        self.frame_size, self.factors, self.iters, self.delta, self.min_overlap = (W, H), factors, iters, delta, min_overlap
        self.max_cost, self.bgr = (None if max_cost is None else float(max_cost)), bool(bgr)
        if search is not None:
            if not isinstance(search, (tuple, list)) or len(search) != 2 or not all(
                    isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 32 for v in search):
                raise ValueError(f"FrameAligner: search={search!r} (None, or (rx, ry), whole numbers in 0..32)")
            if not factors:
                raise ValueError("FrameAligner: search needs a level to search on, factors is empty")
            search = (int(search[0]), int(search[1]))
        self.search = search
        self._work = {}        # (frames, pairs, device, stream) -> buffers

    def __getstate__(self):
        """configuration only: planes, workspaces and state are rebuilt on first use"""
        st = self.__dict__.copy()
        st["_work"] = {}
        return st

    def _buffers(self, N, P, dev):
        key = (N, P, dev, torch.cuda.current_stream(dev).cuda_stream)
        w = self._work.get(key)
        if w is None:
            lib = _lib.load()
            (W, H), fmin = self.frame_size, min(self.factors)
            nbytes = lib.sfh_track_workspace_bytes(P, H // fmin, W // fmin)
            if nbytes < 0:
                raise ValueError(f"FrameAligner: {P} pairs (1..65535)")
            i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
            w = self._work[key] = {
                "planes": [torch.empty((N, H // f, W // f), dtype=torch.float32, device=dev) for f in self.factors],
                "slabs": [lib.sfh_track_workspace_bytes(P, H // f, W // f) // (P * SUMS * 8) for f in self.factors],
                "ws": torch.empty(nbytes // 8, dtype=torch.float64, device=dev), "ws_bytes": nbytes,
                "M_acc": torch.empty((P, 9), dtype=torch.float32, device=dev),
                "cand": torch.empty((P, 9), dtype=torch.float32, device=dev),
                "start": torch.eye(3, dtype=torch.float32, device=dev).reshape(1, 9).repeat(P, 1),
                "sums": torch.empty((P, SUMS), dtype=torch.float64, device=dev),
                "lambda": torch.empty(P, dtype=torch.float64, device=dev),
                "piv": i32(P), "dead": i32(P),
                # the consecutive pairs (k, k + 1)
                "ia": torch.arange(0, P, dtype=torch.int32, device=dev), "ib": torch.arange(1, P + 1, dtype=torch.int32, device=dev),
            }
            if self.search is not None:
                sbytes = lib.sfh_track_search_workspace_bytes(P, *self.search)
                w["search_ws"], w["search_ws_bytes"] = torch.empty(sbytes // 8, dtype=torch.float64, device=dev), sbytes
        return w

    def _planes(self, lib, st, w, frames_u8, prev, N, levels):
        """the plane launches of the given levels: 1 per level, 2 with ``prev``"""
        (W, H), B = self.frame_size, frames_u8.shape[0]
        for li in levels:
            f, pl = self.factors[li], w["planes"][li]
            if prev is not None:
                _lib.check(lib.sfh_track_planes(_ptr(prev), 1, H, W, f, int(self.bgr), _ptr(pl), st), "track_planes")
            _lib.check(lib.sfh_track_planes(_ptr(frames_u8), B, H, W, f, int(self.bgr), _ptr(pl[N - B:]), st), "track_planes")

    def _search(self, lib, st, w, N, P, ia, ib, m0, shift, found, sstats):
        """the two launches of sfh_track_search on the planes of factors[0]"""
        (W, H), f = self.frame_size, self.factors[0]
        nmin = float(math.ceil(self.min_overlap * (H // f) * (W // f)))
        _lib.check(lib.sfh_track_search(_ptr(w["planes"][0]), N, _ptr(ia), _ptr(ib), P, H, W, f, self.search[0], self.search[1],
                                        self.delta, nmin, _ptr(w["search_ws"]), w["search_ws_bytes"], _ptr(shift), _ptr(found),
                                        _ptr(m0), _ptr(sstats), st), "track_search")

    def _pairs_checked(self, frames_u8, prev, pairs):
        """what __call__ and coarse_shift ask of their frames -> (device, B, N, P, ia, ib); ia, ib None: the consecutive pairs"""
        W, H = self.frame_size
        _frames_checked(frames_u8, "frames_u8", H, W)
        dev, B = frames_u8.device, frames_u8.shape[0]
        if prev is not None:
            if pairs is not None:
                raise ValueError("FrameAligner: prev and pairs exclude each other")
            _frames_checked(prev, "prev", H, W)
            if prev.shape[0] != 1 or prev.device != dev:
                raise ValueError(f"FrameAligner: prev must be one frame (1,{H},{W},3) on {dev}")
        N = B + (1 if prev is not None else 0)
        ia = ib = None
        if pairs is not None:
            ia, ib = self._indices(pairs, B, dev)
            P = ia.numel()
        else:
            P = max(N - 1, 0)
        return dev, B, N, P, ia, ib

    def coarse_shift(self, frames_u8, prev=None, pairs=None):
        """the search alone, on the frames and pairs as __call__ takes them -> (m0 (P,1,3,3) float32: the start the best shift
        stands for, shift (P,2) int32 = (dx, dy) in pixels of the plane of factors[0], found (P,) int32: 0 where no shift was
        admissible (m0 is then the identity), sstats (P,3) float64 = [the best mean cost, the mean cost of (0, 0), the counted
        pixels of the best]).  1 plane launch (2 with ``prev``) and 2 for the search; no synchronisation, no read-back."""
        if self.search is None:
            raise ValueError("FrameAligner: coarse_shift needs search=(rx, ry)")
        dev, B, N, P, ia, ib = self._pairs_checked(frames_u8, prev, pairs)
        out = (torch.empty((P, 1, 3, 3), dtype=torch.float32, device=dev), torch.empty((P, 2), dtype=torch.int32, device=dev),
               torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((P, 3), dtype=torch.float64, device=dev))
        if P == 0 or B == 0:
            return out
        with torch.cuda.device(dev):
            lib, st = _lib.load(), _stream()
            w = self._buffers(N, P, dev)
            if ia is None:
                ia, ib = w["ia"], w["ib"]
            self._planes(lib, st, w, frames_u8, prev, N, [0])
            self._search(lib, st, w, N, P, ia, ib, *out)
        return out

    @staticmethod
    def _indices(pairs, N, dev):
        if not isinstance(pairs, (tuple, list)) or len(pairs) != 2:
            raise ValueError("FrameAligner: pairs must be (ia, ib)")
        out = []
        for name, a in zip(("ia", "ib"), pairs):
            t = a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
            if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"FrameAligner: pairs {name} must be a 1-d integer array, got {t.dtype} {tuple(t.shape)}")
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= N):
                raise ValueError(f"FrameAligner: pairs {name} holds an index outside the {N} frames")
            out.append(t.to(torch.int32).to(dev))
        if out[0].numel() != out[1].numel():
            raise ValueError(f"FrameAligner: pairs of {out[0].numel()} and {out[1].numel()} indices")
        return out

    def __call__(self, frames_u8, prev=None, pairs=None, m0=None):
        """frames_u8 (B,H,W,3) uint8; prev (1,H,W,3): the frame before frames_u8[0]; pairs (ia, ib): integer sequences or
        tensors indexing frames_u8; m0 (P,1,3,3) | (P,3,3) float32: the start (default: the identity)"""
        (W, H), L = self.frame_size, len(self.factors)
        dev, B, N, P, ia, ib = self._pairs_checked(frames_u8, prev, pairs)
        if m0 is not None:
            if self.search is not None:
                raise ValueError("FrameAligner: search and m0 exclude each other (the search is about the identity)")
            if not torch.is_tensor(m0) or not m0.is_cuda or m0.dtype != torch.float32 or tuple(m0.shape) not in ((P, 1, 3, 3), (P, 3, 3)):
                raise ValueError(f"FrameAligner: m0 must be a float32 CUDA tensor ({P},1,3,3)")
            if not m0.is_contiguous():
                raise ValueError("FrameAligner: m0 must be contiguous")
        out = (torch.empty((P, 1, 3, 3), dtype=torch.float32, device=dev), torch.empty((P, L, 3), dtype=torch.float64, device=dev),
               torch.empty((P, L), dtype=torch.int32, device=dev), torch.empty((P,), dtype=torch.int32, device=dev))
        if P == 0 or B == 0:
            return out
        M_out, stats, accepted, ok = out
        with torch.cuda.device(dev):
            lib, st = _lib.load(), _stream()
            w = self._buffers(N, P, dev)
            if ia is None:
                ia, ib = w["ia"], w["ib"]
            start = m0 if m0 is not None else w["start"]
            if L == 0:
                M_out.copy_(start.view(P, 1, 3, 3))
                stats.fill_(float("nan")), accepted.zero_(), ok.fill_(1)
                return out
            self._planes(lib, st, w, frames_u8, prev, N, range(L))
            if self.search is not None:
                if "search_out" not in w:
                    w["search_out"] = (torch.empty((P, 9), dtype=torch.float32, device=dev), torch.empty((P, 2), dtype=torch.int32, device=dev),
                                       torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((P, 3), dtype=torch.float64, device=dev))
                self._search(lib, st, w, N, P, ia, ib, *w["search_out"])
                start = w["search_out"][0]
            max_cost = self.max_cost if self.max_cost is not None else 0.0
            cur = start
            for li, f in enumerate(self.factors):
                nmin = float(math.ceil(self.min_overlap * (H // f) * (W // f)))

                def accumulate(m):
                    _lib.check(lib.sfh_track_accumulate(_ptr(m), _ptr(w["planes"][li]), N, _ptr(ia), _ptr(ib), P, H, W, f, self.delta,
                                                        _ptr(w["ws"]), w["ws_bytes"], st), "track_accumulate")

                def step(first, last, m_eval, m_next):
                    _lib.check(lib.sfh_track_step(_ptr(w["ws"]), w["slabs"][li], P, first, last, _ptr(m_eval), _ptr(w["M_acc"]),
                                                  _ptr(w["sums"]), _ptr(w["lambda"]), _ptr(w["piv"]), _ptr(w["dead"]), _ptr(m_next),
                                                  _ptr(stats), _ptr(accepted), _ptr(ok), li, L, nmin, max_cost, st), "track_step")

                final = li == L - 1
                accumulate(cur)
                step(1, int(self.iters == 0), cur, M_out if (final and self.iters == 0) else w["cand"])
                for it in range(self.iters):
                    end = it == self.iters - 1
                    accumulate(w["cand"])
                    step(0, int(end), w["cand"], M_out if (final and end) else w["cand"])
                cur = w["cand"]
        return out


def _clip_checked(who, theta, M, ok, score, max_score):
    """what propagate_theta and smooth_theta ask of a clip -> (F, device, the score to gate by or None)"""
    for name, t in (("theta", theta), ("M", M), ("ok", ok)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} must be a CUDA tensor (there is no CPU path)")
    if theta.dtype != torch.float32 or theta.dim() not in (3, 4) or tuple(theta.shape[-2:]) != (3, 3) or theta.numel() != theta.shape[0] * 9:
        raise ValueError(f"{who}: theta must be float32 (F,1,3,3), got {theta.dtype} {tuple(theta.shape)}")
    F = theta.shape[0]
    if M.dtype != torch.float32 or M.numel() % 9 or M.numel() // 9 not in (F, F - 1) or ok.dtype != torch.int32 or ok.numel() != M.numel() // 9:
        raise ValueError(f"{who}: M float32 and ok int32 must have {F} or {F - 1} rows, got {tuple(M.shape)}, {tuple(ok.shape)}")
    if not (theta.is_contiguous() and M.is_contiguous() and ok.is_contiguous()):
        raise ValueError(f"{who}: theta, M and ok must be contiguous")
    use_score = score is not None and max_score is not None
    if use_score and (not torch.is_tensor(score) or not score.is_cuda or score.dtype != torch.float32 or score.numel() != F
                      or not score.is_contiguous()):
        raise ValueError(f"{who}: score must be a contiguous float32 CUDA tensor ({F},)")
    return F, theta.device, (score if use_score else None)


def _clip_rows(M, ok, F, dev):
    """M and ok as the entries read them: F rows, row t belongs to the pair (t - 1, t)"""
    M9, link = M.reshape(-1, 9), ok.reshape(-1)
    if M9.shape[0] == F - 1:
        M9 = torch.cat([torch.zeros((1, 9), dtype=torch.float32, device=dev), M9])
        link = torch.cat([torch.zeros((1,), dtype=torch.int32, device=dev), link])
    return M9, link


def propagate_theta(theta, M, ok, score=None, max_score=None, max_gap=30):
    """theta (F,1,3,3) | (F,3,3) float32; M, ok: FrameAligner's outputs over the clip - F rows (row t: the pair (t - 1, t);
    row 0 is not read) or F - 1 rows (the consecutive pairs of the F frames).  score (F,) float32 with max_score: the gate of
    visualize / TopViewRenderer.  -> (theta2 of theta's shape, source (F,) int32): frames without a usable theta get the
    nearest good frame's theta carried across the inter-frame homographies; source[t] = the frame it came from, t itself for a
    good frame, -1 (and nine NaNs) where no anchor is within max_gap unbroken links.  One launch, no read-back."""
    max_gap = int(max_gap)
    if max_gap < 0:
        raise ValueError(f"propagate_theta: max_gap={max_gap} (>= 0)")
    F, dev, score = _clip_checked("propagate_theta", theta, M, ok, score, max_score)
    theta2 = torch.empty_like(theta)
    source = torch.empty((F,), dtype=torch.int32, device=dev)
    if F == 0:
        return theta2, source
    with torch.cuda.device(dev):
        M9, link = _clip_rows(M, ok, F, dev)
        _lib.check(_lib.load().sfh_track_propagate(_ptr(theta), _ptr(score) if score is not None else None,
                                                   float(max_score) if score is not None else 0.0, _ptr(M9), _ptr(link), F, max_gap,
                                                   _ptr(theta2), _ptr(source), _stream()), "track_propagate")
    return theta2, source


def _radius(radius):
    r = (radius, radius) if isinstance(radius, (int, np.integer)) else tuple(radius)
    if len(r) != 2 or not all(isinstance(v, (int, np.integer)) and 0 <= v <= 31 for v in r):
        raise ValueError(f"smooth_theta: radius={radius!r} (an int or (back, ahead), each in 0..31)")
    return int(r[0]), int(r[1])


def smooth_theta(theta, M, ok, score=None, max_score=None, radius=12, iters=3, delta=0.05, ctrl=None, min_members=1):
    """theta, M, ok, score, max_score: as propagate_theta takes them.  radius: an int, or (back, ahead) - (r, 0) is the causal
    form; iters: the re-weightings after the plain weighted mean; delta: the scale of the Geman-McClure weight in normalised
    court units; ctrl: four (x, y) points of the normalised frame, host values (default: the lower three fifths of the frame);
    min_members: fewer members give nine NaNs.  -> (theta_s of theta's shape, stats (F,3) float64 = [sum of weights, robust rms
    spread of the members, the frame's own distance from the result (NaN where it has no usable theta)] over the control
    points in normalised court units, members (F,) int32).  One launch, no synchronisation, no read-back."""
    back, ahead = _radius(radius)
    iters, delta, min_members = int(iters), float(delta), int(min_members)
    if iters < 0:
        raise ValueError(f"smooth_theta: iters={iters} (>= 0)")
    if not delta > 0.0 or not math.isfinite(delta):
        raise ValueError(f"smooth_theta: delta={delta} (> 0)")
    if min_members < 1:
        raise ValueError(f"smooth_theta: min_members={min_members} (>= 1)")
    pts = None
    if ctrl is not None:
        pts = np.ascontiguousarray(np.asarray(ctrl.detach().cpu() if torch.is_tensor(ctrl) else ctrl, dtype=np.float32))
        if pts.shape != (4, 2) or not np.isfinite(pts).all():
            raise ValueError(f"smooth_theta: ctrl must be four finite (x, y) points, got shape {pts.shape}")
    F, dev, score = _clip_checked("smooth_theta", theta, M, ok, score, max_score)
    theta_s = torch.empty_like(theta)
    stats = torch.empty((F, 3), dtype=torch.float64, device=dev)
    members = torch.empty((F,), dtype=torch.int32, device=dev)
    if F == 0:
        return theta_s, stats, members
    with torch.cuda.device(dev):
        M9, link = _clip_rows(M, ok, F, dev)
        _lib.check(_lib.load().sfh_track_smooth(_ptr(theta), _ptr(score) if score is not None else None,
                                                float(max_score) if score is not None else 0.0, _ptr(M9), _ptr(link), F, back, ahead,
                                                iters, delta, min_members, pts.ctypes.data if pts is not None else None, _ptr(theta_s),
                                                _ptr(members), _ptr(stats), _stream()), "track_smooth")
    return theta_s, stats, members


def track_game(court_json, frames, dst_json, frame_size=None, factors=(8, 4, 2), iters=6, delta=0.06, min_overlap=0.25,
               max_cost=None, max_score=None, max_gap=30, batch=16, names=None, device="cuda", frames_format="array", bgr=False,
               smooth_radius=None, smooth_iters=3, smooth_delta=0.05, smooth_min_members=1, search=None):
    """The host driver, in the style of ``mapping.rectify_game``: frames - an iterable of host uint8 (H,W,3) arrays (or, with
    frames_format "jpeg" / "png", of files as bytes, decoded on the GPU) in the order of the predictions of ``court_json``
    (names: their frame names, checked when given).  Aligns the clip batch by batch, every batch with the last frame of the
    one before as ``prev``, propagates once over the whole clip and writes ``dst_json``: the court JSON with ``theta``
    replaced and a per-frame ``source`` (the frame the theta came from; -1: none, theta is NaN).  ``mapping.CourtMapping``
    reads it back.  With smooth_radius (an int or (back, ahead)) the clip is smoothed by ``smooth_theta`` instead of
    propagated: ``source`` is the frame itself where a theta was produced and -1 elsewhere, and ``members``, ``spread`` and
    ``deviation`` (smooth_theta's member count and second and third statistic; NaN is written as null) stand next to it.
    search: FrameAligner's, None or (rx, ry).  Returns dst_json."""
    from ._codec import frames_from_files
    from .mapping import CourtMapping
    if frames_format not in ("array", "jpeg", "png"):
        raise ValueError(f'track_game: frames_format={frames_format!r} ("array", "jpeg" or "png")')
    cm = CourtMapping(court_json, device=device)
    if names is not None:
        for k, (n, p) in enumerate(zip(names, cm.names)):
            if str(n) != p:
                raise ValueError(f"track_game: frame {k} is {n!r}, prediction {k} is {p!r} - frames and predictions are not aligned")
    tabs = cm.tables(device)
    dev = tabs["theta"].device
    state = {"al": None, "prev": None}
    Ms, oks = [], []

    def flush(chunk):
        if frames_format != "array":
            fr = frames_from_files(chunk, dev, frames_format)
        else:
            fr = torch.from_numpy(np.ascontiguousarray(np.stack(chunk))).to(dev)
        if state["al"] is None:
            size = frame_size if frame_size is not None else (fr.shape[2], fr.shape[1])
            state["al"] = FrameAligner(size, factors, iters, delta, min_overlap, max_cost, bgr, search=search)
        M, _, _, ok = state["al"](fr, prev=state["prev"])
        Ms.append(M), oks.append(ok)
        state["prev"] = fr[-1:].clone()

    chunk, done = [], 0
    for fr in frames:
        if done + len(chunk) >= len(cm):
            raise ValueError(f"track_game: more frames than the {len(cm)} predictions")
        a = np.frombuffer(fr, np.uint8) if isinstance(fr, (bytes, bytearray, memoryview)) else np.asarray(fr)
        if frames_format != "array":
            if a.dtype != np.uint8 or a.ndim != 1:
                raise ValueError(f"track_game: with frames_format={frames_format!r} a frame is the bytes of a {frames_format.upper()} "
                                 f"file, got {a.dtype} {a.shape}")
        elif a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or (chunk and a.shape != chunk[0].shape):
            raise ValueError(f"track_game: frames must be uint8 (H,W,3) arrays of one size, got {a.dtype} {a.shape}")
        chunk.append(a)
        if len(chunk) == batch:
            flush(chunk)
            done += len(chunk)
            chunk = []
    if chunk:
        flush(chunk)
        done += len(chunk)
    if done != len(cm):
        raise ValueError(f"track_game: {done} frames for {len(cm)} predictions")
    F = len(cm)
    theta = tabs["theta"].reshape(F, 1, 3, 3).contiguous()
    M, ok = torch.cat(Ms).contiguous(), torch.cat(oks).contiguous()      # F - 1 rows: the first batch has no prev
    score = tabs["scores"] if max_score is not None else None
    extra = {}
    if smooth_radius is None:
        theta2, source = propagate_theta(theta, M, ok, score=score, max_score=max_score, max_gap=max_gap)
        theta2, source = theta2.cpu().numpy(), source.cpu().numpy()
    else:
        theta2, stats, members = smooth_theta(theta, M, ok, score=score, max_score=max_score, radius=smooth_radius,
                                              iters=smooth_iters, delta=smooth_delta, min_members=smooth_min_members)
        theta2, stats, members = theta2.cpu().numpy(), stats.cpu().numpy(), members.cpu().numpy()
        source = np.where(np.isfinite(theta2.reshape(F, 9)).all(axis=1), np.arange(F), -1)
        null = lambda v: float(v) if math.isfinite(v) else None
        extra = {"members": [int(m) for m in members], "spread": [null(v) for v in stats[:, 1]],
                 "deviation": [null(v) for v in stats[:, 2]]}
    with open(court_json, "r") as f:
        raw = json.load(f)
    for k, name in enumerate(cm.names):
        raw[name]["theta"] = theta2[k].tolist()
        raw[name]["source"] = int(source[k])
        for key, vals in extra.items():
            raw[name][key] = vals[k]
    os.makedirs(os.path.dirname(os.path.abspath(dst_json)), exist_ok=True)
    with open(dst_json, "w") as f:
        json.dump(raw, f, indent=2)
    return dst_json
