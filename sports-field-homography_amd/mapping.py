"""Frame <-> court mapping and top-view rectification on the HIP path: the reference's ``utils/transform.py``,
``utils/court.py`` and ``utils/mapping_example.py``.

    cm = CourtMapping("game_court.json")                     # or CourtMapping(theta, scores=..., names=...)
    mapper = FrameCourtMapper(cm)
    court_m = mapper.frame_to_court(tracks_px, frame_index, frame_size=(1280, 720), units="meters")
    frame_px = mapper.court_to_frame(court_poi, frame_index, frame_size=(1280, 720))

    top = TopViewRenderer(out_size=(1280, 720))(frames_u8, theta)["top_view"]      # the frames seen from above the court
    mosaic = CourtMosaic((1280, 720)); mosaic.add(frames_u8, theta); image, count = mosaic.result()

``theta`` is frame -> court in the model's convention (``Reconstructor.warp`` samples the court template into the frame with
it); its inverse ``theta_c2f`` samples the frame into the court view and maps court points into the frame.  ``csrc/mapping.hip``
does each of these in one launch on the caller's current stream (a top view: two, invert and render), with no synchronisation
and no stock torch kernel.

Stated deviations from the reference:

* ``Warper.warp`` (utils/transform.py:8-20) runs Kornia's nearest warp in fp64.  The top view here uses the pinned fp32
  coordinate arithmetic of ``Reconstructor.warp()`` (csrc/warp_coords.h), so a top view and a warped court mask agree on
  geometry tap for tap.
* ``CourtMapping`` inverts with ``sfh_theta_invert`` (fp64 adjugate rule, rounded to fp32: the matrix ``transform_poi``
  applies) where utils/court.py:43 calls ``np.linalg.inv``; a singular or non-finite theta gives status 0 instead of raising.
* points: ``cv2.perspectiveTransform`` rounds to float32 before ``/ 2 + 0.5``; ``sfh_map_points`` carries fp64 to the end and
  rounds once.  Drawing markers on the court image (mapping_example.py's ``cv2.circle``) is not reproduced.
"""
import os

import numpy as np
import torch

from . import _lib
from . import outputs as O
from ._codec import frames_from_files, image_files_from_batch, ptr as _ptr, stream as _stream

MODES = {"nearest": 0, "bilinear": 1}


class CourtSizes:
    """utils/court.py:6-17: the constants of the court dimensions"""
    COURT_IN_PIXELS = (1280, 720)
    FRAME_IN_PIXELS = (1280, 720)
    COURT_IN_METERS = (32.2326, 17.145)
    METERS2FEET = 3.28084
    METERS2PIXELS = (COURT_IN_PIXELS[0] / COURT_IN_METERS[0],
                     COURT_IN_PIXELS[1] / COURT_IN_METERS[1])
    PIXELS2METERS = (COURT_IN_METERS[0] / COURT_IN_PIXELS[0],
                     COURT_IN_METERS[1] / COURT_IN_PIXELS[1])


# frame_to_court's units -> scale of the court's unit square
UNITS = {
    "norm": (1.0, 1.0),
    "pixels": (float(CourtSizes.COURT_IN_PIXELS[0]), float(CourtSizes.COURT_IN_PIXELS[1])),
    "meters": CourtSizes.COURT_IN_METERS,
    "feet": (CourtSizes.COURT_IN_METERS[0] * CourtSizes.METERS2FEET, CourtSizes.COURT_IN_METERS[1] * CourtSizes.METERS2FEET),
}


def _need_gpu(t, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: device {t.device} - the HIP path has no CPU fallback")


def _theta33(theta, B, dev):
    _need_gpu(theta, "theta")
    if theta.dtype != torch.float32 or theta.device != dev or theta.numel() != B * 9:
        raise ValueError(f"theta: expected a float32 tensor ({B},3,3) or ({B},1,3,3) on {dev}, got {theta.dtype} "
                         f"{tuple(theta.shape)} on {theta.device}")
    theta = theta.reshape(B, 3, 3)
    if not theta.is_contiguous():
        raise ValueError("theta: expected a contiguous tensor")
    return theta


def _frames_checked(frames_u8, what):
    _need_gpu(frames_u8, what)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"{what}: expected a uint8 tensor (B,H,W,3), got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    if not frames_u8.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous tensor")
    return tuple(int(v) for v in frames_u8.shape[:3])


def _score_checked(score, max_score, B, dev):
    """-> (score tensor or None, max_score float): the gate is on only with both"""
    if max_score is None or score is None:
        return None, 0.0
    _need_gpu(score, "score")
    if score.dtype != torch.float32 or score.device != dev or score.numel() != B or not score.is_contiguous():
        raise ValueError(f"score: expected a contiguous float32 tensor ({B},) on {dev}")
    return score, float(max_score)


def invert_theta(theta, out=None, status=None):
    """theta (B,3,3)|(B,1,3,3) float32 on the GPU -> (theta_c2f (B,3,3) float32, status (B,) uint8); one launch."""
    _need_gpu(theta, "theta")
    B = theta.numel() // 9
    dev = theta.device
    theta = _theta33(theta, B, dev)
    if out is None:
        out = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    if status is None:
        status = torch.empty((B,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sfh_theta_invert(_ptr(theta), B, _ptr(out), _ptr(status), _stream(dev)), "theta_invert")
    return out, status


class CourtMapping:
    """utils/court.py:20-45: the per-frame homographies of a game.  Built from a ``*_court.json`` path
    (outputs.load_court_mapping) or from ``theta`` (F,3,3)|(F,1,3,3) with optional ``scores`` (F,) and ``names`` (F strings).
    The host arrays (``theta``, ``scores``, ``names``, ``rows``: name -> row) exist without a GPU; ``tables(device)`` uploads
    them once and inverts on the device: ``{"theta", "theta_c2f", "status", "scores"}``."""

    def __init__(self, source, scores=None, names=None, device="cuda"):
        self.model = None
        if isinstance(source, (str, os.PathLike)):
            frames, self.model = O.load_court_mapping(source)
            names = list(frames.keys())
            theta = np.stack([frames[k][0] for k in names]) if names else np.zeros((0, 3, 3))
            scores = [frames[k][2] for k in names]
        else:
            theta = source.detach().cpu().numpy() if isinstance(source, torch.Tensor) else np.asarray(source)
        if theta.size == 0 or theta.size % 9:
            raise ValueError(f"CourtMapping: theta of shape {tuple(theta.shape)} is not (F,3,3) with F >= 1")
        self.theta = np.ascontiguousarray(theta.reshape(-1, 3, 3), dtype=np.float32)
        F = self.theta.shape[0]
        if scores is None:
            self.scores = np.zeros((F,), dtype=np.float32)
        else:
            s = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
            self.scores = np.ascontiguousarray(s.reshape(-1), dtype=np.float32)
        if self.scores.shape[0] != F:
            raise ValueError(f"CourtMapping: {self.scores.shape[0]} scores for {F} frames")
        self.names = [str(n) for n in names] if names is not None else [str(k) for k in range(F)]
        if len(self.names) != F:
            raise ValueError(f"CourtMapping: {len(self.names)} names for {F} frames")
        self.rows = {n: k for k, n in enumerate(self.names)}
        if len(self.rows) != F:
            raise ValueError("CourtMapping: frame names are not unique")
        self.device = torch.device(device)
        self._tables = None

    def __len__(self):
        return self.theta.shape[0]

    def row(self, name):
        return self.rows[str(name)]

    def tables(self, device=None):
        dev = torch.device(device) if device is not None else self.device
        if dev.type != "cuda":
            raise RuntimeError(f"CourtMapping: device {dev} - the HIP path has no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._tables is None or self._tables["theta"].device != dev:
            theta = torch.from_numpy(self.theta).to(dev)
            c2f, status = invert_theta(theta)
            self._tables = {"theta": theta, "theta_c2f": c2f, "status": status, "scores": torch.from_numpy(self.scores).to(dev)}
        return self._tables


class FrameCourtMapper:
    """map_frame_to_court / map_court_to_frame (utils/transform.py:33-54) for arbitrary points of arbitrary frames of a
    CourtMapping: one launch per call, whatever the number of points."""

    def __init__(self, mapping):
        if not isinstance(mapping, CourtMapping):
            raise ValueError("FrameCourtMapper: expected a CourtMapping")
        self.mapping = mapping

    def _map(self, points, frame_index, table, in_size, out_scale, what):
        _need_gpu(points, what)
        dev = points.device
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 2 or not points.is_contiguous() \
                or points.shape[0] == 0:
            raise ValueError(f"{what}: expected a contiguous float32 tensor (N,2) with N >= 1, got {points.dtype} {tuple(points.shape)}")
        N = int(points.shape[0])
        tabs = self.mapping.tables(dev)
        idx, frame0 = None, 0
        if isinstance(frame_index, torch.Tensor):
            _need_gpu(frame_index, "frame_index")
            if frame_index.dtype != torch.int32 or frame_index.device != dev or frame_index.shape != (N,) \
                    or not frame_index.is_contiguous():
                raise ValueError(f"frame_index: expected a contiguous int32 tensor ({N},) on {dev}, or one int / frame name")
            idx = frame_index
        elif isinstance(frame_index, str):
            frame0 = self.mapping.row(frame_index)
        else:
            frame0 = int(frame_index)
        in_w, in_h = (0.0, 0.0) if in_size is None else (float(np.float32(in_size[0])), float(np.float32(in_size[1])))
        out = torch.empty((N, 2), dtype=torch.float32, device=dev)
        flag = torch.empty((N,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sfh_map_points(_ptr(points), _ptr(idx), frame0, N, _ptr(tabs[table]), len(self.mapping),
                                                  in_w, in_h, float(out_scale[0]), float(out_scale[1]), _ptr(out), _ptr(flag),
                                                  _stream(dev)), "map_points")
        return out, flag

    def frame_to_court(self, points_px, frame_index, frame_size=None, units="norm"):
        """points_px (N,2) float32 on the GPU in frame pixels of ``frame_size`` = (w, h) (None: already normalised to
        [-1,1]); frame_index: int32 (N,) on the GPU, or one row / frame name for every point.  Returns (out (N,2) float32,
        flag (N,) uint8): court coordinates in ``units`` - "norm" the unit square of map_frame_to_court, "pixels"
        (x CourtSizes.COURT_IN_PIXELS), "meters", "feet"; flag 0 (out 0) where the point could not be mapped."""
        if units not in UNITS:
            raise ValueError(f"units={units!r}: one of {sorted(UNITS)}")
        return self._map(points_px, frame_index, "theta", frame_size, UNITS[units], "points_px")

    def court_to_frame(self, points, frame_index, court_size=None, frame_size=None):
        """points (N,2) float32 on the GPU in court pixels of ``court_size`` = (w, h) (None: normalised to [-1,1], as
        load_court_poi gives them) -> (out, flag): frame coordinates in the unit square, or in pixels of ``frame_size``."""
        return self._map(points, frame_index, "theta_c2f", court_size, (1.0, 1.0) if frame_size is None else frame_size, "points")


class TopViewRenderer:
    """``Warper.warp(theta_c2f, frame)`` of utils/transform.py for a batch of uint8 frames: two launches (invert, render),
    output buffers reused across calls (copy what must outlive the next call)."""

    def __init__(self, out_size=(1280, 720), mode="nearest", max_score=None):
        if mode not in MODES:
            raise ValueError(f"mode={mode!r}: one of {sorted(MODES)}")
        self.out_size = (int(out_size[0]), int(out_size[1]))
        if min(self.out_size) < 2:
            raise ValueError(f"out_size = {out_size}: at least 2 x 2")
        self.mode = mode
        self.max_score = None if max_score is None else float(max_score)
        self._buf = None

    def _buffers(self, B, dev):
        if self._buf is None or self._buf[0] != (B, str(dev)):
            wc, hc = self.out_size
            self._buf = ((B, str(dev)), torch.empty((B, hc, wc, 3), dtype=torch.uint8, device=dev),
                         torch.empty((B, hc, wc), dtype=torch.uint8, device=dev),
                         torch.empty((B, 3, 3), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.uint8, device=dev))
        return self._buf[1:]

    def __call__(self, frames_u8, theta, score=None, out=None):
        """frames_u8 uint8 (B,H,W,3) on the GPU; theta (B,3,3)|(B,1,3,3) float32 frame -> court; score (B,) float32: with
        ``max_score`` set, a frame whose score is NaN or above it comes back as zeros (decided on the device).  out: a dict of
        ``top_view`` / ``valid`` tensors to write into instead of the renderer's own buffers.  Returns {"top_view" uint8
        (B,hc,wc,3), "valid" uint8 (B,hc,wc) 255 / 0, "status" uint8 (B,), "theta_c2f" float32 (B,3,3)}."""
        B, H, W = _frames_checked(frames_u8, "frames_u8")
        dev = frames_u8.device
        theta = _theta33(theta, B, dev)
        score, max_score = _score_checked(score, self.max_score, B, dev)
        top, valid, c2f, status = self._buffers(B, dev)
        if out is not None:
            top, valid = out["top_view"], out["valid"]
        wc, hc = self.out_size
        lib = _lib.load()
        with torch.cuda.device(dev):
            stp = _stream(dev)
            _lib.check(lib.sfh_theta_invert(_ptr(theta), B, _ptr(c2f), _ptr(status), stp), "theta_invert")
            _lib.check(lib.sfh_topview_render(_ptr(frames_u8), B, H, W, _ptr(c2f), _ptr(status), _ptr(score), max_score, hc, wc,
                                              MODES[self.mode], _ptr(top), _ptr(valid), stp), "topview_render")
        return {"top_view": top, "valid": valid, "status": status, "theta_c2f": c2f}


class CourtMosaic:
    """The court seen through a whole clip: per court pixel the mean of the nearest frame taps over every used frame, in
    integers (uint32 sums; a pixel may collect fewer than 2^32 / 255 frames).  ``add`` is two launches (invert,
    accumulate); the rectified frames are never written."""

    def __init__(self, out_size=(1280, 720), max_score=None):
        self.out_size = (int(out_size[0]), int(out_size[1]))
        if min(self.out_size) < 2:
            raise ValueError(f"out_size = {out_size}: at least 2 x 2")
        self.max_score = None if max_score is None else float(max_score)
        self.sum = self.count = None

    def _state(self, dev):
        if self.sum is None:
            wc, hc = self.out_size
            # int32 storage of the kernels' uint32 words
            self.sum = torch.zeros((hc, wc, 3), dtype=torch.int32, device=dev)
            self.count = torch.zeros((hc, wc), dtype=torch.int32, device=dev)
        elif self.sum.device != dev:
            raise ValueError(f"CourtMosaic: accumulators are on {self.sum.device}, the frames on {dev}")

    def add(self, frames_u8, theta, score=None):
        B, H, W = _frames_checked(frames_u8, "frames_u8")
        dev = frames_u8.device
        theta = _theta33(theta, B, dev)
        score, max_score = _score_checked(score, self.max_score, B, dev)
        self._state(dev)
        c2f, status = invert_theta(theta)
        wc, hc = self.out_size
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sfh_topview_accumulate(_ptr(frames_u8), B, H, W, _ptr(c2f), _ptr(status), _ptr(score),
                                                          max_score, hc, wc, _ptr(self.sum), _ptr(self.count), _stream(dev)),
                       "topview_accumulate")
        return self

    def result(self):
        """-> (image uint8 (hc,wc,3), count int32 (hc,wc)): the rounded mean, 0 where no frame saw the pixel"""
        if self.sum is None:
            raise RuntimeError("CourtMosaic.result: nothing was added (the HIP path has no CPU fallback)")
        dev = self.sum.device
        wc, hc = self.out_size
        image = torch.empty((hc, wc, 3), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sfh_topview_finish(_ptr(self.sum), _ptr(self.count), hc, wc, _ptr(image), _stream(dev)),
                       "topview_finish")
        return image, self.count

    def reset(self):
        if self.sum is not None:
            self.sum.zero_()
            self.count.zero_()


def rectify_game(court_json, frames, dst_dir, out_size=(1280, 720), mode="nearest", max_score=None, batch=16, names=None,
                 mosaic=True, device="cuda", png="host", image_format="png", jpeg_quality=90,
                 frames_format="array"):
    """The host driver, in the style of ``visualize.visualize``: frames - an iterable of host uint8 (H,W,3) arrays in the
    order of the predictions of ``court_json`` (names: their frame names, checked when given).  Writes
    ``dst_dir/<name>.png`` (outputs.encode_png), the top view of every frame, and ``dst_dir/mosaic.png``.  png: "host"
    (outputs.encode_png, the default) or "device" (sfh_amd.pngenc: the views are encoded on the GPU).  image_format: "png",
    or "jpeg" for ``<name>.jpeg`` and ``mosaic.jpeg`` at jpeg_quality (``png=`` then selects where the JPEG is encoded:
    outputs.encode_jpeg or sfh_amd.jpegenc, the same bytes).  frames_format: "array", or "jpeg" for an iterable of JPEG files as
    bytes, decoded on the GPU (sfh_amd.jpegdec) to the pixels PIL gives, or "png" for PNG files (sfh_amd.pngdec).  Returns the
    list of written paths."""
    if frames_format not in ("array", "jpeg", "png"):
        raise ValueError(f'rectify_game: frames_format={frames_format!r} ("array", "jpeg" or "png")')
    cm = CourtMapping(court_json, device=device)
    if names is not None:
        for k, (n, p) in enumerate(zip(names, cm.names)):
            if str(n) != p:
                raise ValueError(f"rectify_game: frame {k} is {n!r}, prediction {k} is {p!r} - frames and predictions are not aligned")
    renderer = TopViewRenderer(out_size, mode, max_score)
    mos = CourtMosaic(out_size, max_score) if mosaic else None
    tabs = cm.tables(device)
    os.makedirs(dst_dir, exist_ok=True)
    written = []

    def save(path, buf):
        with open(path, "wb") as f:
            f.write(buf.tobytes())
        written.append(path)

    def flush(chunk, first):
        B = len(chunk)
        if frames_format != "array":              # decoded on the GPU (sfh_amd.jpegdec, pngdec): only the files are uploaded
            fr = frames_from_files(chunk, tabs["theta"].device, frames_format)
        else:
            fr = torch.from_numpy(np.ascontiguousarray(np.stack(chunk))).to(tabs["theta"].device)
        theta, score = tabs["theta"][first:first + B], tabs["scores"][first:first + B]
        out = renderer(fr, theta, score=score)
        if mos is not None:
            mos.add(fr, theta, score=score)
        files, ext = image_files_from_batch(out["top_view"], 3, png, image_format, jpeg_quality)
        for k, buf in zip(cm.names[first:first + B], files):
            save(os.path.join(dst_dir, f"{k}.{ext}"), buf)

    chunk, done = [], 0
    for fr in frames:
        if done + len(chunk) >= len(cm):
            raise ValueError(f"rectify_game: more frames than the {len(cm)} predictions")
        a = np.frombuffer(fr, np.uint8) if isinstance(fr, (bytes, bytearray, memoryview)) else np.asarray(fr)
        if frames_format != "array":
            if a.dtype != np.uint8 or a.ndim != 1:
                raise ValueError(f"rectify_game: with frames_format={frames_format!r} a frame is the bytes of a {frames_format.upper()} "
                                 f"file, got {a.dtype} {a.shape}")
        elif a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or (chunk and a.shape != chunk[0].shape):
            raise ValueError(f"rectify_game: frames must be uint8 (H,W,3) arrays of one size, got {a.dtype} {a.shape}")
        chunk.append(a)
        if len(chunk) == batch:
            flush(chunk, done)
            done += len(chunk)
            chunk = []
    if chunk:
        flush(chunk, done)
        done += len(chunk)
    if done != len(cm):
        raise ValueError(f"rectify_game: {done} frames for {len(cm)} predictions")
    if mos is not None and done:
        files, ext = image_files_from_batch(mos.result()[0][None], 3, png, image_format, jpeg_quality)
        save(os.path.join(dst_dir, f"mosaic.{ext}"), files[0])
    return written
