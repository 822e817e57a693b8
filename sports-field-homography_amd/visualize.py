"""Court overlay frames on the HIP path: the reference's ``viz_preds.py`` (:78-152) with ``utils/postprocess.py:21-71``.

    r = OverlayRenderer(court_img, mask_classes=4, score_threshold=0.17, marker_radius=3)
    out = r(frames_u8, theta, score=score, segm=logits, poi=poi, labels=['{:4f}'.format(s) for s in scores])

Per frame the class-id mask is the court template re-warped with the frame's theta (``score < score_threshold``,
viz_preds.py:120-125) or the segmentation mask (:128-132); it is coloured with the palette of ``outputs.format_masks``,
blended over the frame (``overlay``, postprocess.py:60-65: a black mask pixel keeps the frame, any other becomes
``(colour + frame) >> 1`` per channel - equal to the reference's float64 ``colour * 0.5 + frame * 0.5`` truncated to uint8
for every byte pair) and, optionally, POI markers and a label are stamped on it.  ``csrc/overlay.hip`` does this in at
most two launches per batch on the caller's current stream, with no synchronisation and no stock torch kernel.

Channel order: palette and colour tuples are written into the array as given, exactly as ``outputs.format_masks`` does.
The reference's frames are BGR (OpenCV), so (0,255,0) is green and (0,0,255) is red there; on RGB frames the same bytes
read green and blue.

Stated deviations from the reference:

* the label is drawn with the project's own 5x7 bitmap font (``GLYPHS``, the table of csrc/overlay.hip) at an integer
  scale, top-left at ``label_pos``.  The reference calls ``cv2.putText`` with OpenCV's Hershey font, which does not exist
  here and cannot be pinned, so label pixels are not comparable with the reference's;
* markers are filled discs ``dx^2 + dy^2 <= r^2`` about ``(rint(x * W), rint(y * H))`` (predict.py:383's pixel rule) where
  predict.py:384 draws an OpenCV ring;
* viz_preds.py:143-145 has a precedence slip that calls ``overlay(frame, None)`` when there is no mask and an overlay
  threshold is set; here no mask means the frame is copied;
* overlapping drawings are deterministic: a later point index wins over an earlier one, the label is drawn last.

``visualize`` is the host driver of viz_preds.py:78-152 without ffmpeg: it writes ``dst_dir/<name>.png``.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import outputs as O
from . import pngdec
from ._codec import frames_from_files, image_files_from_batch, ptr as _ptr, stream as _stream

SOURCES = {s: _lib.ABI.defines["SFH_OVERLAY_" + s.upper()] for s in ("auto", "warp", "segm")}
LABEL_MAX = _lib.ABI.defines["SFH_OVERLAY_LABEL_MAX"]
LABEL_COLORS = ((0, 255, 0), (0, 0, 255))       # score < score_threshold, otherwise (viz_preds.py:125,127)
GLYPH_W, GLYPH_H, GLYPH_ADVANCE = 5, 7, 6
CHARSET = "0123456789.-+e naif"                 # glyph code = index
# one byte per glyph row, top row first, bit 4 = leftmost column: the table kGlyphs of csrc/overlay.hip
GLYPHS = (
    (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E),  # 0
    (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),  # 1
    (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),  # 2
    (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),  # 3
    (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02),  # 4
    (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),  # 5
    (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E),  # 6
    (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),  # 7
    (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),  # 8
    (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),  # 9
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C),  # .
    (0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00),  # -
    (0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00),  # +
    (0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E),  # e
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00),  # space
    (0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11),  # n
    (0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F),  # a
    (0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E),  # i
    (0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08),  # f
)


def encode_labels(labels, batch):
    """list of ``batch`` strings -> int8 (batch, L) glyph codes, -1 = end; a character outside CHARSET raises ValueError"""
    if len(labels) != batch:
        raise ValueError(f"labels: {len(labels)} strings for a batch of {batch}")
    L = max(1, max(len(s) for s in labels))
    if L > LABEL_MAX:
        raise ValueError(f"labels: {L} characters (at most {LABEL_MAX})")
    codes = np.full((batch, L), -1, dtype=np.int8)
    for b, s in enumerate(labels):
        for i, ch in enumerate(s):
            k = CHARSET.find(ch)
            if k < 0 or len(ch) != 1:
                raise ValueError(f"labels[{b}] = {s!r}: character {ch!r} is not in the overlay font ({CHARSET!r})")
            codes[b, i] = k
    return codes


class OverlayRenderer:
    def __init__(self, court_img, mask_classes=4, score_threshold=0.1, overlay_threshold=None, source="auto",
                 marker_radius=0, marker_color=(255, 255, 255), label_pos=(15, 15), label_scale=2):
        """court_img: the id template (N,1,Ht,Wt) float32 valued k / mask_classes (``synth.load_court_template`` /
        ``open_court_template``), any size, one image or one per frame; an ``expand``ed (non-contiguous) template is fine.
        source: "auto" (per frame from the score), "warp" or "segm" (every frame; no score needed).  marker_radius 0 = no
        markers.  label_pos = (x, y) of the label's top-left corner, label_scale = frame pixels per font pixel."""
        if source not in SOURCES:
            raise ValueError(f"source={source!r}: one of {sorted(SOURCES)}")
        if not isinstance(court_img, torch.Tensor) or court_img.dim() != 4 or court_img.shape[1] != 1 \
                or court_img.dtype != torch.float32:
            raise ValueError(f"court_img: expected a float32 tensor (N,1,Ht,Wt), got {tuple(getattr(court_img, 'shape', ()))}")
        if int(marker_radius) < 0:
            raise ValueError(f"marker_radius = {marker_radius}: negative")
        if int(label_scale) < 1:
            raise ValueError(f"label_scale = {label_scale}: at least 1")
        self.court_img = court_img
        self.mask_classes = int(mask_classes)
        self.palette = O._palette_bytes(self.mask_classes)       # NotImplementedError for a class count without a table
        self.score_threshold = float(score_threshold)
        self.overlay_threshold = None if overlay_threshold is None else float(overlay_threshold)
        self.source = source
        self.marker_radius = int(marker_radius)
        self.marker_color = np.asarray(marker_color, dtype=np.uint8).reshape(3).copy()
        self.label_pos = (int(label_pos[0]), int(label_pos[1]))
        self.label_scale = int(label_scale)
        self._tmpl = None        # (key, contiguous template on the device, shared?)

    def _template(self, dev):
        """the template as the kernel reads it: ONE image when every frame's is the same (reconstructor._template_is_shared's
        detection: asked once per template tensor), else (N,1,Ht,Wt) contiguous"""
        c = self.court_img
        key = (c.data_ptr(), tuple(c.shape), tuple(c.stride()), c._version, str(dev))
        if self._tmpl is None or self._tmpl[0] != key:
            from . import engine as E
            if c.device != dev:
                raise ValueError(f"court_img is on {c.device}, the frames on {dev}")
            shared = c.shape[0] == 1 or c.stride(0) == 0
            if not shared:
                c = c.contiguous()
                shared = bool(E.rows_all_equal(c))
            t = c[0:1].contiguous() if shared else c
            self._tmpl = (key, t, shared)
        return self._tmpl[1], self._tmpl[2]

    def __call__(self, frames_u8, theta, score=None, segm=None, poi=None, labels=None, out=None):
        """frames_u8 uint8 (B,H,W,3) on the GPU; theta (B,1,3,3)|(B,3,3) float32 (may be None for source="segm"); score (B,)
        float32 (needed for source="auto", for an overlay threshold; colours the label); segm: int32 / uint8 ids (B,hs,ws) or
        float32 logits (B,nc,hs,ws), any size, or None (frames on the segmentation leg are then copied); poi (B,N,2) float32
        in [0,1] as ``predict(project_poi=True)`` returns it; labels: list of B strings over CHARSET; out: a uint8 tensor
        like frames_u8, may BE frames_u8 (in place).  Returns out."""
        if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 \
                or frames_u8.shape[3] != 3:
            raise ValueError(f"frames_u8: expected a uint8 tensor (B,H,W,3), got {getattr(frames_u8, 'dtype', type(frames_u8))} "
                             f"{tuple(getattr(frames_u8, 'shape', ()))}")
        dev = frames_u8.device
        if dev.type != "cuda":
            raise RuntimeError(f"OverlayRenderer: device {dev} - the HIP path has no CPU fallback")
        if not frames_u8.is_contiguous():
            raise ValueError("frames_u8: expected a contiguous tensor")
        B, H, W = (int(v) for v in frames_u8.shape[:3])
        src = SOURCES[self.source]

        def dev_f32(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev:
                raise ValueError(f"{what}: expected a float32 tensor on {dev}")
            t = t.reshape(shape)
            if not t.is_contiguous():
                raise ValueError(f"{what}: expected a contiguous tensor")
            return t

        if score is not None:
            score = dev_f32(score, (B,), "score")
        elif src == 0 or self.overlay_threshold is not None:
            raise ValueError("OverlayRenderer: source='auto' and an overlay threshold need a score")
        tmpl, bstride, ht, wt = None, 0, 0, 0
        if src != 2:
            if theta is None:
                raise ValueError("OverlayRenderer: the warp leg needs theta")
            theta = dev_f32(theta, (B, 3, 3), "theta")
            tmpl, shared = self._template(dev)
            if not shared and tmpl.shape[0] < B:
                raise ValueError(f"batch {B} exceeds the court template batch {tmpl.shape[0]}")
            ht, wt = int(tmpl.shape[2]), int(tmpl.shape[3])
            bstride = 0 if shared else ht * wt
        else:
            theta = None
        kind = nc = hs = ws = 0
        if segm is not None and src != 1:
            if not isinstance(segm, torch.Tensor) or segm.device != dev or not segm.is_contiguous() or segm.shape[0] != B:
                raise ValueError(f"segm: expected a contiguous tensor on {dev} with batch {B}")
            if segm.dim() == 4 and segm.dtype == torch.float32:
                kind, nc, hs, ws = 2, int(segm.shape[1]), int(segm.shape[2]), int(segm.shape[3])
                if nc < 2:
                    raise NotImplementedError("single-channel (sigmoid) logits have no class-id mask")
            elif segm.dim() == 3 and segm.dtype in (torch.int32, torch.uint8):
                kind, nc, hs, ws = (0 if segm.dtype == torch.int32 else 1), self.mask_classes, int(segm.shape[1]), int(segm.shape[2])
            else:
                raise ValueError(f"segm: unsupported source {tuple(segm.shape)} {segm.dtype}")
        else:
            segm = None
        if out is None:
            out = torch.empty_like(frames_u8)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != frames_u8.shape or out.device != dev \
                or not out.is_contiguous():
            raise ValueError("out: expected a contiguous uint8 tensor like frames_u8")
        codes = None
        if labels is not None:
            codes = encode_labels(labels, B)
        if poi is not None:
            if not isinstance(poi, torch.Tensor) or poi.dtype != torch.float32 or poi.device != dev or poi.dim() != 3 \
                    or poi.shape[0] != B or poi.shape[2] != 2 or not poi.is_contiguous():
                raise ValueError(f"poi: expected a contiguous float32 tensor ({B},N,2) on {dev}")
        lib = _lib.load()
        with torch.cuda.device(dev):
            stp = _stream(dev)
            _lib.check(lib.sfh_overlay_render(_ptr(frames_u8), _ptr(out), B, H, W, _ptr(theta), _ptr(tmpl), bstride, ht, wt,
                                              float(self.mask_classes), _ptr(segm), kind, nc, hs, ws, _ptr(score),
                                              self.score_threshold, src, 0 if self.overlay_threshold is None else 1,
                                              self.overlay_threshold or 0.0, self.palette.ctypes.data, stp), "overlay_render")
            draw = poi is not None and self.marker_radius > 0
            if draw or codes is not None:
                codes_dev = None
                if codes is not None:
                    # one small asynchronous upload from a pinned staging buffer; the caching allocators of both sides keep
                    # the blocks alive until the stream has passed the copy
                    host = torch.from_numpy(codes).pin_memory()
                    codes_dev = torch.empty(codes.shape, dtype=torch.int8, device=dev)
                    codes_dev.copy_(host, non_blocking=True)
                _lib.check(lib.sfh_overlay_annotate(_ptr(out), B, H, W, _ptr(poi) if draw else None,
                                                    int(poi.shape[1]) if draw else 0, self.marker_radius,
                                                    self.marker_color.ctypes.data, _ptr(codes_dev),
                                                    codes.shape[1] if codes is not None else 0, self.label_pos[0],
                                                    self.label_pos[1], self.label_scale, _ptr(score), self.score_threshold, src,
                                                    stp), "overlay_annotate")
        return out


def _names_checked(names, pred_names, mask_names):
    """viz_preds.py:109: frame k, prediction k and mask k carry one name"""
    for k, (p, m) in enumerate(zip(pred_names, mask_names if mask_names is not None else pred_names)):
        if p != m:
            raise ValueError(f"visualize: prediction {k} is frame {p!r}, mask {k} is frame {m!r} - the two streams are not aligned")
    if names is not None:
        for k, (n, p) in enumerate(zip(names, pred_names)):
            if str(n) != str(p):
                raise ValueError(f"visualize: frame {k} is {n!r}, prediction {k} is {p!r} - frames and predictions are not aligned")


def visualize(frames, preds_path, dst_dir, court_img, masks_path=None, mask_classes=4, score_threshold=0.1,
              overlay_threshold=None, batch=16, names=None, renderer=None, device="cuda", png="host", image_format="png",
              jpeg_quality=90, frames_format="array", masks_decode="host", **renderer_kw):
    """viz_preds.py:78-152 without video decode and ffmpeg.  frames: an iterable of host uint8 (H,W,3) arrays in the order of
    the predictions (names: their frame names, checked against the predictions' when given; the reference asserts
    ``int(name) == frame number``); preds_path: a ``{game}_court.json`` (outputs.CourtJsonWriter); masks_path: the optional
    ``data.pkl`` mask stream (outputs.MaskPickleWriter) - without it frames on the segmentation leg are copied.  Renders in
    batches with the label ``'{:4f}'.format(score)`` and writes ``dst_dir/<name>.png`` (outputs.encode_png).  renderer: any
    callable with OverlayRenderer's call signature (default: an OverlayRenderer built from the arguments).  png: "host"
    (outputs.encode_png, the default) or "device" (sfh_amd.pngenc: the frames are encoded on the GPU).  image_format: "png",
    or "jpeg" for ``dst_dir/<name>.jpeg`` at jpeg_quality, what the reference's predict.py:394 writes (``png=`` then selects
    where the JPEG is encoded: outputs.encode_jpeg or sfh_amd.jpegenc, the same bytes).  frames_format: "array", or "jpeg" for
    an iterable of JPEG files as bytes, decoded on the GPU (sfh_amd.jpegdec) to the pixels PIL gives, or "png" for PNG files
    (sfh_amd.pngdec).  masks_decode: "host" (outputs.decode_png, the default) or "device" (the masks of a batch in one
    sfh_amd.pngdec decode: only the files are uploaded).  Returns the list of written paths."""
    if frames_format not in ("array", "jpeg", "png"):
        raise ValueError(f'visualize: frames_format={frames_format!r} ("array", "jpeg" or "png")')
    if masks_decode not in ("host", "device"):
        raise ValueError(f'visualize: masks_decode={masks_decode!r} ("host" or "device")')
    mapping, _ = O.load_court_mapping(preds_path)
    pred_names = list(mapping.keys())
    masks = None
    if masks_path is not None:
        reader = O.MaskReader(masks_path)
        masks = [buf for _, buf in reader.entries]
        _names_checked(names, pred_names, [n for n, _ in reader.entries])
        if len(masks) != len(pred_names):
            raise ValueError(f"visualize: {len(pred_names)} predictions, {len(masks)} masks")
    else:
        _names_checked(names, pred_names, None)
    if renderer is None:
        renderer = OverlayRenderer(court_img.to(device), mask_classes=mask_classes, score_threshold=score_threshold,
                                   overlay_threshold=overlay_threshold, **renderer_kw)
    os.makedirs(dst_dir, exist_ok=True)
    written = []

    def flush(chunk, first):
        B = len(chunk)
        if frames_format != "array":              # decoded on the GPU (sfh_amd.jpegdec, pngdec): only the files are uploaded
            fr = frames_from_files(chunk, device, frames_format)
        else:
            fr = torch.from_numpy(np.ascontiguousarray(np.stack(chunk))).to(device)
        keys = pred_names[first:first + B]
        theta = torch.tensor(np.stack([mapping[k][0] for k in keys]), dtype=torch.float32).reshape(B, 1, 3, 3).to(device)
        scores = [mapping[k][2] for k in keys]
        score = torch.tensor(scores, dtype=torch.float32).to(device)
        segm = None
        if masks is not None and masks_decode == "device":
            segm = pngdec.masks_from_files(masks[first:first + B], device)
        elif masks is not None:
            dec = [O.decode_png(m) for m in masks[first:first + B]]
            if any(d.ndim != 2 or d.shape != dec[0].shape for d in dec):
                raise ValueError("visualize: the mask stream must hold gray id masks of one size")
            segm = torch.from_numpy(np.ascontiguousarray(np.stack(dec))).to(device)
        out = renderer(fr, theta, score=score, segm=segm, labels=['{:4f}'.format(s) for s in scores])
        files, ext = image_files_from_batch(out, 3, png, image_format, jpeg_quality)
        for k, buf in zip(keys, files):
            path = os.path.join(dst_dir, f"{k}.{ext}")
            with open(path, "wb") as f:
                f.write(buf.tobytes())
            written.append(path)

    chunk, done = [], 0
    for fr in frames:
        if done + len(chunk) >= len(pred_names):
            raise ValueError(f"visualize: more frames than the {len(pred_names)} predictions")
        a = np.frombuffer(fr, np.uint8) if isinstance(fr, (bytes, bytearray, memoryview)) else np.asarray(fr)
        if frames_format != "array":
            if a.dtype != np.uint8 or a.ndim != 1:
                raise ValueError(f"visualize: with frames_format={frames_format!r} a frame is the bytes of a {frames_format.upper()} "
                                 f"file, got {a.dtype} {a.shape}")
        elif a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or (chunk and a.shape != chunk[0].shape):
            raise ValueError(f"visualize: frames must be uint8 (H,W,3) arrays of one size, got {a.dtype} {a.shape}")
        chunk.append(a)
        if len(chunk) == batch:
            flush(chunk, done)
            done += len(chunk)
            chunk = []
    if chunk:
        flush(chunk, done)
        done += len(chunk)
    if done != len(pred_names):
        raise ValueError(f"visualize: {done} frames for {len(pred_names)} predictions")
    return written
