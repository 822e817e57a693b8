"""Training labels from manual POI annotations on the HIP path: the reference's ``dataset_utils/preparation.py``
(annotations -> homography -> projected POI -> reprojection RMSE -> mask from template and homography -> one-hot masks),
which runs OpenCV on the CPU one frame at a time.

    lm = LabelMaker(court_ids, court_poi, size=(640, 360), num_classes=4)
    labels = lm.make(manual_poi)                       # (B,N,2) in [0,1], (-1,-1) = missing -> dict of device tensors
    batch, dropped = to_batch(labels, frames_u8, names)     # what BatchAugment, TrainStep and eval_reconstructor take

``csrc/prepare.hip`` does a batch in two launches (``sfh_prep_fit``, ``sfh_prep_render``) on the caller's current stream,
with no synchronisation and no stock torch kernel between them when ``manual_poi`` is float64 (host array or device tensor).

The rule of the fit (``cv2.findHomography(from, to)`` with the default method is a Hartley-normalised DLT through the 9 x 9
``L^T L`` followed by a Levenberg-Marquardt polish of the geometric error; OpenCV is not available here and cannot be
pinned, so the rule is stated and pinned by the numpy restatement ``tests/prep_ref.py``), everything in fp64:

1. both point sets are normalised: centroid to the origin, mean distance sqrt(2);
2. ``L^T L`` is accumulated over the usable points (manual x != -1 and y != -1: ``calculate_homography``'s test; the ignore
   list does not enter the fit, it only clears validity flags, as in the reference);
3. the eigenvector of its smallest eigenvalue by 12 cyclic Jacobi sweeps;
4. denormalised and divided by h33;
5. ``refine`` damped Gauss-Newton steps on the 8 free parameters against the summed squared forward reprojection error
   (in normalised frame coordinates); a step is accepted only if it lowers that cost, so the result is never worse than
   the DLT start.  ``refine=0`` returns the DLT.

Sums over points run in a fixed order (slot = index mod 64, slots combined by the butterfly 32, 16, .. 1); no atomics.

The rule of the render: a label pixel is the court id image at exactly the tap of ``Reconstructor.warp()``'s nearest warp
(``oracle/warp_ref.py``: individually rounded fp32, round-half-even, zero outside), for ``theta`` = the fp64 label rounded
once to fp32.

Stated deviations from the reference:

* the reference does not contain the step that writes the UV file.  Here a UV label is uint16 ``(id, u, v)`` per pixel
  with ``u = u_tab[tap x]``, ``v = v_tab[tap y]`` and the tables ``rint(generate_uv_template * 65535)``, so that
  ``preprocess_uv_mask``'s ``/ 65535`` returns the template value to within 0.5 / 65535;
* ``generate_uv_template`` zeroes u AND v outside the offset window; with the two separable tables a tap outside the
  window on one axis only keeps the other axis' value (with zero offsets: the last template column and row);
* the UV label is written as ``<name>.npy`` (uint16 (H,W,3)) by default; ``uv_format="tif"`` / ``"both"`` writes the 16-bit
  ``<name>.tif`` the reference's ``BasicDataset(use_uv=True)`` looks for (``sfh_amd.tiffenc`` / ``outputs.encode_tiff``: LZW,
  predictor 2, stored (v, u, id) so that ``cv2.imread(path, -1)`` returns the id in channel 0).  OpenCV is not available here:
  that its reader swaps the channels of a TIFF is stated from knowledge of its source, not verified;
* frames with fewer than 4 usable points (the reference's ``return None``) get status 0 and are reported, never written.
"""
import json
import os

import numpy as np
import torch

from . import _lib
from . import outputs as O
from ._codec import ptr as _ptr, stream as _stream
from .pngenc import files_from_batch

FOOTBALL_PITCH_IGNORE_POINTS = (12, 13, 16, 19, 20)      # dataset_utils/preparation.py:27
MAX_VALUE_UINT16 = 65535
MAX_POINTS = _lib.ABI.defines["SFH_PREP_MAX_POINTS"]


# ---------------------------------------------------------------------------------------------- host helpers
def uv_tables(size, x_offset=(0, 0), y_offset=(0, 0)):
    """(W,H) -> u_tab uint16 (W,), v_tab uint16 (H,): generate_uv_template's float32 linspace (utils/court.py:102-128:
    1/n .. 1, zero outside [offset[0], n - offset[1] - 1)) times 65535, rounded half to even."""
    W, H = int(size[0]), int(size[1])
    if W < 2 or H < 2:
        raise ValueError(f"uv_tables: size {size!r}")
    out = []
    for n, off in ((W, x_offset), (H, y_offset)):
        lo, hi = int(off[0]), n - int(off[1]) - 1
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"uv_tables: offset {tuple(off)!r} leaves no window in {n}")
        g = np.linspace(1.0 / n, 1, num=n, dtype=np.float32)
        t = np.zeros(n, dtype=np.float32)
        t[lo:hi] = g[lo:hi]
        out.append(np.rint(t.astype(np.float64) * MAX_VALUE_UINT16).astype(np.uint16))
    return out[0], out[1]


def rescale_theta(src_size, dst_size, theta):
    """dataset_utils/preparation.py:129-137 in fp64: diag(dst_w, dst_h, 1) @ theta @ diag(1/src_w, 1/src_h, 1)"""
    src_w, src_h = src_size
    dst_w, dst_h = dst_size
    a = np.array([[dst_w, 0, 0], [0, dst_h, 0], [0, 0, 1]], dtype=np.float64)
    b = np.array([[1 / src_w, 0, 0], [0, 1 / src_h, 0], [0, 0, 1]], dtype=np.float64)
    return np.matmul(np.matmul(a, np.asarray(theta, dtype=np.float64)), b)


def preprocess_weight(reproj_mse):
    """utils/dataset.py:197-209: the per-sample loss weight, a falling sigmoid of the reprojection error; float32, the
    shape of the argument"""
    x = np.asarray(reproj_mse, dtype=np.float64) / 0.01
    x = x * 12 - 6
    x = x * 1.25 + 1
    y = 1 - 1 / (1 + np.exp(-x))
    return np.asarray(y, dtype=np.float32)


def generate_requests(anno_dir):
    """dataset_utils/preparation.py:38-66: {game: {frame id: manual poi (N,2) float64}} from <anno_dir>/<game>/manual_anno.json"""
    requests = {}
    for name in sorted(n for n in os.listdir(anno_dir) if os.path.isdir(os.path.join(anno_dir, n))):
        with open(os.path.join(anno_dir, name, "manual_anno.json"), "r") as f:
            game = json.load(f)
        requests[name] = {fid: np.asarray(v["poi"], dtype=np.float64) for fid, v in game.items()}
    return requests


def _ignore_mask(ignore_pts, npts):
    m = np.zeros(npts, dtype=np.uint8)
    for i in (ignore_pts or ()):
        if not 0 <= int(i) < npts:
            raise ValueError(f"ignore_pts: index {i} outside the {npts} points")
        m[int(i)] = 1
    return m


# ---------------------------------------------------------------------------------------------- device
class LabelMaker:
    def __init__(self, court_ids, court_poi, size, num_classes, uv=False, ignore_pts=None, refine=10, norm_size=None,
                 uv_offsets=((0, 0), (0, 0)), device="cuda"):
        """court_ids: the id image uint8 (Hs,Ws) (``data/court_ids_*.npy``); court_poi (N,2) | (1,N,2) in [-1,1]
        (``synth.load_court_poi`` / ``open_court_poi``); size = (W,H) of the labels, W a multiple of 4; num_classes 4, 7 or
        8; ignore_pts: point indices whose validity flag is cleared (FOOTBALL_PITCH_IGNORE_POINTS); norm_size (w,h): the
        reprojection error is measured after scaling both point sets by it (None: in [0,1] units); uv_offsets = (x_offset,
        y_offset) of ``uv_tables``.  Nothing here touches a device: tensors are uploaded at the first call."""
        ids = court_ids.cpu().numpy() if isinstance(court_ids, torch.Tensor) else np.asarray(court_ids)
        if ids.dtype != np.uint8 or ids.ndim != 2:
            raise ValueError(f"court_ids: expected a uint8 image (Hs,Ws), got {ids.dtype} {ids.shape}")
        O._palette_bytes(int(num_classes))        # NotImplementedError for a class count without a table
        if int(ids.max()) >= int(num_classes):
            raise ValueError(f"court_ids holds id {int(ids.max())}, num_classes = {num_classes}")
        poi = court_poi.cpu().numpy() if isinstance(court_poi, torch.Tensor) else np.asarray(court_poi)
        poi = np.asarray(poi, dtype=np.float64)
        if poi.ndim == 3:
            poi = poi[0]
        if poi.ndim != 2 or poi.shape[1] != 2 or not 4 <= poi.shape[0] <= MAX_POINTS:
            raise ValueError(f"court_poi: expected (N,2) with 4 <= N <= {MAX_POINTS}, got {poi.shape}")
        self.W, self.H = int(size[0]), int(size[1])
        if self.W < 4 or self.H < 2 or self.W % 4:
            raise ValueError(f"size {size!r}: the width must be a multiple of 4")
        if int(refine) < 0:
            raise ValueError(f"refine = {refine}: negative")
        self.court_ids = np.ascontiguousarray(ids)
        self.court_poi = np.ascontiguousarray(poi)
        self.npts = int(poi.shape[0])
        self.num_classes = int(num_classes)
        self.uv = bool(uv)
        self.ignore = _ignore_mask(ignore_pts, self.npts)
        self.refine = int(refine)
        self.norm_size = (1.0, 1.0) if norm_size is None else (float(norm_size[0]), float(norm_size[1]))
        self.u_tab, self.v_tab = uv_tables((ids.shape[1], ids.shape[0]), uv_offsets[0], uv_offsets[1])
        self.device = torch.device(device)
        self._dev = None

    def _tensors(self):
        if self._dev is None:
            if self.device.type != "cuda":
                raise RuntimeError(f"LabelMaker: device {self.device} - the HIP path has no CPU fallback")
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            self._dev = {k: torch.from_numpy(v).to(self.device) for k, v in
                         (("ids", self.court_ids), ("poi", self.court_poi), ("ignore", self.ignore),
                          ("u", self.u_tab), ("v", self.v_tab))}
        return self._dev

    def fit(self, manual_poi, refine=None):
        """manual_poi (B,N,2) in [0,1], (-1,-1) = missing: a float64 host array or device tensor (anything else is
        converted first) -> dict of device tensors: theta_c2f, theta (B,3,3) fp64, theta_f32 (B,3,3), poi (B,N,3) fp64,
        num_nonzero (B,) int32, reproj_mse (B,) fp64, status (B,) int32 (0: fewer than 4 usable points, the rest zero)."""
        d = self._tensors()
        dev = self.device
        if isinstance(manual_poi, torch.Tensor):
            m = manual_poi.to(device=dev, dtype=torch.float64).contiguous()
        else:
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(manual_poi, dtype=np.float64))).to(dev)
        if m.dim() != 3 or m.shape[1] != self.npts or m.shape[2] != 2 or m.shape[0] < 1:
            raise ValueError(f"manual_poi: expected (B,{self.npts},2), got {tuple(m.shape)}")
        B, N = int(m.shape[0]), self.npts
        out = {"theta_c2f": torch.empty((B, 3, 3), dtype=torch.float64, device=dev),
               "theta": torch.empty((B, 3, 3), dtype=torch.float64, device=dev),
               "theta_f32": torch.empty((B, 3, 3), dtype=torch.float32, device=dev),
               "poi": torch.empty((B, N, 3), dtype=torch.float64, device=dev),
               "num_nonzero": torch.empty((B,), dtype=torch.int32, device=dev),
               "reproj_mse": torch.empty((B,), dtype=torch.float64, device=dev),
               "status": torch.empty((B,), dtype=torch.int32, device=dev)}
        lib = _lib.load()
        p = _ptr
        with torch.cuda.device(dev):
            st = _stream(dev)
            _lib.check(lib.sfh_prep_fit(p(d["poi"]), p(m), p(d["ignore"]), B, N, self.norm_size[0], self.norm_size[1],
                                        self.refine if refine is None else int(refine), p(out["theta_c2f"]), p(out["theta"]),
                                        p(out["theta_f32"]), p(out["poi"]), p(out["num_nonzero"]), p(out["reproj_mse"]),
                                        p(out["status"]), st), "prep_fit")
        return out

    def render(self, theta, uv=None):
        """theta (B,3,3) | (B,1,3,3) float32 on the device (frame -> court) -> dict: mask uint8 (B,H,W) and, with uv, uv
        uint16 (B,H,W,3) = (id, u, v)"""
        d = self._tensors()
        dev = self.device
        if not isinstance(theta, torch.Tensor) or theta.dtype != torch.float32 or theta.device != dev \
                or theta.numel() % 9 or theta.numel() == 0 or not theta.is_contiguous():
            raise ValueError(f"theta: expected a contiguous float32 tensor (B,3,3) on {dev}")
        want_uv = self.uv if uv is None else bool(uv)
        B = theta.numel() // 9
        out = {"mask": torch.empty((B, self.H, self.W), dtype=torch.uint8, device=dev)}
        if want_uv:
            out["uv"] = torch.empty((B, self.H, self.W, 3), dtype=torch.uint16, device=dev)
        lib = _lib.load()
        p = _ptr
        with torch.cuda.device(dev):
            st = _stream(dev)
            _lib.check(lib.sfh_prep_render(p(theta), p(d["ids"]), int(self.court_ids.shape[0]), int(self.court_ids.shape[1]),
                                           p(d["u"]), p(d["v"]), B, self.H, self.W, 1 if want_uv else 0, p(out["mask"]),
                                           p(out.get("uv")), st), "prep_render")
        return out

    def make(self, manual_poi):
        """fit + render: the dict of ``fit`` plus mask (and uv).  Frames with status 0 hold an all-zero theta: their mask
        is whatever that renders and nothing downstream reads it (``to_batch`` drops them)."""
        out = self.fit(manual_poi)
        out.update(self.render(out["theta_f32"]))
        return out


def rgb_to_ids(rgb, num_classes):
    """convert_rgb_to_onehot / generate_onehot: uint8 (..,3) on the device -> uint8 (..): k where the pixel equals colour k
    of the table (the inverse of ``outputs.format_masks(.., 'rgb')``), else the pixel's channel-0 byte"""
    O._palette_bytes(int(num_classes))
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() < 2 or rgb.shape[-1] != 3 \
            or not rgb.is_contiguous() or rgb.numel() == 0:
        raise ValueError("rgb_to_ids: expected a contiguous uint8 tensor (..,3)")
    if rgb.device.type != "cuda":
        raise RuntimeError(f"rgb_to_ids: device {rgb.device} - the HIP path has no CPU fallback")
    out = torch.empty(rgb.shape[:-1], dtype=torch.uint8, device=rgb.device)
    with torch.cuda.device(rgb.device):
        st = _stream(rgb.device)
        _lib.check(_lib.load().sfh_prep_rgb_to_ids(_ptr(rgb), out.numel(), int(num_classes), _ptr(out), st), "prep_rgb_to_ids")
    return out


def split_uv(uv_u16):
    """preprocess_uv_mask (utils/dataset.py:172-185) without its resize: uint16 (..,H,W,3) array or tensor -> mask
    (uint8, (..,H,W)) and uv float32 (..,2,H,W) = the two planes / 65535 (the division in fp64, rounded once)"""
    if isinstance(uv_u16, torch.Tensor):
        wide = uv_u16.view(torch.int16).to(torch.int32) & 0xFFFF      # uint16 has few device operators: widen through int16
        m = wide[..., 0].to(torch.uint8)
        uv = (wide[..., 1:3].to(torch.float64) / float(MAX_VALUE_UINT16)).to(torch.float32)
        return m, uv.movedim(-1, -3).contiguous()
    a = np.asarray(uv_u16)
    assert a.dtype == np.uint16
    return a[..., 0].astype(np.uint8), np.ascontiguousarray(
        np.moveaxis((a[..., 1:3] / float(MAX_VALUE_UINT16)).astype(np.float32), -1, -3))


def to_batch(labels, frames=None, names=None, frame_resize=None):
    """labels: the dict of ``LabelMaker.make`` (tensors on any device); frames: uint8 (B,H,W,3) or None; names: B frame
    names or None (then indices).  Returns (batch, dropped): the frames with status 1 as BatchAugment, TrainStep and
    eval_reconstructor take them - frames_u8 and image float32 (B,3,H,W) = / 255 (when frames are given), mask_u8, mask
    int64, uv float32 (B,2,H,W) (when labels hold uv), poi (B,N,2), nonzeros (B,N) float32, num_nonzero (B,) float32, weight
    (B,1) float32 (preprocess_weight of reproj_mse), theta float32 (B,3,3), name - and the names of the dropped frames.
    frame_resize="pil": frames of another size than the labels are resized on the device with Pillow's rule
    (BasicDataset.preprocess_img's `pil_img.resize`, sfh_amd.resample) instead of refused; frames_u8 holds the resized bytes."""
    if frame_resize not in (None, "pil"):
        raise ValueError(f'to_batch: frame_resize={frame_resize!r} (None or "pil")')
    status = labels["status"].cpu().numpy()
    B = int(status.shape[0])
    names = list(range(B)) if names is None else list(names)
    if len(names) != B:
        raise ValueError(f"to_batch: {len(names)} names for {B} frames")
    keep = np.flatnonzero(status == 1)
    dropped = [names[i] for i in np.flatnonzero(status != 1)]
    if keep.size == 0:
        return None, dropped
    dev = labels["mask"].device
    idx = torch.from_numpy(keep).to(dev)
    sel = lambda t: t.index_select(0, idx)
    poi3 = sel(labels["poi"])
    batch = {"name": [names[i] for i in keep],
             "mask_u8": sel(labels["mask"]).contiguous(),
             "poi": poi3[..., :2].to(torch.float32).contiguous(),
             "nonzeros": poi3[..., 2].to(torch.float32).contiguous(),
             "theta": sel(labels["theta"]).to(torch.float32).contiguous()}
    batch["mask"] = batch["mask_u8"].to(torch.int64)
    batch["num_nonzero"] = torch.count_nonzero(batch["nonzeros"], dim=1).to(torch.float32)
    w = preprocess_weight(labels["reproj_mse"].cpu().numpy()[keep])
    batch["weight"] = torch.from_numpy(w).reshape(-1, 1).to(dev)
    if "uv" in labels:
        batch["uv"] = split_uv(sel(labels["uv"].view(torch.int16)).view(torch.uint16))[1]
    if frames is not None:
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[0] != B \
                or frames.shape[3] != 3 \
                or (frame_resize is None and tuple(frames.shape[1:3]) != tuple(labels["mask"].shape[1:])):
            raise ValueError(f"frames: expected uint8 ({B},H,W,3) of the labels' size, got {tuple(getattr(frames, 'shape', ()))}")
        fr = sel(frames.to(dev)).contiguous()
        if tuple(fr.shape[1:3]) != tuple(labels["mask"].shape[1:]):
            from . import resample
            hd, wd = (int(v) for v in labels["mask"].shape[1:])
            fr, batch["image"] = resample.resampler(tuple(int(v) for v in fr.shape[1:3]), (hd, wd), 3).both(fr)
        else:
            batch["image"] = (fr.permute(0, 3, 1, 2).to(torch.float32) / 255).contiguous()      # utils/dataset.py:154-159
        batch["frames_u8"] = fr
    return batch, dropped


# ---------------------------------------------------------------------------------------------- dataset on disk
def prepare_dataset(anno_dir, dst_dir, court_ids=None, court_poi=None, size=(640, 360), num_classes=4, uv=False,
                    ignore_pts=None, refine=10, norm_size=None, batch=64, maker=None, device="cuda", png="host",
                    uv_format="npy", tif="host"):
    """Steps 1-5 and 7 of dataset_utils/preparation.py: reads one ``manual_anno.json`` per game directory of ``anno_dir``
    (``generate_requests``), batches the frames across games and writes per fitted frame, under ``dst_dir/<game>/``,
    ``<frame>.json`` = {theta (frame -> court, 3x3), poi (N,3: x, y, flag), reproj_mse} - the keys ``BasicDataset`` reads -,
    ``<frame>.png`` = the id mask (``outputs.encode_png``) and, with uv, the UV label uint16 (H,W,3) (id, u, v): uv_format "npy"
    (the default) writes ``<frame>.npy``, "tif" the 16-bit ``<frame>.tif`` the reference's reader expects, "both" both.  maker:
    any object with ``LabelMaker.make``'s contract (default: a LabelMaker built from the arguments).  png: "host"
    (outputs.encode_png, the default) or "device" (sfh_amd.pngenc: the masks are encoded on the GPU).  tif: "host"
    (outputs.encode_tiff, the default) or "device" (sfh_amd.tiffenc: the UV labels of a batch are encoded in one
    TiffEncoder.encode and only the files come to the host).  Returns {"written": [game/frame, ..], "skipped": [..]};
    skipped = frames with fewer than 4 usable points (the reference's ``return None``), for which nothing is written."""
    if uv_format not in ("npy", "tif", "both"):
        raise ValueError(f'prepare_dataset: uv_format={uv_format!r} ("npy", "tif" or "both")')
    if tif not in ("host", "device"):
        raise ValueError(f'prepare_dataset: tif={tif!r} ("host" or "device")')
    if maker is None:
        maker = LabelMaker(court_ids, court_poi, size, num_classes, uv=uv, ignore_pts=ignore_pts, refine=refine,
                           norm_size=norm_size, device=device)
    requests = generate_requests(anno_dir)
    todo = [(game, fid, poi) for game, frames in requests.items() for fid, poi in frames.items()]
    written, skipped = [], []
    for first in range(0, len(todo), int(batch)):
        chunk = todo[first:first + int(batch)]
        shapes = {p.shape for _, _, p in chunk}
        if len(shapes) != 1:
            raise ValueError(f"prepare_dataset: manual poi of different shapes in one run: {sorted(shapes)}")
        labels = maker.make(np.stack([p for _, _, p in chunk]))
        files = files_from_batch(labels["mask"], 1, png)
        tif_files = None
        if "uv" in labels and uv_format != "npy":
            from . import tiffenc
            tif_files = tiffenc.files_from_batch(labels["uv"], tif)
        host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in labels.items()
                if k != "mask"}
        for k, (game, fid, _) in enumerate(chunk):
            key = f"{game}/{fid}"
            if int(host["status"][k]) != 1:
                skipped.append(key)
                continue
            os.makedirs(os.path.join(dst_dir, game), exist_ok=True)
            stem = os.path.join(dst_dir, game, str(fid))
            with open(stem + ".json", "w") as f:
                json.dump({"theta": host["theta"][k].reshape(3, 3).tolist(), "poi": host["poi"][k].tolist(),
                           "reproj_mse": float(host["reproj_mse"][k])}, f)
            with open(stem + ".png", "wb") as f:
                f.write(files[k].tobytes())
            if "uv" in host and uv_format != "tif":
                np.save(stem + ".npy", host["uv"][k])
            if tif_files is not None:
                with open(stem + ".tif", "wb") as f:
                    f.write(tif_files[k].tobytes())
            written.append(key)
    return {"written": written, "skipped": skipped}


def read_dataset(dst_dir, keys, use_uv=False, device="cpu", size=None, decode="host", uv_format="npy"):
    """``BasicDataset.__getitem__``'s label side (utils/dataset.py:240-289, anno_keys = theta, poi, reproj_mse; no resize: the
    labels are written at the target size) for the frames ``keys`` (``game/frame``) of a tree written by ``prepare_dataset``,
    collated: the entries ``to_batch`` returns for the same frames (without frames_u8 / image).
    size=(W, H): the labels at another size than the written one, as ``BasicDataset`` resizes them - the mask with
    ``Image.NEAREST`` (preprocess_mask), the uint16 UV label with cv2.INTER_NEAREST before it is split (preprocess_uv_mask) - on
    the device (``resample.resize_nearest``): ``device`` must then be a GPU.
    decode: "host" (outputs.decode_png, the default) or "device" - the mask files of all keys in one sfh_amd.pngdec decode, only
    the files are uploaded: ``device`` must then be a GPU.
    uv_format: "npy" (the default) reads the UV label from ``<frame>.npy``, "tif" from the 16-bit ``<frame>.tif`` - with
    decode="host" through outputs.decode_tiff, with decode="device" the files of all keys in one sfh_amd.tiffdec decode; the
    batch is the one the ``.npy`` route returns for the same labels."""
    if uv_format not in ("npy", "tif"):
        raise ValueError(f'read_dataset: uv_format={uv_format!r} ("npy" or "tif")')
    if decode not in ("host", "device"):
        raise ValueError(f'read_dataset: decode={decode!r} ("host" or "device")')
    if decode == "device" and torch.device(device).type != "cuda":
        raise ValueError(f"read_dataset: decode='device' decodes on the device; device={device!r} is not a GPU")
    if size is not None:
        size = (int(size[0]), int(size[1]))
        if torch.device(device).type != "cuda":
            raise ValueError(f"read_dataset: size={size} resizes on the device; device={device!r} is not a GPU")
        from . import resample
    masks, uvs, pois, nzs, thetas, ws = [], [], [], [], [], []
    mask_files, uv_files = [], []
    if use_uv and uv_format == "tif":
        load_uv = lambda stem: O.decode_tiff(np.fromfile(stem + ".tif", dtype=np.uint8))
    else:
        load_uv = lambda stem: np.load(stem + ".npy")
    for key in keys:
        stem = os.path.join(dst_dir, *str(key).split("/"))
        with open(stem + ".json", "r") as f:
            anno = json.load(f)
        if use_uv and uv_format == "tif" and decode == "device":
            m = None
            uv_files.append(np.fromfile(stem + ".tif", dtype=np.uint8))
        elif use_uv and size is not None:
            lab = torch.from_numpy(np.ascontiguousarray(load_uv(stem)).view(np.int16)).to(device).view(torch.uint16)
            m, uvp = split_uv(resample.resize_nearest(lab[None], (size[1], size[0]), rule="cv2")[0])
            uvs.append(uvp)
            masks.append(m.contiguous())
            m = None
        elif use_uv:
            m, uvp = split_uv(load_uv(stem))
            uvs.append(torch.from_numpy(uvp))
        elif decode == "device":
            m = None
            mask_files.append(np.fromfile(stem + ".png", dtype=np.uint8))
        else:
            m = O.decode_png(np.fromfile(stem + ".png", dtype=np.uint8))
        if m is not None:
            masks.append(torch.from_numpy(np.ascontiguousarray(m)))
        p = torch.from_numpy(np.asarray(anno["poi"], dtype="float")).type(torch.FloatTensor)
        pois.append(p[:, :2])
        nzs.append(p[:, 2])
        thetas.append(torch.from_numpy(np.asarray(anno["theta"], dtype="float")).type(torch.FloatTensor))
        ws.append(torch.from_numpy(preprocess_weight(np.asarray([anno["reproj_mse"]], dtype="float"))))
    uv_planes = None
    if uv_files:
        from . import tiffdec
        labs = tiffdec.decode_tiff_device(uv_files, device=device)
        if labs.dim() != 4 or labs.dtype != torch.uint16:
            raise ValueError("the UV files must hold 3-channel 16-bit labels of one size")
        if size is not None:
            labs = resample.resize_nearest(labs, (size[1], size[0]), rule="cv2")
        mask_u8, uv_planes = split_uv(labs)
        mask_u8 = mask_u8.contiguous()
    elif mask_files:
        from . import pngdec
        mask_u8 = pngdec.masks_from_files(mask_files, device)
    else:
        mask_u8 = torch.stack(masks).to(device)
    if size is not None and not use_uv:
        mask_u8 = resample.resize_nearest(mask_u8.contiguous(), (size[1], size[0]), rule="pil")
    batch = {"name": [str(k) for k in keys], "mask_u8": mask_u8,
             "poi": torch.stack(pois).contiguous().to(device), "nonzeros": torch.stack(nzs).contiguous().to(device),
             "theta": torch.stack(thetas).to(device), "weight": torch.stack(ws).to(device)}
    batch["mask"] = batch["mask_u8"].to(torch.int64)
    batch["num_nonzero"] = torch.count_nonzero(batch["nonzeros"], dim=1).to(torch.float32)
    if use_uv:
        batch["uv"] = uv_planes if uv_planes is not None else torch.stack(uvs).to(device)
    return batch
