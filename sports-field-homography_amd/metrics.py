"""Registration metrics: how good a homography is against a labelled one, frame by frame.

    m = RegistrationMetrics(mask_classes=4, court_size=(640, 360), frame_size=(640, 360), court_pts=court_poi[0])
    m.add(preds["theta"], batch["theta"], batch["mask"], logits=preds["logits"], warp_mask=preds["warp_mask"])
    m.summary()      # per-class IoU / mIoU / pixel accuracy; mean, median, 90th percentile of IoU_part, IoU_whole,
                     # reprojection error (pixels of the frame) and projection error (court units) over the frames
    evaluate_registration(net, loader, "cuda")      # the same through net.predict(), so that a refiner counts

The rules - the confusion counts, the region predicate behind IoU_part and IoU_whole, the two point errors - are stated once in
include/sfh_amd.h above the ``sfh_metrics_*`` entries; csrc/metrics.hip runs them, tests/metrics_ref.py restates them in
numpy.  The reference project has no counterpart.  theta maps the normalised frame to the normalised court, as everywhere here.

The three direct functions (``confusion``, ``region_counts``, ``point_errors``) launch on the caller's current stream,
synchronise nothing and return device tensors.  ``RegistrationMetrics.add`` keeps the per-frame rows on the device;
``table()`` is the one read-back.  The ratio and summary arithmetic below it (``iou_ratio``, ``class_scores``,
``figure_stats``, ``summarize``) is plain numpy on integers and doubles and needs no GPU.
"""
import numpy as np
import torch

from . import _lib
from .mapping import UNITS

MODES = {"part": 0, "whole": 1}
FIGURES = ("iou_part", "iou_whole", "reproj_px", "proj_err")
KIND_I32, KIND_U8, KIND_LOGITS, KIND_WARP = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ host arithmetic (no GPU)
def check_flag(flag):
    """the sticky flag of sfh_metrics_confusion after the read-back: a set bit raises, in eval_reconstructor's wording"""
    flag = int(flag)
    found = []
    if flag & 1:
        found.append("a mask id outside [0, mask_classes) other than -100")
    if flag & 2:
        found.append("a predicted class outside [0, mask_classes) (for a warp mask: trunc(warp_mask * mask_classes), a "
                     "non-finite warp included)")
    if flag:
        raise ValueError("registration metrics: " + (" and ".join(found) or f"flag {flag}")
                         + "; F.cross_entropy raises on the same input")


def iou_ratio(n_a, n_b, n_ab):
    """nAB / (nA + nB - nAB) per frame in fp64; an empty union gives NaN"""
    n_a, n_b, n_ab = (np.asarray(v, dtype=np.int64) for v in (n_a, n_b, n_ab))
    union = n_a + n_b - n_ab
    out = np.full(union.shape, np.nan)
    np.divide(n_ab.astype(np.float64), union.astype(np.float64), out=out, where=union > 0)
    return out


def class_scores(conf):
    """conf (nc,nc) or (F,nc,nc) integer counts [gt][pred], summed over the frames -> dict: iou (nc,) = tp / (gt pixels +
    predicted pixels - tp), NaN for a class absent from both sides; miou = the mean over the classes that are present (NaN if
    none); pixel_acc = trace / total (NaN for no pixel); pixels = total"""
    c = np.asarray(conf, dtype=np.int64)
    if c.ndim == 3:
        c = c.sum(axis=0)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"class_scores: confusion counts of shape {np.shape(conf)}")
    tp = np.diag(c)
    union = c.sum(axis=1) + c.sum(axis=0) - tp
    iou = np.full(len(tp), np.nan)
    np.divide(tp.astype(np.float64), union.astype(np.float64), out=iou, where=union > 0)
    total = int(c.sum())
    present = union > 0
    return {"iou": iou, "miou": float(iou[present].mean()) if present.any() else float("nan"),
            "pixel_acc": float(tp.sum()) / total if total else float("nan"), "pixels": total}


def figure_stats(values):
    """mean, median and 90th percentile (linear interpolation) of a per-frame figure over the frames where it is finite, the
    number of those frames and the number where it is not; no finite frame gives NaN three times"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    ok = np.isfinite(v)
    f = v[ok]
    if f.size == 0:
        return {"mean": float("nan"), "median": float("nan"), "p90": float("nan"), "n": 0, "nonfinite": int(v.size)}
    return {"mean": float(f.mean()), "median": float(np.median(f)), "p90": float(np.percentile(f, 90)), "n": int(f.size),
            "nonfinite": int(v.size - f.size)}


def rows_to_table(names, part, whole, points, conf_seg=None, conf_warp=None):
    """the per-frame rows as read back -> the table: a dict of numpy arrays, one row per frame"""
    part, whole = np.asarray(part, dtype=np.int64).reshape(-1, 3), np.asarray(whole, dtype=np.int64).reshape(-1, 3)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    if not (len(names) == len(part) == len(whole) == len(points)):
        raise ValueError(f"rows_to_table: {len(names)} names, {len(part)} / {len(whole)} region rows, {len(points)} point rows")
    t = {"names": np.asarray(list(names), dtype=object),
         "iou_part": iou_ratio(part[:, 0], part[:, 1], part[:, 2]), "iou_whole": iou_ratio(whole[:, 0], whole[:, 1], whole[:, 2]),
         "reproj_px": points[:, 0].copy(), "proj_err": points[:, 2].copy(),
         "part_counts": part, "whole_counts": whole,
         "n_pts": points[:, 1].astype(np.int64), "n_lattice": points[:, 3].astype(np.int64)}
    for key, c in (("conf_seg", conf_seg), ("conf_warp", conf_warp)):
        if c is not None:
            c = np.asarray(c, dtype=np.int64)
            if c.ndim != 3 or len(c) != len(part):
                raise ValueError(f"rows_to_table: {key} of shape {c.shape} for {len(part)} frames")
            t[key] = c
    return t


def summarize(table):
    """table (rows_to_table) -> {"frames": F, "seg" / "warp": class_scores of the summed confusion counts (where the table has
    them), and figure_stats for each of iou_part, iou_whole, reproj_px, proj_err}"""
    s = {"frames": int(len(table["names"]))}
    for key, name in (("conf_seg", "seg"), ("conf_warp", "warp")):
        if key in table:
            s[name] = class_scores(table[key])
    for f in FIGURES:
        s[f] = figure_stats(table[f])
    return s


# ------------------------------------------------------------------------------------------------ argument checks
def _tensor(t, what, dtypes, dims):
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise ValueError(f"{what}: dtype {t.dtype}, expected {' or '.join(str(d) for d in dtypes)}")
    if t.dim() not in dims:
        raise ValueError(f"{what}: {t.dim()} dimensions {tuple(t.shape)}, expected {' or '.join(str(d) for d in dims)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    return t


def _need_gpu(**tensors):
    """after the checks of form: every tensor on a GPU"""
    for what, t in tensors.items():
        if not t.is_cuda:
            raise ValueError(f"{what}: device {t.device} - the metrics run on the GPU (there is no CPU path)")


def _thetas(theta_pred, theta_gt):
    for t, what in ((theta_pred, "theta_pred"), (theta_gt, "theta_gt")):
        _tensor(t, what, (torch.float32,), (3, 4))
        if tuple(t.shape[-2:]) != (3, 3) or (t.dim() == 4 and t.shape[1] != 1) or t.shape[0] == 0:
            raise ValueError(f"{what}: {tuple(t.shape)}, expected (B,3,3) or (B,1,3,3) with B >= 1")
    if theta_pred.shape[0] != theta_gt.shape[0] or theta_pred.device != theta_gt.device:
        raise ValueError(f"theta_pred {tuple(theta_pred.shape)} on {theta_pred.device} against theta_gt "
                         f"{tuple(theta_gt.shape)} on {theta_gt.device}")
    _need_gpu(theta_pred=theta_pred, theta_gt=theta_gt)
    return int(theta_pred.shape[0])


def _pair(v, what, least):
    try:
        a, b = (int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {v!r}, expected two integers") from None
    if a < least or b < least:
        raise ValueError(f"{what}: {v!r}, both at least {least}")
    return a, b


def _classes(n_classes):
    nc = int(n_classes)
    if not 2 <= nc <= 8:
        raise ValueError(f"n_classes={nc} (2 .. 8)")
    return nc


def _launch():
    from .ops import _ptr, _stream
    return _lib.load(), _ptr, _stream()


# ------------------------------------------------------------------------------------------------ the three entries
def new_flag(device):
    """the sticky error flag of ``confusion``: one zeroed 32-bit word on the device (one small host-to-device copy)"""
    return torch.tensor([0], dtype=torch.int32, device=device)


def confusion(pred, gt, n_classes, flag=None):
    """-> (counts int64 (B,nc,nc) [frame][gt][pred], flag).  gt int64 (B,H,W), -100 ignored.  pred: int32 or uint8 class ids
    (B,H,W), float32 logits (B,nc,H,W) (argmax, the rule above sfh_outconv_fwd), or a float32 warp mask (B,H,W) valued k / nc.
    flag: a word from ``new_flag`` to go on accumulating into (bit 1: a bad gt id, bit 2: a bad predicted class; such pixels
    are counted nowhere); None: a fresh one.  Read it back with the counts and hand it to ``check_flag``."""
    nc = _classes(n_classes)
    _tensor(gt, "gt", (torch.int64,), (3,))
    _tensor(pred, "pred", (torch.int32, torch.uint8, torch.float32), (3, 4))
    B, H, W = (int(s) for s in gt.shape)
    if pred.dim() == 4:
        if pred.dtype != torch.float32:
            raise ValueError(f"pred: a 4-D prediction must be float32 logits, got {pred.dtype}")
        kind, want = KIND_LOGITS, (B, nc, H, W)
    else:
        kind, want = {torch.int32: KIND_I32, torch.uint8: KIND_U8, torch.float32: KIND_WARP}[pred.dtype], (B, H, W)
    if tuple(pred.shape) != want or pred.device != gt.device or B == 0 or H == 0 or W == 0:
        raise ValueError(f"pred {tuple(pred.shape)} on {pred.device} against gt {tuple(gt.shape)} on {gt.device} with "
                         f"{nc} classes: expected {want}, no empty axis")
    _need_gpu(gt=gt, pred=pred)
    if flag is None:
        flag = new_flag(gt.device)
    elif not (torch.is_tensor(flag) and flag.dtype == torch.int32 and flag.numel() == 1 and flag.device == gt.device):
        raise ValueError("flag: expected the one-element int32 tensor of new_flag on gt's device")
    out = torch.empty((B, nc, nc), dtype=torch.int64, device=gt.device)
    with torch.cuda.device(gt.device):
        lib, p, st = _launch()
        _lib.check(lib.sfh_metrics_confusion(p(pred), kind, p(gt), nc, B, H, W, p(out), p(flag), st), "metrics_confusion")
    return out, flag


def default_margin(court_size):
    """half the raster per side"""
    return int(court_size[0]) // 2, int(court_size[1]) // 2


def region_counts(theta_pred, theta_gt, mode, court_size, margin=None):
    """-> int64 (B,3) = [nA, nB, nAB] over the court raster court_size = (wc, hc); IoU = ``iou_ratio`` of the columns.
    mode "part" (0): the court pixels from which the frame is visible under theta_pred / theta_gt; margin None = (0, 0).
    mode "whole" (1): the court rectangle's image under theta_pred theta_gt^-1 against the rectangle, on the raster extended
    by margin = (mx, my) pixels per side; None = half the raster per side."""
    if mode not in MODES and mode not in MODES.values():
        raise ValueError(f"mode={mode!r}: one of {sorted(MODES)} (or 0, 1)")
    mode = MODES.get(mode, mode)
    wc, hc = _pair(court_size, "court_size", 2)
    mx, my = _pair(((0, 0) if mode == 0 else default_margin((wc, hc))) if margin is None else margin, "margin", 0)
    B = _thetas(theta_pred, theta_gt)
    out = torch.empty((B, 3), dtype=torch.int64, device=theta_pred.device)
    with torch.cuda.device(theta_pred.device):
        lib, p, st = _launch()
        _lib.check(lib.sfh_metrics_region(p(theta_pred), p(theta_gt), B, mode, wc, hc, mx, my, p(out), st), "metrics_region")
    return out


def court_scale(units):
    """court units per normalised court unit: half the court's extent in ``units`` (mapping.UNITS)"""
    if units not in UNITS:
        raise ValueError(f"units={units!r}: one of {sorted(UNITS)}")
    return float(UNITS[units][0]) / 2.0, float(UNITS[units][1]) / 2.0


def point_errors(theta_pred, theta_gt, court_pts, frame_size, lattice=(16, 9), units="meters"):
    """-> float64 (B,4) = [reproj_mean, n_pts, proj_mean, n_lattice].  court_pts float64 (N,2) on the device: normalised court
    points shared by the batch; their mean reprojection error is in pixels of a frame of frame_size = (w, h), over the points
    visible in the ground truth.  The projection error is the mean over a lattice = (gx, gy) of frame points that lie on the
    court in the ground truth, in court ``units``."""
    fw, fh = _pair(frame_size, "frame_size", 1)
    gx, gy = _pair(lattice, "lattice", 1)
    csx, csy = court_scale(units)
    _tensor(court_pts, "court_pts", (torch.float64,), (2,))
    B = _thetas(theta_pred, theta_gt)
    if court_pts.shape[1] != 2 or court_pts.device != theta_pred.device:
        raise ValueError(f"court_pts {tuple(court_pts.shape)} on {court_pts.device}: expected (N,2) on {theta_pred.device}")
    out = torch.empty((B, 4), dtype=torch.float64, device=theta_pred.device)
    with torch.cuda.device(theta_pred.device):
        lib, p, st = _launch()
        _lib.check(lib.sfh_metrics_points(p(theta_pred), p(theta_gt), B, p(court_pts), int(court_pts.shape[0]), gx, gy,
                                          fw / 2.0, fh / 2.0, csx, csy, p(out), st), "metrics_points")
    return out


# ------------------------------------------------------------------------------------------------ the accumulator
class RegistrationMetrics:
    """Per-frame registration metrics of a data set, batch by batch.  court_size (wc, hc): the court raster of the two IoUs;
    frame_size (w, h): the frame in pixels; court_pts (N,2): normalised court points (array or tensor) for the reprojection
    error; units: the projection error's (mapping.UNITS); lattice, margin: see ``point_errors`` / ``region_counts``."""

    def __init__(self, mask_classes, court_size, frame_size, court_pts, units="meters", lattice=(16, 9), margin=None):
        self.mask_classes = _classes(mask_classes)
        self.court_size = _pair(court_size, "court_size", 2)
        self.frame_size = _pair(frame_size, "frame_size", 1)
        self.lattice = _pair(lattice, "lattice", 1)
        self.margin = None if margin is None else _pair(margin, "margin", 0)
        court_scale(units)
        self.units = units
        pts = court_pts.detach().cpu().numpy() if torch.is_tensor(court_pts) else np.asarray(court_pts)
        if pts.ndim != 2 or pts.shape[1] != 2 or not np.issubdtype(pts.dtype, np.number):
            raise ValueError(f"court_pts: shape {pts.shape}, expected (N,2) numbers")
        self.court_pts = np.ascontiguousarray(pts, dtype=np.float64)
        self._pts_dev = None
        self._flag = None
        self._rows = []           # per add: (part, whole, points, conf_seg | None, conf_warp | None) on the device
        self._names = []
        self._has = None          # (logits given, warp mask given): the same for every add

    def __len__(self):
        return len(self._names)

    def add(self, theta_pred, theta_gt, gt_mask, logits=None, warp_mask=None, names=None):
        """the rows of one batch, kept on the device; no synchronisation.  gt_mask int64 (B,H,W) is needed only with logits
        (float32 (B,nc,H,W)) or warp_mask (int32 / uint8 ids, or the float32 mask valued k / nc; (B,H,W)), which every add of
        one accumulator gives or omits alike."""
        B = _thetas(theta_pred, theta_gt)
        has = (logits is not None, warp_mask is not None)
        if self._has is not None and has != self._has:
            raise ValueError(f"add: logits / warp_mask given {has}, the earlier batches {self._has}")
        if names is not None and len(names) != B:
            raise ValueError(f"add: {len(names)} names for {B} frames")
        dev = theta_pred.device
        if self._pts_dev is None or self._pts_dev.device != dev:
            self._pts_dev = torch.from_numpy(self.court_pts).to(dev)
        conf = [None, None]
        if any(has):
            if self._flag is None or self._flag.device != dev:
                if self._flag is not None:
                    raise ValueError(f"add: tensors on {dev}, the earlier batches on {self._flag.device}")
                self._flag = new_flag(dev)
            for k, pred in enumerate((logits, warp_mask)):
                if pred is not None:
                    if gt_mask is not None and gt_mask.shape[0] != B:
                        raise ValueError(f"add: gt_mask {tuple(gt_mask.shape)} for {B} frames")
                    conf[k], _ = confusion(pred, gt_mask, self.mask_classes, flag=self._flag)
        part = region_counts(theta_pred, theta_gt, 0, self.court_size, (0, 0))
        whole = region_counts(theta_pred, theta_gt, 1, self.court_size, self.margin)
        pts = point_errors(theta_pred, theta_gt, self._pts_dev, self.frame_size, self.lattice, self.units)
        self._has = has
        self._rows.append((part, whole, pts, conf[0], conf[1]))
        first = len(self._names)
        self._names.extend([str(n) for n in names] if names is not None else [str(first + i) for i in range(B)])

    def table(self):
        """the one read-back: every row and the flag in one device-to-host copy -> dict of numpy arrays, one row per frame:
        names, iou_part, iou_whole, reproj_px, proj_err, part_counts / whole_counts (F,3) [nA, nB, nAB], n_pts, n_lattice and,
        where logits / a warp mask were given, conf_seg / conf_warp (F,nc,nc).  A set flag raises ValueError."""
        if not self._rows:
            raise ValueError("RegistrationMetrics: no batch was added")
        nc2 = self.mask_classes ** 2
        cols = [torch.cat([r[0] for r in self._rows]), torch.cat([r[1] for r in self._rows]),
                torch.cat([r[2] for r in self._rows]).view(torch.int64)]
        cols += [torch.cat([r[k] for r in self._rows]).view(-1, nc2) for k in (3, 4) if self._rows[0][k] is not None]
        flat = torch.cat([c.reshape(-1) for c in cols] + ([self._flag.to(torch.int64)] if self._flag is not None else []))
        host = flat.cpu().numpy()
        F = len(self._names)
        if self._flag is not None:
            check_flag(host[-1])
        at = 0

        def take(width, dtype=np.int64):
            nonlocal at
            v = host[at:at + F * width].view(dtype).reshape(F, width)
            at += F * width
            return v

        part, whole, pts = take(3), take(3), take(4, np.float64)
        confs = [take(nc2).reshape(F, self.mask_classes, self.mask_classes) if h else None for h in self._has]
        return rows_to_table(self._names, part, whole, pts, confs[0], confs[1])

    def summary(self):
        return summarize(self.table())


# ------------------------------------------------------------------------------------------------ the driver
def evaluate_registration(net, loader, device, court_pts=None, court_size=None, lattice=(16, 9), units="meters"):
    """Registration metrics of ``net.predict`` over a labelled loader (batches of ``preparation.to_batch``: image, mask, theta)
    -> {"theta": summary, "frames": table} of the theta predict() returns - the refined one where ``net.refiner`` is set - and
    then also {"theta_stn": summary, "frames_stn": table} of the STN's own theta: the pair says whether refinement helps.
    Where ``net.uv_fitter`` is set, {"theta_uv": summary, "frames_uv": table} score the UV fit on the same frames.
    The segmentation is scored where the logits have the mask's size, the warp mask (of the returned theta) likewise.
    court_pts (N,2) normalised: default the model's ``court_poi``; court_size (wc, hc): default the court template's.  Eval
    mode under no_grad; the net is left in train mode, as eval_reconstructor leaves it."""
    if len(loader) == 0:
        raise ValueError("evaluate_registration: the loader is empty")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"evaluate_registration: device {dev} - the HIP path has no CPU fallback")
    if court_pts is None:
        court_pts = net.court_poi[0, :, :2]
    if court_size is None:
        court_size = (int(net.court_img.shape[-1]), int(net.court_img.shape[-2]))
    nc = int(net.mask_classes)
    acc = {}
    net.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                if 'theta' not in batch:
                    raise ValueError("evaluate_registration: a batch without 'theta' (the labelled frame -> court homography)")
                imgs = batch['image'].to(device=dev, dtype=torch.float32)
                theta_gt = batch['theta'].to(device=dev, dtype=torch.float32).contiguous()
                gt_mask = batch['mask'].to(device=dev, dtype=torch.long).contiguous() if 'mask' in batch else None
                preds = net.predict(imgs, consistency=False)
                if 'theta' not in preds:
                    raise ValueError("evaluate_registration: the model predicts no theta (use_resnet=False)")
                if not acc:
                    fs = (int(gt_mask.shape[-1]), int(gt_mask.shape[-2])) if gt_mask is not None else tuple(net.target_size)
                    for key in ('theta', 'theta_stn', 'theta_uv'):
                        if key in preds:
                            acc[key] = RegistrationMetrics(nc, court_size, fs, court_pts, units=units, lattice=lattice)
                fits = lambda t: t is not None and gt_mask is not None and tuple(t.shape[-2:]) == tuple(gt_mask.shape[-2:])  # noqa: E731
                logits = preds.get('logits') if fits(preds.get('logits')) else None
                warp = preds.get('warp_mask') if fits(preds.get('warp_mask')) else None
                names = batch.get('name')
                acc['theta'].add(preds['theta'].contiguous(), theta_gt, gt_mask, logits=logits, warp_mask=warp, names=names)
                if 'theta_stn' in acc:
                    acc['theta_stn'].add(preds['theta_stn'].contiguous(), theta_gt, gt_mask, logits=logits, names=names)
                if 'theta_uv' in acc:
                    acc['theta_uv'].add(preds['theta_uv'].contiguous(), theta_gt, gt_mask, logits=logits, names=names)
    finally:
        net.train()
    if not acc:
        raise ValueError("evaluate_registration: the loader yielded no batch")
    frames = acc['theta'].table()
    result = {"theta": summarize(frames), "frames": frames}
    if 'theta_stn' in acc:
        stn = acc['theta_stn'].table()
        result["theta_stn"], result["frames_stn"] = summarize(stn), stn
    if 'theta_uv' in acc:
        fit = acc['theta_uv'].table()
        result["theta_uv"], result["frames_uv"] = summarize(fit), fit
    return result
