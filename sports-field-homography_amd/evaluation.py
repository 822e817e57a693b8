"""Validation / test scoring on the HIP path: ``eval_reconstructor`` of the reference (eval.py:142-234).

Drop-in for ``from eval import eval_reconstructor`` (train.py:17,253, test.py): same arguments, same result keys, the net
left in train mode.  Per batch, ``net(imgs)`` (the eval-mode forward) runs the model kernels and ONE library call
(``sfh_eval_batch``, csrc/eval.hip) reads the logits, mask and warp once and adds the batch's seg / rec / consist /
reprojection scores into an fp64 accumulator vector on the device; the uv score goes through ``sfh_uv_loss`` (lambda 1)
into the same vector.  Nothing is read back until the end of the call, where the vector - summed over the ranks by one
all_reduce when there are several - is copied to the host once and divided by the batch and frame counts
(``scores_from_accumulator``).

Divergences from the reference, all on inputs it cannot handle: an empty loader and ``warp_size != target_size`` raise
ValueError up front (the reference dies with ZeroDivisionError / a shape error); a mask id outside [0, nc) other than -100
or a consistency class outside [0, nc) raises ValueError after the loop (torch raises inside it).  The reference scales
``batch['poi']`` in place when the batch already lives on the device (eval.py:209-210); this does not touch the batch.
"""
import ctypes

import torch

from . import _lib
from . import sharding
from .engine import _ptr, _stream

# slots of the accumulator vector (include/sfh_amd.h, SFH_EVAL_*)
SEG, REC, UV, REPROJ, REPROJ_PX, CONSIST, NBATCH, FRAMES, BAD = (_lib.ABI.defines["SFH_EVAL_" + s] for s in (
    "SEG", "REC", "UV", "REPROJ", "REPROJ_PX", "CONSIST", "NBATCH", "FRAMES", "BAD"))
SLOTS = _lib.ABI.defines["SFH_EVAL_SLOTS"]


def scores_from_accumulator(acc):
    """The final arithmetic of eval.py:219-225 on the host: the summed vector (SLOTS numbers, already reduced over the
    ranks) -> the six scores as Python floats.  The seg, rec, uv and consist sums are sums of per-batch means, divided by
    the number of batches; the reprojection sums are sums over frames, divided by the number of frames."""
    a = [float(v) for v in acc]
    if len(a) != SLOTS:
        raise ValueError(f"accumulator has {len(a)} slots, expected {SLOTS}")
    if a[BAD] != 0:
        raise ValueError("eval_reconstructor: a mask id outside [0, mask_classes) other than -100, or a warp class "
                         "trunc(warp_mask * mask_classes) outside that range (a non-finite warp included); "
                         "F.cross_entropy raises on the same input")
    n_val, counter = a[NBATCH], a[FRAMES]
    if n_val <= 0 or counter <= 0:
        raise ValueError("eval_reconstructor: no batch was evaluated")
    return {'val_seg_score': a[SEG] / n_val,
            'val_rec_score': a[REC] / n_val,
            'val_uv_score': a[UV] / n_val,
            'val_reproj_score': a[REPROJ] / counter,
            'val_reproj_px': a[REPROJ_PX] / counter,
            'val_consist_score': a[CONSIST] / n_val}


def _dev_contig(t, device, dtype):
    return t.to(device=device, dtype=dtype).contiguous()


def _batch_scores(lib, net, acc_ptr, flag_ptr, ws, logits, masks, warp, weights, poi, gt_poi, nonzeros, num_nonzero,
                  target_size, st):
    """one sfh_eval_batch call; returns the workspace (grown when a batch needs more)"""
    nc = int(net.mask_classes)
    ref = logits if logits is not None else warp
    B = int(masks.shape[0])
    if ref is not None:
        H, W = int(ref.shape[-2]), int(ref.shape[-1])
        if logits is not None and tuple(logits.shape) != (B, nc, H, W):
            raise ValueError(f"logits {tuple(logits.shape)} against a mask of {tuple(masks.shape)}")
        if warp is not None and tuple(warp.shape) != (B, H, W):
            raise ValueError(f"warp_mask {tuple(warp.shape)} and target {(B, H, W)} differ in size")
        if tuple(masks.shape) != (B, H, W):
            raise ValueError(f"batch['mask'] {tuple(masks.shape)} does not match the predictions {(B, H, W)}")
    else:
        H, W = int(masks.shape[-2]), int(masks.shape[-1])
    if weights is not None and weights.numel() != B:
        raise ValueError(f"{weights.numel()} per-sample weights for a batch of {B}")
    npts = 0
    if poi is not None:
        if tuple(gt_poi.shape) != tuple(poi.shape):
            raise ValueError(f"batch['poi'] {tuple(gt_poi.shape)} against projected points {tuple(poi.shape)}")
        npts = int(poi.shape[1])
        if nonzeros.numel() != B * npts or num_nonzero.numel() != B:
            raise ValueError(f"batch['nonzeros'] {tuple(nonzeros.shape)} / batch['num_nonzero'] "
                             f"{tuple(num_nonzero.shape)} do not match {B} frames of {npts} points")
    need = lib.sfh_eval_workspace_doubles(B, H, W)
    if need < 0:
        raise ValueError(f"eval_reconstructor: batch of {B} frames of {W}x{H} is not supported")
    if ws is None or ws.numel() < need:
        ws = torch.empty((need,), dtype=torch.float64, device=masks.device)
    _lib.check(lib.sfh_eval_batch(_ptr(logits), _ptr(masks), _ptr(warp), _ptr(weights), nc, B, H, W, _ptr(poi),
                                  _ptr(gt_poi), _ptr(nonzeros), _ptr(num_nonzero), npts, float(target_size[0]),
                                  float(target_size[1]), _ptr(ws), flag_ptr, acc_ptr, st), "eval_batch")
    return ws


def eval_reconstructor(net, loader, device, target_size, use_per_sample_weights=True, group=None, force_collective=False):
    """eval.py:142-234 on the HIP path -> dict of val_seg_score, val_rec_score, val_uv_score, val_reproj_score,
    val_reproj_px, val_consist_score (floats) and the LAST batch's imgs, logits, warp_masks, uv_masks (CPU tensors, those
    the net produced).  ``loader``: this rank's batches (dicts of image, mask, weight and optionally poi / nonzeros /
    num_nonzero / uv); with a process group of several ranks (or ``force_collective``) the accumulated sums of all ranks
    are added by one all_reduce before the division, so every rank returns the scores of the whole validation set."""
    n_val = len(loader)
    if n_val == 0:
        raise ValueError("eval_reconstructor: the loader is empty (the reference divides by len(loader) == 0)")
    target_w, target_h = target_size[0], target_size[1]
    has_logits = bool(net.use_unet)
    has_warp = bool(net.use_resnet) and net.warper is not None
    if has_logits and has_warp and tuple(net.warp_size) != (target_w, target_h):
        raise ValueError(f"eval_reconstructor: warp_size {tuple(net.warp_size)} != target_size {(target_w, target_h)}: the "
                         "warp is scored against the mask and the logits pixel by pixel")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"eval_reconstructor: device {dev} - the HIP path has no CPU fallback")
    lib = _lib.load()
    # one host-to-device copy: the accumulator (n_val in its slot, summed over the ranks like every other slot) and, in the
    # word behind it, the kernels' error flag
    init = [0.0] * (SLOTS + 1)
    init[NBATCH] = float(n_val)
    buf = torch.tensor(init, dtype=torch.float64, device=dev)
    acc = buf[:SLOTS]
    acc_ptr = ctypes.c_void_p(buf.data_ptr())
    flag_ptr = ctypes.c_void_p(buf.data_ptr() + 8 * SLOTS)
    ones = torch.tensor([1.0], dtype=torch.float32, device=dev) if net.unet_uv and not use_per_sample_weights else None
    ws = None
    imgs = logits = warp_masks = uv = None
    net.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                imgs = batch['image'].to(device=dev, dtype=torch.float32)
                gt_masks = _dev_contig(batch['mask'], dev, torch.long)
                gt_uv = _dev_contig(batch['uv'], dev, torch.float32) if net.unet_uv else None
                gt_poi = nonzeros = num_nonzero = None
                if 'poi' in batch:
                    gt_poi = _dev_contig(batch['poi'], dev, torch.float32)
                    nonzeros = _dev_contig(batch['nonzeros'], dev, torch.float32)
                    num_nonzero = _dev_contig(batch['num_nonzero'], dev, torch.float32)
                weights = _dev_contig(batch['weight'], dev, torch.float32).reshape(-1) if use_per_sample_weights else None

                preds = net(imgs)
                logits, poi = preds.get('logits'), preds.get('poi')
                warp_masks, uv = preds.get('warp_mask'), preds.get('uv')

                st = _stream()
                ws = _batch_scores(lib, net, acc_ptr, flag_ptr, ws, logits, gt_masks, warp_masks, weights,
                                   poi if gt_poi is not None else None, gt_poi, nonzeros, num_nonzero, target_size, st)
                if uv is not None:
                    if tuple(gt_uv.shape) != tuple(uv.shape):
                        raise ValueError(f"batch['uv'] {tuple(gt_uv.shape)} against the uv head's {tuple(uv.shape)}")
                    B, C, H, W = (int(s) for s in uv.shape)
                    wgt = weights if use_per_sample_weights else ones
                    # models/losses.py:38-39 on the 4-D map: the B weights broadcast along the last axis (B == 1 or W)
                    _lib.check(lib.sfh_uv_loss(_ptr(uv), _ptr(gt_uv), _ptr(wgt), wgt.numel(), B, C, H, W, 1.0, 1,
                                               _ptr(torch.empty_like(uv)), ctypes.c_void_p(buf.data_ptr() + 8 * UV), st),
                               "uv_loss")
    finally:
        net.train()
    if imgs is None:
        raise ValueError("eval_reconstructor: the loader yielded no batch")
    sharding.allreduce_scores(acc, group=group, force_collective=force_collective)
    result = scores_from_accumulator(acc.cpu().tolist())      # the call's one host synchronisation
    result['imgs'] = imgs.cpu()
    if logits is not None:
        result['logits'] = logits.cpu()
    if warp_masks is not None:
        result['warp_masks'] = warp_masks.cpu()
    if uv is not None:
        result['uv_masks'] = uv.cpu()
    return result
