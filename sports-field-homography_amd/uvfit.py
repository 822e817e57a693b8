"""Homography fit from the UV head: a second estimate of theta, independent of the ResNet-STN's regression.

    fit = UVFit(court_size=(320, 180), grid_size=net.warp_size, mask_classes=4, iters=4, delta=2.0)
    theta, stats, status = fit(uv, logits, theta0)
    # theta (B,1,3,3) float32; stats (B,4) float64 = [gated pixels, inliers, robust rms in court px, algebraic cost];
    # status (B,) int32: the number of solves that succeeded (iters + 1 for a frame that never failed)

The UV map is a dense set of frame -> court correspondences, one per court pixel in view.  They are fitted by iteratively
reweighted least squares - a Cauchy weight of ``delta`` court pixels, each pass one linear 8 x 8 solve.  The rule - gate,
coordinates, residual, weight, sums, step - is stated once in include/sfh_amd.h above the ``sfh_uvfit_*`` entries;
csrc/uvfit.hip runs it, tests/uvfit_ref.py restates it in numpy.  The reference project has no counterpart.

``court_size`` (wt, ht) is the court raster the UV labels were rendered from (``LabelMaker``'s ``court_ids`` size), which
need not be the court template's; ``grid_size`` (W, H) the warp grid theta addresses (``net.warp_size``).

A call launches 2 * (iters + 2) kernels on the caller's current stream, synchronises nothing and reads nothing back.
Workspaces are held once per (batch, size, stream); after the first call of a shape only the three outputs are new tensors.
"""
import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

SUMS = _lib.ABI.defines["SFH_UVFIT_SUMS"]


class UVFit:
    def __init__(self, court_size, grid_size, mask_classes=None, iters=4, delta=2.0):
        """mask_classes: the class count of the logits that gate the fit (None: a call takes no logits)"""
        wt, ht = int(court_size[0]), int(court_size[1])
        W, H = int(grid_size[0]), int(grid_size[1])
        if min(wt, ht) < 2:
            raise ValueError(f"UVFit: court_size {court_size}")
        if min(W, H) < 2:
            raise ValueError(f"UVFit: grid_size {grid_size}")
        if mask_classes is not None and not 2 <= int(mask_classes) <= 8:
            raise ValueError(f"UVFit: mask_classes={mask_classes} (2..8)")
        iters, delta = int(iters), float(delta)
        if iters < 0:
            raise ValueError(f"UVFit: iters={iters} (>= 0)")
        if not delta > 0:
            raise ValueError(f"UVFit: delta={delta} (> 0)")
        self.court_size, self.grid_size = (wt, ht), (W, H)
        self.mask_classes = None if mask_classes is None else int(mask_classes)
        self.iters, self.delta = iters, delta
        self._work = {}        # (B, h, w, device, stream) -> buffers

    def __getstate__(self):
        """configuration only: workspaces are rebuilt on first use"""
        st = self.__dict__.copy()
        st["_work"] = {}
        return st

    def constants(self):
        """(u_min, v_min, kx, ky) as the entries take them: the gate thresholds rounded once to fp32, the court offsets fp64"""
        wt, ht = self.court_size
        return float(np.float32(0.5 / wt)), float(np.float32(0.5 / ht)), 1.0 + 1.0 / wt, 1.0 + 1.0 / ht

    def _buffers(self, B, h, w, dev):
        key = (B, h, w, dev, torch.cuda.current_stream(dev).cuda_stream)
        wk = self._work.get(key)
        if wk is None:
            nbytes = _lib.load().sfh_uvfit_workspace_bytes(B, h, w)
            if nbytes < 0:
                raise ValueError(f"UVFit: batch {B} (1..65535) of {w}x{h}")
            wk = self._work[key] = {"ws": torch.empty(nbytes // 8, dtype=torch.float64, device=dev), "ws_bytes": nbytes,
                                    "slabs": nbytes // (B * SUMS * 8),
                                    "cand": torch.empty((B, 9), dtype=torch.float32, device=dev)}
        return wk

    def _check(self, uv, logits, theta0):
        if not torch.is_tensor(uv) or uv.dim() != 4 or uv.shape[1] != 2:
            raise ValueError("UVFit: uv must be a tensor (B,2,h,w)")
        B, _, h, w = uv.shape
        if h < 2 or w < 2:
            raise ValueError(f"UVFit: uv of {w}x{h} (both >= 2)")
        if logits is not None:
            if self.mask_classes is None:
                raise ValueError("UVFit: logits given, but the fit was built without mask_classes")
            if not torch.is_tensor(logits) or tuple(logits.shape) != (B, self.mask_classes, h, w):
                raise ValueError(f"UVFit: logits must be ({B},{self.mask_classes},{h},{w})")
        if theta0 is not None and (not torch.is_tensor(theta0) or tuple(theta0.shape) not in ((B, 1, 3, 3), (B, 3, 3))):
            raise ValueError(f"UVFit: theta0 must be ({B},1,3,3)")
        given = [(name, t) for name, t in (("uv", uv), ("logits", logits), ("theta0", theta0)) if t is not None]
        for name, t in given:
            if t.dtype != torch.float32:
                raise ValueError(f"UVFit: float32 expected, got {name} {t.dtype}")
        for name, t in given:
            if not t.is_cuda or t.device != uv.device:
                raise ValueError(f"UVFit: {name} must be a CUDA tensor on uv's device (there is no CPU path)")

    def __call__(self, uv, logits=None, theta0=None):
        """uv (B,2,h,w), logits (B,mask_classes,h,w) or None, theta0 (B,1,3,3) or None -> (theta, stats, status)"""
        self._check(uv, logits, theta0)
        B, _, h, w = uv.shape
        dev = uv.device
        theta = torch.empty((B, 1, 3, 3), dtype=torch.float32, device=dev)
        stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        if B == 0:
            return theta, stats, status
        with torch.cuda.device(dev):
            lib, st = _lib.load(), _stream()
            wk = self._buffers(B, h, w, dev)
            uvc = uv.contiguous()
            lg = None if logits is None else logits.contiguous()
            t0 = None if theta0 is None else theta0.contiguous()
            (wt, ht), (W, H) = self.court_size, self.grid_size
            u_min, v_min, kx, ky = self.constants()
            nc = self.mask_classes or 0

            def accumulate(t):
                _lib.check(lib.sfh_uvfit_accumulate(_ptr(uvc), _ptr(lg), nc, _ptr(t), B, h, w, H, W, wt, ht, u_min, v_min, kx, ky,
                                                    self.delta, _ptr(wk["ws"]), wk["ws_bytes"], st), "uvfit_accumulate")

            def step(k, last, t_eval, t_next):
                _lib.check(lib.sfh_uvfit_step(_ptr(wk["ws"]), wk["slabs"], B, k, last, _ptr(t_eval), _ptr(t_next), _ptr(status),
                                              _ptr(stats), st), "uvfit_step")

            cand = wk["cand"]
            accumulate(t0)
            step(0, 0, t0, cand)
            for k in range(1, self.iters + 1):
                accumulate(cand)
                step(k, 0, cand, cand)
            accumulate(cand)
            step(self.iters + 1, 1, cand, theta)
        return theta, stats, status
