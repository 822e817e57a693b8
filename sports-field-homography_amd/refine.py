"""Homography refinement against the segmentation: the second stage behind the ResNet-STN's regression.

    r = ThetaRefiner(court_img, mask_classes=4, grid_size=net.warp_size, factors=(4, 2, 1), iters=5)
    out = r(theta, logits)
    # out["theta"] (B,1,3,3) float32, out["cost"] (B,L,2) float64 [first, last per level], out["accepted"] (B,L) int32

Direct alignment of the court template to the UNet's class probabilities: per level of a coarse-to-fine pyramid, ``iters``
Levenberg-Marquardt steps on theta[0..7] (theta[8] is held).  The rule - planes, coordinates, cost, step - is stated once in
include/sfh_amd.h above the ``sfh_refine_*`` entries; csrc/refine.hip runs it, tests/refine_ref.py restates it in numpy.
The reference project has no counterpart: its predict() stops at the regressed theta.

A call launches on the caller's current stream, synchronises nothing and reads nothing back: 1 launch per level for the
evidence planes and 2 * (iters + 1) per level for the steps.  Template planes are built once per template tensor, on the stream
of the call that first needs them; a call on another stream waits for that build through an event.  Workspaces and state are
held once per (batch, logits size, stream); after the first call of a shape only the three small outputs are new tensors.
"""
import torch

from . import _lib
from .ops import _ptr, _stream, rows_all_equal

SUMS = _lib.ABI.defines["SFH_REFINE_SUMS"]


def _channels(nc):
    return 4 if nc <= 5 else 8


class ThetaRefiner:
    def __init__(self, court_img, mask_classes=4, grid_size=(640, 360), factors=(4, 2, 1), iters=5):
        """court_img (N,1,ht,wt) float32 valued k / mask_classes (one template, or one per frame); grid_size (W, H): the warp
        grid theta addresses (``net.warp_size``)"""
        if not torch.is_tensor(court_img) or court_img.dim() != 4 or court_img.shape[1] != 1 or court_img.dtype != torch.float32:
            raise ValueError("ThetaRefiner: court_img must be a float32 tensor (N,1,ht,wt)")
        nc, iters = int(mask_classes), int(iters)
        if not 2 <= nc <= 8:
            raise ValueError(f"ThetaRefiner: mask_classes={nc} (2..8)")
        if iters < 0:
            raise ValueError(f"ThetaRefiner: iters={iters} (>= 0)")
        factors = tuple(int(f) for f in factors)
        ht, wt = court_img.shape[2], court_img.shape[3]
        for f in factors:
            if not 1 <= f <= 64 or ht % f or wt % f:
                raise ValueError(f"ThetaRefiner: level {f} does not divide the template {wt}x{ht}")
        W, H = int(grid_size[0]), int(grid_size[1])
        if W < 2 or H < 2:
            raise ValueError(f"ThetaRefiner: grid_size {grid_size}")
        self.court_img, self.mask_classes, self.grid_size, self.factors, self.iters = court_img, nc, (W, H), factors, iters
        self._tmpl = None      # (key, shared, [planes per level], event behind their build, the stream that built them)
        self._work = {}        # (B, hl, wl, stream) -> buffers

    def __getstate__(self):
        """configuration only: planes, workspaces and state are rebuilt on first use"""
        st = self.__dict__.copy()
        st["_tmpl"], st["_work"] = None, {}
        return st

    # ------------------------------------------------------------------ cached device buffers
    def _template_planes(self):
        t = self.court_img
        key = (t.data_ptr(), tuple(t.shape), t._version)
        if self._tmpl is None or self._tmpl[0] != key:
            lib = _lib.load()
            tc = t.contiguous()
            shared = bool(tc.shape[0] == 1 or rows_all_equal(tc))
            n, ht, wt = (1 if shared else tc.shape[0]), tc.shape[2], tc.shape[3]
            planes = []
            for f in self.factors:
                p = torch.empty((n, ht // f, wt // f, _channels(self.mask_classes)), dtype=torch.float32, device=t.device)
                _lib.check(lib.sfh_refine_template_planes(_ptr(tc), n, ht, wt, self.mask_classes, f, _ptr(p), _stream()),
                           "refine_template_planes")
                planes.append(p)
            built = torch.cuda.Event()
            built.record()
            self._tmpl = (key, shared, planes, built, torch.cuda.current_stream(t.device).cuda_stream)
        elif self._tmpl[4] != torch.cuda.current_stream(t.device).cuda_stream:
            # built on another stream: this stream's launches go behind the build (an event wait, no host synchronisation)
            torch.cuda.current_stream(t.device).wait_event(self._tmpl[3])
        return self._tmpl[1], self._tmpl[2]

    def _buffers(self, B, hl, wl, dev):
        key = (B, hl, wl, dev, torch.cuda.current_stream(dev).cuda_stream)
        w = self._work.get(key)
        if w is None:
            lib = _lib.load()
            cp, fmin = _channels(self.mask_classes), min(self.factors)
            nbytes = lib.sfh_refine_workspace_bytes(B, hl // fmin, wl // fmin)
            if nbytes < 0:
                raise ValueError(f"ThetaRefiner: batch {B} (1..65535)")
            w = self._work[key] = {
                "ev": [torch.empty((B, hl // f, wl // f, cp), dtype=torch.float32, device=dev) for f in self.factors],
                "slabs": [lib.sfh_refine_workspace_bytes(B, hl // f, wl // f) // (B * SUMS * 8) for f in self.factors],
                "ws": torch.empty(nbytes // 8, dtype=torch.float64, device=dev), "ws_bytes": nbytes,
                "theta_acc": torch.empty((B, 9), dtype=torch.float32, device=dev),
                "cand": torch.empty((B, 9), dtype=torch.float32, device=dev),
                "sums": torch.empty((B, SUMS), dtype=torch.float64, device=dev),
                "lambda": torch.empty(B, dtype=torch.float64, device=dev),
                "ok": torch.empty(B, dtype=torch.int32, device=dev),
            }
        return w

    # ------------------------------------------------------------------ the call
    def _check(self, theta, logits, offset):
        if not (torch.is_tensor(theta) and torch.is_tensor(logits)):
            raise ValueError("ThetaRefiner: theta and logits must be tensors")
        if theta.dtype != torch.float32 or logits.dtype != torch.float32:
            raise ValueError(f"ThetaRefiner: float32 expected, got theta {theta.dtype}, logits {logits.dtype}")
        if logits.dim() != 4 or logits.shape[1] != self.mask_classes:
            raise ValueError(f"ThetaRefiner: logits must be (B,{self.mask_classes},hl,wl), got {tuple(logits.shape)}")
        B = logits.shape[0]
        if tuple(theta.shape) not in ((B, 1, 3, 3), (B, 3, 3)):
            raise ValueError(f"ThetaRefiner: theta must be ({B},1,3,3), got {tuple(theta.shape)}")
        hl, wl = logits.shape[2], logits.shape[3]
        for f in self.factors:
            if hl % f or wl % f:
                raise ValueError(f"ThetaRefiner: level {f} does not divide the logits {wl}x{hl}")
        if not (theta.is_cuda and logits.is_cuda and self.court_img.is_cuda):
            raise ValueError("ThetaRefiner: theta, logits and the court template must be CUDA tensors (there is no CPU path)")
        n = self.court_img.shape[0]
        if n == 1 or offset + B <= n:
            return
        with torch.cuda.device(logits.device):
            shared = self._template_planes()[0]
        if not shared:
            raise ValueError(f"ThetaRefiner: batch {offset + B} exceeds the court template batch {n}")

    def __call__(self, theta, logits, offset=0):
        """theta (B,1,3,3), logits (B,nc,hl,wl); offset: the first frame's row of a per-frame template batch"""
        self._check(theta, logits, offset)
        B, nc, hl, wl = logits.shape
        dev, L = logits.device, len(self.factors)
        out = {"theta": torch.empty((B, 1, 3, 3), dtype=torch.float32, device=dev),
               "cost": torch.empty((B, L, 2), dtype=torch.float64, device=dev),
               "accepted": torch.empty((B, L), dtype=torch.int32, device=dev)}
        if B == 0:
            return out
        with torch.cuda.device(dev):
            lib, st = _lib.load(), _stream()
            shared, tplanes = self._template_planes()
            w = self._buffers(B, hl, wl, dev)
            th, lg = theta.contiguous(), logits.contiguous()
            W, H = self.grid_size
            ht, wt = self.court_img.shape[2], self.court_img.shape[3]
            if L == 0:
                out["theta"].copy_(th.view(B, 1, 3, 3))
                return out
            for li, f in enumerate(self.factors):
                _lib.check(lib.sfh_refine_evidence_planes(_ptr(lg), B, nc, hl, wl, f, _ptr(w["ev"][li]), st), "refine_evidence_planes")
            cur = th
            for li, f in enumerate(self.factors):
                tp = tplanes[li] if shared else tplanes[li][offset:]
                bstride = 0 if shared else tp[0].numel()

                def accumulate(t):
                    _lib.check(lib.sfh_refine_accumulate(_ptr(t), _ptr(tp), bstride, ht, wt, _ptr(w["ev"][li]), B, nc, hl, wl, H, W, f,
                                                         _ptr(w["ws"]), w["ws_bytes"], st), "refine_accumulate")

                def step(first, last, t_eval, t_next):
                    _lib.check(lib.sfh_refine_step(_ptr(w["ws"]), w["slabs"][li], B, first, last, _ptr(t_eval), _ptr(w["theta_acc"]),
                                                   _ptr(w["sums"]), _ptr(w["lambda"]), _ptr(w["ok"]), _ptr(t_next), _ptr(out["cost"]),
                                                   _ptr(out["accepted"]), li, L, st), "refine_step")

                final = li == L - 1
                accumulate(cur)
                step(1, int(self.iters == 0), cur, out["theta"] if (final and self.iters == 0) else w["cand"])
                for it in range(self.iters):
                    end = it == self.iters - 1
                    accumulate(w["cand"])
                    step(0, int(end), w["cand"], out["theta"] if (final and end) else w["cand"])
                cur = w["cand"]
        return out
