"""Training augmentation of a whole batch on the HIP path: the reference's ``utils/augmentation.py``
(``apply_transforms``: torchvision ColorJitter, GaussianBlur, RandomResizedCrop, RandomHorizontalFlip and the uv / poi
flips) after the uint8 upload instead of per sample on DataLoader workers.

    aug = BatchAugment(cfg['aug'], target_size=(640, 360))
    params = aug.sample(B, generator=g)                     # host only: what will be done to each sample (AugParams)
    out = aug(frames_u8, masks_u8, poi=poi, nonzeros=nz, params=params)
    losses = step.step(out['image'], {**out, 'weight': w, 'num_nonzero': nnz})

Every random decision is drawn on the host with torchvision's ``get_params`` distributions (not its random stream) and is
shared by image, mask, uv and poi of a sample; the arithmetic runs in csrc/augment.hip in at most three launches per batch
with no host synchronisation.  ``reference_apply`` restates the same arithmetic with stock torch operators (on the CPU in the tests), in
fp32 or fp64: it is the yardstick of the tests and the written-down rule, never a fallback - a call on CPU tensors raises.

Assumed torchvision behaviour (transforms.functional's tensor path, 0.9 - 0.15): float images stay float through
adjust_hue; ``_blend`` = ``(f * a + (1 - f) * b).clamp(0, 1)``; contrast's mean is that of the whole gray frame;
GaussianBlur draws ONE sigma for both axes and pads with reflect; a uint8 mask is resized as float32 with mode='nearest'
(the legacy rule) and no antialiasing applies because a crop is never larger than the target.
"""
import ctypes
import dataclasses
import json
import math

import torch
import torch.nn.functional as F

from . import _lib

BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)
_JITTER_DEFAULTS = {'brightness': 0.35, 'contrast': 0.35, 'saturation': 0.25, 'hue': 0.25}    # augmentation.py:113-117
PARAM_WORDS = 16      # csrc/augment.hip: one block of 16 int32 words per sample


def ncaa_flip_map():
    """PoIHorizontalFlip.flipped_poi_mapping (augmentation.py:28-41): 28 pairs over the 52 NCAA court points."""
    m = list(range(4))
    m += [51 - i for i in range(4)]
    m += [45 - i for i in range(14)]
    m += [47 - i for i in range(2)]
    m += [31 - i for i in range(4)]
    return m


def flip_permutation(flip_map, npts):
    """The pair list of the reference (point i swaps with flip_map[i]) as a permutation of all ``npts`` points.  The
    reference leaves points the list does not cover uninitialised; here that, an index out of range and a list that is not
    an involution are a ValueError."""
    perm = [-1] * npts
    for i, j in enumerate(int(v) for v in flip_map):
        if not (0 <= j < npts and i < npts):
            raise ValueError(f"poi flip map: pair ({i}, {j}) outside the {npts} points")
        for a, c in ((i, j), (j, i)):
            if perm[a] not in (-1, c):
                raise ValueError(f"poi flip map: point {a} is paired with both {perm[a]} and {c}")
            perm[a] = c
    missing = [i for i, v in enumerate(perm) if v < 0]
    if missing:
        raise ValueError(f"poi flip map does not cover points {missing} of {npts}")
    return perm


@dataclasses.dataclass
class AugParams:
    """What is done to each sample of a batch (small CPU tensors): also the log of it.  ``order`` (B,4) int8: the jitter
    op of slot 0..3 (0 brightness, 1 contrast, 2 saturation, 3 hue); ``factor`` (B,4) fp32 indexed by OP; ``enabled`` (B,)
    int32, bit op set = that op runs; ``sigma`` (B,) fp32, 0 = no blur; ``crop`` (B,4) int32 i, j, h, w; ``flip`` (B,) bool."""
    order: torch.Tensor
    factor: torch.Tensor
    enabled: torch.Tensor
    sigma: torch.Tensor
    crop: torch.Tensor
    flip: torch.Tensor

    @property
    def batch(self):
        return int(self.order.shape[0])

    @staticmethod
    def identity(B, H, W):
        return AugParams(order=torch.arange(4, dtype=torch.int8).repeat(B, 1),
                         factor=torch.tensor([1.0, 1.0, 1.0, 0.0]).repeat(B, 1),
                         enabled=torch.zeros(B, dtype=torch.int32), sigma=torch.zeros(B),
                         crop=torch.tensor([0, 0, H, W], dtype=torch.int32).repeat(B, 1),
                         flip=torch.zeros(B, dtype=torch.bool))

    def validate(self, H, W):
        """Raises ValueError unless the block is one the kernels may be given (nothing here touches a device)."""
        B = self.batch
        want = {'order': ((B, 4), torch.int8), 'factor': ((B, 4), torch.float32), 'enabled': ((B,), torch.int32),
                'sigma': ((B,), torch.float32), 'crop': ((B, 4), torch.int32), 'flip': ((B,), torch.bool)}
        for name, (shape, dtype) in want.items():
            t = getattr(self, name)
            if not isinstance(t, torch.Tensor) or t.device.type != 'cpu' or tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError(f"AugParams.{name}: expected a CPU {dtype} tensor of shape {shape}")
        if B < 1:
            raise ValueError("AugParams: empty batch")
        if not torch.equal(self.order.to(torch.int64).sort(dim=1).values, torch.arange(4).repeat(B, 1)):
            raise ValueError("AugParams.order: every row must be a permutation of 0, 1, 2, 3")
        if not bool(torch.isfinite(self.factor).all()) or not bool(torch.isfinite(self.sigma).all()):
            raise ValueError("AugParams: non-finite factor / sigma")
        if bool((self.factor[:, :3] < 0).any()) or bool((self.factor[:, HUE].abs() > 0.5).any()):
            raise ValueError("AugParams.factor: brightness / contrast / saturation >= 0 and |hue| <= 0.5")
        if bool((self.sigma < 0).any()):
            raise ValueError("AugParams.sigma: negative")
        if bool(((self.enabled < 0) | (self.enabled > 15)).any()):
            raise ValueError("AugParams.enabled: a mask of the four op bits")
        i, j, h, w = (self.crop[:, k].to(torch.int64) for k in range(4))
        if bool(((h <= 0) | (w <= 0) | (i < 0) | (j < 0) | (i + h > H) | (j + w > W)).any()):
            raise ValueError(f"AugParams.crop: a rectangle of i, j, h, w outside the {W}x{H} frame or empty")

    def packed(self):
        """(B,16) int32: the parameter block the kernels read."""
        B = self.batch
        blk = torch.zeros((B, PARAM_WORDS), dtype=torch.int32)
        blk[:, 0:4] = self.order.to(torch.int32)
        blk[:, 4:8] = self.factor.contiguous().view(torch.int32)
        blk[:, 8] = self.enabled
        blk[:, 9] = self.sigma.contiguous().view(torch.int32)
        blk[:, 10:14] = self.crop
        blk[:, 14] = self.flip.to(torch.int32)
        return blk


def _parse_cfg(aug_cfg):
    """the reference's aug dict -> (jitter amounts or None, blur size or None, scale or None, hflip p or None, map path)"""
    if aug_cfg is None:
        raise ValueError("aug config is None: build no BatchAugment when there is no augmentation")
    app = aug_cfg.get('apperance')
    geo = aug_cfg.get('geometric')
    if app is None and geo is None:
        raise ValueError("aug['apperance'] and aug['geometric'] are both None (the reference asserts on it)")
    jitter = blur = scale = hflip = map_path = None
    if app is not None:
        if 'jitter' in app:
            jitter = dict(_JITTER_DEFAULTS)
            jitter.update({k: float(v) for k, v in (app['jitter'] or {}).items()})
            unknown = set(jitter) - set(_JITTER_DEFAULTS)
            if unknown:
                raise ValueError(f"aug['apperance']['jitter']: unknown keys {sorted(unknown)}")
            for k in ('brightness', 'contrast', 'saturation'):
                if jitter[k] < 0:
                    raise ValueError(f"jitter {k} must be non-negative")
            if not 0 <= jitter['hue'] <= 0.5:
                raise ValueError("jitter hue must be in [0, 0.5]")
        if 'blur' in app:
            blur = app['blur']
            if isinstance(blur, bool) or not isinstance(blur, int) or blur % 2 == 0 or not 3 <= blur <= 11:
                raise ValueError(f"aug['apperance']['blur'] = {blur!r}: one odd integer 3 .. 11")
        if jitter is None and blur is None:
            raise ValueError("aug['apperance'] is empty: set it to None to switch the group off")
    if geo is not None:
        if 'scale' in geo:
            lo, hi = (float(v) for v in geo['scale'])
            if not 0 < lo <= hi <= 1:
                raise ValueError(f"aug['geometric']['scale'] = {geo['scale']!r}: 0 < lo <= hi <= 1 (a crop never exceeds the frame)")
            scale = (lo, hi)
        if 'hflip' in geo:
            hflip = float(geo['hflip'])
            if not 0 <= hflip <= 1:
                raise ValueError("aug['geometric']['hflip'] is a probability")
        map_path = geo.get('poi_flip_map')
        if scale is None and hflip is None:
            raise ValueError("aug['geometric'] is empty: set it to None to switch the group off")
    return jitter, blur, scale, hflip, map_path


class BatchAugment:
    def __init__(self, aug_cfg, target_size=(640, 360), mask_classes=4, poi_flip_map=None, use_uv=False):
        self.jitter, self.blur, self.scale, self.hflip, map_path = _parse_cfg(aug_cfg)
        self.W, self.H = int(target_size[0]), int(target_size[1])
        if self.W < 1 or self.H < 1:
            raise ValueError(f"target_size {target_size!r}")
        if self.blur is not None and self.blur // 2 >= min(self.W, self.H):
            raise ValueError(f"blur {self.blur} needs a frame larger than {self.blur // 2} pixels (reflect padding)")
        self.mask_classes = int(mask_classes)
        self.use_uv = bool(use_uv)
        if poi_flip_map is None:
            poi_flip_map = map_path
        if poi_flip_map is None:
            self.flip_map = ncaa_flip_map()
        elif isinstance(poi_flip_map, (str, bytes)) or hasattr(poi_flip_map, '__fspath__'):
            with open(poi_flip_map, 'r') as f:
                self.flip_map = [int(v) for v in json.load(f)['hflip']]
        else:
            self.flip_map = [int(v) for v in poi_flip_map]
        self._perm_dev = {}       # (device, npts) -> int32 permutation on the device
        self._ws = None           # row partials of the contrast mean (grown on demand)
        self.last_params = None
        self.last_contrast_mean = None

    # ---- host: what will be done
    def sample(self, B, generator=None):
        """AugParams for ``B`` samples, drawn with torchvision's get_params distributions from ``generator`` (a CPU
        torch.Generator; None = the global one).  The same generator state gives the same AugParams."""
        B = int(B)
        if B < 1:
            raise ValueError("sample: B >= 1")
        H, W = self.H, self.W
        p = AugParams.identity(B, H, W)

        def rand(*shape):
            return torch.rand(*shape, generator=generator, dtype=torch.float64)

        if self.jitter is not None:
            p.order = torch.stack([torch.randperm(4, generator=generator) for _ in range(B)]).to(torch.int8)
            u = rand(B, 4)
            amounts = [self.jitter['brightness'], self.jitter['contrast'], self.jitter['saturation']]
            for op, x in enumerate(amounts):
                lo, hi = max(0.0, 1.0 - x), 1.0 + x
                p.factor[:, op] = (lo + (hi - lo) * u[:, op]).to(torch.float32).clamp_(lo, hi)
            h = self.jitter['hue']
            p.factor[:, HUE] = (-h + 2 * h * u[:, HUE]).to(torch.float32).clamp_(-h, h)
            bits = sum(1 << op for op, x in enumerate(amounts + [h]) if x > 0)     # ColorJitter skips an op whose amount is 0
            p.enabled = torch.full((B,), bits, dtype=torch.int32)
        if self.blur is not None:
            p.sigma = (0.1 + 1.9 * rand(B)).to(torch.float32).clamp_(0.1, 2.0)
        if self.scale is not None:
            # RandomResizedCrop.get_params with ratio = (W / H, W / H): ten tries, then the centre crop (here the frame)
            ar = W / float(H)
            ua, uo = rand(B, 10), rand(B, 2)
            for b in range(B):
                for t in range(10):
                    area = H * W * (self.scale[0] + (self.scale[1] - self.scale[0]) * float(ua[b, t]))
                    w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
                    if 0 < w <= W and 0 < h <= H:
                        i = min(int(float(uo[b, 0]) * (H - h + 1)), H - h)
                        j = min(int(float(uo[b, 1]) * (W - w + 1)), W - w)
                        p.crop[b] = torch.tensor([i, j, h, w], dtype=torch.int32)
                        break
        if self.hflip is not None:
            p.flip = rand(B) < self.hflip
        return p

    # ---- device
    def __call__(self, frames_u8, masks_u8, poi=None, nonzeros=None, uv=None, params=None, generator=None):
        """frames_u8 (B,H,W,3) uint8 and masks_u8 (B,H,W) uint8 on the device -> dict of fresh device tensors: image
        (B,3,H,W) fp32, mask (B,H,W) int64 and poi / nonzeros / uv when given."""
        H, W = self.H, self.W
        _check_inputs(frames_u8, masks_u8, poi, nonzeros, uv, H, W)
        B = int(frames_u8.shape[0])
        if poi is not None and self.scale is not None:
            raise NotImplementedError("aug['geometric']['scale'] with poi (the reference's make_points_transform raises too)")
        if self.use_uv and uv is None:
            raise ValueError("use_uv=True but no uv given")
        perm = None
        if poi is not None:
            perm = flip_permutation(self.flip_map, int(poi.shape[1]))
        if params is None:
            params = self.sample(B, generator=generator)
        if params.batch != B:
            raise ValueError(f"AugParams for {params.batch} samples, batch of {B}")
        params.validate(H, W)
        k = self.blur if self.blur is not None else 1
        if self.blur is None and bool((params.sigma > 0).any()):
            raise ValueError("AugParams.sigma > 0 but the config has no blur size")
        dev = frames_u8.device
        if dev.type != 'cuda':
            raise RuntimeError(f"BatchAugment: device {dev} - the HIP path has no CPU fallback (reference_apply is the CPU rule)")
        for name, t in (('masks_u8', masks_u8), ('poi', poi), ('nonzeros', nonzeros), ('uv', uv)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} on {t.device}, frames on {dev}")
        from .engine import _ptr, _stream
        lib = _lib.load()
        with torch.cuda.device(dev):
            st = _stream()
            blk = params.packed().pin_memory().to(dev, non_blocking=True)
            image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
            mask = torch.empty((B, H, W), dtype=torch.int64, device=dev)
            uv_out = torch.empty_like(uv) if uv is not None else None
            mean = torch.empty((B,), dtype=torch.float32, device=dev)
            ws = None
            if bool(((params.enabled >> CONTRAST) & 1).any()):
                need = lib.sfh_aug_workspace_doubles(B, H)
                if need < 0:
                    raise ValueError(f"BatchAugment: batch of {B} frames of {W}x{H} is not supported")
                if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                    self._ws = torch.empty((need,), dtype=torch.float64, device=dev)
                ws = self._ws
                _lib.check(lib.sfh_aug_gray_mean(_ptr(frames_u8), _ptr(blk), B, H, W, _ptr(ws), st), "aug_gray_mean")
            _lib.check(lib.sfh_aug_apply(_ptr(frames_u8), _ptr(masks_u8), _ptr(uv), _ptr(blk), _ptr(ws), B, H, W, k,
                                         int(uv.shape[1]) if uv is not None else 0, _ptr(image), _ptr(mask), _ptr(uv_out),
                                         _ptr(mean), st), "aug_apply")
            out = {'image': image, 'mask': mask}
            if uv is not None:
                out['uv'] = uv_out
            if poi is not None:
                N = int(poi.shape[1])
                key = (dev, N, tuple(perm))
                if key not in self._perm_dev:
                    self._perm_dev = {key: torch.tensor(perm, dtype=torch.int32).to(dev)}
                poi_out = torch.empty_like(poi)
                nz_out = torch.empty_like(nonzeros) if nonzeros is not None else None
                _lib.check(lib.sfh_aug_poi_flip(_ptr(poi), _ptr(nonzeros), _ptr(self._perm_dev[key]), _ptr(blk), B, N,
                                                _ptr(poi_out), _ptr(nz_out), st), "aug_poi_flip")
                out['poi'] = poi_out
                if nonzeros is not None:
                    out['nonzeros'] = nz_out
        self.last_params = params
        self.last_contrast_mean = mean
        return out


def _check_inputs(frames, masks, poi, nonzeros, uv, H, W):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 \
            or tuple(frames.shape[1:]) != (H, W, 3) or not frames.is_contiguous():
        raise ValueError(f"frames_u8: expected a contiguous uint8 tensor (B,{H},{W},3), got "
                         f"{getattr(frames, 'dtype', type(frames))} {tuple(getattr(frames, 'shape', ()))}")
    B = int(frames.shape[0])
    if B < 1:
        raise ValueError("frames_u8: empty batch")
    if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or tuple(masks.shape) != (B, H, W) \
            or not masks.is_contiguous():
        raise ValueError(f"masks_u8: expected a contiguous uint8 tensor ({B},{H},{W}), got "
                         f"{getattr(masks, 'dtype', type(masks))} {tuple(getattr(masks, 'shape', ()))}")
    if poi is not None:
        if poi.dtype != torch.float32 or poi.dim() != 3 or poi.shape[0] != B or poi.shape[2] != 2 or not poi.is_contiguous():
            raise ValueError(f"poi: expected a contiguous float32 tensor ({B},N,2), got {poi.dtype} {tuple(poi.shape)}")
        if nonzeros is not None and (nonzeros.dtype != torch.float32 or tuple(nonzeros.shape) != tuple(poi.shape[:2])
                                     or not nonzeros.is_contiguous()):
            raise ValueError(f"nonzeros: expected a contiguous float32 tensor {tuple(poi.shape[:2])}, got {nonzeros.dtype} "
                             f"{tuple(nonzeros.shape)}")
    elif nonzeros is not None:
        raise ValueError("nonzeros without poi")
    if uv is not None and (uv.dtype != torch.float32 or uv.dim() != 4 or uv.shape[0] != B or tuple(uv.shape[2:]) != (H, W)
                           or not 1 <= uv.shape[1] <= 8 or not uv.is_contiguous()):
        raise ValueError(f"uv: expected a contiguous float32 tensor ({B},C,{H},{W}) with 1 .. 8 channels, got {uv.dtype} "
                         f"{tuple(uv.shape)}")


# ---- the rule, restated with stock torch operators on the CPU (torchvision.transforms.functional's tensor path)

def _gray(x):
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)


def _blend(a, b, ratio):
    return (ratio * a + (1.0 - ratio) * b).clamp(0, 1.0)


def _rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=img.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def _gaussian_kernel1d(k, sigma, dtype, device=None):
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=dtype, device=device)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def reference_apply(frames_u8, masks_u8, params, blur_k=1, poi=None, nonzeros=None, uv=None, flip_map=None,
                    dtype=torch.float32):
    """Steps 1-4 of the augmentation with plain torch ops in ``dtype`` (fp32: torchvision's own arithmetic; fp64: the
    yardstick) on the device of the inputs: CPU tensors in the tests; profiles/augment_throughput.py times the same ops on
    the GPU as the stand-in for what a user would write without the kernels.  ``params`` stays on the host.  Returns image (B,3,H,W) ``dtype``, mask (B,H,W) int64, contrast_mean (B,) ``dtype`` (0 where
    contrast is off) and poi / nonzeros / uv when given (in their own dtypes)."""
    B, H, W = int(frames_u8.shape[0]), int(frames_u8.shape[1]), int(frames_u8.shape[2])
    _check_inputs(frames_u8, masks_u8, poi, nonzeros, uv, H, W)
    dev = frames_u8.device
    if params.batch != B:
        raise ValueError(f"AugParams for {params.batch} samples, batch of {B}")
    params.validate(H, W)
    if blur_k % 2 == 0 or not 1 <= blur_k <= 11:
        raise ValueError(f"blur_k = {blur_k}: odd, 1 .. 11")
    perm = None
    if poi is not None:
        if bool((params.crop != torch.tensor([0, 0, H, W], dtype=torch.int32)).any()):
            raise NotImplementedError("a crop together with poi (the reference's make_points_transform raises too)")
        perm = torch.tensor(flip_permutation(ncaa_flip_map() if flip_map is None else flip_map, int(poi.shape[1])), device=dev)
    images, masks, uvs, means = [], [], [], []
    poi_out = poi.clone() if poi is not None else None
    nz_out = nonzeros.clone() if nonzeros is not None else None
    for b in range(B):
        x = frames_u8[b].permute(2, 0, 1).to(dtype) / 255
        mean_b = torch.zeros((), dtype=dtype, device=dev)
        for slot in range(4):
            op = int(params.order[b, slot])
            if not (int(params.enabled[b]) >> op) & 1:
                continue
            f = float(params.factor[b, op])
            if op == BRIGHTNESS:
                x = _blend(x, torch.zeros_like(x), f)
            elif op == CONTRAST:
                m = torch.mean(_gray(x), dim=(-3, -2, -1), keepdim=True)
                mean_b = m.reshape(())
                x = _blend(x, m, f)
            elif op == SATURATION:
                x = _blend(x, _gray(x), f)
            else:
                hsv = _rgb2hsv(x)
                h, s, v = hsv.unbind(dim=-3)
                h = (h + f) % 1.0
                x = _hsv2rgb(torch.stack((h, s, v), dim=-3))
        sigma = float(params.sigma[b])
        if sigma > 0 and blur_k > 1:
            k1 = _gaussian_kernel1d(blur_k, sigma, dtype, dev)
            k2 = torch.mm(k1[:, None], k1[None, :])
            pad = blur_k // 2
            xp = F.pad(x[None], [pad, pad, pad, pad], mode='reflect')
            x = F.conv2d(xp, k2.expand(3, 1, blur_k, blur_k), groups=3)[0]
        i, j, h, w = (int(v) for v in params.crop[b])
        m = masks_u8[b]
        u = uv[b] if uv is not None else None
        if (i, j, h, w) != (0, 0, H, W):
            x = F.interpolate(x[None, :, i:i + h, j:j + w], size=(H, W), mode='bilinear', align_corners=False)[0]
            m = torch.round(F.interpolate(m[None, None, i:i + h, j:j + w].to(torch.float32), size=(H, W),
                                          mode='nearest'))[0, 0].to(torch.uint8)
            if u is not None:
                u = F.interpolate(u[None, :, i:i + h, j:j + w], size=(H, W), mode='nearest')[0]
        if bool(params.flip[b]):
            x = x.flip(-1)
            m = m.flip(-1)
            if u is not None:
                u = u.flip(-1).clone()
                u[0] = torch.gt(u[0], 0).type(u.type()) - u[0]
            if poi is not None:
                poi_out[b, :, 0] = 1.0 - poi[b, perm, 0]
                poi_out[b, :, 1] = poi[b, perm, 1]
                if nonzeros is not None:
                    nz_out[b] = nonzeros[b, perm]
        images.append(x)
        masks.append(m.to(torch.int64))
        means.append(mean_b)
        if u is not None:
            uvs.append(u)
    out = {'image': torch.stack(images).contiguous(), 'mask': torch.stack(masks).contiguous(),
           'contrast_mean': torch.stack(means)}
    if uv is not None:
        out['uv'] = torch.stack(uvs).contiguous()
    if poi is not None:
        out['poi'] = poi_out
        if nonzeros is not None:
            out['nonzeros'] = nz_out
    return out
