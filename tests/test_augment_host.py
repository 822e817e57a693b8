"""Host side of sfh_amd.augment (no GPU): the sampling of AugParams, the CPU rule ``reference_apply`` and the argument
checks of ``BatchAugment``."""
import math
import os
import pickle

import pytest
import torch

from conftest import GOLDEN

from sfh_amd import augment as A

W, H = 64, 36
DEFAULT_CFG = {'apperance': {'jitter': {'brightness': 0.35, 'contrast': 0.35, 'saturation': 0.25, 'hue': 0.25}, 'blur': 5},
               'geometric': {'hflip': 0.5}}
FULL_CFG = {'apperance': {'jitter': {}, 'blur': 5}, 'geometric': {'scale': [0.5, 1.0], 'hflip': 0.5}}
PITCH_MAP = os.path.join(GOLDEN, "pitch-poi-flip-mapping.json")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _frames(B, h=H, w=W, seed=3):
    g = _gen(seed)
    return (torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 4, (B, h, w), generator=g, dtype=torch.uint8))


def _same(p, q):
    return all(torch.equal(getattr(p, f), getattr(q, f)) for f in ('order', 'factor', 'enabled', 'sigma', 'crop', 'flip'))


def test_sample_is_a_function_of_the_generator_state():
    aug = A.BatchAugment(FULL_CFG, target_size=(640, 360))
    p, q = aug.sample(32, generator=_gen(11)), aug.sample(32, generator=_gen(11))
    assert _same(p, q)
    assert not _same(p, aug.sample(32, generator=_gen(12)))
    assert _same(pickle.loads(pickle.dumps(p)), p)
    assert "order" in repr(p)
    p.validate(360, 640)


def test_sample_distributions():
    Wt, Ht = 640, 360
    aug = A.BatchAugment(FULL_CFG, target_size=(Wt, Ht))
    n = 4096
    p = aug.sample(n, generator=_gen(5))
    assert torch.equal(p.order.to(torch.int64).sort(dim=1).values, torch.arange(4).repeat(n, 1))
    assert len({tuple(r) for r in p.order.tolist()}) == 24            # all orders occur in 4096 draws
    for op, x in enumerate((0.35, 0.35, 0.25)):
        assert float(p.factor[:, op].min()) >= 1 - x and float(p.factor[:, op].max()) <= 1 + x
    assert float(p.factor[:, 3].abs().max()) <= 0.25
    assert bool((p.enabled == 15).all())
    assert float(p.sigma.min()) >= 0.1 and float(p.sigma.max()) <= 2.0
    i, j, h, w = (p.crop[:, k].to(torch.float64) for k in range(4))
    assert bool(((i >= 0) & (j >= 0) & (h > 0) & (w > 0) & (i + h <= Ht) & (j + w <= Wt)).all())
    # w = round(sqrt(area * ar)), h = round(sqrt(area / ar)): each within half a pixel of the exact side, so w against
    # h * W / H is off by at most 0.5 + 0.5 * W / H
    assert float((w - h * Wt / Ht).abs().max()) <= 0.5 + 0.5 * Wt / Ht
    # the area before rounding lies in scale * H * W; rounding each side by <= 0.5 changes it by <= (w + h) / 2 + 1 / 4
    frac_slack = ((w + h) / 2 + 0.25) / (Ht * Wt)
    frac = h * w / (Ht * Wt)
    assert bool((frac >= 0.5 - frac_slack).all()) and bool((frac <= 1.0 + frac_slack).all())
    assert float(frac.max() - frac.min()) > 0.4                        # the interval is used, not one value
    rate = float(p.flip.to(torch.float64).mean())
    assert abs(rate - 0.5) <= 4 * math.sqrt(0.25 / n)


def test_disabled_groups_give_identity_parameters():
    ident = A.AugParams.identity(8, H, W)
    p = A.BatchAugment({'apperance': None, 'geometric': {'hflip': 0.5}}, target_size=(W, H)).sample(8, generator=_gen(1))
    for f in ('order', 'factor', 'enabled', 'sigma', 'crop'):
        assert torch.equal(getattr(p, f), getattr(ident, f)), f
    p = A.BatchAugment({'apperance': {'blur': 3}}, target_size=(W, H)).sample(8, generator=_gen(1))
    for f in ('order', 'factor', 'enabled', 'crop', 'flip'):
        assert torch.equal(getattr(p, f), getattr(ident, f)), f
    assert bool((p.sigma > 0).all())
    # an amount of 0 switches that op off, as ColorJitter does
    p = A.BatchAugment({'apperance': {'jitter': {'hue': 0, 'contrast': 0}}}, target_size=(W, H)).sample(4, generator=_gen(1))
    assert bool((p.enabled == 0b0101).all())


def test_config_errors():
    with pytest.raises(ValueError):
        A.BatchAugment({'apperance': None, 'geometric': None})
    with pytest.raises(ValueError):
        A.BatchAugment({})
    for bad in (4, 13, 1, 5.0, [5, 5]):
        with pytest.raises(ValueError):
            A.BatchAugment({'apperance': {'blur': bad}})
    with pytest.raises(ValueError):
        A.BatchAugment({'geometric': {'scale': [0.5, 1.5]}})
    aug = A.BatchAugment({'apperance': {'jitter': None}})              # the reference's defaults
    assert aug.jitter == {'brightness': 0.35, 'contrast': 0.35, 'saturation': 0.25, 'hue': 0.25}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reference_identity(dtype):
    fr, mk = _frames(3)
    poi = torch.rand(3, 52, 2, generator=_gen(2))
    nz = (torch.rand(3, 52, generator=_gen(4)) > 0.3).float()
    out = A.reference_apply(fr, mk, A.AugParams.identity(3, H, W), blur_k=5, poi=poi, nonzeros=nz, dtype=dtype)
    assert out['image'].dtype == dtype
    assert torch.equal(out['image'], fr.permute(0, 3, 1, 2).to(dtype) / 255)
    assert torch.equal(out['mask'], mk.to(torch.int64)) and out['mask'].dtype == torch.int64
    assert torch.equal(out['poi'], poi) and torch.equal(out['nonzeros'], nz)


def test_reference_double_flip_is_identity():
    fr, mk = _frames(2)
    poi = torch.rand(2, 52, 2, generator=_gen(2))
    poi = torch.round(poi * 1024) / 1024                               # 1 - (1 - x) == x exactly on this grid
    nz = (torch.rand(2, 52, generator=_gen(4)) > 0.3).float()
    uv = torch.round(torch.rand(2, 2, H, W, generator=_gen(6)) * 254 + 1) / 256      # in (0, 1): u = 1 would flip to 0,
    uv[:, :, :5] = 0.0                                                 # the background value, which (u > 0) - u keeps
    p = A.AugParams.identity(2, H, W)
    p.flip[:] = True
    once = A.reference_apply(fr, mk, p, poi=poi, nonzeros=nz, uv=uv)
    assert not torch.equal(once['image'], fr.permute(0, 3, 1, 2).float() / 255)
    assert torch.equal(once['uv'][:, 1], uv[:, 1].flip(-1))
    assert torch.equal(once['uv'][:, 0], torch.where(uv[:, 0] > 0, 1 - uv[:, 0], uv[:, 0]).flip(-1))
    img_u8 = (once['image'] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    twice = A.reference_apply(img_u8, once['mask'].to(torch.uint8), p, poi=once['poi'], nonzeros=once['nonzeros'],
                              uv=once['uv'])
    assert torch.equal(twice['image'], fr.permute(0, 3, 1, 2).float() / 255)
    assert torch.equal(twice['mask'], mk.to(torch.int64))
    assert torch.equal(twice['poi'], poi) and torch.equal(twice['nonzeros'], nz)
    assert torch.equal(twice['uv'], uv)


def test_flip_maps_are_involutions_that_cover_every_point():
    import json
    for m, n in ((A.ncaa_flip_map(), 52), (json.load(open(PITCH_MAP))['hflip'], 33)):
        perm = A.flip_permutation(m, n)
        assert sorted(perm) == list(range(n))
        assert all(perm[perm[i]] == i for i in range(n))
    assert len(A.ncaa_flip_map()) == 28
    aug = A.BatchAugment({'geometric': {'hflip': 1.0, 'poi_flip_map': PITCH_MAP}}, target_size=(W, H))
    assert A.flip_permutation(aug.flip_map, 33)[0] == 27
    assert A.BatchAugment({'geometric': {'hflip': 1.0}}, poi_flip_map=[1, 0]).flip_map == [1, 0]


def test_uncovered_point_and_scale_with_poi_raise():
    with pytest.raises(ValueError, match="cover"):
        A.flip_permutation(A.ncaa_flip_map(), 53)
    with pytest.raises(ValueError):
        A.flip_permutation([1, 2, 0], 3)                               # not an involution
    with pytest.raises(ValueError):
        A.flip_permutation([5], 3)
    fr, mk = _frames(1)
    poi = torch.rand(1, 53, 2)
    aug = A.BatchAugment({'geometric': {'hflip': 0.5}}, target_size=(W, H))
    with pytest.raises(ValueError, match="cover"):
        aug(fr, mk, poi=poi, nonzeros=torch.ones(1, 53))
    aug = A.BatchAugment({'geometric': {'hflip': 0.5, 'scale': [0.5, 1.0]}}, target_size=(W, H))
    with pytest.raises(NotImplementedError):
        aug(fr, mk, poi=torch.rand(1, 52, 2), nonzeros=torch.ones(1, 52))
    p = A.AugParams.identity(1, H, W)
    p.crop[0] = torch.tensor([1, 1, H - 2, W - 2], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        A.reference_apply(fr, mk, p, poi=torch.rand(1, 52, 2))


def test_argument_checks_fire_without_a_gpu():
    aug = A.BatchAugment(DEFAULT_CFG, target_size=(W, H))
    fr, mk = _frames(2)
    with pytest.raises(ValueError):
        aug(fr.float(), mk)                                            # wrong dtype
    with pytest.raises(ValueError):
        aug(fr.permute(0, 3, 1, 2).contiguous(), mk)                   # NCHW instead of NHWC
    with pytest.raises(ValueError):
        aug(fr, mk.to(torch.int64))
    with pytest.raises(ValueError):
        aug(fr, mk[:1])
    with pytest.raises(ValueError):
        aug(fr, mk, uv=torch.zeros(2, 2, H, W + 1))
    with pytest.raises(ValueError):
        aug(fr, mk, poi=torch.rand(2, 52, 2).double(), nonzeros=torch.ones(2, 52))
    for field, value in (('crop', [0, 0, H + 1, W]), ('crop', [1, 0, H, W]), ('crop', [0, 0, 0, W]),
                         ('order', [0, 1, 1, 3]), ('factor', [float('nan'), 1, 1, 0]), ('factor', [1, 1, 1, 0.75])):
        p = aug.sample(2, generator=_gen(1))
        t = getattr(p, field)
        t[1] = torch.tensor(value, dtype=t.dtype)
        with pytest.raises(ValueError):
            aug(fr, mk, params=p)
    p = aug.sample(2, generator=_gen(1))
    p.sigma[0] = float('inf')
    with pytest.raises(ValueError):
        aug(fr, mk, params=p)
    with pytest.raises(ValueError):
        aug(fr, mk, params=aug.sample(3, generator=_gen(1)))           # batch mismatch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(fr, mk, params=aug.sample(2, generator=_gen(1)))           # valid arguments on CPU tensors: still no fallback


def test_library_argument_checks():
    from sfh_amd import _lib
    lib = _lib.load()
    assert lib.sfh_aug_workspace_doubles(16, 360) == 16 * 360
    assert lib.sfh_aug_workspace_doubles(0, 360) == -1
    assert lib.sfh_aug_gray_mean(None, None, 1, 8, 8, None, None) == -1
    assert lib.sfh_aug_apply(None, None, None, None, None, 1, 8, 8, 5, 0, None, None, None, None, None) == -1
    assert lib.sfh_aug_poi_flip(None, None, None, None, 1, 4, None, None, None) == -1
    with pytest.raises(ValueError):
        _lib.check(-1, "aug_apply")


def test_reference_ops_against_closed_forms():
    """A few values worked by hand pin the restatement itself (the torchvision comparison lives in test_augment_pins)."""
    px = torch.tensor([[[[255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128]]]], dtype=torch.uint8)   # (1,1,4,3)
    mk = torch.zeros(1, 1, 4, dtype=torch.uint8)
    p = A.AugParams.identity(1, 1, 4)
    p.enabled[0] = 1 << A.HUE
    p.factor[0, A.HUE] = 1.0 / 3                                       # red -> green -> blue -> red; gray stays
    out = A.reference_apply(px, mk, p, dtype=torch.float64)['image'][0]            # (3,1,4)
    want = torch.tensor([[0, 0, 1, 128 / 255], [1, 0, 0, 128 / 255], [0, 1, 0, 128 / 255]], dtype=torch.float64)
    assert float((out[:, 0] - want).abs().max()) < 1e-6
    p = A.AugParams.identity(1, 1, 4)
    p.enabled[0] = 1 << A.CONTRAST
    p.factor[0, A.CONTRAST] = 0.0                                      # everything becomes the gray mean
    out = A.reference_apply(px, mk, p, dtype=torch.float64)
    mean = (0.2989 + 0.587 + 0.114 + 128 / 255 * (0.2989 + 0.587 + 0.114)) / 4
    assert abs(float(out['contrast_mean'][0]) - mean) < 1e-12
    assert float((out['image'] - mean).abs().max()) < 1e-12
    # blur of a constant frame is the constant; of an impulse the normalised Gaussian (reflect padding untouched)
    fr = torch.zeros(1, 9, 9, 3, dtype=torch.uint8)
    fr[0, 4, 4] = 255
    p = A.AugParams.identity(1, 9, 9)
    p.sigma[0] = 1.0
    out = A.reference_apply(fr, torch.zeros(1, 9, 9, dtype=torch.uint8), p, blur_k=3, dtype=torch.float64)['image'][0, 0]
    e = math.exp(-0.5)
    k = torch.tensor([e, 1, e], dtype=torch.float64) / (1 + 2 * e)
    assert float((out[3:6, 3:6] - k[:, None] * k[None, :]).abs().max()) < 1e-12
    assert abs(float(out.sum()) - 1) < 1e-12
