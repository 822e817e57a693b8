"""``augment.reference_apply`` against torchvision.transforms.functional itself, op by op with explicit parameters, where
torchvision can be imported (like the Kornia / OpenCV pins: skipped where the package is absent)."""
import pytest
import torch

tvf = pytest.importorskip("torchvision.transforms.functional")

from sfh_amd import augment as A   # noqa: E402

H, W = 45, 80


def _data(B=3):
    g = torch.Generator().manual_seed(17)
    fr = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    mk = torch.randint(0, 4, (B, H, W), generator=g, dtype=torch.uint8)
    return fr, mk, fr.permute(0, 3, 1, 2).float() / 255


@pytest.mark.parametrize("op,fn,f", [(A.BRIGHTNESS, "adjust_brightness", 1.3), (A.CONTRAST, "adjust_contrast", 0.7),
                                     (A.SATURATION, "adjust_saturation", 1.2), (A.HUE, "adjust_hue", -0.21)])
def test_jitter_ops(op, fn, f):
    fr, mk, x = _data()
    p = A.AugParams.identity(3, H, W)
    p.enabled[:] = 1 << op
    p.factor[:, op] = f
    got = A.reference_apply(fr, mk, p)['image']
    f32 = float(torch.tensor(f, dtype=torch.float32))
    want = torch.stack([getattr(tvf, fn)(x[b], f32) for b in range(3)])
    assert torch.equal(got, want)


@pytest.mark.parametrize("k,sigma", [(3, 0.1), (5, 1.3), (11, 2.0)])
def test_gaussian_blur(k, sigma):
    fr, mk, x = _data()
    p = A.AugParams.identity(3, H, W)
    p.sigma[:] = sigma
    s32 = float(torch.tensor(sigma, dtype=torch.float32))
    got = A.reference_apply(fr, mk, p, blur_k=k)['image']
    want = torch.stack([tvf.gaussian_blur(x[b], [k, k], [s32, s32]) for b in range(3)])
    assert float((got - want).abs().max()) <= 2.0 ** -22


def test_resized_crop_and_flip():
    fr, mk, x = _data()
    p = A.AugParams.identity(3, H, W)
    p.crop = torch.tensor([[3, 5, 27, 48], [0, 0, H - 1, W - 1], [10, 20, 18, 32]], dtype=torch.int32)
    p.flip[:] = torch.tensor([True, False, True])
    out = A.reference_apply(fr, mk, p)
    for b in range(3):
        i, j, h, w = (int(v) for v in p.crop[b])
        img = tvf.resized_crop(x[b], i, j, h, w, [H, W], tvf.InterpolationMode.BILINEAR, antialias=False)
        m = tvf.resized_crop(mk[b][None], i, j, h, w, [H, W], tvf.InterpolationMode.NEAREST)[0]
        if bool(p.flip[b]):
            img, m = tvf.hflip(img), tvf.hflip(m)
        assert torch.equal(out['image'][b], img)
        assert torch.equal(out['mask'][b], m.to(torch.int64))
