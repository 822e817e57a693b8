"""sfh_amd.augment on the MI355X against ``augment.reference_apply`` (stock torch operators on the CPU).

The image bound is not a constant: per case the test computes, in the same run, E32 = max|reference(fp32) - reference(fp64)|
and demands max|gpu - reference(fp64)| <= 2 * E32 + 2^-22 over EVERY pixel (factor 2: a different but equally valid fp32
operation order - separable blur, fused blends; 2^-22 = four ulps at 1.0 for cases where fp32 torch happens to be exact).
mask, uv, poi and nonzeros must be equal element by element.  Every figure goes to profiles/augment_parity.jsonl when
SFH_AUG_PARITY_LOG names a file."""
import itertools
import json
import os

import pytest
import torch

from sfh_amd import augment as A

pytestmark = pytest.mark.gpu

SLACK = 2.0 ** -22
SIZES = {"640x360": (640, 360), "322x182": (322, 182)}
JIT = {'brightness': 0.35, 'contrast': 0.35, 'saturation': 0.25, 'hue': 0.25}
DEFAULT_CFG = {'apperance': {'jitter': dict(JIT), 'blur': 5}, 'geometric': {'hflip': 0.5}}
FULL_CFG = {'apperance': {'jitter': dict(JIT), 'blur': 5}, 'geometric': {'scale': [0.5, 1.0], 'hflip': 0.5}}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(kind, B, H, W, seed, npts=52):
    g = _gen(seed)
    if kind == "uniform":
        fr = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    elif kind == "gradient":      # smooth ramps with a different direction and phase per sample and channel
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        a = torch.rand(B, 1, 1, 3, generator=g, dtype=torch.float64)
        ph = torch.rand(B, 1, 1, 3, generator=g, dtype=torch.float64)
        t = (a * xx[None, :, :, None] / W + (1 - a) * yy[None, :, :, None] / H + ph) % 1.0
        fr = (255 * (0.5 - 0.5 * torch.cos(2 * torch.pi * t))).round().to(torch.uint8)
    else:                         # near-gray: |r - g|, |g - b| <= 2, the ill-conditioned side of the hue conversion
        base = torch.randint(2, 252, (B, H, W, 1), generator=g)
        d = torch.randint(-1, 2, (B, H, W, 3), generator=g)
        fr = (base + d).to(torch.uint8)
    mk = torch.randint(0, 4, (B, H, W), generator=g, dtype=torch.uint8)
    uv = torch.rand(B, 2, H, W, generator=g)
    uv[:, :, : H // 3] = 0.0
    poi = torch.rand(B, npts, 2, generator=g)
    nz = (torch.rand(B, npts, generator=g) > 0.3).float()
    return fr.contiguous(), mk, uv, poi, nz


def _rand_factors(p, g, ops):
    B = p.batch
    u = torch.rand(B, 4, generator=g)
    for op in ops:
        x = (0.35, 0.35, 0.25, 0.25)[op]
        p.factor[:, op] = (-x + 2 * x * u[:, op]) if op == A.HUE else (1 - x + 2 * x * u[:, op])
    p.enabled[:] = sum(1 << op for op in ops)


def _rand_crops(p, g, H, W):
    B = p.batch
    for b in range(B):
        if b % 4 == 0:           # in / out = 1 / 2: dst * scale lands on an integer at every even dst
            h, w = H // 2, W // 2
        elif b % 4 == 1:         # one pixel smaller than the frame
            h, w = H - 1, W - 1
        else:
            s = 0.5 + 0.5 * float(torch.rand(1, generator=g))
            h, w = max(1, round(H * s ** 0.5)), max(1, round(W * s ** 0.5))
        i = int(torch.randint(0, H - h + 1, (1,), generator=g))
        j = int(torch.randint(0, W - w + 1, (1,), generator=g))
        if b % 8 == 2:
            i, j = 0, 0          # touches the top and left edges
        if b % 8 == 6:
            i, j = H - h, W - w  # touches the bottom and right edges
        p.crop[b] = torch.tensor([i, j, h, w], dtype=torch.int32)


def _case(name, B, H, W, seed):
    """-> (aug config, AugParams, with_poi)"""
    g = _gen(seed)
    p = A.AugParams.identity(B, H, W)
    cfg = {'apperance': {'jitter': dict(JIT)}, 'geometric': {'hflip': 0.5}}
    if name in ("brightness", "contrast", "saturation", "hue"):
        _rand_factors(p, g, [("brightness", "contrast", "saturation", "hue").index(name)])
    elif name == "orders24":
        perms = list(itertools.permutations(range(4)))
        p.order = torch.tensor([perms[b % 24] for b in range(B)], dtype=torch.int8)
        _rand_factors(p, g, [0, 1, 2, 3])
    elif name.startswith("blur"):
        k, sigma = name[4:].split("_s")
        cfg = {'apperance': {'blur': int(k)}}
        p.sigma[:] = float(sigma)
    elif name == "crop":
        cfg = {'geometric': {'scale': [0.25, 1.0]}}
        _rand_crops(p, g, H, W)
    elif name == "flip":
        p.flip[:] = True
        p.flip[B // 2] = False
    elif name == "default":
        cfg = DEFAULT_CFG
        p = A.BatchAugment(cfg, target_size=(W, H)).sample(B, generator=g)
    elif name == "everything":
        cfg = FULL_CFG
        p = A.BatchAugment(cfg, target_size=(W, H)).sample(B, generator=g)
        p.flip[0] = True
        p.flip[B // 2] = B == 1
    elif name == "all_different":      # every sample its own order, factors, flags, sigma, crop
        cfg = FULL_CFG
        perms = list(itertools.permutations(range(4)))
        p.order = torch.tensor([perms[(5 * b + 3) % 24] for b in range(B)], dtype=torch.int8)
        _rand_factors(p, g, [0, 1, 2, 3])
        p.enabled = torch.tensor([(b * 7 + 1) % 16 for b in range(B)], dtype=torch.int32)
        p.sigma = torch.tensor([0.0 if b % 3 == 0 else 0.1 + 0.19 * (b % 11) for b in range(B)])
        _rand_crops(p, g, H, W)
        p.crop[0] = torch.tensor([0, 0, H, W], dtype=torch.int32)
        p.flip = torch.tensor([b % 2 == 1 for b in range(B)])
    else:
        raise KeyError(name)
    with_poi = 'scale' not in (cfg.get('geometric') or {})
    return cfg, p, with_poi


def _log(rec):
    path = os.environ.get("SFH_AUG_PARITY_LOG")
    print(json.dumps(rec), flush=True)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _run_case(name, kind, size, B, seed, region=None):
    W, H = SIZES[size] if isinstance(size, str) else size
    cfg, p, with_poi = _case(name, B, H, W, seed)
    fr, mk, uv, poi, nz = _inputs(kind, B, H, W, seed + 1)
    if not with_poi:
        poi = nz = None
    aug = A.BatchAugment(cfg, target_size=(W, H), use_uv=True)
    k = aug.blur or 1
    dev = lambda t: None if t is None else t.cuda()
    out = aug(dev(fr), dev(mk), poi=dev(poi), nonzeros=dev(nz), uv=dev(uv), params=p)
    again = aug(dev(fr), dev(mk), poi=dev(poi), nonzeros=dev(nz), uv=dev(uv), params=p)
    torch.cuda.synchronize()
    r64 = A.reference_apply(fr, mk, p, blur_k=k, poi=poi, nonzeros=nz, uv=uv, dtype=torch.float64)
    r32 = A.reference_apply(fr, mk, p, blur_k=k, poi=poi, nonzeros=nz, uv=uv, dtype=torch.float32)
    img = out['image'].cpu().double()
    assert out['image'].dtype == torch.float32 and out['image'].is_contiguous() and tuple(out['image'].shape) == (B, 3, H, W)
    assert out['mask'].dtype == torch.int64 and out['mask'].is_contiguous()
    regions = {"all": (slice(None), slice(None))}
    if region == "borders":
        r = k // 2
        regions.update(top=(slice(0, r), slice(None)), bottom=(slice(H - r, H), slice(None)),
                       left=(slice(None), slice(0, r)), right=(slice(None), slice(W - r, W)))
    failures = []
    for rn, (ys, xs) in regions.items():
        e32 = float((r32['image'].double() - r64['image'])[:, :, ys, xs].abs().max())
        err = float((img - r64['image'])[:, :, ys, xs].abs().max())
        m64, m32, mg = r64['contrast_mean'], r32['contrast_mean'].double(), aug.last_contrast_mean.cpu().double()
        me32, merr = float((m32 - m64).abs().max()), float((mg - m64).abs().max())
        _log({"case": name, "frames": kind, "size": f"{W}x{H}", "batch": B, "region": rn, "E32": e32, "gpu_err": err,
              "bound": 2 * e32 + SLACK, "mean_E32": me32, "mean_gpu_err": merr})
        if not err <= 2 * e32 + SLACK:
            failures.append(f"{rn}: image error {err:.3e} > 2 * {e32:.3e} + 2^-22")
        if not merr <= 2 * me32 + SLACK:
            failures.append(f"{rn}: contrast mean error {merr:.3e} > 2 * {me32:.3e} + 2^-22")
    assert not failures, (name, kind, size, failures)
    assert torch.equal(out['mask'].cpu(), r64['mask'])
    assert torch.equal(out['uv'].cpu(), r32['uv']) and torch.equal(r32['uv'], r64['uv'])
    if poi is not None:
        assert torch.equal(out['poi'].cpu(), r32['poi']) and torch.equal(out['nonzeros'].cpu(), r32['nonzeros'])
    for key in out:            # no atomics anywhere: two runs give the same bits
        assert torch.equal(out[key], again[key]), key


CASES = ["brightness", "contrast", "saturation", "hue", "orders24",
         "blur3_s0.1", "blur3_s2.0", "blur5_s0.1", "blur5_s2.0", "blur11_s0.1", "blur11_s2.0",
         "crop", "flip", "default", "everything"]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("size", list(SIZES))
def test_parity_uniform_frames(name, size):
    _run_case(name, "uniform", size, 24 if name == "orders24" else 16, seed=100 + CASES.index(name))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kind", ["gradient", "neargray"])
def test_parity_smooth_and_near_gray_frames(name, kind):
    _run_case(name, kind, "640x360", 24 if name == "orders24" else 4, seed=200 + CASES.index(name))


@pytest.mark.parametrize("name", ["blur3_s2.0", "blur5_s2.0", "blur11_s2.0", "blur11_s0.1"])
def test_blur_reflect_borders(name):
    """the outermost k / 2 rows and columns, each strip against its own E32"""
    _run_case(name, "uniform", "322x182", 3, seed=300, region="borders")
    _run_case(name, "gradient", "640x360", 2, seed=301, region="borders")


@pytest.mark.parametrize("B", [1, 13])
def test_every_sample_different_and_single_sample(B):
    _run_case("all_different", "uniform", "322x182", B, seed=400 + B)
    _run_case("everything", "neargray", "322x182", B, seed=430 + B)
    _run_case("all_different", "uniform", (64, 16), B, seed=410 + B)          # exactly one tile
    _run_case("all_different", "gradient", (65, 17), B, seed=420 + B)         # one pixel into the next tile


def test_crops_touching_each_edge():
    W, H = SIZES["322x182"]
    fr, mk, uv, _, _ = _inputs("uniform", 6, H, W, 500)
    p = A.AugParams.identity(6, H, W)
    p.sigma[:] = 1.3
    rects = [(0, 40, 100, 177), (H - 100, 40, 100, 177), (30, 0, 100, 177), (30, W - 177, 100, 177),
             (0, 0, H - 1, W - 1), (1, 1, H - 1, W - 1)]
    p.crop = torch.tensor(rects, dtype=torch.int32)
    p.flip[1::2] = True
    aug = A.BatchAugment({'apperance': {'blur': 5}, 'geometric': {'scale': [0.25, 1.0]}}, target_size=(W, H))
    out = aug(fr.cuda(), mk.cuda(), uv=uv.cuda(), params=p)
    r64 = A.reference_apply(fr, mk, p, blur_k=5, uv=uv, dtype=torch.float64)
    r32 = A.reference_apply(fr, mk, p, blur_k=5, uv=uv, dtype=torch.float32)
    for b in range(6):
        e32 = float((r32['image'][b].double() - r64['image'][b]).abs().max())
        err = float((out['image'][b].cpu().double() - r64['image'][b]).abs().max())
        _log({"case": f"edge_crop{rects[b]}", "E32": e32, "gpu_err": err})
        assert err <= 2 * e32 + SLACK, (rects[b], err, e32)
    assert torch.equal(out['mask'].cpu(), r64['mask']) and torch.equal(out['uv'].cpu(), r64['uv'])


def test_pitch_flip_map_and_poi():
    from conftest import GOLDEN
    W, H = 64, 32
    fr, mk, _, poi, nz = _inputs("uniform", 5, H, W, 600, npts=33)
    aug = A.BatchAugment({'geometric': {'hflip': 0.5, 'poi_flip_map': os.path.join(GOLDEN, "pitch-poi-flip-mapping.json")}},
                         target_size=(W, H))
    p = A.AugParams.identity(5, H, W)
    p.flip = torch.tensor([True, False, True, True, False])
    out = aug(fr.cuda(), mk.cuda(), poi=poi.cuda(), nonzeros=nz.cuda(), params=p)
    ref = A.reference_apply(fr, mk, p, poi=poi, nonzeros=nz, flip_map=aug.flip_map)
    assert torch.equal(out['poi'].cpu(), ref['poi']) and torch.equal(out['nonzeros'].cpu(), ref['nonzeros'])
    assert torch.equal(out['image'].cpu(), ref['image']) and torch.equal(out['mask'].cpu(), ref['mask'])
    assert 'uv' not in out


def test_feeds_train_step_directly():
    """out['image'] and out (+ the two per-sample entries augmentation does not touch) go into TrainStep as they are"""
    from sfh_amd import synth, training as T
    from sfh_amd.reconstructor import Reconstructor
    B, H, W = 4, 96, 128
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :H, :W].contiguous().cuda()
    cpoi = synth.load_court_poi("pitch", B).cuda()
    net = Reconstructor(court, cpoi, target_size=(W, H), unet_size=(W, H), warp_size=(W, H))
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 47))
    net.cuda().train()
    ts = T.TrainStep(net, lr=1e-4)
    from conftest import GOLDEN
    aug = A.BatchAugment({'apperance': DEFAULT_CFG['apperance'],
                          'geometric': {'hflip': 0.5, 'poi_flip_map': os.path.join(GOLDEN, "pitch-poi-flip-mapping.json")}},
                         target_size=(W, H))
    g = _gen(9)
    for it in range(2):
        fr, mk, _, poi, nz = _inputs("gradient", B, H, W, 700 + it, npts=int(cpoi.shape[1]))
        out = aug(fr.cuda(), mk.cuda(), poi=poi.cuda(), nonzeros=nz.cuda(), generator=g)
        batch = dict(out, weight=(torch.rand(B, generator=g) + 0.5).cuda(), num_nonzero=nz.sum(1).clamp(min=1.0).cuda())
        losses = ts.loss_and_grads(out['image'], batch) if it == 0 else ts.step(out['image'], batch)
        assert bool(torch.isfinite(losses).all()), losses


def test_non_default_stream_without_a_sync():
    W, H = SIZES["322x182"]
    cfg, p, _ = _case("everything", 8, H, W, 800)
    fr, mk, uv, _, _ = _inputs("uniform", 8, H, W, 801)
    aug = A.BatchAugment(cfg, target_size=(W, H), use_uv=True)
    want = aug(fr.cuda(), mk.cuda(), uv=uv.cuda(), params=p)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        frd, mkd, uvd = fr.cuda(non_blocking=True), mk.cuda(non_blocking=True), uv.cuda(non_blocking=True)
        filler = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):       # work queued in front on the same stream; nothing waits for it on the host
            filler = filler @ filler * 1e-4
        out = aug(frd, mkd, uv=uvd, params=p)
        consumer = out['image'].sum(dtype=torch.float64) + out['mask'].sum() + out['uv'].sum(dtype=torch.float64)
    s.synchronize()
    assert all(torch.equal(out[k], want[k]) for k in want)
    assert float(consumer) == float(want['image'].sum(dtype=torch.float64) + want['mask'].sum()
                                    + want['uv'].sum(dtype=torch.float64))
