"""eval_reconstructor on the HIP path (sfh_amd.evaluation, csrc/eval.hip) against an fp64 restatement of eval.py:142-234
that runs on the SAME float32 tensors the GPU scored (the net's outputs copied to the CPU)."""
import ctypes
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from oracle import train_ref
from sfh_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

KEYS = ("val_seg_score", "val_rec_score", "val_uv_score", "val_reproj_score", "val_reproj_px", "val_consist_score")
RTOL, ATOL = 1e-5, 1e-9


def _close(got, want, what, rtol=RTOL):
    worst = 0.0
    for k in KEYS:
        d = abs(got[k] - want[k])
        worst = max(worst, d / max(abs(want[k]), 1e-30))
        assert d <= rtol * abs(want[k]) + ATOL, (what, k, got[k], want[k])
    print(f"{what}: max relative difference {worst:.2e}")


# ------------------------------------------------------------------ the oracle
def _oracle_batch(b, o, nc, target_size, weighted):
    """one batch of eval.py:168-215 in fp64 over the float32 tensors: dict of the six per-batch terms (reproj as 'sum')"""
    tw, th = target_size
    out = dict.fromkeys(KEYS, 0.0)
    g = b["mask"].long()
    w = b["weight"].double()
    L = o.get("logits")
    v = o.get("warp_mask")
    if L is not None:
        L = L.double()
        ce = F.cross_entropy(L, g, reduction="none")
        out["val_seg_score"] = (train_ref.per_sample_weighted(ce, w) if weighted else F.cross_entropy(L, g)).item()
    if v is not None:
        gf = g.to(torch.float32) / float(nc)
        rec = (v.double() - gf.double()) ** 2
        out["val_rec_score"] = (train_ref.per_sample_weighted(rec, w) if weighted else rec.mean()).item()
    if L is not None and v is not None:
        out["val_consist_score"] = F.cross_entropy(L, (v * nc).to(torch.long)).item()
    if o.get("uv") is not None:
        m = (o["uv"].double() - b["uv"].double()) ** 2
        out["val_uv_score"] = (train_ref.per_sample_weighted(m, w) if weighted else m.mean()).item()
    if "poi" in b and o.get("poi") is not None:
        B = b["poi"].shape[0]
        nz, nnz = b["nonzeros"].double(), b["num_nonzero"].double()
        out["val_reproj_score"] = train_ref.reprojection_loss(o["poi"].double(), b["poi"].double(), nz, nnz).item() * B
        s = torch.tensor([float(tw), float(th)], dtype=torch.float32)      # eval.py:209-212 scales in fp32
        out["val_reproj_px"] = train_ref.reprojection_loss((o["poi"] * s).double(), (b["poi"] * s).double(), nz, nnz).item() * B
    return out


def _oracle(batches, outs, nc, target_size, weighted):
    tot = dict.fromkeys(KEYS, 0.0)
    counter = 0
    for b, o in zip(batches, outs):
        counter += b["image"].shape[0]
        for k, val in _oracle_batch(b, o, nc, target_size, weighted).items():
            tot[k] += val
    n_val = len(batches)
    return {k: tot[k] / (counter if k in ("val_reproj_score", "val_reproj_px") else n_val) for k in KEYS}


# ------------------------------------------------------------------ kernel level
def _kernel(logits, mask, warp, weight, nc, poi=None, gt=None, nz=None, nnz=None, target=(1.0, 1.0)):
    from sfh_amd import _lib
    from sfh_amd import evaluation as ev
    from sfh_amd.engine import _ptr, _stream
    lib = _lib.load()
    B, H, W = mask.shape
    buf = torch.zeros(ev.SLOTS + 1, dtype=torch.float64, device="cuda")
    ws = torch.full((lib.sfh_eval_workspace_doubles(B, H, W),), float("nan"), dtype=torch.float64, device="cuda")
    c = lambda t: t.cuda().contiguous() if t is not None else None   # noqa: E731
    keep = [c(t) for t in (logits, mask, warp, weight, poi, gt, nz, nnz)]
    _lib.check(lib.sfh_eval_batch(_ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), nc, B, H, W, _ptr(keep[4]),
                                  _ptr(keep[5]), _ptr(keep[6]), _ptr(keep[7]), 0 if poi is None else poi.shape[1],
                                  float(target[0]), float(target[1]), _ptr(ws), ctypes.c_void_p(buf.data_ptr() + 8 * ev.SLOTS),
                                  ctypes.c_void_p(buf.data_ptr()), _stream()), "eval_batch")
    torch.cuda.synchronize()
    a = buf.cpu()
    return a, {"val_seg_score": a[ev.SEG].item(), "val_rec_score": a[ev.REC].item(), "val_uv_score": 0.0,
               "val_reproj_score": a[ev.REPROJ].item(), "val_reproj_px": a[ev.REPROJ_PX].item(),
               "val_consist_score": a[ev.CONSIST].item()}


def _random_inputs(B, H, W, nc, seed, npts=13):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, nc, H, W, generator=g) * 3
    hot = torch.rand(B, H, W, generator=g) < 0.05                     # +-80: lse stability
    sign = torch.where(torch.rand(B, H, W, generator=g) < 0.5, -80.0, 80.0)
    logits[:, 0] = torch.where(hot, sign, logits[:, 0])
    logits[:, nc - 1] = torch.where(hot, -sign, logits[:, nc - 1])
    mask = torch.randint(0, nc, (B, H, W), generator=g)
    mask[torch.rand(B, H, W, generator=g) < 0.1] = -100               # ignore_index pixels
    mask.view(-1)[0] = 0                                               # at least one counted pixel
    # warp values on and next to the class boundaries k/nc: pin trunc(fp32(v * nc))
    edges = []
    for k in range(nc):
        e = torch.tensor(k / nc, dtype=torch.float32)
        edges += [e, torch.nextafter(e, torch.tensor(2.0)), torch.nextafter(e, torch.tensor(-1.0))]
    edges = torch.stack(edges)
    warp = torch.rand(B, H, W, generator=g) * 0.999
    pick = torch.rand(B, H, W, generator=g) < 0.3
    warp = torch.where(pick, edges[torch.randint(0, len(edges), (B, H, W), generator=g)], warp).contiguous()
    weight = torch.rand(B, generator=g) + 0.5
    poi = torch.rand(B, npts, 2, generator=g) * 2 - 1
    gt = torch.rand(B, npts, 2, generator=g) * 2 - 1
    nz = (torch.rand(B, npts, generator=g) > 0.3).float()
    nnz = nz.sum(1).clamp(min=1.0)
    return logits, mask, warp, weight, poi, gt, nz, nnz


@pytest.mark.parametrize("B,H,W,nc", [(1, 1, 1, 4), (3, 37, 61, 7), (16, 37, 61, 4), (3, 36, 64, 7), (16, 20, 640, 4),
                                      (1, 9, 12, 1), (3, 5, 8, 8)])
@pytest.mark.parametrize("weighted", [True, False])
def test_kernel_on_random_tensors(B, H, W, nc, weighted):
    logits, mask, warp, weight, poi, gt, nz, nnz = _random_inputs(B, H, W, nc, seed=B * 1000 + H * 7 + W + nc)
    if nc == 1:
        mask.clamp_(max=0)
        warp.mul_(0.5)
    acc, got = _kernel(logits, mask, warp, weight if weighted else None, nc, poi, gt, nz, nnz, target=(640.0, 360.0))
    want = _oracle_batch({"mask": mask, "weight": weight, "poi": gt, "nonzeros": nz, "num_nonzero": nnz},
                         {"logits": logits, "warp_mask": warp, "poi": poi}, nc, (640, 360), weighted)
    from sfh_amd import evaluation as ev
    assert acc[ev.BAD].item() == 0 and acc[ev.FRAMES].item() == B
    _close(got, want, f"kernel B={B} {W}x{H} nc={nc} weighted={weighted}")


def test_kernel_without_logits_or_warp():
    """a net without UNet (no logits) or without warper: the remaining scores alone"""
    logits, mask, warp, weight, *_ = _random_inputs(3, 17, 24, 4, seed=5)
    _, got = _kernel(None, mask.clamp(min=0), warp, weight, 4)
    want = _oracle_batch({"mask": mask.clamp(min=0), "weight": weight}, {"warp_mask": warp}, 4, (24, 17), True)
    _close(got, want, "warp only")
    _, got = _kernel(logits, mask, None, None, 4)
    want = _oracle_batch({"mask": mask, "weight": weight}, {"logits": logits}, 4, (24, 17), False)
    _close(got, want, "logits only")


def test_kernel_flags_bad_classes_without_fault():
    from sfh_amd import evaluation as ev
    logits, mask, warp, weight, *_ = _random_inputs(2, 9, 16, 4, seed=9)
    bad_warp = warp.clone()
    bad_warp[1, 4, 7] = float("nan")
    acc, _ = _kernel(logits, mask, bad_warp, weight, 4)
    assert int(acc[ev.BAD].item()) == 2
    bad_mask = mask.clone()
    bad_mask[0, 2, 3] = 4
    acc, _ = _kernel(logits, bad_mask, warp, weight, 4)
    assert int(acc[ev.BAD].item()) == 1
    acc, _ = _kernel(logits, mask, warp, weight, 4)
    assert int(acc[ev.BAD].item()) == 0


# ------------------------------------------------------------------ end to end
def _net(W, H, B, seed, nearest=True, uv=False, precision=None, dev="cuda"):
    from sfh_amd.reconstructor import Reconstructor
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :H, :W].contiguous()
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.to(dev), poi.to(dev), target_size=(W, H), unet_size=(W, H), warp_size=(W, H),
                        warp_with_nearest=nearest, unet_uv=uv)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed))
    if precision:
        net.precision = precision
    return net.to(dev).train()


def _loader(sizes, H, W, npts, seed, uv=False):
    out = []
    for i, B in enumerate(sizes):
        g = torch.Generator().manual_seed(seed + i)
        b = {"image": synth.smooth_frames(B, H, W, seed=seed + i),
             "mask": torch.randint(0, 4, (B, H, W), generator=g),
             "weight": torch.rand(B, generator=g) + 0.5,
             "poi": torch.rand(B, npts, 2, generator=g) * 2 - 1,
             "nonzeros": (torch.rand(B, npts, generator=g) > 0.3).float()}
        b["mask"][torch.rand(B, H, W, generator=g) < 0.02] = -100
        b["num_nonzero"] = b["nonzeros"].sum(1).clamp(min=1.0)
        if uv:
            b["uv"] = torch.rand(B, 2, H, W, generator=g)
        out.append(b)
    return out


def _outputs(net, loader):
    """the eval-mode forward of every batch, on the CPU (the tensors the scores are computed from)"""
    net.eval()
    outs = []
    with torch.no_grad():
        for b in loader:
            p = net(b["image"].cuda())
            outs.append({k: v.cpu() for k, v in p.items()})
    net.train()
    return outs


def _check_e2e(net, loader, weighted, W, H, what):
    from sfh_amd.evaluation import eval_reconstructor
    res = eval_reconstructor(net, loader, "cuda", (W, H), use_per_sample_weights=weighted)
    assert net.training
    rescales = net.range_rescales
    outs = _outputs(net, loader)
    assert net.range_rescales == rescales
    for k in KEYS:
        assert isinstance(res[k], float)
    last = outs[-1]
    assert torch.equal(res["imgs"], loader[-1]["image"]) and res["imgs"].device.type == "cpu"
    assert torch.equal(res["logits"], last["logits"]) and tuple(res["logits"].shape) == (loader[-1]["image"].shape[0], 4, H, W)
    assert torch.equal(res["warp_masks"], last["warp_mask"]) and res["warp_masks"].dtype == torch.float32
    assert ("uv_masks" in res) == net.unet_uv
    if net.unet_uv:
        assert torch.equal(res["uv_masks"], last["uv"])
    _close(res, _oracle(loader, outs, 4, (W, H), weighted), what)
    return res


@pytest.mark.parametrize("weighted,nearest,precision", [(True, True, "f16x3"), (False, False, "f16x3"),
                                                        (True, False, "f16x3"), (False, True, "bf16x6")])
def test_end_to_end_640x360(weighted, nearest, precision):
    W, H = 640, 360
    net = _net(W, H, 16, seed=31, nearest=nearest, precision=precision)
    loader = _loader([16, 16, 5], H, W, net.court_poi.shape[1], seed=300)
    _check_e2e(net, loader, weighted, W, H, f"e2e weighted={weighted} nearest={nearest} {precision}")


def test_end_to_end_uv_head():
    """unet_uv=True: weighted with batches of one frame (the reference's broadcast rule: B == 1 or B == W) and unweighted"""
    W, H = 640, 360
    net = _net(W, H, 16, seed=37, uv=True)
    _check_e2e(net, _loader([1, 1], H, W, net.court_poi.shape[1], seed=400, uv=True), True, W, H, "uv weighted B=1")
    _check_e2e(net, _loader([16, 5], H, W, net.court_poi.shape[1], seed=410, uv=True), False, W, H, "uv unweighted")
    from sfh_amd.evaluation import eval_reconstructor
    with pytest.raises(ValueError, match="broadcast"):         # B = 5 weights against a (5, 640) loss map
        eval_reconstructor(net, _loader([5], H, W, net.court_poi.shape[1], seed=420, uv=True), "cuda", (W, H))
    assert net.training


def test_deterministic_scores():
    from sfh_amd.evaluation import eval_reconstructor
    W, H = 640, 360
    net = _net(W, H, 16, seed=41)
    loader = _loader([16, 16, 5], H, W, net.court_poi.shape[1], seed=500)
    a = eval_reconstructor(net, loader, "cuda", (W, H))
    r = net.range_rescales
    b = eval_reconstructor(net, loader, "cuda", (W, H))
    assert net.range_rescales == r, "a range event between the calls changes the forward's bits"
    for k in KEYS:
        assert a[k] == b[k], (k, a[k], b[k])
    assert torch.equal(a["logits"], b["logits"])


def test_bad_inputs_raise():
    from sfh_amd.evaluation import eval_reconstructor
    W, H = 96, 64
    net = _net(W, H, 4, seed=43)
    loader = _loader([4, 4], H, W, net.court_poi.shape[1], seed=600)
    loader[0]["mask"][1, 5, 9] = 4                      # class id nc
    with pytest.raises(ValueError, match="mask"):
        eval_reconstructor(net, loader, "cuda", (W, H))
    assert net.training
    with pytest.raises(ValueError, match="empty"):
        eval_reconstructor(net, [], "cuda", (W, H))
    with pytest.raises(ValueError, match="warp_size"):
        eval_reconstructor(net, loader, "cuda", (W // 2, H // 2))
    loader[0]["mask"][1, 5, 9] = 0                      # the same net evaluates cleanly afterwards
    res = eval_reconstructor(net, loader, "cuda", (W, H))
    assert all(res[k] == res[k] for k in KEYS)


def test_eval_between_training_steps():
    """TrainStep.step -> eval_reconstructor -> TrainStep.step: eval sees the updated weights (a fresh eval-mode model with
    net.state_dict() scores the same within 1e-4), and the second step runs."""
    from sfh_amd import training
    from sfh_amd.evaluation import eval_reconstructor
    W, H, B = 128, 96, 4
    net = _net(W, H, B, seed=47)
    loader = _loader([4, 3], H, W, net.court_poi.shape[1], seed=700)
    for b in loader:
        b["mask"].clamp_(min=0)                         # the training losses take class ids only
    tb = {k: v.cuda() for k, v in loader[0].items() if k != "image"}
    x = loader[0]["image"].cuda()
    ts = training.TrainStep(net, lr=1e-4)
    ts.step(x, tb)
    res = eval_reconstructor(net, loader, "cuda", (W, H))
    assert net.training
    fresh = _net(W, H, B, seed=1)
    fresh.load_state_dict(net.state_dict())
    want = eval_reconstructor(fresh, loader, "cuda", (W, H))
    _close(res, want, "after a training step", rtol=1e-4)
    l2 = ts.step(x, tb)
    assert torch.isfinite(l2).all()


# ------------------------------------------------------------------ RCCL, one rank
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_force_collective_one_rank_nccl_is_bit_identical():
    import torch.distributed as dist
    from sfh_amd.evaluation import eval_reconstructor
    assert not dist.is_initialized(), "another test left a process group behind"
    W, H = 112, 90
    net = _net(W, H, 4, seed=53)
    loader = _loader([4, 4, 2], H, W, net.court_poi.shape[1], seed=800)
    plain = eval_reconstructor(net, loader, "cuda", (W, H))
    r = net.range_rescales
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        coll = eval_reconstructor(net, loader, "cuda", (W, H), force_collective=True)
    finally:
        dist.destroy_process_group()
    assert net.range_rescales == r
    for k in KEYS:
        assert coll[k] == plain[k], (k, coll[k], plain[k])
