"""sfh_amd.visualize on the MI355X against tests/overlay_ref.py (numpy restatement on the CPU): every case compares ALL output
bytes for equality - the arithmetic is integral and the warp's coordinates are pinned fp32, so there is no tolerance."""
import numpy as np
import pytest
import torch

import overlay_ref as R
from sfh_amd import synth
from sfh_amd import visualize as V

pytestmark = pytest.mark.gpu

SIZES = {"640x360": (640, 360), "1280x720": (1280, 720), "333x187": (333, 187)}


def _frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _thetas(B, seed=5):
    """identity, the synth thetas, random ones, Z crossing zero inside the frame, most of the frame out of bounds, Z == 0"""
    ident = np.eye(3, dtype=np.float32)
    sing = ident.copy(); sing[2] = (0.9, 0.4, 1e-3)
    far = ident.copy(); far[0, 2] = 1.7                 # most of the frame maps outside the template
    gone = ident.copy(); gone[0, 2] = 5.0               # all of it
    zero = ident.copy(); zero[2] = (0.0, 0.0, 0.0)
    t = [ident, synth.REALISTIC_THETAS[0], synth.REALISTIC_THETAS[1], sing, far, gone, zero]
    g = synth._rng(seed, "overlay-thetas")
    while len(t) < B:
        t.append((ident + g.normal(0, 0.15, (3, 3))).astype(np.float32))
    return torch.from_numpy(np.stack(t[:B])).reshape(-1, 1, 3, 3)


def _template(nc, ht, wt, n=1, seed=0):
    """id template (n,1,ht,wt) valued k / nc: the packaged court for 4 classes at its sizes, else blocks of random ids"""
    if nc == 4 and n == 1 and (wt, ht) in ((640, 360), (1280, 720)):
        return synth.load_court_template(f"ncaa_nc4_{wt}x{ht}", 4, 1)
    g = np.random.default_rng(100 + seed)
    ids = g.integers(0, nc, (n, 1, (ht + 7) // 8, (wt + 7) // 8))
    ids = np.repeat(np.repeat(ids, 8, axis=2), 8, axis=3)[:, :, :ht, :wt]
    return torch.from_numpy(ids.astype(np.float32) / np.float32(nc)).contiguous()


def _gpu(a):
    if a is None:
        return None
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).cuda()


def _same(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        raise AssertionError(f"{len(bad)} pixels differ, first (b, y, x) = {bad[0].tolist()}: got "
                             f"{got[tuple(bad[0])].tolist()}, want {want[tuple(bad[0])].tolist()}")


# ------------------------------------------------------------------------------------------------- warp leg
@pytest.mark.parametrize("B", [1, 13, 16])
@pytest.mark.parametrize("size", list(SIZES))
def test_warp_leg(size, B):
    W, H = SIZES[size]
    fr, th = _frames(B, H, W, 1), _thetas(B)
    court = _template(4, 360, 640)                      # at 1280x720 and 333x187 the template differs from the frame size
    r = V.OverlayRenderer(court.cuda(), source="warp")
    want = R.render(fr, th, court, source="warp", shared=True)
    assert not np.array_equal(want, fr)
    _same(r(_gpu(fr), th.cuda()), want)


@pytest.mark.parametrize("how", ["per_frame", "expanded", "replicated", "larger_than_frame"])
def test_warp_leg_templates(how):
    W, H = SIZES["640x360"]
    B = 13
    fr, th = _frames(B, H, W, 2), _thetas(B, seed=6)
    if how == "per_frame":
        court = _template(4, H, W, n=B, seed=1)
        dev, shared = court.cuda(), False
    elif how == "expanded":                             # non-contiguous, batch stride 0
        court = _template(4, H, W)
        dev, shared = court.cuda().expand(B, -1, -1, -1), True
        assert not dev.is_contiguous()
    elif how == "replicated":                           # B equal copies: found to be one image
        court = _template(4, H, W)
        dev, shared = court.repeat(B, 1, 1, 1).cuda(), True
    else:
        court = _template(4, 720, 1280)
        dev, shared = court.cuda(), True
    r = V.OverlayRenderer(dev, source="warp")
    _same(r(_gpu(fr), th.cuda()), R.render(fr, th, court, source="warp", shared=shared))
    if how == "replicated":
        assert r._tmpl[2] and r._tmpl[1].shape[0] == 1


@pytest.mark.parametrize("nc", [4, 7, 8])
def test_palettes(nc):
    W, H = SIZES["333x187"]
    B = 3
    fr, th = _frames(B, H, W, 3), _thetas(B)
    court = _template(nc, 90, 160, seed=nc) if nc != 4 else _template(4, 360, 640)
    r = V.OverlayRenderer(court.cuda(), mask_classes=nc, source="warp")
    want = R.render(fr, th, court, mask_classes=nc, source="warp", shared=True)
    _same(r(_gpu(fr), th.cuda()), want)
    # the segmentation leg with every id 0 .. 7 and ids outside the table (they count as 0)
    ids = np.random.default_rng(nc).integers(-2, 12, (B, H, W)).astype(np.int32)
    r = V.OverlayRenderer(court.cuda(), mask_classes=nc, source="segm")
    _same(r(_gpu(fr), None, segm=_gpu(ids)), R.render(fr, mask_classes=nc, segm=ids, source="segm"))


@pytest.mark.parametrize("size", ["1280x720", "640x360"])
def test_warp_leg_against_the_existing_warp_and_format_masks(size):
    """the expected bytes from code that exists without the overlay and is pinned to the oracle: sfh_homography_warp_fwd
    (nearest, int32 ids) -> format_masks(rgb); only the blend is the restatement's"""
    from sfh_amd import engine as E
    from sfh_amd import outputs as O
    W, H = SIZES[size]
    B = 16
    fr, th = _frames(B, H, W, 4), _thetas(B, seed=7)
    for court, shared in ((_template(4, 360, 640), True), (_template(4, H, W, n=B, seed=2), False)):
        cd = court.cuda()
        _, ids = E.homography_warp(th.cuda(), cd, H, W, True, scale=4.0, want_f32=False, want_i32=True, shared_template=shared)
        rgb = O.format_masks(ids, "rgb", 4).cpu().numpy()
        got = V.OverlayRenderer(cd, source="warp")(_gpu(fr), th.cuda())
        _same(got, R.blend(fr, rgb))
        assert np.array_equal(ids.cpu().numpy(), R.warp_ids(th, court, H, W, 4, shared))


# ----------------------------------------------------------------------------------------- segmentation leg
def _tied_logits(B, nc, hs, ws, seed):
    """logits from a few values, so that exact ties are everywhere (the first maximum must win)"""
    g = np.random.default_rng(seed)
    lg = g.integers(-1, 2, (B, nc, hs, ws)).astype(np.float32)
    assert ((lg == lg.max(1, keepdims=True)).sum(1) > 1).mean() > 0.3
    return lg


@pytest.mark.parametrize("case", ["u8_same", "i32_half", "logits", "logits_odd", "none"])
def test_segmentation_leg(case):
    size = {"u8_same": "640x360", "i32_half": "1280x720", "logits": "640x360", "logits_odd": "333x187", "none": "640x360"}[case]
    W, H = SIZES[size]
    B = 13
    fr = _frames(B, H, W, 11)
    g = np.random.default_rng(12)
    if case == "u8_same":
        segm = g.integers(0, 4, (B, H, W), dtype=np.uint8)
    elif case == "i32_half":
        segm = g.integers(0, 4, (B, H // 2, W // 2)).astype(np.int32)
    elif case == "logits":
        segm = _tied_logits(B, 4, H, W, 13)
    elif case == "logits_odd":
        segm = _tied_logits(B, 4, H, W, 14)
    else:
        segm = None
    r = V.OverlayRenderer(_template(4, 360, 640).cuda(), source="segm")
    want = R.render(fr, segm=segm, source="segm")
    if segm is None:
        assert np.array_equal(want, fr)
    _same(r(_gpu(fr), None, segm=_gpu(segm)), want)


# --------------------------------------------------------------------------------------------- source choice
def test_auto_source_follows_the_score():
    W, H = SIZES["640x360"]
    B = 16
    fr, th = _frames(B, H, W, 21), _thetas(B, seed=8)
    court = _template(4, 360, 640)
    segm = np.random.default_rng(22).integers(0, 4, (B, H // 2, W // 2), dtype=np.uint8)
    thr = 0.1
    below = np.nextafter(np.float32(thr), np.float32(0))
    score = np.array([0.0, 0.05, below, thr, np.nextafter(np.float32(thr), np.float32(1)), 0.5, np.nan, -1.0, np.inf, -np.inf,
                      0.0999, 0.1001, 3.0, 0.02, 0.2, 0.09], dtype=np.float32)
    r = V.OverlayRenderer(court.cuda(), score_threshold=thr)
    want = R.render(fr, th, court, score=score, segm=segm, score_threshold=thr, shared=True)
    _same(r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm)), want)
    # the two legs really differ on these frames, so a wrong choice would show
    ww = R.render(fr, th, court, source="warp", shared=True)
    ws = R.render(fr, segm=segm, source="segm")
    for b in range(B):
        assert np.array_equal(want[b], ww[b] if score[b] < np.float32(thr) else ws[b]) and not np.array_equal(ww[b], ws[b])
    # no segmentation source: frames at or above the threshold (and the NaN one) are copied
    want = R.render(fr, th, court, score=score, score_threshold=thr, shared=True)
    assert np.array_equal(want[3], fr[3]) and np.array_equal(want[6], fr[6])
    _same(r(_gpu(fr), th.cuda(), score=_gpu(score)), want)
    # overlay threshold: only frames below it are drawn on, whichever leg they take
    r = V.OverlayRenderer(court.cuda(), score_threshold=thr, overlay_threshold=0.2)
    want = R.render(fr, th, court, score=score, segm=segm, score_threshold=thr, overlay_threshold=0.2, shared=True)
    assert np.array_equal(want[5], fr[5]) and np.array_equal(want[6], fr[6]) and not np.array_equal(want[11], fr[11])
    _same(r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm)), want)
    with pytest.raises(ValueError, match="score"):
        r(_gpu(fr), th.cuda(), segm=_gpu(segm))


def test_forced_sources_need_no_score():
    W, H = SIZES["333x187"]
    B = 5
    fr, th = _frames(B, H, W, 31), _thetas(B)
    court = _template(4, 360, 640)
    segm = np.random.default_rng(32).integers(0, 4, (B, H, W), dtype=np.uint8)
    score = np.array([0.0, 1.0, np.nan, 0.05, 0.3], np.float32)
    for src in ("warp", "segm"):
        r = V.OverlayRenderer(court.cuda(), source=src)
        want = R.render(fr, th, court, segm=segm, source=src, shared=True)
        _same(r(_gpu(fr), th.cuda(), segm=_gpu(segm)), want)
        _same(r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm)), want)      # a score does not change a forced source
    with pytest.raises(ValueError, match="score"):
        V.OverlayRenderer(court.cuda())(_gpu(fr), th.cuda(), segm=_gpu(segm))


@pytest.mark.parametrize("size", ["640x360", "333x187"])
def test_in_place_and_repeatable(size):
    W, H = SIZES[size]
    B = 13
    fr, th = _frames(B, H, W, 41), _thetas(B)
    court = _template(4, 360, 640)
    segm = np.random.default_rng(42).integers(0, 4, (B, H, W), dtype=np.uint8)
    score = np.linspace(0, 0.2, B).astype(np.float32)
    r = V.OverlayRenderer(court.cuda(), overlay_threshold=0.15)
    a = r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm))
    b = r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm))
    assert torch.equal(a, b)
    buf = _gpu(fr)
    c = r(buf, th.cuda(), score=_gpu(score), segm=_gpu(segm), out=buf)
    assert c is buf and torch.equal(c, a)
    given = torch.empty_like(buf)
    assert r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm), out=given) is given and torch.equal(given, a)
    _same(a, R.render(fr, th, court, score=score, segm=segm, overlay_threshold=0.15, shared=True))


# ------------------------------------------------------------------------------------------ markers and label
def _marker_points(H, W):
    """centres inside, on each border, outside (partly visible and invisible), NaN / inf, ties of the rounding, overlaps"""
    px = [(0.5, 0.5), (0.0, 0.3), (1.0, 0.6), (0.4, 0.0), (0.7, 1.0), (0.0, 0.0), (1.0, 1.0),
          ((W - 1) / W, (H - 1) / H), (-2.0 / W, 0.5), (0.5, -3.0 / H), (1.0 + 2.0 / W, 0.2), (0.3, 1.0 + 1.0 / H),
          (-0.5, 0.5), (2.0, 2.0), (float("nan"), 0.5), (0.5, float("nan")), (float("inf"), 0.1), (0.2, float("-inf")),
          (10.5 / W, 20.5 / H), (11.5 / W, 21.5 / H), (1e30, 0.5), (-1e30, -1e30),
          (0.5 + 2.0 / W, 0.5 + 1.0 / H), (0.5 - 3.0 / W, 0.5), (20.0 / W, 18.0 / H), (40.0 / W, 24.0 / H)]
    return np.array(px, dtype=np.float32)


@pytest.mark.parametrize("size", ["640x360", "333x187"])
def test_markers_and_label(size):
    W, H = SIZES[size]
    B = 4
    fr, th = _frames(B, H, W, 51), _thetas(B)
    court = _template(4, 360, 640)
    pts = _marker_points(H, W)
    poi = np.stack([np.roll(pts, b, axis=0) for b in range(B)])       # another drawing order per frame
    score = np.array([0.01, 0.5, np.nan, 0.1], np.float32)
    labels = ["0.010000", "0.500000", "nan", "-1.5e+07 inf"]
    kw = dict(label_pos=(15, 15), label_scale=2)
    for radius, color in ((5, (255, 255, 255)), (1, (7, 200, 31)), (0, (1, 2, 3))):
        r = V.OverlayRenderer(court.cuda(), marker_radius=radius, marker_color=color, **kw)
        base = R.render(fr, th, court, score=score, shared=True)
        want = R.annotate(base.copy(), poi=poi, radius=radius, marker_color=color, labels=labels, score=score, **kw)
        _same(r(_gpu(fr), th.cuda(), score=_gpu(score), poi=_gpu(poi), labels=labels), want)
        # markers only / label only
        _same(r(_gpu(fr), th.cuda(), score=_gpu(score), poi=_gpu(poi)),
              R.annotate(base.copy(), poi=poi, radius=radius, marker_color=color))
        _same(r(_gpu(fr), th.cuda(), score=_gpu(score), labels=labels), R.annotate(base.copy(), labels=labels, score=score, **kw))
        if radius == 0:     # radius 0 draws nothing
            _same(r(_gpu(fr), th.cuda(), score=_gpu(score), poi=_gpu(poi)), base)
    # a label that is clipped on every side, scale 3, and a forced source without a score
    for pos in ((-7, -5), (W - 20, H - 9)):
        r = V.OverlayRenderer(court.cuda(), source="segm", marker_radius=4, label_pos=pos, label_scale=3)
        base = R.render(fr, source="segm")
        want = R.annotate(base.copy(), poi=poi, radius=4, labels=labels, label_pos=pos, label_scale=3, source="segm")
        _same(r(_gpu(fr), None, poi=_gpu(poi), labels=labels), want)
    with pytest.raises(ValueError, match="not in the overlay font"):
        r(_gpu(fr), None, labels=["0.1", "0.2", "score", "0.4"])


def test_label_is_drawn_over_markers_and_later_markers_over_earlier():
    """the stated order, seen directly: a marker under the label's glyphs keeps only what the glyphs do not light"""
    W, H = 96, 40
    fr = np.zeros((1, H, W, 3), np.uint8)
    court = _template(4, 360, 640)
    poi = np.array([[(12.0 / W, 10.0 / H), (14.0 / W, 11.0 / H)]], np.float32)
    r = V.OverlayRenderer(court.cuda(), source="segm", marker_radius=6, marker_color=(9, 9, 9), label_pos=(4, 4), label_scale=2)
    got = r(_gpu(fr), None, poi=_gpu(poi), labels=["88"]).cpu().numpy()
    want = R.annotate(fr.copy(), poi=poi, radius=6, marker_color=(9, 9, 9), labels=["88"], label_pos=(4, 4), label_scale=2,
                      source="segm")
    assert np.array_equal(got, want)
    lit = (got[0] == (0, 0, 255)).all(-1)
    disc = (got[0] == (9, 9, 9)).all(-1)
    yy, xx = np.mgrid[0:H, 0:W]
    under = ((xx - 12) ** 2 + (yy - 10) ** 2 <= 36) | ((xx - 14) ** 2 + (yy - 11) ** 2 <= 36)
    # every glyph pixel is lit (4 frame pixels per font pixel), also those over the discs; the discs keep the rest
    assert lit.sum() == 2 * sum(bin(v).count("1") for v in R.glyph_rows("8")) * 4
    assert (lit & under).any() and np.array_equal(disc, under & ~lit)


# ------------------------------------------------------------------------------------------------- streams
def test_non_default_stream_without_a_sync():
    W, H = SIZES["640x360"]
    B = 16
    fr, th = _frames(B, H, W, 61), _thetas(B)
    court = _template(4, 360, 640)
    segm = np.random.default_rng(62).integers(0, 4, (B, H, W), dtype=np.uint8)
    score = np.linspace(0, 0.2, B).astype(np.float32)
    poi = np.random.default_rng(63).random((B, 20, 2)).astype(np.float32)
    labels = ['{:4f}'.format(s) for s in score]
    r = V.OverlayRenderer(court.cuda(), marker_radius=3)
    want = r(_gpu(fr), th.cuda(), score=_gpu(score), segm=_gpu(segm), poi=_gpu(poi), labels=labels)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    frp, thp = torch.from_numpy(fr).pin_memory(), th.pin_memory()
    with torch.cuda.stream(s):
        frd, thd = frp.cuda(non_blocking=True), thp.cuda(non_blocking=True)
        scd, sgd, pd = (torch.from_numpy(a).pin_memory().cuda(non_blocking=True) for a in (score, segm, poi))
        filler = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):       # work queued in front on the same stream; nothing waits for it on the host
            filler = filler @ filler * 1e-4
        out = r(frd, thd, score=scd, segm=sgd, poi=pd, labels=labels)
        consumer = out.sum(dtype=torch.int64)
    s.synchronize()
    assert torch.equal(out, want)
    assert int(consumer) == int(want.sum(dtype=torch.int64))
    _same(want, R.annotate(R.render(fr, th, court, score=score, segm=segm, shared=True), poi=poi, radius=3, labels=labels,
                           score=score))


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.mark.parametrize("scale", [1, 3])
def test_frame_pipeline_overlay_output(scale):
    from sfh_amd import engine as E
    from sfh_amd.pipeline import FramePipeline
    from sfh_amd.reconstructor import Reconstructor
    w, h, B = 112, 90, 2
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :h, :w].contiguous()
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(w, h), unet_size=(w, h), warp_size=(w, h), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.cuda().eval()
    batches = [torch.from_numpy(synth.synth_frames_u8(B, h * scale, w * scale, seed=40 + k)).pin_memory() for k in range(5)]
    req = ("theta", "warp_mask", "segm_mask", "poi")
    tmpl = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    with torch.no_grad():
        plain = {c: list(FramePipeline(net, B, (h * scale, w * scale), req_outputs=req, consistency=c).run(iter(batches)))
                 for c in (True, False)}
        scores = np.concatenate([p["consist_score"] for p in plain[True]])
        thr = float(np.median(scores))      # inside the range of this model's scores, so that "auto" takes both legs
        assert (scores < np.float32(thr)).any() and not (scores < np.float32(thr)).all()
        for src, consistency in (("auto", True), ("segm", False), ("warp", False)):
            r = V.OverlayRenderer(tmpl.cuda(), score_threshold=thr, source=src, marker_radius=2)
            pipe = FramePipeline(net, B, (h * scale, w * scale), req_outputs=req + ("overlay",), consistency=consistency, overlay=r)
            got = list(pipe.run(iter(batches)))
            assert len(got) == len(batches)
            for fr, res, ref in zip(batches, got, plain[consistency]):
                assert res["overlay"].dtype == np.uint8 and res["overlay"].shape == tuple(fr.shape)
                assert set(res) == set(ref) | {"overlay"}
                for k in ref:          # every other output is what the pipeline gives without the keyword
                    assert res[k].dtype == ref[k].dtype and np.array_equal(res[k], ref[k]), k
                x = E.frames_u8_to_input(fr.cuda(), (w, h) if scale != 1 else None)
                p = net.predict(x, consistency=consistency, project_poi=True)
                direct = r(fr.cuda(), p["theta"], score=p.get("consist_score"), segm=p["logits"], poi=p["poi"])
                assert np.array_equal(res["overlay"], direct.cpu().numpy())
                # and the direct call gives the restatement's bytes
                sc = p["consist_score"].cpu().numpy() if consistency else None
                want = R.render(fr.numpy(), p["theta"].cpu(), tmpl, score=sc, segm=p["logits"].cpu().numpy(),
                                score_threshold=thr, source=src, shared=True)
                R.annotate(want, poi=p["poi"].cpu().numpy(), radius=2)
                assert np.array_equal(res["overlay"], want)
