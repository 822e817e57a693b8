"""sfh_amd.mapping on the MI355X against tests/mapping_ref.py (numpy / torch restatement on the CPU).

The inverse, the nearest top view, ``valid``, the mosaic and the mapped points are compared for EQUALITY of every byte / bit:
the coordinates are the pinned fp32 arithmetic of csrc/warp_coords.h, the sums are integers and the point rule is
individually rounded fp64.  The top view is checked against the restatement evaluated with the GPU's own theta_c2f (the
discipline of the C2 / C5 tests), which separates the inverse from the sampling.  Only the bilinear blend has a bound,
derived and not measured: four products and three sums of values <= 255 in fp32, each within 2^-24 relative, total about
1.1e-4 < 2^-12, on top of the half unit of the rounding to a byte."""
import ctypes

import numpy as np
import pytest
import torch

import mapping_ref as R
from sfh_amd import mapping as M
from sfh_amd import synth

pytestmark = pytest.mark.gpu

# name -> ((W, H) of the frames, (wc, hc) of the court view)
CASES = {
    "1280x720_to_1280x720": ((1280, 720), (1280, 720)),
    "640x360_to_1280x720": ((640, 360), (1280, 720)),
    "1920x1080_to_1280x720": ((1920, 1080), (1280, 720)),
    "333x187_to_1280x720": ((333, 187), (1280, 720)),
    "1280x720_to_640x360": ((1280, 720), (640, 360)),
    "333x187_to_640x360": ((333, 187), (640, 360)),
    "640x360_to_335x189": ((640, 360), (335, 189)),        # a court view that is no multiple of 4 wide: the byte-store path
}
BILINEAR_BOUND = 0.5 + 2.0 ** -12


def _coded(H, W):
    """R = x & 255, G = y & 255, B = (x >> 8) | ((y >> 8) << 4): a wrong tap reads out as coordinates"""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([x & 255, y & 255, (x >> 8) | ((y >> 8) << 4)], axis=-1).astype(np.uint8)


def _frames(B, H, W, seed):
    """uniform noise and coordinate-coded frames, alternating (which comes first alternates with the batch size)"""
    fr = np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    for b in range(B):
        if (b + B) % 2:
            fr[b] = _coded(H, W)
    return fr


def _c2f_specials():
    """court -> frame matrices: identity, Z crossing zero inside the view, mostly out of frame, entirely out of frame"""
    ident = np.eye(3, dtype=np.float32)
    cross = ident.copy(); cross[2] = (0.9, 0.4, 1e-3)
    far = ident.copy(); far[0, 2] = 1.7
    gone = ident.copy(); gone[0, 2] = 5.0
    return ident, cross, far, gone


def _thetas(B, seed=5):
    """frame -> court: identity, the two realistic matrices, the inverses of the special court -> frame matrices, a zero last
    row, a singular theta (two equal rows), a theta with a NaN, then random ones"""
    ident, cross, far, gone = _c2f_specials()
    inv = lambda m: np.linalg.inv(m.astype(np.float64)).astype(np.float32)
    zero = ident.copy(); zero[2] = (0.0, 0.0, 0.0)
    twin = ident.copy(); twin[0] = twin[1] = (1.0, 0.5, 0.25)
    nan = synth.REALISTIC_THETAS[0].copy(); nan[1, 2] = np.nan
    t = [ident, synth.REALISTIC_THETAS[0], synth.REALISTIC_THETAS[1], inv(cross), inv(far), inv(gone), zero, twin, nan]
    g = synth._rng(seed, "mapping-thetas")
    while len(t) < B:
        t.append((ident + g.normal(0, 0.15, (3, 3))).astype(np.float32))
    return torch.from_numpy(np.stack(t[:B])).reshape(-1, 1, 3, 3)


def _gpu(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).cuda()


def _same(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, "
                             f"want {want[tuple(bad[0])]}")


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_views(fr, c2f, status, hc, wc, got_n, got_b, score=None, max_score=None):
    """got_n / got_b: (top, valid) host arrays of the nearest / bilinear render of fr with this theta_c2f and status"""
    want_top, want_valid, _ = R.top_view(fr, c2f, status, hc, wc, "nearest", score, max_score)
    _same(got_n[0], want_top, "nearest top view")
    _same(got_n[1], want_valid, "valid (nearest)")
    _, _, val = R.top_view(fr, c2f, status, hc, wc, "bilinear", score, max_score)
    _same(got_b[1], want_valid, "valid (bilinear)")
    err = np.abs(got_b[0].astype(np.float32) - val)
    print(f"bilinear: max |byte - oracle| = {err.max():.6f} (bound {BILINEAR_BOUND:.6f})")
    assert err.max() <= BILINEAR_BOUND
    return want_top, want_valid


# ------------------------------------------------------------------------------------------- inverse and top view
@pytest.mark.parametrize("B", [1, 13, 16, 17])
@pytest.mark.parametrize("case", list(CASES))
def test_top_view(case, B):
    (W, H), (wc, hc) = CASES[case]
    fr, th = _frames(B, H, W, 1), _thetas(B)
    frd, thd = _gpu(fr), th.cuda()
    rn, rb = M.TopViewRenderer((wc, hc), "nearest"), M.TopViewRenderer((wc, hc), "bilinear")
    out = rn(frd, thd)
    # the inverse: status and every bit of theta_c2f
    want_c2f, want_status = R.inverse_theta(th.numpy())
    c2f, status = out["theta_c2f"].cpu().numpy(), out["status"].cpu().numpy()
    _same(status, want_status, "status")
    _same(_bits(c2f), _bits(want_c2f), "theta_c2f bits")
    if B >= 9:
        assert status[:9].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0]
    got_n = (out["top_view"].cpu().numpy(), out["valid"].cpu().numpy())
    outb = rb(frd, thd)
    got_b = (outb["top_view"].cpu().numpy(), outb["valid"].cpu().numpy())
    want_top, _ = _check_views(fr, c2f, status, hc, wc, got_n, got_b)
    assert want_top[0].any()                                  # the identity frame is on screen
    assert set(np.unique(got_n[1])) <= {0, 255}
    # reproducibility: the same bits from a second call (into the same buffers) and from a fresh renderer
    again = rn(frd, thd)
    _same(again["top_view"], got_n[0], "second call")
    _same(again["valid"], got_n[1], "second call valid")
    _same(_bits(again["theta_c2f"]), _bits(c2f), "second inverse")
    _same(M.TopViewRenderer((wc, hc), "bilinear")(frd, thd)["top_view"], got_b[0], "second bilinear")


def _render_direct(fr, c2f, status, wc, hc, mode, score=None, max_score=0.0):
    """sfh_topview_render itself with a given theta_c2f (the renderer always inverts first)"""
    from sfh_amd import _lib
    from sfh_amd.engine import _ptr
    B, H, W = fr.shape[:3]
    frd, cd, sd = _gpu(fr), _gpu(np.ascontiguousarray(c2f, dtype=np.float32)), _gpu(np.ascontiguousarray(status, dtype=np.uint8))
    scd = _gpu(np.asarray(score, dtype=np.float32)) if score is not None else None
    top = torch.full((B, hc, wc, 3), 77, dtype=torch.uint8, device="cuda")
    valid = torch.full((B, hc, wc), 77, dtype=torch.uint8, device="cuda")
    stp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().sfh_topview_render(_ptr(frd), B, H, W, _ptr(cd), _ptr(sd), _ptr(scd), float(max_score), hc, wc, mode,
                                              _ptr(top), _ptr(valid), stp), "topview_render")
    torch.cuda.synchronize()
    return top.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("out_size", [(640, 360), (335, 189)])
def test_render_with_given_court_to_frame_matrices(out_size):
    """the special matrices as theta_c2f themselves, and what the inverse never hands over with status 1: a zero last row
    (Z == 0 everywhere), a NaN and entries beyond the fast reciprocal's range (the IEEE path of the kernel)"""
    wc, hc = out_size
    W, H = 333, 187
    ident, cross, far, gone = _c2f_specials()
    zero = ident.copy(); zero[2] = 0.0
    nan = ident.copy(); nan[0, 1] = np.nan
    huge = ident.copy(); huge[0, 0] = 1e30; huge[2, 2] = 1e30
    inf = ident.copy(); inf[1, 2] = np.inf
    tilt = (ident + np.float32([[0.1, 0.3, 0.2], [-0.2, 0.05, -0.1], [0.3, -0.2, 0.0]])).astype(np.float32)
    c2f = np.stack([ident, cross, far, gone, zero, nan, huge, inf, tilt, tilt * np.float32(3e30)])
    B = c2f.shape[0]
    status = np.ones((B,), dtype=np.uint8)
    fr = _frames(B, H, W, 8)
    got_n, got_b = _render_direct(fr, c2f, status, wc, hc, 0), _render_direct(fr, c2f, status, wc, hc, 1)
    want_top, want_valid = _check_views(fr, c2f, status, hc, wc, got_n, got_b)
    assert not want_valid[3].any() and want_valid[2].any() and not want_valid[2].all()


# ---------------------------------------------------------------------------------------------------- score gating
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_score_gating(mode):
    (W, H), (wc, hc) = (640, 360), (640, 360)
    B = 6
    fr, th = _frames(B, H, W, 2), _thetas(B)
    th[3:] = th[:3].clone()                      # every frame is usable: what disappears is the score's doing
    score = np.float32([0.1, 0.9, np.nan, 0.5, 0.50001, -np.inf])
    free = M.TopViewRenderer((wc, hc), mode)(_gpu(fr), th.cuda())
    free_top, free_valid = free["top_view"].cpu().numpy(), free["valid"].cpu().numpy()
    gated = M.TopViewRenderer((wc, hc), mode, max_score=0.5)(_gpu(fr), th.cuda(), score=_gpu(score))
    top, valid = gated["top_view"].cpu().numpy(), gated["valid"].cpu().numpy()
    assert gated["status"].cpu().tolist() == [1] * B
    for b in (1, 2, 4):                          # above max_score, NaN, just above: zeros and valid 0
        assert not top[b].any() and not valid[b].any()
    for b in (0, 3, 5):                          # the neighbours are unchanged
        assert free_top[b].any()
        _same(top[b], free_top[b], f"frame {b}")
        _same(valid[b], free_valid[b], f"valid {b}")
    if mode == "nearest":
        c2f, status = gated["theta_c2f"].cpu().numpy(), gated["status"].cpu().numpy()
        want_top, want_valid, _ = R.top_view(fr, c2f, status, hc, wc, "nearest", score, 0.5)
        _same(top, want_top, "gated top view")
        _same(valid, want_valid, "gated valid")
    # a renderer without max_score ignores the score
    same = M.TopViewRenderer((wc, hc), mode)(_gpu(fr), th.cuda(), score=_gpu(score))
    _same(same["top_view"], free_top, "no max_score")


# ---------------------------------------------------------------------------------------------------------- mosaic
def test_mosaic():
    (W, H), (wc, hc) = (640, 360), (640, 360)
    sizes = (5, 13, 3)
    N = sum(sizes)
    fr = _frames(N, H, W, 3)
    th = _thetas(N)
    score = np.random.default_rng(4).uniform(0, 1, N).astype(np.float32)
    score[4] = np.nan
    mos = M.CourtMosaic((wc, hc), max_score=0.8)
    s_ref, n_ref = np.zeros((hc, wc, 3), dtype=np.uint32), np.zeros((hc, wc), dtype=np.uint32)
    k = 0
    for n in sizes:                              # three add calls of different batch sizes
        sl = slice(k, k + n)
        mos.add(_gpu(fr[sl]), th[sl].cuda(), score=_gpu(score[sl]))
        c2f, status = M.invert_theta(th[sl].cuda())
        R.mosaic_add(s_ref, n_ref, fr[sl], c2f.cpu().numpy(), status.cpu().numpy(), score[sl], 0.8)
        k += n
    assert n_ref.max() > 1 and n_ref.min() < n_ref.max()
    _same(mos.sum.cpu().numpy().view(np.uint32), s_ref, "sum")
    _same(mos.count.cpu().numpy().view(np.uint32), n_ref, "count")
    image, count = mos.result()
    _same(image, R.mosaic_finish(s_ref, n_ref), "mosaic image")
    _same(mos.result()[0], image.cpu().numpy(), "second result")
    # the same frames split differently: the integer sums are order-free
    other = M.CourtMosaic((wc, hc), max_score=0.8)
    for a, b in ((0, 16), (16, 17), (17, N)):
        other.add(_gpu(fr[a:b]), th[a:b].cuda(), score=_gpu(score[a:b]))
    assert torch.equal(other.sum, mos.sum) and torch.equal(other.count, mos.count)
    assert torch.equal(other.result()[0], image)
    # without max_score the score is ignored: more frames contribute
    free = M.CourtMosaic((wc, hc)).add(_gpu(fr), th.cuda(), score=_gpu(score))
    assert int(free.count.sum()) > int(mos.count.sum())
    mos.reset()
    assert not mos.sum.any() and not mos.count.any()
    assert not mos.result()[0].any()


# ---------------------------------------------------------------------------------------------------------- points
def _mapping(F=24):
    th = _thetas(F).reshape(F, 3, 3)
    return M.CourtMapping(th, scores=np.linspace(0, 1, F, dtype=np.float32), names=[f"{k:06d}" for k in range(F)])


@pytest.mark.parametrize("N", [1, 7, 4096, 1000003])
def test_points(N):
    cm = _mapping()
    F = len(cm)
    mapper = M.FrameCourtMapper(cm)
    tabs = cm.tables("cuda")
    c2f, status = tabs["theta_c2f"].cpu().numpy(), tabs["status"].cpu().numpy()
    want_c2f, want_status = R.inverse_theta(cm.theta)
    _same(_bits(c2f), _bits(want_c2f), "theta_c2f table")
    _same(status, want_status, "status table")
    g = np.random.default_rng(N)
    px = (g.uniform(-0.2, 1.2, (N, 2)) * [1280, 720]).astype(np.float32)
    idx = g.integers(-2, F + 2, N).astype(np.int32)          # indices out of range on both sides
    idx[0] = 1
    if N > 3:
        idx[1:4] = (6, 7, 8)                                 # the singular frames
    pd, idd = _gpu(px), _gpu(idx)
    for units in ("norm", "pixels", "meters", "feet"):
        out, flag = mapper.frame_to_court(pd, idd, (1280, 720), units=units)
        want, wflag = R.map_points(px, idx, cm.theta, (1280, 720), M.UNITS[units])
        _same(flag, wflag, f"flag {units}")
        _same(_bits(out), _bits(want), f"frame_to_court {units}")
        assert wflag[0] == 1 and (N < 100 or (wflag == 0).any())
        out2, flag2 = mapper.frame_to_court(pd, idd, (1280, 720), units=units)          # reproducible
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(flag2, flag)
    # the other direction: court pixels and normalised court points into frame pixels / the unit square
    cpx = (g.uniform(-0.1, 1.1, (N, 2)) * [1280, 720]).astype(np.float32)
    out, flag = mapper.court_to_frame(_gpu(cpx), idd, court_size=(1280, 720), frame_size=(1920, 1080))
    want, wflag = R.map_points(cpx, idx, c2f, (1280, 720), (1920, 1080))
    _same(flag, wflag, "flag court_to_frame")
    _same(_bits(out), _bits(want), "court_to_frame pixels")
    if N > 3:
        assert wflag[1:4].tolist() == [0, 0, 0] and not want[1:4].any()       # theta_c2f of a singular frame is all zeros
    cn = g.uniform(-1, 1, (N, 2)).astype(np.float32)
    out, flag = mapper.court_to_frame(_gpu(cn), 2)                              # one frame for every point, by row ...
    want, wflag = R.map_points(cn, 2, c2f)
    _same(flag, wflag, "flag one frame")
    _same(_bits(out), _bits(want), "court_to_frame one frame")
    out, _ = mapper.court_to_frame(_gpu(cn), "000002")                          # ... and by name
    _same(_bits(out), _bits(want), "court_to_frame by name")
    # already normalised frame points
    out, flag = mapper.frame_to_court(_gpu(cn), idd)
    want, wflag = R.map_points(cn, idx, cm.theta)
    _same(flag, wflag, "flag normalised")
    _same(_bits(out), _bits(want), "frame_to_court normalised")


def test_court_to_frame_agrees_with_poi_project():
    """sfh_poi_project_fwd applies the same theta_c2f in fp32 (Kornia's 1 / (z + 1e-8)): close, not bitwise"""
    from sfh_amd import ops
    th = torch.from_numpy(np.stack([synth.REALISTIC_THETAS[0], synth.REALISTIC_THETAS[1], np.eye(3, dtype=np.float32)]))
    poi = synth.load_court_poi("pitch", 3)
    want = ops.poi_project(th.cuda().reshape(3, 1, 3, 3), poi.cuda(), normalize=True).cpu().numpy()
    mapper = M.FrameCourtMapper(M.CourtMapping(th))
    n = poi.shape[1]
    idx = torch.arange(3, dtype=torch.int32).repeat_interleave(n).cuda()
    out, flag = mapper.court_to_frame(poi.reshape(-1, 2).contiguous().cuda(), idx)
    assert flag.all()
    d = np.abs(out.cpu().numpy().reshape(3, n, 2) - want).max()
    print(f"court_to_frame against sfh_poi_project_fwd: max |d| = {d:.3e}")
    assert d <= 1e-5


# -------------------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("scale", [1, 3])
def test_frame_pipeline_top_view_output(scale):
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
    with torch.no_grad():
        plain = {c: list(FramePipeline(net, B, (h * scale, w * scale), req_outputs=req, consistency=c).run(iter(batches)))
                 for c in (True, False)}
        scores = np.concatenate([p["consist_score"] for p in plain[True]])
        thr = float(np.median(scores))          # inside the range of this model's scores: some frames are gated away
        for max_score, consistency, mode in ((thr, True, "nearest"), (None, False, "bilinear")):
            r = M.TopViewRenderer((160, 96), mode, max_score=max_score)
            pipe = FramePipeline(net, B, (h * scale, w * scale), req_outputs=req, consistency=consistency, top_view=r)
            got = list(pipe.run(iter(batches)))
            assert len(got) == len(batches)
            gated = 0
            for fr, res, ref in zip(batches, got, plain[consistency]):
                assert set(res) == set(ref) | {"top_view", "top_view_valid"}
                assert res["top_view"].dtype == np.uint8 and res["top_view"].shape == (B, 96, 160, 3)
                assert res["top_view_valid"].dtype == np.uint8 and res["top_view_valid"].shape == (B, 96, 160)
                for k in ref:          # every other output is what the pipeline gives without the keyword
                    assert res[k].dtype == ref[k].dtype and np.array_equal(res[k], ref[k]), k
                x = E.frames_u8_to_input(fr.cuda(), (w, h) if scale != 1 else None)
                p = net.predict(x, consistency=consistency, project_poi=True)
                direct = M.TopViewRenderer((160, 96), mode, max_score=max_score)(fr.cuda(), p["theta"], score=p.get("consist_score"))
                assert np.array_equal(res["top_view"], direct["top_view"].cpu().numpy())
                assert np.array_equal(res["top_view_valid"], direct["valid"].cpu().numpy())
                if mode == "nearest":  # and the direct call gives the restatement's bytes
                    sc = p["consist_score"].cpu().numpy()
                    want, wvalid, _ = R.top_view(fr.numpy(), direct["theta_c2f"].cpu().numpy(), direct["status"].cpu().numpy(),
                                                 96, 160, "nearest", sc, max_score)
                    assert np.array_equal(res["top_view"], want) and np.array_equal(res["top_view_valid"], wvalid)
                    gated += int((~R.used_frames(direct["status"].cpu().numpy(), sc, max_score)).sum())
            if max_score is not None:
                assert 0 < gated < B * len(batches)
    with pytest.raises(ValueError, match="max_score"):
        FramePipeline(net, B, (h, w), req_outputs=req, consistency=False, top_view=M.TopViewRenderer((160, 96), max_score=0.5))


# ----------------------------------------------------------------------------------------------------- host driver
def test_rectify_game(tmp_path):
    from sfh_amd import outputs as O
    W, H, N = 333, 187, 5
    fr = _frames(N, H, W, 6)
    th = _thetas(N).numpy()
    scores = [0.1, 0.2, 0.9, 0.3, 0.4]
    names = [f"{k:06d}" for k in range(N)]
    with O.CourtJsonWriter(str(tmp_path), "game", "m") as w:
        for n, s, t in zip(names, scores, th):
            w.add(n, score=s, theta=t)
    dst = str(tmp_path / "top")
    written = M.rectify_game(w.path, iter(fr), dst, out_size=(320, 180), max_score=0.5, batch=2, names=names)
    assert [p.rsplit("/", 1)[1] for p in written] == [f"{n}.png" for n in names] + ["mosaic.png"]
    c2f, status = R.inverse_theta(th)
    sc = np.float32([O.format_score(s) for s in scores])
    want, wvalid, _ = R.top_view(fr, c2f, status, 180, 320, "nearest", sc, 0.5)
    assert not want[2].any() and want[0].any()
    for k, p in enumerate(written[:N]):
        assert np.array_equal(O.decode_png(np.fromfile(p, dtype=np.uint8)), want[k])
    s_ref, n_ref = np.zeros((180, 320, 3), dtype=np.uint32), np.zeros((180, 320), dtype=np.uint32)
    R.mosaic_add(s_ref, n_ref, fr, c2f, status, sc, 0.5)
    assert np.array_equal(O.decode_png(np.fromfile(written[N], dtype=np.uint8)), R.mosaic_finish(s_ref, n_ref))
    with pytest.raises(ValueError, match="5 predictions"):
        M.rectify_game(w.path, iter(fr[:3]), dst, out_size=(320, 180))
