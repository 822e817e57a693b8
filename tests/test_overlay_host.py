"""CPU-side checks of the court overlay (sfh_amd.visualize, csrc/overlay.hip): the blend rule, the argument checks of the two
C entries (they fire before anything touches a device), the glyph table, and the host driver with the renderer stubbed by
tests/overlay_ref.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import overlay_ref as R
from conftest import ROOT


def test_integer_blend_equals_the_float64_rule_for_every_byte_pair():
    """utils/postprocess.py:63-65: (mask * 0.5 + frame * 0.5).astype('uint8') in float64 == (mask + frame) >> 1"""
    c, f = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    want = (c.astype(np.float64) * 0.5 + f.astype(np.float64) * 0.5).astype("uint8")
    got = ((c.astype(np.uint16) + f.astype(np.uint16)) >> 1).astype(np.uint8)
    assert np.array_equal(got, want)
    # overlay_ref.blend on the same pairs (a non-black colour: channel 1 = 255 keeps the pixel on the blend side)
    colour = np.stack([c, np.full_like(c, 255), c], axis=-1)
    frame = np.stack([f, f, f], axis=-1)
    out = R.blend(frame, colour)
    assert np.array_equal(out[..., 0], want) and np.array_equal(out[..., 2], want)
    # a black colour keeps the frame
    assert np.array_equal(R.blend(frame, np.zeros_like(colour)), frame)
    # the packed form of the kernel: (a & b) + (((a ^ b) & 0xFE) >> 1) per byte
    a, b = c.astype(np.uint32), f.astype(np.uint32)
    assert np.array_equal((a & b) + (((a ^ b) & 0xFE) >> 1), want)


def _lib():
    from sfh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import sfh_amd.build as b
        b.build(verbose=False)
    return _lib.load()


def _render(lib, **kw):
    """sfh_overlay_render with plausible non-null dummies (never dereferenced: every case fails an argument check)"""
    one = ctypes.c_void_p(0x1000)
    pal = (ctypes.c_uint8 * 24)()
    a = dict(frames=one, out=one, batch=2, H=8, W=8, theta=one, tmpl=one, bstride=0, ht=8, wt=8, scale=4.0, segm=one, kind=1,
             nc=4, hs=8, ws=8, score=one, thr=0.1, source=0, use_ot=0, ot=0.0, palette=ctypes.cast(pal, ctypes.c_void_p))
    a.update(kw)
    return lib.sfh_overlay_render(a["frames"], a["out"], a["batch"], a["H"], a["W"], a["theta"], a["tmpl"], a["bstride"],
                                  a["ht"], a["wt"], a["scale"], a["segm"], a["kind"], a["nc"], a["hs"], a["ws"], a["score"],
                                  a["thr"], a["source"], a["use_ot"], a["ot"], a["palette"], None)


def _annotate(lib, **kw):
    one = ctypes.c_void_p(0x1000)
    col = (ctypes.c_uint8 * 3)(255, 255, 255)
    a = dict(out=one, batch=2, H=8, W=8, poi=one, npts=4, radius=2, color=ctypes.cast(col, ctypes.c_void_p), labels=one, L=8,
             lx=1, ly=1, scale=1, score=one, thr=0.1, source=0)
    a.update(kw)
    return lib.sfh_overlay_annotate(a["out"], a["batch"], a["H"], a["W"], a["poi"], a["npts"], a["radius"], a["color"],
                                    a["labels"], a["L"], a["lx"], a["ly"], a["scale"], a["score"], a["thr"], a["source"], None)


def test_overlay_entries_check_their_arguments_without_a_gpu():
    lib = _lib()
    err = lambda: lib.sfh_last_error().decode()
    assert _render(lib, frames=None) == -1 and "null" in err()
    assert _render(lib, out=None) == -1 and "null" in err()
    assert _render(lib, palette=None) == -1 and "null" in err()
    assert _render(lib, theta=None) == -1 and "null" in err()
    assert _render(lib, tmpl=None, source=1) == -1 and "null" in err()
    assert _render(lib, score=None) == -1 and "null" in err()                   # auto needs a score
    assert _render(lib, score=None, source=1, use_ot=1) == -1 and "null" in err()   # and so does an overlay threshold
    assert _render(lib, batch=0) == -1 and "b=0" in err()
    assert _render(lib, batch=-3) == -1 and "b=-3" in err()
    assert _render(lib, source=3) == -1 and "source 3" in err()
    assert _render(lib, source=-1) == -1 and "source -1" in err()
    assert _render(lib, kind=3) == -1 and "segm_kind 3" in err()
    assert _render(lib, kind=-1) == -1 and "segm_kind -1" in err()
    assert _render(lib, kind=2, nc=1) == -1 and "nc >= 2" in err()
    assert _render(lib, bstride=5) == -1 and "stride" in err()

    assert _annotate(lib, out=None) == -1 and "null" in err()
    assert _annotate(lib, batch=0) == -1 and "b=0" in err()
    assert _annotate(lib, radius=-1) == -1 and "radius -1" in err()
    assert _annotate(lib, color=None) == -1 and "null" in err()
    from sfh_amd import visualize as V
    assert _annotate(lib, L=V.LABEL_MAX + 1) == -1 and "label" in err() and str(V.LABEL_MAX + 1) in err()
    assert _annotate(lib, L=0) == -1 and "label" in err()
    assert _annotate(lib, scale=0) == -1 and "scale" in err()
    assert _annotate(lib, score=None, source=0) == -1 and "null" in err()
    assert _annotate(lib, source=7, score=None) == -1 and "source 7" in err()
    # nothing to draw is not an error and launches nothing
    assert _annotate(lib, poi=None, labels=None) == 0
    assert _annotate(lib, radius=0, labels=None) == 0


def test_header_constants_match_the_python_side():
    from sfh_amd import visualize as V
    txt = open(os.path.join(ROOT, "include", "sfh_amd.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    assert V.SOURCES == {"auto": val("SFH_OVERLAY_AUTO"), "warp": val("SFH_OVERLAY_WARP"), "segm": val("SFH_OVERLAY_SEGM")}
    assert V.LABEL_MAX == val("SFH_OVERLAY_LABEL_MAX")


def test_glyph_table_is_the_same_in_python_hip_and_the_restatement():
    from sfh_amd import visualize as V
    src = open(os.path.join(ROOT, "sports-field-homography_amd", "csrc", "overlay.hip")).read()
    body = src[src.index("kGlyphs[SFH_OVERLAY_NGLYPHS][7] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    rows = [tuple(int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]+", line)) for line in body.splitlines() if "{" in line]
    assert int(re.search(r"#define SFH_OVERLAY_NGLYPHS (\d+)", src).group(1)) == len(rows) == len(V.CHARSET)
    assert tuple(rows) == tuple(V.GLYPHS)
    assert V.CHARSET == R.CHARSET
    for k, ch in enumerate(V.CHARSET):
        assert V.GLYPHS[k] == R.glyph_rows(ch), ch
        assert all(0 <= r < 32 for r in V.GLYPHS[k])
    # the character set the issue names: digits, . - + e, space and the letters of nan / inf
    assert set(V.CHARSET) == set("0123456789.-+e naninf")
    # every string '{:4f}'.format produces is drawable
    for s in (0.0, 0.123456, -1.5, 1e20, float("nan"), float("inf"), -float("inf")):
        V.encode_labels(['{:4f}'.format(s)], 1)


def test_labels_are_encoded_and_refused():
    from sfh_amd import visualize as V
    codes = V.encode_labels(["0.17", "nan", ""], 3)
    assert codes.dtype == np.int8 and codes.shape == (3, 4)
    assert codes[0].tolist() == [0, 10, 1, 7] and codes[1].tolist() == [15, 16, 15, -1] and codes[2].tolist() == [-1] * 4
    with pytest.raises(ValueError, match="not in the overlay font"):
        V.encode_labels(["0.5x"], 1)
    with pytest.raises(ValueError, match="not in the overlay font"):
        V.encode_labels(["Score"], 1)
    with pytest.raises(ValueError):
        V.encode_labels(["1"], 2)
    with pytest.raises(ValueError, match="at most"):
        V.encode_labels(["1" * (V.LABEL_MAX + 1)], 1)


def test_renderer_refuses_cpu_tensors_and_bad_arguments():
    from sfh_amd import synth
    from sfh_amd import visualize as V
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    r = V.OverlayRenderer(court, source="warp")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(torch.zeros(1, 36, 64, 3, dtype=torch.uint8), torch.eye(3).reshape(1, 1, 3, 3))
    with pytest.raises(ValueError):
        r(torch.zeros(1, 36, 64, 3), torch.eye(3).reshape(1, 1, 3, 3))           # float frames
    with pytest.raises(ValueError):
        V.OverlayRenderer(court, source="both")
    with pytest.raises(ValueError):
        V.OverlayRenderer(court, marker_radius=-1)
    with pytest.raises(NotImplementedError):
        V.OverlayRenderer(court, mask_classes=5)


def test_frame_pipeline_validates_the_overlay_arguments():
    from sfh_amd import synth
    from sfh_amd import visualize as V
    from sfh_amd.pipeline import FramePipeline
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    net = torch.nn.Linear(1, 1)           # never reached: the overlay arguments are checked first
    with pytest.raises(ValueError, match="OverlayRenderer"):
        FramePipeline(net, 2, (360, 640), req_outputs=("theta", "overlay"))
    with pytest.raises(ValueError, match="consistency"):
        FramePipeline(net, 2, (360, 640), req_outputs=("theta", "overlay"), overlay=V.OverlayRenderer(court, source="auto"))
    with pytest.raises(ValueError, match="consistency"):
        FramePipeline(net, 2, (360, 640), req_outputs=("theta", "overlay"),
                      overlay=V.OverlayRenderer(court, source="warp", overlay_threshold=0.5))
    # a forced source passes the overlay checks and gets as far as the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FramePipeline(net, 2, (360, 640), req_outputs=("theta", "overlay"), overlay=V.OverlayRenderer(court, source="warp"))


def _write_preds(tmp_path, names, thetas, scores, masks=None):
    from sfh_amd import outputs as O
    with O.CourtJsonWriter(str(tmp_path), "game", "model-x") as w:
        for n, t, s in zip(names, thetas, scores):
            w.add(n, score=s, theta=t.reshape(1, 3, 3))
    mpath = None
    if masks is not None:
        with O.MaskPickleWriter(str(tmp_path), "mask") as mw:
            for n, m in zip(names, masks):
                mw.write(n, m)
        mpath = mw.path
    return os.path.join(str(tmp_path), "game_court.json"), mpath


def test_visualize_writes_one_png_per_frame(tmp_path):
    from sfh_amd import outputs as O
    from sfh_amd import synth
    from sfh_amd import visualize as V
    H, W, N = 45, 80, 5
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    g = np.random.default_rng(3)
    frames = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    thetas = np.stack([np.eye(3, dtype=np.float32)] + [m for m in synth.REALISTIC_THETAS[:2]]
                      + [np.eye(3, dtype=np.float32) + g.normal(0, 0.1, (3, 3)).astype(np.float32) for _ in range(2)])
    scores = [0.05, 0.5, 0.0999, 0.1, 2.25]
    masks = g.integers(0, 4, (N, 30, 40), dtype=np.uint8)          # a stream of another size: resized by the renderer
    names = [str(k) for k in range(N)]
    preds, mpath = _write_preds(tmp_path, names, thetas, scores, masks)
    stub = R.StubRenderer(court, score_threshold=0.1)
    dst = tmp_path / "viz"
    written = V.visualize(iter(frames), preds, str(dst), court, masks_path=mpath, batch=2, names=names, renderer=stub, device="cpu")
    assert stub.calls == [2, 2, 1]
    assert [os.path.basename(p) for p in written] == [f"{k}.png" for k in range(N)]
    assert sorted(os.listdir(dst)) == sorted(f"{k}.png" for k in range(N))
    fs = [O.format_score(s) for s in scores]
    plain = R.render(frames, torch.from_numpy(thetas), court, score=np.array(fs, np.float32), segm=masks, score_threshold=0.1,
                     shared=True)
    want = R.annotate(plain.copy(), labels=['{:4f}'.format(s) for s in fs], score=np.array(fs, np.float32), score_threshold=0.1)
    for k in range(N):
        got = O.decode_png(np.frombuffer(open(dst / f"{k}.png", "rb").read(), np.uint8))
        assert got.shape == (H, W, 3) and np.array_equal(got, want[k]), k
    assert not np.array_equal(plain, frames)       # a court was drawn
    # the frames on the warp side of the threshold carry a (0,255,0) label, the others a (0,0,255) one
    lit = [tuple(int(v) for v in want[k][(want[k] != plain[k]).any(-1)][0]) for k in range(N)]
    assert lit == [(0, 255, 0), (0, 0, 255), (0, 255, 0), (0, 0, 255), (0, 0, 255)]


def test_visualize_checks_the_name_alignment(tmp_path):
    from sfh_amd import synth
    from sfh_amd import visualize as V
    court = synth.load_court_template("ncaa_nc4_640x360", 4, 1)
    frames = np.zeros((3, 18, 32, 3), np.uint8)
    thetas = np.stack([np.eye(3, dtype=np.float32)] * 3)
    masks = np.zeros((3, 18, 32), np.uint8)
    stub = R.StubRenderer(court)
    # the mask stream names another frame than the predictions
    (tmp_path / "a").mkdir()
    preds, _ = _write_preds(tmp_path / "a", ["0", "1", "2"], thetas, [0.0] * 3)
    (tmp_path / "b").mkdir()
    _, mpath = _write_preds(tmp_path / "b", ["0", "2", "1"], thetas, [0.0] * 3, masks)
    with pytest.raises(ValueError, match="not aligned"):
        V.visualize(frames, preds, str(tmp_path / "out"), court, masks_path=mpath, renderer=stub, device="cpu")
    # the caller's frame names disagree with the predictions
    with pytest.raises(ValueError, match="not aligned"):
        V.visualize(frames, preds, str(tmp_path / "out"), court, names=["0", "1", "3"], renderer=stub, device="cpu")
    # frame count and prediction count differ
    with pytest.raises(ValueError, match="frames"):
        V.visualize(frames[:2], preds, str(tmp_path / "out"), court, renderer=stub, device="cpu")
    with pytest.raises(ValueError, match="frames"):
        V.visualize(np.zeros((4, 18, 32, 3), np.uint8), preds, str(tmp_path / "out"), court, renderer=stub, device="cpu")
    # aligned: passes, without a mask stream the frames above the threshold are copied
    written = V.visualize(frames, preds, str(tmp_path / "ok"), court, names=["0", "1", "2"], renderer=R.StubRenderer(court), device="cpu")
    assert len(written) == 3
    assert json.load(open(preds))["model"] == "model-x"
