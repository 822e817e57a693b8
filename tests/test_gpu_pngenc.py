"""sfh_amd.pngenc on the MI355X: the device encoder against the numpy restatement tests/pngenc_ref.py, byte for byte."""
import os

import numpy as np
import pytest
import torch

import pngenc_cases as cases
import pngenc_ref as R

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 17)
_SMALL = cases.small_cases()
# at full size one gray and one colour case
_FULL = {"ncaa_640x360_gray": lambda: cases.template("ncaa_nc4_640x360"),
         "pitch_1280x720_rgb": lambda: cases.template("pitch_v3_nc4_1280x720", rgb=True)}
_REFS = {}


def _case(name):
    return _SMALL[name] if name in _SMALL else _FULL[name]()


def _batch_and_refs(name):
    """17 variants of a case and their reference files, computed once"""
    if name not in _REFS:
        img = _case(name)
        imgs = [cases.variant(img, k) for k in range(max(BATCHES))]
        _REFS[name] = (np.stack(imgs), [np.frombuffer(R.ref_encode(im), np.uint8) for im in imgs])
    return _REFS[name]


def _encoder(img, batch, **kw):
    from sfh_amd.pngenc import PngEncoder
    return PngEncoder(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, batch, **kw)


@pytest.mark.parametrize("name", list(_SMALL) + list(_FULL))
def test_bytes_equal_restatement(name):
    imgs, refs = _batch_and_refs(name)
    enc = _encoder(imgs[0], max(BATCHES))
    dev = torch.from_numpy(imgs).cuda()
    for b in BATCHES:
        out = enc.encode(dev[:b].contiguous())
        files = out.to_host()
        sizes = out.sizes.cpu().numpy()
        off = out.offsets.cpu().numpy()
        assert len(files) == b
        for k in range(b):
            assert int(sizes[k]) == refs[k].size, f"{name} batch {b} image {k}: {int(sizes[k])} bytes, restatement {refs[k].size}"
            assert np.array_equal(files[k], refs[k]), f"{name} batch {b} image {k}: first difference at byte " \
                                                      f"{int(np.flatnonzero(files[k] != refs[k])[0])}"
        assert off[0] == 0 and np.array_equal(np.diff(off), sizes)            # compact: back to back


def test_rgb_switch_and_spread_layout():
    """bgr=False writes the tensor's channels as they are; compact=False puts file b at b * capacity"""
    img = _SMALL["333x187_rgb"]
    dev = torch.from_numpy(np.stack([img, cases.variant(img, 1)])).cuda()
    enc = _encoder(img, 2, bgr=False, compact=False)
    out = enc.encode(dev)
    off = out.offsets.cpu().numpy()
    assert off.tolist() == [0, enc.capacity, 2 * enc.capacity]
    data, sizes = out.data.cpu().numpy(), out.sizes.cpu().numpy()
    for k, im in enumerate((img, cases.variant(img, 1))):
        want = np.frombuffer(R.ref_encode(im, bgr=False), np.uint8)
        assert np.array_equal(data[off[k]:off[k] + sizes[k]], want)


def test_one_off_entry_point():
    from sfh_amd.outputs import decode_png
    from sfh_amd.pngenc import encode_png_device
    img = _SMALL["333x187_rgb"]
    buf = encode_png_device(torch.from_numpy(img).cuda())
    assert buf.dtype == np.uint8 and buf.ndim == 1 and np.array_equal(buf, np.frombuffer(R.ref_encode(img), np.uint8))
    assert np.array_equal(decode_png(buf), img)
    gray = np.stack([_SMALL["63x40"], cases.variant(_SMALL["63x40"], 2)])
    files = encode_png_device(torch.from_numpy(gray).cuda())
    assert [np.array_equal(decode_png(f), g) for f, g in zip(files, gray)] == [True, True]


def test_deterministic():
    imgs, _ = _batch_and_refs("333x187_rgb")
    enc = _encoder(imgs[0], 17)
    dev = torch.from_numpy(imgs).cuda()
    a, b = enc.new_output(), enc.new_output()
    a.data.zero_()
    b.data.zero_()
    enc.encode(dev, out=a)
    enc.encode(dev, out=b)
    assert torch.equal(a.data, b.data) and torch.equal(a.offsets, b.offsets) and torch.equal(a.sizes, b.sizes)


@pytest.mark.parametrize("compact", [True, False])
def test_guard_after_capacity_untouched(compact):
    """noise fills a file to its capacity (every strip stored): nothing may be written behind batch * capacity"""
    from sfh_amd.pngenc import PngBatch
    imgs, refs = _batch_and_refs("noise")
    B, guard = 3, 4096
    enc = _encoder(imgs[0], B, compact=compact)
    assert refs[0].size == enc.capacity                                       # the bound is reached
    buf = torch.full((B * enc.capacity + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = PngBatch(buf[:B * enc.capacity], torch.empty(B + 1, dtype=torch.int64, device="cuda"),
                   torch.empty(B, dtype=torch.int32, device="cuda"))
    enc.encode(torch.from_numpy(imgs[:B]).cuda(), out=out)
    torch.cuda.synchronize()
    assert bool((buf[B * enc.capacity:] == 0xA5).all())
    assert out.sizes.cpu().tolist() == [enc.capacity] * B


def _small_pipeline(**kw):
    from sfh_amd import synth
    from sfh_amd.pipeline import FramePipeline
    from sfh_amd.reconstructor import Reconstructor
    w, h, B = 112, 90, 2
    court = synth.load_court_template("ncaa_nc4_640x360", 4, B)[:, :, :h, :w].contiguous()
    poi = synth.load_court_poi("pitch", B)
    net = Reconstructor(court.cuda(), poi.cuda(), target_size=(w, h), unet_size=(w, h), warp_size=(w, h), warp_with_nearest=True)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 19))
    net.cuda().eval()
    return FramePipeline(net, B, (h, w), req_outputs=("theta", "warp_mask", "segm_mask"), consistency=True, **kw)


def _frames(n, B=2, h=90, w=112):
    from sfh_amd import synth
    return [torch.from_numpy(synth.synth_frames_u8(B, h, w, seed=40 + k)).pin_memory() for k in range(n)]


@pytest.mark.parametrize("budget", [None, 64])
def test_pipeline_png_outputs(budget, tmp_path):
    """decoded segm_mask_png / warp_mask_png == the raw masks of a pipeline without png; every other output bit-identical.
    budget 64: every batch overflows and takes the second copy.  The same files through MaskPickleWriter.write_encoded read
    back through MaskReader to the same masks."""
    from sfh_amd.outputs import MaskPickleWriter, MaskReader, decode_png
    frames = _frames(3)
    with torch.no_grad():
        plain = list(_small_pipeline().run(frames))
        coded = list(_small_pipeline(png=("segm_mask", "warp_mask"), png_budget=budget).run(frames))
    assert len(plain) == len(coded) == 3
    with MaskPickleWriter(str(tmp_path), "mask") as wr:
        for i, (p, c) in enumerate(zip(plain, coded)):
            assert sorted(c) == sorted([k for k in p if k not in ("segm_mask", "warp_mask")] + ["segm_mask_png", "warp_mask_png"])
            for k in c:
                if not k.endswith("_png"):
                    assert np.array_equal(p[k], c[k]), k
            for name in ("segm_mask", "warp_mask"):
                files = c[name + "_png"]
                assert len(files) == 2 and all(f.dtype == np.uint8 and f.ndim == 1 for f in files)
                for b in range(2):
                    assert np.array_equal(decode_png(files[b]), p[name][b]), (name, i, b)
                    assert np.array_equal(files[b], np.frombuffer(R.ref_encode(p[name][b]), np.uint8))
            for b in range(2):
                wr.write_encoded(f"{i}_{b}", c["segm_mask_png"][b])
    got = list(MaskReader(os.path.join(str(tmp_path), "mask", "data.pkl")).get(decode=True))
    assert [n for n, _ in got] == [f"{i}_{b}" for i in range(3) for b in range(2)]
    for (n, m), want in zip(got, [p["segm_mask"][b] for p in plain for b in range(2)]):
        assert np.array_equal(m, want), n
