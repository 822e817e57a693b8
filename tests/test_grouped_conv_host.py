"""CPU checks of the grouped 3x3 convolution: the fp64 references of tests/grouped_conv_ref.py against torch's own grouped
conv and its autograd; the index arithmetic of csrc/conv_grouped_core.h, walked output by output by the stand-alone program
tests/grouped_conv_host_main.cpp under AddressSanitizer and UBSan, against those references on every case of
tests/grouped_conv_cases.py (integers and impulses exactly, randn inside its bound); and the ResNeXt parameter containers
against the fixtures made with the reference's own class (tests/resnext_golden_make.py)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grouped_conv_cases as K
import grouped_conv_ref as R
import host_program
from conftest import GOLDEN
from train_kernel_ref import ratio


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("case", [(2, 7, 5, 32, 4, 2), (1, 9, 20, 3, 4, 1), (2, 6, 7, 1, 64, 2)], ids=K.case_id)
def test_references_against_torch(case):
    """conv / bwd_data / wgrad restate F.conv2d(groups=) and its autograd (they call it; this pins the layout handling),
    and the absolute sums dominate the values"""
    B, H, W, G, cg, s = case
    x, w, dz, _ = K.randn_inputs(case)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_()
    wt = torch.from_numpy(w).double().requires_grad_()
    y = F.conv2d(xt, wt, None, s, 1, 1, G)
    gx, gw = torch.autograd.grad(y, (xt, wt), torch.from_numpy(dz).double().permute(0, 3, 1, 2))
    acc, A = R.conv(x, w, s)
    assert np.array_equal(acc, y.detach().permute(0, 2, 3, 1).numpy()) and (np.abs(acc) <= A * (1 + 1e-12)).all()
    dx, Ad = R.bwd_data(dz, w, s, H, W)
    assert np.allclose(dx, gx.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13) and (np.abs(dx) <= Ad * (1 + 1e-12)).all()
    dw, Aw = R.wgrad(dz, x, cg, s)
    assert np.allclose(dw, gw.numpy(), rtol=0, atol=1e-12) and (np.abs(dw) <= Aw * (1 + 1e-12)).all()
    # one element by hand: output channel o of group g, pixel (oy, ox)
    g, o, oy, ox = G - 1, cg - 1, (H - 1) // s, 0
    want = sum(float(x[0, oy * s + ky - 1, ox * s + kx - 1, g * cg + c]) * float(w[g * cg + o, c, ky, kx])
               for ky in range(3) for kx in range(3) for c in range(cg)
               if 0 <= oy * s + ky - 1 < H and 0 <= ox * s + kx - 1 < W)
    assert abs(acc[0, oy, ox, g * cg + o] - want) < 1e-12


def test_shifted_copy_is_the_impulse_response():
    case = (1, 5, 6, 2, 4, 2)
    src = K.impulse_source((1, 5, 6, 8))
    dz = K.impulse_source((1, 3, 3, 8))
    for w, g, o, c, ky, kx in K.impulse_weights(case):
        assert np.array_equal(R.conv(src, w, 2)[0], R.shifted_copy(src, g * 4 + c, g * 4 + o, ky, kx, 2))
        assert np.array_equal(R.bwd_data(dz, w, 2, 5, 6)[0], R.scattered_copy(dz, g * 4 + o, g * 4 + c, ky, kx, 2, 5, 6))


# ------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    return host_program.build_host_program(tmp_path_factory, "grouped_conv")


def _run_host(host_bin, d, case, x, w, dz, raw0, scale=None, shift=None, relu=False, forward_only=False):
    """-> y (n_w,B,Ho,Wo,C), dx (n_w,B,H,W,C), raw (C,9,cg) of the host program (forward_only: y alone); w: one weight or a
    list"""
    B, H, W, G, cg, s = case
    C, (ho, wo) = G * cg, K.out_hw(case)
    ws = w if isinstance(w, list) else [w]
    os.makedirs(d, exist_ok=True)
    dims = [B, H, W, G, cg, s, int(relu), int(scale is not None), len(ws), int(forward_only)]
    np.asarray(dims, dtype=np.int64).tofile(os.path.join(d, "dims.i64"))
    files = {"x": x, "w": np.stack(ws), "dz": dz, "raw0": raw0}
    if scale is not None:
        files.update(scale=scale, shift=shift)
    for name, a in files.items():
        np.ascontiguousarray(a, dtype=np.float32).tofile(os.path.join(d, name + ".f32"))
    r = subprocess.run([host_bin, str(d)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda name, *shape: np.fromfile(os.path.join(d, name), dtype=np.float32).reshape(shape)
    y = rd("y.f32", len(ws), B, ho, wo, C)
    return y if forward_only else (y, rd("dx.f32", len(ws), B, H, W, C), rd("raw.f32", C, 9, cg))


_WORST = {"forward": 0.0, "epilogue": 0.0, "backward-data": 0.0, "backward-filter": 0.0}


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_host_program_on_every_case(host_bin, tmp_path, case):
    """integers: the fp64 value bit for bit; randn: inside the bound, with and without the epilogue"""
    B, H, W, G, cg, s = case
    # small integers: exact
    x, w, dz, raw0 = K.int_inputs(case)
    y, dx, raw = _run_host(host_bin, tmp_path / "int", case, x, w, dz, raw0)
    assert np.array_equal(y[0].astype(np.float64), R.conv(x, w, s)[0])
    assert np.array_equal(dx[0].astype(np.float64), R.bwd_data(dz, w, s, H, W)[0])
    assert np.array_equal(R.raw_to_oihw(raw, cg).astype(np.float64), R.wgrad(dz, x, cg, s)[0] + R.raw_to_oihw(raw0, cg))
    # randn
    x, w, dz, raw0 = K.randn_inputs(case)
    acc, A = R.conv(x, w, s)
    y, dx, raw = _run_host(host_bin, tmp_path / "randn", case, x, w, dz, raw0)
    _WORST["forward"] = max(_WORST["forward"], ratio(y[0], acc, R.conv_bound(A, cg)))
    ref, Ad = R.bwd_data(dz, w, s, H, W)
    _WORST["backward-data"] = max(_WORST["backward-data"], ratio(dx[0], ref, R.conv_bound(Ad, cg)))
    dw, Aw = R.wgrad(dz, x, cg, s)
    r0 = R.raw_to_oihw(raw0, cg).astype(np.float64)
    _WORST["backward-filter"] = max(_WORST["backward-filter"],
                                    ratio(R.raw_to_oihw(raw, cg), dw + r0, R.wgrad_bound(Aw, r0, *K.wgrad_plan(case))))
    scale, shift = K.epilogue_inputs(case, acc)
    y = _run_host(host_bin, tmp_path / "epi", case, x, w, dz, raw0, scale, shift, relu=True, forward_only=True)
    want, bound = R.epilogue(acc, A, cg, scale, shift, True)
    _WORST["epilogue"] = max(_WORST["epilogue"], ratio(y[0], want, bound))
    assert np.array_equal(y[0][..., 1], np.full_like(y[0][..., 1], 0.25))      # the scale = 0 channel: the shift alone
    if want.size >= 64:
        assert 0.2 < (want > 0).mean() < 0.8                                    # the shift splits the outputs
    print("largest error / bound so far:", _WORST)
    assert max(_WORST.values()) <= 1.0, _WORST


@pytest.mark.parametrize("case", K.IMPULSE, ids=K.case_id)
def test_host_program_impulses(host_bin, tmp_path, case):
    """a single 1 in the weight: the output is one shifted, zero-padded source channel in one destination channel"""
    B, H, W, G, cg, s = case
    C, (ho, wo) = G * cg, K.out_hw(case)
    src, dz = K.impulse_source((B, H, W, C)), K.impulse_source((B, ho, wo, C))
    imp = list(K.impulse_weights(case))
    y, dx, _ = _run_host(host_bin, tmp_path / "imp", case, src, [t[0] for t in imp], dz, np.zeros((C, 9, cg), np.float32))
    for k, (_, g, o, c, ky, kx) in enumerate(imp):
        assert np.array_equal(y[k], R.shifted_copy(src, g * cg + c, g * cg + o, ky, kx, s)), (g, o, c, ky, kx)
        assert np.array_equal(dx[k], R.scattered_copy(dz, g * cg + o, g * cg + c, ky, kx, s, H, W)), (g, o, c, ky, kx)


# ------------------------------------------------------------------------------------------------ the containers
_SEEDS = {"resnext50_32x4d": 21, "resnext101_32x8d": 22}


@pytest.mark.parametrize("name", sorted(_SEEDS))
def test_resnext_container_layout_and_restated_stn(name, golden_blocks):
    """parameter names, shapes and dtypes are the reference's; the restated STN on the container's state dict gives the
    reference's theta"""
    from sfh_amd import modules, synth
    rn = modules.ResNetSTN(name, 7)
    with open(os.path.join(GOLDEN, "resnext_layouts.json")) as f:
        want = json.load(f)[name]
    got = {k: [list(v.shape), str(v.dtype)] for k, v in rn.state_dict().items()}
    assert got == want
    width = {"resnext50_32x4d": 128, "resnext101_32x8d": 256}[name]
    assert tuple(rn.layer1[0].conv2.weight.shape) == (width, width // 32, 3, 3) and rn.layer1[0].conv2.groups == 32
    sd = synth.synth_state_dict(rn.state_dict(), _SEEDS[name])
    rn.load_state_dict(sd, strict=True)
    with torch.no_grad():
        theta = R.resnet_stn(torch.from_numpy(golden_blocks["resnet34_7.x"]), sd, p="")
    g = np.load(os.path.join(GOLDEN, "resnext_stn.npz"))
    assert np.abs(theta.numpy() - g[name + "_7.theta"]).max() < 1e-6


def test_names_outside_the_table_are_still_refused():
    from sfh_amd import modules
    with pytest.raises(NotImplementedError):
        modules.ResNetSTN("resnext50_32x8d", 7)


def test_entry_points_refuse_without_a_device():
    """argument checks fire before anything touches a device"""
    from sfh_amd import _lib
    lib = _lib.load()
    assert lib.sfh_packed_grouped_weight_floats(32, 4) == 4 * 9 * 4 * 32 and lib.sfh_packed_grouped_weight_floats(3, 4) == 9 * 4 * 32
    assert lib.sfh_packed_grouped_weight_floats(32, 64) == 32 * 9 * 64 * 64
    for g, cg in ((32, 5), (32, 128), (0, 4), (32, 0)):
        assert lib.sfh_packed_grouped_weight_floats(g, cg) == -1
    assert lib.sfh_conv_grouped_fwd(None, None, None, None, 0, None, 2, 7, 5, 32, 4, 1, None) == -1
    assert b"null" in lib.sfh_last_error()
    assert lib.sfh_conv_grouped_wgrad(None, None, None, 2, 7, 5, 32, 4, 1, None) == -1
    assert lib.sfh_pack_grouped_weights(None, None, 32, 4, 0, None) == -1
