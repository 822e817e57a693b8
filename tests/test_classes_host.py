"""The 7- and 8-class court models, host side: the two template fixtures, the index arithmetic of the tap-packed stem kernels
(csrc/stem_core.h, walked by tests/stem_core_host_main.cpp under AddressSanitizer and UBSan) and the state-dict shapes of the
wide models.  No GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from host_program import build_host_program

# pixels per class id at 640x360 after open_court_template's NEAREST resize (utils/dataset.py:51-55) of the reference's
# assets mask_ncaa_v4_wo-center_m_onehot.png (7 classes) and mask_ncaa_v4_m_onehot.png (8 classes)
COUNTS = {7: [43200, 104692, 45975, 16417, 9694, 6360, 4062],
          8: [43200, 100302, 45975, 16417, 4116, 6360, 4062, 9968]}


def load_ids(nc):
    with np.load(os.path.join(GOLDEN, f"court_ids_ncaa_nc{nc}_640x360.npz")) as z:
        return z["ids"]


@pytest.mark.parametrize("nc", [7, 8])
def test_wide_template_fixture_has_every_id(nc):
    ids = load_ids(nc)
    assert ids.dtype == np.uint8 and ids.shape == (360, 640)
    assert np.bincount(ids.reshape(-1), minlength=nc).tolist() == COUNTS[nc]
    assert os.path.getsize(os.path.join(GOLDEN, f"court_ids_ncaa_nc{nc}_640x360.npz")) < 16384


@pytest.fixture(scope="module")
def stem_core_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "stem_core")


def test_stem_index_core_covers_every_tap_and_channel_once_and_stays_inside_the_halo(stem_core_program):
    """both instances (8 and 16 channels per tap): see the program's header for the two checks"""
    r = subprocess.run([stem_core_program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "OK", r.stdout
    # the figures the kernels' comments and the README state
    assert lines[0] == "CH=8 steps=13 tile=8x32 halo=21x69 lds3=69888 lds2=46592 packed3=159744", lines[0]
    assert lines[1] == "CH=16 steps=25 tile=8x16 halo=21x37 lds3=75264 lds2=50176 packed3=307200", lines[1]


@pytest.mark.parametrize("nc", [7, 8])
def test_wide_model_state_dict_shapes_follow_the_reference_rule(nc):
    """models/reconstructor.py:150-166: OutConv(64, mask_classes); resnet_input='img+mask' gives the STN mask_classes + 3
    input channels"""
    from sfh_amd import modules
    from sfh_amd.reconstructor import Reconstructor
    assert tuple(modules.OutConv(64, nc).conv.weight.shape) == (nc, 64, 1, 1)
    assert tuple(modules.resnet_stn("resnet34", in_channels=nc + 3).conv0.weight.shape) == (64, nc + 3, 7, 7)
    court = torch.from_numpy(load_ids(nc)[None, None, :90, :112].astype(np.float32) / nc)
    net = Reconstructor(court, torch.zeros(1, 4, 2), mask_classes=nc, target_size=(112, 90), unet_size=(112, 90),
                        warp_size=(112, 90))
    sd = net.state_dict()
    assert tuple(sd["outc.conv.weight"].shape) == (nc, 64, 1, 1) and tuple(sd["outc.conv.bias"].shape) == (nc,)
    assert tuple(sd["resnet_reg.conv0.weight"].shape) == (64, nc + 3, 7, 7)
