"""Makes the two ResNeXt fixtures, tests/golden/resnext_stn.npz and tests/golden/resnext_layouts.json, with the reference's OWN
ResNetSTN class.  Run once where a checkout of the reference exists; never collected, no test runs it, nothing imports it.

    python tests/resnext_golden_make.py REFERENCE_ROOT

models/resnet.py is imported by file path (the reference's package __init__ pulls in Kornia), as oracle/make_fixtures.py
does; the weights are sfh_amd.synth's deterministic ones (seeds 21 and 22), the input is the (2,7,72,128) tensor of the
other depths' fixture (tests/golden/blocks.npz, resnet34_7.x).  Data only: two (2,1,3,3) thetas and the parameter layouts.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from oracle import golden  # noqa: E402
from sfh_amd import synth  # noqa: E402

# name -> (blocks per stage, width per group, seed); 32 groups (models/resnet.py:308-337)
VARIANTS = {"resnext50_32x4d": ([3, 4, 6, 3], 4, 21), "resnext101_32x8d": ([3, 4, 23, 3], 8, 22)}


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_resnet", os.path.join(ref_root, "models", "resnet.py"))
    rn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rn)
    x = torch.from_numpy(golden.load(os.path.join(GOLD, "blocks.npz"))["resnet34_7.x"])
    thetas, layouts = {}, {}
    torch.manual_seed(0)
    with torch.no_grad():
        for name, (layers, wpg, seed) in VARIANTS.items():
            m = rn.ResNetSTN(rn.Bottleneck, layers, groups=32, width_per_group=wpg, in_channels=7)
            m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed), strict=True)
            thetas[name + "_7.theta"] = m.eval()(x).numpy()
            layouts[name] = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
    np.savez_compressed(os.path.join(GOLD, "resnext_stn.npz"), **thetas)
    with open(os.path.join(GOLD, "resnext_layouts.json"), "w") as f:
        json.dump(layouts, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: v.reshape(-1)[:3] for k, v in thetas.items()})


if __name__ == "__main__":
    main(sys.argv[1])
