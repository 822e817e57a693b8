"""Makes the two wide court-template fixtures, tests/golden/court_ids_ncaa_nc7_640x360.npz and ..._nc8_..., from the
reference's id templates.  Run once where a checkout of the reference exists; never collected, no test runs it, nothing
imports it.

    python tests/classes_golden_make.py REFERENCE_ROOT

The resize is open_court_template's (utils/dataset.py:51-55): PIL, NEAREST, to 640x360.  Data only: one uint8 (360, 640)
array of class ids per file, key "ids"; the 7-class template (assets/mask_ncaa_v4_wo-center_m_onehot.png) has ids 0..6, the
8-class one (assets/mask_ncaa_v4_m_onehot.png) ids 0..7, and the resize keeps every id.
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = {7: "mask_ncaa_v4_wo-center_m_onehot.png", 8: "mask_ncaa_v4_m_onehot.png"}


def main(ref_root):
    for nc, asset in ASSETS.items():
        img = Image.open(os.path.join(ref_root, "assets", asset)).resize((640, 360), resample=Image.NEAREST)
        ids = np.array(img)
        if ids.ndim != 2 or ids.dtype != np.uint8 or sorted(np.unique(ids)) != list(range(nc)):
            raise SystemExit(f"{asset}: expected a uint8 id image with ids 0..{nc - 1}, got {ids.dtype} {ids.shape} "
                             f"{np.unique(ids)}")
        np.savez_compressed(os.path.join(GOLD, f"court_ids_ncaa_nc{nc}_640x360.npz"), ids=ids)
        print(nc, ids.shape, np.bincount(ids.reshape(-1)).tolist())


if __name__ == "__main__":
    main(sys.argv[1])
