"""Shared inputs of the label-preparation tests (tests/test_prep_host.py, tests/test_gpu_prep.py): realistic homographies and
synthetic manual annotations built from them in fp64."""
import os

import numpy as np

from conftest import GOLDEN, ROOT

DATA = os.path.join(ROOT, "sports-field-homography_amd", "data")


def court_poi(name="pitch"):
    return np.load(os.path.join(DATA, f"court_poi_{name}.npy")).astype(np.float64)


def court_ids(name="ncaa_nc4_640x360"):
    return np.load(os.path.join(DATA, f"court_ids_{name}.npy"))


def fixture_thetas():
    """frame -> court homographies, fp64 (n,3,3), last entry 1: the two golden predictions of full_640x360.npz, the two
    published predictions of synth.REALISTIC_THETAS and four mild perturbations of the identity"""
    from sfh_amd import synth
    th = [t for t in np.load(os.path.join(GOLDEN, "full_640x360.npz"))["theta"].reshape(-1, 3, 3).astype(np.float64)]
    th += [t for t in synth.REALISTIC_THETAS.astype(np.float64)]
    g = np.random.default_rng(11)
    th += [np.eye(3) + g.normal(0, 0.04, (3, 3)) for _ in range(4)]
    return np.stack([t / t[2, 2] for t in th])


def project(theta, court):
    """court points through inverse(theta) (plain homogeneous division) to [0,1] frame coordinates, fp64"""
    M = np.linalg.inv(theta)
    q = np.concatenate([court, np.ones((court.shape[0], 1))], axis=1) @ M.T
    return (q[:, :2] / q[:, 2:3]) / 2.0 + 0.5


def project_c2f(theta_c2f, court):
    """court points through a court -> frame matrix (plain homogeneous division) to [0,1] frame coordinates, fp64"""
    q = np.concatenate([court, np.ones((court.shape[0], 1))], axis=1) @ np.asarray(theta_c2f, dtype=np.float64).reshape(3, 3).T
    return (q[:, :2] / q[:, 2:3]) / 2.0 + 0.5


def inside(p):
    return (p[:, 0] >= 0) & (p[:, 0] <= 1) & (p[:, 1] >= 0) & (p[:, 1] <= 1)


def exact_annotations(court, thetas, seed=3, n_short=2, noise_px=0.0, size=(1280, 720)):
    """manual poi (B,N,2): frame k shows between 4 and N of the points that fall inside the frame (the rest are (-1,-1)),
    frame 0 all of them; the last n_short frames show exactly 3 points.  noise_px: Gaussian click noise in pixels of
    ``size``.  Returns manual, the number of frames built with fewer than 4 points."""
    g = np.random.default_rng(seed)
    B, N = thetas.shape[0], court.shape[0]
    manual = np.full((B, N, 2), -1.0)
    for b in range(B):
        p = project(thetas[b], court)
        vis = np.flatnonzero(inside(p))
        assert vis.size >= 4, f"fixture theta {b} leaves {vis.size} template points inside the frame"
        if b >= B - n_short:
            keep = g.choice(vis, 3, replace=False)
        elif b == 0:
            keep = vis
        else:
            keep = g.choice(vis, int(g.integers(4, vis.size + 1)), replace=False)
        q = p[keep]
        if noise_px:
            q = q + g.normal(0, noise_px, q.shape) / np.asarray(size, dtype=np.float64)
        manual[b, keep] = q
    return manual, n_short
