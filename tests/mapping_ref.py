"""numpy / torch restatement of csrc/mapping.hip on the CPU (test infrastructure only, holds no tests).

* ``inverse_theta``: tests/prep_ref.py:inverse_h33's formula without its final normalisation - adjugate / determinant,
  evaluated as the kernel (and sfh_poi_project_fwd before it) does: the adjugate times the fp64 reciprocal of the
  determinant, every operation individually rounded, each entry rounded once to fp32.
* ``top_view``: ``oracle.warp_ref.homography_warp(theta_c2f, frames.float().permute(0,3,1,2), hc, wc, mode)`` plus the
  quantisation rule (nearest: the tap's bytes; bilinear: round half to even, clamped to a byte) and ``valid``.
* ``mosaic_add`` / ``mosaic_finish``: the integer rule of the court mosaic.
* ``map_points``: the point rule in fp64 (cv2.perspectiveTransform's published rule; OpenCV is not needed).
"""
import numpy as np
import torch

from oracle import warp_ref

FLT_EPSILON = float(np.finfo(np.float32).eps)


def inverse_theta_f64(theta):
    """theta (B,3,3) float32 -> (inverse (B,3,3) float64 before its rounding to fp32, det (B,) float64)"""
    th = np.asarray(theta, dtype=np.float32).reshape(-1, 9)
    out = np.zeros(th.shape, dtype=np.float64)
    dets = np.zeros((th.shape[0],), dtype=np.float64)
    with np.errstate(all="ignore"):
        for b, t in enumerate(th):
            m = t.astype(np.float64)
            c00 = m[4] * m[8] - m[5] * m[7]
            c01 = m[5] * m[6] - m[3] * m[8]
            c02 = m[3] * m[7] - m[4] * m[6]
            det = (m[0] * c00 + m[1] * c01) + m[2] * c02
            inv = np.float64(1.0) / det
            adj = [c00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                   c01, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                   c02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
            out[b] = [a * inv for a in adj]
            dets[b] = det
    return out.reshape(-1, 3, 3), dets


def inverse_theta(theta):
    """theta (B,3,3)|(B,1,3,3) float32 -> (theta_c2f (B,3,3) float32, status (B,) uint8)"""
    th = np.asarray(theta, dtype=np.float32).reshape(-1, 9)
    inv, det = inverse_theta_f64(th)
    status = (np.isfinite(th).all(axis=1) & np.isfinite(det) & (det != 0.0)).astype(np.uint8)
    with np.errstate(all="ignore"):
        out = np.where(status[:, None, None] != 0, inv, 0.0).astype(np.float32)
    return out, status


def used_frames(status, score=None, max_score=None):
    """status 0, a NaN score or a score above max_score: the frame is not used"""
    use = np.asarray(status) != 0
    if score is not None and max_score is not None:
        with np.errstate(invalid="ignore"):
            use &= np.asarray(score, dtype=np.float32) <= np.float32(max_score)      # False for NaN
    return use


def _valid(theta_c2f_b, H, W, hc, wc):
    """(hc,wc) bool: the nearest tap of every court pixel lies inside the H x W frame"""
    grid = warp_ref.warp_grid(theta_c2f_b, hc, wc)
    px = warp_ref.unnormalize(grid[..., 0], W)[0]
    py = warp_ref.unnormalize(grid[..., 1], H)[0]
    rx, ry = torch.round(px), torch.round(py)
    ok = torch.isfinite(px) & torch.isfinite(py) & (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    return ok.numpy()


def top_view(frames, theta_c2f, status, hc, wc, mode="nearest", score=None, max_score=None):
    """frames uint8 (B,H,W,3) -> (top uint8 (B,hc,wc,3), valid uint8 (B,hc,wc), value float32 (B,hc,wc,3): the oracle's
    unquantised result)"""
    frames = np.asarray(frames)
    B, H, W = frames.shape[:3]
    th = torch.from_numpy(np.asarray(theta_c2f, dtype=np.float32).reshape(B, 3, 3))
    use = used_frames(status, score, max_score)
    top = np.zeros((B, hc, wc, 3), dtype=np.uint8)
    val = np.zeros((B, hc, wc, 3), dtype=np.float32)
    valid = np.zeros((B, hc, wc), dtype=np.uint8)
    for b in range(B):
        if not use[b]:
            continue
        img = torch.from_numpy(frames[b:b + 1]).float().permute(0, 3, 1, 2)
        v = warp_ref.homography_warp(th[b:b + 1], img, hc, wc, mode)[0].permute(1, 2, 0).numpy()
        val[b] = v
        top[b] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        valid[b] = np.where(_valid(th[b:b + 1], H, W, hc, wc), 255, 0)
    return top, valid, val


def mosaic_add(sum_, count, frames, theta_c2f, status, score=None, max_score=None):
    """sum (hc,wc,3) / count (hc,wc) uint32 accumulators += the valid nearest taps of the used frames, in place"""
    hc, wc = count.shape
    top, valid, _ = top_view(frames, theta_c2f, status, hc, wc, "nearest", score, max_score)
    ok = valid != 0
    sum_ += (top.astype(np.uint32) * ok[..., None]).sum(axis=0, dtype=np.uint32)
    count += ok.sum(axis=0, dtype=np.uint32)


def mosaic_finish(sum_, count):
    s, n = sum_.astype(np.uint64), count.astype(np.uint64)[..., None]
    q = (2 * s + n) // np.maximum(2 * n, 1)
    return np.where(n > 0, np.minimum(q, 255), 0).astype(np.uint8)


def project_f64(x, y, t):
    """x, y (N,) float64 through t (N,9) float64: the 3 x 3 product in the order ((t0 x + t1 y) + t2) and
    cv2.perspectiveTransform's w' = 1 / w if |w| > FLT_EPSILON else 0 -> (X w', Y w', w'), nothing rounded to fp32"""
    with np.errstate(all="ignore"):
        X = (t[:, 0] * x + t[:, 1] * y) + t[:, 2]
        Y = (t[:, 3] * x + t[:, 4] * y) + t[:, 5]
        Wh = (t[:, 6] * x + t[:, 7] * y) + t[:, 8]
        wi = np.where(np.abs(Wh) > FLT_EPSILON, 1.0 / Wh, 0.0)
        return X * wi, Y * wi, wi


def map_points(points, frame_index, thetas, in_size=None, out_scale=(1.0, 1.0)):
    """points (N,2) float32, frame_index (N,) int (or one int), thetas (F,3,3) float32 -> (out (N,2) float32, flag (N,) uint8)"""
    p = np.array(points, dtype=np.float32).reshape(-1, 2)
    N = p.shape[0]
    th = np.asarray(thetas, dtype=np.float32).reshape(-1, 9)
    F = th.shape[0]
    idx = np.broadcast_to(np.asarray(frame_index, dtype=np.int64), (N,))
    inside = (idx >= 0) & (idx < F)
    t = th[np.where(inside, idx, 0)].astype(np.float64)
    x, y = p[:, 0].copy(), p[:, 1].copy()
    with np.errstate(all="ignore"):
        if in_size is not None:     # transform.py:38-39 on its float32 array
            x = (x / np.float32(in_size[0]) - np.float32(0.5)) * np.float32(2.0)
            y = (y / np.float32(in_size[1]) - np.float32(0.5)) * np.float32(2.0)
        pu, pv, wi = project_f64(x.astype(np.float64), y.astype(np.float64), t)
        u = ((pu / 2.0 + 0.5) * np.float64(out_scale[0])).astype(np.float32)
        v = ((pv / 2.0 + 0.5) * np.float64(out_scale[1])).astype(np.float32)
    ok = inside & (wi != 0.0) & np.isfinite(u) & np.isfinite(v)
    out = np.stack([np.where(ok, u, np.float32(0)), np.where(ok, v, np.float32(0))], axis=1).astype(np.float32)
    return out, ok.astype(np.uint8)
