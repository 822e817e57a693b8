"""numpy fp64 restatement of the label-preparation rules of sfh_amd.preparation (test infrastructure only), written from
the rule in that module's docstring / include/sfh_amd.h: Hartley-normalised DLT through the 9 x 9 L^T L, smallest
eigenvector by 12 cyclic Jacobi sweeps, denormalisation, damped Gauss-Newton polish that only accepts descending steps;
sums over points in the stated fixed order (slot = index mod 64, butterfly 32 .. 1).  Plus the host-side rules:
generate_uv_template, rescale_theta, preprocess_weight, rgb -> ids, and the fp64 form of transform_poi."""
import numpy as np

from chol8_ref import chol8_solve

SWEEPS = 12
_IDX = np.arange(64)


def wave_sum(vals):
    """vals (n, ...) per point -> the fixed-order sum over points: slot l adds points l, l + 64, .. in order, then the
    butterfly.  Returns (...)."""
    vals = np.asarray(vals, dtype=np.float64)
    n = vals.shape[0]
    slots = np.zeros((64,) + vals.shape[1:], dtype=np.float64)
    for k in range(0, n, 64):
        part = vals[k:k + 64]
        slots[:part.shape[0]] = slots[:part.shape[0]] + part
    o = 32
    while o:
        slots = slots + slots[_IDX ^ o]
        o >>= 1
    return slots[0]


def usable_points(manual):
    return (manual[:, 0] != -1.0) & (manual[:, 1] != -1.0)


def nonzero_flags(manual, ignore_pts=None):
    """find_nonzero_points"""
    f = ~((manual[:, 0] == -1.0) & (manual[:, 1] == -1.0))
    for i in (ignore_pts or ()):
        f[i] = False
    return f


def jacobi_smallest(A):
    """eigenvector of the smallest eigenvalue of the symmetric 9 x 9 A by SWEEPS cyclic Jacobi sweeps"""
    A = A.copy()
    V = np.eye(9)
    for _ in range(SWEEPS):
        for p in range(8):
            for q in range(p + 1, 9):
                app, aqq, apq = A[p, p], A[q, q], A[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(over="ignore"):          # a huge th gives t = 0, as on the device
                    th = (aqq - app) / (2.0 * apq)
                    t = (-1.0 if th < 0.0 else 1.0) / (abs(th) + np.sqrt(th * th + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                akp, akq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * akp - s * akq
                A[:, q] = s * akp + c * akq
                vkp, vkq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vkp - s * vkq
                V[:, q] = s * vkp + c * vkq
                apk, aqk = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c * apk - s * aqk
                A[q, :] = s * apk + c * aqk
                A[p, q] = 0.0
                A[q, p] = 0.0
    d = np.diag(A)
    kmin = 0
    for k in range(1, 9):
        if d[k] < d[kmin]:
            kmin = k
    return V[:, kmin].copy(), d


def forward_cost(h, src, dst, use):
    """summed squared forward reprojection error of h (9, h[8] = 1) over the usable points, the fixed-order sum"""
    x, y = src[:, 0], src[:, 1]
    iw = 1.0 / ((h[6] * x + h[7] * y) + 1.0)
    rx = ((h[0] * x + h[1] * y) + h[2]) * iw - dst[:, 0]
    ry = ((h[3] * x + h[4] * y) + h[5]) * iw - dst[:, 1]
    return float(wave_sum(np.where(use, rx * rx + ry * ry, 0.0)))


def dlt(src, dst, use):
    """src -> dst homography (9, last entry 1) from the usable pairs; also returns the eigenvalues of L^T L"""
    u8 = use.astype(np.float64)
    n = wave_sum(u8)
    cx1, cy1 = wave_sum(np.where(use, src[:, 0], 0.0)) / n, wave_sum(np.where(use, src[:, 1], 0.0)) / n
    cx2, cy2 = wave_sum(np.where(use, dst[:, 0], 0.0)) / n, wave_sum(np.where(use, dst[:, 1], 0.0)) / n
    ax, ay, bx, by = src[:, 0] - cx1, src[:, 1] - cy1, dst[:, 0] - cx2, dst[:, 1] - cy2
    sc1 = np.sqrt(2.0) / (wave_sum(np.where(use, np.sqrt(ax * ax + ay * ay), 0.0)) / n)
    sc2 = np.sqrt(2.0) / (wave_sum(np.where(use, np.sqrt(bx * bx + by * by), 0.0)) / n)
    x, y, u, v = ax * sc1, ay * sc1, bx * sc2, by * sc2
    z, one = np.zeros_like(x), np.ones_like(x)
    r1 = np.stack([-x, -y, -one, z, z, z, u * x, u * y, u], axis=1)
    r2 = np.stack([z, z, z, -x, -y, -one, v * x, v * y, v], axis=1)
    A = np.zeros((9, 9))
    for i in range(9):
        for j in range(i, 9):
            term = r1[:, i] * r1[:, j] + r2[:, i] * r2[:, j]
            A[i, j] = A[j, i] = wave_sum(np.where(use, term, 0.0))
    hn, eig = jacobi_smallest(A)
    M = np.zeros(9)
    for r in range(3):
        M[r * 3 + 0] = hn[r * 3 + 0] * sc1
        M[r * 3 + 1] = hn[r * 3 + 1] * sc1
        M[r * 3 + 2] = hn[r * 3 + 2] - (M[r * 3 + 0] * cx1 + M[r * 3 + 1] * cy1)
    h = np.zeros(9)
    for c in range(3):
        h[c] = M[c] / sc2 + cx2 * M[6 + c]
        h[3 + c] = M[3 + c] / sc2 + cy2 * M[6 + c]
        h[6 + c] = M[6 + c]
    return h / h[8], eig


def gn_system(h, src, dst, use, lam):
    """the damped normal equations of one Gauss-Newton step at h: (L, b, cost) - the 8 x 8 list of lists J^T J + lam
    diag(J^T J), the right-hand side -J^T r and the cost |r|^2, sums over points in the fixed order"""
    x, y = src[:, 0], src[:, 1]
    z = np.zeros_like(x)
    iw = 1.0 / ((h[6] * x + h[7] * y) + 1.0)
    px, py = ((h[0] * x + h[1] * y) + h[2]) * iw, ((h[3] * x + h[4] * y) + h[5]) * iw
    rx, ry = px - dst[:, 0], py - dst[:, 1]
    xi, yi = x * iw, y * iw
    jx = np.stack([xi, yi, iw, z, z, z, -(px * xi), -(px * yi)], axis=1)
    jy = np.stack([z, z, z, xi, yi, iw, -(py * xi), -(py * yi)], axis=1)
    JtJ = np.zeros((8, 8))
    for i in range(8):
        for j in range(i, 8):
            JtJ[i, j] = JtJ[j, i] = wave_sum(np.where(use, jx[:, i] * jx[:, j] + jy[:, i] * jy[:, j], 0.0))
    g = [wave_sum(np.where(use, jx[:, i] * rx + jy[:, i] * ry, 0.0)) for i in range(8)]
    L = [[JtJ[i, j] + lam * JtJ[i, j] if i == j else JtJ[i, j] for j in range(8)] for i in range(8)]
    return L, [-v for v in g], wave_sum(np.where(use, rx * rx + ry * ry, 0.0))


def refine_gn(h, src, dst, use, steps):
    h = h.copy()
    lam = 1e-3
    for _ in range(steps):
        L, yv, cost0 = gn_system(h, src, dst, use, lam)
        ok = chol8_solve(L, yv, True)
        hc = h.copy()
        hc[:8] = h[:8] + yv
        c1 = forward_cost(hc, src, dst, use)
        if ok and c1 < cost0:
            h = hc
            lam = lam / 10.0
        else:
            lam = lam * 10.0
    return h


def project_poi(theta_c2f, court):
    """transform_poi's rule in fp64 on the court -> frame matrix: Kornia's 1 / (z + 1e-8), then / 2 + 0.5"""
    h = np.asarray(theta_c2f, dtype=np.float64).reshape(9)
    x, y = court[:, 0], court[:, 1]
    X = (h[0] * x + h[1] * y) + h[2]
    Y = (h[3] * x + h[4] * y) + h[5]
    Z = (h[6] * x + h[7] * y) + h[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(np.abs(Z) > 1e-8, 1.0 / (Z + 1e-8), 1.0)
    return np.stack([(s * X) / 2.0 + 0.5, (s * Y) / 2.0 + 0.5], axis=1)


def reprojection_rmse(p1, p2, flags, norm=(1.0, 1.0)):
    """calculate_reprojection_rmse with the fixed-order sum"""
    ex = p1[:, 0] * norm[0] - p2[:, 0] * norm[0]
    ey = p1[:, 1] * norm[1] - p2[:, 1] * norm[1]
    f = flags.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return wave_sum(np.sqrt(ex * ex + ey * ey) * f) / wave_sum(f)


def inverse_h33(h):
    h = np.asarray(h, dtype=np.float64).reshape(9)
    inv = np.array([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                    h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                    h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]])
    return inv / inv[8]


def fit_frame(court, manual, ignore_pts=None, norm=(1.0, 1.0), refine=10):
    """one frame of sfh_prep_fit -> dict (status 0: everything else zero)"""
    court = np.asarray(court, dtype=np.float64)
    manual = np.asarray(manual, dtype=np.float64)
    N = court.shape[0]
    use = usable_points(manual)
    out = {"theta_c2f": np.zeros((3, 3)), "theta": np.zeros((3, 3)), "poi": np.zeros((N, 3)), "num_nonzero": 0,
           "reproj_mse": 0.0, "status": 0, "eig": np.zeros(9)}
    if int(use.sum()) < 4:
        return out
    dst = manual * 2.0 - 1.0
    h, eig = dlt(court, dst, use)
    if refine:
        h = refine_gn(h, court, dst, use, refine)
    flags = nonzero_flags(manual, ignore_pts)
    p = project_poi(h, court)
    out.update(theta_c2f=h.reshape(3, 3), theta=inverse_h33(h).reshape(3, 3),
               poi=np.concatenate([p, flags.astype(np.float64)[:, None]], axis=1), num_nonzero=int(flags.sum()),
               reproj_mse=float(reprojection_rmse(p, manual, flags, norm)), status=1, eig=eig)
    return out


def fit_batch(court, manual, ignore_pts=None, norm=(1.0, 1.0), refine=10):
    rows = [fit_frame(court, m, ignore_pts, norm, refine) for m in manual]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


# ---- host-side rules
def generate_uv_template(size, x_offset=(0, 0), y_offset=(0, 0)):
    """utils/court.py:102-128 for float32: the full (H,W) u and v images"""
    W, H = size
    gu, gv = np.meshgrid(np.linspace(1.0 / W, 1, num=W, dtype=np.float32), np.linspace(1.0 / H, 1, num=H, dtype=np.float32))
    u, v = np.zeros(gu.shape, np.float32), np.zeros(gv.shape, np.float32)
    x1, x2 = x_offset[0], W - x_offset[1] - 1
    y1, y2 = y_offset[0], H - y_offset[1] - 1
    u[y1:y2, x1:x2] = gu[y1:y2, x1:x2]
    v[y1:y2, x1:x2] = gv[y1:y2, x1:x2]
    return u, v


def rescale_theta(src_size, dst_size, theta):
    s = np.diag([float(dst_size[0]), float(dst_size[1]), 1.0])
    d = np.diag([1.0 / src_size[0], 1.0 / src_size[1], 1.0])
    return s @ np.asarray(theta, dtype=np.float64) @ d


def preprocess_weight(mse):
    x = (np.asarray(mse, dtype=np.float64) / 0.01 * 12 - 6) * 1.25 + 1
    return (1 - 1 / (1 + np.exp(-x))).astype(np.float32)


PALETTE = {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255), 4: (255, 255, 255), 5: (255, 0, 255), 6: (0, 255, 255),
           7: (255, 255, 0)}


def rgb_to_ids(rgb, num_classes):
    """convert_rgb_to_onehot's loop: pixel == colour k -> k, else channel 0"""
    out = rgb[..., 0].copy()
    for k in range(1, num_classes):
        out[np.all(rgb == np.array(PALETTE[k], dtype=np.uint8), axis=-1)] = k
    return out


class RefMaker:
    """LabelMaker.make's contract on the host (fit by this module, mask by the oracle's nearest warp): stands in for the
    device in the prepare_dataset test"""

    def __init__(self, court_ids, court_poi, size, ignore_pts=None, refine=10, uv=False, tables=None):
        self.ids, self.court, self.size = court_ids, np.asarray(court_poi, dtype=np.float64), size
        self.ignore, self.refine, self.uv, self.tables = ignore_pts, refine, uv, tables

    def make(self, manual):
        import torch
        from oracle import warp_ref
        out = fit_batch(self.court, np.asarray(manual, dtype=np.float64), self.ignore, refine=self.refine)
        out.pop("eig")
        W, H = self.size
        th = torch.from_numpy(out["theta"].astype(np.float32))
        tm = torch.from_numpy(self.ids.astype(np.float32))[None, None].expand(th.shape[0], 1, -1, -1)
        out["mask"] = warp_ref.homography_warp(th, tm, H, W, "nearest").numpy().astype(np.uint8)
        if self.uv:
            ix, iy, ok = tap_indices(th, self.ids.shape, H, W)
            u = np.where(ok, self.tables[0][ix], 0).astype(np.uint16)
            v = np.where(ok, self.tables[1][iy], 0).astype(np.uint16)
            out["uv"] = np.stack([out["mask"].astype(np.uint16), u, v], axis=-1)
        return out


def tap_indices(theta_f32, src_shape, h, w):
    """the oracle's nearest tap of every pixel: ix, iy (clamped, int64) and ok = inside the source image"""
    import torch
    from oracle import warp_ref
    Hs, Ws = src_shape
    grid = warp_ref.warp_grid(theta_f32, h, w)
    px, py = warp_ref.unnormalize(grid[..., 0], Ws), warp_ref.unnormalize(grid[..., 1], Hs)
    fin = torch.isfinite(px) & torch.isfinite(py)
    ix = torch.round(px).clamp(-2.0, Ws + 1.0).nan_to_num(-2.0).to(torch.int64)
    iy = torch.round(py).clamp(-2.0, Hs + 1.0).nan_to_num(-2.0).to(torch.int64)
    ok = fin & (ix >= 0) & (ix < Ws) & (iy >= 0) & (iy < Hs)
    return ix.clamp(0, Ws - 1).numpy(), iy.clamp(0, Hs - 1).numpy(), ok.numpy()
