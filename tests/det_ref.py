"""The sum pass of the deterministic training mode, restated in numpy from the text of include/sfh_amd.h ("Deterministic
training mode"); imports nothing from the library.

    dst[e] = (...((dst0[e] + p_0[e]) + p_1[e]) + ...) + p_{R-1}[e]

the ascending chain over the R slabs, starting from what the destination held, every add rounded once in the accumulator's
own type (float32 for raw, float64 for the fp64 accumulators).  numpy adds two arrays of one dtype element by element in that
dtype, so a loop over the slabs IS the chain of every element.

The slab geometry of each entry (R = slabs, E = elements per slab) is restated here too, from the table of that header
section, for the entries whose R is a closed form; the backward-filter split counts are the launch plan's own
(csrc/det_core.h) and come from the size queries."""
import numpy as np


def det_sum(dst0, partial):
    """dst0 (E,), partial (R, E), one dtype (float32 or float64) -> (E,) in that dtype"""
    partial = np.asarray(partial)
    acc = np.array(dst0, dtype=partial.dtype, copy=True).reshape(-1)
    assert partial.ndim == 2 and partial.shape[1] == acc.size and partial.dtype in (np.float32, np.float64)
    for r in range(partial.shape[0]):
        acc = acc + partial[r]          # one rounding per element, in partial.dtype
        assert acc.dtype == partial.dtype
    return acc


def det_sum_columns(dst0, partial, ncol, n_off):
    """a backward-filter source: the compact slabs (R, rows * ncol) land on columns [n_off, n_off + ncol) of dst0 (rows, raw_n);
    the other columns keep their bits"""
    out = np.array(dst0, copy=True)
    rows = out.shape[0]
    out[:, n_off:n_off + ncol] = det_sum(out[:, n_off:n_off + ncol].reshape(-1), partial).reshape(rows, ncol)
    return out


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- slab geometry: (R, E) per entry, from the header's table
def red_blocks(npix):
    return min(1024, max(1, cdiv(npix, 256)))


def bn_slabs(npix, C):               # sfh_bn_stats_det, sfh_bn_bwd_reduce_det: [row][c]
    return red_blocks(npix), 2 * C


def colsum_slabs(npix, C):
    return red_blocks(npix), C


def outconv_slabs(npix, nc, cin):    # [k][ci], then [k]
    ppb = max(1024, 256 * cdiv(npix // 1024, 256))
    return cdiv(npix, ppb), nc * cin + nc


def avgpool_slabs(batch, C, nout):   # [j][c], then [j]
    return batch, nout * C + nout


def losses_slabs(npix):
    return min(2048, cdiv(npix, 256)), 3


def uv_slabs(total):
    return min(1024, cdiv(total, 256)), 1


def reproj_slabs(batch):
    return cdiv(batch, 64), 1


def warp_slabs(batch, h, w):         # block (x, y) -> y * gx + x; [b][k]
    return cdiv(w, 256) * cdiv(h, 4), 9 * batch


def grouped_slabs(batch, H, W, groups, cg, stride):
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return batch * cdiv(ho, 8 if stride == 1 else 4) * cdiv(wo, 16), groups * cg * 9 * cg


def cancelling(R, E, dtype, seed=0):
    """slabs whose sum shows the order: (big, 1, -big, 1, ...) rows with big beyond the type's integer range, shuffled per
    column by a fixed permutation - any other order of the same rows gives other bits in most columns"""
    rng = np.random.default_rng(seed)
    big = dtype(1e8) if dtype == np.float32 else dtype(1e17)
    base = np.empty(R, dtype=dtype)
    base[0::4], base[1::4], base[2::4], base[3::4] = big, 1, -big, 1
    p = np.empty((R, E), dtype=dtype)
    for e in range(E):
        p[:, e] = base[rng.permutation(R)]
    return p
