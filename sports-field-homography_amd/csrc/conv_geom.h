// conv_geom.h - the conventions the forward conv kernels share, stated once: the out-of-range offset, the tile grid over the
// flattened row space (host), the row split that undoes it (device) and the workgroup -> (pixel tile, cout block) orders.
// conv_s3.hip, conv_mfma.hip, conv_c4h2.hip, conv_small.hip, conv_upfused.hip, conv_inc_fused.hip and conv_epilogue.h call
// these; engine.py restates the grid (_zero_rows, _ntiles) where it chooses tiles.  tests/conv_geom_host_main.cpp runs this
// file on the CPU: every order is a bijection, the reciprocal division is exact wherever the guard admits, and Python agrees.
//
// Plain C++, no HIP header: SFH_GEOM_FN marks what the device runs too.
#pragma once

#if defined(__HIPCC__)
#define SFH_GEOM_FN __host__ __device__ __forceinline__
#else
#define SFH_GEOM_FN inline
#endif

// All global accesses of these kernels are buffer loads / stores with 32-bit byte offsets.  A slot outside the frame carries
// this offset: the descriptor's range check rejects it (loads return zeros, stores are dropped) without a branch.
constexpr unsigned kSfhOOB = 0xFFFFFFF0u;
// ... which is why a tensor must end below it to be addressed through one descriptor ("the 4 GiB range")
SFH_GEOM_FN bool sfh_fits_descriptor(unsigned long long bytes) { return bytes < kSfhOOB; }

SFH_GEOM_FN int sfh_geom_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- the tile grid -------------------------------------------------------------------------------------------------------
// Stride 1 ("flat"): the output rows of all frames form ONE row space, consecutive frames separated by shared zero rows, so
// that row tiles may straddle frames and only the last tile is partial.  Zero rows per frame: the padding before the window
// (ksize / 2); the split-operand kernels add one where that leaves an odd count of rows per frame, so that a 2x2 pool
// window of the fused max-pool output never straddles a tile edge (tile heights are even).
SFH_GEOM_FN int sfh_zero_rows(int ksize, int Ho, bool even_rows) {
  int zr = ksize / 2;
  if (even_rows) zr += (Ho + zr) & 1;
  return zr;
}

// (geometry structs without a tiles_y field - kernels that never need it - are served too)
template <class G>
SFH_GEOM_FN auto sfh_set_tiles_y(G& g, int v, int) -> decltype((void)g.tiles_y) { g.tiles_y = v; }
template <class G>
SFH_GEOM_FN void sfh_set_tiles_y(G&, int, long) {}

// Fills Ho, Wo, rows_per_img, rows_total, rows_magic, tiles_x, tiles_y (tiles per image where !flat) and ntiles of a kernel's
// geometry struct for th x tw tiles.  flat: the row space above, r = b * rows_per_img + y, split on the device by
// sfh_row_split with rows_magic = floor(2^32 / rows_per_img) + 1; !flat (stride 2, conv_small): tiles per image, a tile's
// first row travels as (b << 16) | y.  false: the geometry is refused - the reciprocal would not be exact for every row a
// tile can reach (rows_total + 63 at most; one row per frame has no 32-bit reciprocal), b / y do not fit their halves, or
// the tiles are not countable in an int.
template <class G>
SFH_GEOM_FN bool sfh_conv_grid(G& g, int batch, int H, int W, int ksize, int stride, bool flat, bool even_rows, int th, int tw) {
  const int pad2 = ksize / 2 + (ksize - 1) / 2;   // padding before + after
  g.Ho = (H + pad2 - ksize) / stride + 1;
  g.Wo = (W + pad2 - ksize) / stride + 1;
  g.tiles_x = sfh_geom_cdiv(g.Wo, tw);
  if (flat) {
    g.rows_per_img = g.Ho + sfh_zero_rows(ksize, g.Ho, even_rows);
    const long long rows = (long long)batch * g.rows_per_img;
    if (g.rows_per_img < 2 || (unsigned long long)(rows + 64) * (unsigned)g.rows_per_img >= (1ULL << 32)) return false;
    g.rows_total = (int)rows;
    g.rows_magic = (unsigned)((1ULL << 32) / (unsigned)g.rows_per_img) + 1u;
    const int ty = sfh_geom_cdiv(g.rows_total, th);
    sfh_set_tiles_y(g, ty, 0);
    const long long nt = (long long)g.tiles_x * ty;
    g.ntiles = (int)nt;
    return nt < 0x7FFFFFFFLL;
  }
  g.rows_total = 0;
  g.rows_per_img = g.Ho;
  g.rows_magic = 0;
  const int ty = sfh_geom_cdiv(g.Ho, th);
  sfh_set_tiles_y(g, ty, 0);
  const long long nt = (long long)g.tiles_x * ty * batch;
  g.ntiles = (int)nt;
  return g.Ho < 65536 && batch < 32768 && nt < 0x7FFFFFFFLL;
}

// Row r of the flat row space -> frame b and row y inside it, by the reciprocal (exact for every r < rows_total + 64 of a
// geometry sfh_conv_grid admitted).  true: r is an OUTPUT row of a frame, neither a shared zero row nor behind the last frame
// (and ok, the caller's other conditions, holds).  A halo row is tested against the input frame by its caller: r >= 0,
// b < batch, y < H.
template <class G>
SFH_GEOM_FN bool sfh_row_split(const G& g, int r, int& b, int& y, bool ok = true) {
  b = (int)(unsigned)(((unsigned long long)(unsigned)r * g.rows_magic) >> 32);
  y = r - b * g.rows_per_img;
  return ok && r < g.rows_total && y < g.Ho;
}

// ---- workgroup -> (pixel tile, cout block) --------------------------------------------------------------------------------
// Workgroups go round-robin to the 8 XCDs (blockIdx & 7), each with its own 4 MB L2; every launcher sizes its grid as
// cdiv(ntiles, 8) * 8 * nblk, and a workgroup that is not live leaves at once (uniformly).  xcd = bid & 7, k = bid >> 3 for
// block bid (the k-th workgroup of its XCD).
struct SfhWg {
  int tile, nb;
  bool live;
};

// The tile-range-per-XCD order (round 6, profiles/r06_tcc_per_launch.txt).  XCD x owns the contiguous tile range
// [x * tpx, (x + 1) * tpx), tpx = cdiv(ntiles, 8): whole tile rows next to each other, so vertically adjacent tiles meet
// their halo rows in that L2 (tile = 8 * k + xcd measured 1.4x the L2 fills).  nb_group (a divisor of nblk) cout blocks of
// one pixel tile run back to back: its input tile is fetched into the L2 once instead of nb_group times, and a transposed
// conv completes its interleaved output rows there.  Across groups the tiles of ONE group run back to back, so that the
// workgroups resident on the XCD stream the same weight fragments.  reverse: every XCD walks its range backwards, i.e.
// starts on what it wrote last in the previous launch; nothing else changes.  conv_s3_kernel (it spells these statements out
// itself: inlined from here they compile to another schedule).
SFH_GEOM_FN SfhWg sfh_wg_xcd_range(int xcd, int kk, int ntiles, int nb_group, bool reverse) {
  const int tpx = (ntiles + 7) >> 3;
  const int per = tpx * nb_group;
  const int gi = kk / per, rr = kk - gi * per;
  const int nb = gi * nb_group + rr % nb_group;
  const int tl = reverse ? tpx - 1 - rr / nb_group : rr / nb_group;
  const int tile = xcd * tpx + tl;
  return SfhWg{tile, nb, tile < ntiles};
}
// ... with nb_group == nblk (all cout blocks of a tile back to back), forwards: conv_upfused, and conv_small (spelled out
// there) where all weights of the layer fit an XCD's L2 - with the weight-stationary order below every XCD reads the WHOLE
// input (ResNet layer3: 147 MB of L2 misses per launch for 33 MB of tensors; its weights are 2.4 MB)
SFH_GEOM_FN SfhWg sfh_wg_xcd_range_all(int xcd, int k, int ntiles, int nblk) {
  const int tpx = (ntiles + 7) >> 3;
  SfhWg w;
  w.nb = k % nblk;
  w.tile = xcd * tpx + k / nblk;
  w.live = w.tile < ntiles && k / nblk < tpx;
  return w;
}
// ... with one cout block: conv_inc_fused
SFH_GEOM_FN SfhWg sfh_wg_xcd_range_one(int xcd, int rr, int ntiles, bool reverse) {
  const int tpx = (ntiles + 7) >> 3;
  SfhWg w;
  w.nb = 0;
  w.tile = xcd * tpx + (reverse ? tpx - 1 - rr : rr);
  w.live = w.tile < ntiles;
  return w;
}

// The round-robin order: the cout blocks of one pixel tile stay on one XCD (its halo is re-read from that L2), tiles go
// round the XCDs.  conv_mfma, conv_c4h2 (one or two cout blocks, short K), and conv_small's fallback.
SFH_GEOM_FN SfhWg sfh_wg_round_robin(int xcd, int k, int ntiles, int nblk) {
  SfhWg w;
  w.nb = k % nblk;
  w.tile = (k / nblk) * 8 + xcd;
  w.live = w.tile < ntiles;
  return w;
}
// conv_small's weight-stationary order (nblk a multiple of 8): an XCD keeps to nblk / 8 cout blocks, whose weights stay in
// its L2, and walks all tiles for them
SFH_GEOM_FN SfhWg sfh_wg_weight_stationary(int xcd, int idx, int ntiles, int nblk) {
  const int per = nblk >> 3;
  SfhWg w;
  w.nb = xcd * per + idx % per;
  w.tile = idx / per;
  w.live = w.tile < ntiles;
  return w;
}
