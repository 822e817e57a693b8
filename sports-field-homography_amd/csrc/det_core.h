// det_core.h - the partition arithmetic of the deterministic training mode, stated once.
//
// THE RULE.  In deterministic mode every sum that crosses workgroups is taken in two launches:
//   store pass: the accumulating kernel stores what it would have added - one value per element and SHARE of the work - into
//     its own SLAB of a caller-provided workspace.  The slab index is the index that selects the kernel's share: the pixel
//     split of a backward-filter launch, the block of a pixel reduction, the tile of the grouped backward-filter, the frame
//     of the pooled head.  Slab r holds elements [r * E, (r + 1) * E) of the workspace, E = elements per slab, in the
//     accumulator's own type (fp32 for raw, fp64 for the fp64 accumulators).  Every element of every slab is written exactly
//     once per launch with a plain store (an empty share stores zeros); no float atomic runs, no workgroup waits for another.
//   sum pass (det_reduce_kernel, csrc/det.hip): dst[e] = (...((dst0[e] + p_0[e]) + p_1[e]) + ...) + p_{R-1}[e] - the ASCENDING
//     CHAIN over the R slabs, starting from what the destination held (det_sum below), in the accumulator's precision.
// The result is a function of the operands and the geometry alone; it does not depend on what else runs on the device.
//
// Everything below is plain integer arithmetic that host and device evaluate alike.  What the library itself reads here:
// every accumulating launch has ONE PLAN (det_*_plan), a function of exactly the arguments of its size query: whether the
// geometry is admitted, the slab count, the elements per slab, the element size, and the grid numbers the launcher needs.
// The launcher of an entry and of its sibling (one static function for both), the size query (sfh_*_det_bytes) and
// tests/det_host_main.cpp all call that function; a geometric refusal is stated in the plan and nowhere else, and bytes are
// formed in det_bytes(plan) and nowhere else.  The DET kernels read the slab offsets (det_slab_offset), the backward-filter
// element offset (det_wgrad_elem) and det_add; the sum pass det_sum and det_dst_offset.  The share -> slab maps marked
// RESTATEMENT are not called by any kernel: a kernel's tile or pixel loop is the one its default instantiation has always had
// (that instruction stream must not move), and the map states beside it which slab that loop's share ends in, for
// tests/det_host_main.cpp to hold against the same loop written out on the host.
// Plain C++, no HIP header outside the __HIPCC__ block at the end.
#pragma once

#include "conv_grouped_core.h"   // gc_cg_ok: the group widths the grouped backward-filter admits

#if defined(__HIPCC__)
#define SFH_DET_FN __host__ __device__ __forceinline__
#else
#define SFH_DET_FN inline
#endif

SFH_DET_FN int det_cdiv(int a, int b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ plan, workspace and sum pass
// Which rule of a plan refused the geometry: the launcher words its message by it.  Families with one rule use DET_BAD_ARG.
enum DetWhy { DET_OK = 0, DET_BAD_ARG, DET_BAD_FRAME, DET_BAD_M, DET_BAD_N, DET_BAD_FIT, DET_BAD_KSIZE, DET_BAD_K4N, DET_BAD_CG,
              DET_BAD_STRIDE, DET_BAD_CIN, DET_BAD_NC, DET_TOO_LARGE };
// The share geometry of one launch.  A refused geometry is ok == false (why says which rule; slabs = 0).
struct DetPlan {
  bool ok;
  DetWhy why;
  long slabs, elems;   // elems: per slab
  int elem_bytes;
};
SFH_DET_FN DetPlan det_refuse(DetWhy why) { return DetPlan{false, why, 0, 0, 0}; }
SFH_DET_FN DetPlan det_admit(long slabs, long elems, int elem_bytes) { return DetPlan{true, DET_OK, slabs, elems, elem_bytes}; }
// what a size query answers: the workspace of the launch, -1 for a refused geometry
SFH_DET_FN long long det_bytes(const DetPlan& p) { return p.ok ? (long long)p.slabs * p.elems * p.elem_bytes : -1; }
SFH_DET_FN long det_slab_offset(long slab, long elems) { return slab * elems; }

// the sum pass of ONE element e: partial = the workspace, `stride` elements from slab to slab
template <typename T>
SFH_DET_FN T det_sum(T dst0, const T* partial, long slabs, long stride, long e) {
  T s = dst0;
  for (long r = 0; r < slabs; ++r) s += partial[r * stride + e];
  return s;
}
// element e of a slab whose rows are ncol wide -> offset in a destination whose rows are dst_row_stride apart (a
// backward-filter source that fills columns [n_off, n_off + N) of raw: ncol = N, dst_row_stride = raw_n, dst = raw + n_off)
SFH_DET_FN long det_dst_offset(long e, int ncol, long dst_row_stride) { return (e / ncol) * dst_row_stride + e % ncol; }

// ------------------------------------------------------------------ pixel reductions (csrc/train_bn.hip)
// sfh_bn_stats / sfh_colsum / sfh_bn_bwd_reduce: at most DET_RED_BLOCKS blocks of 256 threads, one more per DET_RED_ROWS
// pixels.  Slab = block.  Elements per slab: 2 * C (bn_stats, bn_bwd_reduce: [row][channel]) or C (colsum).
#define DET_RED_ROWS 256
#define DET_RED_BLOCKS 1024
SFH_DET_FN long det_red_blocks(long npix) {
  const long nb = (npix + DET_RED_ROWS - 1) / DET_RED_ROWS;
  return nb < 1 ? 1 : (nb > DET_RED_BLOCKS ? DET_RED_BLOCKS : nb);
}
// rows = 2: sfh_bn_stats, sfh_bn_bwd_reduce; rows = 1: sfh_colsum
SFH_DET_FN DetPlan det_red_plan(long npix, int C, int rows) {
  if (npix <= 0 || C <= 0 || C % 4 != 0) return det_refuse(DET_BAD_ARG);
  return det_admit(det_red_blocks(npix), (long)rows * C, sizeof(double));
}
// RESTATEMENT (host walk only) of the kernels' pixel loops:
// bn_stats: block b streams the contiguous range [b * chunk, min(npix, (b + 1) * chunk)), possibly empty
SFH_DET_FN long det_red_chunk(long npix, long nblocks) { return (npix + nblocks - 1) / nblocks; }
SFH_DET_FN long det_red_block_of_pixel_chunked(long p, long npix, long nblocks) { return p / det_red_chunk(npix, nblocks); }
// colsum / bn_bwd_reduce / train_losses / uv_loss: grid-stride in groups of `lanes` consecutive pixels
SFH_DET_FN long det_red_block_of_pixel_strided(long p, int lanes, long nblocks) { return (p / lanes) % nblocks; }
// pixel lanes of a 256-thread block over C channels (channel quads, at most 1024 channels per pass)
SFH_DET_FN int det_red_lanes(int C) { const int cq = (C < 1024 ? C : 1024) >> 2; return 256 / cq; }

// sfh_outconv_bwd: block b owns pixels [b * ppb, min(npix, (b + 1) * ppb)); slab = block; elements [nc][cin] then [nc]
SFH_DET_FN long det_outconv_ppb(long npix) {
  long ppb = (npix / 1024 + 255) / 256 * 256;
  return ppb < 1024 ? 1024 : ppb;
}
SFH_DET_FN long det_outconv_elems(int nc, int cin) { return (long)nc * cin + nc; }
SFH_DET_FN DetPlan det_outconv_plan(int cin, int nc, int batch, int H, int W) {
  if (batch <= 0 || H <= 0 || W <= 0) return det_refuse(DET_BAD_FRAME);
  if (cin % 4 != 0 || cin < 4 || cin > 256) return det_refuse(DET_BAD_CIN);
  if (nc < 1 || nc > 8) return det_refuse(DET_BAD_NC);
  const long npix = (long)batch * H * W, ppb = det_outconv_ppb(npix);
  return det_admit((npix + ppb - 1) / ppb, det_outconv_elems(nc, cin), sizeof(double));
}

// sfh_avgpool_linear_bwd: slab = frame; elements [nout][C] then [nout]
SFH_DET_FN long det_avgpool_elems(int nout, int C) { return (long)nout * C + nout; }
SFH_DET_FN DetPlan det_avgpool_plan(int batch, int C, int nout) {
  if (batch <= 0 || C <= 0 || nout <= 0 || nout > 256) return det_refuse(DET_BAD_ARG);
  return det_admit(batch, det_avgpool_elems(nout, C), sizeof(double));
}

// sfh_train_losses (3 loss words per slab, at most 2048 blocks of 256 pixels) and sfh_uv_loss (1, at most 1024): slab = block
SFH_DET_FN DetPlan det_losses_plan(int batch, int H, int W) {
  if (batch <= 0 || H <= 0 || W <= 0) return det_refuse(DET_BAD_ARG);
  const long nb = ((long)batch * H * W + 255) / 256;
  return det_admit(nb > 2048 ? 2048 : nb, 3, sizeof(double));
}
SFH_DET_FN DetPlan det_uv_plan(int batch, int C, int H, int W) {
  if (batch <= 0 || C <= 0 || H <= 0 || W <= 0) return det_refuse(DET_BAD_ARG);
  const long nb = ((long)batch * C * H * W + 255) / 256;
  return det_admit(nb > 1024 ? 1024 : nb, 1, sizeof(double));
}
// sfh_reproj_loss: one thread per frame, 64 frames per block; slab = block, one loss word
SFH_DET_FN DetPlan det_reproj_plan(int batch) {
  return batch <= 0 ? det_refuse(DET_BAD_ARG) : det_admit(det_cdiv(batch, 64), 1, sizeof(double));
}

// warp_bwd_theta_kernel: block (bx, by) covers 256 columns x 4 rows of every frame; slab = by * gx + bx, elements [batch][9]
SFH_DET_FN int det_warp_gx(int w) { return det_cdiv(w, 256); }
SFH_DET_FN int det_warp_gy(int h) { return det_cdiv(h, 4); }
SFH_DET_FN long det_warp_slab(int bx, int by, int gx) { return (long)by * gx + bx; }
SFH_DET_FN DetPlan det_warp_plan(int batch, int h, int w) {   // batch is gridDim.z
  if (batch <= 0 || batch > 65535 || h <= 1 || w <= 1) return det_refuse(DET_BAD_ARG);
  return det_admit((long)det_warp_gx(w) * det_warp_gy(h), 9L * batch, sizeof(double));
}

// refine_accumulate_kernel (csrc/refine.hip) and uvfit_accumulate_kernel (csrc/uvfit.hip): block (bx, by) covers 64 columns
// x 64 rows of every frame; slab = by * gx + bx, elements [batch][sums], fp64.  batch is gridDim.z: at most 65535.
#define DET_FIT_TILE 64
#define DET_REFINE_SUMS 45   // SFH_REFINE_SUMS
#define DET_UVFIT_SUMS 27    // SFH_UVFIT_SUMS
SFH_DET_FN DetPlan det_fit_tiles(int batch, int h, int w, int sums) {
  return det_admit((long)det_cdiv(w, DET_FIT_TILE) * det_cdiv(h, DET_FIT_TILE), (long)sums * batch, sizeof(double));
}
SFH_DET_FN DetPlan det_refine_plan(int batch, int h, int w) {   // h x w: the evidence grid of a level
  if (batch <= 0 || batch > 65535 || h < 1 || w < 1) return det_refuse(DET_BAD_ARG);
  return det_fit_tiles(batch, h, w, DET_REFINE_SUMS);
}
SFH_DET_FN DetPlan det_uvfit_plan(int batch, int h, int w) {    // by is gridDim.y: at most 65535 tile rows
  if (batch <= 0 || batch > 65535 || h < 2 || w < 2 || det_cdiv(h, DET_FIT_TILE) > 65535) return det_refuse(DET_BAD_ARG);
  return det_fit_tiles(batch, h, w, DET_UVFIT_SUMS);
}
// track_accumulate_kernel (csrc/track.hip): the same tiles over the current frame's plane of a level; `pairs` stands where
// the batch does (gridDim.z), a plane has at least 2 x 2 pixels
#define DET_TRACK_SUMS 46    // SFH_TRACK_SUMS
SFH_DET_FN DetPlan det_track_plan(int pairs, int h, int w) {
  if (pairs <= 0 || pairs > 65535 || h < 2 || w < 2 || det_cdiv(h, DET_FIT_TILE) > 65535) return det_refuse(DET_BAD_ARG);
  return det_fit_tiles(pairs, h, w, DET_TRACK_SUMS);
}

// ------------------------------------------------------------------ backward-filter, fp32 MFMA (csrc/train_wgrad.hip)
// 64-pixel tiles of th x tw (the shape with the fewest tiles; ties go to the widest), tile index = (b * nty + ty) * ntx + tx.
// Split s owns the tiles s, s + nsplit, s + 2 * nsplit, ...: slab of a tile = tile % nsplit.  Slab element of raw[m][tap][n]
// (n counted from the source's first channel): (m * kk + tap) * N + n - the slab is compact, the sum pass places it at
// column n_off of raw.
SFH_DET_FN int det_wgrad_tile_shape(int H, int W) {   // 0: 2x32, 1: 4x16, 2: 8x8
  const int th[3] = {2, 4, 8}, tw[3] = {32, 16, 8};
  int best = 0;
  long bc = -1;
  for (int i = 0; i < 3; ++i) {
    const long c = (long)det_cdiv(H, th[i]) * det_cdiv(W, tw[i]);
    if (bc < 0 || c < bc) { bc = c; best = i; }
  }
  return best;
}
SFH_DET_FN int det_tile_h(int shape) { return shape == 0 ? 2 : (shape == 1 ? 4 : 8); }
SFH_DET_FN int det_tile_w(int shape) { return shape == 0 ? 32 : (shape == 1 ? 16 : 8); }
// n columns of a workgroup (16 per sub-block)
SFH_DET_FN int det_wgrad_nsub(int ksize, int N) { return ksize == 3 ? (N <= 16 ? 1 : 4) : (ksize == 1 ? 4 : 2); }

struct DetWgradPlan : DetPlan {   // slabs = nsplit
  bool c4;
  int shape, ntx, nty, ntiles, mt, mn, nsplit, kk;
};
// sfh_conv_wgrad: x_cs the source's channel stride, xh x xw its size, placed at (pad_top, pad_left) of the H x W frame
SFH_DET_FN DetWgradPlan det_wgrad_plan(int M, int x_cs, int xh, int xw, int N, int pad_top, int pad_left, int batch, int H, int W,
                                       int ksize) {
  DetWgradPlan p = {};   // refused until the last line admits it
  if (!(batch > 0 && H > 0 && W > 0 && xh > 0 && xw > 0)) p.why = DET_BAD_FRAME;
  else if (!(M > 0 && M % 4 == 0)) p.why = DET_BAD_M;
  else if (!(N > 0 && N % 4 == 0 && x_cs % 4 == 0 && x_cs >= N)) p.why = DET_BAD_N;
  else if (!(pad_top >= 0 && pad_left >= 0 && pad_top + xh <= H && pad_left + xw <= W)) p.why = DET_BAD_FIT;
  else if (!(ksize == 1 || ksize == 3 || ksize == 4)) p.why = DET_BAD_KSIZE;
  else if (!(ksize != 4 || N <= 32)) p.why = DET_BAD_K4N;
  if (p.why != DET_OK) return p;
  // the first-layer form (wgrad_c4_kernel): 3x3 over at most four channels stored as four, one source of the frame's own size
  const bool c4 = p.c4 = ksize == 3 && N <= 4 && x_cs == 4 && xh == H && xw == W && pad_top == 0 && pad_left == 0;
  p.shape = det_wgrad_tile_shape(H, W);
  p.ntx = det_cdiv(W, det_tile_w(p.shape));
  p.nty = det_cdiv(H, det_tile_h(p.shape));
  p.ntiles = batch * p.ntx * p.nty;
  p.mt = det_cdiv(M, 64);
  p.mn = c4 ? p.mt : p.mt * det_cdiv(N, 16 * det_wgrad_nsub(ksize, N));
  int ns = det_cdiv(c4 ? 2048 : 1024, p.mn);   // c4: four workgroups per CU, two rounds of 1024
  if (ns > p.ntiles) ns = p.ntiles;
  if (ns < 1) ns = 1;
  if (!c4 && ns > 65535) ns = 65535;
  if (ns < 8 && p.ntiles >= 8) ns = 8;         // one split per XCD at least
  p.nsplit = ns;
  p.kk = ksize * ksize;
  static_cast<DetPlan&>(p) = det_admit(ns, (long)M * p.kk * N, sizeof(float));
  return p;
}
SFH_DET_FN int det_wgrad_slab_of_tile(int tile, int nsplit) { return tile % nsplit; }   // RESTATEMENT (host walk only)
// what the DET instantiations of wgrad_kernel, wgrad_c4_kernel and wgrad_s3_kernel store through
SFH_DET_FN long det_wgrad_elem(int m, int tap, int n, int kk, int N) { return ((long)m * kk + tap) * N + n; }

// ------------------------------------------------------------------ backward-filter, split operands (csrc/wgrad_s3.hip)
// Split s owns the contiguous tiles [s * tps, min(ntiles, (s + 1) * tps)): slab of a tile = tile / tps.  Elements as above.
SFH_DET_FN int det_wgrad_s3_tile_shape(int H, int W) {   // least padded area; ties: the widest
  const long c0 = (long)det_cdiv(H, 2) * det_cdiv(W, 32), c1 = (long)det_cdiv(H, 4) * det_cdiv(W, 16),
             c2 = (long)det_cdiv(H, 8) * det_cdiv(W, 8);
  if (c0 <= c1 && c0 <= c2) return 0;
  return c1 <= c2 ? 1 : 2;
}
struct DetWgradS3Plan : DetPlan {   // slabs = nsplit
  int shape, ntx, nty, ntiles, mn, nsplit, tps, kk;
  long nblocks;   // the grid: whole rounds of 8 splits
};
SFH_DET_FN DetWgradS3Plan det_wgrad_s3_plan(int M, int N, int batch, int H, int W, int ksize) {
  DetWgradS3Plan p = {};   // refused until the last line admits it
  if (!(ksize == 3 || ksize == 1)) p.why = DET_BAD_KSIZE;
  else if (!(batch > 0 && H > 0 && W > 0)) p.why = DET_BAD_FRAME;
  else if (!(M > 0 && M % 64 == 0)) p.why = DET_BAD_M;
  else if (!(N > 0 && N % 32 == 0)) p.why = DET_BAD_N;
  if (p.why != DET_OK) return p;
  p.shape = det_wgrad_s3_tile_shape(H, W);
  p.ntx = det_cdiv(W, det_tile_w(p.shape));
  p.nty = det_cdiv(H, det_tile_h(p.shape));
  p.ntiles = p.ntx * p.nty * batch;
  p.mn = (M / 64) * (N / 32);
  // about three rounds of two workgroups per CU - and a multiple of 8: split s runs on XCD s % 8
  int nsplit = ((1536 / p.mn + 7) / 8) * 8;
  // at least 16 tiles per split, as long as one round of workgroups (512) is still launched
  const int by_tiles = ((p.ntiles / 16 + 7) / 8) * 8, one_round = ((512 / p.mn + 7) / 8) * 8;
  if (nsplit > by_tiles) nsplit = by_tiles > one_round ? by_tiles : (one_round < nsplit ? one_round : nsplit);
  if (nsplit < 8) nsplit = 8;
  if (nsplit > p.ntiles) nsplit = p.ntiles;
  p.tps = det_cdiv(p.ntiles, nsplit);
  p.nsplit = det_cdiv(p.ntiles, p.tps);
  if (p.nsplit > 8 && p.nsplit % 8 != 0 && p.nsplit < 32) {   // e.g. 13 of 16: shave the tail to a multiple of 8
    const int want = (p.nsplit / 8) * 8;
    const int tps2 = det_cdiv(p.ntiles, want);
    if (det_cdiv(p.ntiles, tps2) % 8 == 0) { p.tps = tps2; p.nsplit = det_cdiv(p.ntiles, tps2); }
  }
  p.kk = ksize * ksize;
  p.nblocks = (long)det_cdiv(p.nsplit, 8) * 8 * p.mn;
  if (p.nblocks >= (1L << 31)) { p.why = DET_TOO_LARGE; return p; }
  static_cast<DetPlan&>(p) = det_admit(p.nsplit, (long)M * p.kk * N, sizeof(float));
  return p;
}
SFH_DET_FN int det_wgrad_s3_slab_of_tile(int tile, int tps) { return tile / tps; }   // RESTATEMENT (host walk only)

// ------------------------------------------------------------------ grouped backward-filter (csrc/conv_grouped.hip)
// One workgroup row (blockIdx.x) per tile of tile_h x 16 OUTPUT pixels; slab = tile; a slab is a whole raw (C, 9, cg), indexed
// by gc_raw_index (conv_grouped_core.h); the workgroups of one tile (blockIdx.y: 32 output channels x a 32-channel chunk)
// write disjoint parts of it.
// Also what sfh_conv_grouped_fwd admits: the same tiles, the same limits.
SFH_DET_FN DetPlan det_grouped_plan(int batch, int H, int W, int groups, int cg, int stride) {
  if (!gc_cg_ok(cg)) return det_refuse(DET_BAD_CG);
  if (!(stride == 1 || stride == 2)) return det_refuse(DET_BAD_STRIDE);
  if (!(batch > 0 && H > 0 && W > 0 && groups > 0)) return det_refuse(DET_BAD_FRAME);
  if (!((long)groups * cg <= 65536 && (long)batch * H * W < (1L << 31) / 16)) return det_refuse(DET_TOO_LARGE);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  return det_admit((long)batch * det_cdiv(Ho, stride == 1 ? 8 : 4) * det_cdiv(Wo, 16), (long)groups * cg * 9 * cg, sizeof(float));
}

#if defined(__HIPCC__)
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>
// the last add of an accumulating kernel: the default mode's atomic, or the store pass's plain store into the slab
template <bool DET, typename T>
__device__ __forceinline__ void det_add(T* p, T v) {
  if constexpr (DET) *p = v;
  else unsafeAtomicAdd(p, v);
}
// What the launchers share (host code; SFH_REQUIRE: common.h).  A workspace that is NULL or smaller than the plan's bytes is
// refused before anything is launched.
#define SFH_REQUIRE_WS(who, ws, ws_bytes, plan)                                                                         \
  SFH_REQUIRE((ws) != nullptr && (long long)(ws_bytes) >= det_bytes(plan), "%s: workspace of %lld bytes, %lld needed", \
              who, (ws) ? (long long)(ws_bytes) : 0LL, det_bytes(plan))
// kernel<DET> for a run-time det
#define SFH_LAUNCH_DET(kernel, det, grid, block, stream, ...)                                         \
  do {                                                                                                \
    if (!(det)) hipLaunchKernelGGL(kernel<false>, grid, block, 0, (hipStream_t)(stream), __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel<true>, grid, block, 0, (hipStream_t)(stream), __VA_ARGS__);         \
  } while (0)
#endif
