// conv_inc_fused.hip - the UNet's first DoubleConv (inc: frame -> 64 -> 64 channels at full resolution, unet/unet_parts.py:14-21)
// as ONE launch in "f16x3" arithmetic: the 64-channel intermediate (0.94 GB of H2 planes per batch of 16 at 640x360, written by
// conv3x3_c4h2_kernel and read straight back by conv_s3_kernel) lives in LDS only.
//
// Per workgroup (256 pixels x 64 couts, the 8 x 32 tile both two-launch kernels use, four waves):
//   * the FH2 frame halo of the tile's INTERMEDIATE halo ((8 + 2 + 2) x (32 + 2 + 2) pixels x 16 bytes) is staged once;
//   * producer, once per 32-channel half: the first conv for every pixel of the (8 + 2) x (32 + 2) intermediate halo, 22 pixel
//     groups of 16 spread over the waves - the MFMA sequence of conv_c4h2.hip (tap-packed K, two k-steps, three products,
//     smallest first) -, then that layer's epilogue (folded BatchNorm, ReLU, sfh_split4_h2) into LDS in the layout the
//     consumer's operand reads expect: [plane 2][group of 8 channels 4][pixel][16 bytes].  Halo pixels outside the frame are
//     stored as zeros: they are the second conv's zero padding, not a convolution of out-of-frame input;
//   * consumer: the stage body of conv_s3.hip (nine taps x eight pixel groups per wave, three products each) on that half, so
//     every output accumulates the same products in the same order as in the two launches, then the shared epilogue
//     (pooled second output, range word).
// The halves take turns in one stage buffer: 44 KB + 6.8 KB of frame halo per workgroup, three workgroups per CU.
//
// The intermediate's range / overflow words keep their values: every pixel of the flattened tile grid is the interior pixel of
// exactly one tile, as in conv3x3_c4h2_kernel's grid (the same tiles), and only interior pixels enter the maximum.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "conv_epilogue.h"
#include "split_mfma.h"

namespace {

struct IFCfg {   // geometry as S3Cfg<3, 1, 1, 16, 8, 32, 2> (conv_s3.hip) + the frame halo
  static constexpr int KS = 3, NP = 2, NWN = 2, NWM = 2, NT = 256, NTAP = 9;
  static constexpr int SH = 1, SW = 16, TH = 8, TW = 32;
  static constexpr int HH = TH + 2, HW = TW + 2, HPIX = HH * HW;       // intermediate halo
  static constexpr int HPIXP = (HPIX + 15) / 16 * 16;
  static constexpr int BUF = 4 * NP * HPIXP;                           // 16-byte slots of one 32-channel stage
  static constexpr int FH = HH + 2, FW = HW + 2, FPIX = FH * FW;       // frame halo; slot FPIX stays zero
  static constexpr int LDS_BYTES = (BUF + FPIX + 1) * 16;
  static constexpr int SUBX = TW / SW, NSUBT = (TH / SH) * SUBX, MT_M = NSUBT / NWM;
  static constexpr bool FLATROWS = true;
  static_assert((4 * HPIXP * 16) % 256 == 0, "plane stride must be a multiple of 256 bytes");
  static_assert(TW == 32 && (HH * 2) % 4 == 0 && 2 * HH <= 32 && HPIX + 32 - 2 * HH <= HPIXP, "the producer's pixel groups");
  static_assert(LDS_BYTES <= 53 * 1024, "three workgroups per CU");
};

struct IFProd {   // the first conv (the launch sfh_conv3x3_c4h2_fwd would make)
  const void* frame;
  const void* wpacked;
  const float* scale;
  const float* shift;
  unsigned* overflow;
  unsigned* range;
  int relu, exp_mid;
  unsigned frame_bytes;
};

struct IFGeom {
  int tiles_x, ntiles;
  int Ho, Wo, rows_total, rows_per_img;
  unsigned rows_magic;
};

__global__ __launch_bounds__(IFCfg::NT, 2) void conv_inc_fused_kernel(const sfh_conv_desc d, const IFProd pr, const IFGeom g) {
  using C = IFCfg;
  extern __shared__ __attribute__((aligned(16))) float smem_f[];
  u32x4* const lds = reinterpret_cast<u32x4*>(smem_f);   // the stage buffer
  u32x4* const fh = lds + C::BUF;                        // frame halo + the zero slot
  u32x2* const lds2 = reinterpret_cast<u32x2*>(smem_f);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv / C::NWN, wn = wv % C::NWN;
  const int lq = lane & 15, lg = lane >> 4;

  const int bid = (int)blockIdx.x;
  const SfhWg wg = sfh_wg_xcd_range_one(bid & 7, bid >> 3, g.ntiles, d.reverse_tiles);
  if (!wg.live) return;
  const int tile = wg.tile;
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  const int x0 = tx * C::TW, r0 = ty * C::TH;

  // ---- frame halo: rows r0 - 2 .. r0 + TH + 1, columns x0 - 2 .. x0 + TW + 1; out-of-frame slots read zeros
  {
    const __amdgpu_buffer_rsrc_t rsf =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(pr.frame), 0, (int)pr.frame_bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < (C::FPIX + C::NT - 1) / C::NT; ++i) {
      const int p = tid + C::NT * i;
      if (p < C::FPIX) {
        const int hy = p / C::FW, hx = p - hy * C::FW;
        const int r = r0 - 2 + hy, x = x0 - 2 + hx;
        unsigned off = kSfhOOB;
        if (r >= 0 && x >= 0 && x < d.W) {
          int b, y;
          sfh_row_split(g, r, b, y);
          if (b < d.batch && y < d.H) off = frame_pixel_offset(b, y, x, d.H, d.W);
        }
        fh[p] = __builtin_amdgcn_raw_buffer_load_b128(rsf, (int)off, 0, 0);
      }
    }
    if (tid == 0) fh[C::FPIX] = (u32x4){0u, 0u, 0u, 0u};
  }

  // ---- producer: couts [32 st, 32 st + 32) of the first conv for the whole intermediate halo -> the stage buffer
  // k = 32 * s + 8 * lg + j: taps (8s + 2lg, 8s + 2lg + 1), channel j & 3 (conv_c4h2.hip); step 1: tap 8 for lg == 0 only
  const int ta = 2 * lg, tb = 2 * lg + 1;
  const int oa = (ta / 3) * C::FW + ta % 3, ob = (tb / 3) * C::FW + tb % 3;
  constexpr int O8 = 2 * C::FW + 2;
  using P = SplitProducts<IFCfg::NP>;
  const float mid_scale = sfh_h2_pow2(pr.exp_mid);
  unsigned over_mid = 0u;
  auto produce = [&](int st) {
    // weights of this half: packed [k-step 2][plane 2][cout group 4][lane 64][8 x fp16]
    const u32x4* const wp = reinterpret_cast<const u32x4*>(pr.wpacked) + lane;
    u32x4 pw[2][2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) pw[s][p][ni] = wp[((s * 2 + p) * 4 + 2 * st + ni) * 64];
    // One pixel group per turn (two at once, i.e. four independent accumulators, cost 24 more registers than three workgroups
    // per CU leave).  A group is 16 pixels of ONE halo row, so that its row arithmetic (frame row, in-frame and interior
    // tests, LDS row offsets) is wave-uniform and stays on the scalar unit: the vector issue port is what this kernel runs
    // short of.  Columns 0 .. 31 of the ten halo rows are groups 0 .. 19; the two remaining columns of all rows make two more
    // (the last one four pixels; its idle lanes compute pixel 19 again and write zeros to the padding slots behind the halo).
    const u32x2* const fh2 = reinterpret_cast<const u32x2*>(fh);
    auto group = [&](const int hy, const int hx, const int pp, const bool real) {
      const int fb = hy * C::FW + hx;
      u32x4 x[2][2];   // [k-step][plane]
      {
        // 8-byte reads: each lands in the operand half it belongs to
        const u32x2 a0 = fh2[2 * (fb + oa)], a1 = fh2[2 * (fb + oa) + 1];
        const u32x2 b0 = fh2[2 * (fb + ob)], b1 = fh2[2 * (fb + ob) + 1];
        const int ci = lg == 0 ? fb + O8 : C::FPIX;
        const u32x2 c0 = fh2[2 * ci], c1 = fh2[2 * ci + 1];
        x[0][0] = (u32x4){a0[0], a0[1], b0[0], b0[1]};
        x[0][1] = (u32x4){a1[0], a1[1], b1[0], b1[1]};
        x[1][0] = (u32x4){c0[0], c0[1], 0u, 0u};
        x[1][1] = (u32x4){c1[0], c1[1], 0u, 0u};
      }
      f32x4 pa[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k3 = 0; k3 < P::N; ++k3)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) pa[ni] = split_mfma<IFCfg::NP>(pw[s][P::PW[k3]][ni], x[s][P::PX[k3]], pa[ni]);
      // the first conv's epilogue (as sfh_conv_epilogue's pass 1 for an H2 destination) into the stage buffer
      const int r = r0 - 1 + hy, xx = x0 - 1 + hx;
      int b, y;
      sfh_row_split(g, r, b, y);
      const bool in_frame = real && r >= 0 && b < d.batch && y < d.H && (unsigned)xx < (unsigned)d.W;
      const bool interior = real && hy >= 1 && hy <= C::TH && hx >= 1 && hx <= C::TW;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int co = 32 * st + ni * 16 + 4 * lg;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(pr.scale + co);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(pr.shift + co);
        f32x4 v = pa[ni];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] * sc[j] + sh[j];
        if (pr.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = sfh_relu(v[j]);
        }
        u32x2 pl[2];
        unsigned o = 0u;
        sfh_split4_h2(v, mid_scale, pl, o);
        o = (interior && in_frame) ? o : 0u;   // (as sfh_conv_epilogue: only pixels of the tensor enter the words)
        over_mid = o > over_mid ? o : over_mid;
        // channel 16 ni + 4 lg + j of the half: group 2 ni + (lg >> 1), the (lg & 1) half of its 16 bytes
        const int slot = (2 * ni + (lg >> 1)) * C::HPIXP + pp;
#pragma unroll
        for (int p = 0; p < 2; ++p)
          lds2[(slot + p * 4 * C::HPIXP) * 2 + (lg & 1)] = in_frame ? pl[p] : (u32x2){0u, 0u};
      }
    };
#pragma unroll 1
    for (int k = 0; k < (C::HH * 2) / 4; ++k) {
      const int gq = wv + 4 * k;                     // (wave-uniform)
      const int hy = gq >> 1, hx = (gq & 1) * 16 + lq;
      group(hy, hx, hy * C::HW + hx, true);
    }
    if (wv < 2) {
      const int idx = wv * 16 + lq;                  // pixel idx: halo row idx >> 1, column 32 + (idx & 1)
      const bool real = idx < 2 * C::HH;
      const int ic = real ? idx : 2 * C::HH - 1;
      const int hy = ic >> 1, hx = C::TW + (ic & 1);
      group(hy, hx, real ? hy * C::HW + hx : C::HPIX + idx - 2 * C::HH, real);
    }
  };

  // ---- consumer: conv_s3_kernel's single-buffer H2 stage body on the stage buffer
  constexpr int NP = C::NP;
  using WS = SplitWeights<NP>;
  constexpr unsigned WTAP = WS::TAP;
  constexpr unsigned wtotal = 2u * C::NTAP * WTAP;              // [stage 2][tap 9][plane 2][cout group 4][lane 64][8 x fp16]
  const __amdgpu_buffer_rsrc_t rsw =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.wpacked), 0, (int)wtotal, 0x00020000);
  const unsigned wvoff = lane * 16u + (unsigned)(2 * wn) * WS::GROUP;
  auto load_w = [&](u32x4 (&w)[NP][2], unsigned soff) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        w[p][ni] = __builtin_amdgcn_raw_buffer_load_b128(rsw, (int)(wvoff + ni * WS::GROUP), (int)(soff + p * WS::PLANE), 0);
  };
  const int pixbase0 = lg * C::HPIXP + ((wm * C::MT_M / C::SUBX) * C::SH + lq / C::SW) * C::HW + (lq % C::SW);
  static_assert(C::MT_M % C::SUBX == 0, "a wave's pixel groups must start on a tile-row boundary");

  f32x4 acc[2][C::MT_M];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < C::MT_M; ++mi) acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int WD = 2, XD = 2;   // weight ring / operand read-ahead of the H2 instances of conv_s3_kernel
  u32x4 wr[WD][NP][2];
  // tap t of stage ST lives in ring set (ST * NTAP + t) % WD; unlike conv_s3_kernel's, a stage does not request tap 0 of the
  // next one at its end - those sixteen registers would stay live across the producer, which is where the kernel peaks
  auto stage = [&](auto st_tag) {
    constexpr int ST = decltype(st_tag)::value;
    constexpr int R0 = (ST * C::NTAP) % WD;       // ring position of tap 0 in this stage
    constexpr int NSTEP = C::NTAP * C::MT_M;
    u32x4 xq[XD + 1][NP];
    auto ld_x = [&](int s, int buf) {
      const int t = s / C::MT_M, mi = s % C::MT_M;
      const int toff = (t / C::KS) * C::HW + (t % C::KS);
      const int moff = (mi / C::SUBX) * C::SH * C::HW + (mi % C::SUBX) * C::SW;
#pragma unroll
      for (int p = 0; p < NP; ++p) xq[buf][p] = lds[pixbase0 + (p * 4 * C::HPIXP + moff + toff)];
    };
#pragma unroll
    for (int i = 0; i < XD; ++i) ld_x(i, i);
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      const int t = s / C::MT_M, mi = s % C::MT_M;
      const int xb = s % (XD + 1);
      u32x4 (&wc)[NP][2] = wr[(R0 + t) % WD];
      u32x4 (&wnx)[NP][2] = wr[(R0 + t + WD - 1) % WD];
      if (s + XD < NSTEP) ld_x(s + XD, (s + XD) % (XD + 1));
      if (mi == 0 && t + 1 < C::NTAP) load_w(wnx, (unsigned)(ST * C::NTAP + t + 1) * WTAP);  // next tap: one tap of MFMAs ahead
#pragma unroll
      for (int k3 = 0; k3 < P::N; ++k3)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[ni][mi] = split_mfma<NP>(wc[P::PW[k3]][ni], xq[xb][P::PX[k3]], acc[ni][mi]);
      // as conv_s3_kernel: each step's memory instructions stay inside the step, the next operand reads right behind the
      // first MFMA
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, NP, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 5, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  __syncthreads();            // the frame halo is complete
  produce(0);
  load_w(wr[0], 0u);          // tap 0 of stage 0 lands under the barrier
  __syncthreads();
  stage(std::integral_constant<int, 0>{});
  __syncthreads();            // every wave is past its last operand read of half 0
  produce(1);
  load_w(wr[C::NTAP % WD], (unsigned)C::NTAP * WTAP);
  sfh_h2_report(over_mid, pr.overflow, pr.range);   // the intermediate's words (all lanes arrive here)
  __syncthreads();
  stage(std::integral_constant<int, 1>{});

  sfh_conv_epilogue<C, 2, C::MT_M, 2>(d, g, acc, 32 * wn, wm * C::MT_M, r0, x0, lq, lg, 0, (unsigned)(tile * C::NWM + wm));
}

}  // namespace

extern "C" int sfh_conv_inc_fused_fwd(const sfh_conv_desc* inc0, const sfh_conv_desc* inc3, void* stream_) {
  SFH_REQUIRE(inc0 && inc3, "conv_inc_fused_fwd: null descriptor");
  const sfh_conv_desc& a = *inc0;
  const sfh_conv_desc& d = *inc3;
  // the first conv: what sfh_conv3x3_c4h2_fwd takes, with 64 output channels and an H2 intermediate (dst itself is not used)
  SFH_REQUIRE(a.src0 && a.wpacked && a.scale && a.shift, "conv_inc_fused_fwd: first conv: null pointer");
  SFH_REQUIRE(!a.src1 && !a.pool0 && a.ksize == 3 && a.stride == 1 && a.h0 == a.H && a.w0 == a.W && !a.dst_pool &&
                  a.out_mode == SFH_OUT_NHWC && !a.residual && !a.head_w && !a.acc_init && !(a.ksplit > 1) && !a.stats_partial,
              "conv_inc_fused_fwd: first conv: needs one FH2 frame source (sfh_frame_to_h2), 3x3 stride 1, a plain output");
  SFH_REQUIRE(a.src_fmt == SFH_FMT_FH2 && a.dst_fmt == SFH_FMT_H2, "conv_inc_fused_fwd: first conv: src_fmt=%d dst_fmt=%d, expected "
              "the FH2 frame tensor and an H2 intermediate", a.src_fmt, a.dst_fmt);
  SFH_REQUIRE(a.c0 >= 1 && a.c0 <= 4 && a.cs0 == 4 && a.cout == 64, "conv_inc_fused_fwd: first conv: c0=%d cs0=%d cout=%d, expected "
              "1..4 channels stored as 4 and 64 output channels", a.c0, a.cs0, a.cout);
  if (!sfh_h2_exp_ok("conv_inc_fused_fwd: first conv", "h2_exp_dst", a.h2_exp_dst)) return SFH_E_ARG;
  // the second conv: a plain 64 -> 64 3x3 stride-1 H2 launch of sfh_conv_s3_fwd (src0 is not used: its source never exists)
  SFH_REQUIRE(d.wpacked && d.scale && d.shift && d.dst, "conv_inc_fused_fwd: second conv: null pointer");
  SFH_REQUIRE(d.src_fmt == SFH_FMT_H2 && d.dst_fmt == SFH_FMT_H2, "conv_inc_fused_fwd: second conv: src_fmt=%d dst_fmt=%d, expected H2",
              d.src_fmt, d.dst_fmt);
  SFH_REQUIRE(d.ksize == 3 && d.stride == 1 && d.c0 == 64 && d.cout == 64 && !d.src1 && !d.pool0 && d.out_mode == SFH_OUT_NHWC &&
                  !d.residual && !d.head_w && !d.acc_init && !(d.ksplit > 1) && !d.stats_partial && !d.shift_border,
              "conv_inc_fused_fwd: second conv: needs a plain 3x3 stride-1 conv, 64 -> 64 channels (optional pooled output)");
  SFH_REQUIRE(d.tile == SFH_TILE_8x32, "conv_inc_fused_fwd: tile=%d, the fused kernel has the 8 x 32 tile only", d.tile);
  SFH_REQUIRE(d.batch == a.batch && d.H == a.H && d.W == a.W && d.batch > 0 && d.H > 0 && d.W > 0,
              "conv_inc_fused_fwd: the two convs disagree on the frame (%d x %d x %d / %d x %d x %d)", a.batch, a.H, a.W, d.batch, d.H, d.W);
  SFH_REQUIRE(d.h2_exp_src == a.h2_exp_dst, "conv_inc_fused_fwd: the intermediate's exponent differs (%d written, %d read)",
              a.h2_exp_dst, d.h2_exp_src);
  if (!sfh_h2_exp_ok("conv_inc_fused_fwd: second conv", "h2_exp_dst", d.h2_exp_dst)) return SFH_E_ARG;
  SFH_REQUIRE(d.dst_cs >= 64 && d.dst_cs % 32 == 0 && (!d.dst_pool || (d.pool_cs >= 64 && d.pool_cs % 32 == 0)),
              "conv_inc_fused_fwd: dst_cs=%d / pool_cs=%d must be multiples of 32, at least 64", d.dst_cs, d.pool_cs);
  IFGeom g;
  SFH_REQUIRE(sfh_conv_grid(g, d.batch, d.H, d.W, 3, 1, true, true, IFCfg::TH, IFCfg::TW), "conv_inc_fused_fwd: too many rows");
  const unsigned long long fb = 16ULL * d.batch * d.H * d.W;
  const unsigned long long db = 4ULL * d.batch * d.H * d.W * d.dst_cs;
  SFH_REQUIRE(sfh_fits_descriptor(fb) && sfh_fits_descriptor(db), "conv_inc_fused_fwd: a tensor exceeds the 4 GiB descriptor range; split the batch");
  IFProd pr;
  pr.frame = a.src0;
  pr.wpacked = a.wpacked;
  pr.scale = a.scale;
  pr.shift = a.shift;
  pr.overflow = a.h2_overflow;
  pr.range = a.h2_range;
  pr.relu = a.relu;
  pr.exp_mid = a.h2_exp_dst;
  pr.frame_bytes = (unsigned)fb;
  const long nblocks = (long)sfh_cdiv(g.ntiles, 8) * 8;
  SFH_REQUIRE(nblocks < (1L << 31), "conv_inc_fused_fwd: grid too large");
  sfh_allow_big_lds(reinterpret_cast<const void*>(&conv_inc_fused_kernel));
  hipLaunchKernelGGL(conv_inc_fused_kernel, dim3((unsigned)nblocks), dim3(IFCfg::NT), IFCfg::LDS_BYTES, (hipStream_t)stream_, d, pr, g);
  return sfh_check_launch("conv_inc_fused_kernel");
}
