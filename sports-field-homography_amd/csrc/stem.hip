// stem.hip - the ResNetSTN stem (7x7, stride 2, padding 3, <= 16 input channels -> 64; models/resnet.py:172,
// 241-243 conv0 + bn1 + relu) on the bf16 matrix cores with the split-bf16 (bf16x6) arithmetic of conv_s3.hip.
//
// The generic kernels see this layer as a 4x4 conv over a space-to-depth copy of the input (K = 16 taps x
// 32 channels, a third of it padding; 0.55 ms per batch on the fp32 MFMA kernel, 1.6 ms on the generic
// split-bf16 one).  Here K is packed by tap: one v_mfma_f32_16x16x32_bf16 covers 4 taps x 8 channels (lane
// group k = lane/16 owns one tap), 13 k-steps for the 49 taps; the 8 channels of a pixel are one 16-byte
// LDS element per plane.  The input (fp32 NHWC, 8 stored channels = cat((logits, frame)) zero-padded) is
// split into its three bf16 planes while it is staged, so no converted copy and no space-to-depth pass exist.
// Workgroup = 8 x 32 output pixels x 64 couts (4 waves: 2 pixel halves x 2 cout halves), halo 21 x 69 input
// pixels = 70 KB of LDS, two workgroups per CU.  Epilogue: conv_epilogue.h (BatchNorm scale/shift, ReLU, fp32 NHWC).
//
// 9..16 input channels (cat((logits, frame)) at 6..8 classes, img+mask+uv) take the second instance below: one MFMA covers
// 2 taps x 16 channels, 25 k-steps, source of 12 or 16 stored channels.  Which lane group owns which tap and channel half,
// and where a packed weight lies, is stated once for both instances in stem_core.h.
#include "common.h"
#include "conv_epilogue.h"
#include "split_mfma.h"
#include "stem_core.h"

namespace {

struct StemCfg {  // what the shared epilogue needs to know about the tile
  static constexpr int KS = 7, SUBX = 2, SH = 1, SW = 16, TH = 8, TW = 32;
  static constexpr bool FLATROWS = false;
  static constexpr int HH = 2 * (TH - 1) + 7, HW = 2 * (TW - 1) + 7;  // 21 x 69 input pixels
  static constexpr int HPIX = HH * HW, HPIXP = (HPIX + 15) / 16 * 16;
  static constexpr int LDS_BYTES = 3 * HPIXP * 16;   // three planes; the two-plane instance uses two thirds of it
  static constexpr int NSTEP = 13;  // ceil(49 taps / 4 per MFMA)
};
static_assert(StemCfg::TH == st_tile_h(8) && StemCfg::TW == st_tile_w(8) && StemCfg::HW == st_halo_w(8) &&
              StemCfg::HPIXP == st_halo_padded(8) && StemCfg::NSTEP == st_nstep(8) && StemCfg::LDS_BYTES == st_lds_bytes(8, 3),
              "stem_core.h states this tile");

struct StemWideCfg {   // the 16-channel instance: 8 x 16 output pixels, one pixel group of 16 per tile row
  static constexpr int CH = 16;
  static constexpr int KS = 7, SUBX = 1, SH = 1, SW = 16, TH = st_tile_h(CH), TW = st_tile_w(CH);
  static constexpr bool FLATROWS = false;
  static constexpr int HW = st_halo_w(CH), HPIX = st_halo_pixels(CH);   // 21 x 37 input pixels
  static constexpr int NSTEP = st_nstep(CH);   // ceil(49 taps / 2 per MFMA) = 25
};

struct StemGeom {
  int Ho, Wo, rows_total, rows_per_img;
  unsigned rows_magic;
  int tiles_x, tiles_y, ntiles;
};

// NP = 3: the input is split into three bf16 planes, six products (bf16x6); NP = 2: two fp16 planes of v * 2^2, three
// products (f16x3: weights packed as planes of w * 2^wexp, the caller folds 2^-(wexp + 2) into `scale`)
template <int NP>
__global__ __launch_bounds__(256, 2) void stem7x7_kernel(const sfh_conv_desc d, const StemGeom g) {
  using C = StemCfg;
  extern __shared__ __attribute__((aligned(16))) float smem_f[];
  u32x4* const lds = reinterpret_cast<u32x4*>(smem_f);   // [3 planes][HPIXP] x 16 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv >> 1, wn = wv & 1;
  const int lq = lane & 15, lg = lane >> 4;
  const int tile = blockIdx.x;
  const int tpi = g.tiles_x * g.tiles_y;
  const int img = tile / tpi, tl = tile - img * tpi;
  const int ty = tl / g.tiles_x, tx = tl - ty * g.tiles_x;
  const int y0 = ty * C::TH, x0 = tx * C::TW;

  // ---- stage the input halo: fp32 (8 channels) -> three bf16 planes, zeros outside the frame
  const float* src = d.src0 + (long)img * d.H * d.W * 8;
  unsigned over = 0u;   // NP = 2: see sfh_split4_h2
  const float in_scale = sfh_h2_pow2(d.h2_exp_src);   // the planes carry x * 2^h2_exp_src (folded into `scale` by the caller)
  for (int p = tid; p < C::HPIX; p += 256) {
    const int hy = p / C::HW, hx = p - hy * C::HW;
    const int y = 2 * y0 - 3 + hy, x = 2 * x0 - 3 + hx;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < d.H && x >= 0 && x < d.W) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + ((long)y * d.W + x) * 8);
      const f32x4 b = *reinterpret_cast<const f32x4*>(src + ((long)y * d.W + x) * 8 + 4);
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    }
    if constexpr (NP == 3) {
      u32x4 pl[3];
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = v[j];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const unsigned w = sfh_cvt_pk(r[2 * h], r[2 * h + 1]);
          pl[q][h] = w;
          r[2 * h] -= __builtin_bit_cast(float, w << 16);
          r[2 * h + 1] -= __builtin_bit_cast(float, w & 0xFFFF0000u);
        }
        lds[q * C::HPIXP + p] = pl[q];
      }
    } else {
      u32x2 pa[2], pb[2];
      sfh_split4_h2((f32x4){v[0], v[1], v[2], v[3]}, in_scale, pa, over);
      sfh_split4_h2((f32x4){v[4], v[5], v[6], v[7]}, in_scale, pb, over);
      lds[p] = (u32x4){pa[0][0], pa[0][1], pb[0][0], pb[0][1]};
      lds[C::HPIXP + p] = (u32x4){pa[1][0], pa[1][1], pb[1][0], pb[1][1]};
    }
  }
  if constexpr (NP == 2) {
    sfh_h2_report(over, d.h2_overflow, d.h2_range);   // (all lanes are back from the staging loop)
  }

  // ---- weights: packed [step 13][plane NP][cout subtile 4][lane 64] x 16 B; this wave: subtiles 2*wn, 2*wn+1
  const u32x4* wp = reinterpret_cast<const u32x4*>(d.wpacked) + (2 * wn) * 64 + lane;
  auto load_w = [&](u32x4 (&w)[NP][2], int s) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) w[p][ni] = wp[((s * NP + p) * 4 + ni) * 64];
  };
  u32x4 wa[NP][2], wb[NP][2];
  load_w(wa, 0);

  f32x4 acc[2][8];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  // lane's pixel in pixel group mi of this wave: row wm*4 + mi/2, col 16*(mi%2) + lq; halo pixel of tap
  // (ky,kx): (2*row + ky) * HW + 2*col + kx.  The tap of a lane is 4*s + lg.
  const int pix0 = (2 * (wm * 4)) * C::HW + 2 * lq;
  using P = SplitProducts<NP>;
#pragma unroll
  for (int s = 0; s < C::NSTEP; ++s) {
    u32x4 (&wc)[NP][2] = (s & 1) ? wb : wa;
    u32x4 (&wn_)[NP][2] = (s & 1) ? wa : wb;
    if (s + 1 < C::NSTEP) load_w(wn_, s + 1);
    const int toff = st_tap_off(8, st_tap(8, s, lg));   // padding taps carry zero weights: any valid address will do
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      const int moff = (2 * (mi >> 1)) * C::HW + 32 * (mi & 1);
      u32x4 xq[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) xq[p] = lds[p * C::HPIXP + pix0 + moff + toff];
#pragma unroll
      for (int k6 = 0; k6 < P::N; ++k6)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[ni][mi] = split_mfma<NP>(wc[P::PW[k6]][ni], xq[P::PX[k6]], acc[ni][mi]);
    }
  }
  sfh_conv_epilogue<C, 2, 8>(d, g, acc, 32 * wn, wm * 8, (img << 16) | y0, x0, lq, lg);
}

// The 16-channel instance: source fp32 NHWC with d.cs0 = 12 or 16 stored channels.  Workgroup = 8 x 16 output pixels x 64
// couts (4 waves: 2 row halves x 2 cout halves), halo 21 x 37 input pixels; a pixel is two 16-byte LDS elements per plane
// (channels 0..7 and 8..15), planes laid out [plane][half][pixel] so that a lane group's read is the 8-channel instance's.
// LDS 75,264 B (NP = 3) / 50,176 B (NP = 2): two / three workgroups per CU - the 8 x 32 tile would need 139,776 B with three
// planes, ONE workgroup per CU, whose staging (global loads, plane split) then runs with the matrix cores idle: within a
// workgroup a barrier separates staging from the k-loop, only a co-resident workgroup overlaps them.
template <int NP>
__global__ __launch_bounds__(256, 2) void stem7x7_wide_kernel(const sfh_conv_desc d, const StemGeom g) {
  using C = StemWideCfg;
  extern __shared__ __attribute__((aligned(16))) float smem_f[];
  u32x4* const lds = reinterpret_cast<u32x4*>(smem_f);   // st_lds_elem: [NP planes][2 halves][HPIXP] x 16 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv >> 1, wn = wv & 1;
  const int lq = lane & 15, lg = lane >> 4;
  const int tile = blockIdx.x;
  const int tpi = g.tiles_x * g.tiles_y;
  const int img = tile / tpi, tl = tile - img * tpi;
  const int ty = tl / g.tiles_x, tx = tl - ty * g.tiles_x;
  const int y0 = ty * C::TH, x0 = tx * C::TW;

  // ---- stage the input halo, one (channel half, pixel) per thread and round: fp32 -> NP planes, zeros outside the frame and
  // in channels >= cs0 (cs0 = 12: the second half holds four stored channels)
  const int cs = d.cs0;
  const float* src = d.src0 + (long)img * d.H * d.W * cs;
  unsigned over = 0u;   // NP = 2: see sfh_split4_h2
  const float in_scale = sfh_h2_pow2(d.h2_exp_src);
  for (int u = tid; u < 2 * C::HPIX; u += 256) {
    const int hf = u >= C::HPIX ? 1 : 0, p = u - hf * C::HPIX;
    const int hy = p / C::HW, hx = p - hy * C::HW;
    const int y = 2 * y0 - 3 + hy, x = 2 * x0 - 3 + hx;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < d.H && x >= 0 && x < d.W) {
      const float* px = src + ((long)y * d.W + x) * cs + 8 * hf;
      a = *reinterpret_cast<const f32x4*>(px);
      if (8 * hf + 8 <= cs) b = *reinterpret_cast<const f32x4*>(px + 4);
    }
    if constexpr (NP == 3) {
      float r[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        u32x4 pl;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const unsigned w = sfh_cvt_pk(r[2 * h], r[2 * h + 1]);
          pl[h] = w;
          r[2 * h] -= __builtin_bit_cast(float, w << 16);
          r[2 * h + 1] -= __builtin_bit_cast(float, w & 0xFFFF0000u);
        }
        lds[st_lds_elem(C::CH, q, hf, p)] = pl;
      }
    } else {
      u32x2 pa[2], pb[2];
      sfh_split4_h2(a, in_scale, pa, over);
      sfh_split4_h2(b, in_scale, pb, over);
      lds[st_lds_elem(C::CH, 0, hf, p)] = (u32x4){pa[0][0], pa[0][1], pb[0][0], pb[0][1]};
      lds[st_lds_elem(C::CH, 1, hf, p)] = (u32x4){pa[1][0], pa[1][1], pb[1][0], pb[1][1]};
    }
  }
  if constexpr (NP == 2) {
    sfh_h2_report(over, d.h2_overflow, d.h2_range);   // (all lanes are back from the staging loop)
  }

  // ---- weights: packed [step 25][plane NP][cout subtile 4][lane 64] x 16 B; this wave: subtiles 2*wn, 2*wn+1
  const u32x4* wp = reinterpret_cast<const u32x4*>(d.wpacked) + (2 * wn) * 64 + lane;
  auto load_w = [&](u32x4 (&w)[NP][2], int s) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) w[p][ni] = wp[((s * NP + p) * 4 + ni) * 64];
  };
  u32x4 wa[NP][2], wb[NP][2];
  load_w(wa, 0);

  f32x4 acc[2][4];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  // lane's pixel in pixel group mi of this wave: tile row wm*4 + mi, column lq; its channel half: st_chan0 / 8
  const int hf = st_chan0(C::CH, lg) >> 3;
  const int pix0 = st_pixel_off(C::CH, wm * 4, lq);
  using P = SplitProducts<NP>;
#pragma unroll
  for (int s = 0; s < C::NSTEP; ++s) {
    u32x4 (&wc)[NP][2] = (s & 1) ? wb : wa;
    u32x4 (&wn_)[NP][2] = (s & 1) ? wa : wb;
    if (s + 1 < C::NSTEP) load_w(wn_, s + 1);
    const int toff = st_tap_off(C::CH, st_tap(C::CH, s, lg));   // padding taps carry zero weights: any valid address will do
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      u32x4 xq[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) xq[p] = lds[st_lds_elem(C::CH, p, hf, pix0 + st_pixel_off(C::CH, mi, 0) + toff)];
#pragma unroll
      for (int k6 = 0; k6 < P::N; ++k6)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[ni][mi] = split_mfma<NP>(wc[P::PW[k6]][ni], xq[P::PX[k6]], acc[ni][mi]);
    }
  }
  sfh_conv_epilogue<C, 2, 4>(d, g, acc, 32 * wn, wm * 4, (img << 16) | y0, x0, lq, lg);
}

// packed[s][plane][subtile][lane][j] (st_packed_index): cout = subtile*16 + (lane & 15); tap and first channel of lane group
// lane >> 4 by st_tap / st_chan0 (CH = 8: tap 4*s + (lane >> 4), channel j)
template <int NP, int CH>
__global__ void pack_stem_weights_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed, int cin,
                                         int total, float wscale) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // one (s, subtile, lane)
  if (idx >= total) return;
  const int lane = idx & 63, sub = (idx >> 6) & 3, s = idx >> 8;
  const int co = sub * 16 + (lane & 15), t = st_tap(CH, s, lane >> 4), c0 = st_chan0(CH, lane >> 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = (t < ST_TAPS && c0 + j < cin) ? w[((long)co * cin + c0 + j) * ST_TAPS + t] : 0.f;
    if constexpr (NP == 3) {
      const __bf16 v0 = (__bf16)v;
      const float r1 = v - (float)v0;
      const __bf16 v1 = (__bf16)r1;
      const __bf16 v2 = (__bf16)(r1 - (float)v1);
      packed[st_packed_index(NP, s, 0, sub, lane, j)] = __builtin_bit_cast(unsigned short, v0);
      packed[st_packed_index(NP, s, 1, sub, lane, j)] = __builtin_bit_cast(unsigned short, v1);
      packed[st_packed_index(NP, s, 2, sub, lane, j)] = __builtin_bit_cast(unsigned short, v2);
    } else {
      const float u = fminf(fmaxf(v * wscale, -65504.f), 65504.f);
      const _Float16 h0 = (_Float16)u;
      const _Float16 h1 = (_Float16)(u - (float)h0);
      packed[st_packed_index(NP, s, 0, sub, lane, j)] = __builtin_bit_cast(unsigned short, h0);
      packed[st_packed_index(NP, s, 1, sub, lane, j)] = __builtin_bit_cast(unsigned short, h1);
    }
  }
}

}  // namespace

extern "C" int64_t sfh_packed_stem_weight_bytes(void) { return st_packed_elems(8, 3) * 2; }
extern "C" int64_t sfh_packed_stem16_weight_bytes(void) { return st_packed_elems(16, 3) * 2; }

template <int CH>
static int pack_stem_weights(const float* w, void* packed, int cin, int fmt, int wexp, void* stream) {
  SFH_REQUIRE(w && packed && cin >= 1 && cin <= CH, "pack_stem_weights: 1..%d input channels", CH);
  SFH_REQUIRE(fmt == SFH_FMT_S3 || (fmt == SFH_FMT_H2 && wexp >= -100 && wexp <= 100), "pack_stem_weights: fmt=%d wexp=%d", fmt, wexp);
  const int total = st_nstep(CH) * 4 * 64;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (fmt == SFH_FMT_H2)
    hipLaunchKernelGGL((pack_stem_weights_kernel<2, CH>), grid, dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)packed, cin,
                       total, ldexpf(1.f, wexp));
  else
    hipLaunchKernelGGL((pack_stem_weights_kernel<3, CH>), grid, dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)packed, cin,
                       total, 1.f);
  return sfh_check_launch("pack_stem_weights_kernel");
}

extern "C" int sfh_pack_stem_weights(const float* w, void* packed, int cin, int fmt, int wexp, void* stream) {
  return pack_stem_weights<8>(w, packed, cin, fmt, wexp, stream);
}
extern "C" int sfh_pack_stem16_weights(const float* w, void* packed, int cin, int fmt, int wexp, void* stream) {
  return pack_stem_weights<16>(w, packed, cin, fmt, wexp, stream);
}

extern "C" int sfh_stem7x7_fwd(const sfh_conv_desc* dp, void* stream) {
  SFH_REQUIRE(dp, "stem7x7_fwd: null descriptor");
  const sfh_conv_desc& d = *dp;
  SFH_REQUIRE(d.src0 && d.wpacked && d.scale && d.shift && d.dst, "stem7x7_fwd: null pointer");
  SFH_REQUIRE((st_cs_ok(8, d.cs0) || st_cs_ok(16, d.cs0)) && d.c0 >= 1 && d.c0 <= d.cs0 && d.src_fmt == SFH_FMT_F32,
              "stem7x7_fwd: fp32 NHWC source with 8, 12 or 16 stored channels (cs0=%d c0=%d)", d.cs0, d.c0);
  const bool wide = st_cs_ok(16, d.cs0);    // the 16-channel instance (weights from sfh_pack_stem16_weights)
  SFH_REQUIRE(d.cout == 64 && d.dst_cs >= 64 && d.dst_fmt == SFH_FMT_F32 && d.out_mode == SFH_OUT_NHWC && !d.residual &&
                  !d.dst_pool && !d.src1, "stem7x7_fwd: 64 output channels, plain fp32 NHWC destination");
  SFH_REQUIRE(d.batch > 0 && d.batch < 32768 && d.H > 0 && d.W > 0 && d.h0 == d.H && d.w0 == d.W, "stem7x7_fwd: bad geometry");
  StemGeom g;
  SFH_REQUIRE(sfh_conv_grid(g, d.batch, d.H, d.W, 7, 2, false, false, wide ? StemWideCfg::TH : StemCfg::TH, wide ? StemWideCfg::TW : StemCfg::TW),
              "stem7x7_fwd: frame too tall or too many tiles");
  SFH_REQUIRE(sfh_fits_descriptor((unsigned long long)d.batch * g.Ho * g.Wo * d.dst_cs * 4ULL), "stem7x7_fwd: destination exceeds 4 GiB");
  SFH_REQUIRE(d.split_arith == 0 || d.split_arith == SFH_FMT_S3 || d.split_arith == SFH_FMT_H2, "stem7x7_fwd: split_arith=%d", d.split_arith);
  if (!sfh_h2_exp_ok("stem7x7_fwd", "h2_exp_src", d.h2_exp_src)) return SFH_E_ARG;
  if (wide) {
    if (d.split_arith == SFH_FMT_H2) {
      hipLaunchKernelGGL(stem7x7_wide_kernel<2>, dim3((unsigned)g.ntiles), dim3(256), st_lds_bytes(16, 2), (hipStream_t)stream, d, g);
    } else {
      sfh_allow_big_lds(reinterpret_cast<const void*>(&stem7x7_wide_kernel<3>));
      hipLaunchKernelGGL(stem7x7_wide_kernel<3>, dim3((unsigned)g.ntiles), dim3(256), st_lds_bytes(16, 3), (hipStream_t)stream, d, g);
    }
    return sfh_check_launch("stem7x7_wide_kernel");
  }
  if (d.split_arith == SFH_FMT_H2) {
    sfh_allow_big_lds(reinterpret_cast<const void*>(&stem7x7_kernel<2>));
    hipLaunchKernelGGL(stem7x7_kernel<2>, dim3((unsigned)g.ntiles), dim3(256), StemCfg::LDS_BYTES / 3 * 2, (hipStream_t)stream, d, g);
  } else {
    sfh_allow_big_lds(reinterpret_cast<const void*>(&stem7x7_kernel<3>));
    hipLaunchKernelGGL(stem7x7_kernel<3>, dim3((unsigned)g.ntiles), dim3(256), StemCfg::LDS_BYTES, (hipStream_t)stream, d, g);
  }
  return sfh_check_launch("stem7x7_kernel");
}
