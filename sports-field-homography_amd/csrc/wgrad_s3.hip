// wgrad_s3.hip - backward-filter (weight gradient) of stride-1 3x3 and 1x1 convolutions on the 16-bit matrix cores.
//
//   raw[m][tap][n_off + n] += sum_{b,y,x} dz[b][y][x][m] * xin[b][y + ky - 1][x + kx - 1][n]        (1x1: one tap, no shift)
//
// Same "bf16x6" arithmetic as the forward kernel (conv_s3.hip): both operands are exact three-plane bf16
// splits of fp32 values (S3 tensors), every product is accumulated from its six partial products >= 2^-16
// in fp32 by v_mfma_f32_16x16x32_bf16.  GEMM view: M = cout (A operand, from dz), N = cin (B operand, from
// the layer input), K = pixels.
//
// The S3 layout keeps 8 channels of one pixel in 16 bytes, i.e. it is K-strided for this product.  gfx950's
// transposing LDS read (ds_read_b64_tr_b16: a 4-row x 16-column block of 16-bit elements delivered
// column-major) turns it into MFMA fragments for free: "rows" are four pixels of a k-step, "columns" the 16
// channels of the fragment, and every lane supplies the address of its own row piece, so the tap shift of
// the input window is just another immediate offset.
//
// Workgroup (4 waves) = 64 couts x 32 cins x 9 taps, looped over a contiguous range of 64-pixel tiles
// (split-K over workgroups, fp32 atomics at the end).  Per tile the dz pixels and the input halo go
// global -> LDS by LDS-DMA in the S3 chunk order ([plane][8-channel group][pixel][16 B]; group stride = 4 mod
// 16 chunks, which makes the transposed reads of a 32-lane half conflict-free); one LDS buffer, two
// workgroups per CU, so that the DMA of one hides under the MFMAs of the other.  Wave w: cin half w&1
// (16 cins), cout half w>>1 (32 couts): 18 accumulator tiles, per 32-pixel k-step 66 transposed reads
// against 108 MFMAs.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "common.h"
#include "det_core.h"   // the split plan and det_add: the deterministic mode's slabs
#include "split_mfma.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

struct WgS3Args {
  const void* dz; int M;               // dz S3 (B, H, M/32, 3, 4, W, 8)
  const void* x; int xc, xh, xw;       // input S3 (B, xh, xc/32, 3, 4, xw, 8)
  int N, pad_top, pad_left;            // N channels used (from channel 0), tensor placed at (pad_top, pad_left)
  int batch, H, W;
  float* raw; int raw_n, n_off;
  int ntx, nty, ntiles, nsplit, tps, mblk, nblk;
  unsigned bytes_dz, bytes_x;
};

__device__ __forceinline__ bf16x8 frag(s16x4 lo, s16x4 hi) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// NP = planes per operand: 3 = S3 tensors (bf16, six products), 2 = H2 tensors (fp16 planes of v * 2^SFH_H2_ACT_EXP,
// three products; the accumulators are multiplied by 2^-(2 * SFH_H2_ACT_EXP) before they are added to raw)
// KS = 3: nine taps; KS = 1: one tap (ConvTranspose2d as a 1x1 conv over space_to_depth2(dY), Bottleneck 1x1s) - the same
// tile loop with 12 instead of 108 MFMAs per wave and tile, i.e. bound by the LDS-DMA of the two operands, which is still
// several times the rate of the fp32 kernel these layers ran on
// DET: the store pass of the deterministic mode (det_core.h): a.raw is the workspace, split s stores its sums (an empty
// split: zeros) into slab s, element det_wgrad_elem(m, tap, n); DET = false is the kernel as it was
template <int TR, int TW, int NP, int KS = 3, bool DET = false>
__global__ __launch_bounds__(256, NP == 2 ? 3 : 2) void wgrad_s3_kernel(const WgS3Args a) {
  static_assert(TR * TW == 64 && (TW == 8 || TW == 16 || TW == 32), "64-pixel tiles, two 32-pixel k-steps");
  static_assert(KS == 3 || KS == 1, "3x3 or 1x1");
  constexpr int NTAP = KS * KS, PADK = KS / 2;
  constexpr int R4 = 4 * NP;                                         // (plane, group) runs per 32-channel block
  constexpr int HWD = TW + KS - 1, HR = TR + KS - 1, HP = HR * HWD; // input halo of a tile
  constexpr int PX = ((HP - 4 + 15) / 16) * 16 + 4;                 // chunks per (plane, group) of the halo image
  constexpr int PD = 68;                                            // ... of the dz image (64 pixels)
  constexpr int XCH = R4 * PX;
  constexpr int NXI = (HP + 63) / 64;                               // DMA instructions per (plane, group) of the halo
  constexpr int RS = 32 / TW;                                       // tile rows per k-step
  extern __shared__ __attribute__((aligned(16))) u32x4 lds[];       // [halo image 12 * PX][dz image 24 * PD] chunks

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int nb16 = wv & 1, mh = wv >> 1;

  // blocks of one pixel split run back to back on ONE XCD (workgroups go round-robin to the 8 XCDs): the
  // split's dz / input tiles are fetched into that L2 once, not once per (m, n) block
  const int mn = a.mblk * a.nblk;
  const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
  const int split = (kq / mn) * 8 + xcd, mni = kq % mn;
  if (split >= a.nsplit) return;
  const int mb64 = mni / a.nblk, nb32 = mni % a.nblk;

  const __amdgpu_buffer_rsrc_t rdz = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dz), 0, (int)a.bytes_dz, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.bytes_x, 0x00020000);
  const int MB = a.M >> 5, CBX = a.xc >> 5;

  // transposed-read byte bases of this lane (k index inside a step: 8g + 4h + q; h and the k-step are immediates)
  const int kk0 = 8 * g + q;
  const unsigned dzb = (unsigned)(((4 * mh + (pp >> 1)) * PD + kk0) * 16 + (pp & 1) * 8 + XCH * 16);
  const unsigned xb = (unsigned)(((2 * nb16 + (pp >> 1)) * PX + (kk0 / TW) * HWD + (kk0 % TW)) * 16 + (pp & 1) * 8);

  f32x4 acc[2][NTAP];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int t = 0; t < NTAP; ++t) acc[mb][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  typedef __attribute__((address_space(3))) char* lds_char_ptr;
  const lds_char_ptr ldsc = (lds_char_ptr)(lds_ptr_t)lds;
  auto tr = [&](unsigned byte_off) -> s16x4 {   // EXEC is all ones here (no divergent control flow around the reads)
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(ldsc + byte_off));
  };

  const int t_begin = split * a.tps;
  const int t_end = (t_begin + a.tps < a.ntiles) ? t_begin + a.tps : a.ntiles;
  for (int t = t_begin; t < t_end; ++t) {
    const int tx = t % a.ntx, r1 = t / a.ntx;
    const int ty = r1 % a.nty, b = r1 / a.nty;
    const int y0 = ty * TR, x0 = tx * TW;
    // ---- LDS-DMA: 12 (plane, group) runs of the input halo, 24 of dz; wave w takes 3 and 6 of them
    {
      unsigned voff[NXI];
      bool act[NXI];
#pragma unroll
      for (int i = 0; i < NXI; ++i) {
        const int hp = i * 64 + lane;
        const int r = hp / HWD, c = hp - r * HWD;
        const int yy = y0 - PADK + r - a.pad_top, xx = x0 - PADK + c - a.pad_left;
        const bool ok = (unsigned)yy < (unsigned)a.xh && (unsigned)xx < (unsigned)a.xw;
        voff[i] = ok ? (unsigned)((yy * CBX * R4 * a.xw + xx) * 16) : kSfhOOB;
        act[i] = hp < HP;
      }
      const unsigned xsb = (unsigned)((b * a.xh * CBX + nb32) * R4) * (unsigned)a.xw * 16u;
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int pg = wv * NP + j;                      // plane * 4 + group
        const unsigned soff = xsb + (unsigned)pg * (unsigned)a.xw * 16u;
#pragma unroll
        for (int i = 0; i < NXI; ++i) {
          if (act[i])
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)(lds + pg * PX + i * 64), 16, (int)voff[i], (int)soff, 0, 0);
        }
      }
      const int py = lane / TW, px = lane - py * TW;
      const int y = y0 + py, x = x0 + px;
      const unsigned dvoff = (y < a.H && x < a.W) ? (unsigned)((y * MB * R4 * a.W + x) * 16) : kSfhOOB;
      const unsigned dsb = (unsigned)((b * a.H * MB + mb64 * 2) * R4) * (unsigned)a.W * 16u;
#pragma unroll
      for (int j = 0; j < 2 * NP; ++j) {
        const int pg8 = wv * (2 * NP) + j;               // plane * 8 + group of the 64 couts
        const int p = pg8 >> 3, g8 = pg8 & 7;
        const unsigned soff = dsb + (unsigned)(((g8 >> 2) * R4 + p * 4 + (g8 & 3))) * (unsigned)a.W * 16u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rdz, (lds_ptr_t)(lds + XCH + pg8 * PD), 16, (int)dvoff, (int)soff, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- two k-steps of 32 pixels
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[2][NP];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const unsigned ad = dzb + (unsigned)(((p * 8 + 2 * mb) * PD + 32 * s) * 16);
          af[mb][p] = frag(tr(ad), tr(ad + 64));
        }
#pragma unroll
      for (int t9 = 0; t9 < NTAP; ++t9) {
        const int ky = t9 / KS, kx = t9 % KS;
        bf16x8 bfr[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const unsigned ad = xb + (unsigned)(((p * 4) * PX + (s * RS + ky) * HWD + kx) * 16);
          bfr[p] = frag(tr(ad), tr(ad + 64));
        }
        using P = SplitProducts<NP>;   // dz takes the weights' place (first operand), x the activations'
#pragma unroll
        for (int k6 = 0; k6 < P::N; ++k6)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) acc[mb][t9] = split_mfma<NP>(af[mb][P::PW[k6]], bfr[P::PX[k6]], acc[mb][t9]);
      }
    }
    __syncthreads();   // every wave is done with the buffer before the next tile's DMA lands in it
  }

  // ---- split-K: add this workgroup's partial sums
  const int m0 = mb64 * 64 + 32 * mh + 4 * g;
  const int n = a.n_off + nb32 * 32 + 16 * nb16 + (lane & 15);
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int t9 = 0; t9 < NTAP; ++t9)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if constexpr (DET)
          a.raw[det_slab_offset(split, (long)a.M * NTAP * a.N) + det_wgrad_elem(m0 + 16 * mb + r, t9, n - a.n_off, NTAP, a.N)] =
              NP == 2 ? acc[mb][t9][r] * (1.f / (float)(1 << (2 * SFH_H2_ACT_EXP))) : acc[mb][t9][r];
        else
          unsafeAtomicAdd(a.raw + ((long)(m0 + 16 * mb + r) * NTAP + t9) * a.raw_n + n,
                          NP == 2 ? acc[mb][t9][r] * (1.f / (float)(1 << (2 * SFH_H2_ACT_EXP))) : acc[mb][t9][r]);
}

// p: the split plan (det_core.h, det_wgrad_s3_plan - the split count is a multiple of 8 where it can be, split s runs on XCD
// s % 8: 22x40 layers with 3 splits ran on 3 of the 8 XCDs, 103 instead of 250 TFLOP/s-equivalent; and at least 16 tiles per
// split, every split ends with 64 x 32 x 9 fp32 adds per workgroup: ResNet layer1, 90x160, 768 splits of 5 tiles = 28 M atomics
// for 17 GFLOP, 138 us).  ws == nullptr: the default mode, atomics onto raw; else the store pass into ws and the sum pass.
template <int TR, int TW, int NP, int KS = 3>
int launch(WgS3Args a, const DetWgradS3Plan& p, float* ws, hipStream_t stream) {
  constexpr int HP = (TR + KS - 1) * (TW + KS - 1);
  constexpr int PX = ((HP - 4 + 15) / 16) * 16 + 4;
  constexpr int LDS_BYTES = (4 * NP * PX + 8 * NP * 68) * 16;
  a.ntx = p.ntx;
  a.nty = p.nty;
  a.ntiles = p.ntiles;
  a.tps = p.tps;
  a.nsplit = p.nsplit;
  float* raw = a.raw;
  if (!ws) {
    sfh_allow_big_lds(reinterpret_cast<const void*>(&wgrad_s3_kernel<TR, TW, NP, KS>));
    hipLaunchKernelGGL((wgrad_s3_kernel<TR, TW, NP, KS>), dim3((unsigned)p.nblocks), dim3(256), LDS_BYTES, stream, a);
  } else {
    a.raw = ws;
    sfh_allow_big_lds(reinterpret_cast<const void*>(&wgrad_s3_kernel<TR, TW, NP, KS, true>));
    hipLaunchKernelGGL((wgrad_s3_kernel<TR, TW, NP, KS, true>), dim3((unsigned)p.nblocks), dim3(256), LDS_BYTES, stream, a);
  }
  if (int rc = sfh_check_launch(ws ? "wgrad_s3_kernel (deterministic)" : "wgrad_s3_kernel")) return rc;
  return ws ? sfh_det_reduce_f32(ws, p.slabs, p.elems, p.elems, a.N, raw + a.n_off, a.raw_n, stream) : SFH_OK;
}

}  // namespace

static int conv_wgrad_s3_impl(const void* dz_s3, int M, const void* x_s3, int x_channels, int xh, int xw, int N, int pad_top,
                              int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n, int n_off, int fmt,
                              bool det, void* workspace, long long workspace_bytes, void* stream) {
  const char* who = det ? "conv_wgrad_s3_det" : "conv_wgrad_s3";
  // 96-pixel tiles (3x32 / 6x16 / 12x8: three k-steps per LDS fill, so that the MFMAs of one workgroup outlast
  // the DMA wait of its co-resident partner) were measured no faster: 25.7 vs 24.0 ms per step for all launches.
  // tile shape with the least padded area (ties: the widest).  Weighting the area by the rate each shape
  // reaches on full tiles (2x32 250, 4x16 190, 8x8 103 TFLOP/s-equivalent) and so moving the 45x80 and 22x40
  // layers to 2x32 tiles was measured slower overall (31.0 vs 27.8 ms per step for all launches).
  // the split plan covers what the size query sees (M, N, batch, H, W, ksize); the source's own size and place it does not
  const DetWgradS3Plan p = det_wgrad_s3_plan(M, N, batch, H, W, ksize);
  SFH_REQUIRE(fmt == SFH_FMT_S3 || fmt == SFH_FMT_H2, "%s: fmt=%d (S3 or H2)", who, fmt);
  SFH_REQUIRE(p.why != DET_BAD_KSIZE, "%s: ksize=%d (3 or 1)", who, ksize);
  const unsigned long long bpe = fmt == SFH_FMT_H2 ? 4ULL : 6ULL;
  SFH_REQUIRE(dz_s3 && x_s3 && raw, "%s: null pointer", who);
  SFH_REQUIRE(p.why != DET_BAD_FRAME && xh > 0 && xw > 0, "%s: bad geometry", who);
  SFH_REQUIRE(p.why != DET_BAD_M, "%s: M=%d must be a multiple of 64", who, M);
  SFH_REQUIRE(p.why != DET_BAD_N && x_channels % 32 == 0 && x_channels >= N, "%s: N=%d of %d channels", who, N, x_channels);
  SFH_REQUIRE(n_off >= 0 && n_off + N <= raw_n, "%s: n_off=%d N=%d raw_n=%d", who, n_off, N, raw_n);
  SFH_REQUIRE(pad_top >= 0 && pad_left >= 0 && pad_top + xh <= H && pad_left + xw <= W, "%s: source does not fit the frame", who);
  const unsigned long long bdz = bpe * batch * H * W * M, bx = bpe * batch * xh * xw * x_channels;
  SFH_REQUIRE(sfh_fits_descriptor(bdz) && sfh_fits_descriptor(bx), "%s: a tensor of %llu bytes exceeds the 4 GiB descriptor range", who, bdz > bx ? bdz : bx);
  SFH_REQUIRE(p.ok, "%s: grid too large", who);
  WgS3Args a;
  a.dz = dz_s3; a.M = M; a.x = x_s3; a.xc = x_channels; a.xh = xh; a.xw = xw; a.N = N;
  a.pad_top = pad_top; a.pad_left = pad_left; a.batch = batch; a.H = H; a.W = W;
  a.raw = raw; a.raw_n = raw_n; a.n_off = n_off;
  a.mblk = M / 64; a.nblk = N / 32;
  a.bytes_dz = (unsigned)bdz; a.bytes_x = (unsigned)bx;
  a.ntx = a.nty = a.ntiles = a.nsplit = a.tps = 0;
  if (det) SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  float* ws = det ? (float*)workspace : nullptr;   // launch(): nullptr is the default mode
  hipStream_t st = (hipStream_t)stream;
#define SFH_WG_PICK(NP_, KS_)                                              \
  do {                                                                     \
    if (p.shape == 0) return launch<2, 32, NP_, KS_>(a, p, ws, st);        \
    if (p.shape == 1) return launch<4, 16, NP_, KS_>(a, p, ws, st);        \
    return launch<8, 8, NP_, KS_>(a, p, ws, st);                           \
  } while (0)
  if (fmt == SFH_FMT_H2) {
    if (ksize == 1) SFH_WG_PICK(2, 1);
    SFH_WG_PICK(2, 3);
  }
  if (ksize == 1) SFH_WG_PICK(3, 1);
  SFH_WG_PICK(3, 3);
#undef SFH_WG_PICK
}

extern "C" int sfh_conv_wgrad_s3(const void* dz_s3, int M, const void* x_s3, int x_channels, int xh, int xw, int N,
                                 int pad_top, int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n,
                                 int n_off, int fmt, void* stream) {
  return conv_wgrad_s3_impl(dz_s3, M, x_s3, x_channels, xh, xw, N, pad_top, pad_left, batch, H, W, ksize, raw, raw_n, n_off, fmt,
                            false, nullptr, 0, stream);
}

extern "C" int64_t sfh_conv_wgrad_s3_det_bytes(int M, int N, int batch, int H, int W, int ksize) {
  return det_bytes(det_wgrad_s3_plan(M, N, batch, H, W, ksize));
}

extern "C" int sfh_conv_wgrad_s3_det(const void* dz_s3, int M, const void* x_s3, int x_channels, int xh, int xw, int N,
                                     int pad_top, int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n,
                                     int n_off, int fmt, void* workspace, long long workspace_bytes, void* stream) {
  return conv_wgrad_s3_impl(dz_s3, M, x_s3, x_channels, xh, xw, N, pad_top, pad_left, batch, H, W, ksize, raw, raw_n, n_off, fmt,
                            true, workspace, workspace_bytes, stream);
}
