// eval.hip - the validation scores of eval.py:142-234 (eval_reconstructor) for one batch, added into a device accumulator.
//
// Two launches per batch, no atomics on any sum (bit-reproducible; the pattern of warpce_kernel + warpce_final_kernel):
//  1. eval_pixels_kernel: one wave per frame row.  The logits (NCHW), the int64 mask and the warp of a row are streamed once
//     with 16-byte loads (4 pixels per lane) when the row allows it; per pixel lse = logsumexp_k L[k] is formed ONCE and gives
//       seg     = lse - L[g]                          (0 and not counted where g == -100, torch's ignore_index)
//       rec     = (v - fp32(g) / nc)^2
//       consist = lse - L[trunc(fp32(v * nc))]        (0 and not counted where that class is -100)
//     Lanes accumulate in fp64; each wave writes its five sums (seg, seg count, rec, consist, consist count) to the workspace.
//  2. eval_combine_kernel: ONE workgroup.  Wave w sums the row partials of frames w, w + 16, ... in row order (the per-frame
//     sums, fp64), together with the frame's reprojection distances (models/losses.py:6-19); after a barrier wave 0 forms the
//     batch's seg / rec / consist scores exactly as eval.py:180-203 reduces them and adds them to acc[].
//  A mask id outside [0, nc) other than -100, or a consistency class outside [0, nc) other than -100 (a non-finite warp
//  included), ORs bit 1 / bit 2 into *flag - torch raises on those inputs; the caller reads the flag once at the end.
#include "common.h"

namespace {

constexpr int kTerms = 5;          // per row / per frame: seg, seg count, rec, consist, consist count
constexpr int kFrameWords = 7;     // per frame: the five terms + reprojection (normalised, pixels)
constexpr int kCombineWaves = 16;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

struct Terms {
  double seg = 0.0, cnt = 0.0, rec = 0.0, cons = 0.0, ccnt = 0.0;
};

template <int NC>
__device__ __forceinline__ void eval_pixel(const float (&v)[NC], long long g, float wv, bool hl, bool hw, Terms& a,
                                           unsigned& bad) {
  float m = v[0], ls = 0.f;
  if (hl) {
#pragma unroll
    for (int k = 1; k < NC; ++k) m = sfh_max_nan(m, v[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) se += expf(v[k] - m);
    ls = logf(se);
    const bool ign = g == -100;
    const bool ok = g >= 0 && g < NC;
    bad |= (!ign && !ok) ? 1u : 0u;
    float xt = m;
#pragma unroll
    for (int k = 0; k < NC; ++k) xt = (g == k) ? v[k] : xt;
    // (m - L[g]) first: exact when the two are close, so a confident pixel keeps its small loss to full relative precision
    if (!ign) {
      a.seg += (double)((m - xt) + ls);
      a.cnt += 1.0;
    }
  }
  if (hw) {
    const float d = wv - __fdiv_rn((float)g, (float)NC);
    a.rec += (double)__fmul_rn(d, d);
    if (hl) {
      const float f = __fmul_rn(wv, (float)NC);      // (warp_masks * nc).to(torch.long): fp32 product, truncated
      const bool ok = f > -1.f && f < (float)NC;     // NaN fails both tests
      const bool ign = f > -101.f && f <= -100.f;
      bad |= (!ok && !ign) ? 2u : 0u;
      const int c = ok ? (int)f : 0;
      float xc = m;
#pragma unroll
      for (int k = 0; k < NC; ++k) xc = (c == k) ? v[k] : xc;
      if (ok) {
        a.cons += (double)((m - xc) + ls);
        a.ccnt += 1.0;
      }
    }
  }
}

// grid (ceil(H / 4), B), 256 threads: wave wv of block x handles row 4x + wv of frame blockIdx.y.  VEC = 4: W % 4 == 0 and
// every base pointer 16-byte aligned (checked by the launcher), so each lane moves 16 bytes per logit plane and per warp row
// and 32 bytes of mask.  logits / warp may be null (the net has no UNet / no warper).
template <int NC, int VEC>
__global__ __launch_bounds__(256) void eval_pixels_kernel(const float* __restrict__ logits, const int64_t* __restrict__ mask,
                                                          const float* __restrict__ warp, int H, int W,
                                                          double* __restrict__ part, unsigned* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (y >= H) return;                                 // whole waves only; the kernel has no barrier
  const bool hl = logits != nullptr, hw = warp != nullptr;
  const size_t plane = (size_t)H * W;
  const size_t row = ((size_t)b * H + y) * W;
  const float* lrow = hl ? logits + (size_t)b * NC * plane + (size_t)y * W : nullptr;
  Terms a;
  unsigned bad = 0;
  if (VEC == 4) {
    for (int x = lane * 4; x < W; x += 256) {
      f32x4 lv[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) lv[k] = hl ? *reinterpret_cast<const f32x4*>(lrow + k * plane + x) : f32x4{0.f, 0.f, 0.f, 0.f};
      const i64x2 g01 = *reinterpret_cast<const i64x2*>(mask + row + x);
      const i64x2 g23 = *reinterpret_cast<const i64x2*>(mask + row + x + 2);
      const f32x4 wv = hw ? *reinterpret_cast<const f32x4*>(warp + row + x) : f32x4{0.f, 0.f, 0.f, 0.f};
      const long long g[4] = {g01.x, g01.y, g23.x, g23.y};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k] = lv[k][i];
        eval_pixel<NC>(v, g[i], wv[i], hl, hw, a, bad);
      }
    }
  } else {
    for (int x = lane; x < W; x += 64) {
      float v[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) v[k] = hl ? lrow[k * plane + x] : 0.f;
      eval_pixel<NC>(v, (long long)mask[row + x], hw ? warp[row + x] : 0.f, hl, hw, a, bad);
    }
  }
  if (bad) atomicOr(flag, bad);                       // the error flag is the only atomic (bits, order-free)
  const double s0 = wave_sum(a.seg), s1 = wave_sum(a.cnt), s2 = wave_sum(a.rec), s3 = wave_sum(a.cons), s4 = wave_sum(a.ccnt);
  if (lane == 0) {
    const size_t n = (size_t)gridDim.y * H, i = (size_t)b * H + y;   // term-major: part[k * B * H + b * H + y]
    part[i] = s0;
    part[n + i] = s1;
    part[2 * n + i] = s2;
    part[3 * n + i] = s3;
    part[4 * n + i] = s4;
  }
}

// One workgroup of 16 waves.  fsum (B x 7 doubles, the workspace tail) holds the per-frame sums between the two phases.
__global__ __launch_bounds__(1024) void eval_combine_kernel(const double* __restrict__ part, double* __restrict__ fsum,
                                                            int B, int H, int W, int has_pix, int has_logits, int has_warp,
                                                            const float* __restrict__ weight, const float* __restrict__ poi,
                                                            const float* __restrict__ gt, const float* __restrict__ nz,
                                                            const float* __restrict__ nnz, int npts, float tw, float th,
                                                            const unsigned* __restrict__ flag, double* __restrict__ acc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t n = (size_t)B * H;
  for (int b = wv; b < B; b += kCombineWaves) {
    double s[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (has_pix)
      for (int y = lane; y < H; y += 64)
#pragma unroll
        for (int k = 0; k < kTerms; ++k) s[k] += part[k * n + (size_t)b * H + y];
    // models/losses.py:6-19 for frame b: sum_n ||gt - poi|| * nonzeros / num_nonzero, normalised and in pixels (x * tw,
    // y * th in fp32 first, as eval.py:209-212 scales the tensors)
    double r = 0.0, rp = 0.0;
    if (poi)
      for (int p = lane; p < npts; p += 64) {
        const size_t o = ((size_t)b * npts + p) * 2;
        const float px = poi[o], py = poi[o + 1], gx = gt[o], gy = gt[o + 1];
        const double w = (double)nz[(size_t)b * npts + p];
        const double dx = (double)gx - (double)px, dy = (double)gy - (double)py;
        const double ex = (double)__fmul_rn(gx, tw) - (double)__fmul_rn(px, tw);
        const double ey = (double)__fmul_rn(gy, th) - (double)__fmul_rn(py, th);
        r += sqrt(dx * dx + dy * dy) * w;
        rp += sqrt(ex * ex + ey * ey) * w;
      }
#pragma unroll
    for (int k = 0; k < kTerms; ++k) s[k] = wave_sum(s[k]);
    r = wave_sum(r);
    rp = wave_sum(rp);
    if (lane == 0) {
      double* f = fsum + (size_t)b * kFrameWords;
#pragma unroll
      for (int k = 0; k < kTerms; ++k) f[k] = s[k];
      const double d = poi ? (double)nnz[b] : 1.0;
      f[5] = r / d;
      f[6] = rp / d;
    }
  }
  __syncthreads();
  if (wv != 0) return;
  // eval.py:180-203 over the frames of the batch, lanes in frame order, then a fixed shuffle tree
  const double hw = (double)H * (double)W;
  double seg = 0.0, cnt = 0.0, rec = 0.0, cons = 0.0, ccnt = 0.0, r = 0.0, rp = 0.0;
  for (int b = lane; b < B; b += 64) {
    const double* f = fsum + (size_t)b * kFrameWords;
    const double w = weight ? (double)weight[b] : 1.0;
    seg += weight ? w * (f[0] / hw) : f[0];           // per_sample_weighted_criterion: mean over the frame's pixels * w_b
    cnt += f[1];
    rec += weight ? w * (f[2] / hw) : f[2];
    cons += f[3];
    ccnt += f[4];
    r += f[5];
    rp += f[6];
  }
  seg = wave_sum(seg);
  cnt = wave_sum(cnt);
  rec = wave_sum(rec);
  cons = wave_sum(cons);
  ccnt = wave_sum(ccnt);
  r = wave_sum(r);
  rp = wave_sum(rp);
  if (lane == 0) {
    if (has_logits) acc[SFH_EVAL_SEG] += weight ? seg / (double)B : seg / cnt;      // unweighted: F.cross_entropy 'mean'
    if (has_warp) acc[SFH_EVAL_REC] += weight ? rec / (double)B : rec / ((double)B * hw);
    if (has_logits && has_warp) acc[SFH_EVAL_CONSIST] += cons / ccnt;
    if (poi) {
      acc[SFH_EVAL_REPROJ] += r;
      acc[SFH_EVAL_REPROJ_PX] += rp;
    }
    acc[SFH_EVAL_FRAMES] += (double)B;
    acc[SFH_EVAL_BAD] = (double)*flag;              // sticky: the flag is only ever OR'ed
  }
}

}  // namespace

extern "C" int64_t sfh_eval_workspace_doubles(int batch, int H, int W) {
  if (batch <= 0 || batch > 65535 || H <= 0 || W <= 0) return -1;
  return (int64_t)kTerms * batch * H + (int64_t)kFrameWords * batch;
}

extern "C" int sfh_eval_batch(const float* logits, const int64_t* mask, const float* warp_mask, const float* weight, int nc,
                              int batch, int H, int W, const float* poi, const float* gt_poi, const float* nonzeros,
                              const float* num_nonzero, int npts, float target_w, float target_h, double* workspace,
                              uint32_t* flag, double* acc, void* stream) {
  SFH_REQUIRE(workspace && flag && acc, "eval_batch: null workspace / flag / accumulator");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 0 && W > 0, "eval_batch: bad geometry b=%d h=%d w=%d", batch, H, W);
  SFH_REQUIRE(nc >= 1 && nc <= 8, "eval_batch: nc=%d (1 .. 8 classes)", nc);
  const bool has_pix = logits || warp_mask;
  SFH_REQUIRE(!has_pix || mask, "eval_batch: logits / warp without a mask");
  SFH_REQUIRE(!poi || (gt_poi && nonzeros && num_nonzero && npts > 0),
              "eval_batch: poi needs gt_poi, nonzeros, num_nonzero and npts > 0 (npts=%d)", npts);
  SFH_REQUIRE((int64_t)nc * H * W <= ((int64_t)1 << 40), "eval_batch: frame too large");
  if (has_pix) {
    const bool vec = W % 4 == 0 && (((uintptr_t)logits | (uintptr_t)mask | (uintptr_t)warp_mask) & 15) == 0;
    const dim3 grid((unsigned)sfh_cdiv(H, 4), (unsigned)batch);
#define SFH_EVAL_PIX(NC)                                                                                                    \
  case NC:                                                                                                                  \
    if (vec)                                                                                                                \
      hipLaunchKernelGGL((eval_pixels_kernel<NC, 4>), grid, dim3(256), 0, (hipStream_t)stream, logits, mask, warp_mask, H, \
                         W, workspace, flag);                                                                               \
    else                                                                                                                    \
      hipLaunchKernelGGL((eval_pixels_kernel<NC, 1>), grid, dim3(256), 0, (hipStream_t)stream, logits, mask, warp_mask, H, \
                         W, workspace, flag);                                                                               \
    break
    switch (nc) {
      SFH_EVAL_PIX(1); SFH_EVAL_PIX(2); SFH_EVAL_PIX(3); SFH_EVAL_PIX(4);
      SFH_EVAL_PIX(5); SFH_EVAL_PIX(6); SFH_EVAL_PIX(7); SFH_EVAL_PIX(8);
    }
#undef SFH_EVAL_PIX
    const int rc = sfh_check_launch("eval_pixels_kernel");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(eval_combine_kernel, dim3(1), dim3(64 * kCombineWaves), 0, (hipStream_t)stream, workspace,
                     workspace + (size_t)kTerms * batch * H, batch, H, W, has_pix ? 1 : 0, logits ? 1 : 0, warp_mask ? 1 : 0,
                     weight, poi, gt_poi, nonzeros, num_nonzero, npts, target_w, target_h, (const unsigned*)flag, acc);
  return sfh_check_launch("eval_combine_kernel");
}
