// refine.hip - homography refinement against the segmentation: direct alignment of the court template to the UNet's class
// probabilities by damped Gauss-Newton steps, coarse to fine.  The rule (planes, coordinates, cost, step) is stated once in
// include/sfh_amd.h above the sfh_refine_* entries; tests/refine_ref.py restates it in numpy.
//
// * refine_template_planes_kernel / refine_evidence_planes_kernel: one thread per averaged pixel; channel-last planes, so a
//   bilinear tap of every class is one (CP = 4) or two (CP = 8) 16-byte loads.
// * refine_accumulate_kernel: a workgroup covers 64 columns x 64 rows of the evidence grid (a wave 64 x 16, a lane one column);
//   the coordinate walk is warp_coords.h's on the grid of sfh_refine_axis, the fp32 / fp64 staging that of
//   warp_bwd_theta_kernel (warp.hip).  The 45 sums are reduced by wave shuffle, then across the four waves through LDS, and
//   stored once into the workgroup's slab: the store pass of det_core.h.  No atomics, no workgroup waits for another.
// * refine_step_kernel: one wave per frame; lanes 0..44 take the ascending chain over the slabs (det_sum), every lane then
//   holds all 45 sums and solves the 8 x 8 system redundantly in registers, as prep_fit_kernel (prepare.hip) does: both
//   call chol8_solve (chol8.h).
#include "common.h"
#include "warp_coords.h"
#include "det_core.h"
#include "chol8.h"

namespace {

constexpr int kSums = SFH_REFINE_SUMS;   // upper triangle of 8 x 8 (36) + J^T r (8) + cost (1)
constexpr int kTile = DET_FIT_TILE, kWaveRows = 16;   // a workgroup's 64 x 64 pixels, four waves of 64 x 16

__host__ __device__ inline int refine_cp(int nc) { return nc <= 5 ? 4 : 8; }

// ------------------------------------------------------------------ planes
template <int CP>
__global__ __launch_bounds__(256) void refine_template_planes_kernel(const float* __restrict__ tmpl, int n, int ht, int wt, int nc,
                                                                     int f, float* __restrict__ planes) {
  const int wo = wt / f, ho = ht / f;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * ho * wo) return;
  const int x = (int)(idx % wo), y = (int)((idx / wo) % ho), b = (int)(idx / ((long)wo * ho));
  int cnt[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) cnt[c] = 0;
  const float* src = tmpl + ((long)b * ht + (long)y * f) * wt + (long)x * f;
  for (int dy = 0; dy < f; ++dy)
    for (int dx = 0; dx < f; ++dx) {
      const int id = (int)rintf(__fmul_rn(src[(long)dy * wt + dx], (float)nc));
#pragma unroll
      for (int c = 0; c < CP; ++c) cnt[c] += (id == c + 1 && c + 1 < nc) ? 1 : 0;
    }
  const float ff = (float)(f * f);
#pragma unroll
  for (int c = 0; c < CP; ++c) planes[idx * CP + c] = __fdiv_rn((float)cnt[c], ff);
}

template <int CP>
__global__ __launch_bounds__(256) void refine_evidence_planes_kernel(const float* __restrict__ logits, int batch, int nc, int hl,
                                                                     int wl, int f, float* __restrict__ planes) {
  const int wo = wl / f, ho = hl / f;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)batch * ho * wo) return;
  const int x = (int)(idx % wo), y = (int)((idx / wo) % ho), b = (int)(idx / ((long)wo * ho));
  const long plane = (long)hl * wl;
  const float* src = logits + (long)b * nc * plane + ((long)y * f) * wl + (long)x * f;
  float sum[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) sum[c] = 0.f;
  for (int dy = 0; dy < f; ++dy)
    for (int dx = 0; dx < f; ++dx) {
      float l[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) l[k] = k < nc ? src[k * plane + (long)dy * wl + dx] : 0.f;
      float m = l[0];
#pragma unroll
      for (int k = 1; k < 8; ++k) m = (k < nc) ? sfh_max_nan(m, l[k]) : m;
      float e[8], se = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        e[k] = k < nc ? expf(__fsub_rn(l[k], m)) : 0.f;
        se = k < nc ? __fadd_rn(se, e[k]) : se;
      }
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c + 1 < nc) sum[c] = __fadd_rn(sum[c], __fdiv_rn(e[(c + 1) & 7], se));
    }
  const float ff = (float)(f * f);
#pragma unroll
  for (int c = 0; c < CP; ++c) planes[idx * CP + c] = __fdiv_rn(sum[c], ff);
}

// ------------------------------------------------------------------ accumulate
// the CP planes of the tap at integral-valued (fx, fy) (or NaN / inf): in range -> the planes, else 0
template <int CP>
__device__ __forceinline__ void refine_tap(const float* __restrict__ tp, float fx, float fy, int wtf, int htf, float (&v)[CP]) {
  if (fx >= 0.f && fx <= (float)(wtf - 1) && fy >= 0.f && fy <= (float)(htf - 1)) {
    const f32x4* p = reinterpret_cast<const f32x4*>(tp + ((long)(int)fy * wtf + (int)fx) * CP);
#pragma unroll
    for (int q = 0; q < CP / 4; ++q) {
      const f32x4 t = p[q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < CP; ++c) v[c] = 0.f;
  }
}

template <int CP>
__global__ __launch_bounds__(256) void refine_accumulate_kernel(const float* __restrict__ theta, const float* __restrict__ tplanes,
                                                                long tplanes_bstride, int htf, int wtf,
                                                                const float* __restrict__ eplanes, int he, int we, float ax,
                                                                float cx, float ay, float cy, double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.z;
  const int x = blockIdx.x * kTile + lane;
  Homog H;
#pragma unroll
  for (int k = 0; k < 9; ++k) H.t[k] = theta[b * 9 + k];
  const float* tp = tplanes + (long)b * tplanes_bstride;
  const double hx = 0.5 * wtf, hy = 0.5 * htf;
  double acc[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
  if (x < we) {
    const float xn = __builtin_fmaf(ax, (float)x, cx);
    for (int r = 0; r < kWaveRows; ++r) {
      const int y = blockIdx.y * kTile + wv * kWaveRows + r;
      if (y >= he) break;
      const float yn = __builtin_fmaf(ay, (float)y, cy);
      const float X = __fadd_rn(__fadd_rn(__fmul_rn(H.t[0], xn), __fmul_rn(H.t[1], yn)), H.t[2]);
      const float Y = __fadd_rn(__fadd_rn(__fmul_rn(H.t[3], xn), __fmul_rn(H.t[4], yn)), H.t[5]);
      const float Z = __fadd_rn(__fadd_rn(__fmul_rn(H.t[6], xn), __fmul_rn(H.t[7], yn)), H.t[8]);
      const bool live = fabsf(Z) > 1e-8f;
      const float s = live ? __fdiv_rn(1.0f, __fadd_rn(Z, 1e-8f)) : 1.0f;
      const float px = unnorm(__fmul_rn(s, X), wtf), py = unnorm(__fmul_rn(s, Y), htf);
      const float x0 = floorf(px), y0 = floorf(py);
      const float wx1 = __fsub_rn(px, x0), wx0 = __fsub_rn(1.0f, wx1), wy1 = __fsub_rn(py, y0), wy0 = __fsub_rn(1.0f, wy1);
      const float w00 = __fmul_rn(wy0, wx0), w01 = __fmul_rn(wy0, wx1), w10 = __fmul_rn(wy1, wx0), w11 = __fmul_rn(wy1, wx1);
      float t00[CP], t01[CP], t10[CP], t11[CP], ev[CP];
      refine_tap<CP>(tp, x0, y0, wtf, htf, t00);
      refine_tap<CP>(tp, x0 + 1.f, y0, wtf, htf, t01);
      refine_tap<CP>(tp, x0, y0 + 1.f, wtf, htf, t10);
      refine_tap<CP>(tp, x0 + 1.f, y0 + 1.f, wtf, htf, t11);
      {
        const f32x4* p = reinterpret_cast<const f32x4*>(eplanes + (((long)b * he + y) * we + x) * CP);
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
          const f32x4 t = p[q];
          ev[4 * q] = t.x; ev[4 * q + 1] = t.y; ev[4 * q + 2] = t.z; ev[4 * q + 3] = t.w;
        }
      }
      double Suu = 0.0, Suv = 0.0, Svv = 0.0, Sur = 0.0, Svr = 0.0, Srr = 0.0;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        float val = __fmul_rn(t00[c], w00);
        val = __fadd_rn(val, __fmul_rn(t01[c], w01));
        val = __fadd_rn(val, __fmul_rn(t10[c], w10));
        val = __fadd_rn(val, __fmul_rn(t11[c], w11));
        const float duf = __fadd_rn(__fmul_rn(wy0, __fsub_rn(t01[c], t00[c])), __fmul_rn(wy1, __fsub_rn(t11[c], t10[c])));
        const float dvf = __fadd_rn(__fmul_rn(wx0, __fsub_rn(t10[c], t00[c])), __fmul_rn(wx1, __fsub_rn(t11[c], t01[c])));
        const double rr = (double)val - (double)ev[c];
        const double du = (double)duf * hx, dv = (double)dvf * hy;
        Suu += du * du; Suv += du * dv; Svv += dv * dv;
        Sur += du * rr; Svr += dv * rr; Srr += rr * rr;
      }
      const double ds = (double)s, dxn = (double)xn, dyn = (double)yn;
      const double gu = live ? -((double)X * ds) * ds : 0.0, gv = live ? -((double)Y * ds) * ds : 0.0;
      const double a[8] = {ds * dxn, ds * dyn, ds, 0.0, 0.0, 0.0, gu * dxn, gu * dyn};
      const double bb[8] = {0.0, 0.0, 0.0, ds * dxn, ds * dyn, ds, gv * dxn, gv * dyn};
      int e = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i; j < 8; ++j, ++e)
          acc[e] += (Suu * (a[i] * a[j]) + Suv * (a[i] * bb[j] + bb[i] * a[j])) + Svv * (bb[i] * bb[j]);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[36 + i] += Sur * a[i] + Svr * bb[i];
      acc[44] += Srr;
    }
  }
  __shared__ double sh[4][kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) {
    double v = acc[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) sh[wv][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const int e = threadIdx.x;
    const long slab = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[det_slab_offset(slab, (long)kSums * gridDim.z) + (long)b * kSums + e] = ((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e];
  }
}

// ------------------------------------------------------------------ step
__global__ __launch_bounds__(64) void refine_step_kernel(const double* __restrict__ partial, long slabs, int batch, int first,
                                                         int last, const float* theta_eval, float* theta_acc, double* sums_acc,
                                                         double* lambda, int32_t* pivots_ok, float* theta_next, double* cost,
                                                         int32_t* accepted, int level, int nlevels) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const double mine = lane < kSums ? det_sum(0.0, partial, slabs, (long)kSums * batch, (long)b * kSums + lane) : 0.0;
  double S[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) S[e] = __shfl(mine, e);
  float te[9], ta[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) te[k] = theta_eval[b * 9 + k];
  double lam = 1e-3;
  int nacc = 0;
  bool take = true;
  if (!first) {
    take = pivots_ok[b] != 0 && S[44] < sums_acc[b * kSums + 44];   // false for a NaN cost
    lam = take ? lambda[b] / 10.0 : lambda[b] * 10.0;
    nacc = accepted[b * nlevels + level] + (take ? 1 : 0);
  }
  if (!take) {
#pragma unroll
    for (int e = 0; e < kSums; ++e) S[e] = sums_acc[b * kSums + e];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) ta[k] = take ? te[k] : theta_acc[b * 9 + k];

  // (J^T J + lambda diag(J^T J)) delta = -J^T r by chol8.h; a pivot that is not positive rejects the step
  double Lm[8][8], gv[8];
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = i; j < 8; ++j, ++e) Lm[j][i] = (i == j) ? S[e] + lam * S[e] : S[e];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) gv[i] = -S[36 + i];
  const bool ok = chol8_solve(Lm, gv, true);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      theta_acc[b * 9 + k] = ta[k];
      theta_next[b * 9 + k] = (last || !ok || k == 8) ? ta[k] : (float)((double)ta[k] + gv[k]);
    }
    if (take) {
#pragma unroll
      for (int e = 0; e < kSums; ++e) sums_acc[b * kSums + e] = S[e];
    }
    lambda[b] = lam;
    pivots_ok[b] = ok ? 1 : 0;
    accepted[b * nlevels + level] = nacc;
    if (first) cost[((long)b * nlevels + level) * 2] = S[44];
    cost[((long)b * nlevels + level) * 2 + 1] = S[44];
  }
}

// what accumulate, the size query and the step's caller agree on: the slab grid of an evidence grid of h x w
// (det_refine_plan, det_core.h)
static_assert(kSums == DET_REFINE_SUMS, "refine sums");

inline void refine_axis(int f, int n, int nl, float& a, float& c) {
  a = (float)((2.0 * f * n) / ((double)nl * (n - 1)));
  c = (float)((((double)f * n / nl - 1.0) / (n - 1)) - 1.0);
}

}  // namespace

extern "C" int sfh_refine_axis(int f, int n, int nl, float* a) {
  SFH_REQUIRE(a, "refine_axis: null pointer");
  SFH_REQUIRE(f >= 1 && n > 1 && nl >= 1 && nl % f == 0, "refine_axis: level %d, %d grid points, %d logits", f, n, nl);
  refine_axis(f, n, nl, a[0], a[1]);
  return SFH_OK;
}

extern "C" int sfh_refine_template_planes(const float* tmpl, int n, int ht, int wt, int nc, int f, float* planes, void* stream) {
  SFH_REQUIRE(tmpl && planes, "refine_template_planes: null pointer");
  SFH_REQUIRE(nc >= 2 && nc <= 8, "refine_template_planes: nc=%d (2..8)", nc);
  SFH_REQUIRE(n > 0 && ht > 0 && wt > 0 && f >= 1 && f <= 64, "refine_template_planes: bad geometry n=%d ht=%d wt=%d f=%d", n, ht, wt, f);
  SFH_REQUIRE(ht % f == 0 && wt % f == 0, "refine_template_planes: level %d does not divide the template %dx%d", f, wt, ht);
  const long total = (long)n * (ht / f) * (wt / f);
  SFH_REQUIRE(total * 8 < (1L << 31), "refine_template_planes: %ld pixels: too large", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (refine_cp(nc) == 4)
    hipLaunchKernelGGL(refine_template_planes_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, tmpl, n, ht, wt, nc, f, planes);
  else
    hipLaunchKernelGGL(refine_template_planes_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, tmpl, n, ht, wt, nc, f, planes);
  return sfh_check_launch("refine_template_planes_kernel");
}

extern "C" int sfh_refine_evidence_planes(const float* logits, int batch, int nc, int hl, int wl, int f, float* planes,
                                          void* stream) {
  SFH_REQUIRE(logits && planes, "refine_evidence_planes: null pointer");
  SFH_REQUIRE(nc >= 2 && nc <= 8, "refine_evidence_planes: nc=%d (2..8)", nc);
  SFH_REQUIRE(batch > 0 && hl > 0 && wl > 0 && f >= 1 && f <= 64, "refine_evidence_planes: bad geometry b=%d hl=%d wl=%d f=%d", batch,
              hl, wl, f);
  SFH_REQUIRE(hl % f == 0 && wl % f == 0, "refine_evidence_planes: level %d does not divide the logits %dx%d", f, wl, hl);
  const long total = (long)batch * (hl / f) * (wl / f);
  SFH_REQUIRE(total * 8 < (1L << 31), "refine_evidence_planes: %ld pixels: too large", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (refine_cp(nc) == 4)
    hipLaunchKernelGGL(refine_evidence_planes_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, logits, batch, nc, hl, wl, f, planes);
  else
    hipLaunchKernelGGL(refine_evidence_planes_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, logits, batch, nc, hl, wl, f, planes);
  return sfh_check_launch("refine_evidence_planes_kernel");
}

extern "C" int64_t sfh_refine_workspace_bytes(int batch, int h, int w) { return det_bytes(det_refine_plan(batch, h, w)); }

extern "C" int sfh_refine_accumulate(const float* theta, const float* tplanes, int64_t tplanes_bstride, int ht, int wt,
                                     const float* eplanes, int batch, int nc, int hl, int wl, int H, int W, int f, void* workspace,
                                     long long workspace_bytes, void* stream) {
  const char* who = "refine_accumulate";
  SFH_REQUIRE(theta && tplanes && eplanes, "%s: null pointer", who);
  SFH_REQUIRE(nc >= 2 && nc <= 8, "%s: nc=%d (2..8)", who, nc);
  SFH_REQUIRE(ht > 0 && wt > 0 && hl > 0 && wl > 0 && H > 1 && W > 1 && f >= 1 && f <= 64,
              "%s: bad geometry ht=%d wt=%d hl=%d wl=%d H=%d W=%d f=%d", who, ht, wt, hl, wl, H, W, f);
  SFH_REQUIRE(ht % f == 0 && wt % f == 0 && hl % f == 0 && wl % f == 0,
              "%s: level %d does not divide the template %dx%d and the logits %dx%d", who, f, wt, ht, wl, hl);
  const int htf = ht / f, wtf = wt / f, he = hl / f, we = wl / f, cp = refine_cp(nc);
  const DetPlan p = det_refine_plan(batch, he, we);
  SFH_REQUIRE(p.ok, "%s: batch %d (1..65535)", who, batch);
  SFH_REQUIRE((long)htf * wtf * cp < (1L << 29) && (long)batch * he * we * cp < (1L << 31), "%s: planes too large", who);
  SFH_REQUIRE(tplanes_bstride == 0 || (tplanes_bstride >= (int64_t)htf * wtf * cp && tplanes_bstride % 4 == 0),
              "%s: bad template plane stride %lld (0, or a multiple of 4 floats not below one frame's planes)", who,
              (long long)tplanes_bstride);
  // both plane sets are read with 16-byte loads
  SFH_REQUIRE(((uintptr_t)tplanes | (uintptr_t)eplanes) % 16 == 0, "%s: the planes must be 16-byte aligned", who);
  SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  float ax, cx, ay, cy;
  refine_axis(f, W, wl, ax, cx);
  refine_axis(f, H, hl, ay, cy);
  const dim3 grid((unsigned)det_cdiv(we, kTile), (unsigned)det_cdiv(he, kTile), (unsigned)batch);
  if (cp == 4)
    hipLaunchKernelGGL(refine_accumulate_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, theta, tplanes, (long)tplanes_bstride,
                       htf, wtf, eplanes, he, we, ax, cx, ay, cy, (double*)workspace);
  else
    hipLaunchKernelGGL(refine_accumulate_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, theta, tplanes, (long)tplanes_bstride,
                       htf, wtf, eplanes, he, we, ax, cx, ay, cy, (double*)workspace);
  return sfh_check_launch("refine_accumulate_kernel");
}

extern "C" int sfh_refine_step(const double* partial, int64_t slabs, int batch, int first, int last, const float* theta_eval,
                               float* theta_acc, double* sums_acc, double* lambda, int32_t* pivots_ok, float* theta_next,
                               double* cost, int32_t* accepted, int level, int nlevels, void* stream) {
  SFH_REQUIRE(partial && theta_eval && theta_acc && sums_acc && lambda && pivots_ok && theta_next && cost && accepted,
              "refine_step: null pointer");
  SFH_REQUIRE(slabs >= 1 && batch > 0 && batch <= 65535 && nlevels >= 1 && level >= 0 && level < nlevels,
              "refine_step: bad geometry slabs=%lld batch=%d level=%d of %d", (long long)slabs, batch, level, nlevels);
  hipLaunchKernelGGL(refine_step_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, partial, (long)slabs, batch, first,
                     last, theta_eval, theta_acc, sums_acc, lambda, pivots_ok, theta_next, cost, accepted, level, nlevels);
  return sfh_check_launch("refine_step_kernel");
}
