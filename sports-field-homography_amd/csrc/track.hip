// track.hip - inter-frame homography tracking: direct photometric alignment of a frame to the one before it by robust
// Levenberg-Marquardt steps, coarse to fine, and the rule that carries theta across the result.  The rule (planes,
// coordinates, residual, weight, step, propagation) is stated once in include/sfh_amd.h above the sfh_track_* entries;
// tests/track_ref.py restates it in numpy.  A close relative of refine.hip, whose structure it keeps:
//
// * track_planes_kernel: one thread per averaged pixel; the luma is ycc.h's, the sum an exact integer, one IEEE division.
// * track_accumulate_kernel: a workgroup covers 64 columns x 64 rows of the current frame's plane (a wave 64 x 16, a lane one
//   column, so the current plane's row is one contiguous load at any width); the previous plane is a gather of four scalar
//   taps.  fp32 staging as in refine_accumulate_kernel, fp64 behind it.  The 46 sums are reduced by wave_sum, then across the
//   four waves through LDS, and stored once into the workgroup's slab: the store pass of det_core.h.  No atomics.
// * track_step_kernel: one wave per pair; lanes 0..45 take the ascending chain over the slabs (det_sum), every lane then
//   holds all 46 sums and solves the 8 x 8 system redundantly in registers through chol8_solve (chol8.h).
// * track_propagate_kernel: one thread per frame, O(max_gap) work, no scan.
// * track_smooth_kernel: one wave per frame, a lane per frame of its window (smooth_core.h: chain, projection, weights, refit);
//   the nine sums of a pass through wave_sum_all, so every lane holds the combined points and solves the refit for itself.
// * track_search_cost_kernel, track_search_choice_kernel (at the end of the file): the coarse shift search that gives an
//   alignment its start.  One wave per (pair, whole-pixel shift) sums the robust cost of the coarsest planes in a fixed order
//   and stores the mean into a table; one wave per pair then takes the smallest key (search_core.h).  No atomics.
#include <cmath>

#include "common.h"
#include "det_core.h"
#include "chol8.h"
#include "ycc.h"
#include "track_core.h"
#include "smooth_core.h"
#include "search_core.h"

namespace {

constexpr int kSums = SFH_TRACK_SUMS;   // upper triangle of 8 x 8 (36) + g (8) + cost (1) + n (1)
constexpr int kCost = 44, kN = 45;
constexpr int kTile = DET_FIT_TILE, kWaveRows = 16;
static_assert(kSums == DET_TRACK_SUMS, "track sums");
static_assert(kSums <= 64, "one lane per sum in the step");

// ------------------------------------------------------------------ planes
__global__ __launch_bounds__(256) void track_planes_kernel(const uint8_t* __restrict__ frames, int batch, int H, int W, int f,
                                                           int ro, float* __restrict__ planes) {
  const int wo = W / f, ho = H / f;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)batch * ho * wo) return;
  const int x = (int)(idx % wo), y = (int)((idx / wo) % ho), b = (int)(idx / ((long)wo * ho));
  const uint8_t* src = frames + (((long)b * H + (long)y * f) * W + (long)x * f) * 3;
  int S = 0;
  for (int dy = 0; dy < f; ++dy)
    for (int dx = 0; dx < f; ++dx) {
      const uint8_t* p = src + ((long)dy * W + dx) * 3;
      S += ycc_y(p[ro], p[1], p[2 - ro]);
    }
  planes[idx] = __fdiv_rn((float)S, (float)(255 * f * f));
}

// ------------------------------------------------------------------ accumulate
struct TrackGeom {
  int hl, wl, nframes;
  float ax, cx, ay, cy, kx, ox, ky, oy;
  double d2;
};

__global__ __launch_bounds__(256) void track_accumulate_kernel(const float* __restrict__ M, const float* __restrict__ planes,
                                                               const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                               TrackGeom g, double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.z;
  const int x = blockIdx.x * kTile + lane;
  const int fa = ia[p], fb = ib[p];
  const bool pair_ok = fa >= 0 && fa < g.nframes && fb >= 0 && fb < g.nframes;   // wave-uniform
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = M[p * 9 + k];
  const long plane = (long)g.hl * g.wl;
  const float* prev = planes + (pair_ok ? fa : 0) * plane;
  const float* cur = planes + (pair_ok ? fb : 0) * plane;
  const float xmax = (float)(g.wl - 1), ymax = (float)(g.hl - 1);
  const double dkx = (double)g.kx, dky = (double)g.ky;
  double acc[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
  if (pair_ok && x < g.wl) {
    const float xn = __builtin_fmaf(g.ax, (float)x, g.cx);
    for (int r = 0; r < kWaveRows; ++r) {
      const int y = blockIdx.y * kTile + wv * kWaveRows + r;
      if (y >= g.hl) break;
      const float yn = __builtin_fmaf(g.ay, (float)y, g.cy);
      const float X = __fadd_rn(__fadd_rn(__fmul_rn(m[0], xn), __fmul_rn(m[1], yn)), m[2]);
      const float Y = __fadd_rn(__fadd_rn(__fmul_rn(m[3], xn), __fmul_rn(m[4], yn)), m[5]);
      const float Z = __fadd_rn(__fadd_rn(__fmul_rn(m[6], xn), __fmul_rn(m[7], yn)), m[8]);
      const bool live = fabsf(Z) > 1e-8f;
      const float s = live ? __fdiv_rn(1.0f, __fadd_rn(Z, 1e-8f)) : 1.0f;
      const float px = __builtin_fmaf(__fadd_rn(__fmul_rn(s, X), 1.0f), g.kx, -g.ox);
      const float py = __builtin_fmaf(__fadd_rn(__fmul_rn(s, Y), 1.0f), g.ky, -g.oy);
      const float x0 = floorf(px), y0 = floorf(py);
      // all four taps inside the previous plane; a NaN or an infinity fails a comparison
      const bool counts = live && x0 >= 0.f && __fadd_rn(x0, 1.0f) <= xmax && y0 >= 0.f && __fadd_rn(y0, 1.0f) <= ymax;
      if (!counts) continue;
      const float wx1 = __fsub_rn(px, x0), wx0 = __fsub_rn(1.0f, wx1), wy1 = __fsub_rn(py, y0), wy0 = __fsub_rn(1.0f, wy1);
      const float w00 = __fmul_rn(wy0, wx0), w01 = __fmul_rn(wy0, wx1), w10 = __fmul_rn(wy1, wx0), w11 = __fmul_rn(wy1, wx1);
      const float* tp = prev + (long)(int)y0 * g.wl + (int)x0;
      const float t00 = tp[0], t01 = tp[1], t10 = tp[g.wl], t11 = tp[g.wl + 1];
      const float cv = cur[(long)y * g.wl + x];
      float val = __fmul_rn(t00, w00);
      val = __fadd_rn(val, __fmul_rn(t01, w01));
      val = __fadd_rn(val, __fmul_rn(t10, w10));
      val = __fadd_rn(val, __fmul_rn(t11, w11));
      const float duf = __fadd_rn(__fmul_rn(wy0, __fsub_rn(t01, t00)), __fmul_rn(wy1, __fsub_rn(t11, t10)));
      const float dvf = __fadd_rn(__fmul_rn(wx0, __fsub_rn(t10, t00)), __fmul_rn(wx1, __fsub_rn(t11, t01)));
      const double rr = (double)val - (double)cv;
      const double du = (double)duf * dkx, dv = (double)dvf * dky;
      const double r2 = rr * rr;
      const double c = 1.0 + r2 / g.d2;
      const double ic = 1.0 / c;
      const double rho = r2 * ic, om = ic * ic;
      const double ds = (double)s, dxn = (double)xn, dyn = (double)yn;
      const double gu = -((double)X * ds) * ds, gv = -((double)Y * ds) * ds;
      const double a0 = ds * dxn, a1 = ds * dyn;
      const double J[8] = {du * a0, du * a1, du * ds, dv * a0, dv * a1, dv * ds,
                           du * (gu * dxn) + dv * (gv * dxn), du * (gu * dyn) + dv * (gv * dyn)};
      int e = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double wj = om * J[i];
#pragma unroll
        for (int j = i; j < 8; ++j, ++e) acc[e] += wj * J[j];
        acc[36 + i] += wj * rr;
      }
      acc[kCost] += rho;
      acc[kN] += 1.0;
    }
  }
  __shared__ double sh[4][kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) {
    const double v = wave_sum(acc[e]);
    if (lane == 0) sh[wv][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const int e = threadIdx.x;
    const long slab = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[det_slab_offset(slab, (long)kSums * gridDim.z) + (long)p * kSums + e] = ((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e];
  }
}

// ------------------------------------------------------------------ step
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for a NaN

__global__ __launch_bounds__(64) void track_step_kernel(const double* __restrict__ partial, long slabs, int pairs, int first,
                                                        int last, const float* M_eval, float* M_acc, double* sums_acc,
                                                        double* lambda, int32_t* pivots_ok, int32_t* dead, float* M_next,
                                                        double* stats, int32_t* accepted, int32_t* ok_out, int level,
                                                        int nlevels, double nmin, double max_cost) {
  const int lane = threadIdx.x, p = blockIdx.x;
  const double mine = lane < kSums ? det_sum(0.0, partial, slabs, (long)kSums * pairs, (long)p * kSums + lane) : 0.0;
  double S[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) S[e] = __shfl(mine, e);
  float me[9], ma[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) me[k] = M_eval[p * 9 + k];
  double lam = 1e-3;
  int nacc = 0;
  bool take = true, is_dead = false;
  if (first) {
    bool fin = true;
#pragma unroll
    for (int e = 0; e < kSums; ++e) fin = fin && finite_d(S[e]);
    is_dead = (level > 0 && dead[p] != 0) || !fin || !(S[kN] >= nmin);
  } else {
    is_dead = dead[p] != 0;
    const double mc = S[kCost] / S[kN], mk = sums_acc[p * kSums + kCost] / sums_acc[p * kSums + kN];
    take = !is_dead && pivots_ok[p] != 0 && S[kN] >= nmin && mc < mk;   // false for a NaN
    lam = is_dead ? lambda[p] : (take ? lambda[p] / 10.0 : lambda[p] * 10.0);
    nacc = accepted[p * nlevels + level] + (take ? 1 : 0);
  }
  if (!take) {
#pragma unroll
    for (int e = 0; e < kSums; ++e) S[e] = sums_acc[p * kSums + e];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) ma[k] = take ? me[k] : M_acc[p * 9 + k];

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
  const bool piv = chol8_solve(Lm, gv, true);
  if (lane == 0) {
    bool mfin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      M_acc[p * 9 + k] = ma[k];
      M_next[p * 9 + k] = (last || is_dead || !piv || k == 8) ? ma[k] : (float)((double)ma[k] + gv[k]);
      mfin = mfin && fabsf(ma[k]) <= 3.4028234663852886e38f;
    }
    if (take) {
#pragma unroll
      for (int e = 0; e < kSums; ++e) sums_acc[p * kSums + e] = S[e];
    }
    lambda[p] = lam;
    pivots_ok[p] = piv ? 1 : 0;
    dead[p] = is_dead ? 1 : 0;
    accepted[p * nlevels + level] = nacc;
    const double mean = S[kCost] / S[kN];
    double* st = stats + ((long)p * nlevels + level) * 3;
    if (first) st[0] = mean;
    st[1] = mean;
    st[2] = S[kN];
    ok_out[p] = (!is_dead && mfin && (!(max_cost > 0.0) || mean <= max_cost)) ? 1 : 0;
  }
}

// ------------------------------------------------------------------ propagate
__global__ __launch_bounds__(64) void track_propagate_kernel(const float* __restrict__ theta, const float* __restrict__ score,
                                                             float max_score, const float* __restrict__ M,
                                                             const int32_t* __restrict__ link, int frames, int max_gap,
                                                             float* __restrict__ theta_out, int32_t* __restrict__ source) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= frames) return;
  if (frame_good(theta, score, max_score, t)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) theta_out[(long)t * 9 + k] = theta[(long)t * 9 + k];
    source[t] = t;
    return;
  }
  int back = -1, fwd = -1;
  for (int d = 1; d <= max_gap; ++d) {       // the pairs (k, k+1) .. (t-1, t): link[k+1 .. t]
    const int k = t - d;
    if (k < 0 || link[k + 1] == 0) break;
    if (frame_good(theta, score, max_score, k)) { back = k; break; }
  }
  for (int d = 1; d <= max_gap; ++d) {       // the pairs (t, t+1) .. (k-1, k): link[t+1 .. k]
    const int k = t + d;
    if (k >= frames || link[k] == 0) break;
    if (frame_good(theta, score, max_score, k)) { fwd = k; break; }
  }
  const bool use_back = back >= 0 && (fwd < 0 || t - back <= fwd - t);
  const int k = use_back ? back : fwd;
  M3 P;
  bool have = k >= 0;
  if (have) {
    load3(theta + (long)k * 9, P);
    if (use_back) {
      for (int j = k + 1; j <= t; ++j) {
        M3 m;
        load3(M + (long)j * 9, m);
        mul3(P, m);
      }
    } else {
      for (int j = k; j >= t + 1; --j) {
        M3 m, a;
        load3(M + (long)j * 9, m);
        adj3(m, a);
        mul3(P, a);
      }
    }
    have = fabs(P.v[8]) > 0.0 && finite_d(P.v[8]);
  }
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < 9; ++i) theta_out[(long)t * 9 + i] = !have ? nan : (i == 8 ? 1.0f : (float)(P.v[i] / P.v[8]));
  source[t] = have ? k : -1;
}

// ------------------------------------------------------------------ smooth
struct SmoothCtrl {
  float p[8];
};

__global__ __launch_bounds__(64) void track_smooth_kernel(const float* __restrict__ theta, const float* __restrict__ score,
                                                          float max_score, const float* __restrict__ M,
                                                          const int32_t* __restrict__ link, int frames, int back, int ahead,
                                                          int iters, double d2, int min_members, SmoothCtrl ctrl,
                                                          float* __restrict__ theta_out, int32_t* __restrict__ members,
                                                          double* __restrict__ stats) {
  const int lane = threadIdx.x, t = blockIdx.x;
  const int k = t - back + lane;              // lane `back` is frame t itself
  bool mem = lane <= back + ahead && smooth_linked(theta, score, max_score, link, frames, k, t);
  double q[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (mem) {
    M3 P;
    smooth_chain(theta, M, k, t, P);
    mem = smooth_project(P, ctrl.p, q);
  }
  const unsigned long long mask = __ballot(mem);
  const int n = __popcll(mask);
  int ref = -1;                               // the member nearest to t, a tie goes back
  for (int d = 0; d <= SMOOTH_MAX_RADIUS && ref < 0; ++d) {
    if (d <= back && ((mask >> (back - d)) & 1ull)) ref = back - d;
    else if ((mask >> (back + d)) & 1ull) ref = back + d;
  }
  if (ref < 0) ref = 0;                       // no member: every sum is +0.0 and c is NaN
  const double g = smooth_triangle(k < t ? back : ahead, k < t ? t - k : k - t);
  double c0[8], dq[8], c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c0[i] = __shfl(q[i], ref);
    dq[i] = q[i] - c0[i];
    c[i] = c0[i];
  }
  double gw = 0.0, sw = 0.0;
  for (int pass = 0; pass <= iters; ++pass) {
    const double om = pass == 0 ? 1.0 : smooth_omega(smooth_r2(q, c), d2);
    gw = mem ? g * om : 0.0;
    sw = wave_sum_all(gw);
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i] = c0[i] + wave_sum_all(mem ? gw * dq[i] : 0.0) / sw;
  }
  const double r2 = smooth_r2(q, c);
  const double srr = wave_sum_all(mem ? gw * r2 : 0.0);
  const double own = __shfl(mem ? sqrt(r2) : (double)__builtin_nanf(""), back);
  bool ok = n >= min_members;
#pragma unroll
  for (int i = 0; i < 8; ++i) ok = ok && track_finite(c[i]);
  double h[8];
  ok = smooth_refit(ctrl.p, c, h, ok);
  if (lane == 0) {
    const float nanf_ = __builtin_nanf("");
    const double nand = (double)nanf_;
#pragma unroll
    for (int i = 0; i < 9; ++i) theta_out[(long)t * 9 + i] = !ok ? nanf_ : (i == 8 ? 1.0f : (float)h[i]);
    members[t] = n;
    stats[(long)t * 3] = ok ? sw : nand;
    stats[(long)t * 3 + 1] = ok ? sqrt(srr / sw) : nand;
    stats[(long)t * 3 + 2] = ok ? own : nand;
  }
}

}  // namespace

extern "C" int sfh_track_axis(int f, int n, float* a) {
  SFH_REQUIRE(a, "track_axis: null pointer");
  SFH_REQUIRE(track_level_ok(f, n), "track_axis: level %d (1..16) must divide %d pixels", f, n);
  track_axis(f, n, a[0], a[1]);
  return SFH_OK;
}

extern "C" int sfh_track_planes(const uint8_t* frames, int batch, int H, int W, int f, int bgr, float* planes, void* stream) {
  SFH_REQUIRE(frames && planes, "track_planes: null pointer");
  SFH_REQUIRE(batch > 0 && H > 0 && W > 0, "track_planes: bad geometry b=%d H=%d W=%d", batch, H, W);
  SFH_REQUIRE(track_level_ok(f, H) && track_level_ok(f, W), "track_planes: level %d (1..16) does not divide the frame %dx%d", f, W, H);
  SFH_REQUIRE((long)batch * H * W * 3 < (1L << 31), "track_planes: %ld bytes of frames: too large", (long)batch * H * W * 3);
  const long total = (long)batch * (H / f) * (W / f);
  hipLaunchKernelGGL(track_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, batch, H,
                     W, f, bgr ? 2 : 0, planes);
  return sfh_check_launch("track_planes_kernel");
}

extern "C" int64_t sfh_track_workspace_bytes(int pairs, int h, int w) { return det_bytes(det_track_plan(pairs, h, w)); }

extern "C" int sfh_track_accumulate(const float* M, const float* planes, int nframes, const int32_t* ia, const int32_t* ib,
                                    int pairs, int H, int W, int f, double delta, void* workspace, long long workspace_bytes,
                                    void* stream) {
  const char* who = "track_accumulate";
  SFH_REQUIRE(M && planes && ia && ib, "%s: null pointer", who);
  SFH_REQUIRE(nframes > 0 && H > 0 && W > 0, "%s: bad geometry frames=%d H=%d W=%d", who, nframes, H, W);
  SFH_REQUIRE(track_level_ok(f, H) && track_level_ok(f, W), "%s: level %d (1..16) does not divide the frame %dx%d", who, f, W, H);
  SFH_REQUIRE(delta > 0.0 && delta * delta > 0.0 && std::isfinite(delta * delta), "%s: delta=%g (> 0)", who, delta);
  TrackGeom g;
  g.hl = H / f;
  g.wl = W / f;
  g.nframes = nframes;
  const DetPlan p = det_track_plan(pairs, g.hl, g.wl);
  SFH_REQUIRE(p.ok, "%s: %d pairs (1..65535) of planes %dx%d", who, pairs, g.wl, g.hl);
  SFH_REQUIRE((long)nframes * g.hl * g.wl < (1L << 31), "%s: planes too large", who);
  SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  float a[2];
  if (sfh_refine_axis(f, W, W, a) != SFH_OK) return SFH_E_ARG;
  g.ax = a[0], g.cx = a[1];
  if (sfh_refine_axis(f, H, H, a) != SFH_OK) return SFH_E_ARG;
  g.ay = a[0], g.cy = a[1];
  track_axis(f, W, g.kx, g.ox);
  track_axis(f, H, g.ky, g.oy);
  g.d2 = delta * delta;
  const dim3 grid((unsigned)det_cdiv(g.wl, kTile), (unsigned)det_cdiv(g.hl, kTile), (unsigned)pairs);
  hipLaunchKernelGGL(track_accumulate_kernel, grid, dim3(256), 0, (hipStream_t)stream, M, planes, ia, ib, g, (double*)workspace);
  return sfh_check_launch("track_accumulate_kernel");
}

extern "C" int sfh_track_step(const double* partial, int64_t slabs, int pairs, int first, int last, const float* M_eval,
                              float* M_acc, double* sums_acc, double* lambda, int32_t* pivots_ok, int32_t* dead, float* M_next,
                              double* stats, int32_t* accepted, int32_t* ok, int level, int nlevels, double nmin, double max_cost,
                              void* stream) {
  SFH_REQUIRE(partial && M_eval && M_acc && sums_acc && lambda && pivots_ok && dead && M_next && stats && accepted && ok,
              "track_step: null pointer");
  SFH_REQUIRE(slabs >= 1 && pairs > 0 && pairs <= 65535 && nlevels >= 1 && level >= 0 && level < nlevels,
              "track_step: bad geometry slabs=%lld pairs=%d level=%d of %d", (long long)slabs, pairs, level, nlevels);
  SFH_REQUIRE(nmin >= 0.0 && max_cost == max_cost, "track_step: nmin=%g (>= 0), max_cost=%g (not a NaN)", nmin, max_cost);
  hipLaunchKernelGGL(track_step_kernel, dim3((unsigned)pairs), dim3(64), 0, (hipStream_t)stream, partial, (long)slabs, pairs, first,
                     last, M_eval, M_acc, sums_acc, lambda, pivots_ok, dead, M_next, stats, accepted, ok, level, nlevels, nmin,
                     max_cost);
  return sfh_check_launch("track_step_kernel");
}

extern "C" int sfh_track_propagate(const float* theta, const float* score, float max_score, const float* M, const int32_t* link,
                                   int frames, int max_gap, float* theta_out, int32_t* source, void* stream) {
  SFH_REQUIRE(theta && M && link && theta_out && source, "track_propagate: null pointer");
  SFH_REQUIRE(frames > 0 && frames < (1 << 24) && max_gap >= 0, "track_propagate: frames=%d (1..2^24-1), max_gap=%d (>= 0)", frames,
              max_gap);
  SFH_REQUIRE(theta_out + (long)frames * 9 <= theta || theta + (long)frames * 9 <= theta_out,
              "track_propagate: theta_out overlaps theta");
  hipLaunchKernelGGL(track_propagate_kernel, dim3((unsigned)det_cdiv(frames, 64)), dim3(64), 0, (hipStream_t)stream, theta, score,
                     max_score, M, link, frames, max_gap, theta_out, source);
  return sfh_check_launch("track_propagate_kernel");
}

extern "C" int sfh_track_smooth(const float* theta, const float* score, float max_score, const float* M, const int32_t* link,
                                int frames, int back, int ahead, int iters, double delta, int min_members, const float* ctrl,
                                float* theta_out, int32_t* members, double* stats, void* stream) {
  const char* who = "track_smooth";
  SFH_REQUIRE(frames >= 0, "%s: frames=%d (>= 0)", who, frames);
  SFH_REQUIRE(back >= 0 && back <= SMOOTH_MAX_RADIUS && ahead >= 0 && ahead <= SMOOTH_MAX_RADIUS, "%s: back=%d, ahead=%d (0..%d)", who,
              back, ahead, SMOOTH_MAX_RADIUS);
  SFH_REQUIRE(iters >= 0, "%s: iters=%d (>= 0)", who, iters);
  SFH_REQUIRE(delta > 0.0 && delta * delta > 0.0 && std::isfinite(delta * delta), "%s: delta=%g (> 0)", who, delta);
  SFH_REQUIRE(min_members >= 1, "%s: min_members=%d (>= 1)", who, min_members);
  SFH_REQUIRE(theta && M && link && theta_out && members && stats, "%s: null pointer", who);
  SFH_REQUIRE(theta_out + (long)frames * 9 <= theta || theta + (long)frames * 9 <= theta_out, "%s: theta_out overlaps theta", who);
  if (frames == 0) return SFH_OK;
  static const float kDefault[8] = {-1.0f, 0.2f, 1.0f, 0.2f, 1.0f, 1.0f, -1.0f, 1.0f};
  SmoothCtrl cp;
  for (int i = 0; i < 8; ++i) cp.p[i] = (ctrl ? ctrl : kDefault)[i];
  hipLaunchKernelGGL(track_smooth_kernel, dim3((unsigned)frames), dim3(64), 0, (hipStream_t)stream, theta, score, max_score, M, link,
                     frames, back, ahead, iters, delta * delta, min_members, cp, theta_out, members, stats);
  return sfh_check_launch("track_smooth_kernel");
}

// ------------------------------------------------------------------ coarse shift search
namespace {

constexpr int kSearchWaves = 4;   // candidates per workgroup of the cost kernel: one wave each

struct SearchGeom {
  int hl, wl, nframes, rx, ry, ncand;
  double d2;
};

// One wave per (pair, candidate).  Lane l adds the costs of its counted pixels for I ascending and, within a row, J = l, l + 64,
// .. ascending; wave_sum_all; one division by the analytic n; one plain store.  Both planes come through plain cached loads:
// a row of the current plane and the shifted row of the previous one are each one contiguous run per wave instruction.
__global__ __launch_bounds__(256) void track_search_cost_kernel(const float* __restrict__ planes, const int32_t* __restrict__ ia,
                                                                const int32_t* __restrict__ ib, SearchGeom g,
                                                                double* __restrict__ table) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.y;
  const int c = blockIdx.x * kSearchWaves + wv;   // wave-uniform
  if (c >= g.ncand) return;
  const int fa = ia[p], fb = ib[p];
  const bool pair_ok = fa >= 0 && fa < g.nframes && fb >= 0 && fb < g.nframes;   // wave-uniform
  int dx, dy;
  search_candidate(c, g.rx, g.ry, dx, dy);
  double acc = 0.0;
  if (pair_ok) {
    const long plane = (long)g.hl * g.wl;
    const float* prev = planes + fa * plane;
    const float* cur = planes + fb * plane;
    const int i0 = dy < 0 ? -dy : 0, i1 = dy > 0 ? g.hl - dy : g.hl;   // 0 <= I + dy < hl; empty when |dy| >= hl
    const int j0 = dx < 0 ? -dx : 0, j1 = dx > 0 ? g.wl - dx : g.wl;   // 0 <= J + dx < wl
    for (int I = i0; I < i1; ++I) {
      const float* pr = prev + (long)(I + dy) * g.wl + dx;
      const float* cr = cur + (long)I * g.wl;
      for (int J = lane; J < j1; J += 64)
        if (J >= j0) acc += search_rho(pr[J], cr[J], g.d2);
    }
  }
  const double cost = wave_sum_all(acc);
  const double mean = pair_ok ? cost / search_count(g.hl, g.wl, dx, dy) : (double)__builtin_nanf("");
  if (lane == 0) table[(long)p * g.ncand + c] = mean;
}

// One wave per pair walks the table in candidate order, lane l the candidates l, l + 64, ..; each lane keeps its best key,
// then the xor butterfly 32 .. 1 over keys (search_before is a strict total order on admissible keys, so every lane ends with
// the same one).  Lane 0 stores.
__global__ __launch_bounds__(64) void track_search_choice_kernel(const double* __restrict__ table, SearchGeom g, int f, int H, int W,
                                                                 double nmin, int32_t* __restrict__ shift,
                                                                 int32_t* __restrict__ found, float* __restrict__ m0,
                                                                 double* __restrict__ sstats) {
  const int lane = threadIdx.x, p = blockIdx.x;
  const double* row = table + (long)p * g.ncand;
  SearchKey best;
  best.mean = 0.0, best.dx = 0, best.dy = 0, best.ok = false;
  for (int c = lane; c < g.ncand; c += 64) {
    int dx, dy;
    search_candidate(c, g.rx, g.ry, dx, dy);
    const SearchKey k = search_key(row[c], search_count(g.hl, g.wl, dx, dy), nmin, dx, dy);
    if (search_before(k, best)) best = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    SearchKey other;
    other.mean = __shfl_xor(best.mean, o);
    other.dx = __shfl_xor(best.dx, o);
    other.dy = __shfl_xor(best.dy, o);
    other.ok = __shfl_xor(best.ok ? 1 : 0, o) != 0;
    if (search_before(other, best)) best = other;
  }
  if (lane == 0) {
    const double nand = (double)__builtin_nanf("");
    const SearchKey zero = search_key(row[search_index(0, 0, g.rx, g.ry)], search_count(g.hl, g.wl, 0, 0), nmin, 0, 0);
    const int dx = best.ok ? best.dx : 0, dy = best.ok ? best.dy : 0;
    shift[p * 2] = dx;
    shift[p * 2 + 1] = dy;
    found[p] = best.ok ? 1 : 0;
    float m[9];
    search_m0(f, W, H, dx, dy, m);
#pragma unroll
    for (int k = 0; k < 9; ++k) m0[(long)p * 9 + k] = m[k];
    sstats[(long)p * 3] = best.ok ? best.mean : nand;
    sstats[(long)p * 3 + 1] = (best.ok && zero.ok) ? zero.mean : nand;
    sstats[(long)p * 3 + 2] = best.ok ? search_count(g.hl, g.wl, dx, dy) : 0.0;
  }
}

}  // namespace

extern "C" int64_t sfh_track_search_workspace_bytes(int pairs, int rx, int ry) {
  if (pairs < 1 || pairs > 65535 || !search_radii_ok(rx, ry)) return -1;
  return (int64_t)pairs * search_candidates(rx, ry) * (int64_t)sizeof(double);
}

extern "C" int sfh_track_search(const float* planes, int nframes, const int32_t* ia, const int32_t* ib, int pairs, int H, int W,
                                int f, int rx, int ry, double delta, double nmin, void* workspace, long long workspace_bytes,
                                int32_t* shift, int32_t* found, float* m0, double* sstats, void* stream) {
  const char* who = "track_search";
  SFH_REQUIRE(planes && ia && ib && shift && found && m0 && sstats, "%s: null pointer", who);
  SFH_REQUIRE(nframes > 0 && H > 0 && W > 0, "%s: bad geometry frames=%d H=%d W=%d", who, nframes, H, W);
  SFH_REQUIRE(pairs >= 1 && pairs <= 65535, "%s: %d pairs (1..65535)", who, pairs);
  SFH_REQUIRE(track_level_ok(f, H) && track_level_ok(f, W), "%s: level %d (1..16) does not divide the frame %dx%d", who, f, W, H);
  SearchGeom g;
  g.hl = H / f;
  g.wl = W / f;
  g.nframes = nframes;
  SFH_REQUIRE(g.hl >= 2 && g.wl >= 2, "%s: planes %dx%d (at least 2x2)", who, g.wl, g.hl);
  SFH_REQUIRE((long)nframes * g.hl * g.wl < (1L << 31), "%s: planes too large", who);
  SFH_REQUIRE(search_radii_ok(rx, ry), "%s: radius rx=%d, ry=%d (0..%d)", who, rx, ry, SEARCH_MAX_RADIUS);
  SFH_REQUIRE(delta > 0.0 && delta * delta > 0.0 && std::isfinite(delta * delta), "%s: delta=%g (> 0)", who, delta);
  SFH_REQUIRE(nmin >= 1.0, "%s: nmin=%g (>= 1)", who, nmin);
  const long long need = sfh_track_search_workspace_bytes(pairs, rx, ry);
  SFH_REQUIRE(workspace != nullptr && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who,
              workspace ? workspace_bytes : 0LL, need);
  g.rx = rx, g.ry = ry, g.ncand = search_candidates(rx, ry);
  g.d2 = delta * delta;
  const dim3 grid((unsigned)det_cdiv(g.ncand, kSearchWaves), (unsigned)pairs);
  hipLaunchKernelGGL(track_search_cost_kernel, grid, dim3(64 * kSearchWaves), 0, (hipStream_t)stream, planes, ia, ib, g,
                     (double*)workspace);
  const int rc = sfh_check_launch("track_search_cost_kernel");
  if (rc != SFH_OK) return rc;
  hipLaunchKernelGGL(track_search_choice_kernel, dim3((unsigned)pairs), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, g,
                     f, H, W, nmin, shift, found, m0, sstats);
  return sfh_check_launch("track_search_choice_kernel");
}
