// uvfit.hip - homography fit from the UV head: the dense frame -> court correspondences the head regresses (or a label holds)
// are fitted by iteratively reweighted least squares, one linear 8 x 8 solve per pass.  The rule (gate, coordinates, residual,
// weight, the 27 sums, the assembly, the step) is stated once in include/sfh_amd.h above the sfh_uvfit_* entries;
// tests/uvfit_ref.py restates it in numpy.
//
// * uvfit_accumulate_kernel: a workgroup covers 64 columns x 64 rows of the h x w grid (a wave 64 x 16, a lane one column: a
//   wave's load of a row is 256 contiguous bytes of every plane it reads, at any w and any alignment - no wide loads, which
//   an odd w would misalign on every second row).  Everything behind the fp32 loads and the fp32 pixel centre is fp64.  The 27
//   sums are reduced by wave shuffle, then across the four waves through LDS, and stored once into the workgroup's slab: the
//   store pass of det_core.h, as refine_accumulate_kernel does it.  No atomics, no workgroup waits for another.
// * uvfit_step_kernel: one wave per frame; lanes 0..26 take the ascending chain over the slabs (det_sum), every lane then holds
//   all 27 sums, assembles the 8 x 8 system and solves it redundantly in registers (chol8_solve, chol8.h).
#include "common.h"
#include "det_core.h"
#include "chol8.h"

namespace {

constexpr int kSums = SFH_UVFIT_SUMS;
constexpr int kTile = DET_FIT_TILE, kWaveRows = 16;   // a workgroup's 64 x 64 pixels, four waves of 64 x 16

template <bool HAS_THETA, bool HAS_LOGITS>
__global__ __launch_bounds__(256) void uvfit_accumulate_kernel(const float* __restrict__ uv, const float* __restrict__ logits, int nc,
                                                               const float* __restrict__ theta, int h, int w, float ax, float cx0,
                                                               float ay, float cy0, double half_wt, double half_ht, float u_min,
                                                               float v_min, double kx, double ky, double delta,
                                                               double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.z;
  const int j = blockIdx.x * kTile + lane;
  const long plane = (long)h * w;
  double t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = HAS_THETA ? (double)theta[b * 9 + k] : 0.0;
  const double d2 = delta * delta;
  double acc[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
  if (j < w) {
    const double x = (double)__builtin_fmaf(ax, (float)j, cx0);
    // the wave's 16 rows of u and v are loaded before any of them is used: 32 independent loads in flight per lane in place
    // of 16 dependent round trips (a row outside the grid reads nothing and holds 0, which the gate refuses); the rows are
    // still ADDED in ascending order
    const int i0 = blockIdx.y * kTile + wv * kWaveRows;
    float ur[kWaveRows], vr[kWaveRows];
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
      const bool in = i0 + r < h;
      const long pix = (long)(in ? i0 + r : 0) * w + j;
      ur[r] = in ? uv[(long)b * 2 * plane + pix] : 0.f;
      vr[r] = in ? uv[((long)b * 2 + 1) * plane + pix] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
      const int i = i0 + r;
      if (i >= h) break;
      const long pix = (long)i * w + j;
      const float u = ur[r], v = vr[r];
      bool gate = u > u_min && v > v_min;   // a NaN fails
      if (HAS_LOGITS) {
        const float* lg = logits + (long)b * nc * plane + pix;
        int best = 0;
        float lb = lg[0];
        for (int k = 1; k < nc; ++k) {
          const float lk = lg[(long)k * plane];
          if (lk > lb) { lb = lk; best = k; }
        }
        gate = gate && best != 0;
      }
      if (!gate) continue;
      const double y = (double)__builtin_fmaf(ay, (float)i, cy0);
      const double cx = 2.0 * (double)u - kx, cy = 2.0 * (double)v - ky;
      double om = 1.0;
      if (HAS_THETA) {
        const double X = (t[0] * x + t[1] * y) + t[2], Y = (t[3] * x + t[4] * y) + t[5], Wd = (t[6] * x + t[7] * y) + t[8];
        const double ex = (X / Wd - cx) * half_wt, ey = (Y / Wd - cy) * half_ht;
        const double r2 = ex * ex + ey * ey;
        const double c = 1.0 + r2 / d2;
        const bool live = fabs(Wd) > 1e-8 && fabs(r2) <= 1.79769313486231570815e308;   // r2 finite; false for a NaN
        om = live ? (1.0 / c) / (Wd * Wd) : 0.0;
        if (r2 <= d2) acc[25] += 1.0;
        if (om != 0.0) acc[26] += r2 / c;
      }
      acc[24] += 1.0;
      if (om == 0.0) continue;              // adds nothing to the moments
      const double wx = om * x, wy = om * y;
      const double m[6] = {wx * x, wx * y, wy * y, wx, wy, om};
      const double q = cx * cx + cy * cy;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc[e] += m[e];
#pragma unroll
      for (int e = 0; e < 5; ++e) acc[6 + e] += cx * m[e];
#pragma unroll
      for (int e = 0; e < 5; ++e) acc[11 + e] += cy * m[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[16 + e] += q * m[e];
      acc[19] += om * cx;
      acc[20] += om * cy;
      acc[21] += q * wx;
      acc[22] += q * wy;
      acc[23] += om * q;
    }
  }
  __shared__ double sh[4][kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) {
    double s = acc[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) sh[wv][e] = s;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const int e = threadIdx.x;
    const long slab = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[det_slab_offset(slab, (long)kSums * gridDim.z) + (long)b * kSums + e] = ((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e];
  }
}

__global__ __launch_bounds__(64) void uvfit_step_kernel(const double* __restrict__ partial, long slabs, int batch, int pass, int last,
                                                        const float* theta_eval, float* theta_next, int32_t* status,
                                                        double* __restrict__ stats) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const double mine = lane < kSums ? det_sum(0.0, partial, slabs, (long)kSums * batch, (long)b * kSums + lane) : 0.0;
  double S[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) S[e] = __shfl(mine, e);
  const int solved = pass > 0 ? status[b] : 0;
  const bool dead = solved < pass;
  float te[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) te[k] = theta_eval ? theta_eval[b * 9 + k] : __builtin_nanf("");

  // the assembly of include/sfh_amd.h: A = sum w (r1^T r1 + r2^T r2), g = sum w (r1 cx + r2 cy)
  double A[8][8], g[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) A[i][k] = 0.0;
  const double P[3][3] = {{S[0], S[1], S[3]}, {S[1], S[2], S[4]}, {S[3], S[4], S[5]}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) A[i][k] = A[3 + i][3 + k] = P[i][k];
  A[0][6] = -S[6];  A[1][6] = -S[7];  A[2][6] = -S[9];
  A[0][7] = -S[7];  A[1][7] = -S[8];  A[2][7] = -S[10];
  A[3][6] = -S[11]; A[4][6] = -S[12]; A[5][6] = -S[14];
  A[3][7] = -S[12]; A[4][7] = -S[13]; A[5][7] = -S[15];
  A[6][6] = S[16];  A[6][7] = S[17];  A[7][7] = S[18];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int k = 0; k < i; ++k) A[i][k] = A[k][i];
  g[0] = S[9]; g[1] = S[10]; g[2] = S[19]; g[3] = S[14]; g[4] = S[15]; g[5] = S[20]; g[6] = -S[21]; g[7] = -S[22];

  bool ok = !dead && !last && S[24] >= 4.0;
#pragma unroll
  for (int e = 0; e < kSums; ++e) ok = ok && fabs(S[e]) <= 1.79769313486231570815e308;
  // A hv = g by chol8.h (A itself is read again below); a pivot that is not positive fails the solve
  double Lm[8][8], hv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hv[i] = g[i];
#pragma unroll
    for (int k = 0; k <= i; ++k) Lm[i][k] = A[i][k];
  }
  ok = chol8_solve(Lm, hv, ok);
  float tn[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) tn[k] = ok ? (k < 8 ? (float)hv[k] : 1.0f) : te[k];
  // the algebraic cost of what is written: h^T A h - 2 h^T g + S23, h = the first eight entries of theta_next
  double quad = 0.0, lin = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    double row = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) row += A[i][k] * (double)tn[k];
    quad += (double)tn[i] * row;
    lin += (double)tn[i] * g[i];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) theta_next[b * 9 + k] = tn[k];
    status[b] = solved + (ok ? 1 : 0);
    stats[b * 4 + 0] = S[24];
    stats[b * 4 + 1] = S[25];
    stats[b * 4 + 2] = sqrt(S[26] / S[24]);
    stats[b * 4 + 3] = (quad - 2.0 * lin) + S[23];
  }
}

// what accumulate, the size query and the step's caller agree on: the slab grid of an h x w grid
// (det_uvfit_plan, det_core.h)
static_assert(kSums == DET_UVFIT_SUMS, "uvfit sums");

}  // namespace

extern "C" int64_t sfh_uvfit_workspace_bytes(int batch, int h, int w) { return det_bytes(det_uvfit_plan(batch, h, w)); }

extern "C" int sfh_uvfit_accumulate(const float* uv, const float* logits, int nc, const float* theta, int batch, int h, int w, int H,
                                    int W, int wt, int ht, float u_min, float v_min, double kx, double ky, double delta,
                                    void* workspace, long long workspace_bytes, void* stream) {
  const char* who = "uvfit_accumulate";
  SFH_REQUIRE(uv, "%s: null pointer", who);
  SFH_REQUIRE(!logits || (nc >= 2 && nc <= 8), "%s: nc=%d (2..8)", who, nc);
  SFH_REQUIRE(h >= 2 && w >= 2 && H >= 2 && W >= 2 && wt >= 2 && ht >= 2, "%s: bad geometry h=%d w=%d H=%d W=%d wt=%d ht=%d", who, h,
              w, H, W, wt, ht);
  SFH_REQUIRE(delta > 0.0, "%s: delta=%g (> 0)", who, delta);
  const DetPlan p = det_uvfit_plan(batch, h, w);
  SFH_REQUIRE(p.ok, "%s: batch %d (1..65535), or more than 65535 tile rows (h=%d)", who, batch, h);
  SFH_REQUIRE((long)h * w < (1L << 31), "%s: %d x %d pixels: too large", who, w, h);
  SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  float a[2], c[2];
  if (sfh_refine_axis(1, W, w, a) != SFH_OK || sfh_refine_axis(1, H, h, c) != SFH_OK) return SFH_E_ARG;
  const dim3 grid((unsigned)det_cdiv(w, kTile), (unsigned)det_cdiv(h, kTile), (unsigned)batch);
#define SFH_UVFIT_LAUNCH(T, L)                                                                                                  \
  hipLaunchKernelGGL((uvfit_accumulate_kernel<T, L>), grid, dim3(256), 0, (hipStream_t)stream, uv, logits, nc, theta, h, w, a[0], \
                     a[1], c[0], c[1], 0.5 * wt, 0.5 * ht, u_min, v_min, kx, ky, delta, (double*)workspace)
  if (theta && logits) SFH_UVFIT_LAUNCH(true, true);
  else if (theta) SFH_UVFIT_LAUNCH(true, false);
  else if (logits) SFH_UVFIT_LAUNCH(false, true);
  else SFH_UVFIT_LAUNCH(false, false);
#undef SFH_UVFIT_LAUNCH
  return sfh_check_launch("uvfit_accumulate_kernel");
}

extern "C" int sfh_uvfit_step(const double* partial, int64_t slabs, int batch, int pass, int last, const float* theta_eval,
                              float* theta_next, int32_t* status, double* stats, void* stream) {
  SFH_REQUIRE(partial && theta_next && status && stats, "uvfit_step: null pointer");
  SFH_REQUIRE(theta_eval || (pass == 0 && !last), "uvfit_step: no theta_eval on pass %d%s (only the first pass has none)", pass,
              last ? ", the last" : "");
  SFH_REQUIRE(slabs >= 1 && batch > 0 && batch <= 65535 && pass >= 0, "uvfit_step: bad geometry slabs=%lld batch=%d pass=%d",
              (long long)slabs, batch, pass);
  hipLaunchKernelGGL(uvfit_step_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, partial, (long)slabs, batch, pass,
                     last, theta_eval, theta_next, status, stats);
  return sfh_check_launch("uvfit_step_kernel");
}
