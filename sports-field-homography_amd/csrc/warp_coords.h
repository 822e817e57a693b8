// warp_coords.h - the pinned fp32 coordinate arithmetic of the homography warp, shared by every kernel that must land on
// the same template tap as Reconstructor.warp() (warp.hip, prepare.hip, mapping.hip).  Every operation is individually rounded, in the
// order of oracle/warp_ref.py; the translation units that include this are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace {

struct Homog {
  float t[9];
};

__device__ __forceinline__ void apply_h(const Homog& H, float x, float y, float& u, float& v) {
  const float X = __fadd_rn(__fadd_rn(__fmul_rn(H.t[0], x), __fmul_rn(H.t[1], y)), H.t[2]);
  const float Y = __fadd_rn(__fadd_rn(__fmul_rn(H.t[3], x), __fmul_rn(H.t[4], y)), H.t[5]);
  const float Z = __fadd_rn(__fadd_rn(__fmul_rn(H.t[6], x), __fmul_rn(H.t[7], y)), H.t[8]);
  const float s = (fabsf(Z) > 1e-8f) ? __fdiv_rn(1.0f, __fadd_rn(Z, 1e-8f)) : 1.0f;
  u = __fmul_rn(s, X);
  v = __fmul_rn(s, Y);
}

// inverse(theta) in fp64: adjugate times the reciprocal of the determinant, every operation individually rounded, each
// entry rounded once to fp32 (transform_poi's court -> frame matrix; sfh_theta_invert).  Returns the determinant.
__device__ __forceinline__ double inverse_h33(const float* __restrict__ theta, Homog& Hi) {
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = (double)theta[k];
  const double c00 = m[4] * m[8] - m[5] * m[7];
  const double c01 = m[5] * m[6] - m[3] * m[8];
  const double c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  const double id = 1.0 / det;
  Hi.t[0] = (float)(c00 * id);
  Hi.t[1] = (float)((m[2] * m[7] - m[1] * m[8]) * id);
  Hi.t[2] = (float)((m[1] * m[5] - m[2] * m[4]) * id);
  Hi.t[3] = (float)(c01 * id);
  Hi.t[4] = (float)((m[0] * m[8] - m[2] * m[6]) * id);
  Hi.t[5] = (float)((m[2] * m[3] - m[0] * m[5]) * id);
  Hi.t[6] = (float)(c02 * id);
  Hi.t[7] = (float)((m[1] * m[6] - m[0] * m[7]) * id);
  Hi.t[8] = (float)((m[0] * m[4] - m[1] * m[3]) * id);
  return det;
}

__device__ __forceinline__ float norm_axis(int i, int n) {
  // create_meshgrid: (i/(n-1) - 0.5) * 2
  return __fmul_rn(__fsub_rn(__fdiv_rn((float)i, (float)(n - 1)), 0.5f), 2.0f);
}

__device__ __forceinline__ float unnorm(float c, int size) {
  // ATen CPU grid sampler, align_corners=False: fma(fl(c + 1), size/2, -0.5) - the rounding
  // that reproduces torch's F.grid_sample bit for bit (see oracle/warp_ref.py:unnormalize).
  return __builtin_fmaf(__fadd_rn(c, 1.0f), 0.5f * (float)size, -0.5f);
}

// LEVEL 0: IEEE divisions (any theta); 1: fast reciprocal; 2: fast reciprocal and |Z| > 1e-8 everywhere
template <int LEVEL>
__device__ __forceinline__ float recip_rn(float z) {
  if (LEVEL == 0) return __fdiv_rn(1.0f, z);
  // caller guarantees |z| <= 2^60 (a tiny or zero z gives a result the caller discards)
  float r = __builtin_amdgcn_rcpf(z);
  float e = __builtin_fmaf(-z, r, 1.0f);
  r = __builtin_fmaf(e, r, r);
  e = __builtin_fmaf(-z, r, 1.0f);
  return __builtin_fmaf(e, r, r);
}

// i / d for integral 0 <= i <= d < 2^14, rd = __fdiv_rn(1, d)
__device__ __forceinline__ float div_small(float i, float d, float rd) {
  const float q0 = __fmul_rn(i, rd);
  return __builtin_fmaf(__builtin_fmaf(-q0, d, i), rd, q0);
}

template <bool SMALL>
__device__ __forceinline__ float norm_axis2(int i, int n, float rd) {
  const float q = SMALL ? div_small((float)i, (float)(n - 1), rd) : __fdiv_rn((float)i, (float)(n - 1));
  return __fmul_rn(__fsub_rn(q, 0.5f), 2.0f);
}

__device__ __forceinline__ float tap_ld(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0));
}

constexpr unsigned kTapOOB = 0xFFFFFFFCu;   // beyond any descriptor's num_records: the load returns 0

// rx, ry integral-valued floats -> byte offset of the tap or kTapOOB.  LEVEL 0 tolerates NaN / inf.
template <int LEVEL>
__device__ __forceinline__ unsigned tap_off(float rx, float ry, int wt, int ht) {
  if (LEVEL == 0) {
    const bool ok = (rx >= 0.f) & (rx <= (float)(wt - 1)) & (ry >= 0.f) & (ry <= (float)(ht - 1));
    const float fi = __builtin_fmaf(ry, (float)wt, rx);             // exact: < 2^24 (checked by the launcher)
    return ok ? ((unsigned)(int)fi << 2) : kTapOOB;
  }
  // finite coordinates: v_cvt_i32_f32 saturates, one unsigned compare per axis
  const int ix = (int)rx, iy = (int)ry;
  const bool ok = ((unsigned)ix < (unsigned)wt) & ((unsigned)iy < (unsigned)ht);
  return ok ? (__umul24((unsigned)iy, (unsigned)wt) + (unsigned)ix) << 2 : kTapOOB;   // valid => iy, wt < 2^24
}

// wave-uniform classification of theta (|xn|, |yn| <= 1 on the whole frame): fin = every entry small enough for the fast
// reciprocal, live = |Z| > 1e-8 on the whole frame (the select between 1/(Z + 1e-8) and 1 disappears)
__device__ __forceinline__ void theta_class(const float (&t)[9], bool& fin, bool& live) {
  fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) fin &= fabsf(t[k]) <= 0x1p59f;      // false for NaN
  const float zs = fabsf(t[6]) + fabsf(t[7]) + fabsf(t[8]);
  live = (fabsf(t[8]) - fabsf(t[6]) - fabsf(t[7])) > 1e-6f * zs + 1e-7f;
}

// rx, ry integral-valued floats -> tap column and row, ok = inside the wt x ht template.  The validity rule of tap_off.
template <int LEVEL>
__device__ __forceinline__ bool tap_xy(float rx, float ry, int wt, int ht, int& ix, int& iy) {
  if (LEVEL == 0) {
    const bool ok = (rx >= 0.f) & (rx <= (float)(wt - 1)) & (ry >= 0.f) & (ry <= (float)(ht - 1));
    ix = ok ? (int)rx : 0;
    iy = ok ? (int)ry : 0;
    return ok;
  }
  ix = (int)rx;
  iy = (int)ry;
  return ((unsigned)ix < (unsigned)wt) & ((unsigned)iy < (unsigned)ht);
}

}  // namespace
