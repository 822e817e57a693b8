// track_core.h - the arithmetic of the inter-frame tracker (track.hip) that host and device share, stated once: the two
// numbers per axis that take a normalised frame coordinate back to a plane of level f, and the 3 x 3 fp64 matrices of the
// rule that carries theta across a clip (adjugate, product, the GOOD rule).  The rule stands in
// include/sfh_amd.h above the sfh_track_* entries; tests/track_host_main.cpp and tests/smooth_host_main.cpp run this file on
// the CPU against tests/track_ref.py and tests/smooth_ref.py.
// Plain C++, no HIP header: SFH_TRACK_FN marks what the device runs too.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SFH_TRACK_FN __host__ __device__ __forceinline__
#else
#define SFH_TRACK_FN inline
#endif

// px = fmaf(u + 1, k, -o) is the column of the level-f plane under the normalised coordinate u of a frame n pixels wide:
// full-resolution pixel j sits at u = 2 j / (n - 1) - 1 and plane column J is centred on pixel f J + (f - 1) / 2, so
// k = (n - 1) / (2 f) and o = (f - 1) / (2 f), both evaluated in fp64 and rounded once to fp32.
inline void track_axis(int f, int n, float& k, float& o) {
  k = (float)((double)(n - 1) / (2.0 * f));
  o = (float)((double)(f - 1) / (2.0 * f));
}
// what sfh_track_axis and the launchers admit: a level in 1..16 that divides the axis (that an alignment needs planes of at
// least 2 x 2 pixels is det_track_plan's rule)
inline bool track_level_ok(int f, int n) { return f >= 1 && f <= 16 && n >= f && n % f == 0; }

// ------------------------------------------------------------------ carrying theta: sfh_track_propagate, sfh_track_smooth
struct M3 {
  double v[9];
};

SFH_TRACK_FN bool track_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for a NaN

SFH_TRACK_FN void load3(const float* __restrict__ t, M3& m) {
#pragma unroll
  for (int k = 0; k < 9; ++k) m.v[k] = (double)t[k];
}
// the nine expressions stated above sfh_metrics_region; returns det
SFH_TRACK_FN double adj3(const M3& m, M3& a) {
  const double* t = m.v;
  a.v[0] = t[4] * t[8] - t[5] * t[7];
  a.v[1] = t[2] * t[7] - t[1] * t[8];
  a.v[2] = t[1] * t[5] - t[2] * t[4];
  a.v[3] = t[5] * t[6] - t[3] * t[8];
  a.v[4] = t[0] * t[8] - t[2] * t[6];
  a.v[5] = t[2] * t[3] - t[0] * t[5];
  a.v[6] = t[3] * t[7] - t[4] * t[6];
  a.v[7] = t[1] * t[6] - t[0] * t[7];
  a.v[8] = t[0] * t[4] - t[1] * t[3];
  return (t[0] * a.v[0] + t[1] * a.v[3]) + t[2] * a.v[6];
}
SFH_TRACK_FN void mul3(M3& P, const M3& m) {
  M3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.v[i * 3 + j] = (P.v[i * 3] * m.v[j] + P.v[i * 3 + 1] * m.v[3 + j]) + P.v[i * 3 + 2] * m.v[6 + j];
  P = o;
}
SFH_TRACK_FN bool frame_good(const float* __restrict__ theta, const float* __restrict__ score, float max_score, int t) {
  M3 m, a;
  load3(theta + (long)t * 9, m);
  const double det = adj3(m, a);
  const bool usable = fabs(det) > 0.0 && track_finite(det);
  return usable && (score == nullptr || score[t] <= max_score);   // a NaN score fails
}
