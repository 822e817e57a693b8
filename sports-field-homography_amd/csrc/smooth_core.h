// smooth_core.h - the per-lane arithmetic of the motion-compensated temporal smoothing of theta (track_smooth_kernel,
// track.hip), stated once for host and device: which frames are members of a window, what a member sees of the control points,
// the two weights, and the refit of a homography to the combined points.  The rule stands in include/sfh_amd.h above
// sfh_track_smooth; what is NOT here is the sum across the lanes of a wave (wave_sum_all, common.h).  tests/smooth_ref.py
// restates it in numpy; tests/smooth_host_main.cpp runs this file on the CPU against that restatement, bit for bit.
// Plain C++, no HIP header.
#pragma once
#include "chol8.h"
#include "track_core.h"

#define SMOOTH_MAX_RADIUS 31

// frame k can be a member of frame t's window: inside the clip, GOOD, and every link between k and t non-zero
// (link[k+1 .. t] for a back member, link[t+1 .. k] for a forward one)
SFH_TRACK_FN bool smooth_linked(const float* __restrict__ theta, const float* __restrict__ score, float max_score,
                                const int32_t* __restrict__ link, int frames, int k, int t) {
  if (k < 0 || k >= frames || !frame_good(theta, score, max_score, k)) return false;
  const int lo = k < t ? k : t, hi = k < t ? t : k;
  for (int j = lo + 1; j <= hi; ++j)
    if (link[j] == 0) return false;
  return true;
}

// theta_k seen from frame t, by the chains of track_propagate_kernel.  Back (k < t): P = theta_k, then P = P M_j, j = k+1 .. t
// ascending.  Forward (k > t): P = theta_k, then P = P adj(M_j), j = k .. t+1 descending.  k == t: theta_t itself.  P is not
// normalised.
SFH_TRACK_FN void smooth_chain(const float* __restrict__ theta, const float* __restrict__ M, int k, int t, M3& P) {
  load3(theta + (long)k * 9, P);
  for (int j = k + 1; j <= t; ++j) {
    M3 m;
    load3(M + (long)j * 9, m);
    mul3(P, m);
  }
  for (int j = k; j >= t + 1; --j) {
    M3 m, a;
    load3(M + (long)j * 9, m);
    adj3(m, a);
    mul3(P, a);
  }
}

// the four control points (x, y, 1) under P, in()'s expressions with c = 1 (P2 c is P2 exactly): q = (X / W, Y / W) per point.
// false unless all eight are finite and the four W are non-zero and of one sign
SFH_TRACK_FN bool smooth_project(const M3& P, const float* ctrl, double (&q)[8]) {
  bool fin = true;
  int pos = 0, neg = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double x = (double)ctrl[2 * c], y = (double)ctrl[2 * c + 1];
    const double X = (P.v[0] * x + P.v[1] * y) + P.v[2];
    const double Y = (P.v[3] * x + P.v[4] * y) + P.v[5];
    const double W = (P.v[6] * x + P.v[7] * y) + P.v[8];
    q[2 * c] = X / W;
    q[2 * c + 1] = Y / W;
    fin = fin && track_finite(q[2 * c]) && track_finite(q[2 * c + 1]);
    pos += W > 0.0 ? 1 : 0;
    neg += W < 0.0 ? 1 : 0;
  }
  return fin && (pos == 4 || neg == 4);
}

// the temporal weight of a member at distance dist <= R on a side of radius R: a triangle that reaches 0 at R + 1
SFH_TRACK_FN double smooth_triangle(int R, int dist) { return (double)(R + 1 - dist) / (double)(R + 1); }

// the eight squared components of q - c, added in index order
SFH_TRACK_FN double smooth_r2(const double (&q)[8], const double (&c)[8]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double e = q[i] - c[i];
    s += e * e;
  }
  return s;
}

// sfh_track_accumulate's Geman-McClure weight
SFH_TRACK_FN double smooth_omega(double r2, double d2) {
  const double ic = 1.0 / (1.0 + r2 / d2);
  return ic * ic;
}

// the homography h (h8 = 1) that takes the control points to c.  Rows of A h = b: 2p = [x y 1 0 0 0 -ux -uy | u], 2p + 1 =
// [0 0 0 x y 1 -vx -vy | v] for point p = 0..3 with (u, v) = (c[2p], c[2p+1]).  N = A^T A and g = A^T b, each entry a sum over the
// rows r = 0..7 ascending from +0.0, every product rounded; N h = g by chol8_solve.  ok carries the caller's precondition in.
SFH_TRACK_FN bool smooth_refit(const float* ctrl, const double (&c)[8], double (&h)[8], bool ok) {
  double A[8][8], b[8];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const double x = (double)ctrl[2 * p], y = (double)ctrl[2 * p + 1], u = c[2 * p], v = c[2 * p + 1];
    const double ru[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y)};
    const double rv[8] = {0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y)};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      A[2 * p][j] = ru[j];
      A[2 * p + 1][j] = rv[j];
    }
    b[2 * p] = u;
    b[2 * p + 1] = v;
  }
  double N[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 8; ++r) s += A[r][i] * A[r][j];
      N[i][j] = s;
    }
#pragma unroll
    for (int j = i + 1; j < 8; ++j) N[i][j] = 0.0;   // not read by the solve
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) s += A[r][i] * b[r];
    h[i] = s;
  }
  return chol8_solve(N, h, ok);
}
