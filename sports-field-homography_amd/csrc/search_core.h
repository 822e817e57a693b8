// search_core.h - the coarse shift search of the inter-frame tracker (track.hip: track_search_cost_kernel,
// track_search_choice_kernel), the parts that host and device share, stated once: the candidate order, the counted pixels of
// a shift, the per-pixel cost, the key by which a shift is chosen and the start matrix a shift stands for.  The rule stands
// in include/sfh_amd.h above sfh_track_search; tests/search_host_main.cpp runs this file on the CPU against
// tests/search_ref.py.
// Plain C++, no HIP header: SFH_TRACK_FN (track_core.h) marks what the device runs too.
#pragma once
#include "track_core.h"

#define SEARCH_MAX_RADIUS 32

// what sfh_track_search and sfh_track_search_workspace_bytes admit
inline bool search_radii_ok(int rx, int ry) { return rx >= 0 && rx <= SEARCH_MAX_RADIUS && ry >= 0 && ry <= SEARCH_MAX_RADIUS; }

// candidates (dx, dy), |dx| <= rx, |dy| <= ry, in the order c = (dy + ry) (2 rx + 1) + (dx + rx)
SFH_TRACK_FN int search_candidates(int rx, int ry) { return (2 * rx + 1) * (2 * ry + 1); }
SFH_TRACK_FN int search_index(int dx, int dy, int rx, int ry) { return (dy + ry) * (2 * rx + 1) + (dx + rx); }
SFH_TRACK_FN void search_candidate(int c, int rx, int ry, int& dx, int& dy) {
  const int w = 2 * rx + 1;
  dy = c / w - ry;
  dx = c % w - rx;
}

// current pixels (I, J) of an hl x wl plane with (I + dy, J + dx) inside it: analytic, exact as a double
SFH_TRACK_FN double search_count(int hl, int wl, int dx, int dy) {
  const int ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx;
  const int rows = hl - ay > 0 ? hl - ay : 0, cols = wl - ax > 0 ? wl - ax : 0;
  return (double)rows * (double)cols;
}

// the accumulate kernel's Geman-McClure cost of one pixel, operation for operation
SFH_TRACK_FN double search_rho(float prev, float cur, double d2) {
  const double r = (double)prev - (double)cur;
  const double r2 = r * r;
  const double c = 1.0 + r2 / d2;
  const double ic = 1.0 / c;
  return r2 * ic;
}

// a candidate as the choice sees it; ok = admissible
struct SearchKey {
  double mean;
  int dx, dy;
  bool ok;
};
SFH_TRACK_FN SearchKey search_key(double mean, double n, double nmin, int dx, int dy) {
  SearchKey k;
  k.mean = mean, k.dx = dx, k.dy = dy;
  k.ok = n >= nmin && track_finite(mean);
  return k;
}
// a before b: an admissible key before an inadmissible one, then (mean, dx dx + dy dy, dy, dx) lexicographically
SFH_TRACK_FN bool search_before(const SearchKey& a, const SearchKey& b) {
  if (!a.ok || !b.ok) return a.ok && !b.ok;
  if (a.mean != b.mean) return a.mean < b.mean;
  const int da = a.dx * a.dx + a.dy * a.dy, db = b.dx * b.dx + b.dy * b.dy;
  if (da != db) return da < db;
  if (a.dy != b.dy) return a.dy < b.dy;
  return a.dx < b.dx;
}

// the start a shift stands for: under it sfh_track_accumulate's px is J + dx up to rounding.  d 2 f is an exact integer
// product, one fp64 division, one rounding to fp32.
SFH_TRACK_FN float search_offset(int d, int f, int n) { return (float)((double)(d * 2 * f) / (double)(n - 1)); }
SFH_TRACK_FN void search_m0(int f, int W, int H, int dx, int dy, float* m) {
  m[0] = 1.0f, m[1] = 0.0f, m[2] = search_offset(dx, f, W);
  m[3] = 0.0f, m[4] = 1.0f, m[5] = search_offset(dy, f, H);
  m[6] = 0.0f, m[7] = 0.0f, m[8] = 1.0f;
}
