// track_core.h - the host arithmetic of the inter-frame tracker (track.hip), stated once: the two numbers per axis that
// take a normalised frame coordinate back to a plane of level f.  The rule stands in include/sfh_amd.h above the sfh_track_*
// entries; tests/track_host_main.cpp runs this file on the CPU against tests/track_ref.py.
// Plain C++, no HIP header.
#pragma once

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
