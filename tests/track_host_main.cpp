// track_host_main.cpp - the host arithmetic of the inter-frame tracker run on the CPU: det_track_plan (csrc/det_core.h), the
// one plan of sfh_track_accumulate's launcher and of sfh_track_workspace_bytes, and track_axis / track_level_ok
// (csrc/track_core.h).  Built and run by tests/test_track_host.py with -fsanitize=address,undefined and -ffp-contract=off; it
// links nothing of the library.
//
//   track_host_main < QUERIES
//
// QUERIES: one per line.  "plan PAIRS H W" -> "ok slabs elems elem_bytes bytes" (bytes = -1 when refused);
// "axis F N" -> "ok k o" with k, o as the 8 hexadecimal digits of their float32 words (zeros when the level is refused).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../sports-field-homography_amd/csrc/det_core.h"
#include "../sports-field-homography_amd/csrc/track_core.h"

int main() {
  char what[16];
  while (scanf("%15s", what) == 1) {
    if (!strcmp(what, "plan")) {
      int pairs, h, w;
      if (scanf("%d %d %d", &pairs, &h, &w) != 3) return 2;
      const DetPlan p = det_track_plan(pairs, h, w);
      printf("%d %ld %ld %d %lld\n", p.ok ? 1 : 0, p.slabs, p.elems, p.elem_bytes, det_bytes(p));
    } else if (!strcmp(what, "axis")) {
      int f, n;
      if (scanf("%d %d", &f, &n) != 2) return 2;
      float k = 0.f, o = 0.f;
      const bool ok = track_level_ok(f, n);
      if (ok) track_axis(f, n, k, o);
      uint32_t wk, wo;
      memcpy(&wk, &k, 4);
      memcpy(&wo, &o, 4);
      printf("%d %08x %08x\n", ok ? 1 : 0, wk, wo);
    } else {
      fprintf(stderr, "unknown query %s\n", what);
      return 2;
    }
  }
  return 0;
}
