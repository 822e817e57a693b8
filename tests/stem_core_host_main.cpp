// Stand-alone host program over csrc/stem_core.h (the index arithmetic of the tap-packed stem kernels, csrc/stem.hip): walks
// every index the two instances make and prints "OK" or the first violation.  Built with AddressSanitizer and UBSan by
// tests/test_classes_host.py (tests/host_program.py), so an index outside a table is caught twice.
//
//   1. (step, lane, j) -> (tap, channel): distinct, inside 49 x CH or padding, and every (tap, channel) owned exactly once
//      per output-channel row; the packed-weight index is a bijection onto [0, st_packed_elems).
//   2. every halo offset of every step stays inside the staged halo for every pixel of the tile (the last one included), is
//      the pixel (2 oy + ky, 2 ox + kx) for a real tap, and its LDS element lies inside the instance's LDS bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../sports-field-homography_amd/csrc/stem_core.h"

static int fail(const char* what, int ch, int a, int b, int c) {
  std::printf("FAIL CH=%d %s (%d, %d, %d)\n", ch, what, a, b, c);
  return 1;
}

static int check_instance(int ch) {
  if (!st_ch_ok(ch)) return fail("st_ch_ok", ch, 0, 0, 0);
  const int nstep = st_nstep(ch);
  if (nstep != (ch == 8 ? 13 : 25)) return fail("st_nstep", ch, nstep, 0, 0);
  // ---- 1. the (step, lane, j) -> (tap, channel) map
  std::vector<int> owners(ST_TAPS * ch * 16, 0);   // [cout row lane & 15][tap][channel]
  for (int s = 0; s < nstep; ++s)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int lg = lane >> 4, t = st_tap(ch, s, lg), c = st_chan0(ch, lg) + j;
        if (t < 0 || c < 0 || c >= ch) return fail("tap / channel out of range", ch, s, lane, j);
        if (t >= ST_TAPS) {
          if (s != nstep - 1) return fail("padding tap before the last step", ch, s, lane, j);
          continue;
        }
        owners.at(((lane & 15) * ST_TAPS + t) * ch + c) += 1;
      }
  for (size_t i = 0; i < owners.size(); ++i)
    if (owners[i] != 1) return fail("(tap, channel) not owned exactly once", ch, (int)i, owners[i], 0);
  for (int np = 2; np <= 3; ++np) {
    const long n = st_packed_elems(ch, np);
    std::vector<char> seen((size_t)n, 0);
    for (int s = 0; s < nstep; ++s)
      for (int p = 0; p < np; ++p)
        for (int sub = 0; sub < 4; ++sub)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
              const long i = st_packed_index(np, s, p, sub, lane, j);
              if (i < 0 || i >= n) return fail("packed index out of range", ch, s, lane, j);
              if (seen.at((size_t)i)++) return fail("packed index used twice", ch, s, lane, j);
            }
    for (long i = 0; i < n; ++i)
      if (!seen[(size_t)i]) return fail("packed element never written", ch, (int)i, np, 0);
  }
  // ---- 2. halo offsets
  const int th = st_tile_h(ch), tw = st_tile_w(ch), hw = st_halo_w(ch), hh = st_halo_h(ch), hpix = st_halo_pixels(ch);
  if (hh != 2 * (th - 1) + 7 || hw != 2 * (tw - 1) + 7 || hpix != hh * hw || st_halo_padded(ch) < hpix ||
      st_halo_padded(ch) % 16)
    return fail("halo geometry", ch, hh, hw, hpix);
  std::vector<char> halo((size_t)hpix, 0);
  for (int oy = 0; oy < th; ++oy)
    for (int ox = 0; ox < tw; ++ox)
      for (int s = 0; s < nstep; ++s)
        for (int lg = 0; lg < 4; ++lg) {
          const int t = st_tap(ch, s, lg), off = st_pixel_off(ch, oy, ox) + st_tap_off(ch, t);
          if (off < 0 || off >= hpix) return fail("halo offset outside the staged halo", ch, oy, ox, t);
          if (t < ST_TAPS && off != (2 * oy + t / 7) * hw + 2 * ox + t % 7) return fail("halo offset is not the tap's pixel", ch, oy, ox, t);
          halo.at((size_t)off) = 1;
          for (int np = 2; np <= 3; ++np)
            for (int p = 0; p < np; ++p) {
              const int e = st_lds_elem(ch, p, st_chan0(ch, lg) >> 3, off);
              if (e < 0 || (e + 1) * 16 > st_lds_bytes(ch, np)) return fail("LDS element outside the allocation", ch, p, off, np);
            }
        }
  for (int i = 0; i < hpix; ++i)
    if (!halo[(size_t)i]) return fail("staged halo pixel never read", ch, i, 0, 0);   // the halo is exactly what the taps need
  // distinct (plane, half, pixel) -> distinct LDS elements
  for (int np = 2; np <= 3; ++np) {
    std::vector<char> el((size_t)st_lds_bytes(ch, np) / 16, 0);
    for (int p = 0; p < np; ++p)
      for (int hf = 0; hf < ch / 8; ++hf)
        for (int pix = 0; pix < hpix; ++pix)
          if (el.at((size_t)st_lds_elem(ch, p, hf, pix))++) return fail("LDS element used twice", ch, p, hf, pix);
  }
  if (!st_cs_ok(8, 8) || st_cs_ok(8, 12) || !st_cs_ok(16, 12) || !st_cs_ok(16, 16) || st_cs_ok(16, 8) || st_cs_ok(16, 20))
    return fail("st_cs_ok", ch, 0, 0, 0);
  std::printf("CH=%d steps=%d tile=%dx%d halo=%dx%d lds3=%d lds2=%d packed3=%ld\n", ch, nstep, th, tw, hh, hw,
              st_lds_bytes(ch, 3), st_lds_bytes(ch, 2), st_packed_elems(ch, 3) * 2);
  return 0;
}

int main() {
  for (int ch : {8, 16})
    if (check_instance(ch)) return 1;
  std::printf("OK\n");
  return 0;
}
