// conv_geom_host_main.cpp - csrc/conv_geom.h run on the host: the tile grid, the reciprocal row split and the workgroup orders
// that the forward conv kernels share.  Built and run by tests/test_conv_geom_host.py with -fsanitize=address,undefined; it
// links nothing of the library.
//
//   conv_geom_host_main orders     every order is a bijection; per order one line "NAME configurations=N failures=F"
//   conv_geom_host_main rows       the reciprocal row split; per rows_per_img one line
//                                  "rows_per_img=D max_batch=B checked=N wrong=W next_refused=0/1"
//   conv_geom_host_main grid < T   T: lines "batch H W ksize stride flat even th tw"; per line
//                                  "ok Ho Wo rows_per_img rows_total rows_magic tiles_x tiles_y ntiles" (ok: 0 = refused)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sports-field-homography_amd/csrc/conv_geom.h"

namespace {

struct Geom {   // the fields of the kernels' geometry structs
  int tiles_x, tiles_y, ntiles;
  int Ho, Wo, rows_total, rows_per_img;
  unsigned rows_magic;
};

struct Tally {
  long configurations = 0, failures = 0;
};

// over the grid cdiv(ntiles, 8) * 8 * nblk the live workgroups map one-to-one onto {tile < ntiles} x {nb < nblk}
template <class Order>
void bijection(Tally& t, int ntiles, int nblk, Order order) {
  const int grid = (ntiles + 7) / 8 * 8 * nblk;
  std::vector<char> seen((size_t)ntiles * nblk, 0);
  long live = 0;
  bool good = true;
  for (int bid = 0; bid < grid; ++bid) {
    const SfhWg w = order(bid & 7, bid >> 3);
    if (w.live != (w.tile < ntiles)) good = false;   // live says exactly that the tile exists
    if (!w.live) continue;
    if (w.tile < 0 || w.nb < 0 || w.nb >= nblk || seen[(size_t)w.tile * nblk + w.nb]) {
      good = false;
      continue;
    }
    seen[(size_t)w.tile * nblk + w.nb] = 1;
    ++live;
  }
  ++t.configurations;
  if (!good || live != (long)ntiles * nblk) ++t.failures;
}

int orders() {
  Tally general, reversed, all, one, robin, stationary;
  const int nblks[] = {1, 2, 3, 4, 8, 16, 32};
  for (int ntiles = 1; ntiles <= 200; ++ntiles) {
    const int tpx = (ntiles + 7) >> 3;
    for (int nblk : nblks) {
      for (int G = 1; G <= nblk; ++G) {
        if (nblk % G) continue;
        for (int rev = 0; rev < 2; ++rev)
          bijection(general, ntiles, nblk, [&](int x, int k) { return sfh_wg_xcd_range(x, k, ntiles, G, rev != 0); });
        // reverse_tiles: every XCD walks its own range backwards and nothing else changes
        ++reversed.configurations;
        bool same = true;
        for (int bid = 0; bid < tpx * 8 * nblk; ++bid) {
          const SfhWg f = sfh_wg_xcd_range(bid & 7, bid >> 3, ntiles, G, false), r = sfh_wg_xcd_range(bid & 7, bid >> 3, ntiles, G, true);
          const int lo = (bid & 7) * tpx;
          if (r.nb != f.nb || f.tile < lo || f.tile >= lo + tpx || r.tile != lo + (tpx - 1 - (f.tile - lo))) same = false;
        }
        if (!same) ++reversed.failures;
      }
      // the specialisations are the general form with nb_group = nblk / one cout block
      bijection(all, ntiles, nblk, [&](int x, int k) { return sfh_wg_xcd_range_all(x, k, ntiles, nblk); });
      for (int bid = 0; bid < tpx * 8 * nblk; ++bid) {
        const SfhWg a = sfh_wg_xcd_range_all(bid & 7, bid >> 3, ntiles, nblk), g = sfh_wg_xcd_range(bid & 7, bid >> 3, ntiles, nblk, false);
        if (a.tile != g.tile || a.nb != g.nb || a.live != g.live) {
          ++all.failures;
          break;
        }
      }
      if (nblk == 1)
        for (int rev = 0; rev < 2; ++rev) {
          bijection(one, ntiles, 1, [&](int x, int k) { return sfh_wg_xcd_range_one(x, k, ntiles, rev != 0); });
          for (int bid = 0; bid < tpx * 8; ++bid) {
            const SfhWg a = sfh_wg_xcd_range_one(bid & 7, bid >> 3, ntiles, rev != 0), g = sfh_wg_xcd_range(bid & 7, bid >> 3, ntiles, 1, rev != 0);
            if (a.tile != g.tile || a.nb != g.nb || a.live != g.live) {
              ++one.failures;
              break;
            }
          }
        }
      bijection(robin, ntiles, nblk, [&](int x, int k) { return sfh_wg_round_robin(x, k, ntiles, nblk); });
      if (nblk % 8 == 0) bijection(stationary, ntiles, nblk, [&](int x, int k) { return sfh_wg_weight_stationary(x, k, ntiles, nblk); });
    }
  }
  const struct { const char* name; const Tally& t; } rows[] = {{"xcd_range", general}, {"xcd_range_reverse", reversed}, {"xcd_range_all", all},
                                                               {"xcd_range_one", one}, {"round_robin", robin}, {"weight_stationary", stationary}};
  for (const auto& r : rows) printf("%s configurations=%ld failures=%ld\n", r.name, r.t.configurations, r.t.failures);
  return 0;
}

// rows_per_img = D through the fill function: a 1x1 fp32 conv (no zero rows) over frames of D rows
bool fill(Geom& g, long long batch, int D) { return batch < (1LL << 31) && sfh_conv_grid(g, (int)batch, D, 1, 1, 1, true, false, 8, 32); }

int rows() {
  const int ds[] = {1, 2, 3, 8, 17, 46, 182, 362, 722, 65535};
  for (int D : ds) {
    Geom g;
    long long lo = 0, hi = 1LL << 32;   // the guard is monotone in the batch: lo admitted (or 0), hi refused
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (fill(g, mid, D)) lo = mid;
      else hi = mid;
    }
    long checked = 0, wrong = 0;
    if (lo >= 1 && fill(g, lo, D)) {
      auto check = [&](long long r) {
        if (r < 0 || r > (long long)g.rows_total + 63) return;
        int b, y;
        const bool out_row = sfh_row_split(g, (int)r, b, y);
        ++checked;
        if (b != (int)(r / D) || y != (int)(r % D) || out_row != (r < g.rows_total && y < g.Ho)) ++wrong;
      };
      const long long ks[] = {0, 1, 2, lo / 2, lo};
      for (long long k : ks)
        for (int e = -1; e <= 1; ++e) check(k * D + e);
      for (long long r = (long long)g.rows_total - 64; r <= (long long)g.rows_total + 63; ++r) check(r);   // what the last tile reaches
      for (long long r = 0; r <= (long long)g.rows_total + 63; r += 1009) check(r);                     // and a sweep of the rest
    }
    Geom g2;
    printf("rows_per_img=%d max_batch=%lld checked=%ld wrong=%ld next_refused=%d\n", D, lo, checked, wrong, fill(g2, lo + 1, D) ? 0 : 1);
  }
  return 0;
}

int grid() {
  int batch, H, W, ksize, stride, flat, even, th, tw;
  while (scanf("%d %d %d %d %d %d %d %d %d", &batch, &H, &W, &ksize, &stride, &flat, &even, &th, &tw) == 9) {
    Geom g;
    memset(&g, 0, sizeof(g));
    const bool ok = sfh_conv_grid(g, batch, H, W, ksize, stride, flat != 0, even != 0, th, tw);
    printf("%d %d %d %d %d %u %d %d %d\n", ok ? 1 : 0, g.Ho, g.Wo, g.rows_per_img, g.rows_total, g.rows_magic, g.tiles_x, g.tiles_y, g.ntiles);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "orders")) return orders();
  if (argc == 2 && !strcmp(argv[1], "rows")) return rows();
  if (argc == 2 && !strcmp(argv[1], "grid")) return grid();
  fprintf(stderr, "usage: conv_geom_host_main orders | rows | grid < TABLE\n");
  return 2;
}
