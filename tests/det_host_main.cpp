// det_host_main.cpp - the partition arithmetic of the deterministic training mode (csrc/det_core.h) walked on the host, for
// every kernel family, with the kernels' own loops and lane maps RESTATED beside it (the kernels do not call the share -> slab
// maps of det_core.h).  Slabs, elements per slab and bytes of every line come from the family's plan (det_*_plan, det_bytes):
// the function the launcher and the size query call; the slab and element offsets and the sum pass are the kernels' own too.
// Built and run by tests/test_det_host.py
// with -fsanitize=address,undefined and -ffp-contract=off; it links nothing of the library.
//
//   det_host_main walk CASES      CASES: one geometry per line,
//       wgrad M N ks x_cs xh xw pad_top pad_left B H W | wgrad_s3 M N ks B H W | grouped B H W G cg stride | red npix C |
//       colsum npix C | outconv npix nc cin | avgpool B C nout | losses npix | uv total | reproj batch | warp B h w
//     For each line: every share of the work (tile, pixel, frame) is given to exactly one slab, every slab index is below the
//     slab count, and the store pass - the kernel's lanes, each writing where the kernel writes - touches every element of the
//     R * E workspace exactly once (the workspace is a heap block of exactly R * E counters: one element too far is a
//     sanitizer report).  Prints "<line> -> slabs elems bytes"; the test compares the bytes with the size queries.
//   det_host_main sum DIR         dims.i64 = is_f64 R E ncol raw_n n_off; partial.bin (R, E); dst0.bin (E / ncol, raw_n)
//                              -> dst.bin: the sum pass (det_sum, det_dst_offset) over every element
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sports-field-homography_amd/csrc/conv_grouped_core.h"
#include "../sports-field-homography_amd/csrc/det_core.h"

static int g_fail = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");              \
      ++g_fail;                           \
    }                                     \
  } while (0)

// the workspace of one launch: R * E write counters
struct Ws {
  long R, E;
  std::vector<unsigned char> n;
  Ws(long r, long e) : R(r), E(e), n((size_t)(r * e), 0) {}
  void store(long slab, long elem) {
    CHECK(slab >= 0 && slab < R && elem >= 0 && elem < E, "store outside the workspace: slab %ld of %ld, element %ld of %ld", slab, R,
          elem, E);
    if (slab >= 0 && slab < R && elem >= 0 && elem < E) ++n.at((size_t)(det_slab_offset(slab, E) + elem));
  }
  void finish(const char* who) const {
    long bad = 0;
    for (unsigned char c : n) bad += c != 1;
    CHECK(bad == 0, "%s: %ld of %ld workspace elements not written exactly once", who, bad, R * E);
  }
};

// what every walk starts from: the family's plan (the function the launcher and the size query call), and what it prints
static bool admitted(const DetPlan& p, const char* who) {
  CHECK(p.ok && p.why == DET_OK && p.slabs >= 1 && p.elems >= 1, "%s: a case geometry is refused (rule %d)", who, (int)p.why);
  if (!p.ok) printf("0 0 -1\n");
  return p.ok;
}
static void print_plan(const DetPlan& p) { printf("%ld %ld %lld\n", p.slabs, p.elems, det_bytes(p)); }

static void once(const std::vector<int>& seen, const char* who) {
  long bad = 0;
  for (int c : seen) bad += c != 1;
  CHECK(bad == 0, "%s: %ld of %zu shares not owned by exactly one slab", who, bad, seen.size());
}

static void walk_wgrad(int M, int N, int ks, int x_cs, int xh, int xw, int pt, int pl, int B, int H, int W) {
  const DetWgradPlan p = det_wgrad_plan(M, x_cs, xh, xw, N, pt, pl, B, H, W, ks);
  if (!admitted(p, "wgrad")) return;
  const bool c4 = p.c4;
  CHECK(p.slabs == p.nsplit && p.ntiles == B * det_cdiv(H, det_tile_h(p.shape)) * det_cdiv(W, det_tile_w(p.shape)) && p.nsplit >= 1 && p.nsplit <= p.ntiles,
        "wgrad plan: %d tiles, %d splits", p.ntiles, p.nsplit);
  std::vector<int> seen((size_t)p.ntiles, 0);
  for (int s = 0; s < p.nsplit; ++s)
    for (int tile = s; tile < p.ntiles; tile += p.nsplit) {   // the kernel's loop
      CHECK(det_wgrad_slab_of_tile(tile, p.nsplit) == s, "wgrad: tile %d in split %d", tile, s);
      ++seen[(size_t)tile];
    }
  once(seen, "wgrad tiles");
  Ws ws(p.slabs, p.elems);
  const int nsub = det_wgrad_nsub(ks, N);
  for (int split = 0; split < p.nsplit; ++split)
    for (int mni = 0; mni < p.mn; ++mni)
      for (int tid = 0; tid < 256; ++tid) {
        const int lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
        if (c4) {
          const int m0 = mni * 64;
          for (int nb = 0; nb < 3; ++nb) {
            const int n = nb * 16 + l16, tap = n >> 2, c = n & 3;
            if (n >= 36 || c >= N) continue;
            for (int r = 0; r < 4; ++r) {
              const int m = m0 + wave * 16 + 4 * kq + r;
              if (m < M) ws.store(split, det_wgrad_elem(m, tap, c, 9, N));
            }
          }
          continue;
        }
        const int m0 = (mni % p.mt) * 64, n0 = (mni / p.mt) * (16 * nsub);
        for (int t = 0; t < p.kk; ++t)
          for (int s = 0; s < nsub; ++s) {
            const int n = n0 + s * 16 + l16;
            if (n >= N) continue;
            for (int r = 0; r < 4; ++r) {
              const int m = m0 + wave * 16 + 4 * kq + r;
              if (m < M) ws.store(split, det_wgrad_elem(m, t, n, p.kk, N));
            }
          }
      }
  ws.finish("wgrad");
  print_plan(p);
}

static void walk_wgrad_s3(int M, int N, int ks, int B, int H, int W) {
  const DetWgradS3Plan p = det_wgrad_s3_plan(M, N, B, H, W, ks);
  if (!admitted(p, "wgrad_s3")) return;
  CHECK(p.slabs == p.nsplit && p.nsplit >= 1 && p.tps >= 1 && (long)p.nsplit * p.tps >= p.ntiles && (long)(p.nsplit - 1) * p.tps < p.ntiles,
        "wgrad_s3 plan: %d tiles, %d splits of %d", p.ntiles, p.nsplit, p.tps);
  std::vector<int> seen((size_t)p.ntiles, 0);
  for (int s = 0; s < p.nsplit; ++s) {
    const int t_begin = s * p.tps, t_end = t_begin + p.tps < p.ntiles ? t_begin + p.tps : p.ntiles;   // the kernel's range
    for (int t = t_begin; t < t_end; ++t) {
      CHECK(det_wgrad_s3_slab_of_tile(t, p.tps) == s, "wgrad_s3: tile %d in split %d", t, s);
      ++seen[(size_t)t];
    }
  }
  once(seen, "wgrad_s3 tiles");
  Ws ws(p.slabs, p.elems);
  const int nblk = N / 32;
  for (int split = 0; split < p.nsplit; ++split)
    for (int mni = 0; mni < p.mn; ++mni)
      for (int tid = 0; tid < 256; ++tid) {
        const int lane = tid & 63, wv = tid >> 6, g = lane >> 4, nb16 = wv & 1, mh = wv >> 1;
        const int mb64 = mni / nblk, nb32 = mni % nblk;
        const int m0 = mb64 * 64 + 32 * mh + 4 * g, n = nb32 * 32 + 16 * nb16 + (lane & 15);
        for (int mb = 0; mb < 2; ++mb)
          for (int t9 = 0; t9 < p.kk; ++t9)
            for (int r = 0; r < 4; ++r) ws.store(split, det_wgrad_elem(m0 + 16 * mb + r, t9, n, p.kk, N));
      }
  ws.finish("wgrad_s3");
  print_plan(p);
}

static void walk_grouped(int B, int H, int W, int G, int cg, int s) {
  const int C = G * cg, KC = gc_chunk(cg), NCH = cg / KC, NU = 32 * (KC / 4);
  const DetPlan p = det_grouped_plan(B, H, W, G, cg, s);
  if (!admitted(p, "grouped")) return;
  const long tiles = p.slabs;
  CHECK(tiles == (long)B * det_cdiv(gc_out_size(H, s), gc_tile_h(s)) * det_cdiv(gc_out_size(W, s), GC_TW), "grouped tiles");
  Ws ws(tiles, p.elems);
  for (long tile = 0; tile < tiles; ++tile)                       // blockIdx.x = the tile = the slab
    for (int by = 0; by < det_cdiv(C, 32) * NCH; ++by) {
      const int ob = by / NCH, chunk = by % NCH;
      for (int v = 0; v < NU * 36; ++v) {
        const int uu = v / 36, k = (v % 36) / 4, j = v % 4, o = ob * 32 + uu % 32;
        if (o < C) ws.store(tile, gc_raw_index(cg, o, k, chunk * 32 + 4 * (uu / 32) + j));
      }
    }
  ws.finish("grouped");
  print_plan(p);
}

// red_tail of a block: NV / 4 rows of the quad's four channels, for every channel chunk
static void red_tail_store(Ws& ws, long block, int C, int rows, long row_stride) {
  for (int c0 = 0; c0 < C; c0 += 1024) {
    const int cq = (C - c0 < 1024 ? C - c0 : 1024) >> 2;
    for (int tid = 0; tid < cq; ++tid)
      for (int j = 0; j < 4 * rows; ++j) ws.store(block, (long)(j >> 2) * row_stride + c0 + 4 * tid + (j & 3));
  }
}

static void walk_red(long npix, int C, bool colsum) {
  const DetPlan plan = det_red_plan(npix, C, colsum ? 1 : 2);
  if (!admitted(plan, colsum ? "colsum" : "red")) return;
  const long nb = plan.slabs;
  CHECK(nb >= 1 && nb <= DET_RED_BLOCKS, "red blocks %ld", nb);
  std::vector<int> chunked((size_t)npix, 0), strided((size_t)npix, 0);
  const long chunk = det_red_chunk(npix, nb);
  const int lanes = det_red_lanes(C);
  for (long b = 0; b < nb; ++b) {
    const long pend = npix < (b + 1) * chunk ? npix : (b + 1) * chunk;       // bn_stats_kernel's range
    for (long p = b * chunk; p < pend; ++p) {
      CHECK(det_red_block_of_pixel_chunked(p, npix, nb) == b, "red: pixel %ld in block %ld", p, b);
      ++chunked[(size_t)p];
    }
    for (int plane = 0; plane < lanes; ++plane)                              // bn_bwd_reduce_kernel / colsum_kernel's stride
      for (long p = b * lanes + plane; p < npix; p += nb * lanes) {
        CHECK(det_red_block_of_pixel_strided(p, lanes, nb) == b, "red: pixel %ld in block %ld (strided)", p, b);
        ++strided[(size_t)p];
      }
  }
  once(chunked, "red pixels (chunked)");
  if (C <= 1024) once(strided, "red pixels (strided)");   // (wider tensors: the lane count changes per channel chunk)
  Ws ws(nb, plan.elems);
  for (long b = 0; b < nb; ++b) {
    if (!colsum) { red_tail_store(ws, b, C, 2, C); continue; }
    for (int q0 = 0; q0 < C / 4; q0 += 256) {                                // colsum_kernel: 256 quads per pass, one row
      const int qn = C / 4 - q0 < 256 ? C / 4 - q0 : 256;
      for (int tid = 0; tid < qn; ++tid)
        for (int j = 0; j < 4; ++j) ws.store(b, 4L * q0 + 4 * tid + j);
    }
  }
  ws.finish(colsum ? "colsum" : "red");
  print_plan(plan);
}

static void walk_outconv(long npix, int nc, int cin) {
  const DetPlan plan = det_outconv_plan(cin, nc, 1, 1, (int)npix);   // the plan reads batch * H * W
  if (!admitted(plan, "outconv")) return;
  const long ppb = det_outconv_ppb(npix), nb = plan.slabs;
  std::vector<int> seen((size_t)npix, 0);
  for (long b = 0; b < nb; ++b)
    for (long p = b * ppb; p < (npix < (b + 1) * ppb ? npix : (b + 1) * ppb); ++p) ++seen[(size_t)p];
  once(seen, "outconv pixels");
  Ws ws(nb, plan.elems);
  for (long b = 0; b < nb; ++b)
    for (int k = 0; k < nc; ++k) {
      for (int tid = 0; tid < cin / 4; ++tid)
        for (int j = 0; j < 4; ++j) ws.store(b, (long)k * cin + 4 * tid + j);
      ws.store(b, (long)nc * cin + k);
    }
  ws.finish("outconv");
  print_plan(plan);
}

static void walk_flat(const char* who, const DetPlan& p, int per_slab_rows, int row) {
  if (!admitted(p, who)) return;
  Ws ws(p.slabs, p.elems);
  for (long b = 0; b < p.slabs; ++b)
    for (int r = 0; r < per_slab_rows; ++r)
      for (int k = 0; k < row; ++k) ws.store(b, (long)r * row + k);
  ws.finish(who);
  print_plan(p);
}

static int walk(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  char fam[32];
  long a[11];
  while (fscanf(f, "%31s", fam) == 1) {
    const std::string k = fam;
    const int want = k == "wgrad" ? 11 : (k == "wgrad_s3" || k == "grouped") ? 6 : (k == "red" || k == "colsum") ? 2
                     : (k == "outconv" || k == "avgpool" || k == "warp") ? 3 : 1;
    for (int i = 0; i < want; ++i)
      if (fscanf(f, "%ld", &a[i]) != 1) { fprintf(stderr, "short line for %s\n", fam); fclose(f); return 2; }
    printf("%s", fam);
    for (int i = 0; i < want; ++i) printf(" %ld", a[i]);
    printf(" -> ");
    if (k == "wgrad") walk_wgrad((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[10]);
    else if (k == "wgrad_s3") walk_wgrad_s3((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5]);
    else if (k == "grouped") walk_grouped((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5]);
    else if (k == "red") walk_red(a[0], (int)a[1], false);
    else if (k == "colsum") walk_red(a[0], (int)a[1], true);
    else if (k == "outconv") walk_outconv(a[0], (int)a[1], (int)a[2]);
    else if (k == "avgpool") walk_flat("avgpool", det_avgpool_plan((int)a[0], (int)a[1], (int)a[2]), 1, (int)a[2] * (int)a[1] + (int)a[2]);
    else if (k == "losses") walk_flat("losses", det_losses_plan(1, 1, (int)a[0]), 1, 3);   // the plan reads batch * H * W
    else if (k == "uv") walk_flat("uv", det_uv_plan(1, 1, 1, (int)a[0]), 1, 1);           // batch * C * H * W
    else if (k == "reproj") walk_flat("reproj", det_reproj_plan((int)a[0]), 1, 1);
    else if (k == "warp") {
      const int gx = det_warp_gx((int)a[2]), gy = det_warp_gy((int)a[1]);
      std::vector<int> seen((size_t)gx * gy, 0);
      for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < gx; ++bx) ++seen.at((size_t)det_warp_slab(bx, by, gx));
      once(seen, "warp blocks");
      walk_flat("warp", det_warp_plan((int)a[0], (int)a[1], (int)a[2]), (int)a[0], 9);
    } else { fprintf(stderr, "unknown family %s\n", fam); fclose(f); return 2; }
  }
  fclose(f);
  return g_fail ? 1 : 0;
}

template <class T>
static std::vector<T> load(const std::string& path, size_t count) {
  FILE* f = fopen(path.c_str(), "rb");
  std::vector<T> v(count);
  if (!f || fread(v.data(), sizeof(T), count, f) != count || fgetc(f) != EOF) {
    fprintf(stderr, "cannot read %zu elements from %s\n", count, path.c_str());
    exit(2);
  }
  fclose(f);
  return v;
}

template <class T>
static int sum_pass(const std::string& dir, long R, long E, int ncol, long raw_n, long n_off) {
  const std::vector<T> partial = load<T>(dir + "/partial.bin", (size_t)(R * E));
  std::vector<T> dst = load<T>(dir + "/dst0.bin", (size_t)(E / ncol * raw_n));
  for (long e = 0; e < E; ++e) {
    T& d = dst.at((size_t)(n_off + det_dst_offset(e, ncol, raw_n)));
    d = det_sum(d, partial.data(), R, E, e);
  }
  FILE* f = fopen((dir + "/dst.bin").c_str(), "wb");
  if (!f || fwrite(dst.data(), sizeof(T), dst.size(), f) != dst.size()) return 2;
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "walk")) return walk(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "sum")) {
    const std::string dir = argv[2];
    const std::vector<int64_t> d = load<int64_t>(dir + "/dims.i64", 6);
    return d[0] ? sum_pass<double>(dir, d[1], d[2], (int)d[3], d[4], d[5]) : sum_pass<float>(dir, d[1], d[2], (int)d[3], d[4], d[5]);
  }
  fprintf(stderr, "usage: det_host_main walk CASES | sum DIR\n");
  return 2;
}
