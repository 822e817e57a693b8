// grouped_conv_host_main.cpp - the grouped 3x3 convolution of csrc/conv_grouped.hip run on the host, output by output through
// the index functions of csrc/conv_grouped_core.h and in the kernels' order of terms: pack (forward and backward-data
// layout), forward with the optional epilogue, backward-data (stride 2: zero-stuffed dz, then the stride-1 forward over the
// backward-data weights, as the library does) and backward-filter with the accumulation plan of the kernel.  Built and run by
// tests/test_grouped_conv_host.py with -fsanitize=address,undefined and -ffp-contract=off (the library's own setting); it
// links nothing of the library.
//
//   grouped_conv_host_main DIR     dims.i64 = B H W G cg stride relu with_epilogue n_w forward_only
//                                  x.f32 (B,H,W,C)  w.f32 (n_w, C,cg,3,3)  dz.f32 (B,Ho,Wo,C)  raw0.f32 (C,9,cg)
//                                  [scale.f32 shift.f32 (C)]
//                               -> y.f32 (n_w, B,Ho,Wo,C)  [dx.f32 (n_w, B,H,W,C)  raw.f32 (C,9,cg): not with forward_only]
//
// Every file is a raw little-endian array, read into a heap block of exactly its size: one element too many is a sanitizer
// report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../sports-field-homography_amd/csrc/bn_math.h"
#include "../sports-field-homography_amd/csrc/conv_grouped_core.h"

static std::string g_dir;

template <class T>
static std::vector<T> load(const char* name, size_t count) {
  const std::string path = g_dir + "/" + name;
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
static void store(const char* name, const std::vector<T>& v) {
  const std::string path = g_dir + "/" + name;
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || fclose(f) != 0) {
    fprintf(stderr, "cannot write %s\n", path.c_str());
    exit(2);
  }
}

// pack_grouped_kernel: every packed element from its checkpoint element, zero where a channel block reaches past C
static std::vector<float> pack(const float* w, int G, int cg, int mode) {
  std::vector<float> packed((size_t)gc_packed_floats(G, cg), 0.f);
  for (int oc = 0; oc < G * cg; ++oc)
    for (int tap = 0; tap < 9; ++tap)
      for (int c = 0; c < cg; ++c) packed[(size_t)gc_packed_index(cg, oc, tap, c)] = w[gc_weight_index(mode, cg, oc, tap, c)];
  return packed;
}

// conv_grouped_kernel: one output at a time, its terms in the order conv_grouped_core.h states
static void forward(const float* src, const std::vector<float>& packed, const float* scale, const float* shift, bool relu,
                    float* dst, int B, int H, int W, int G, int cg, int S) {
  const int C = G * cg, Ho = gc_out_size(H, S), Wo = gc_out_size(W, S), kc = gc_chunk(cg);
  for (int b = 0; b < B; ++b)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox)
        for (int oc = 0; oc < C; ++oc) {
          const int g = oc / cg;
          float acc = 0.f;
          for (int chunk = 0; chunk < cg / kc; ++chunk)
            for (int tap = 0; tap < 9; ++tap) {
              const int sy = gc_src_coord(oy, tap / 3, S, H), sx = gc_src_coord(ox, tap % 3, S, W);
              for (int c = chunk * kc; c < (chunk + 1) * kc; ++c) {
                const float x = (sy >= 0 && sx >= 0) ? src[gc_nhwc((long)(b * H + sy) * W + sx, C, cg, g, c)] : 0.f;
                acc += x * packed[(size_t)gc_packed_index(cg, oc, tap, c)];
              }
            }
          float v = acc;
          if (scale) v = v * scale[oc] + shift[oc];
          dst[gc_nhwc((long)(b * Ho + oy) * Wo + ox, C, cg, g, oc % cg)] = relu ? sfh_relu(v) : v;
        }
}

// conv_grouped_wgrad_kernel: tile by tile (the order of the tiles' atomic adds is free on the device; here: ascending)
static void wgrad(const float* dz, const float* src, float* raw, int B, int H, int W, int G, int cg, int S) {
  const int C = G * cg, Ho = gc_out_size(H, S), Wo = gc_out_size(W, S), th = gc_tile_h(S), lanes = gc_wgrad_lanes(cg);
  std::vector<float> part((size_t)lanes);
  for (int b = 0; b < B; ++b)
    for (int ty0 = 0; ty0 < Ho; ty0 += th)
      for (int tx0 = 0; tx0 < Wo; tx0 += GC_TW)
        for (int o = 0; o < C; ++o)
          for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < cg; ++c) {
              for (int l = 0; l < lanes; ++l) {
                float acc = 0.f;
                for (int p = l; p < th * GC_TW; p += lanes) {
                  const int oy = ty0 + p / GC_TW, ox = tx0 + p % GC_TW;
                  if (oy >= Ho || ox >= Wo) continue;   // the kernel adds d * x with d = 0 there: no change to acc
                  const int sy = gc_src_coord(oy, tap / 3, S, H), sx = gc_src_coord(ox, tap % 3, S, W);
                  const float x = (sy >= 0 && sx >= 0) ? src[gc_nhwc((long)(b * H + sy) * W + sx, C, cg, o / cg, c)] : 0.f;
                  acc += dz[(long)((b * Ho + oy) * Wo + ox) * C + o] * x;
                }
                part[(size_t)l] = acc;
              }
              float s = part[0];
              for (int l = 1; l < lanes; ++l) s += part[(size_t)l];
              raw[gc_raw_index(cg, o, tap, c)] += s;
            }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: grouped_conv_host_main DIR\n");
    return 2;
  }
  g_dir = argv[1];
  const auto d = load<int64_t>("dims.i64", 10);
  const int B = (int)d[0], H = (int)d[1], W = (int)d[2], G = (int)d[3], cg = (int)d[4], S = (int)d[5];
  const bool relu = d[6], with_epilogue = d[7];
  const int n_w = (int)d[8];
  const bool forward_only = d[9];
  if (!gc_cg_ok(cg) || (S != 1 && S != 2) || B < 1 || H < 1 || W < 1 || G < 1 || n_w < 1) return 2;
  const int C = G * cg, Ho = gc_out_size(H, S), Wo = gc_out_size(W, S);
  const size_t nx = (size_t)B * H * W * C, ny = (size_t)B * Ho * Wo * C, nw = (size_t)C * cg * 9;
  const auto x = load<float>("x.f32", nx), w = load<float>("w.f32", nw * n_w), dz = load<float>("dz.f32", ny);
  auto raw = load<float>("raw0.f32", nw);
  const auto scale = with_epilogue ? load<float>("scale.f32", C) : std::vector<float>();
  const auto shift = with_epilogue ? load<float>("shift.f32", C) : std::vector<float>();

  // sfh_zero_stuff2: dz at the input resolution (stride 1: dz itself)
  std::vector<float> up;
  if (S == 2 && !forward_only) {
    up.assign(nx, 0.f);
    for (int b = 0; b < B; ++b)
      for (int oy = 0; oy < Ho; ++oy)
        for (int ox = 0; ox < Wo; ++ox)
          for (int c = 0; c < C; ++c)
            up[((size_t)(b * H + 2 * oy) * W + 2 * ox) * C + c] = dz[((size_t)(b * Ho + oy) * Wo + ox) * C + c];
  }
  std::vector<float> y(ny * n_w), dx(forward_only ? 0 : nx * n_w);
  for (int k = 0; k < n_w; ++k) {
    forward(x.data(), pack(w.data() + nw * k, G, cg, 0), with_epilogue ? scale.data() : nullptr,
            with_epilogue ? shift.data() : nullptr, relu, y.data() + ny * k, B, H, W, G, cg, S);
    if (!forward_only)
      forward(S == 2 ? up.data() : dz.data(), pack(w.data() + nw * k, G, cg, 1), nullptr, nullptr, false, dx.data() + nx * k, B,
              H, W, G, cg, 1);
  }
  store("y.f32", y);
  if (forward_only) return 0;
  wgrad(dz.data(), x.data(), raw.data(), B, H, W, G, cg, S);
  store("dx.f32", dx);
  store("raw.f32", raw);
  return 0;
}
