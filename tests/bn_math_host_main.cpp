// bn_math_host_main.cpp - the training-mode BatchNorm arithmetic of csrc/bn_math.h run on the host, element by element through
// the same functions the kernels of csrc/train_bn.hip, train_heads.hip and train_wgrad.hip and the conv epilogue call.
// Built and run by
// tests/test_train_kernel_host.py with -fsanitize=address,undefined and -ffp-contract=off (the library's own setting); it links
// nothing of the library.
//
//   bn_math_host_main apply DIR      dims.i64 = npix C relu with_res; z mi gamma beta [residual] (.f32)          -> y.f32
//   bn_math_host_main bwd DIR        dims.i64 = npix C relu with_y;   dy z mi gamma beta [y] (.f32), acc.f64     -> g.f32 dz.f32
//   bn_math_host_main finalize DIR   dims.i64 = npix C with_running;  acc.f64, params.f32 = eps momentum,
//                                    [running_mean running_var] (.f32) -> mean_invstd.f32 [running_mean.out running_var.out]
//
// Every file is a raw little-endian array, read into a heap block of exactly its size: one element too many is a sanitizer
// report.  C is a multiple of 4 in apply and bwd (the kernels' quads, through bn_load<4>).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../sports-field-homography_amd/csrc/bn_math.h"

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

// bn_apply_kernel: y = [relu](bn(z) [+ residual])
static void apply() {
  const auto d = load<int64_t>("dims.i64", 4);
  const long npix = d[0];
  const int C = (int)d[1];
  const bool relu = d[2], with_res = d[3];
  const size_t n = (size_t)npix * C;
  const auto z = load<float>("z.f32", n), mi = load<float>("mi.f32", 2 * C), gamma = load<float>("gamma.f32", C),
             beta = load<float>("beta.f32", C);
  const auto res = with_res ? load<float>("residual.f32", n) : std::vector<float>();
  std::vector<float> y(n);
  for (long p = 0; p < npix; ++p)
    for (int c = 0; c < C; c += 4) {
      const BnChannels<4> bn = bn_load<4>(mi.data(), gamma.data(), beta.data(), C, c);
      for (int j = 0; j < 4; ++j) {
        const size_t i = (size_t)p * C + c + j;
        float o = bn.y(j, z[i]);
        if (with_res) o += res[i];
        y[i] = relu ? sfh_relu(o) : o;
      }
    }
  store("y.f32", y);
}

// bn_bwd_apply_kernel: g = dy behind the ReLU (y given, or recomputed from z), dz
static void bwd() {
  const auto d = load<int64_t>("dims.i64", 4);
  const long npix = d[0];
  const int C = (int)d[1];
  const bool relu = d[2], with_y = d[3];
  const bool sign_from_z = relu && !with_y;
  const size_t n = (size_t)npix * C;
  const auto dy = load<float>("dy.f32", n), z = load<float>("z.f32", n), mi = load<float>("mi.f32", 2 * C),
             gamma = load<float>("gamma.f32", C);
  const auto beta = sign_from_z ? load<float>("beta.f32", C) : std::vector<float>();
  const auto y = with_y ? load<float>("y.f32", n) : std::vector<float>();
  const auto acc = load<double>("acc.f64", 2 * C);
  std::vector<float> g(n), dz(n);
  for (long p = 0; p < npix; ++p)
    for (int c = 0; c < C; c += 4) {
      const BnChannels<4> bn =
          bn_load<4, true>(mi.data(), gamma.data(), sign_from_z ? beta.data() : nullptr, C, c, sign_from_z, acc.data(), bn_inv_n(npix));
      for (int j = 0; j < 4; ++j) {
        const size_t i = (size_t)p * C + c + j;
        g[i] = bn_gate(sign_from_z ? bn.y(j, z[i]) : (relu ? y[i] : 1.f), dy[i]);
        dz[i] = bn.dz(j, z[i], g[i]);
      }
    }
  store("g.f32", g);
  store("dz.f32", dz);
}

// bn_finalize_kernel
static void finalize() {
  const auto d = load<int64_t>("dims.i64", 3);
  const long npix = d[0];
  const int C = (int)d[1];
  const bool with_running = d[2];
  const auto acc = load<double>("acc.f64", 2 * C);
  const auto par = load<float>("params.f32", 2);
  auto rm = with_running ? load<float>("running_mean.f32", C) : std::vector<float>();
  auto rv = with_running ? load<float>("running_var.f32", C) : std::vector<float>();
  std::vector<float> mi(2 * C);
  for (int c = 0; c < C; ++c)
    bn_finalize_channel(acc[c], acc[C + c], npix, par[0], par[1], C, c, mi.data(), with_running ? rm.data() : nullptr,
                        with_running ? rv.data() : nullptr);
  store("mean_invstd.f32", mi);
  if (with_running) {
    store("running_mean.out", rm);
    store("running_var.out", rv);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: bn_math_host_main apply|bwd|finalize DIR\n");
    return 2;
  }
  const std::string mode = argv[1];
  g_dir = argv[2];
  if (mode == "apply") apply();
  else if (mode == "bwd") bwd();
  else if (mode == "finalize") finalize();
  else return 2;
  return 0;
}
