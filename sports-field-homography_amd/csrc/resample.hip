// resample.hip - Pillow's 8-bit image resize on the device (the byte-exact rule: tests/resample_ref.py).
//
// The image-directory datasets of the reference resize with PIL (utils/dataset.py:146-185): `pil_img.resize(size)` for the frames
// (Pillow's default filter, BICUBIC with antialiasing), `Image.NEAREST` for the label masks and cv2.INTER_NEAREST for the uint16
// UV labels.  Pillow's 8-bit resampler (libImaging/Resample.c) is integer arithmetic: per axis a table of (xmin, n) and n
// coefficients in 22-bit fixed point per output index, a horizontal pass into a uint8 intermediate, then a vertical pass, each
// `clamp((2^21 + sum pixel * k) >> 22, 0, 255)` in 32-bit int.  The tables are host code (sfh_resample_tab, fp64 like
// Pillow's); the kernel only multiplies and adds integers, so its bytes do not depend on the order anything runs in.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"

namespace {

constexpr int kMaxTaps = SFH_RESAMPLE_MAX_TAPS;
constexpr int kMaxRows = SFH_RESAMPLE_MAX_ROWS;   // source rows of a tile's uint8 intermediate in LDS
constexpr int kTileW = 64;                        // output pixels of a tile row
constexpr int kTileH = 16;                        // output rows of a tile at most
constexpr int kCoefStride = kMaxTaps + 1;         // odd: lanes of neighbouring pixels read their rows from different banks
constexpr int kPrecisionBits = 32 - 8 - 2;
#ifndef SFH_RESAMPLE_THREADS
#define SFH_RESAMPLE_THREADS 256                  // a host emulation of the kernels runs them with 1
#endif
constexpr int kThreads = SFH_RESAMPLE_THREADS;

// ------------------------------------------------------------------------------------------------ host: the tables
double filter_value(int filter, double x) {
  if (filter == SFH_FILTER_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
  if (x < 0.0) x = -x;
  if (filter == SFH_FILTER_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

double filter_support(int filter) { return filter == SFH_FILTER_BOX ? 0.5 : (filter == SFH_FILTER_BILINEAR ? 1.0 : 2.0); }

bool filter_known(int filter) { return filter == SFH_FILTER_BOX || filter == SFH_FILTER_BILINEAR || filter == SFH_FILTER_BICUBIC; }

// precompute_coeffs of Resample.c for the whole axis (box = (0, in)): the row stride ksize and, per output index, (xmin, n)
int axis_ksize(int in, int out, int filter, double* scale_out, double* support_out) {
  double scale = (double)in / (double)out, filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = filter_support(filter) * filterscale;
  *scale_out = scale;
  *support_out = support;
  const double ks = ceil(support) * 2 + 1;
  return ks > 1e8 ? -1 : (int)ks;
}

void axis_bounds(int in, double scale, double support, int xx, int* xmin_out, int* n_out) {
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  *xmin_out = xmin;
  *n_out = xmax - xmin;
}

}  // namespace

extern "C" int sfh_resample_max_taps(void) { return kMaxTaps; }

extern "C" int sfh_resample_tab(int in, int out, int filter, int32_t* bounds, int32_t* coef, int cap) {
  if (!bounds || !coef || in <= 0 || out <= 0 || !filter_known(filter)) return -1;
  double scale, support;
  const int ksize = axis_ksize(in, out, filter, &scale, &support);
  if (ksize <= 0 || (int64_t)ksize * out > (int64_t)cap) return -1;
  double fs = scale < 1.0 ? 1.0 : scale;
  const double ss = 1.0 / fs;
  std::vector<double> k((size_t)ksize);
  for (int xx = 0; xx < out; ++xx) {
    int xmin, n;
    axis_bounds(in, scale, support, xx, &xmin, &n);
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      const double w = filter_value(filter, (x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    int32_t* row = coef + (size_t)xx * ksize;
    for (int x = 0; x < n; ++x) {
      double w = k[x];
      if (ww != 0.0) w /= ww;
      row[x] = w < 0 ? (int)(-0.5 + w * (1 << kPrecisionBits)) : (int)(0.5 + w * (1 << kPrecisionBits));
    }
    for (int x = n < 0 ? 0 : n; x < ksize; ++x) row[x] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return ksize;
}

// rows of an output tile on the vertical axis: the largest of 16, 8, 4, 2, 1 for which the source rows every tile's taps reach
// fit the LDS intermediate; -1 when an output index has more than SFH_RESAMPLE_MAX_TAPS taps (then 1 row does not fit either way)
extern "C" int sfh_resample_tile_rows(int in, int out, int filter) {
  if (in <= 0 || out <= 0 || !filter_known(filter)) return -1;
  double scale, support;
  if (axis_ksize(in, out, filter, &scale, &support) <= 0) return -1;
  std::vector<int> lo((size_t)out), hi((size_t)out);
  for (int xx = 0; xx < out; ++xx) {
    int xmin, n;
    axis_bounds(in, scale, support, xx, &xmin, &n);
    if (n > kMaxTaps) return -1;
    lo[xx] = xmin;
    hi[xx] = xmin + (n > 0 ? n : 0);
  }
  for (int th = kTileH; th >= 1; th >>= 1) {
    bool ok = true;
    for (int y0 = 0; y0 < out && ok; y0 += th) {
      int a = lo[y0], b = hi[y0];
      for (int y = y0; y < out && y < y0 + th; ++y) {
        a = lo[y] < a ? lo[y] : a;
        b = hi[y] > b ? hi[y] : b;
      }
      ok = b - a <= kMaxRows;
    }
    if (ok) return th;
  }
  return -1;
}

extern "C" int sfh_nearest_tab(int in, int out, int rule, int32_t* idx, int cap) {
  if (!idx || in <= 0 || out <= 0 || cap < out || (rule != SFH_NEAREST_PIL && rule != SFH_NEAREST_CV2)) return -1;
  if (rule == SFH_NEAREST_PIL) {
    // ImagingScaleAffine of Pillow's Geometry.c: a running fp64 sum, not the closed form
    const double a = (double)in / (double)out;
    double x = a * 0.5;
    for (int i = 0; i < out; ++i) {
      int v = x < 0.0 ? 0 : (int)x;
      idx[i] = v > in - 1 ? in - 1 : v;
      x += a;
    }
  } else {
    // OpenCV's resizeNN: sx = min(floor(dx * (1 / fx)), in - 1), fx = out / in in double
    const double ifx = 1.0 / ((double)out / (double)in);
    for (int i = 0; i < out; ++i) {
      int v = (int)floor(i * ifx);
      idx[i] = v > in - 1 ? in - 1 : v;
    }
  }
  return out;
}

// ------------------------------------------------------------------------------------------------ device
namespace {

struct ResampleArgs {
  const uint8_t* src;
  uint8_t* dst_u8;
  float* dst_f32;
  int C, Hs, Ws, Hd, Wd;
  const int32_t *xb, *xk, *yb, *yk;
  int xstride, ystride, tile_rows;
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrecisionBits;          // arithmetic shift, as Pillow's table index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// coefficient rows [first, first + count) of one axis -> LDS, every (xmin, n) forced inside the source so that a table that does
// not belong to this size pair cannot make the kernel read outside its buffers
__device__ __forceinline__ void stage_axis(const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef, int stride,
                                           int first, int count, int in, int* s_min, int* s_n, int* s_k) {
  for (int i = threadIdx.x; i < count; i += kThreads) {
    int n = bounds[2 * (first + i) + 1];
    n = n < 0 ? 0 : (n > kMaxTaps ? kMaxTaps : n);
    n = n > in ? in : n;
    n = n > stride ? stride : n;
    int lo = bounds[2 * (first + i)];
    lo = lo < 0 ? 0 : (lo > in - n ? in - n : lo);
    s_min[i] = lo;
    s_n[i] = n;
  }
  for (int i = threadIdx.x; i < count * kMaxTaps; i += kThreads) {
    const int r = i / kMaxTaps, t = i - r * kMaxTaps;
    s_k[r * kCoefStride + t] = t < stride ? coef[(long)(first + r) * stride + t] : 0;
  }
}

// one output byte: item j of a tile row of `tw` pixels -> (x, c).  With a float destination the planes are walked one after the
// other (lanes write consecutive floats of a plane); with bytes only, the interleaved row (lanes write consecutive bytes).
__device__ __forceinline__ void item_xc(int j, int tw, int C, bool planes, int* x, int* c) {
  if (planes) {
    *c = j / tw;
    *x = j - *c * tw;
  } else {
    *x = j / C;
    *c = j - *x * C;
  }
}

__device__ __forceinline__ void emit(const ResampleArgs& a, long b, int y, int x, int c, int v) {
  if (a.dst_u8) a.dst_u8[((b * a.Hd + y) * a.Wd + x) * a.C + c] = (uint8_t)v;
  // the dataset's `img / 255 -> FloatTensor` (u8hwc_to_f32nchw_kernel's rule): one IEEE division
  if (a.dst_f32) a.dst_f32[((b * a.C + c) * a.Hd + y) * a.Wd + x] = (float)v / 255.0f;
}

// MODE 0: both passes through the LDS intermediate, 1: widths differ only, 2: heights differ only.
// grid (tiles of kTileW output columns, tiles of tile_rows output rows, images); kThreads threads.
template <int MODE>
__global__ __launch_bounds__(kThreads) void resample_kernel(ResampleArgs a) {
  __shared__ int s_xmin[kTileW], s_xn[kTileW], s_ymin[kTileH], s_yn[kTileH];
  __shared__ int s_xk[MODE == 2 ? 1 : kTileW * kCoefStride];
  __shared__ int s_yk[MODE == 1 ? 1 : kTileH * kCoefStride];
  __shared__ uint8_t s_mid[MODE == 0 ? kMaxRows * kTileW * 3 : 4];

  const int C = a.C;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * a.tile_rows;
  const long b = blockIdx.z;
  const int tw = min(kTileW, a.Wd - x0), th = min(a.tile_rows, a.Hd - y0);
  const int twc = tw * C;
  const uint8_t* __restrict__ img = a.src + b * (long)a.Hs * a.Ws * C;
  const bool planes = a.dst_f32 != nullptr;

  if (MODE != 2) stage_axis(a.xb, a.xk, a.xstride, x0, tw, a.Ws, s_xmin, s_xn, s_xk);
  if (MODE != 1) stage_axis(a.yb, a.yk, a.ystride, y0, th, a.Hs, s_ymin, s_yn, s_yk);
  __syncthreads();

  if (MODE == 1) {
    for (int i = threadIdx.x; i < th * twc; i += kThreads) {
      const int r = i / twc;
      int x, c;
      item_xc(i - r * twc, tw, C, planes, &x, &c);
      const uint8_t* p = img + ((long)(y0 + r) * a.Ws + s_xmin[x]) * C + c;
      const int* k = s_xk + x * kCoefStride;
      int acc = 1 << (kPrecisionBits - 1);
      for (int t = 0; t < s_xn[x]; ++t) acc += (int)p[t * C] * k[t];
      emit(a, b, y0 + r, x0 + x, c, clip8(acc));
    }
    return;
  }

  if (MODE == 2) {
    for (int i = threadIdx.x; i < th * twc; i += kThreads) {
      const int r = i / twc;
      int x, c;
      item_xc(i - r * twc, tw, C, planes, &x, &c);
      const uint8_t* p = img + ((long)s_ymin[r] * a.Ws + x0 + x) * C + c;
      const int* k = s_yk + r * kCoefStride;
      const long rs = (long)a.Ws * C;
      int acc = 1 << (kPrecisionBits - 1);
      for (int t = 0; t < s_yn[r]; ++t) acc += (int)p[t * rs] * k[t];
      emit(a, b, y0 + r, x0 + x, c, clip8(acc));
    }
    return;
  }

  // the source rows this tile's vertical taps reach (the bounds rise with the output index; the min / max keeps any table safe)
  int row0 = s_ymin[0], row1 = s_ymin[0] + s_yn[0];
  for (int r = 1; r < th; ++r) {
    row0 = min(row0, s_ymin[r]);
    row1 = max(row1, s_ymin[r] + s_yn[r]);
  }
  const int rows = min(row1 - row0, kMaxRows);

  // horizontal pass: lanes walk the interleaved bytes of an intermediate row, so a wave's loads of one tap cover one run of a
  // source row
  for (int i = threadIdx.x; i < rows * twc; i += kThreads) {
    const int r = i / twc, j = i - r * twc;
    const int x = j / C, c = j - x * C;
    const uint8_t* p = img + ((long)(row0 + r) * a.Ws + s_xmin[x]) * C + c;
    const int* k = s_xk + x * kCoefStride;
    int acc = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < s_xn[x]; ++t) acc += (int)p[t * C] * k[t];
    s_mid[r * (kTileW * 3) + j] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  // vertical pass out of LDS
  for (int i = threadIdx.x; i < th * twc; i += kThreads) {
    const int r = i / twc;
    int x, c;
    item_xc(i - r * twc, tw, C, planes, &x, &c);
    const int first = s_ymin[r] - row0;
    const int n = min(s_yn[r], rows - first);       // == s_yn[r] for this library's tables
    const uint8_t* p = s_mid + first * (kTileW * 3) + x * C + c;
    const int* k = s_yk + r * kCoefStride;
    int acc = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) acc += (int)p[t * (kTileW * 3)] * k[t];
    emit(a, b, y0 + r, x0 + x, c, clip8(acc));
  }
}

// nearest resize through two index tables: one thread per output element (pixel x channel); grid (row chunks, Hd, images)
template <typename T>
__global__ __launch_bounds__(kThreads) void resize_gather_kernel(const T* __restrict__ src, T* __restrict__ dst, int C, int Hs, int Ws,
                                                            int Hd, int Wd, const int32_t* __restrict__ yidx,
                                                            const int32_t* __restrict__ xidx) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= Wd * C) return;
  const int x = j / C, c = j - x * C;
  const int y = blockIdx.y;
  const long b = blockIdx.z;
  const int sy = min(max(yidx[y], 0), Hs - 1), sx = min(max(xidx[x], 0), Ws - 1);
  dst[((b * Hd + y) * Wd) * C + j] = src[((b * Hs + sy) * Ws + sx) * C + c];
}

}  // namespace

extern "C" int sfh_resample_u8(const uint8_t* src, uint8_t* dst_u8, float* dst_f32, int batch, int C, int Hs, int Ws, int Hd,
                               int Wd, const int32_t* xbounds, const int32_t* xcoef, int xstride, int xtaps,
                               const int32_t* ybounds, const int32_t* ycoef, int ystride, int ytaps, int tile_rows, void* stream) {
  SFH_REQUIRE(src && (dst_u8 || dst_f32), "resample_u8: null pointer (a source and at least one destination)");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && (C == 1 || C == 3) && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0,
              "resample_u8: bad geometry: batch %d (1 .. 65535) of %dx%dx%d -> %dx%d (1 or 3 channels)", batch, Ws, Hs, C, Wd, Hd);
  SFH_REQUIRE((long)Hs * Ws * C < (1L << 31) && (long)Hd * Wd * C < (1L << 31),
              "resample_u8: an image of 2 GiB or more");
  const bool hp = Ws != Wd, vp = Hs != Hd;
  if (hp) {
    SFH_REQUIRE(xbounds && xcoef && xstride > 0 && xtaps > 0, "resample_u8: the widths differ and there is no x table");
    SFH_REQUIRE(xtaps <= kMaxTaps, "resample_u8: %d -> %d columns needs %d taps, above the bound of %d (SFH_RESAMPLE_MAX_TAPS)", Ws,
                Wd, xtaps, kMaxTaps);
  }
  if (vp) {
    SFH_REQUIRE(ybounds && ycoef && ystride > 0 && ytaps > 0, "resample_u8: the heights differ and there is no y table");
    SFH_REQUIRE(ytaps <= kMaxTaps, "resample_u8: %d -> %d rows needs %d taps, above the bound of %d (SFH_RESAMPLE_MAX_TAPS)", Hs, Hd,
                ytaps, kMaxTaps);
    SFH_REQUIRE(tile_rows == 1 || tile_rows == 2 || tile_rows == 4 || tile_rows == 8 || tile_rows == 16,
                "resample_u8: tile_rows %d (sfh_resample_tile_rows: 1, 2, 4, 8 or 16)", tile_rows);
  }
  if (!hp && !vp) {      // equal sizes: Pillow returns a copy
    if (dst_u8) {
      hipError_t e = hipMemcpyAsync(dst_u8, src, (size_t)batch * Hs * Ws * C, hipMemcpyDeviceToDevice, (hipStream_t)stream);
      if (e != hipSuccess) {
        sfh_set_error("resample_u8: copy: %s", hipGetErrorString(e));
        return SFH_E_LAUNCH;
      }
    }
    return dst_f32 ? sfh_u8hwc_to_f32nchw(src, dst_f32, batch, C, Hs, Ws, stream) : SFH_OK;
  }
  ResampleArgs a;
  a.src = src, a.dst_u8 = dst_u8, a.dst_f32 = dst_f32;
  a.C = C, a.Hs = Hs, a.Ws = Ws, a.Hd = Hd, a.Wd = Wd;
  a.xb = xbounds, a.xk = xcoef, a.yb = ybounds, a.yk = ycoef;
  a.xstride = xstride, a.ystride = ystride;
  a.tile_rows = vp ? tile_rows : kTileH;
  const int tiles_y = (Hd + a.tile_rows - 1) / a.tile_rows;
  SFH_REQUIRE(tiles_y <= 65535, "resample_u8: %d output rows in tiles of %d: more than 65535 tiles", Hd, a.tile_rows);
  const dim3 grid((unsigned)((Wd + kTileW - 1) / kTileW), (unsigned)tiles_y, (unsigned)batch);
  if (hp && vp)
    hipLaunchKernelGGL(resample_kernel<0>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
  else if (hp)
    hipLaunchKernelGGL(resample_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(resample_kernel<2>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
  return sfh_check_launch("resample_kernel");
}

extern "C" int sfh_resize_gather(const void* src, void* dst, int batch, int C, int elem_bytes, int Hs, int Ws, int Hd, int Wd,
                                 const int32_t* yidx, const int32_t* xidx, void* stream) {
  SFH_REQUIRE(src && dst && yidx && xidx, "resize_gather: null pointer");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && Hs > 0 && Ws > 0 && Hd > 0 && Hd <= 65535 && Wd > 0,
              "resize_gather: bad geometry: batch %d of %dx%d -> %dx%d (batch and rows at most 65535)", batch, Ws, Hs, Wd, Hd);
  SFH_REQUIRE((elem_bytes == 1 && (C == 1 || C == 3)) || (elem_bytes == 2 && C == 3),
              "resize_gather: %d channels of %d bytes (uint8 with 1 or 3 channels, uint16 with 3)", C, elem_bytes);
  SFH_REQUIRE((long)Hs * Ws * C < (1L << 31) && (long)Hd * Wd * C < (1L << 31), "resize_gather: an image of 2^31 elements or more");
  const dim3 grid((unsigned)((Wd * C + kThreads - 1) / kThreads), (unsigned)Hd, (unsigned)batch);
  if (elem_bytes == 1)
    hipLaunchKernelGGL(resize_gather_kernel<uint8_t>, grid, dim3(kThreads), 0, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, C,
                       Hs, Ws, Hd, Wd, yidx, xidx);
  else
    hipLaunchKernelGGL(resize_gather_kernel<uint16_t>, grid, dim3(kThreads), 0, (hipStream_t)stream, (const uint16_t*)src,
                       (uint16_t*)dst, C, Hs, Ws, Hd, Wd, yidx, xidx);
  return sfh_check_launch("resize_gather_kernel");
}
