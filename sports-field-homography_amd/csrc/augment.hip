// augment.hip - the reference's training augmentation (utils/augmentation.py: torchvision ColorJitter, GaussianBlur,
// RandomResizedCrop, RandomHorizontalFlip + the uv / poi flips) for a whole batch of decoded uint8 frames on the device.
//
// Every random decision is made on the host (augment.py, AugParams) and arrives as one 16-word block per sample:
//   [0..3] order: the jitter op of slot 0..3 (0 brightness, 1 contrast, 2 saturation, 3 hue)   [4..7] factor per OP (fp32 bits)
//   [8] enabled: bit op set = that op runs     [9] sigma (fp32 bits, 0 = no blur)     [10..13] crop i, j, h, w     [14] flip
// At most three launches per batch, no atomics (bit-reproducible), none inside a host loop over samples:
//  1. aug_gray_mean_kernel (only when some sample has contrast on): one wave per frame row; the ops that precede contrast in
//     the sample's order are applied to each pixel, gray = 0.2989 r + 0.587 g + 0.114 b summed in fp64, one partial per row.
//  2. aug_apply_kernel: a workgroup owns a 64 x 16 OUTPUT tile.  Head: the H row partials of its sample are summed in a
//     fixed order (the combine step of eval.hip folded in; every workgroup of a sample gets the same bits) -> the fp32 mean.
//     The tile is mapped back through flip and crop to its source rectangle; that rectangle plus the blur halo (k / 2, reflect
//     at the FRAME border as F.pad does before the crop) and the bilinear tap row / column goes from uint8 into LDS with the
//     jitter chain applied on the way in; the blur runs separably in LDS; the tile is resampled (bilinear, align_corners
//     False) and written as fp32 NCHW planes.  The same threads gather mask (uint8 -> int64) and uv (legacy nearest).
//  3. aug_poi_flip_kernel: poi / nonzeros through the flip permutation.
// The arithmetic restates torchvision.transforms.functional's tensor path op by op in fp32 (augment.reference_apply is the
// CPU yardstick); -ffp-contract=off keeps every product and sum a separate rounding, as torch's are.
#include "common.h"
#include "split_mfma.h"   // u32x4

namespace {

constexpr int kTW = 64, kTH = 16;            // output tile
constexpr int kSrcW = kTW + 2, kSrcH = kTH + 2;   // source rectangle of a tile: scale <= 1, + the bilinear tap (+ 1 spare)
constexpr int kParamWords = 16;
constexpr int kMaxK = 11;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

struct Sample {
  int order[4];
  float factor[4];
  int enabled;
  float sigma;
  int ci, cj, ch, cw;
  int flip;
};

__device__ __forceinline__ Sample load_sample(const int32_t* __restrict__ params, int b) {
  const int32_t* p = params + (size_t)b * kParamWords;   // the same address in every lane: scalar loads
  Sample s;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s.order[i] = p[i];
    s.factor[i] = __int_as_float(p[4 + i]);
  }
  s.enabled = p[8];
  s.sigma = __int_as_float(p[9]);
  s.ci = p[10];
  s.cj = p[11];
  s.ch = p[12];
  s.cw = p[13];
  s.flip = p[14];
  return s;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

// adjust_hue on a float image: _rgb2hsv, h = (h + f) % 1, _hsv2rgb, in torchvision's operation order
__device__ __forceinline__ void hue_op(float f, float& r, float& g, float& b) {
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = __fdiv_rn(cr, eqc ? 1.f : maxc);
  const float crd = eqc ? 1.f : cr;
  const float rc = __fdiv_rn(maxc - r, crd), gc = __fdiv_rn(maxc - g, crd), bc = __fdiv_rn(maxc - b, crd);
  const float hr = (maxc == r) ? (bc - gc) : 0.f;
  const float hg = (maxc == g && maxc != r) ? ((2.f + rc) - bc) : 0.f;
  const float hb = (maxc != g && maxc != r) ? ((4.f + gc) - rc) : 0.f;
  float h = (hr + hg) + hb;
  h = fmodf(__fdiv_rn(h, 6.f) + 1.f, 1.f);
  h = fmodf(h + f, 1.f);                     // torch.remainder: the result takes the divisor's sign
  if (h < 0.f) h += 1.f;
  const float h6 = h * 6.f;
  const float fl = floorf(h6);
  const float ff = h6 - fl;
  const int i = ((int)fl) % 6;
  const float v = maxc;
  const float p = clamp01(v * (1.f - s));
  const float q = clamp01(v * (1.f - s * ff));
  const float t = clamp01(v * (1.f - (s * (1.f - ff))));
  r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// The ColorJitter chain of one pixel.  The switch is uniform over the workgroup (one sample per workgroup): no divergence.
// UNTIL_CONTRAST: stop in front of contrast (the pre-pass that forms its mean).
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_chain(const Sample& sp, float mean, float& r, float& g, float& b) {
#pragma unroll
  for (int slot = 0; slot < 4; ++slot) {
    const int op = sp.order[slot];
    if (!((sp.enabled >> op) & 1)) continue;
    const float f = op == 0 ? sp.factor[0] : op == 1 ? sp.factor[1] : op == 2 ? sp.factor[2] : sp.factor[3];
    switch (op) {
      case 0:
        r = clamp01(f * r);
        g = clamp01(f * g);
        b = clamp01(f * b);
        break;
      case 1: {
        if (UNTIL_CONTRAST) return;
        const float m = (1.f - f) * mean;
        r = clamp01(f * r + m);
        g = clamp01(f * g + m);
        b = clamp01(f * b + m);
        break;
      }
      case 2: {
        const float m = (1.f - f) * gray_of(r, g, b);
        r = clamp01(f * r + m);
        g = clamp01(f * g + m);
        b = clamp01(f * b + m);
        break;
      }
      default:
        hue_op(f, r, g, b);
        break;
    }
  }
}

// grid (ceil(H / 4), B), 256 threads: wave wv of block x handles row 4x + wv of frame blockIdx.y.  VEC: W % 16 == 0 and the
// frames 16-byte aligned (checked by the launcher): a lane moves 48 bytes = 16 pixels with three 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_gray_mean_kernel(const uint8_t* __restrict__ frames,
                                                            const int32_t* __restrict__ params, int H, int W,
                                                            double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (y >= H) return;                                   // whole waves only; the kernel has no barrier
  const Sample sp = load_sample(params, b);
  double acc = 0.0;
  if (sp.enabled & 2) {
    const uint8_t* row = frames + ((size_t)b * H + y) * (size_t)W * 3;
    if (VEC) {
      for (int c = lane; c < W / 16; c += 64) {
        const u32x4* q = reinterpret_cast<const u32x4*>(row + (size_t)c * 48);
        const u32x4 v0 = q[0], v1 = q[1], v2 = q[2];
        const unsigned w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          float ch[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const int byte = p * 3 + k;
            ch[k] = __fdiv_rn((float)((w[byte >> 2] >> (8 * (byte & 3))) & 255u), 255.f);
          }
          jitter_chain<true>(sp, 0.f, ch[0], ch[1], ch[2]);
          acc += (double)gray_of(ch[0], ch[1], ch[2]);
        }
      }
    } else {
      for (int x = lane; x < W; x += 64) {
        float r = __fdiv_rn((float)row[x * 3], 255.f), g = __fdiv_rn((float)row[x * 3 + 1], 255.f),
              bl = __fdiv_rn((float)row[x * 3 + 2], 255.f);
        jitter_chain<true>(sp, 0.f, r, g, bl);
        acc += (double)gray_of(r, g, bl);
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) part[(size_t)b * H + y] = acc;
}

__device__ __forceinline__ int reflect(int v, int n) {   // F.pad(mode='reflect'), pad < n
  v = v < 0 ? -v : v;
  v = v >= n ? 2 * (n - 1) - v : v;
  return min(max(v, 0), n - 1);                          // in range whatever the parameter block holds
}

// bilinear source position of destination index d (align_corners False): area_pixel_compute_source_index +
// guard_index_and_lambda of ATen, in fp32 as the CPU kernel evaluates them for a float tensor
__device__ __forceinline__ void lin_src(int d, float scale, int in, int& i0, int& i1, float& lam) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min((int)floorf(s), in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

// legacy 'nearest': min(floor(dst * scale), in - 1) with the fp32 scale (float)in / out
__device__ __forceinline__ int near_src(int d, float scale, int in) { return min((int)floorf((float)d * scale), in - 1); }

// grid (ceil(W / 64), ceil(H / 16), B), 256 threads.  Dynamic LDS (floats): wk[16] | S0[3][kSrcH + 2R][kSrcW + 2R] |
// S1[3][kSrcH + 2R][kSrcW] with R = K / 2; the blurred tile overwrites the head of S0.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_apply_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                        const float* __restrict__ uv, const int32_t* __restrict__ params,
                                                        const double* __restrict__ part, int H, int W, int K, int uvc,
                                                        float* __restrict__ image, int64_t* __restrict__ mask_out,
                                                        float* __restrict__ uv_out, float* __restrict__ mean_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int x1 = min(x0 + kTW, W) - 1, y1 = min(y0 + kTH, H) - 1;      // last output column / row of the tile
  Sample sp = load_sample(params, b);
  // the host validates the crop (augment.py); clamped all the same so that no parameter block can address outside the frame
  sp.ci = min(max(sp.ci, 0), H - 1);
  sp.cj = min(max(sp.cj, 0), W - 1);
  sp.ch = min(max(sp.ch, 1), H - sp.ci);
  sp.cw = min(max(sp.cw, 1), W - sp.cj);
  const bool blur = sp.sigma > 0.f && K > 1;
  const int R = K / 2, r = blur ? R : 0;
  const int ld0 = kSrcW + 2 * R, ld1 = kSrcW;
  const int rows_max = kSrcH + 2 * R;
  float* wk = lds;
  float* S0 = lds + 16;
  float* S1 = S0 + 3 * rows_max * ld0;

  // ---- head: contrast mean (fixed-order sum of the row partials) and the blur weights
  float mean = 0.f;
  if ((sp.enabled & 2) && part) {
    double s = 0.0;
    for (int y = tid; y < H; y += 256) s += part[(size_t)b * H + y];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    mean = (float)(red[0] / ((double)H * (double)W));
    if (mean_out && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) mean_out[b] = mean;
  } else if (mean_out && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    mean_out[b] = 0.f;
  }
  if (blur && tid < K) {
    // _get_gaussian_kernel1d: exp(-0.5 (t / sigma)^2) on linspace(-(K-1)/2, (K-1)/2, K), normalised; formed in fp64
    const double sg = (double)sp.sigma, half = 0.5 * (double)(K - 1);
    double sum = 0.0, mine = 0.0;
    for (int t = 0; t < K; ++t) {
      const double u = ((double)t - half) / sg;
      const double e = exp(-0.5 * u * u);
      sum += e;
      mine = t == tid ? e : mine;
    }
    wk[tid] = (float)(mine / sum);
  }

  // ---- source rectangle of the tile, crop-relative (columns through the flip)
  const float sclx = __fdiv_rn((float)sp.cw, (float)W), scly = __fdiv_rn((float)sp.ch, (float)H);
  const int xd_lo = sp.flip ? W - 1 - x1 : x0, xd_hi = sp.flip ? W - 1 - x0 : x1;
  int cx_lo, cx_hi, cy_lo, cy_hi, t0, t1;
  float tl;
  lin_src(xd_lo, sclx, sp.cw, cx_lo, t1, tl);
  lin_src(xd_hi, sclx, sp.cw, t0, cx_hi, tl);
  lin_src(y0, scly, sp.ch, cy_lo, t1, tl);
  lin_src(y1, scly, sp.ch, t0, cy_hi, tl);
  const int nx = min(cx_hi - cx_lo + 1, kSrcW), ny = min(cy_hi - cy_lo + 1, kSrcH);   // <= kTW + 1, kTH + 1 (scale <= 1)
  const int nxh = nx + 2 * r, nyh = ny + 2 * r;

  // ---- stage uint8 -> jittered fp32, halo reflected at the frame border
  const uint8_t* fb = frames + (size_t)b * H * (size_t)W * 3;
  for (int e = tid; e < nyh * nxh; e += 256) {
    const int ry = e / nxh, rx = e - ry * nxh;
    const int fy = reflect(sp.ci + cy_lo - r + ry, H), fx = reflect(sp.cj + cx_lo - r + rx, W);
    const uint8_t* px = fb + ((size_t)fy * W + fx) * 3;
    float cr = __fdiv_rn((float)px[0], 255.f), cg = __fdiv_rn((float)px[1], 255.f), cb = __fdiv_rn((float)px[2], 255.f);
    jitter_chain<false>(sp, mean, cr, cg, cb);
    S0[(0 * rows_max + ry) * ld0 + rx] = cr;
    S0[(1 * rows_max + ry) * ld0 + rx] = cg;
    S0[(2 * rows_max + ry) * ld0 + rx] = cb;
  }
  __syncthreads();
  if (blur) {
    // rows: S1[c][ry][cx] = sum_t wk[t] S0[c][ry][cx + t]
    for (int e = tid; e < 3 * nyh * nx; e += 256) {
      const int c = e / (nyh * nx), q = e - c * (nyh * nx);
      const int ry = q / nx, cx = q - ry * nx;
      const float* s = S0 + (c * rows_max + ry) * ld0 + cx;
      float a = 0.f;
      for (int t = 0; t < K; ++t) a += wk[t] * s[t];
      S1[(c * rows_max + ry) * ld1 + cx] = a;
    }
    __syncthreads();
    // columns, into the head of S0: S0[c][cy][cx] = sum_t wk[t] S1[c][cy + t][cx]
    for (int e = tid; e < 3 * ny * nx; e += 256) {
      const int c = e / (ny * nx), q = e - c * (ny * nx);
      const int cy = q / nx, cx = q - cy * nx;
      const float* s = S1 + (c * rows_max + cy) * ld1 + cx;
      float a = 0.f;
      for (int t = 0; t < K; ++t) a += wk[t] * s[t * ld1];
      S0[(c * rows_max + cy) * ld0 + cx] = a;
    }
    __syncthreads();
  }

  // ---- resample: thread -> 4 consecutive output pixels of one row
  const int ty = tid >> 4, tx = (tid & 15) * 4;
  const int y = y0 + ty, xb = x0 + tx;
  if (y > y1 || xb > x1) return;
  int iy0, iy1;
  float ly;
  lin_src(y, scly, sp.ch, iy0, iy1, ly);
  iy0 = min(max(iy0 - cy_lo, 0), ny - 1);
  iy1 = min(max(iy1 - cy_lo, 0), ny - 1);
  const float wy0 = 1.f - ly;
  const float nsx = __fdiv_rn((float)sp.cw, (float)W), nsy = __fdiv_rn((float)sp.ch, (float)H);
  const int my = sp.ci + near_src(y, nsy, sp.ch);
  const size_t plane = (size_t)H * W;
  float o[3][4];
  long long mo[4];
  int msrc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int x = min(xb + e, x1);                   // lanes past the tile edge repeat the last pixel (never stored)
    const int xd = sp.flip ? W - 1 - x : x;
    int ix0, ix1;
    float lx;
    lin_src(xd, sclx, sp.cw, ix0, ix1, lx);
    ix0 = min(max(ix0 - cx_lo, 0), nx - 1);
    ix1 = min(max(ix1 - cx_lo, 0), nx - 1);
    const float wx0 = 1.f - lx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* t = S0 + (c * rows_max + iy0) * ld0;
      const float* u = S0 + (c * rows_max + iy1) * ld0;
      const float top = wx0 * t[ix0] + lx * t[ix1];
      const float bot = wx0 * u[ix0] + lx * u[ix1];
      o[c][e] = wy0 * top + ly * bot;
    }
    msrc[e] = my * W + sp.cj + near_src(xd, nsx, sp.cw);
    mo[e] = masks ? (long long)masks[(size_t)b * plane + msrc[e]] : 0;
  }
  const size_t orow = (size_t)y * W + xb;
  const bool full = xb + 3 <= x1;
  if (VEC && full) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<f32x4*>(image + ((size_t)b * 3 + c) * plane + orow) = f32x4{o[c][0], o[c][1], o[c][2], o[c][3]};
    if (mask_out) {
      i64x2* m = reinterpret_cast<i64x2*>(mask_out + (size_t)b * plane + orow);
      m[0] = i64x2{mo[0], mo[1]};
      m[1] = i64x2{mo[2], mo[3]};
    }
  } else {
    for (int e = 0; e < 4 && xb + e <= x1; ++e) {
#pragma unroll
      for (int c = 0; c < 3; ++c) image[((size_t)b * 3 + c) * plane + orow + e] = o[c][e];
      if (mask_out) mask_out[(size_t)b * plane + orow + e] = mo[e];
    }
  }
  if (uv_out) {
    for (int c = 0; c < uvc; ++c) {
      const float* us = uv + ((size_t)b * uvc + c) * plane;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = us[msrc[e]];
        // UVHorizontalFlip: u -> (u > 0) - u on channel 0
        if (sp.flip && c == 0) v[e] = (v[e] > 0.f ? 1.f : 0.f) - v[e];
      }
      float* ud = uv_out + ((size_t)b * uvc + c) * plane + orow;
      if (VEC && full) {
        *reinterpret_cast<f32x4*>(ud) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
        for (int e = 0; e < 4 && xb + e <= x1; ++e) ud[e] = v[e];
      }
    }
  }
}

// PoIHorizontalFlip for the batch: out[b][n] = flip_b ? (1 - poi[b][perm[n]].x, poi[b][perm[n]].y) : poi[b][n], nonzeros
// alongside.  perm is the involution built from the pair list (validated on the host).
__global__ __launch_bounds__(256) void aug_poi_flip_kernel(const float* __restrict__ poi, const float* __restrict__ nz,
                                                           const int32_t* __restrict__ perm,
                                                           const int32_t* __restrict__ params, int batch, int npts,
                                                           float* __restrict__ poi_out, float* __restrict__ nz_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= batch * npts) return;
  const int b = i / npts, n = i - b * npts;
  const bool flip = params[(size_t)b * kParamWords + 14] != 0;
  int s = flip ? perm[n] : n;
  s = min(max(s, 0), npts - 1);
  const size_t src = (size_t)b * npts + s;
  const float x = poi[src * 2], y = poi[src * 2 + 1];
  poi_out[(size_t)i * 2] = flip ? 1.f - x : x;
  poi_out[(size_t)i * 2 + 1] = y;
  if (nz) nz_out[i] = nz[src];
}

size_t apply_lds_bytes(int K) {
  const int R = K / 2;
  return sizeof(float) * (16 + (size_t)3 * (kSrcH + 2 * R) * ((kSrcW + 2 * R) + kSrcW));
}

}  // namespace

extern "C" int64_t sfh_aug_workspace_doubles(int batch, int H) {
  if (batch <= 0 || batch > 65535 || H <= 0) return -1;
  return (int64_t)batch * H;
}

extern "C" int sfh_aug_gray_mean(const uint8_t* frames, const int32_t* params, int batch, int H, int W, double* workspace,
                                 void* stream) {
  SFH_REQUIRE(frames && params && workspace, "aug_gray_mean: null frames / params / workspace");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 28),
              "aug_gray_mean: bad geometry b=%d h=%d w=%d", batch, H, W);
  const bool vec = W % 16 == 0 && ((uintptr_t)frames & 15) == 0;
  const dim3 grid((unsigned)sfh_cdiv(H, 4), (unsigned)batch);
  if (vec)
    hipLaunchKernelGGL(aug_gray_mean_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, frames, params, H, W, workspace);
  else
    hipLaunchKernelGGL(aug_gray_mean_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, frames, params, H, W, workspace);
  return sfh_check_launch("aug_gray_mean_kernel");
}

extern "C" int sfh_aug_apply(const uint8_t* frames, const uint8_t* masks, const float* uv, const int32_t* params,
                             const double* workspace, int batch, int H, int W, int blur_k, int uv_channels, float* image,
                             int64_t* mask_out, float* uv_out, float* mean_out, void* stream) {
  SFH_REQUIRE(frames && params && image, "aug_apply: null frames / params / image");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 28) && H <= 65535 * kTH,
              "aug_apply: bad geometry b=%d h=%d w=%d", batch, H, W);
  SFH_REQUIRE(blur_k >= 1 && blur_k <= kMaxK && (blur_k & 1), "aug_apply: blur size %d (odd, 1 .. %d)", blur_k, kMaxK);
  SFH_REQUIRE(blur_k / 2 < H && blur_k / 2 < W, "aug_apply: blur size %d needs a frame larger than %d", blur_k, blur_k / 2);
  SFH_REQUIRE(!masks == !mask_out, "aug_apply: masks and mask_out go together");
  SFH_REQUIRE(!uv == !uv_out && (!uv || (uv_channels >= 1 && uv_channels <= 8)),
              "aug_apply: uv and uv_out go together, 1 .. 8 channels (%d)", uv_channels);
  const bool vec = W % 4 == 0 && (((uintptr_t)image | (uintptr_t)mask_out | (uintptr_t)uv_out) & 15) == 0;
  const dim3 grid((unsigned)sfh_cdiv(W, kTW), (unsigned)sfh_cdiv(H, kTH), (unsigned)batch);
  const size_t lds = apply_lds_bytes(blur_k);
  if (vec)
    hipLaunchKernelGGL(aug_apply_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, frames, masks, uv, params, workspace,
                       H, W, blur_k, uv_channels, image, mask_out, uv_out, mean_out);
  else
    hipLaunchKernelGGL(aug_apply_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, frames, masks, uv, params, workspace,
                       H, W, blur_k, uv_channels, image, mask_out, uv_out, mean_out);
  return sfh_check_launch("aug_apply_kernel");
}

extern "C" int sfh_aug_poi_flip(const float* poi, const float* nonzeros, const int32_t* perm, const int32_t* params, int batch,
                                int npts, float* poi_out, float* nonzeros_out, void* stream) {
  SFH_REQUIRE(poi && perm && params && poi_out, "aug_poi_flip: null poi / perm / params / output");
  SFH_REQUIRE(!nonzeros == !nonzeros_out, "aug_poi_flip: nonzeros and nonzeros_out go together");
  SFH_REQUIRE(batch > 0 && npts > 0 && (int64_t)batch * npts <= ((int64_t)1 << 24), "aug_poi_flip: bad shape b=%d n=%d", batch,
              npts);
  hipLaunchKernelGGL(aug_poi_flip_kernel, dim3((unsigned)sfh_cdiv(batch * npts, 256)), dim3(256), 0, (hipStream_t)stream, poi,
                     nonzeros, perm, params, batch, npts, poi_out, nonzeros_out);
  return sfh_check_launch("aug_poi_flip_kernel");
}
