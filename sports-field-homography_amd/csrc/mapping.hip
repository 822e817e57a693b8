// mapping.hip - what the homography is for: things seen in the frame onto the court plane (utils/transform.py, utils/court.py,
// utils/mapping_example.py of the reference).
//
// * theta_invert_kernel: theta (frame -> court) -> theta_c2f by inverse_h33 (warp_coords.h: the fp64 adjugate rule of
//   sfh_poi_project_fwd, shared, not copied) and a status byte per frame.
// * topview_kernel: uint8 HWC frames -> the uint8 HWC court view in ONE pass.  Per court pixel one homography evaluation with
//   the pinned fp32 coordinate arithmetic of warp.hip (norm_axis -> apply_h -> unnorm with the FRAME size, all through
//   warp_coords.h) and the frame bytes of one (nearest) or four (bilinear) taps.  Algorithmic traffic: 3 B read + 3 B + 1 B
//   written per court pixel.  warp.hip and overlay.hip measured this arithmetic as bound by vector issue, not by bandwidth, so
//   the structure is theirs: a wave-uniform classification of theta selects the fast-reciprocal forms (proven equal to the IEEE
//   divisions by sfh_selftest_warp_arith), a lane owns a run of four pixels of one output row (12 bytes, stored as 8 + 4), a wave
//   covers RPT rows and keeps the row-invariant products in registers.  Whether a frame is used (status, score against
//   max_score) is decided on the device: blockIdx.z is the frame, so the decision is uniform in a workgroup.
// * topview_accum_kernel / topview_finish_kernel: the court mosaic of a clip.  One thread owns one court pixel and walks the
//   frames in batch order, so the integer sums need no atomics and the B rectified images are never written.
// * map_points_kernel: arbitrary points through per-frame homographies in fp64 (cv2.perspectiveTransform's published rule),
//   one thread per point.
#include <float.h>

#include "common.h"
#include "warp_coords.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// an invalid tap's offset: beyond any descriptor's num_records and far enough from 2^32 that the channel offsets +1, +2 of a
// tap cannot wrap - the load returns 0 (grid_sample's zeros padding)
constexpr unsigned kByteOOB = 0xFFFFFF00u;

__global__ __launch_bounds__(64) void theta_invert_kernel(const float* __restrict__ theta, int batch, float* __restrict__ out,
                                                         uint8_t* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  Homog Hi;
  const double det = inverse_h33(theta + b * 9, Hi);
  bool ok = fabs(det) < (double)INFINITY && det != 0.0;          // false for NaN
#pragma unroll
  for (int k = 0; k < 9; ++k) ok &= fabsf(theta[b * 9 + k]) < INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[b * 9 + k] = ok ? Hi.t[k] : 0.f;
  status[b] = ok ? 1 : 0;
}

// status 0, a NaN score or a score above max_score: the frame is not used (score NULL: no gate)
__device__ __forceinline__ bool frame_used(const uint8_t* __restrict__ status, const float* __restrict__ score, float max_score,
                                           int b) {
  bool use = status[b] != 0;
  if (score) use &= score[b] <= max_score;      // false for NaN
  return use;
}

__device__ __forceinline__ unsigned ld_u8(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)off, 0, 0);
}

// the three bytes of a tap as floats
struct Px3 {
  float c[3];
};

__device__ __forceinline__ Px3 ld_px(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  Px3 p;
  p.c[0] = (float)ld_u8(rs, off);
  p.c[1] = (float)ld_u8(rs, off + 1u);
  p.c[2] = (float)ld_u8(rs, off + 2u);
  return p;
}

// MODE 0 nearest, 1 bilinear.  VEC: wc % 4 == 0 and 4-byte aligned outputs - a lane's four pixels are 12 bytes of the
// top view and one of `valid`; otherwise byte stores.
template <int MODE, int RPT, bool VEC, int LEVEL, bool SMALL>
__device__ __forceinline__ void topview_body(const float (&t)[9], int b, int lane, int c0, int r0,
                                             const uint8_t* __restrict__ frames, int H, int W, int hc, int wc, float rdw,
                                             float rdh, uint8_t* __restrict__ top, uint8_t* __restrict__ valid) {
  float a0[4], a3[4], a6[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + j;
    const float xn = norm_axis2<SMALL>(c < wc ? c : wc - 1, wc, rdw);
    a0[j] = __fmul_rn(t[0], xn);
    a3[j] = __fmul_rn(t[3], xn);
    a6[j] = __fmul_rn(t[6], xn);
  }
  // lane rr holds the row constants of row r0 + rr
  const int rl = r0 + (lane & (RPT - 1));
  const float ynl = norm_axis2<SMALL>(rl < hc ? rl : hc - 1, hc, rdh);
  const float c1l = __fmul_rn(t[1], ynl), c4l = __fmul_rn(t[4], ynl), c7l = __fmul_rn(t[7], ynl);
  const int nrows = (hc - r0 < RPT) ? hc - r0 : RPT;
  const long rowbase = ((long)b * hc + r0) * wc;
  const __amdgpu_buffer_rsrc_t rf =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(frames + (long)b * H * W * 3), 0, H * W * 3, 0x00020000);
  const __amdgpu_buffer_rsrc_t rtop = __builtin_amdgcn_make_buffer_rsrc(top + rowbase * 3, 0, nrows * wc * 3, 0x00020000);
  const __amdgpu_buffer_rsrc_t rval = __builtin_amdgcn_make_buffer_rsrc(valid + rowbase, 0, nrows * wc, 0x00020000);
  const float sx = 0.5f * (float)W, sy = 0.5f * (float)H;
#pragma unroll
  for (int rr = 0; rr < RPT; ++rr) {
    if (rr >= nrows) break;                 // wave-uniform
    const float c1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c1l), rr));
    const float c4 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c4l), rr));
    const float c7 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c7l), rr));
    unsigned px3[4][3], vld[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float X = __fadd_rn(__fadd_rn(a0[j], c1), t[2]);
      const float Y = __fadd_rn(__fadd_rn(a3[j], c4), t[5]);
      const float Z = __fadd_rn(__fadd_rn(a6[j], c7), t[8]);
      const float r = recip_rn<LEVEL>(__fadd_rn(Z, 1e-8f));
      const float s = (LEVEL == 2 || fabsf(Z) > 1e-8f) ? r : 1.0f;
      // unnorm(): fma(fl(u + 1), size/2, -0.5)
      const float px = __builtin_fmaf(__fadd_rn(__fmul_rn(s, X), 1.0f), sx, -0.5f);
      const float py = __builtin_fmaf(__fadd_rn(__fmul_rn(s, Y), 1.0f), sy, -0.5f);
      int ix, iy;
      const bool ok = tap_xy<LEVEL>(rintf(px), rintf(py), W, H, ix, iy);
      vld[j] = ok ? 255u : 0u;
      if (MODE == 0) {
        const unsigned off = ok ? (unsigned)(iy * W + ix) * 3u : kByteOOB;      // H * W < 2^24 (checked by the launcher)
        px3[j][0] = ld_u8(rf, off);
        px3[j][1] = ld_u8(rf, off + 1u);
        px3[j][2] = ld_u8(rf, off + 2u);
      } else {
        float qx = px, qy = py;
        if (LEVEL == 0) {   // the oracle's nan_to_num + clamp; finite coordinates give the same bytes without it
          qx = (px != px) ? -10.0f : px;
          qy = (py != py) ? -10.0f : py;
          qx = fminf(fmaxf(qx, -4.0f), (float)W + 3.0f);
          qy = fminf(fmaxf(qy, -4.0f), (float)H + 3.0f);
        }
        const float x0 = floorf(qx), y0 = floorf(qy);
        const float wx1 = __fsub_rn(qx, x0), wx0 = __fsub_rn(1.0f, wx1);
        const float wy1 = __fsub_rn(qy, y0), wy0 = __fsub_rn(1.0f, wy1);
        // x0, y0 finite: saturating conversions; validity masks every use, a wrapped offset is never used
        const int jx = (int)x0, jy = (int)y0;
        const unsigned ux = (unsigned)jx, uy = (unsigned)jy, uw = (unsigned)W, uh = (unsigned)H;
        const unsigned o00 = (unsigned)(__mul24(jy, W) + jx) * 3u;
        const Px3 t00 = ld_px(rf, (ux < uw && uy < uh) ? o00 : kByteOOB);
        const Px3 t01 = ld_px(rf, (ux + 1u < uw && uy < uh) ? o00 + 3u : kByteOOB);
        const Px3 t10 = ld_px(rf, (ux < uw && uy + 1u < uh) ? o00 + uw * 3u : kByteOOB);
        const Px3 t11 = ld_px(rf, (ux + 1u < uw && uy + 1u < uh) ? o00 + uw * 3u + 3u : kByteOOB);
        const float w00 = __fmul_rn(wy0, wx0), w01 = __fmul_rn(wy0, wx1), w10 = __fmul_rn(wy1, wx0), w11 = __fmul_rn(wy1, wx1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float v = __fmul_rn(t00.c[c], w00);
          v = __fadd_rn(v, __fmul_rn(t01.c[c], w01));
          v = __fadd_rn(v, __fmul_rn(t10.c[c], w10));
          v = __fadd_rn(v, __fmul_rn(t11.c[c], w11));
          px3[j][c] = (unsigned)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
        }
      }
    }
    if (VEC) {
      if (c0 < wc) {                        // wc % 4 == 0: a lane's four pixels are inside the row together
        // 8 + 4 bytes, not one 12-byte store: with the row offset in a scalar register the compiler puts no wait state
        // between a 12-byte buffer store and the next vector instruction that overwrites its data registers, and on the
        // MI355X the store was then seen to write the overwritten value (about 2 % of the first dwords of the bilinear
        // RPT = 8 instantiation); stores of at most 8 bytes have no such hazard
        const u32x2 d01 = {px3[0][0] | (px3[0][1] << 8) | (px3[0][2] << 16) | (px3[1][0] << 24),
                           px3[1][1] | (px3[1][2] << 8) | (px3[2][0] << 16) | (px3[2][1] << 24)};
        __builtin_amdgcn_raw_buffer_store_b64(d01, rtop, c0 * 3, rr * wc * 3, 0);
        __builtin_amdgcn_raw_buffer_store_b32(px3[2][2] | (px3[3][0] << 8) | (px3[3][1] << 16) | (px3[3][2] << 24), rtop,
                                              c0 * 3 + 8, rr * wc * 3, 0);
        __builtin_amdgcn_raw_buffer_store_b32(vld[0] | (vld[1] << 8) | (vld[2] << 16) | (vld[3] << 24), rval, c0, rr * wc, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c0 + j < wc) {
          const int o = (rr * wc + c0 + j) * 3;
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)px3[j][0], rtop, o, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)px3[j][1], rtop, o + 1, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)px3[j][2], rtop, o + 2, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)vld[j], rval, rr * wc + c0 + j, 0, 0);
        }
      }
    }
  }
}

template <int MODE, int RPT, bool VEC>
__global__ __launch_bounds__(256) void topview_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                      const float* __restrict__ theta_c2f, const uint8_t* __restrict__ status,
                                                      const float* __restrict__ score, float max_score, int hc, int wc,
                                                      float rdw, float rdh, uint8_t* __restrict__ top,
                                                      uint8_t* __restrict__ valid) {
  static_assert((RPT & (RPT - 1)) == 0 && RPT <= 64, "RPT: power of two");
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z;
  const int c0 = (blockIdx.x * 64 + lane) * 4;
  const int r0 = (blockIdx.y * 4 + wv) * RPT;
  if (r0 >= hc) return;
  if (!frame_used(status, score, max_score, b)) {      // frame-uniform: zeros and valid 0
    const int nrows = (hc - r0 < RPT) ? hc - r0 : RPT;
    for (int rr = 0; rr < nrows; ++rr) {
      const long p = ((long)b * hc + r0 + rr) * wc + c0;
      if (VEC) {
        if (c0 < wc) {
          uint32_t* o = reinterpret_cast<uint32_t*>(top + p * 3);
          o[0] = 0u;
          o[1] = 0u;
          o[2] = 0u;
          *reinterpret_cast<uint32_t*>(valid + p) = 0u;
        }
      } else {
        for (int j = 0; j < 4 && c0 + j < wc; ++j) {
          top[(p + j) * 3] = 0;
          top[(p + j) * 3 + 1] = 0;
          top[(p + j) * 3 + 2] = 0;
          valid[p + j] = 0;
        }
      }
    }
    return;
  }
  float t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = theta_c2f[b * 9 + k];
  bool fin, live;
  theta_class(t, fin, live);
#define SFH_TOPVIEW_GO(LEVEL, SMALL) \
  topview_body<MODE, RPT, VEC, LEVEL, SMALL>(t, b, lane, c0, r0, frames, H, W, hc, wc, rdw, rdh, top, valid)
  if (fin) {                                            // hc, wc <= 16384: checked by the launcher
    if (live) SFH_TOPVIEW_GO(2, true); else SFH_TOPVIEW_GO(1, true);
  } else {
    SFH_TOPVIEW_GO(0, false);
  }
#undef SFH_TOPVIEW_GO
}

// One thread = one court pixel over the B frames in batch order: sum += the nearest tap's bytes, count += 1 for every used
// frame whose tap is inside the frame.  The coordinates are those of topview_kernel bit for bit (plain IEEE forms of
// warp_coords.h; the fast reciprocal where the frame's theta admits it is the same correctly rounded quotient).
__global__ __launch_bounds__(256) void topview_accum_kernel(const uint8_t* __restrict__ frames, int batch, int H, int W,
                                                            const float* __restrict__ theta_c2f,
                                                            const uint8_t* __restrict__ status, const float* __restrict__ score,
                                                            float max_score, int hc, int wc, uint32_t* __restrict__ sum,
                                                            uint32_t* __restrict__ count) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= hc * wc) return;
  const int y = idx / wc, x = idx - y * wc;
  const float xn = norm_axis(x, wc), yn = norm_axis(y, hc);
  uint32_t s0 = 0, s1 = 0, s2 = 0, n = 0;
  for (int b = 0; b < batch; ++b) {
    if (!frame_used(status, score, max_score, b)) continue;     // uniform
    float t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = theta_c2f[b * 9 + k];
    bool fin, live;
    theta_class(t, fin, live);
    const float X = __fadd_rn(__fadd_rn(__fmul_rn(t[0], xn), __fmul_rn(t[1], yn)), t[2]);
    const float Y = __fadd_rn(__fadd_rn(__fmul_rn(t[3], xn), __fmul_rn(t[4], yn)), t[5]);
    const float Z = __fadd_rn(__fadd_rn(__fmul_rn(t[6], xn), __fmul_rn(t[7], yn)), t[8]);
    const float zz = __fadd_rn(Z, 1e-8f);
    const float r = fin ? recip_rn<1>(zz) : __fdiv_rn(1.0f, zz);
    const float s = (fabsf(Z) > 1e-8f) ? r : 1.0f;
    const float px = unnorm(__fmul_rn(s, X), W), py = unnorm(__fmul_rn(s, Y), H);
    int ix, iy;
    if (tap_xy<0>(rintf(px), rintf(py), W, H, ix, iy)) {
      const uint8_t* f = frames + ((long)b * H * W + (long)iy * W + ix) * 3;
      s0 += f[0];
      s1 += f[1];
      s2 += f[2];
      n += 1;
    }
  }
  if (n) {
    sum[(long)idx * 3] += s0;
    sum[(long)idx * 3 + 1] += s1;
    sum[(long)idx * 3 + 2] += s2;
    count[idx] += n;
  }
}

// image = round-half-up(sum / count) as (2 * sum + count) / (2 * count) in 64-bit integers; 0 where count == 0
__global__ __launch_bounds__(256) void topview_finish_kernel(const uint32_t* __restrict__ sum, const uint32_t* __restrict__ count,
                                                             int npix, uint8_t* __restrict__ image) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix) return;
  const uint64_t n = count[idx];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint64_t q = n ? (2ull * sum[(long)idx * 3 + c] + n) / (2ull * n) : 0ull;
    image[(long)idx * 3 + c] = (uint8_t)(q > 255ull ? 255ull : q);
  }
}

// One thread = one point.  Every fp64 operation is individually rounded (-ffp-contract=off).
__global__ __launch_bounds__(256) void map_points_kernel(const float* __restrict__ points, const int32_t* __restrict__ frame_index,
                                                         int frame0, long n, const float* __restrict__ thetas, int nframes,
                                                         float in_w, float in_h, double sx, double sy, float* __restrict__ out,
                                                         uint8_t* __restrict__ flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int f = frame_index ? frame_index[i] : frame0;
  float ou = 0.f, ov = 0.f;
  bool ok = f >= 0 && f < nframes;
  if (ok) {
    float x = points[2 * i], y = points[2 * i + 1];
    if (in_w != 0.f) {        // transform.py:38-39 on its float32 array
      x = __fmul_rn(__fsub_rn(__fdiv_rn(x, in_w), 0.5f), 2.0f);
      y = __fmul_rn(__fsub_rn(__fdiv_rn(y, in_h), 0.5f), 2.0f);
    }
    const float* t = thetas + (long)f * 9;
    const double xd = (double)x, yd = (double)y;
    const double X = ((double)t[0] * xd + (double)t[1] * yd) + (double)t[2];
    const double Y = ((double)t[3] * xd + (double)t[4] * yd) + (double)t[5];
    const double Wh = ((double)t[6] * xd + (double)t[7] * yd) + (double)t[8];
    const double wi = fabs(Wh) > (double)FLT_EPSILON ? 1.0 / Wh : 0.0;      // cv2.perspectiveTransform
    ou = (float)(((X * wi) / 2.0 + 0.5) * sx);
    ov = (float)(((Y * wi) / 2.0 + 0.5) * sy);
    ok = wi != 0.0 && fabsf(ou) < INFINITY && fabsf(ov) < INFINITY;          // false for NaN
  }
  out[2 * i] = ok ? ou : 0.f;
  out[2 * i + 1] = ok ? ov : 0.f;
  flag[i] = ok ? 1 : 0;
}

}  // namespace

extern "C" int sfh_theta_invert(const float* theta, int batch, float* theta_c2f, uint8_t* status, void* stream) {
  SFH_REQUIRE(theta && theta_c2f && status, "theta_invert: null pointer (theta, theta_c2f, status)");
  SFH_REQUIRE(batch > 0 && batch <= (1 << 24), "theta_invert: batch %d", batch);
  hipLaunchKernelGGL(theta_invert_kernel, dim3((unsigned)sfh_cdiv(batch, 64)), dim3(64), 0, (hipStream_t)stream, theta, batch,
                     theta_c2f, status);
  return sfh_check_launch("theta_invert_kernel");
}

// shared argument checks of the render and the accumulation
static int topview_check(const char* who, const void* frames, const void* theta_c2f, const void* status, int batch, int H, int W,
                         const float* score, float max_score, int hc, int wc) {
  SFH_REQUIRE(frames && theta_c2f && status, "%s: null pointer (frames, theta_c2f, status)", who);
  SFH_REQUIRE(batch > 0 && batch <= 65535, "%s: batch %d (1 .. 65535)", who, batch);
  SFH_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1 << 24), "%s: frame %dx%d (H * W below 2^24)", who, W, H);
  SFH_REQUIRE(hc > 1 && wc > 1 && hc <= 16384 && wc <= 16384, "%s: court view %dx%d (2 .. 16384 per side)", who, wc, hc);
  SFH_REQUIRE(!score || max_score == max_score, "%s: max_score is NaN", who);
  return SFH_OK;
}

extern "C" int sfh_topview_render(const uint8_t* frames, int batch, int H, int W, const float* theta_c2f, const uint8_t* status,
                                  const float* score, float max_score, int hc, int wc, int mode, uint8_t* top_view,
                                  uint8_t* valid, void* stream) {
  if (int rc = topview_check("topview_render", frames, theta_c2f, status, batch, H, W, score, max_score, hc, wc)) return rc;
  SFH_REQUIRE(top_view && valid, "topview_render: null pointer (top_view, valid)");
  SFH_REQUIRE(mode == 0 || mode == 1, "topview_render: mode %d (0 nearest, 1 bilinear)", mode);
  const float rdw = 1.0f / (float)(wc - 1), rdh = 1.0f / (float)(hc - 1);   // IEEE single divisions
  const long segs = (long)sfh_cdiv(wc, 256) * batch;
  int rpt = 8;
  while (rpt > 2 && segs * sfh_cdiv(hc, rpt) < 4096) rpt >>= 1;
  const bool vec = wc % 4 == 0 && (((uintptr_t)top_view | (uintptr_t)valid) & 3) == 0;
  const dim3 grid((unsigned)sfh_cdiv(wc, 256), (unsigned)sfh_cdiv(hc, 4 * rpt), (unsigned)batch);
#define SFH_TV(M, RR, V)                                                                                                  \
  hipLaunchKernelGGL((topview_kernel<M, RR, V>), grid, dim3(256), 0, (hipStream_t)stream, frames, H, W, theta_c2f, status, \
                     score, max_score, hc, wc, rdw, rdh, top_view, valid)
#define SFH_TV_V(M, RR) do { if (vec) SFH_TV(M, RR, true); else SFH_TV(M, RR, false); } while (0)
#define SFH_TV_R(M)                 \
  do {                              \
    if (rpt == 8) SFH_TV_V(M, 8);   \
    else if (rpt == 4) SFH_TV_V(M, 4); \
    else SFH_TV_V(M, 2);            \
  } while (0)
  if (mode == 0) SFH_TV_R(0);
  else SFH_TV_R(1);
#undef SFH_TV_R
#undef SFH_TV_V
#undef SFH_TV
  return sfh_check_launch("topview_kernel");
}

extern "C" int sfh_topview_accumulate(const uint8_t* frames, int batch, int H, int W, const float* theta_c2f,
                                      const uint8_t* status, const float* score, float max_score, int hc, int wc, uint32_t* sum,
                                      uint32_t* count, void* stream) {
  if (int rc = topview_check("topview_accumulate", frames, theta_c2f, status, batch, H, W, score, max_score, hc, wc)) return rc;
  SFH_REQUIRE(sum && count, "topview_accumulate: null pointer (sum, count)");
  hipLaunchKernelGGL(topview_accum_kernel, dim3((unsigned)sfh_cdiv(hc * wc, 256)), dim3(256), 0, (hipStream_t)stream, frames, batch,
                     H, W, theta_c2f, status, score, max_score, hc, wc, sum, count);
  return sfh_check_launch("topview_accum_kernel");
}

extern "C" int sfh_topview_finish(const uint32_t* sum, const uint32_t* count, int hc, int wc, uint8_t* image, void* stream) {
  SFH_REQUIRE(sum && count && image, "topview_finish: null pointer (sum, count, image)");
  SFH_REQUIRE(hc > 0 && wc > 0 && hc <= 16384 && wc <= 16384, "topview_finish: court view %dx%d (1 .. 16384 per side)", wc, hc);
  hipLaunchKernelGGL(topview_finish_kernel, dim3((unsigned)sfh_cdiv(hc * wc, 256)), dim3(256), 0, (hipStream_t)stream, sum, count,
                     hc * wc, image);
  return sfh_check_launch("topview_finish_kernel");
}

extern "C" int sfh_map_points(const float* points, const int32_t* frame_index, int frame0, int64_t n, const float* thetas,
                              int nframes, float in_w, float in_h, double out_sx, double out_sy, float* out, uint8_t* flag,
                              void* stream) {
  SFH_REQUIRE(points && thetas && out && flag, "map_points: null pointer (points, thetas, out, flag)");
  SFH_REQUIRE(n > 0 && n <= ((int64_t)1 << 30), "map_points: %lld points (1 .. 2^30)", (long long)n);
  SFH_REQUIRE(nframes > 0, "map_points: theta table of %d frames", nframes);
  SFH_REQUIRE((in_w == 0.f && in_h == 0.f) || (in_w > 0.f && in_h > 0.f && in_w < INFINITY && in_h < INFINITY),
              "map_points: in_size %g x %g (positive, or 0 x 0 for normalised input)", (double)in_w, (double)in_h);
  SFH_REQUIRE(fabs(out_sx) < (double)INFINITY && fabs(out_sy) < (double)INFINITY, "map_points: out_scale %g x %g is not finite",
              out_sx, out_sy);
  hipLaunchKernelGGL(map_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, frame_index,
                     frame0, (long)n, thetas, nframes, in_w, in_h, out_sx, out_sy, out, flag);
  return sfh_check_launch("map_points_kernel");
}
