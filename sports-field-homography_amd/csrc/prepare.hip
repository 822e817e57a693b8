// prepare.hip - training labels from manual POI annotations: the reference's dataset_utils/preparation.py
// (calculate_homography -> projected POI -> calculate_reprojection_rmse -> mask from template and homography ->
// convert_rgb_to_onehot), which runs OpenCV on the CPU one frame at a time.
//
// * prep_fit_kernel: one wave per frame, four frames per workgroup.  Lanes run across the points for every sum over points
//   (slot = point index mod 64, slots combined by an xor butterfly: every lane ends with the same bits, no atomics); the
//   9 x 9 Jacobi eigen-solve lives in LDS with lanes 0..8 across the rows / columns of a rotation; the 8 x 8 Gauss-Newton
//   system is solved redundantly by every lane in registers (chol8_solve, chol8.h).  All fp64, individually rounded
//   (-ffp-contract=off): the numpy restatement tests/prep_ref.py follows the same order of operations.
// * prep_render_kernel: the nearest warp of the uint8 id image with warp.hip's coordinate arithmetic (warp_coords.h: the
//   same functions, so the tap is the same), four consecutive pixels per lane: one 4-byte mask store and three 8-byte uv
//   stores per lane and row, a wave writes 256 / 1536 consecutive bytes.  Taps go through buffer descriptors: an invalid
//   tap reads 0 from the id image and both tables.
// * prep_rgb_to_ids_kernel: 12 bytes in, 4 bytes out per thread.
#include "common.h"
#include "warp_coords.h"
#include "chol8.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kFitWaves = 4;                          // frames per workgroup
constexpr int kPer = SFH_PREP_MAX_POINTS / 64;        // points per lane at most
constexpr int kSums = 45;                             // upper triangle of 9 x 9 = upper triangle of 8 x 8 + 8 + 1

__global__ __launch_bounds__(64 * kFitWaves) void prep_fit_kernel(
    const double* __restrict__ court, const double* __restrict__ manual, const uint8_t* __restrict__ ignore, int batch,
    int npts, double norm_w, double norm_h, int refine, double* __restrict__ theta_c2f, double* __restrict__ theta,
    float* __restrict__ theta_f32, double* __restrict__ poi, int32_t* __restrict__ num_nonzero, double* __restrict__ rmse,
    int32_t* __restrict__ status) {
  __shared__ double As[kFitWaves][81], Vs[kFitWaves][81];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bq = blockIdx.x * kFitWaves + wv;
  const bool active = bq < batch;                     // wave-uniform; an idle wave walks through the barriers on frame 0
  const int b = active ? bq : 0;
  double* A = As[wv];
  double* V = Vs[wv];

  // ---- this lane's points
  double tx[kPer], ty[kPer], mx[kPer], my[kPer], fx[kPer], fy[kPer];
  bool use[kPer], flag[kPer];
  double cnt = 0.0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = lane + 64 * k;
    const bool in = i < npts;
    tx[k] = in ? court[2 * i] : 0.0;
    ty[k] = in ? court[2 * i + 1] : 0.0;
    mx[k] = in ? manual[((long)b * npts + i) * 2] : -1.0;
    my[k] = in ? manual[((long)b * npts + i) * 2 + 1] : -1.0;
    fx[k] = mx[k] * 2.0 - 1.0;
    fy[k] = my[k] * 2.0 - 1.0;
    use[k] = in && mx[k] != -1.0 && my[k] != -1.0;
    flag[k] = in && !(ignore && ignore[i]) && !(mx[k] == -1.0 && my[k] == -1.0);
    cnt += use[k] ? 1.0 : 0.0;
  }
  const double n = wave_sum_all(cnt);
  const bool fitted = n >= 4.0;
  const double nd = fitted ? n : 1.0;

  // ---- Hartley normalisation of both sets
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    s4[0] += use[k] ? tx[k] : 0.0;
    s4[1] += use[k] ? ty[k] : 0.0;
    s4[2] += use[k] ? fx[k] : 0.0;
    s4[3] += use[k] ? fy[k] : 0.0;
  }
  const double cx1 = wave_sum_all(s4[0]) / nd, cy1 = wave_sum_all(s4[1]) / nd;
  const double cx2 = wave_sum_all(s4[2]) / nd, cy2 = wave_sum_all(s4[3]) / nd;
  double d1 = 0.0, d2 = 0.0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const double ax = tx[k] - cx1, ay = ty[k] - cy1, bx = fx[k] - cx2, by = fy[k] - cy2;
    d1 += use[k] ? sqrt(ax * ax + ay * ay) : 0.0;
    d2 += use[k] ? sqrt(bx * bx + by * by) : 0.0;
  }
  const double sc1 = sqrt(2.0) / (wave_sum_all(d1) / nd), sc2 = sqrt(2.0) / (wave_sum_all(d2) / nd);

  // ---- L^T L over the usable points
  double acc[kSums];
#pragma unroll
  for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (64 * k >= npts) break;              // wave-uniform: the slots beyond hold no point
    const double x = (tx[k] - cx1) * sc1, y = (ty[k] - cy1) * sc1, u = (fx[k] - cx2) * sc2, v = (fy[k] - cy2) * sc2;
    const double r1[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
    const double r2[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = i; j < 9; ++j, ++e) {
        const double term = r1[i] * r1[j] + r2[i] * r2[j];
        acc[e] += use[k] ? term : 0.0;
      }
  }
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = i; j < 9; ++j, ++e) {
        const double s = wave_sum_all(acc[e]);
        if (lane == 0) {
          A[i * 9 + j] = s;
          A[j * 9 + i] = s;
        }
      }
  }
  for (int e = lane; e < 81; e += 64) V[e] = (e / 9 == e % 9) ? 1.0 : 0.0;
  __syncthreads();

  // ---- cyclic Jacobi: A <- P^T A P, V <- V P with P = [[c, s], [-s, c]] on (p, q); lanes 0..8 across k
  for (int sweep = 0; sweep < SFH_PREP_JACOBI_SWEEPS; ++sweep)
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double app = A[p * 9 + p], aqq = A[q * 9 + q], apq = A[p * 9 + q];
        double c = 1.0, s = 0.0;
        if (apq != 0.0) {
          const double th = (aqq - app) / (2.0 * apq);
          const double t = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        if (lane < 9) {
          const int k = lane;
          const double akp = A[k * 9 + p], akq = A[k * 9 + q], vkp = V[k * 9 + p], vkq = V[k * 9 + q];
          A[k * 9 + p] = c * akp - s * akq;
          A[k * 9 + q] = s * akp + c * akq;
          V[k * 9 + p] = c * vkp - s * vkq;
          V[k * 9 + q] = s * vkp + c * vkq;
        }
        __syncthreads();
        if (lane < 9) {
          const int k = lane;
          const double apk = A[p * 9 + k], aqk = A[q * 9 + k];
          const double np_ = c * apk - s * aqk, nq_ = s * apk + c * aqk;
          A[p * 9 + k] = (k == q && apq != 0.0) ? 0.0 : np_;
          A[q * 9 + k] = (k == p && apq != 0.0) ? 0.0 : nq_;
        }
        __syncthreads();
      }
  int kmin = 0;
  double emin = A[0];
  for (int k = 1; k < 9; ++k) {
    const double ek = A[k * 9 + k];
    if (ek < emin) {
      emin = ek;
      kmin = k;
    }
  }
  double hn[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) hn[k] = V[k * 9 + kmin];

  // ---- denormalise: H = T2^-1 Hn T1, then / h33
  double h[9];
  {
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      M[r * 3 + 0] = hn[r * 3 + 0] * sc1;
      M[r * 3 + 1] = hn[r * 3 + 1] * sc1;
      M[r * 3 + 2] = hn[r * 3 + 2] - (M[r * 3 + 0] * cx1 + M[r * 3 + 1] * cy1);
    }
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      h[cc] = M[cc] / sc2 + cx2 * M[6 + cc];
      h[3 + cc] = M[3 + cc] / sc2 + cy2 * M[6 + cc];
      h[6 + cc] = M[6 + cc];
    }
    const double h33 = h[8];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = h[k] / h33;
  }

  // ---- damped Gauss-Newton on h[0..7] (h[8] = 1): cost = sum |proj(h, court) - frame|^2 over the usable points
  auto cost_of = [&](const double (&g)[9]) {
    double cs = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const double iw = 1.0 / ((g[6] * tx[k] + g[7] * ty[k]) + 1.0);
      const double rx = ((g[0] * tx[k] + g[1] * ty[k]) + g[2]) * iw - fx[k];
      const double ry = ((g[3] * tx[k] + g[4] * ty[k]) + g[5]) * iw - fy[k];
      cs += use[k] ? (rx * rx + ry * ry) : 0.0;
    }
    return wave_sum_all(cs);
  };
  double lambda = 1e-3;
  for (int it = 0; it < refine; ++it) {
#pragma unroll
    for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (64 * k >= npts) break;
      const double x = tx[k], y = ty[k];
      const double iw = 1.0 / ((h[6] * x + h[7] * y) + 1.0);
      const double px = ((h[0] * x + h[1] * y) + h[2]) * iw, py = ((h[3] * x + h[4] * y) + h[5]) * iw;
      const double rx = px - fx[k], ry = py - fy[k];
      const double xi = x * iw, yi = y * iw;
      const double jx[8] = {xi, yi, iw, 0.0, 0.0, 0.0, -(px * xi), -(px * yi)};
      const double jy[8] = {0.0, 0.0, 0.0, xi, yi, iw, -(py * xi), -(py * yi)};
      int e = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i; j < 8; ++j, ++e) {
          const double term = jx[i] * jx[j] + jy[i] * jy[j];
          acc[e] += use[k] ? term : 0.0;
        }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double term = jx[i] * rx + jy[i] * ry;
        acc[36 + i] += use[k] ? term : 0.0;
      }
      acc[44] += use[k] ? (rx * rx + ry * ry) : 0.0;
    }
#pragma unroll
    for (int e = 0; e < kSums; ++e) acc[e] = wave_sum_all(acc[e]);
    // (J^T J + lambda diag(J^T J)) delta = -J^T r by chol8.h; a pivot that is not positive rejects the step
    double Lm[8][8], gv[8];
    {
      int e = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i; j < 8; ++j, ++e) Lm[j][i] = (i == j) ? acc[e] + lambda * acc[e] : acc[e];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) gv[i] = -acc[36 + i];
    const bool ok = chol8_solve(Lm, gv, true);
    double hc[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) hc[i] = h[i] + gv[i];
    hc[8] = 1.0;
    const double c1 = cost_of(hc);
    if (ok && c1 < acc[44]) {              // wave-uniform: every lane holds the same bits
#pragma unroll
      for (int i = 0; i < 8; ++i) h[i] = hc[i];
      lambda = lambda / 10.0;
    } else {
      lambda = lambda * 10.0;
    }
  }

  // ---- outputs
  double inv[9];
  inv[0] = h[4] * h[8] - h[5] * h[7];
  inv[1] = h[2] * h[7] - h[1] * h[8];
  inv[2] = h[1] * h[5] - h[2] * h[4];
  inv[3] = h[5] * h[6] - h[3] * h[8];
  inv[4] = h[0] * h[8] - h[2] * h[6];
  inv[5] = h[2] * h[3] - h[0] * h[5];
  inv[6] = h[3] * h[7] - h[4] * h[6];
  inv[7] = h[1] * h[6] - h[0] * h[7];
  inv[8] = h[0] * h[4] - h[1] * h[3];
  const double i33 = inv[8];
#pragma unroll
  for (int k = 0; k < 9; ++k) inv[k] = inv[k] / i33;
  double nz = 0.0, ds = 0.0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = lane + 64 * k;
    const double X = (h[0] * tx[k] + h[1] * ty[k]) + h[2];
    const double Y = (h[3] * tx[k] + h[4] * ty[k]) + h[5];
    const double Z = (h[6] * tx[k] + h[7] * ty[k]) + h[8];
    const double s = fabs(Z) > 1e-8 ? 1.0 / (Z + 1e-8) : 1.0;
    const double pu = (s * X) / 2.0 + 0.5, pv = (s * Y) / 2.0 + 0.5;
    const double ex = pu * norm_w - mx[k] * norm_w, ey = pv * norm_h - my[k] * norm_h;
    const double f = flag[k] ? 1.0 : 0.0;
    nz += f;
    ds += (i < npts) ? sqrt(ex * ex + ey * ey) * f : 0.0;
    if (active && i < npts) {
      double* o = poi + ((long)b * npts + i) * 3;
      o[0] = fitted ? pu : 0.0;
      o[1] = fitted ? pv : 0.0;
      o[2] = fitted ? f : 0.0;
    }
  }
  nz = wave_sum_all(nz);
  ds = wave_sum_all(ds);
  if (active && lane < 9) {
    theta_c2f[b * 9 + lane] = fitted ? h[lane] : 0.0;
    theta[b * 9 + lane] = fitted ? inv[lane] : 0.0;
    if (theta_f32) theta_f32[b * 9 + lane] = fitted ? (float)inv[lane] : 0.0f;
  }
  if (active && lane == 0) {
    num_nonzero[b] = fitted ? (int32_t)nz : 0;
    rmse[b] = fitted ? ds / nz : 0.0;
    status[b] = fitted ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ label rendering
// A wave covers 256 consecutive pixels (lane -> pixels 4 * lane .. + 3) of RPT rows; the row-invariant products and the
// row constants are kept as warp2_body (warp.hip) keeps them, so a homogeneous coordinate costs two additions per pixel.
template <int RPT, bool UV, int LEVEL, bool SMALL>
__device__ __forceinline__ void render_body(const float (&t)[9], int b, int lane, int c0, int r0,
                                            const uint8_t* __restrict__ ids, const uint16_t* __restrict__ utab,
                                            const uint16_t* __restrict__ vtab, int hs, int ws, int h, int w, float rdw,
                                            float rdh, uint8_t* __restrict__ mask, uint16_t* __restrict__ uv) {
  float a0[4], a3[4], a6[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + j;
    const float xn = norm_axis2<SMALL>(c < w ? c : w - 1, w, rdw);
    a0[j] = __fmul_rn(t[0], xn);
    a3[j] = __fmul_rn(t[3], xn);
    a6[j] = __fmul_rn(t[6], xn);
  }
  const int rl = r0 + (lane & (RPT - 1));
  const float ynl = norm_axis2<SMALL>(rl < h ? rl : h - 1, h, rdh);
  const float c1l = __fmul_rn(t[1], ynl), c4l = __fmul_rn(t[4], ynl), c7l = __fmul_rn(t[7], ynl);
  const int nrows = (h - r0 < RPT) ? h - r0 : RPT;
  const long rowbase = ((long)b * h + r0) * w;
  const __amdgpu_buffer_rsrc_t rid = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(ids), 0, hs * ws, 0x00020000);
  const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(utab), 0, UV ? ws * 2 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(vtab), 0, UV ? hs * 2 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(mask + rowbase, 0, nrows * w, 0x00020000);
  const __amdgpu_buffer_rsrc_t ruv =
      __builtin_amdgcn_make_buffer_rsrc(UV ? uv + rowbase * 3 : nullptr, 0, UV ? nrows * w * 6 : 0, 0x00020000);
  const float sx = 0.5f * (float)ws, sy = 0.5f * (float)hs;
  const bool cols = c0 < w;                 // w % 4 == 0: a lane's four pixels are inside the row together
#pragma unroll
  for (int rr = 0; rr < RPT; ++rr) {
    if (rr >= nrows) break;                 // wave-uniform
    const float c1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c1l), rr));
    const float c4 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c4l), rr));
    const float c7 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c7l), rr));
    unsigned id[4], uu[4], vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float X = __fadd_rn(__fadd_rn(a0[j], c1), t[2]);
      const float Y = __fadd_rn(__fadd_rn(a3[j], c4), t[5]);
      const float Z = __fadd_rn(__fadd_rn(a6[j], c7), t[8]);
      const float r = recip_rn<LEVEL>(__fadd_rn(Z, 1e-8f));
      const float s = (LEVEL == 2 || fabsf(Z) > 1e-8f) ? r : 1.0f;
      const float px = __builtin_fmaf(__fadd_rn(__fmul_rn(s, X), 1.0f), sx, -0.5f);
      const float py = __builtin_fmaf(__fadd_rn(__fmul_rn(s, Y), 1.0f), sy, -0.5f);
      int ix, iy;
      const bool ok = tap_xy<LEVEL>(rintf(px), rintf(py), ws, hs, ix, iy) && cols;
      id[j] = __builtin_amdgcn_raw_buffer_load_b8(rid, ok ? iy * ws + ix : (int)kTapOOB, 0, 0);
      if (UV) {
        uu[j] = __builtin_amdgcn_raw_buffer_load_b16(ru, ok ? ix * 2 : (int)kTapOOB, 0, 0);
        vv[j] = __builtin_amdgcn_raw_buffer_load_b16(rv, ok ? iy * 2 : (int)kTapOOB, 0, 0);
      }
    }
    if (!cols) continue;                    // nothing below depends on the range check of a store
    __builtin_amdgcn_raw_buffer_store_b32(id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24), rm, c0, rr * w, 0);
    if (UV) {
      const int uoff = c0 * 6;
      const u32x2 d0 = {id[0] | (uu[0] << 16), vv[0] | (id[1] << 16)};
      const u32x2 d1 = {uu[1] | (vv[1] << 16), id[2] | (uu[2] << 16)};
      const u32x2 d2 = {vv[2] | (id[3] << 16), uu[3] | (vv[3] << 16)};
      __builtin_amdgcn_raw_buffer_store_b64(d0, ruv, uoff, rr * w * 6, 0);
      __builtin_amdgcn_raw_buffer_store_b64(d1, ruv, uoff + 8, rr * w * 6, 0);
      __builtin_amdgcn_raw_buffer_store_b64(d2, ruv, uoff + 16, rr * w * 6, 0);
    }
  }
}

template <int RPT, bool UV>
__global__ __launch_bounds__(256) void prep_render_kernel(const float* __restrict__ theta, const uint8_t* __restrict__ ids,
                                                          const uint16_t* __restrict__ utab,
                                                          const uint16_t* __restrict__ vtab, int hs, int ws, int h, int w,
                                                          float rdw, float rdh, uint8_t* __restrict__ mask,
                                                          uint16_t* __restrict__ uv) {
  static_assert((RPT & (RPT - 1)) == 0 && RPT <= 64, "RPT: power of two");
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z;
  const int c0 = (blockIdx.x * 64 + lane) * 4;
  const int r0 = (blockIdx.y * 4 + wv) * RPT;
  if (r0 >= h) return;
  float t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = theta[b * 9 + k];
  bool fin, live;
  theta_class(t, fin, live);
#define SFH_RENDER_GO(LEVEL, SMALL) \
  render_body<RPT, UV, LEVEL, SMALL>(t, b, lane, c0, r0, ids, utab, vtab, hs, ws, h, w, rdw, rdh, mask, uv)
  if (fin && w <= 16384 && h <= 16384) {
    if (live) SFH_RENDER_GO(2, true); else SFH_RENDER_GO(1, true);
  } else {
    SFH_RENDER_GO(0, false);
  }
#undef SFH_RENDER_GO
}

// ------------------------------------------------------------------------------------------------ rgb -> ids
struct RgbTable {
  uint32_t c[8];     // colour k as byte0 | byte1 << 8 | byte2 << 16; entry 0 unused
  int n;
};

__device__ __forceinline__ uint32_t rgb_id(uint32_t px, const RgbTable& tb) {
  uint32_t r = px & 0xffu;
#pragma unroll
  for (int k = 1; k < 8; ++k) r = (k < tb.n && px == tb.c[k]) ? (uint32_t)k : r;
  return r;
}

__global__ __launch_bounds__(256) void prep_rgb_to_ids_kernel(const uint8_t* __restrict__ rgb, long npix, RgbTable tb,
                                                              uint8_t* __restrict__ out) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long p0 = q * 4;
  if (p0 >= npix) return;
  if (p0 + 4 <= npix) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rgb) + q * 3;
    const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
    const uint32_t a = w0 & 0xffffffu, bb = (w0 >> 24) | ((w1 & 0xffffu) << 8), c = (w1 >> 16) | ((w2 & 0xffu) << 16), d = w2 >> 8;
    reinterpret_cast<uint32_t*>(out)[q] = rgb_id(a, tb) | (rgb_id(bb, tb) << 8) | (rgb_id(c, tb) << 16) | (rgb_id(d, tb) << 24);
  } else {
    for (long p = p0; p < npix; ++p) {
      const uint32_t px = (uint32_t)rgb[p * 3] | ((uint32_t)rgb[p * 3 + 1] << 8) | ((uint32_t)rgb[p * 3 + 2] << 16);
      out[p] = (uint8_t)rgb_id(px, tb);
    }
  }
}

}  // namespace

extern "C" int sfh_prep_fit(const double* court_poi, const double* manual_poi, const uint8_t* ignore_mask, int batch,
                            int npts, double norm_w, double norm_h, int refine, double* theta_c2f, double* theta,
                            float* theta_f32, double* poi, int32_t* num_nonzero, double* rmse, int32_t* status,
                            void* stream) {
  SFH_REQUIRE(court_poi && manual_poi && theta_c2f && theta && poi && num_nonzero && rmse && status, "prep_fit: null pointer");
  SFH_REQUIRE(batch > 0 && batch <= (1 << 24), "prep_fit: batch %d", batch);
  SFH_REQUIRE(npts >= 4 && npts <= SFH_PREP_MAX_POINTS, "prep_fit: %d template points (4 .. %d)", npts, SFH_PREP_MAX_POINTS);
  SFH_REQUIRE(norm_w > 0.0 && norm_h > 0.0 && norm_w < 1e9 && norm_h < 1e9, "prep_fit: norm_size %g x %g (positive; 1 x 1 for none)",
              norm_w, norm_h);
  SFH_REQUIRE(refine >= 0 && refine <= 1000, "prep_fit: refine %d (0 .. 1000 Gauss-Newton steps)", refine);
  hipLaunchKernelGGL(prep_fit_kernel, dim3((unsigned)sfh_cdiv(batch, kFitWaves)), dim3(64 * kFitWaves), 0, (hipStream_t)stream,
                     court_poi, manual_poi, ignore_mask, batch, npts, norm_w, norm_h, refine, theta_c2f, theta, theta_f32, poi,
                     num_nonzero, rmse, status);
  return sfh_check_launch("prep_fit_kernel");
}

extern "C" int sfh_prep_render(const float* theta, const uint8_t* ids, int hs, int ws, const uint16_t* u_tab,
                               const uint16_t* v_tab, int batch, int H, int W, int want_uv, uint8_t* mask, uint16_t* uv,
                               void* stream) {
  SFH_REQUIRE(theta && ids && mask, "prep_render: null pointer (theta, ids, mask)");
  SFH_REQUIRE(!want_uv || (u_tab && v_tab && uv), "prep_render: uv requested without u_tab / v_tab / uv");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 1 && W > 1 && hs > 0 && ws > 0, "prep_render: bad geometry b=%d h=%d w=%d hs=%d ws=%d",
              batch, H, W, hs, ws);
  SFH_REQUIRE(W % 4 == 0, "prep_render: frame width %d is not a multiple of 4", W);
  SFH_REQUIRE((int64_t)hs * ws <= (1 << 22) && W <= (1 << 20) && H <= (1 << 20),
              "prep_render: template %dx%d (at most 4 Mi pixels) or frame %dx%d too large", ws, hs, W, H);
  const float rdw = 1.0f / (float)(W - 1), rdh = 1.0f / (float)(H - 1);   // IEEE single divisions
  const long segs = (long)sfh_cdiv(W, 256) * batch;
  int rpt = 8;
  while (rpt > 2 && segs * sfh_cdiv(H, rpt) < 4096) rpt >>= 1;
  const dim3 grid((unsigned)sfh_cdiv(W, 256), (unsigned)sfh_cdiv(H, 4 * rpt), (unsigned)batch);
#define SFH_RENDER_LAUNCH(RR, UU)                                                                                       \
  hipLaunchKernelGGL((prep_render_kernel<RR, UU>), grid, dim3(256), 0, (hipStream_t)stream, theta, ids, u_tab, v_tab, hs, ws, \
                     H, W, rdw, rdh, mask, uv)
#define SFH_RENDER_UV(RR) do { if (want_uv) SFH_RENDER_LAUNCH(RR, true); else SFH_RENDER_LAUNCH(RR, false); } while (0)
  if (rpt == 8) SFH_RENDER_UV(8);
  else if (rpt == 4) SFH_RENDER_UV(4);
  else SFH_RENDER_UV(2);
#undef SFH_RENDER_UV
#undef SFH_RENDER_LAUNCH
  return sfh_check_launch("prep_render_kernel");
}

extern "C" int sfh_prep_rgb_to_ids(const uint8_t* rgb, int64_t npix, int num_classes, uint8_t* ids, void* stream) {
  SFH_REQUIRE(rgb && ids, "prep_rgb_to_ids: null pointer");
  SFH_REQUIRE(npix > 0 && npix < ((int64_t)1 << 40), "prep_rgb_to_ids: %lld pixels", (long long)npix);
  SFH_REQUIRE(num_classes == 4 || num_classes == 7 || num_classes == 8,
              "prep_rgb_to_ids: no colour table for %d classes (4, 7, 8)", num_classes);
  SFH_REQUIRE(((uintptr_t)rgb & 3) == 0 && ((uintptr_t)ids & 3) == 0, "prep_rgb_to_ids: pointers must be 4-byte aligned");
  // utils/postprocess.py:29-51 = generate_onehot's mapping, bytes in the order given
  static const uint8_t kColours[8][3] = {{0, 0, 0},       {0, 255, 0},   {255, 0, 0},   {0, 0, 255},
                                         {255, 255, 255}, {255, 0, 255}, {0, 255, 255}, {255, 255, 0}};
  RgbTable tb;
  for (int k = 0; k < 8; ++k)
    tb.c[k] = (uint32_t)kColours[k][0] | ((uint32_t)kColours[k][1] << 8) | ((uint32_t)kColours[k][2] << 16);
  tb.n = num_classes;
  const int64_t quads = (npix + 3) / 4;
  hipLaunchKernelGGL(prep_rgb_to_ids_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb,
                     (long)npix, tb, ids);
  return sfh_check_launch("prep_rgb_to_ids_kernel");
}
