// metrics.hip - registration metrics per frame: confusion counts, region counts (IoU part / whole), point errors.  The rules
// are stated in include/sfh_amd.h above the three entries; tests/metrics_ref.py restates them in numpy.
//
//  sfh_metrics_confusion  the hot path: it streams the prediction (logits: nc planes) and the int64 mask once, 16 bytes per
//    lane and load where the frame allows it.  Neighbouring pixels almost always share their (g, p) key, so a per-pixel LDS
//    atomic would serialise on one bin.  Instead: per wave ONE step per distinct key present (ballot of the lanes that hold the
//    first pending key, popcount), the count of key k kept in a register of lane k (nc^2 <= 64 = the wave); per workgroup one
//    LDS word per key; across workgroups 64-bit integer atomic adds onto the output, which a first launch has cleared.  Integer
//    addition gives the same bits in any order, so the result is reproducible although the adds arrive in any order.
//  sfh_metrics_region     exact-integer raster, fp64 predicate, the two matrices formed once per workgroup (thread 0, LDS);
//    counts combined like the confusion's (ballot, LDS, integer atomics onto the cleared output).
//  sfh_metrics_points     one wave per frame, fp64, fixed order.
//
// This translation unit relies on -ffp-contract=off (global in build.py): every fp64 operation below is individually rounded.
#include "common.h"

namespace {

constexpr int kKeys = 64;            // nc <= 8: keys g * nc + p
constexpr int kNoKey = kKeys;        // a pixel that is counted nowhere
constexpr int kPixPerBlockIter = 1024;

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ void clear_i64_kernel(unsigned long long* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0ull;
}

// every lane of the wave calls this (converged); key in [0, kKeys) or kNoKey.  acc of lane k counts key k.
__device__ __forceinline__ void wave_count(int key, int lane, unsigned& acc) {
  unsigned long long todo = __ballot(key != kNoKey);
  while (todo) {                                            // wave-uniform: one turn per distinct key present
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __builtin_amdgcn_readlane(key, leader);
    const unsigned long long same = __ballot(key == k);
    acc += (lane == k) ? (unsigned)__popcll(same) : 0u;
    todo &= ~same;
  }
}

// gt id and predicted class -> key; the defects go into bad (bit 1: gt, bit 2: prediction)
__device__ __forceinline__ int make_key(long long g, bool pred_ok, int p, int nc, unsigned& bad) {
  const bool ign = g == -100;
  const bool gok = g >= 0 && g < nc;
  bad |= (!ign && !gok) ? 1u : 0u;
  bad |= pred_ok ? 0u : 2u;
  return (gok && pred_ok) ? (int)g * nc + p : kNoKey;
}

__device__ __forceinline__ int warp_class(float v, int nc, bool& ok) {
  const float f = __fmul_rn(v, (float)nc);                  // the rule of sfh_eval_batch: fp32 product, truncated
  ok = f > -1.f && f < (float)nc;                           // NaN fails both tests
  return ok ? (int)f : 0;
}

// grid (blocks per frame, B), 256 threads.  KIND: pred_kind; NC: the class count of KIND 2 (0 otherwise, nc at run time);
// VEC 4: H * W % 4 == 0 and every base pointer aligned for 4 pixels per load (checked by the launcher), else 1.
template <int KIND, int NC, int VEC>
__global__ __launch_bounds__(256) void confusion_kernel(const void* __restrict__ pred, const int64_t* __restrict__ gt,
                                                        int nc_rt, int HW, unsigned long long* __restrict__ out,
                                                        unsigned* __restrict__ flag) {
  __shared__ unsigned hist[kKeys];
  const int nc = NC ? NC : nc_rt;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y;
  const size_t frame = (size_t)b * HW;
  const int64_t* g0 = gt + frame;
  if (threadIdx.x < kKeys) hist[threadIdx.x] = 0u;
  unsigned acc = 0u, bad = 0u;
  const int step = (int)gridDim.x * 256 * VEC;
  // the loop bound is workgroup-uniform: every lane takes every turn, so the ballots of wave_count see whole waves
  for (long long base = (long long)blockIdx.x * 256 * VEC; base < HW; base += step) {
    const long long i = base + (long long)threadIdx.x * VEC;
    const bool live = i < HW;                               // VEC 4: HW % 4 == 0, so i < HW covers i + 3
    int key[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) key[e] = kNoKey;
    if (live) {
      long long g[VEC];
      if (VEC == 4) {
        const i64x2 g01 = *reinterpret_cast<const i64x2*>(g0 + i);
        const i64x2 g23 = *reinterpret_cast<const i64x2*>(g0 + i + 2);
        g[0] = g01.x;
        g[1 % VEC] = g01.y;
        g[2 % VEC] = g23.x;
        g[3 % VEC] = g23.y;
      } else {
        g[0] = g0[i];
      }
      int p[VEC];
      bool ok[VEC];
      if (KIND == 0) {
        const int* s = static_cast<const int*>(pred) + frame + i;
        int v[VEC];
        if (VEC == 4) {
          const i32x4 q = *reinterpret_cast<const i32x4*>(s);
#pragma unroll
          for (int e = 0; e < VEC; ++e) v[e] = q[e];
        } else {
          v[0] = s[0];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          ok[e] = v[e] >= 0 && v[e] < nc;
          p[e] = ok[e] ? v[e] : 0;
        }
      } else if (KIND == 1) {
        const uint8_t* s = static_cast<const uint8_t*>(pred) + frame + i;
        unsigned w = VEC == 4 ? *reinterpret_cast<const unsigned*>(s) : (unsigned)s[0];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const int v = (int)((w >> (8 * e)) & 255u);
          ok[e] = v < nc;
          p[e] = ok[e] ? v : 0;
        }
      } else if (KIND == 2) {
        constexpr int N = NC ? NC : 1;
        const float* s = static_cast<const float*>(pred) + (size_t)b * N * HW + i;
        float best[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          p[e] = 0;
          ok[e] = true;
          best[e] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          float v[VEC];
          if (VEC == 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(s + (size_t)k * HW);
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = q[e];
          } else {
            v[0] = s[(size_t)k * HW];
          }
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            // the argmax rule above sfh_outconv_fwd: strict >, scanning from class 0 (a NaN never compares greater)
            const bool up = k > 0 && v[e] > best[e];
            if (k == 0 || up) best[e] = v[e];
            p[e] = up ? k : p[e];
          }
        }
      } else {
        const float* s = static_cast<const float*>(pred) + frame + i;
        float v[VEC];
        if (VEC == 4) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(s);
#pragma unroll
          for (int e = 0; e < VEC; ++e) v[e] = q[e];
        } else {
          v[0] = s[0];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) p[e] = warp_class(v[e], nc, ok[e]);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) key[e] = make_key(g[e], ok[e], p[e], nc, bad);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) wave_count(key[e], lane, acc);
  }
  const unsigned long long b1 = __ballot((bad & 1u) != 0u), b2 = __ballot((bad & 2u) != 0u);
  if (lane == 0 && (b1 | b2)) atomicOr(flag, (b1 ? 1u : 0u) | (b2 ? 2u : 0u));   // bits: order-free
  __syncthreads();
  if (acc) atomicAdd(&hist[lane], acc);                     // at most four adders per word: the waves of the workgroup
  __syncthreads();
  if ((int)threadIdx.x < nc * nc && hist[threadIdx.x])
    atomicAdd(out + (size_t)b * nc * nc + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------- matrices
struct Mat3 {
  double v[9];
};

// adj(theta) in fp64, the nine expressions of inverse_h33 (warp_coords.h) without 1 / det; returns usable (det finite, != 0).
// Not usable: theta's fp64 copy m and the adjugate both become the zero matrix.
__device__ __forceinline__ bool adj_checked(const float* __restrict__ theta, Mat3& m, Mat3& a) {
#pragma unroll
  for (int k = 0; k < 9; ++k) m.v[k] = (double)theta[k];
  const double* t = m.v;
  a.v[0] = t[4] * t[8] - t[5] * t[7];
  a.v[1] = t[2] * t[7] - t[1] * t[8];
  a.v[2] = t[1] * t[5] - t[2] * t[4];
  a.v[3] = t[5] * t[6] - t[3] * t[8];
  a.v[4] = t[0] * t[8] - t[2] * t[6];
  a.v[5] = t[2] * t[3] - t[0] * t[5];
  a.v[6] = t[3] * t[7] - t[4] * t[6];
  a.v[7] = t[1] * t[6] - t[0] * t[7];
  a.v[8] = t[0] * t[4] - t[1] * t[3];
  const double det = (t[0] * a.v[0] + t[1] * a.v[3]) + t[2] * a.v[6];
  const bool ok = fabs(det) > 0.0 && fabs(det) <= 1.7976931348623157e308;    // finite and != 0; NaN fails the first test
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 9; ++k) m.v[k] = a.v[k] = 0.0;
  }
  return ok;
}

__device__ __forceinline__ void apply3(const double* __restrict__ M, double a, double b, double c, double& X, double& Y,
                                       double& W) {
  X = (M[0] * a + M[1] * b) + M[2] * c;
  Y = (M[3] * a + M[4] * b) + M[5] * c;
  W = (M[6] * a + M[7] * b) + M[8] * c;
}

__device__ __forceinline__ bool inside(double X, double Y, double W) {
  const double w = fabs(W);
  return w > 0.0 && fabs(X) <= w && fabs(Y) <= w;           // a NaN fails its comparison
}

// grid (blocks per frame, B), 256 threads; canvas cw x ch = (wc + 2 mx) x (hc + 2 my) pixels, fewer than 2^31
__global__ __launch_bounds__(256) void region_kernel(const float* __restrict__ theta_pred, const float* __restrict__ theta_gt,
                                                     int mode, int wc, int hc, int mx, int my,
                                                     unsigned long long* __restrict__ out) {
  __shared__ double mat[18];
  __shared__ unsigned cnt[3];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    Mat3 mp, ap, mg, ag;
    const bool okp = adj_checked(theta_pred + (size_t)b * 9, mp, ap);
    const bool okg = adj_checked(theta_gt + (size_t)b * 9, mg, ag);
    if (mode == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        mat[k] = ap.v[k];
        mat[9 + k] = ag.v[k];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double e = (mg.v[3 * i] * ap.v[j] + mg.v[3 * i + 1] * ap.v[3 + j]) + mg.v[3 * i + 2] * ap.v[6 + j];
          mat[3 * i + j] = (okp && okg) ? e : 0.0;
          mat[9 + 3 * i + j] = i == j ? 1.0 : 0.0;
        }
    }
    cnt[0] = cnt[1] = cnt[2] = 0u;
  }
  __syncthreads();
  double A[9], Bm[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    A[k] = mat[k];
    Bm[k] = mat[9 + k];
  }
  const int cw = wc + 2 * mx, ch = hc + 2 * my;
  const long long total = (long long)cw * ch;
  const double c = (double)((long long)(wc - 1) * (hc - 1));
  unsigned nA = 0u, nB = 0u, nAB = 0u;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int row = (int)((unsigned)i / (unsigned)cw);
    const int x = (int)((unsigned)i - (unsigned)row * (unsigned)cw) - mx, y = row - my;
    const double a = (double)((long long)(2 * x - (wc - 1)) * (hc - 1));
    const double bq = (double)((long long)(2 * y - (hc - 1)) * (wc - 1));
    double X, Y, W;
    apply3(A, a, bq, c, X, Y, W);
    const bool ia = inside(X, Y, W);
    apply3(Bm, a, bq, c, X, Y, W);
    const bool ib = inside(X, Y, W);
    nA += ia ? 1u : 0u;
    nB += ib ? 1u : 0u;
    nAB += (ia && ib) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nA += __shfl_down(nA, o);
    nB += __shfl_down(nB, o);
    nAB += __shfl_down(nAB, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&cnt[0], nA);
    atomicAdd(&cnt[1], nB);
    atomicAdd(&cnt[2], nAB);
  }
  __syncthreads();
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(out + (size_t)b * 3 + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------------ points
// the error of one point under the two matrices (g: ground truth, p: prediction); counted iff in(g, q)
__device__ __forceinline__ bool point_error(const double* __restrict__ Mg, const double* __restrict__ Mp, double x, double y,
                                            double sx, double sy, double& err) {
  double Xg, Yg, Wg, Xp, Yp, Wp;
  apply3(Mg, x, y, 1.0, Xg, Yg, Wg);
  apply3(Mp, x, y, 1.0, Xp, Yp, Wp);
  const double dx = (Xp / Wp - Xg / Wg) * sx;
  const double dy = (Yp / Wp - Yg / Wg) * sy;
  err = __dsqrt_rn(dx * dx + dy * dy);
  return inside(Xg, Yg, Wg);
}

// grid B, one wave per frame
__global__ __launch_bounds__(64) void points_kernel(const float* __restrict__ theta_pred, const float* __restrict__ theta_gt,
                                                    const double* __restrict__ court_pts, int npts, int gx, int gy,
                                                    double frame_sx, double frame_sy, double court_sx, double court_sy,
                                                    double* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  Mat3 mp, ap, mg, ag;                                      // every lane forms them: 9 + 9 floats, no exchange needed
  adj_checked(theta_pred + (size_t)b * 9, mp, ap);
  adj_checked(theta_gt + (size_t)b * 9, mg, ag);
  double rs = 0.0, rn = 0.0, ps = 0.0, pn = 0.0;
  for (int n = lane; n < npts; n += 64) {
    double e;
    if (point_error(ag.v, ap.v, court_pts[2 * (size_t)n], court_pts[2 * (size_t)n + 1], frame_sx, frame_sy, e)) {
      rs += e;
      rn += 1.0;
    }
  }
  const int nl = gx * gy;
  for (int n = lane; n < nl; n += 64) {
    const int l = n / gx, k = n - l * gx;                   // row-major lattice: n = l gx + k
    const double x = -1.0 + (double)(2 * k + 1) / (double)gx;
    const double y = -1.0 + (double)(2 * l + 1) / (double)gy;
    double e;
    if (point_error(mg.v, mp.v, x, y, court_sx, court_sy, e)) {
      ps += e;
      pn += 1.0;
    }
  }
  rs = wave_sum(rs);
  rn = wave_sum(rn);
  ps = wave_sum(ps);
  pn = wave_sum(pn);
  if (lane == 0) {
    double* o = out + (size_t)b * 4;
    o[0] = rs / rn;                                         // 0 / 0 = NaN: no counted point
    o[1] = rn;
    o[2] = ps / pn;
    o[3] = pn;
  }
}

int clear_i64(int64_t* out, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(clear_i64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (unsigned long long*)out, (int)n);
  return sfh_check_launch("metrics clear_i64_kernel");
}

}  // namespace

extern "C" int sfh_metrics_confusion(const void* pred, int pred_kind, const int64_t* gt, int nc, int batch, int H, int W,
                                     int64_t* out, uint32_t* flag, void* stream) {
  SFH_REQUIRE(pred && gt && out && flag, "metrics_confusion: null pred / gt / out / flag");
  SFH_REQUIRE(pred_kind >= 0 && pred_kind <= 3, "metrics_confusion: pred_kind=%d (0 int32, 1 uint8, 2 logits, 3 warp mask)", pred_kind);
  SFH_REQUIRE(nc >= 2 && nc <= 8, "metrics_confusion: nc=%d (2 .. 8 classes)", nc);
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 0 && W > 0, "metrics_confusion: bad geometry b=%d h=%d w=%d", batch, H, W);
  SFH_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "metrics_confusion: frame of %d x %d has 2^31 pixels or more", W, H);
  const int HW = H * W;
  hipStream_t st = (hipStream_t)stream;
  int rc = clear_i64(out, (int64_t)batch * nc * nc, st);
  if (rc) return rc;
  // 4 pixels per load: 32 bytes of gt in two 16-byte loads, 16 bytes of int32 / fp32, 4 bytes of uint8
  const uintptr_t pa = (uintptr_t)pred, ga = (uintptr_t)gt;
  const bool vec = HW % 4 == 0 && (ga & 15) == 0 && (pa & (pred_kind == 1 ? 3 : 15)) == 0;
  const int per = kPixPerBlockIter * 4;                     // about four turns of the loop per workgroup
  const dim3 grid((unsigned)((HW + per - 1) / per), (unsigned)batch);
  unsigned long long* o = (unsigned long long*)out;
#define SFH_CONF(KIND, NC)                                                                                                \
  do {                                                                                                                    \
    if (vec)                                                                                                              \
      hipLaunchKernelGGL((confusion_kernel<KIND, NC, 4>), grid, dim3(256), 0, st, pred, gt, nc, HW, o, (unsigned*)flag);  \
    else                                                                                                                  \
      hipLaunchKernelGGL((confusion_kernel<KIND, NC, 1>), grid, dim3(256), 0, st, pred, gt, nc, HW, o, (unsigned*)flag);  \
  } while (0)
  switch (pred_kind) {
    case 0: SFH_CONF(0, 0); break;
    case 1: SFH_CONF(1, 0); break;
    case 3: SFH_CONF(3, 0); break;
    default:
      switch (nc) {
        case 2: SFH_CONF(2, 2); break;
        case 3: SFH_CONF(2, 3); break;
        case 4: SFH_CONF(2, 4); break;
        case 5: SFH_CONF(2, 5); break;
        case 6: SFH_CONF(2, 6); break;
        case 7: SFH_CONF(2, 7); break;
        default: SFH_CONF(2, 8); break;
      }
  }
#undef SFH_CONF
  return sfh_check_launch("metrics confusion_kernel");
}

extern "C" int sfh_metrics_region(const float* theta_pred, const float* theta_gt, int batch, int mode, int wc, int hc, int mx,
                                  int my, int64_t* out, void* stream) {
  SFH_REQUIRE(theta_pred && theta_gt && out, "metrics_region: null theta / out");
  SFH_REQUIRE(batch > 0 && batch <= 65535, "metrics_region: batch=%d (1 .. 65535)", batch);
  SFH_REQUIRE(mode == 0 || mode == 1, "metrics_region: mode=%d (0 part, 1 whole)", mode);
  const int lim = 1 << 20;                                  // (2 (wc-1+mx) - (wc-1)) (hc-1) < 2^43: exact in fp64
  SFH_REQUIRE(wc >= 2 && hc >= 2 && wc <= lim && hc <= lim, "metrics_region: raster %d x %d (2 .. 2^20 per axis)", wc, hc);
  SFH_REQUIRE(mx >= 0 && my >= 0 && mx <= lim && my <= lim, "metrics_region: margin %d, %d (0 .. 2^20)", mx, my);
  const int64_t total = ((int64_t)wc + 2 * mx) * ((int64_t)hc + 2 * my);
  SFH_REQUIRE(total < ((int64_t)1 << 31), "metrics_region: canvas of %lld pixels (fewer than 2^31)", (long long)total);
  hipStream_t st = (hipStream_t)stream;
  int rc = clear_i64(out, (int64_t)batch * 3, st);
  if (rc) return rc;
  const int64_t blocks = (total + 2047) / 2048;             // about eight pixels per thread
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)batch);
  hipLaunchKernelGGL(region_kernel, grid, dim3(256), 0, st, theta_pred, theta_gt, mode, wc, hc, mx, my, (unsigned long long*)out);
  return sfh_check_launch("metrics region_kernel");
}

extern "C" int sfh_metrics_points(const float* theta_pred, const float* theta_gt, int batch, const double* court_pts, int npts,
                                  int gx, int gy, double frame_sx, double frame_sy, double court_sx, double court_sy,
                                  double* out, void* stream) {
  SFH_REQUIRE(theta_pred && theta_gt && out, "metrics_points: null theta / out");
  SFH_REQUIRE(batch > 0 && batch <= 65535, "metrics_points: batch=%d (1 .. 65535)", batch);
  SFH_REQUIRE(npts >= 0 && npts <= (1 << 24) && (npts == 0 || court_pts), "metrics_points: npts=%d with%s court points", npts,
              court_pts ? "" : "out");
  SFH_REQUIRE(gx >= 1 && gy >= 1 && gx <= 4096 && gy <= 4096, "metrics_points: lattice %d x %d (1 .. 4096 per axis)", gx, gy);
  hipLaunchKernelGGL(points_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, theta_pred, theta_gt, court_pts,
                     npts, gx, gy, frame_sx, frame_sy, court_sx, court_sy, out);
  return sfh_check_launch("metrics points_kernel");
}
