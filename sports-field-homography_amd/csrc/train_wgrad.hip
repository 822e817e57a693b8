// train_wgrad.hip - the weight-gradient convolution of the training step on the fp32 matrix cores.
//
// Replaces, for loss.backward() (train.py:233), cuDNN's backward-filter.  All activations fp32 NHWC.
// (An accumulating entry, its _det sibling and its _det_bytes query: the rule stands above bn_stats_impl, train_bn.hip.)

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "common.h"
#include "bn_math.h"    // wgrad_c4_kernel<TH, TW, true>
#include "det_core.h"   // det_wgrad_plan, the slab offsets of the deterministic mode

namespace {
// ------------------------------------------------------------------ weight gradient (fp32 MFMA)
// raw[m][tap][n] += sum over pixels p of dz[p][m] * xin[p + tap][n]
//   GEMM view: M = output channels, N = input channels of one source, K = B*H*W pixels.
// Workgroup = 64 m x 16*NSUB n x all taps, over a strided subset of 2x32-pixel tiles (blockIdx.z =
// split); each wave owns 16 m.  v_mfma_f32_16x16x4_f32: A[i=m][k=pixel], B[k=pixel][j=n] - in NHWC the
// 16 channels of a pixel are contiguous, so both fragments are plain ds_read_b32 with k = lane/16.
// LDS rows are 64 floats per pixel; bit 4 of the channel index is XORed with the pixel parity so the
// two pixels a 32-lane group reads land in different bank halves.
struct WgradArgs {
  const float* dz; int dz_cs; int M;
  const float* x; int x_cs, xh, xw, N, pad_top, pad_left;
  int batch, H, W;
  float* raw; int raw_n, n_off;
  int ntx, nty, ntiles, nsplit, mt, mn;
  // wgrad_c4_kernel only (sfh_conv_wgrad_c4_bn): dz points at dy, the gradient of the BatchNorm + ReLU OUTPUT, and the
  // BatchNorm backward is applied while a tile is loaded (bn_z != nullptr): z, mean | invstd, gamma, beta, the finished
  // backward sums [sum g | sum g * xhat] and 1 / (pixels per channel)
  const float* bn_z; const float* bn_mi; const float* bn_gamma; const float* bn_beta; const double* bn_acc; float bn_inv_n;
};

// DET: a.raw is the workspace: split s stores its sums into slab s, element det_wgrad_elem(m, tap, n) (det_core.h)
template <int KS, int NSUB, int TH, int TW, bool DET = false>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(const WgradArgs a) {
  static_assert(TH * TW == 64 && TW % 4 == 0, "64-pixel tiles");
  constexpr int PADB = KS == 3 ? 1 : (KS == 4 ? 2 : 0);
  constexpr int HR = TH + KS - 1, HW = TW + KS - 1, HPX = HR * HW;
  constexpr int KK = KS * KS;
  constexpr int NHV = (HPX * 4 * NSUB + 255) / 256;  // halo float4 loads per thread
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xL = lds;               // [HPX][64]
  float* zL = lds + HPX * 64;    // [64][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, kq = lane >> 4;
  // XCD-aware order (workgroups go round-robin to the 8 XCDs): the mn = (m tiles) x (n tiles) workgroups
  // of one pixel split run back to back on ONE XCD, so the split's dz / x tiles are fetched into that
  // L2 once instead of once per (m, n) block
  const int xcd = blockIdx.x & 7, kk_ = blockIdx.x >> 3;
  const int split = (kk_ / a.mn) * 8 + xcd, mni = kk_ % a.mn;
  if (split >= a.nsplit) return;
  const int m0 = (mni % a.mt) * 64, n0 = (mni / a.mt) * (16 * NSUB);
  f32x4 acc[KK][NSUB];
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int s = 0; s < NSUB; ++s) acc[t][s] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // global loads of one tile into registers (zero outside the frame / the channel range)
  f32x4 hv[NHV], zv[4];
  auto load_tile = [&](int tile) {
    const int tx = tile % a.ntx;
    const int ty = (tile / a.ntx) % a.nty;
    const int b = tile / (a.ntx * a.nty);
    const int y0 = ty * TH, x0 = tx * TW;
#pragma unroll
    for (int k = 0; k < NHV; ++k) {
      const int i = tid + k * 256;
      const int q = i % (4 * NSUB), hp = i / (4 * NSUB);
      const int hr = hp / HW, hc = hp - hr * HW;
      const int sy = y0 + hr - PADB - a.pad_top, sx = x0 + hc - PADB - a.pad_left;
      const int n = n0 + 4 * q;
      hv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (hp < HPX && sy >= 0 && sy < a.xh && sx >= 0 && sx < a.xw && n < a.N)
        hv[k] = *reinterpret_cast<const f32x4*>(a.x + (((long)b * a.xh + sy) * a.xw + sx) * a.x_cs + n);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = tid + k * 256;
      const int q = i & 15, p = i >> 4;
      const int r = p / TW, c = p - r * TW;
      const int y = y0 + r, x = x0 + c, m = m0 + 4 * q;
      zv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (y < a.H && x < a.W && m < a.M)
        zv[k] = *reinterpret_cast<const f32x4*>(a.dz + (((long)b * a.H + y) * a.W + x) * a.dz_cs + m);
    }
  };
  // Software pipeline over the workgroup's tiles (round 4): the loads of tile t + 1 are requested right behind the
  // barrier that publishes tile t in LDS and stay in flight during its contraction; before, every tile paid its own
  // load latency between two barriers (the 3-channel first layer: 1.03 ms for 0.94 GB = 0.9 TB/s).
  // Only for the small instances (the 3-channel first layer: 36 accumulator registers): with 128+ accumulator registers
  // the prefetched tile costs occupancy and the 7x7 stem's instance measured 0.63 -> 0.71 ms.
  constexpr bool PIPE = KK * NSUB <= 9;
  if (PIPE && split < a.ntiles) load_tile(split);
  for (int tile = split; tile < a.ntiles; tile += a.nsplit) {
    if (!PIPE) load_tile(tile);   // every global load of the tile issued first (one latency, not one per iteration)
    __syncthreads();  // previous tile's fragments consumed
#pragma unroll
    for (int k = 0; k < NHV; ++k) {
      const int i = tid + k * 256;
      const int q = i % (4 * NSUB), hp = i / (4 * NSUB);
      if (hp < HPX) *reinterpret_cast<f32x4*>(xL + hp * 64 + 4 * (q ^ ((hp & 1) << 2))) = hv[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = tid + k * 256;
      const int q = i & 15, p = i >> 4;
      *reinterpret_cast<f32x4*>(zL + p * 64 + 4 * (q ^ ((p & 1) << 2))) = zv[k];
    }
    __syncthreads();
    if (PIPE && tile + a.nsplit < a.ntiles) load_tile(tile + a.nsplit);
    // ---- contraction over the 64 pixels of the tile, 4 per MFMA
#pragma unroll 1
    for (int r = 0; r < TH; ++r) {
#pragma unroll 2
      for (int c4 = 0; c4 < TW / 4; ++c4) {
        const int pz = r * TW + c4 * 4 + kq;
        const float av = zL[pz * 64 + ((wave * 16 + l16) ^ ((pz & 1) << 4))];
#pragma unroll
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
          for (int kx = 0; kx < KS; ++kx) {
            const int ph = (r + ky) * HW + c4 * 4 + kq + kx;
            const float* row = xL + ph * 64;
            const int sw = (ph & 1) << 4;
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
              const float bv = row[(s * 16 + l16) ^ sw];
              acc[ky * KS + kx][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[ky * KS + kx][s], 0, 0, 0);
            }
          }
      }
    }
  }
  // ---- D[i = 4*(lane/16) + r][j = lane%16]
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
      const int n = n0 + s * 16 + l16;
      if (n >= a.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wave * 16 + 4 * kq + r;
        if (m < a.M) {
          if constexpr (DET) a.raw[det_slab_offset(split, (long)a.M * KK * a.N) + det_wgrad_elem(m, t, n, KK, a.N)] = acc[t][s][r];
          else unsafeAtomicAdd(a.raw + ((long)m * KK + t) * a.raw_n + a.n_off + n, acc[t][s][r]);
        }
      }
    }
}

// the plan's grid numbers into the kernel's arguments; returns the grid: whole rounds of 8 splits (one per XCD)
static dim3 wgrad_grid(WgradArgs& a, const DetWgradPlan& p) {
  a.ntx = p.ntx;
  a.nty = p.nty;
  a.ntiles = p.ntiles;
  a.nsplit = p.nsplit;
  a.mt = p.mt;   // (the first-layer form: mn == mt)
  a.mn = p.mn;
  return dim3((unsigned)(sfh_cdiv(p.nsplit, 8) * 8 * p.mn));
}

// A backward-filter launch.  ws == nullptr: the default mode, atomics onto raw.  Else the deterministic sibling: the store pass
// into `ws` (slab per split, compact rows of N columns), then the sum pass onto columns [n_off, n_off + N) of raw.
template <int KS, int NSUB, int TH, int TW>
int launch_wgrad(WgradArgs a, const DetWgradPlan& p, float* ws, hipStream_t stream) {
  constexpr int HPX = (TH + KS - 1) * (TW + KS - 1);
  const size_t lds = (size_t)(HPX + 64) * 64 * sizeof(float);
  const dim3 grid = wgrad_grid(a, p);
  float* raw = a.raw;
  if (ws) a.raw = ws;
  if (!ws) hipLaunchKernelGGL((wgrad_kernel<KS, NSUB, TH, TW>), grid, dim3(256), lds, stream, a);
  else hipLaunchKernelGGL((wgrad_kernel<KS, NSUB, TH, TW, true>), grid, dim3(256), lds, stream, a);
  if (int rc = sfh_check_launch(ws ? "wgrad_kernel (deterministic)" : "wgrad_kernel")) return rc;
  return ws ? sfh_det_reduce_f32(ws, p.slabs, p.elems, p.elems, a.N, raw + a.n_off, a.raw_n, stream) : SFH_OK;
}

// Backward-filter of a 3x3 conv over at most FOUR input channels (the UNet's first layer: N = 3 stored as 4; round 4).
// The generic kernel above spends one MFMA per tap on a 16-wide n block of which 4 columns are channels (75 % padding:
// 0.75 ms, bound by the fp32 matrix pipe).  Here the n axis is (tap, channel): n = 4 * tap + c, 36 real columns in three
// blocks of 16 - three MFMAs per four pixels instead of nine - and the halo is 16 bytes per pixel (2 KB instead of 35 KB of
// LDS: four workgroups per CU).  B fragment: lane (j = n in the block, k = pixel) reads x[pixel + tap(n)][c(n)], one
// ds_read_b32 at a per-lane constant offset; columns 36 .. 47 read a slot that stays zero.
// BN: the layer's BatchNorm backward rides in the tile load (bn_math.h: bn_bwd_apply_kernel's values): the
// kernel reads dy and z (8 B per element) instead of a dz tensor that a separate pass would first write and this one read
// back (12 + 4 B per element moved by the pair).
template <int TH, int TW, bool BN, bool DET = false>
__global__ __launch_bounds__(256, 4) void wgrad_c4_kernel(const WgradArgs a) {
  static_assert(TH * TW == 64 && TW % 4 == 0, "64-pixel tiles");
  constexpr int HR = TH + 2, HW = TW + 2, HPX = HR * HW;
  __shared__ __attribute__((aligned(16))) float zL[64 * 64];     // dz tile [64 pixels][64 m]
  __shared__ __attribute__((aligned(16))) f32x4 xL[HPX + 1];     // halo, 4 channels per pixel; slot HPX stays zero
  const float* xf = reinterpret_cast<const float*>(xL);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, kq = lane >> 4;
  const int xcd = blockIdx.x & 7, kk_ = blockIdx.x >> 3;
  const int split = (kk_ / a.mn) * 8 + xcd, mni = kk_ % a.mn;
  if (split >= a.nsplit) return;
  const int m0 = mni * 64;
  int offn[3];
#pragma unroll
  for (int nb = 0; nb < 3; ++nb) {
    const int n = nb * 16 + l16, tap = n >> 2, c = n & 3;
    offn[nb] = n < 36 ? ((tap / 3) * HW + tap % 3) * 4 + c : -1;
  }
  f32x4 acc[3];
#pragma unroll
  for (int nb = 0; nb < 3; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (tid == 0) xL[HPX] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 hv, zv[4];
  // (BN) the four channels m0 + 4 * (tid & 15) .. + 3 of every value this thread loads: 256 % 16 == 0
  BnChannels<4> bn;
  if constexpr (BN)
    bn = bn_load<4, true>(a.bn_mi, a.bn_gamma, a.bn_beta, a.M, m0 + 4 * (tid & 15), true, a.bn_acc, a.bn_inv_n, a.M - 1);
  auto load_tile = [&](int tile) {
    const int tx = tile % a.ntx;
    const int ty = (tile / a.ntx) % a.nty;
    const int b = tile / (a.ntx * a.nty);
    const int y0 = ty * TH, x0 = tx * TW;
    hv = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (tid < HPX) {
      const int hr = tid / HW, hc = tid - hr * HW;
      const int sy = y0 + hr - 1, sx = x0 + hc - 1;
      if (sy >= 0 && sy < a.H && sx >= 0 && sx < a.W)
        hv = *reinterpret_cast<const f32x4*>(a.x + (((long)b * a.H + sy) * a.W + sx) * 4);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = tid + k * 256;
      const int q = i & 15, p = i >> 4;
      const int r = p / TW, c = p - r * TW;
      const int y = y0 + r, x = x0 + c, m = m0 + 4 * q;
      zv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (y < a.H && x < a.W && m < a.M) {
        const long o = (((long)b * a.H + y) * a.W + x) * a.dz_cs + m;
        zv[k] = *reinterpret_cast<const f32x4*>(a.dz + o);
        if constexpr (BN) {
          const f32x4 zz = *reinterpret_cast<const f32x4*>(a.bn_z + o);
#pragma unroll
          for (int j = 0; j < 4; ++j) zv[k][j] = bn.dz(j, zz[j], bn_gate(bn.y(j, zz[j]), zv[k][j]));
        }
      }
    }
  };
  if (split < a.ntiles) load_tile(split);
  for (int tile = split; tile < a.ntiles; tile += a.nsplit) {
    __syncthreads();  // previous tile's fragments consumed
    if (tid < HPX) xL[tid] = hv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = tid + k * 256;
      const int q = i & 15, p = i >> 4;
      *reinterpret_cast<f32x4*>(zL + p * 64 + 4 * (q ^ ((p & 1) << 2))) = zv[k];
    }
    __syncthreads();
    if (tile + a.nsplit < a.ntiles) load_tile(tile + a.nsplit);   // in flight during the contraction
#pragma unroll 2
    for (int r = 0; r < TH; ++r) {
#pragma unroll
      for (int c4 = 0; c4 < TW / 4; ++c4) {
        const int pz = r * TW + c4 * 4 + kq;
        const float av = zL[pz * 64 + ((wave * 16 + l16) ^ ((pz & 1) << 4))];
        const int ph4 = (r * HW + c4 * 4 + kq) * 4;     // float index of the window's top-left pixel
#pragma unroll
        for (int nb = 0; nb < 3; ++nb) {
          const float bv = xf[offn[nb] >= 0 ? ph4 + offn[nb] : HPX * 4];
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[nb], 0, 0, 0);
        }
      }
    }
  }
  // D[i = 4 * (lane / 16) + r][j = lane % 16]: m = m0 + 16 * wave + i, n = 16 * nb + j = 4 * tap + c
#pragma unroll
  for (int nb = 0; nb < 3; ++nb) {
    const int n = nb * 16 + l16, tap = n >> 2, c = n & 3;
    if (n >= 36 || c >= a.N) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * 16 + 4 * kq + r;
      if (m < a.M) {
        if constexpr (DET) a.raw[det_slab_offset(split, (long)a.M * 9 * a.N) + det_wgrad_elem(m, tap, c, 9, a.N)] = acc[nb][r];
        else unsafeAtomicAdd(a.raw + ((long)m * 9 + tap) * a.raw_n + a.n_off + c, acc[nb][r]);
      }
    }
  }
}

template <int TH, int TW>
int launch_wgrad_c4(WgradArgs a, const DetWgradPlan& p, float* ws, hipStream_t stream) {
  const dim3 grid = wgrad_grid(a, p);
  float* raw = a.raw;
  if (ws) a.raw = ws;
  if (!ws) hipLaunchKernelGGL((wgrad_c4_kernel<TH, TW, false>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((wgrad_c4_kernel<TH, TW, false, true>), grid, dim3(256), 0, stream, a);
  if (int rc = sfh_check_launch(ws ? "wgrad_c4_kernel (deterministic)" : "wgrad_c4_kernel")) return rc;
  return ws ? sfh_det_reduce_f32(ws, p.slabs, p.elems, p.elems, a.N, raw + a.n_off, a.raw_n, stream) : SFH_OK;
}

// the fused BatchNorm form (sfh_conv_wgrad_c4_bn) has no deterministic sibling: the mode takes sfh_bn_bwd_apply + sfh_conv_wgrad
template <int TH, int TW>
int launch_wgrad_c4_bn(WgradArgs a, const DetWgradPlan& p, hipStream_t stream) {
  const dim3 grid = wgrad_grid(a, p);
  hipLaunchKernelGGL((wgrad_c4_kernel<TH, TW, true>), grid, dim3(256), 0, stream, a);
  return sfh_check_launch("wgrad_c4_kernel");
}
}  // namespace

static int conv_wgrad_impl(const float* dz, int dz_cs, int M, const float* x, int x_cs, int xh, int xw, int N, int pad_top,
                           int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n, int n_off, bool det,
                           void* workspace, long long workspace_bytes, void* stream) {
  const char* who = det ? "conv_wgrad_det" : "conv_wgrad";
  // the network's first layer (3 input channels stored as 4, one source of the frame's own size): p.c4, n = (tap, channel)
  const DetWgradPlan p = det_wgrad_plan(M, x_cs, xh, xw, N, pad_top, pad_left, batch, H, W, ksize);
  SFH_REQUIRE(dz && x && raw, "%s: null pointer", who);
  SFH_REQUIRE(p.why != DET_BAD_FRAME, "%s: bad geometry", who);
  SFH_REQUIRE(p.why != DET_BAD_M && dz_cs % 4 == 0 && dz_cs >= M, "%s: M=%d dz_cs=%d", who, M, dz_cs);
  SFH_REQUIRE(p.why != DET_BAD_N, "%s: N=%d x_cs=%d", who, N, x_cs);
  SFH_REQUIRE(n_off >= 0 && n_off + N <= raw_n, "%s: n_off=%d N=%d raw_n=%d", who, n_off, N, raw_n);
  SFH_REQUIRE(p.why != DET_BAD_FIT, "%s: source (%dx%d at %d,%d) does not fit the %dx%d frame", who, xh, xw, pad_top, pad_left, H, W);
  SFH_REQUIRE(p.why != DET_BAD_KSIZE, "%s: ksize %d", who, ksize);
  SFH_REQUIRE(p.ok, "%s: the 4x4 (stem) case supports N <= 32", who);
  WgradArgs a;
  a.dz = dz; a.dz_cs = dz_cs; a.M = M;
  a.x = x; a.x_cs = x_cs; a.xh = xh; a.xw = xw; a.N = N; a.pad_top = pad_top; a.pad_left = pad_left;
  a.batch = batch; a.H = H; a.W = W;
  a.raw = raw; a.raw_n = raw_n; a.n_off = n_off;
  a.ntx = a.nty = a.ntiles = a.nsplit = a.mt = a.mn = 0;
  a.bn_z = a.bn_mi = a.bn_gamma = a.bn_beta = nullptr; a.bn_acc = nullptr; a.bn_inv_n = 0.f;
  hipStream_t st = (hipStream_t)stream;
  if (det) SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  float* ws = det ? (float*)workspace : nullptr;   // the launchers: nullptr is the default mode
  const int t = p.shape;
#define SFH_WG(KS_, NS_)                                         \
  (t == 0 ? launch_wgrad<KS_, NS_, 2, 32>(a, p, ws, st)           \
          : (t == 1 ? launch_wgrad<KS_, NS_, 4, 16>(a, p, ws, st) : launch_wgrad<KS_, NS_, 8, 8>(a, p, ws, st)))
  if (p.c4)
    return t == 0 ? launch_wgrad_c4<2, 32>(a, p, ws, st)
                  : (t == 1 ? launch_wgrad_c4<4, 16>(a, p, ws, st) : launch_wgrad_c4<8, 8>(a, p, ws, st));
  if (ksize == 3 && N <= 16) return SFH_WG(3, 1);
  if (ksize == 3) return SFH_WG(3, 4);
  if (ksize == 1) return SFH_WG(1, 4);
  return SFH_WG(4, 2);
#undef SFH_WG
}

extern "C" int sfh_conv_wgrad(const float* dz, int dz_cs, int M, const float* x, int x_cs, int xh, int xw, int N,
                              int pad_top, int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n,
                              int n_off, void* stream) {
  return conv_wgrad_impl(dz, dz_cs, M, x, x_cs, xh, xw, N, pad_top, pad_left, batch, H, W, ksize, raw, raw_n, n_off, false,
                         nullptr, 0, stream);
}

extern "C" int64_t sfh_conv_wgrad_det_bytes(int M, int x_cs, int xh, int xw, int N, int pad_top, int pad_left, int batch, int H,
                                            int W, int ksize) {
  return det_bytes(det_wgrad_plan(M, x_cs, xh, xw, N, pad_top, pad_left, batch, H, W, ksize));
}

extern "C" int sfh_conv_wgrad_det(const float* dz, int dz_cs, int M, const float* x, int x_cs, int xh, int xw, int N,
                                  int pad_top, int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n,
                                  int n_off, void* workspace, long long workspace_bytes, void* stream) {
  return conv_wgrad_impl(dz, dz_cs, M, x, x_cs, xh, xw, N, pad_top, pad_left, batch, H, W, ksize, raw, raw_n, n_off, true,
                         workspace, workspace_bytes, stream);
}

extern "C" int sfh_conv_wgrad_c4_bn(const float* dy, const float* z, const float* mean_invstd, const float* gamma,
                                    const float* beta, const double* acc, int M, const float* x, int N, int batch, int H,
                                    int W, float* raw, int raw_n, void* stream) {
  SFH_REQUIRE(dy && z && mean_invstd && gamma && beta && acc && x && raw, "conv_wgrad_c4_bn: null pointer");
  SFH_REQUIRE(batch > 0 && H > 0 && W > 0 && M > 0 && M % 4 == 0 && N > 0 && N <= 4 && raw_n >= N,
              "conv_wgrad_c4_bn: M=%d N=%d raw_n=%d", M, N, raw_n);
  WgradArgs a;
  a.dz = dy; a.dz_cs = M; a.M = M;
  a.x = x; a.x_cs = 4; a.xh = H; a.xw = W; a.N = N; a.pad_top = 0; a.pad_left = 0;
  a.batch = batch; a.H = H; a.W = W;
  a.raw = raw; a.raw_n = raw_n; a.n_off = 0;
  a.ntx = a.nty = a.ntiles = a.nsplit = a.mt = a.mn = 0;
  a.bn_z = z; a.bn_mi = mean_invstd; a.bn_gamma = gamma; a.bn_beta = beta; a.bn_acc = acc;
  a.bn_inv_n = bn_inv_n((long)batch * H * W);
  hipStream_t st = (hipStream_t)stream;
  const DetWgradPlan p = det_wgrad_plan(M, 4, H, W, 4, 0, 0, batch, H, W, 3);   // the first-layer form: channels as stored, four
  return p.shape == 0 ? launch_wgrad_c4_bn<2, 32>(a, p, st)
                      : (p.shape == 1 ? launch_wgrad_c4_bn<4, 16>(a, p, st) : launch_wgrad_c4_bn<8, 8>(a, p, st));
}
