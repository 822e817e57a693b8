// conv_grouped.hip - the grouped 3x3 convolution of the ResNeXt Bottleneck (models/resnet.py:108-112, groups = 32):
// forward / backward-data (one kernel) and backward-filter, plain fp32 multiply-add with the halo and the weights in LDS.
//
// Why no matrix cores: one output contracts K = 9 * cg = 36 .. 576 terms over a tile only cg = 4 .. 64 channels wide; the
// 64-cout MFMA tiles of conv_mfma.hip / conv_s3.hip would multiply 8 - 16x zeros at cg = 4 / 8, and the fp32 VALU rate of this
// chip equals its fp32 MFMA rate.  fp32 in, fp32 out, one rounding per product and per add: no split operands.
//
// Index arithmetic, packed-weight layout and the order of one output's terms: conv_grouped_core.h.
//
// conv_grouped_kernel<CG, S>: 256 threads; one workgroup = one tile of TH x 16 output pixels (TH = 8 at stride 1, 4 at stride
//   2) x CB = gc_cb(CG) output channels (whole groups: 8 / 4 / 2 / 1 / 1 of them).  LDS: the halo, (TH-1)*S+3 rows x
//   15*S+3 columns x 32 input channels at a pixel stride of 33 floats, and the chunk's weights [tap][c][CB]:
//       stride 1:  23,760 B halo + 9 * gc_chunk * CB * 4 B weights  =  28,368 (cg 4) .. 60,624 (cg 32), 97,488 (cg 64)
//       stride 2:  39,204 B halo + the same weights                  =  43,824 (cg 4) .. 76,080 (cg 32), 112,932 (cg 64)
//   (the compiler's figures; 86 VGPRs at stride 1, 48 at stride 2, 178 / 100 at cg 64, no scratch)
//   A thread owns 4 consecutive output channels x PPT pixels of one tile column (PPT = 2 .. 8): per (tap, c) one 16-byte LDS
//   read of weights, PPT 4-byte reads of the halo, 4 * PPT multiply-adds.  Channel blocks that reach past the last channel
//   (G * cg = 12: one block of 32) load zeros and store nothing there.
// conv_grouped_wgrad_kernel<CG, S>: same tile; LDS: the halo at a pixel stride of 36 floats and the tile's dz [pixel][33];
//   51,216 B at stride 2, 42,816 B at stride 1 (re-used for the lanes' partial sums); 116 - 120 VGPRs, no scratch.  A thread
//   owns (output channel, 4 input channels, all 9 taps) = 36 accumulators.  Accumulation plan: conv_grouped_core.h (fp32
//   throughout, one fp32 atomic add per raw element and workgroup, no fp64).
#include "common.h"
#include "conv_grouped_core.h"
#include "det_core.h"   // det_add and det_grouped_plan: the admitted geometries and the deterministic mode's slabs

namespace {

template <int CG, int S>
__global__ __launch_bounds__(256) void conv_grouped_kernel(const float* __restrict__ src, const float* __restrict__ wpacked,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           int relu, float* __restrict__ dst, int H, int W, int Ho, int Wo,
                                                           int C, int tiles_x, int tiles_y) {
  constexpr int CB = CG < 32 ? 32 : CG, KC = CG < 32 ? CG : 32, NCH = CG / KC;
  constexpr int TH = S == 1 ? 8 : 4, TW = GC_TW, HH = (TH - 1) * S + 3, HW = (TW - 1) * S + 3, PS = 33;
  constexpr int NQ = CB / 4, NSLOT = 256 / NQ, RSTEP = NSLOT / TW, PPT = TH / RSTEP;
  __shared__ float halo[HH * HW * PS];
  __shared__ __attribute__((aligned(16))) float wl[9 * KC * CB];

  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int tx0 = (t % tiles_x) * TW;
  t /= tiles_x;
  const int ty0 = (t % tiles_y) * TH;
  const int b = t / tiles_y;
  const int cb = blockIdx.y;

  const int q = tid % NQ, slot = tid / NQ;
  const int ocl = 4 * q, col = slot % TW, r0 = slot / TW;
  // the thread's input channels inside the 32 halo channels: its group's (cg < 32), or the chunk's (one group per block)
  const int hbase = CG < 32 ? (ocl / CG) * CG : 0;

  float acc[PPT][4];
#pragma unroll
  for (int i = 0; i < PPT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  for (int chunk = 0; chunk < NCH; ++chunk) {
    if (chunk) __syncthreads();
    const int in_base = cb * CB + chunk * 32;
    for (int idx = tid; idx < HH * HW * 32; idx += 256) {
      const int px = idx >> 5, ch = idx & 31;
      const int sy = gc_src_coord(ty0, px / HW, S, H), sx = gc_src_coord(tx0, px % HW, S, W);
      float v = 0.f;
      if (sy >= 0 && sx >= 0 && in_base + ch < C) v = src[((size_t)(b * H + sy) * W + sx) * C + in_base + ch];
      halo[px * PS + ch] = v;
    }
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(wpacked + (size_t)(cb * NCH + chunk) * (9 * KC * CB));
    for (int idx = tid; idx < 9 * KC * CB / 4; idx += 256) reinterpret_cast<f32x4*>(wl)[idx] = wsrc[idx];
    __syncthreads();
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      const float* hp = halo + ((r0 * S + ky) * HW + col * S + kx) * PS + hbase;
      const float* wp = wl + tap * KC * CB + ocl;
#pragma unroll 4
      for (int c = 0; c < KC; ++c) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wp + c * CB);
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
          const float x = hp[i * RSTEP * S * HW * PS + c];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += x * w4[j];
        }
      }
    }
  }

  const int oc = cb * CB + ocl, ox = tx0 + col;
  if (oc >= C || ox >= Wo) return;
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (scale) {
    sc = *reinterpret_cast<const f32x4*>(scale + oc);
    sh = *reinterpret_cast<const f32x4*>(shift + oc);
  }
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int oy = ty0 + r0 + i * RSTEP;
    if (oy >= Ho) continue;
    f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = acc[i][j];
      if (scale) v = v * sc[j] + sh[j];
      y[j] = relu ? sfh_relu(v) : v;
    }
    *reinterpret_cast<f32x4*>(dst + ((size_t)(b * Ho + oy) * Wo + ox) * C + oc) = y;
  }
}

// DET: the store pass of the deterministic mode (det_core.h): raw is the workspace, the tile's workgroups store their sums into
// slab blockIdx.x (a whole raw); DET = false is the kernel as it was
template <int CG, int S, bool DET = false>
__global__ __launch_bounds__(256) void conv_grouped_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ src,
                                                                 float* __restrict__ raw, int H, int W, int Ho, int Wo, int C,
                                                                 int tiles_x, int tiles_y) {
  constexpr int KC = CG < 32 ? CG : 32, NCH = CG / KC;
  constexpr int TH = S == 1 ? 8 : 4, TW = GC_TW, HH = (TH - 1) * S + 3, HW = (TW - 1) * S + 3, PS = 36, DS = 33;
  constexpr int NU = 32 * (KC / 4), NPL = 256 / NU, NPIX = TH * TW;
  constexpr int NSH = HH * HW * PS + NPIX * DS > 256 * 36 ? HH * HW * PS + NPIX * DS : 256 * 36;
  __shared__ __attribute__((aligned(16))) float sm[NSH];
  float* halo = sm;
  float* dzt = sm + HH * HW * PS;

  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int tx0 = (t % tiles_x) * TW;
  t /= tiles_x;
  const int ty0 = (t % tiles_y) * TH;
  const int b = t / tiles_y;
  const int ob = blockIdx.y / NCH, chunk = blockIdx.y % NCH;
  // the 32 source channels of this workgroup: the block's own (cg <= 32), or one half of its group's 64
  const int in_base = CG < 64 ? ob * 32 : (ob * 32 / CG) * CG + chunk * 32;

  for (int idx = tid; idx < HH * HW * 32; idx += 256) {
    const int px = idx >> 5, ch = idx & 31;
    const int sy = gc_src_coord(ty0, px / HW, S, H), sx = gc_src_coord(tx0, px % HW, S, W);
    float v = 0.f;
    if (sy >= 0 && sx >= 0 && in_base + ch < C) v = src[((size_t)(b * H + sy) * W + sx) * C + in_base + ch];
    halo[px * PS + ch] = v;
  }
  for (int idx = tid; idx < NPIX * 32; idx += 256) {
    const int px = idx >> 5, ch = idx & 31;
    const int oy = ty0 + px / TW, ox = tx0 + px % TW;
    float v = 0.f;
    if (oy < Ho && ox < Wo && ob * 32 + ch < C) v = dz[((size_t)(b * Ho + oy) * Wo + ox) * C + ob * 32 + ch];
    dzt[px * DS + ch] = v;
  }
  __syncthreads();

  const int u = tid % NU, pl = tid / NU;
  const int ol = u % 32, cq = u / 32;
  const int hch = (CG < 32 ? (ol / CG) * CG : 0) + 4 * cq;
  float acc[9][4];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
#pragma unroll 2
  for (int p = pl; p < NPIX; p += NPL) {
    const float d = dzt[p * DS + ol];
    const float* hp = halo + ((p / TW) * S * HW + (p % TW) * S) * PS + hch;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const f32x4 x4 = *reinterpret_cast<const f32x4*>(hp + ((k / 3) * HW + k % 3) * PS);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][j] += d * x4[j];
    }
  }
  __syncthreads();   // halo and dz are dead: the lanes' partial sums take their place
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) sm[(pl * NU + u) * 36 + 4 * k + j] = acc[k][j];
  __syncthreads();
  for (int v = tid; v < NU * 36; v += 256) {
    float s = sm[v];
#pragma unroll
    for (int l = 1; l < NPL; ++l) s += sm[l * NU * 36 + v];
    const int uu = v / 36, k = (v % 36) / 4, j = v % 4;
    const int o = ob * 32 + uu % 32;
    if (o < C)
      det_add<DET>(&raw[(DET ? det_slab_offset(blockIdx.x, (long)C * 9 * CG) : 0L) + gc_raw_index(CG, o, k, chunk * 32 + 4 * (uu / 32) + j)],
                   s);
  }
}

__global__ void pack_grouped_kernel(const float* __restrict__ w, float* __restrict__ packed, int C, int cg, int mode,
                                    long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  // invert gc_packed_index
  const int cb = gc_cb(cg), kc = gc_chunk(cg), nch = cg / kc;
  long r = i;
  const int ocl = (int)(r % cb);
  r /= cb;
  const int cl = (int)(r % kc);
  r /= kc;
  const int tap = (int)(r % 9);
  r /= 9;
  const int chunk = (int)(r % nch);
  const int oc = (int)(r / nch) * cb + ocl, c = chunk * kc + cl;
  packed[i] = oc < C ? w[gc_weight_index(mode, cg, oc, tap, c)] : 0.f;
}

template <template <int, int> class L, typename... A>
int dispatch(int cg, int stride, A... a) {
#define SFH_GC_CASE(CG)                                              \
  case CG:                                                           \
    return stride == 1 ? L<CG, 1>::launch(a...) : L<CG, 2>::launch(a...);
  switch (cg) {
    SFH_GC_CASE(4)
    SFH_GC_CASE(8)
    SFH_GC_CASE(16)
    SFH_GC_CASE(32)
    SFH_GC_CASE(64)
  }
#undef SFH_GC_CASE
  return SFH_E_ARG;
}

template <int CG, int S>
struct FwdLaunch {
  static int launch(const float* src, const float* wpacked, const float* scale, const float* shift, int relu, float* dst,
                    int batch, int H, int W, int C, hipStream_t st) {
    const int Ho = gc_out_size(H, S), Wo = gc_out_size(W, S);
    const int tx = sfh_cdiv(Wo, GC_TW), ty = sfh_cdiv(Ho, gc_tile_h(S));
    hipLaunchKernelGGL((conv_grouped_kernel<CG, S>), dim3((unsigned)(batch * ty * tx), (unsigned)sfh_cdiv(C, gc_cb(CG))),
                       dim3(256), 0, st, src, wpacked, scale, shift, relu, dst, H, W, Ho, Wo, C, tx, ty);
    return sfh_check_launch("conv_grouped_kernel");
  }
};

template <int CG, int S>
struct WgradLaunch {
  // ws == nullptr: the default mode, atomics onto raw; else the store pass into ws (slab per tile) and the sum pass
  static int launch(const float* dz, const float* src, float* raw, float* ws, int batch, int H, int W, int C, hipStream_t st) {
    const int Ho = gc_out_size(H, S), Wo = gc_out_size(W, S);
    const int tx = sfh_cdiv(Wo, GC_TW), ty = sfh_cdiv(Ho, gc_tile_h(S));
    const dim3 grid((unsigned)(batch * ty * tx), (unsigned)(sfh_cdiv(C, 32) * (CG / gc_chunk(CG))));
    if (!ws) {
      hipLaunchKernelGGL((conv_grouped_wgrad_kernel<CG, S>), grid, dim3(256), 0, st, dz, src, raw, H, W, Ho, Wo, C, tx, ty);
      return sfh_check_launch("conv_grouped_wgrad_kernel");
    }
    hipLaunchKernelGGL((conv_grouped_wgrad_kernel<CG, S, true>), grid, dim3(256), 0, st, dz, src, ws, H, W, Ho, Wo, C, tx, ty);
    if (int rc = sfh_check_launch("conv_grouped_wgrad_kernel (deterministic)")) return rc;
    const long elems = (long)C * 9 * CG;
    return sfh_det_reduce_f32(ws, (long)batch * ty * tx, elems, elems, CG, raw, CG, st);
  }
};

// the words for what det_grouped_plan (det_core.h) refuses: forward, backward-filter, its sibling and the size query refuse
// alike; nothing is launched after a refusal
int check_geometry(const char* who, const DetPlan& p, int batch, int H, int W, int groups, int cg, int stride) {
  SFH_REQUIRE(p.why != DET_BAD_CG, "%s: %d channels per group (4, 8, 16, 32 or 64)", who, cg);
  SFH_REQUIRE(p.why != DET_BAD_STRIDE, "%s: stride %d (1 or 2)", who, stride);
  SFH_REQUIRE(p.why != DET_BAD_FRAME, "%s: bad geometry batch=%d H=%d W=%d groups=%d", who, batch, H, W, groups);
  SFH_REQUIRE(p.ok, "%s: %d x %d x %d x %d groups too large", who, batch, H, W, groups);
  return SFH_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int64_t sfh_packed_grouped_weight_floats(int groups, int cg) {
  if (groups <= 0 || !gc_cg_ok(cg) || (long)groups * cg > 65536) return -1;
  return gc_packed_floats(groups, cg);
}

extern "C" int sfh_pack_grouped_weights(const float* w, float* packed, int groups, int cg, int mode, void* stream) {
  SFH_REQUIRE(w && packed, "pack_grouped_weights: null pointer");
  SFH_REQUIRE(groups > 0 && gc_cg_ok(cg) && (long)groups * cg <= 65536, "pack_grouped_weights: groups=%d cg=%d", groups, cg);
  SFH_REQUIRE(mode == 0 || mode == 1, "pack_grouped_weights: mode %d (0 forward, 1 backward-data)", mode);
  const long total = gc_packed_floats(groups, cg);
  hipLaunchKernelGGL(pack_grouped_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, packed,
                     groups * cg, cg, mode, total);
  return sfh_check_launch("pack_grouped_kernel");
}

extern "C" int sfh_conv_grouped_fwd(const float* src, const float* wpacked, const float* scale, const float* shift, int relu,
                                    float* dst, int batch, int H, int W, int groups, int cg, int stride, void* stream) {
  SFH_REQUIRE(src && wpacked && dst, "conv_grouped_fwd: null pointer");
  SFH_REQUIRE((scale == nullptr) == (shift == nullptr), "conv_grouped_fwd: scale and shift come together");
  const DetPlan p = det_grouped_plan(batch, H, W, groups, cg, stride);   // the forward admits what the backward-filter admits
  if (int rc = check_geometry("conv_grouped_fwd", p, batch, H, W, groups, cg, stride)) return rc;
  SFH_REQUIRE(aligned16(wpacked) && aligned16(dst) && aligned16(scale) && aligned16(shift),
              "conv_grouped_fwd: wpacked, dst, scale and shift must be 16-byte aligned");
  return dispatch<FwdLaunch>(cg, stride, src, wpacked, scale, shift, relu ? 1 : 0, dst, batch, H, W, groups * cg,
                             (hipStream_t)stream);
}

static int conv_grouped_wgrad_impl(const float* dz, const float* src, float* raw, int batch, int H, int W, int groups, int cg,
                                   int stride, bool det, void* workspace, long long workspace_bytes, void* stream) {
  const char* who = det ? "conv_grouped_wgrad_det" : "conv_grouped_wgrad";
  const DetPlan p = det_grouped_plan(batch, H, W, groups, cg, stride);
  SFH_REQUIRE(dz && src && raw, "%s: null pointer", who);
  if (int rc = check_geometry(who, p, batch, H, W, groups, cg, stride)) return rc;
  if (det) SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  return dispatch<WgradLaunch>(cg, stride, dz, src, raw, det ? (float*)workspace : (float*)nullptr, batch, H, W, groups * cg,
                               (hipStream_t)stream);
}

extern "C" int sfh_conv_grouped_wgrad(const float* dz, const float* src, float* raw, int batch, int H, int W, int groups,
                                      int cg, int stride, void* stream) {
  return conv_grouped_wgrad_impl(dz, src, raw, batch, H, W, groups, cg, stride, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_conv_grouped_wgrad_det_bytes(int batch, int H, int W, int groups, int cg, int stride) {
  return det_bytes(det_grouped_plan(batch, H, W, groups, cg, stride));
}

extern "C" int sfh_conv_grouped_wgrad_det(const float* dz, const float* src, float* raw, int batch, int H, int W, int groups,
                                          int cg, int stride, void* workspace, long long workspace_bytes, void* stream) {
  return conv_grouped_wgrad_impl(dz, src, raw, batch, H, W, groups, cg, stride, true, workspace, workspace_bytes, stream);
}
