// train_bn.hip - training-mode BatchNorm and the 2x2 max-pool of the hot path: batch statistics,
// normalisation forward / backward with the optional split copy, ReLU / max-pool backward and the kernels that fuse them.
//
// Replaces, for Reconstructor.forward in train() mode + loss.backward() (train.py:170,233):
//   nn.BatchNorm2d(training=True) fwd/bwd of DoubleConv / BasicBlock (unet/unet_parts.py:16,19,
//   models/resnet.py:67-74), nn.ReLU / nn.MaxPool2d backward.
// All activations fp32 NHWC with channel stride == channel count.
//
// Reductions over pixels accumulate in fp64 (ATen's CPU batch-norm uses a double accumulator).

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "common.h"
#include "bn_math.h"         // the BatchNorm arithmetic of every kernel below
#include "conv_epilogue.h"   // sfh_split4_h2: the two-plane fp16 split of the H2 format
#include "det_core.h"        // block counts, split plans and det_add: the deterministic mode's slabs
#include "train_reduce.h"    // red_tail

namespace {
// acc[0][c] += sum z, acc[1][c] += sum z^2
template <bool DET = false>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ z, long npix, int C,
                                                       double* __restrict__ acc) {
  __shared__ double sh[256];
  if constexpr (DET) acc += det_slab_offset(blockIdx.x, 2L * C);
  for (int c0 = 0; c0 < C; c0 += 1024) {
    const int cq = min(1024, C - c0) >> 2;
    const int lanes = 256 / cq;
    const int q = threadIdx.x % cq, pl = threadIdx.x / cq;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // [sum z | sum z^2] of the quad's four channels
    if (pl < lanes) {
      // every block streams ONE contiguous range of pixels, four pixels per iteration (64 B per thread in
      // flight; one 16-byte load per thread kept the chip at 2 TB/s).  Measured: 3.4-3.5 TB/s on the 0.94 GB tensors, which is what a read-only stream reaches here
      // (grid-stride order and 2048 blocks were no faster).
      const long chunk = (npix + gridDim.x - 1) / gridDim.x;
      const long pend = min(npix, (long)(blockIdx.x + 1) * chunk);
      const long stride = lanes;
      long p = (long)blockIdx.x * chunk + pl;
      const float* zc = z + c0 + 4 * q;
      for (; p + 3 * stride < pend; p += 4 * stride) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(zc + (p + u * stride) * C);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s[j] += (double)v[u][j];
            s[4 + j] += (double)v[u][j] * (double)v[u][j];
          }
      }
      for (; p < pend; p += stride) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(zc + p * C);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s[j] += (double)v[j];
          s[4 + j] += (double)v[j] * (double)v[j];
        }
      }
    }
    red_tail<DET>(s, pl < lanes, cq, sh, acc + c0, C);
  }
}
}  // namespace

// An accumulating entry, its deterministic sibling (sfh_*_det, include/sfh_amd.h: same arguments + (workspace,
// workspace_bytes)) and its size query (sfh_*_det_bytes) share one plan (det_core.h): the two entries forward into one static
// function (ws == nullptr, 0 bytes for the plain entry), which checks what the query does not see, refuses what the plan
// refuses, in deterministic mode checks the workspace (SFH_REQUIRE_WS), launches the DET = det instantiation and then runs the
// sum pass (sfh_det_reduce_*) onto the destination; the query answers det_bytes(plan).
static int bn_stats_impl(const float* z, int64_t npix, int C, double* acc, bool det, void* ws, long long ws_bytes, void* stream) {
  const char* who = det ? "bn_stats_det" : "bn_stats";
  const DetPlan p = det_red_plan((long)npix, C, 2);
  SFH_REQUIRE(z && acc && p.ok, "%s: bad argument", who);
  if (det) SFH_REQUIRE_WS(who, ws, ws_bytes, p);
  SFH_LAUNCH_DET(bn_stats_kernel, det, dim3((unsigned)p.slabs), dim3(256), stream, z, (long)npix, C, det ? (double*)ws : acc);
  if (int rc = sfh_check_launch(det ? "bn_stats_kernel (deterministic)" : "bn_stats_kernel")) return rc;
  return det ? sfh_det_reduce_f64((const double*)ws, p.slabs, p.elems, p.elems, 2 * C, acc, 2 * C, stream) : SFH_OK;
}

extern "C" int sfh_bn_stats(const float* z, int64_t npix, int C, double* acc, void* stream) {
  return bn_stats_impl(z, npix, C, acc, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_bn_stats_det_bytes(int64_t npix, int C) { return det_bytes(det_red_plan((long)npix, C, 2)); }

extern "C" int sfh_bn_stats_det(const float* z, int64_t npix, int C, double* acc, void* workspace, long long workspace_bytes,
                                void* stream) {
  return bn_stats_impl(z, npix, C, acc, true, workspace, workspace_bytes, stream);
}

namespace {
// acc[k] += sum_r partial[r][k], k < 2 * C: the per-wave fp64 sums a convolution's epilogue left (sfh_conv_desc.stats_partial).
// Block = 64 columns x 4 row lanes; blockIdx.y strides over the rows.
__global__ __launch_bounds__(256) void bn_stats_partials_kernel(const double* __restrict__ partial, int rows, int ncol,
                                                                double* __restrict__ acc) {
  __shared__ double sh[256];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  double s = 0.0;
  if (col < ncol)
    for (int r = blockIdx.y * 4 + rl; r < rows; r += gridDim.y * 4) s += partial[(long)r * ncol + col];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < 64 && col < ncol)
    unsafeAtomicAdd(&acc[col], sh[threadIdx.x] + sh[threadIdx.x + 64] + sh[threadIdx.x + 128] + sh[threadIdx.x + 192]);
}
}  // namespace

extern "C" int sfh_bn_stats_partials(const double* partial, int rows, int C, double* acc, void* stream) {
  SFH_REQUIRE(partial && acc && rows > 0 && C > 0, "bn_stats_partials: bad argument");
  const int ncol = 2 * C;
  const dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)(rows >= 128 ? 32 : (rows + 3) / 4));
  hipLaunchKernelGGL(bn_stats_partials_kernel, grid, dim3(256), 0, (hipStream_t)stream, partial, rows, ncol, acc);
  return sfh_check_launch("bn_stats_partials_kernel");
}

namespace {
// acc[c] += sum x[:, c] over a channel slice (cs >= C)
template <bool DET = false>
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, long npix, int C, int cs,
                                                     double* __restrict__ acc) {
  // one channel quad per thread column; supports cs >= C (channel slices)
  __shared__ double sh[256];
  if constexpr (DET) acc += det_slab_offset(blockIdx.x, C);
  const int cq = C >> 2;
  for (int q0 = 0; q0 < cq; q0 += 256) {
    const int qn = min(256, cq - q0);
    const int lanes = 256 / qn;
    const int q = threadIdx.x % qn, pl = threadIdx.x / qn;
    double s[4] = {0, 0, 0, 0};
    if (pl < lanes)
      for (long p = (long)blockIdx.x * lanes + pl; p < npix; p += (long)gridDim.x * lanes) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + p * cs + 4 * (q0 + q));
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += (double)v[j];
      }
    red_tail<DET>(s, pl < lanes, qn, sh, acc + 4 * q0, 0);
  }
}
}  // namespace

static int colsum_impl(const float* x, int64_t npix, int C, int cs, double* acc, bool det, void* ws, long long ws_bytes,
                       void* stream) {
  const char* who = det ? "colsum_det" : "colsum";
  const DetPlan p = det_red_plan((long)npix, C, 1);
  SFH_REQUIRE(x && acc && p.ok && cs >= C && cs % 4 == 0, "%s: bad argument", who);
  if (det) SFH_REQUIRE_WS(who, ws, ws_bytes, p);
  SFH_LAUNCH_DET(colsum_kernel, det, dim3((unsigned)p.slabs), dim3(256), stream, x, (long)npix, C, cs, det ? (double*)ws : acc);
  if (int rc = sfh_check_launch(det ? "colsum_kernel (deterministic)" : "colsum_kernel")) return rc;
  return det ? sfh_det_reduce_f64((const double*)ws, p.slabs, p.elems, p.elems, C, acc, C, stream) : SFH_OK;
}

extern "C" int sfh_colsum(const float* x, int64_t npix, int C, int cs, double* acc, void* stream) {
  return colsum_impl(x, npix, C, cs, acc, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_colsum_det_bytes(int64_t npix, int C) { return det_bytes(det_red_plan((long)npix, C, 1)); }

extern "C" int sfh_colsum_det(const float* x, int64_t npix, int C, int cs, double* acc, void* workspace,
                              long long workspace_bytes, void* stream) {
  return colsum_impl(x, npix, C, cs, acc, true, workspace, workspace_bytes, stream);
}

namespace {
__global__ void bn_finalize_kernel(const double* __restrict__ acc, long npix, int C, float eps, float momentum,
                                   float* __restrict__ running_mean, float* __restrict__ running_var,
                                   float* __restrict__ mean_invstd, long* __restrict__ num_batches_tracked) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;   // nn.BatchNorm2d's counter (one launch less per layer)
  if (c >= C) return;
  bn_finalize_channel(acc[c], acc[C + c], npix, eps, momentum, C, c, mean_invstd, running_mean, running_var);
}
}  // namespace

extern "C" int sfh_bn_finalize(const double* acc, int64_t npix, int C, float eps, float momentum,
                               float* running_mean, float* running_var, float* mean_invstd, int64_t* num_batches_tracked,
                               void* stream) {
  SFH_REQUIRE(acc && mean_invstd && npix > 0 && C > 0, "bn_finalize: bad argument");
  SFH_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize: running stats must come in pairs");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, acc,
                     (long)npix, C, eps, momentum, running_mean, running_var, mean_invstd, (long*)num_batches_tracked);
  return sfh_check_launch("bn_finalize_kernel");
}

namespace {
// bn_stats_partials + bn_finalize in ONE launch (round 6: a training step had 54 such pairs): a workgroup of 16 row lanes x 64
// channels sums the (rows, 2, C) table of per-wave sums a conv epilogue left - in a fixed order, no atomics - and finishes
// mean / invstd / running statistics for its 64 channels.
__global__ __launch_bounds__(1024) void bn_finalize_partials_kernel(const double* __restrict__ partial, int rows, long npix,
                                                                    int C, float eps, float momentum,
                                                                    float* __restrict__ running_mean,
                                                                    float* __restrict__ running_var,
                                                                    float* __restrict__ mean_invstd,
                                                                    long* __restrict__ num_batches_tracked) {
  __shared__ double sh[2][16][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s0 = 0.0, s1 = 0.0;
  if (c < C)
    for (int r = rl; r < rows; r += 16) {
      s0 += partial[(long)r * 2 * C + c];
      s1 += partial[(long)r * 2 * C + C + c];
    }
  sh[0][rl][cl] = s0;
  sh[1][rl][cl] = s1;
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches_tracked) *num_batches_tracked += 1;
  if (rl != 0 || c >= C) return;
#pragma unroll
  for (int k = 1; k < 16; ++k) {
    s0 += sh[0][k][cl];
    s1 += sh[1][k][cl];
  }
  bn_finalize_channel(s0, s1, npix, eps, momentum, C, c, mean_invstd, running_mean, running_var);
}
}  // namespace

extern "C" int sfh_bn_finalize_partials(const double* partial, int rows, int64_t npix, int C, float eps, float momentum,
                                        float* running_mean, float* running_var, float* mean_invstd,
                                        int64_t* num_batches_tracked, void* stream) {
  SFH_REQUIRE(partial && mean_invstd && rows > 0 && npix > 0 && C > 0, "bn_finalize_partials: bad argument");
  SFH_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize_partials: running stats must come in pairs");
  hipLaunchKernelGGL(bn_finalize_partials_kernel, dim3((unsigned)((C + 63) / 64)), dim3(1024), 0, (hipStream_t)stream, partial,
                     rows, (long)npix, C, eps, momentum, running_mean, running_var, mean_invstd, (long*)num_batches_tracked);
  return sfh_check_launch("bn_finalize_partials_kernel");
}

namespace {
// g = dy * (y > 0 if relu); sums: [0] = sum g, [1] = sum g * xhat
// relu with y == nullptr: the layer has no residual, so the ReLU decision y > 0 is recomputed from z (bn_math.h) instead
// of reading y: 8 instead of 12 bytes per element.
template <bool DET = false>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ z, const float* __restrict__ mi,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            int relu, long npix, int C, double* __restrict__ acc) {
  const bool sign_from_z = relu && !y;
  __shared__ double sh[256];
  if constexpr (DET) acc += det_slab_offset(blockIdx.x, 2L * C);
  for (int c0 = 0; c0 < C; c0 += 1024) {
    const int cq = min(1024, C - c0) >> 2;
    const int lanes = 256 / cq;
    const int q = threadIdx.x % cq, pl = threadIdx.x / cq;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pl < lanes) {
      const long stride = (long)gridDim.x * lanes;
      long p = (long)blockIdx.x * lanes + pl;
      const BnChannels<4> bn = bn_load<4>(mi, gamma, beta, C, c0 + 4 * q, sign_from_z);
      auto add = [&](const f32x4& g, const f32x4& zz, const f32x4& yy) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gj = bn_gate(sign_from_z ? bn.y(j, zz[j]) : yy[j], g[j]);
          s[j] += (double)gj;
          s[4 + j] += (double)gj * (double)bn.xhat(j, zz[j]);
        }
      };
      // two pixels per iteration: six 16-byte loads per thread in flight
      for (; p + stride < npix; p += 2 * stride) {
        const long o0 = p * C + c0 + 4 * q, o1 = (p + stride) * C + c0 + 4 * q;
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(dy + o0), g1 = *reinterpret_cast<const f32x4*>(dy + o1);
        const f32x4 z0 = *reinterpret_cast<const f32x4*>(z + o0), z1 = *reinterpret_cast<const f32x4*>(z + o1);
        f32x4 y0 = {1.f, 1.f, 1.f, 1.f}, y1 = {1.f, 1.f, 1.f, 1.f};
        if (relu && y) {
          y0 = *reinterpret_cast<const f32x4*>(y + o0);
          y1 = *reinterpret_cast<const f32x4*>(y + o1);
        }
        add(g0, z0, y0);
        add(g1, z1, y1);
      }
      for (; p < npix; p += stride) {
        const long o = p * C + c0 + 4 * q;
        f32x4 yy = {1.f, 1.f, 1.f, 1.f};
        if (relu && y) yy = *reinterpret_cast<const f32x4*>(y + o);
        add(*reinterpret_cast<const f32x4*>(dy + o), *reinterpret_cast<const f32x4*>(z + o), yy);
      }
    }
    red_tail<DET>(s, pl < lanes, cq, sh, acc + c0, C);
  }
}
}  // namespace

static int bn_bwd_reduce_impl(const float* dy, const float* y, const float* z, const float* mean_invstd, const float* gamma,
                              const float* beta, int relu, int64_t npix, int C, double* acc, bool det, void* ws,
                              long long ws_bytes, void* stream) {
  const char* who = det ? "bn_bwd_reduce_det" : "bn_bwd_reduce";
  const DetPlan p = det_red_plan((long)npix, C, 2);
  SFH_REQUIRE(dy && z && mean_invstd && acc && (y || !relu || (gamma && beta)) && p.ok,
              "%s: bad argument (relu needs y, or gamma and beta to recompute its sign from z)", who);
  if (det) SFH_REQUIRE_WS(who, ws, ws_bytes, p);
  SFH_LAUNCH_DET(bn_bwd_reduce_kernel, det, dim3((unsigned)p.slabs), dim3(256), stream, dy, y, z, mean_invstd, gamma, beta, relu,
                 (long)npix, C, det ? (double*)ws : acc);
  if (int rc = sfh_check_launch(det ? "bn_bwd_reduce_kernel (deterministic)" : "bn_bwd_reduce_kernel")) return rc;
  return det ? sfh_det_reduce_f64((const double*)ws, p.slabs, p.elems, p.elems, 2 * C, acc, 2 * C, stream) : SFH_OK;
}

extern "C" int sfh_bn_bwd_reduce(const float* dy, const float* y, const float* z, const float* mean_invstd,
                                 const float* gamma, const float* beta, int relu, int64_t npix, int C, double* acc,
                                 void* stream) {
  return bn_bwd_reduce_impl(dy, y, z, mean_invstd, gamma, beta, relu, npix, C, acc, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_bn_bwd_reduce_det_bytes(int64_t npix, int C) { return sfh_bn_stats_det_bytes(npix, C); }

extern "C" int sfh_bn_bwd_reduce_det(const float* dy, const float* y, const float* z, const float* mean_invstd,
                                     const float* gamma, const float* beta, int relu, int64_t npix, int C, double* acc,
                                     void* workspace, long long workspace_bytes, void* stream) {
  return bn_bwd_reduce_impl(dy, y, z, mean_invstd, gamma, beta, relu, npix, C, acc, true, workspace, workspace_bytes, stream);
}

namespace {
// y = [relu]( (z - mean) * invstd * gamma + beta [+ residual] )
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ mi,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ residual, int relu, long total4,
                                                       int C, float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const f32x4 v = reinterpret_cast<const f32x4*>(z)[i];
  const BnChannels<4> bn = bn_load<4>(mi, gamma, beta, C, c);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = bn.y(j, v[j]);
  if (residual) {
    const f32x4 r = reinterpret_cast<const f32x4*>(residual)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] += r[j];
  }
  if (relu) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = sfh_relu(o[j]);
  }
  reinterpret_cast<f32x4*>(y)[i] = o;
}

// dz = gamma * invstd * (g - sum_g / N - xhat * sum_gx / N); optionally dres = g
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ z, const float* __restrict__ mi,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const double* __restrict__ acc, int relu, long npix, long total4,
                                                           int C, float* __restrict__ dz, float* __restrict__ dres,
                                                           float* __restrict__ acc_f32) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (acc_f32 && blockIdx.x == 0)   // dbeta | dgamma as float32 for the caller (one conversion launch less per layer)
    for (int k = threadIdx.x; k < 2 * C; k += 256) acc_f32[k] = (float)acc[k];
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const bool sign_from_z = relu && !y;   // (see bn_bwd_reduce_kernel)
  const f32x4 g4 = reinterpret_cast<const f32x4*>(dy)[i];
  const f32x4 zz = reinterpret_cast<const f32x4*>(z)[i];
  f32x4 yy = {1.f, 1.f, 1.f, 1.f};
  if (relu && y) yy = reinterpret_cast<const f32x4*>(y)[i];
  const BnChannels<4> bn = bn_load<4, true>(mi, gamma, beta, C, c, sign_from_z, acc, bn_inv_n(npix));
  f32x4 o, gg;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gg[j] = bn_gate(sign_from_z ? bn.y(j, zz[j]) : yy[j], g4[j]);
    o[j] = bn.dz(j, zz[j], gg[j]);
  }
  reinterpret_cast<f32x4*>(dz)[i] = o;
  if (dres) reinterpret_cast<f32x4*>(dres)[i] = gg;
}

// ------------------------------------------------------------------ BatchNorm kernels with an S3 copy
// Same arithmetic as bn_apply / bn_bwd_apply, with the thread mapping of f32_to_s3 (one thread = 8
// channels of one pixel, a wave = 16 pixels x the 4 groups of a 32-channel block) so that the result is
// written twice in one pass: fp32 NHWC (for BatchNorm backward and the backward-filter kernel) and the
// split-bf16 S3 layout (B*H, C/32, 3, 4, W, 8) that the next convolution reads.  C % 32 == 0.
typedef unsigned short tr_u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void tr_split8(const float (&v)[8], unsigned short* __restrict__ dst, long e, long ps) {
  tr_u16x8 p0, p1, p2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 v0 = (__bf16)v[j];
    const float r1 = v[j] - (float)v0;
    const __bf16 v1 = (__bf16)r1;
    const __bf16 v2 = (__bf16)(r1 - (float)v1);
    p0[j] = __builtin_bit_cast(unsigned short, v0);
    p1[j] = __builtin_bit_cast(unsigned short, v1);
    p2[j] = __builtin_bit_cast(unsigned short, v2);
  }
  *reinterpret_cast<tr_u16x8*>(dst + e) = p0;
  *reinterpret_cast<tr_u16x8*>(dst + e + ps) = p1;
  *reinterpret_cast<tr_u16x8*>(dst + e + 2 * ps) = p2;
}

__device__ __forceinline__ long tr_s3_elem(long row, int x, int c, int W, int C, int np) {
  return ((((row * (C >> 5) + (c >> 5)) * np) * 4 + ((c & 31) >> 3)) * W + x) * 8;
}

// the same 8 values as two fp16 planes (H2 format, include/sfh_amd.h); `over`: see sfh_split4_h2
__device__ __forceinline__ void tr_split8_h2(const float (&v)[8], unsigned short* __restrict__ dst, long e, long ps,
                                             unsigned& over) {
  u32x2 pa[2], pb[2];
  sfh_split4_h2((f32x4){v[0], v[1], v[2], v[3]}, kSfhH2Scale, pa, over);
  sfh_split4_h2((f32x4){v[4], v[5], v[6], v[7]}, kSfhH2Scale, pb, over);
  typedef unsigned int tr_u32x4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<tr_u32x4*>(dst + e) = (tr_u32x4){pa[0][0], pa[0][1], pb[0][0], pb[0][1]};
  *reinterpret_cast<tr_u32x4*>(dst + e + ps) = (tr_u32x4){pa[1][0], pa[1][1], pb[1][0], pb[1][1]};
}

// 8 channels (c0 ..) of pixel (row, x) into the NP planes of a (rows, C/32, NP, 4, W, 8) tensor; a kernel of the H2 format
// collects `over` across its stores and ends with tr_report
template <int NP>   // planes of the split copy: 3 = S3 (bf16), 2 = H2 (fp16)
__device__ __forceinline__ void tr_store_split(const float (&v)[8], unsigned short* __restrict__ dst, long row, int x, int c0,
                                               int W, int C, unsigned& over) {
  const long e = tr_s3_elem(row, x, c0, W, C, NP), ps = 4L * W * 8;
  if constexpr (NP == 3) tr_split8(v, dst, e, ps);
  else tr_split8_h2(v, dst, e, ps, over);
}

template <int NP>
__device__ __forceinline__ void tr_report(unsigned* __restrict__ overflow, unsigned over) {
  if constexpr (NP == 2)
    if (overflow && sfh_h2_out_of_range(over)) atomicOr(overflow, 1u);
}

// the <2> or <3> instance of a split kernel by the launcher's split_fmt (checked to be S3 or H2), 256 threads
#define SFH_LAUNCH_SPLIT(kernel, split_fmt, grid, stream, ...)                                     \
  do {                                                                                             \
    if ((split_fmt) == SFH_FMT_H2)                                                                 \
      hipLaunchKernelGGL(kernel<2>, grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);       \
    else                                                                                           \
      hipLaunchKernelGGL(kernel<3>, grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);       \
  } while (0)

// Thread mapping of the two kernels below: a workgroup = 64 consecutive pixels (of the flattened (rows, W) tensor) x one
// 32-channel block, wave g of it = channel group g (8 channels): the per-channel terms are wave-uniform (scalar loads, no
// vector-memory traffic beside the tensors themselves) and a wave's split-layout store is one 1 KB run per plane.  The
// fp32 copy (y / dz) is optional: a layer whose only consumers read the split copy skips a third of its traffic.
__device__ __forceinline__ bool tr_block_thread(long npix, int W, int C, long& p, long& row, int& x, int& c0) {
  const int nb = C >> 5;
  const int cb = (int)(blockIdx.x % (unsigned)nb);
  const long chunk = (long)(blockIdx.x / (unsigned)nb);
  const int g = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  c0 = cb * 32 + g * 8;
  p = chunk * 64 + (threadIdx.x & 63);
  const unsigned r32 = (unsigned)p / (unsigned)W;   // the launchers require npix < 2^31
  row = (long)r32;
  x = (int)((unsigned)p - r32 * (unsigned)W);
  return p < npix;
}

template <int NP>   // planes of the split copy: 3 = S3 (bf16), 2 = H2 (fp16)
__global__ __launch_bounds__(256) void bn_apply_s3_kernel(const float* __restrict__ z, const float* __restrict__ mi,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ residual, int relu, long npix, int W,
                                                          int C, float* __restrict__ y,
                                                          unsigned short* __restrict__ y_s3, unsigned* __restrict__ overflow) {
  long p, row; int x, c0;
  const bool live = tr_block_thread(npix, W, C, p, row, x, c0);
  const BnChannels<8> bn = bn_load<8>(mi, gamma, beta, C, c0);
  if (!live) return;
  const long o = p * C + c0;
  float v[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 zz = *reinterpret_cast<const f32x4*>(z + o + 4 * h);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[4 * h + j] = bn.y(4 * h + j, zz[j]);
    if (residual) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(residual + o + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * h + j] += r[j];
    }
  }
  if (relu) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = sfh_relu(v[j]);
  }
  if (y) {
    *reinterpret_cast<f32x4*>(y + o) = (f32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(y + o + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  }
  unsigned over = 0u;
  tr_store_split<NP>(v, y_s3, row, x, c0, W, C, over);
  tr_report<NP>(overflow, over);
}

template <int NP>
__global__ __launch_bounds__(256) void bn_bwd_apply_s3_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ z, const float* __restrict__ mi,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const double* __restrict__ acc, int relu, long npix, int W,
                                                              int C, float* __restrict__ dz, float* __restrict__ dres,
                                                              float* __restrict__ acc_f32,
                                                              unsigned short* __restrict__ dz_s3, unsigned* __restrict__ overflow) {
  if (acc_f32 && blockIdx.x == 0)   // dbeta | dgamma as float32 for the caller (one conversion launch less per layer)
    for (int k = threadIdx.x; k < 2 * C; k += 256) acc_f32[k] = (float)acc[k];
  long p, row; int x, c0;
  const bool live = tr_block_thread(npix, W, C, p, row, x, c0);
  const bool sign_from_z = relu && !y;   // (see bn_bwd_reduce_kernel)
  const BnChannels<8> bn = bn_load<8, true>(mi, gamma, beta, C, c0, sign_from_z, acc, bn_inv_n(npix));
  if (!live) return;
  const long o = p * C + c0;
  float v[8], gg[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(dy + o + 4 * h);
    const f32x4 zz = *reinterpret_cast<const f32x4*>(z + o + 4 * h);
    f32x4 yy = {1.f, 1.f, 1.f, 1.f};
    if (relu && y) yy = *reinterpret_cast<const f32x4*>(y + o + 4 * h);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gg[4 * h + j] = bn_gate(sign_from_z ? bn.y(4 * h + j, zz[j]) : yy[j], g4[j]);
      v[4 * h + j] = bn.dz(4 * h + j, zz[j], gg[4 * h + j]);
    }
  }
  if (dz) {
    *reinterpret_cast<f32x4*>(dz + o) = (f32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dz + o + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  }
  if (dres) {
    *reinterpret_cast<f32x4*>(dres + o) = (f32x4){gg[0], gg[1], gg[2], gg[3]};
    *reinterpret_cast<f32x4*>(dres + o + 4) = (f32x4){gg[4], gg[5], gg[6], gg[7]};
  }
  unsigned over = 0u;
  tr_store_split<NP>(v, dz_s3, row, x, c0, W, C, over);
  tr_report<NP>(overflow, over);
}
}  // namespace

extern "C" int sfh_bn_apply(const float* z, const float* mean_invstd, const float* gamma, const float* beta,
                            const float* residual, int relu, int64_t npix, int C, float* y, void* y_s3, int W,
                            int split_fmt, uint32_t* overflow, void* stream) {
  SFH_REQUIRE(z && mean_invstd && gamma && beta && (y || y_s3) && npix > 0 && C > 0 && C % 4 == 0, "bn_apply: bad argument");
  if (y_s3) {
    SFH_REQUIRE(C % 32 == 0 && W > 0 && npix % W == 0, "bn_apply: the split copy needs C %% 32 == 0 and npix = rows * W");
    SFH_REQUIRE(split_fmt == SFH_FMT_S3 || split_fmt == SFH_FMT_H2, "bn_apply: split_fmt=%d (S3 or H2)", split_fmt);
    const long nblk = ((long)npix + 63) / 64 * (C / 32);
    SFH_REQUIRE(nblk < (1L << 31) && npix < (1L << 31) - 64, "bn_apply: tensor too large for one launch");
    SFH_LAUNCH_SPLIT(bn_apply_s3_kernel, split_fmt, dim3((unsigned)nblk), stream, z, mean_invstd, gamma, beta, residual, relu,
                     (long)npix, W, C, y, (unsigned short*)y_s3, overflow);
    return sfh_check_launch("bn_apply_s3_kernel");
  }
  const long total4 = (long)npix * C / 4;
  hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z,
                     mean_invstd, gamma, beta, residual, relu, total4, C, y);
  return sfh_check_launch("bn_apply_kernel");
}

extern "C" int sfh_bn_bwd_apply(const float* dy, const float* y, const float* z, const float* mean_invstd,
                                const float* gamma, const float* beta, const double* acc, int relu, int64_t npix, int C,
                                float* dz, float* dres, void* dz_s3, int W, int split_fmt, uint32_t* overflow,
                                float* acc_f32, void* stream) {
  SFH_REQUIRE(dy && z && mean_invstd && gamma && acc && (dz || dz_s3) && (y || !relu || beta) && npix > 0 && C > 0 &&
                  C % 4 == 0,
              "bn_bwd_apply: bad argument (relu needs y, or beta to recompute its sign from z)");
  if (dz_s3) {
    SFH_REQUIRE(C % 32 == 0 && W > 0 && npix % W == 0, "bn_bwd_apply: the split copy needs C %% 32 == 0 and npix = rows * W");
    SFH_REQUIRE(split_fmt == SFH_FMT_S3 || split_fmt == SFH_FMT_H2, "bn_bwd_apply: split_fmt=%d (S3 or H2)", split_fmt);
    const long nblk = ((long)npix + 63) / 64 * (C / 32);
    SFH_REQUIRE(nblk < (1L << 31) && npix < (1L << 31) - 64, "bn_bwd_apply: tensor too large for one launch");
    SFH_LAUNCH_SPLIT(bn_bwd_apply_s3_kernel, split_fmt, dim3((unsigned)nblk), stream, dy, y, z, mean_invstd, gamma, beta, acc,
                     relu, (long)npix, W, C, dz, dres, acc_f32, (unsigned short*)dz_s3, overflow);
    return sfh_check_launch("bn_bwd_apply_s3_kernel");
  }
  const long total4 = (long)npix * C / 4;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     dy, y, z, mean_invstd, gamma, beta, acc, relu, (long)npix, total4, C, dz, dres, acc_f32);
  return sfh_check_launch("bn_bwd_apply_kernel");
}

namespace {
// ------------------------------------------------------------------ ConvTranspose2d(2, stride 2) backward, first pass
// du (B, 2h, 2w, cout) fp32 -> s (B, h, w, 4 * cout) in the split format ONLY, s[(py * 2 + px) * cout + co] at (y, x) =
// du[2y + py][2x + px][co] (the 1x1 backward-data conv and the backward-filter kernel of the transposed conv read nothing
// else), and acc[co] += sum over pixels of du[..., co] - the bias gradient - from the same read.  Replaces colsum +
// space_to_depth2 + f32_to_h2 (three passes, 20 bytes per element) by one of 8.  Mapping as tr_block_thread, but a block
// strides over many 64-pixel chunks so that its column sums end in one fp64 atomic per channel and wave.
template <int NP>
__global__ __launch_bounds__(256) void s2d_split_colsum_kernel(const float* __restrict__ du, int h, int w, int cout,
                                                               long npix, long nchunks, int chunk_stride,
                                                               unsigned short* __restrict__ s_split,
                                                               double* __restrict__ acc, int acc_rows,
                                                               unsigned* __restrict__ overflow) {
  const int C4 = 4 * cout, nb = C4 >> 5;
  const int cb = (int)(blockIdx.x % (unsigned)nb);
  const int g = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int c0 = cb * 32 + g * 8;
  const int par = c0 / cout, co = c0 - par * cout, py = par >> 1, px = par & 1;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned over = 0u;
  // four chunks per iteration, all eight 16-byte loads of a lane issued before the first value is used
  for (long chunk = (long)(blockIdx.x / (unsigned)nb); chunk < nchunks; chunk += 4L * chunk_stride) {
    f32x4 a[4], bq[4];
    unsigned rowu[4];
    int xu[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long p = (chunk + (long)u * chunk_stride) * 64 + (threadIdx.x & 63);
      ok[u] = chunk + (long)u * chunk_stride < nchunks && p < npix;
      const unsigned pu = ok[u] ? (unsigned)p : 0u;             // (npix < 2^31: checked by the launcher)
      rowu[u] = pu / (unsigned)w;                               // b * h + y
      xu[u] = (int)(pu - rowu[u] * (unsigned)w);
      const unsigned b = rowu[u] / (unsigned)h, y = rowu[u] - b * (unsigned)h;
      const float* sp = du + (((long)b * 2 * h + 2 * y + py) * (2L * w) + 2 * xu[u] + px) * cout + co;
      a[u] = bq[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (ok[u]) {
        a[u] = *reinterpret_cast<const f32x4*>(sp);
        bq[u] = *reinterpret_cast<const f32x4*>(sp + 4);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!ok[u]) continue;
      const float v[8] = {a[u][0], a[u][1], a[u][2], a[u][3], bq[u][0], bq[u][1], bq[u][2], bq[u][3]};
#ifndef SFH_S2D_NOSUM   // (experiment build: without the column sums)
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += (double)v[j];
#endif
      tr_store_split<NP>(v, s_split, (long)rowu[u], xu[u], c0, w, C4, over);
    }
  }
  tr_report<NP>(overflow, over);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double t = s[j];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    // (same-address fp64 atomics are what this kernel would otherwise wait for: 4096 blocks on ONE row of 64 addresses ran
    // at 3.5 TB/s, on 32 rows at the 5 TB/s of the plain BatchNorm pass - profiles/r05_s2d_atomics.txt)
    if ((threadIdx.x & 63) == 0)
      unsafeAtomicAdd(&acc[(size_t)((blockIdx.x / (unsigned)nb) % (unsigned)acc_rows) * (size_t)cout + co + j], t);
  }
}
}  // namespace

extern "C" int sfh_s2d_split_colsum(const float* du, int batch, int h, int w, int cout, void* s_split, int split_fmt,
                                    double* acc, int acc_rows, uint32_t* overflow, void* stream) {
  SFH_REQUIRE(du && s_split && acc && batch > 0 && h > 0 && w > 0 && cout > 0 && cout % 8 == 0 && acc_rows >= 1 && acc_rows <= 4096,
              "s2d_split_colsum: bad argument (cout %% 8 == 0, 1 <= acc_rows <= 4096)");
  SFH_REQUIRE(split_fmt == SFH_FMT_S3 || split_fmt == SFH_FMT_H2, "s2d_split_colsum: split_fmt=%d (S3 or H2)", split_fmt);
  const long npix = (long)batch * h * w;
  SFH_REQUIRE(npix < (1L << 31) - 64 && (long)batch * 2 * h < (1L << 31), "s2d_split_colsum: tensor too large for one launch");
  const int nb = 4 * cout / 32;
  const long nchunks = (npix + 63) / 64;
#ifdef SFH_S2D_BLOCKS                          // (experiment build: another number of blocks)
  long per = SFH_S2D_BLOCKS / nb;
#else
  long per = 4096 / nb;                       // about 4096 blocks: 16 per CU, each striding over its share of the chunks
#endif
  if (per < 1) per = 1;
  if (per > nchunks) per = nchunks;
  SFH_LAUNCH_SPLIT(s2d_split_colsum_kernel, split_fmt, dim3((unsigned)(per * nb)), stream, du, h, w, cout, npix, nchunks,
                   (int)per, (unsigned short*)s_split, acc, acc_rows, overflow);
  return sfh_check_launch("s2d_split_colsum_kernel");
}

namespace {
// ------------------------------------------------------------------ max-pool 2x2 (floor)
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float* __restrict__ x, int H, int W, int C,
                                                           int Ho, int Wo, long total4, float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int cq = C >> 2;
  const int q = (int)(i % cq);
  long r = i / cq;
  const int xo = (int)(r % Wo); r /= Wo;
  const int yo = (int)(r % Ho);
  const long b = r / Ho;
  const float* p = x + ((b * H + 2 * yo) * (long)W + 2 * xo) * C + 4 * q;
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), bq = *reinterpret_cast<const f32x4*>(p + C);
  const f32x4 c = *reinterpret_cast<const f32x4*>(p + (long)W * C), d = *reinterpret_cast<const f32x4*>(p + (long)W * C + C);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = sfh_max_nan(sfh_max_nan(a[j], bq[j]), sfh_max_nan(c[j], d[j]));
  reinterpret_cast<f32x4*>(y)[i] = o;
}
}  // namespace

extern "C" int sfh_maxpool2_fwd(const float* x, float* y, int batch, int H, int W, int C, void* stream) {
  SFH_REQUIRE(x && y && batch > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "maxpool2_fwd: bad argument");
  const int Ho = H / 2, Wo = W / 2;
  const long total4 = (long)batch * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     H, W, C, Ho, Wo, total4, y);
  return sfh_check_launch("maxpool2_fwd_kernel");
}

namespace {
// dx[b,y,x,c] (+)= dy[b,y/2,x/2,c] where (y,x) is the FIRST maximum of its window in scan order
// (ATen's max_pool2d keeps the first index), 0 elsewhere (incl. the floor-cropped border).
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           int H, int W, int C, int Ho, int Wo, long total4,
                                                           int accumulate, float* __restrict__ dx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // one thread per pooled output quad
  if (i >= total4) return;
  const int cq = C >> 2;
  const int q = (int)(i % cq);
  long r = i / cq;
  const int xo = (int)(r % Wo); r /= Wo;
  const int yo = (int)(r % Ho);
  const long b = r / Ho;
  const long base = ((b * H + 2 * yo) * (long)W + 2 * xo) * C + 4 * q;
  const long off[4] = {0, C, (long)W * C, (long)W * C + C};
  f32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(x + base + off[k]);
  const f32x4 g = reinterpret_cast<const f32x4*>(dy)[i];
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int best = 0;
    float bv = v[0][j];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (v[k][j] > bv) { bv = v[k][j]; best = k; }
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k][j] = (k == best) ? g[j] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f32x4* d = reinterpret_cast<f32x4*>(dx + base + off[k]);
    if (accumulate) {
      f32x4 t = *d;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] += o[k][j];
      *d = t;
    } else {
      *d = o[k];
    }
  }
}
}  // namespace

extern "C" int sfh_maxpool2_bwd(const float* x, const float* dy, float* dx, int batch, int H, int W, int C,
                                int accumulate, void* stream) {
  SFH_REQUIRE(x && dy && dx && batch > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "maxpool2_bwd: bad argument");
  SFH_REQUIRE(accumulate || (H % 2 == 0 && W % 2 == 0),
              "maxpool2_bwd: odd sizes leave a border the kernel does not write; zero dx and pass accumulate=1");
  const int Ho = H / 2, Wo = W / 2;
  const long total4 = (long)batch * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     dy, H, W, C, Ho, Wo, total4, accumulate, dx);
  return sfh_check_launch("maxpool2_bwd_kernel");
}

namespace {
// ------------------------------------------------------------------ BatchNorm + ReLU + max-pool 2x2 of a skip tensor
// The encoder's skip tensors (DoubleConv outputs that feed both MaxPool2d(2) and an Up block, unet/unet_model.py) in
// training mode, split formats: one pass over the conv output z writes y = relu(bn(z)) AND maxpool2(y), both in the split
// format only.  The split is monotone and the maximum is taken on the fp32 values, so the pooled planes are bit for bit
// those of bn_apply -> maxpool2_fwd -> f32_to_h2, without the fp32 copy of y (4 B per element written, 4 read), the pooled
// fp32 tensor and its conversion pass.  One thread = a 2x2 window (cropped at odd borders: those pixels still get their y)
// x 8 channels; a wave = 64 consecutive windows of the flattened (B * ceil(H/2), ceil(W/2)) grid x one channel group.
template <int NP>
__global__ __launch_bounds__(256) void bn_apply_pool_s3_kernel(const float* __restrict__ z, const float* __restrict__ mi,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               int H, int W, int C, long ncols,
                                                               unsigned short* __restrict__ y_s3, unsigned short* __restrict__ p_s3,
                                                               unsigned* __restrict__ overflow) {
  // one thread = the two rows of a window row x ONE column x 8 channels; lanes run along x (every store of a wave is one
  // contiguous run), the horizontal half of the maximum comes from the neighbouring lane.  Columns are counted over a width
  // rounded up to even, so that lanes 2i / 2i + 1 always hold the two columns of one window.
  const int nb = C >> 5;
  const int cb = (int)(blockIdx.x % (unsigned)nb);
  const long chunk = (long)(blockIdx.x / (unsigned)nb);
  const int g = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int c0 = cb * 32 + g * 8;
  const BnChannels<8> bn = bn_load<8>(mi, gamma, beta, C, c0);
  const int qh = (H + 1) >> 1, Wp = (W + 1) & ~1, Ho = H >> 1, Wo = W >> 1;
  const long q = chunk * 64 + (threadIdx.x & 63);
  const unsigned qu = q < ncols ? (unsigned)q : 0u;
  const unsigned prow = qu / (unsigned)Wp;                 // b * qh + qy
  const int x = (int)(qu - prow * (unsigned)Wp);
  const unsigned b = prow / (unsigned)qh;
  const int qy = (int)(prow - b * (unsigned)qh);
  const bool live = q < ncols && x < W;
  float vr[2][8] = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
  unsigned over = 0u;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int yy = 2 * qy + k;
    if (!live || yy >= H) continue;
    const long row = (long)b * H + yy;
    const long o = (row * W + x) * C + c0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 zz = *reinterpret_cast<const f32x4*>(z + o + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) vr[k][4 * h + j] = sfh_relu(bn.y(4 * h + j, zz[j]));
    }
    tr_store_split<NP>(vr[k], y_s3, row, x, c0, W, C, over);
  }
  // the window's maximum with maxpool2_fwd's nesting, max(max(a, b), max(c, d)) over (row 0: a b, row 1: c d) - sfh_max_nan
  // picks its second argument on ties, so the nesting decides the sign of a zero; used on the even lane (a, c are its own)
  float m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float r0 = __shfl_xor(vr[0][j], 1, 64), r1 = __shfl_xor(vr[1][j], 1, 64);
    m[j] = sfh_max_nan(sfh_max_nan(vr[0][j], r0), sfh_max_nan(vr[1][j], r1));
  }
  if (live && !(x & 1) && qy < Ho && (x >> 1) < Wo) {
    tr_store_split<NP>(m, p_s3, (long)b * Ho + qy, x >> 1, c0, Wo, C, over);
  }
  tr_report<NP>(overflow, over);
}
}  // namespace

extern "C" int sfh_bn_apply_pool(const float* z, const float* mean_invstd, const float* gamma, const float* beta, int batch,
                                 int H, int W, int C, void* y_s3, void* pool_s3, int split_fmt, uint32_t* overflow,
                                 void* stream) {
  SFH_REQUIRE(z && mean_invstd && gamma && beta && y_s3 && pool_s3 && batch > 0 && H >= 2 && W >= 2 && C > 0 && C % 32 == 0,
              "bn_apply_pool: bad argument (C %% 32 == 0, H and W >= 2)");
  SFH_REQUIRE(split_fmt == SFH_FMT_S3 || split_fmt == SFH_FMT_H2, "bn_apply_pool: split_fmt=%d (S3 or H2)", split_fmt);
  const long nquads = (long)batch * ((H + 1) / 2) * ((W + 1) & ~1);   // (row pair, column) slots, width rounded up to even
  const long nblk = (nquads + 63) / 64 * (C / 32);
  SFH_REQUIRE(nblk < (1L << 31) && nquads < (1L << 31) - 64 && (long)batch * H * W < (1L << 31),
              "bn_apply_pool: tensor too large for one launch");
  SFH_LAUNCH_SPLIT(bn_apply_pool_s3_kernel, split_fmt, dim3((unsigned)nblk), stream, z, mean_invstd, gamma, beta, H, W, C,
                   nquads, (unsigned short*)y_s3, (unsigned short*)pool_s3, overflow);
  return sfh_check_launch("bn_apply_pool_s3_kernel");
}

namespace {
// Backward of the same pair, up to the BatchNorm sums: dx (B,H,W,C; the gradient y already has from its other consumer
// when accumulate != 0) += the max-pool routing of dp (first maximum of each window in scan order, as maxpool2_bwd; the
// window values y = relu(bn(z)) are recomputed from z (bn_math.h) instead of read), and, since dx is then
// the layer's total gradient, acc[0][c] += sum g, acc[1][c] += sum g * xhat with g = dx * (y > 0): what bn_bwd_reduce would
// find in a second pass over dx and z.  Mapping of the reductions above; one thread-iteration = a 2x2 window x 4 channels.
__global__ __launch_bounds__(256) void pool2_bwd_bn_reduce_kernel(const float* __restrict__ z, const float* __restrict__ mi,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ dp, int H, int W, int C,
                                                                  long nquads, int accumulate, float* __restrict__ dx,
                                                                  double* __restrict__ acc) {
  __shared__ double sh[256];
  const int qh = (H + 1) >> 1, qw = (W + 1) >> 1, Ho = H >> 1, Wo = W >> 1;
  for (int c0 = 0; c0 < C; c0 += 1024) {
    const int cq = min(1024, C - c0) >> 2;
    const int lanes = 256 / cq;
    const int cqi = threadIdx.x % cq, pl = threadIdx.x / cq;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pl < lanes) {
      const int cc = c0 + 4 * cqi;
      const BnChannels<4> bn = bn_load<4>(mi, gamma, beta, C, cc);
      for (long q = (long)blockIdx.x * lanes + pl; q < nquads; q += (long)gridDim.x * lanes) {
        const unsigned qrow = (unsigned)q / (unsigned)qw;
        const int qx = (int)((unsigned)q - qrow * (unsigned)qw);
        const unsigned b = qrow / (unsigned)qh;
        const int qy = (int)(qrow - b * (unsigned)qh);
        const bool window = qy < Ho && qx < Wo;
        const long base = (((long)b * H + 2 * qy) * W + 2 * qx) * C + cc;
        const long off[4] = {0, C, (long)W * C, (long)W * C + C};
        const bool valid[4] = {true, 2 * qx + 1 < W, 2 * qy + 1 < H, 2 * qx + 1 < W && 2 * qy + 1 < H};
        f32x4 yv[4], xh[4], t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          f32x4 zz = {0.f, 0.f, 0.f, 0.f};
          t[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (valid[k]) {
            zz = *reinterpret_cast<const f32x4*>(z + base + off[k]);
            if (accumulate) t[k] = *reinterpret_cast<const f32x4*>(dx + base + off[k]);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            yv[k][j] = bn.y(j, zz[j]);
            xh[k][j] = bn.xhat(j, zz[j]);
          }
        }
        if (window) {
          const f32x4 gq = *reinterpret_cast<const f32x4*>(dp + (((long)b * Ho + qy) * Wo + qx) * C + cc);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int best = 0;
            float bv = sfh_relu(yv[0][j]);
#pragma unroll
            for (int k = 1; k < 4; ++k) {
              const float v = sfh_relu(yv[k][j]);
              if (v > bv) { bv = v; best = k; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k][j] += (k == best) ? gq[j] : 0.f;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!valid[k]) continue;
          if (window || !accumulate) *reinterpret_cast<f32x4*>(dx + base + off[k]) = t[k];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float gj = bn_gate(yv[k][j], t[k][j]);
            s[j] += (double)gj;
            s[4 + j] += (double)gj * (double)xh[k][j];
          }
        }
      }
    }
    red_tail(s, pl < lanes, cq, sh, acc + c0, C);
  }
}
}  // namespace

extern "C" int sfh_pool2_bwd_bn_reduce(const float* z, const float* mean_invstd, const float* gamma, const float* beta,
                                       const float* dpool, int batch, int H, int W, int C, int accumulate, float* dx,
                                       double* acc, void* stream) {
  SFH_REQUIRE(z && mean_invstd && gamma && beta && dpool && dx && acc && batch > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0,
              "pool2_bwd_bn_reduce: bad argument");
  const long nquads = (long)batch * ((H + 1) / 2) * ((W + 1) / 2);
  SFH_REQUIRE(nquads < (1L << 31) && (long)batch * H * W < (1L << 31), "pool2_bwd_bn_reduce: tensor too large for one launch");
  const unsigned nb = (unsigned)det_red_blocks(nquads);
  hipLaunchKernelGGL(pool2_bwd_bn_reduce_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, z, mean_invstd, gamma, beta,
                     dpool, H, W, C, nquads, accumulate, dx, acc);
  return sfh_check_launch("pool2_bwd_bn_reduce_kernel");
}
