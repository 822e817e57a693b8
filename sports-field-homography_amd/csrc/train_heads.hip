// train_heads.hip - what the backward pass of a training step runs besides BatchNorm and the backward-filter (SURVEY.md §8
// row f2): the two data movers, the OutConv backward and the ResNet-STN's max-pool, pooled head and stem backward-data.
//
// Replaces, for loss.backward() (train.py:233), the autograd backward of those layers.  Backward-data convolutions
// reuse sfh_conv_fwd with weights packed by sfh_pack_conv_weights mode 3 / 4; the data movers bring their operands into
// place.  All activations fp32 NHWC with channel stride == channel count.
// (An accumulating entry, its _det sibling and its _det_bytes query: the rule stands above bn_stats_impl, train_bn.hip.)

#include "common.h"
#include "bn_math.h"        // outconv_bwd_kernel<NC, true>
#include "det_core.h"       // split plans and det_add: the deterministic mode's slabs
#include "train_reduce.h"   // red_tail

namespace {
// ------------------------------------------------------------------ data movers
// dst (B,h,w,C) (+)= src[b, y+oy, x+ox, c_off : c_off+C] with src (B,Hs,Ws,cs); out-of-range -> 0
__global__ __launch_bounds__(256) void slice_add_kernel(const float* __restrict__ src, int Hs, int Ws, int cs, int c_off,
                                                        int oy, int ox, int h, int w, int C, long total4,
                                                        int accumulate, float* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int cq = C >> 2;
  const int q = (int)(i % cq);
  long r = i / cq;
  const int x = (int)(r % w); r /= w;
  const int y = (int)(r % h);
  const long b = r / h;
  const int sy = y + oy, sx = x + ox;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws)
    v = *reinterpret_cast<const f32x4*>(src + ((b * Hs + sy) * (long)Ws + sx) * cs + c_off + 4 * q);
  f32x4* d = reinterpret_cast<f32x4*>(dst) + i;
  if (accumulate) {
    f32x4 t = *d;
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] += v[j];
    *d = t;
  } else {
    *d = v;
  }
}
}  // namespace

extern "C" int sfh_slice_add(const float* src, int Hs, int Ws, int cs, int c_off, int oy, int ox, float* dst,
                             int batch, int h, int w, int C, int accumulate, void* stream) {
  SFH_REQUIRE(src && dst && batch > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && cs % 4 == 0 && c_off % 4 == 0 &&
                  c_off >= 0 && c_off + C <= cs && Hs > 0 && Ws > 0,
              "slice_add: bad argument");
  const long total4 = (long)batch * h * w * (C / 4);
  hipLaunchKernelGGL(slice_add_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                     Hs, Ws, cs, c_off, oy, ox, h, w, C, total4, accumulate, dst);
  return sfh_check_launch("slice_add_kernel");
}

namespace {
// dst (B,H,W,C): dst[2j,2i] = src[j,i] (src (B,ho,wo,C)), zero elsewhere
__global__ __launch_bounds__(256) void zero_stuff2_kernel(const float* __restrict__ src, int ho, int wo, int H, int W,
                                                          int C, long total4, float* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int cq = C >> 2;
  const int q = (int)(i % cq);
  long r = i / cq;
  const int x = (int)(r % W); r /= W;
  const int y = (int)(r % H);
  const long b = r / H;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!(y & 1) && !(x & 1) && (y >> 1) < ho && (x >> 1) < wo)
    v = *reinterpret_cast<const f32x4*>(src + ((b * ho + (y >> 1)) * (long)wo + (x >> 1)) * C + 4 * q);
  reinterpret_cast<f32x4*>(dst)[i] = v;
}
}  // namespace

extern "C" int sfh_zero_stuff2(const float* src, float* dst, int batch, int ho, int wo, int H, int W, int C,
                               void* stream) {
  SFH_REQUIRE(src && dst && batch > 0 && ho > 0 && wo > 0 && C > 0 && C % 4 == 0, "zero_stuff2: bad argument");
  SFH_REQUIRE(H >= 2 * ho - 1 && W >= 2 * wo - 1, "zero_stuff2: destination %dx%d too small for %dx%d", H, W, ho, wo);
  const long total4 = (long)batch * H * W * (C / 4);
  hipLaunchKernelGGL(zero_stuff2_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                     ho, wo, H, W, C, total4, dst);
  return sfh_check_launch("zero_stuff2_kernel");
}

namespace {
// ------------------------------------------------------------------ OutConv backward
// logits = w x + b (1x1, cin -> NC): dx[p][ci] = sum_k dl[k][p] w[k][ci];
// acc_w[k][ci] += sum_p dl[k][p] x[p][ci]; acc_b[k] += sum_p dl[k][p].   dl is NCHW, x / dx NHWC.
// BN (sfh_outconv_bwd_bn): x is not read - it is the BatchNorm + ReLU output of the layer in front, recomputed from that
// layer's conv output z (bn_math.h) - and, dx being that layer's whole gradient, the pass also leaves
// its backward sums [sum g | sum g * xhat], g = dx * (x > 0): sfh_bn_bwd_reduce's second pass over dx and z is not needed.
template <int NC, bool BN, bool DET = false>
__global__ __launch_bounds__(256) void outconv_bwd_kernel(const float* __restrict__ x, int cin,
                                                          const float* __restrict__ w, const float* __restrict__ dl,
                                                          long npix, int HW, float* __restrict__ dx,
                                                          double* __restrict__ acc_w, double* __restrict__ acc_b,
                                                          int pix_per_block, const float* __restrict__ bn_mi,
                                                          const float* __restrict__ bn_gamma, const float* __restrict__ bn_beta,
                                                          double* __restrict__ acc_bn) {
  __shared__ double sh[256];
  if constexpr (DET) {   // acc_w = the workspace: this block's slab is [NC][cin] weight sums, then [NC] bias sums
    acc_w += det_slab_offset(blockIdx.x, det_outconv_elems(NC, cin));
    acc_b = acc_w + (long)NC * cin;
  }
  const int cq = cin >> 2;  // <= 64
  const int lanes = 256 / cq;
  const int q = threadIdx.x % cq, pl = threadIdx.x / cq;
  f32x4 wk[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) wk[k] = *reinterpret_cast<const f32x4*>(w + k * cin + 4 * q);
  BnChannels<4> bn;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (BN) bn = bn_load<4>(bn_mi, bn_gamma, bn_beta, cin, 4 * q);
  // dW / db partial sums: fp32 over at most 64 pixels of a thread, then promoted into fp64 - a workgroup covers npix / 1024
  // pixels, so a thread's chain grows with the image (about 900 terms at 1280x720 x 16) and must not stay in fp32
  float sw[NC][4], sb[NC];
  double dsw[NC][4], dsb[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    sb[k] = 0.f;
    dsb[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sw[k][j] = 0.f;
      dsw[k][j] = 0.0;
    }
  }
  const long p0 = (long)blockIdx.x * pix_per_block, p1 = min(p0 + (long)pix_per_block, npix);
  int since_flush = 0;
  if (pl < lanes)
    for (long p = p0 + pl; p < p1; p += lanes) {
      if (++since_flush > 64) {
        since_flush = 1;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          dsb[k] += (double)sb[k];
          sb[k] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            dsw[k][j] += (double)sw[k][j];
            sw[k][j] = 0.f;
          }
        }
      }
      const long b = p / HW, i = p - b * HW;
      f32x4 xv = *reinterpret_cast<const f32x4*>(x + p * cin + 4 * q);
      f32x4 xh = {0.f, 0.f, 0.f, 0.f};
      if constexpr (BN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xh[j] = bn.xhat(j, xv[j]);
          xv[j] = sfh_relu(bn.y(j, xv[j]));
        }
      }
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const float g = dl[(b * NC + k) * HW + i];
        sb[k] += g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] += g * wk[k][j];
          sw[k][j] += g * xv[j];
        }
      }
      if (dx) *reinterpret_cast<f32x4*>(dx + p * cin + 4 * q) = o;
      if constexpr (BN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gj = bn_gate(xv[j], o[j]);
          s[j] += (double)gj;
          s[4 + j] += (double)gj * (double)xh[j];
        }
      }
    }
  if constexpr (BN) red_tail(s, pl < lanes, cq, sh, acc_bn, cin);
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    double tw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tw[j] = dsw[k][j] + (double)sw[k][j];
    red_tail<DET>(tw, pl < lanes, cq, sh, acc_w + k * cin, 0);
    __syncthreads();
    sh[threadIdx.x] = (pl < lanes) ? dsb[k] + (double)sb[k] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int l = 0; l < lanes; ++l) t += sh[l * cq];  // q == 0 lanes
      det_add<DET>(&acc_b[k], t);
    }
  }
}
}  // namespace

// acc_bn != nullptr: the BatchNorm-fused form (sfh_outconv_bwd_bn), which has no deterministic sibling
static int launch_outconv_bwd(const float* x, int cin, const float* w, const float* dlogits_nchw, int nc, int batch, int H,
                              int W, float* dx, double* acc_w, double* acc_b, const float* bn_mi, const float* bn_gamma,
                              const float* bn_beta, double* acc_bn, bool det, void* workspace, long long workspace_bytes,
                              void* stream) {
  const char* who = det ? "outconv_bwd_det" : "outconv_bwd";
  const DetPlan p = det_outconv_plan(cin, nc, batch, H, W);
  SFH_REQUIRE(x && w && dlogits_nchw && acc_w && acc_b && p.why != DET_BAD_FRAME, "%s: bad argument", who);
  SFH_REQUIRE(p.why != DET_BAD_CIN, "%s: cin=%d (multiple of 4, <= 256)", who, cin);
  SFH_REQUIRE(p.ok, "%s: nc=%d unsupported (1..8)", who, nc);
  SFH_REQUIRE(!(det && acc_bn), "%s: the BatchNorm-fused form has no deterministic mode", who);
  if (det) SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  const long npix = (long)batch * H * W;
  // every workgroup ends with nc * (cin + 1) fp64 atomics on the same addresses: about 1024 workgroups (at 640x360 x 16:
  // 3840 pixels each, 0.49 ms; 1024 pixels each = 3600 workgroups: 0.56 ms; 8192: 0.63 - profiles/r05_s2d_atomics.txt)
  const long ppb = det_outconv_ppb(npix);
  double* ws = (double*)workspace;   // the store pass finds both parts of its slab from the workspace's base
#define SFH_OB_LAUNCH(...)                                                                                              \
  hipLaunchKernelGGL((outconv_bwd_kernel<__VA_ARGS__>), dim3((unsigned)p.slabs), dim3(256), 0, (hipStream_t)stream, x, cin, \
                     w, dlogits_nchw, npix, H * W, dx, det ? ws : acc_w, det ? ws : acc_b, (int)ppb, bn_mi, bn_gamma,     \
                     bn_beta, acc_bn)
#define SFH_OB(N)                                 \
  case N:                                         \
    if (acc_bn) SFH_OB_LAUNCH(N, true);           \
    else if (!det) SFH_OB_LAUNCH(N, false);       \
    else SFH_OB_LAUNCH(N, false, true);           \
    break;
  switch (nc) { SFH_OB(1) SFH_OB(2) SFH_OB(3) SFH_OB(4) SFH_OB(5) SFH_OB(6) SFH_OB(7) SFH_OB(8) }
#undef SFH_OB
#undef SFH_OB_LAUNCH
  if (int rc = sfh_check_launch(det ? "outconv_bwd_kernel (deterministic)" : "outconv_bwd_kernel")) return rc;
  if (!det) return SFH_OK;
  if (int rc = sfh_det_reduce_f64(ws, p.slabs, p.elems, (long)nc * cin, nc * cin, acc_w, nc * cin, stream)) return rc;
  return sfh_det_reduce_f64(ws + (long)nc * cin, p.slabs, p.elems, nc, nc, acc_b, nc, stream);
}

extern "C" int sfh_outconv_bwd(const float* x, int cin, const float* w, const float* dlogits_nchw, int nc,
                               int batch, int H, int W, float* dx, double* acc_w, double* acc_b, void* stream) {
  return launch_outconv_bwd(x, cin, w, dlogits_nchw, nc, batch, H, W, dx, acc_w, acc_b, nullptr, nullptr, nullptr, nullptr, false,
                            nullptr, 0, stream);
}

extern "C" int64_t sfh_outconv_bwd_det_bytes(int cin, int nc, int batch, int H, int W) {
  return det_bytes(det_outconv_plan(cin, nc, batch, H, W));
}

extern "C" int sfh_outconv_bwd_det(const float* x, int cin, const float* w, const float* dlogits_nchw, int nc, int batch, int H,
                                   int W, float* dx, double* acc_w, double* acc_b, void* workspace, long long workspace_bytes,
                                   void* stream) {
  return launch_outconv_bwd(x, cin, w, dlogits_nchw, nc, batch, H, W, dx, acc_w, acc_b, nullptr, nullptr, nullptr, nullptr, true,
                            workspace, workspace_bytes, stream);
}

extern "C" int sfh_outconv_bwd_bn(const float* z, const float* mean_invstd, const float* gamma, const float* beta, int cin,
                                  const float* w, const float* dlogits_nchw, int nc, int batch, int H, int W, float* dx,
                                  double* acc_w, double* acc_b, double* acc_bn, void* stream) {
  SFH_REQUIRE(mean_invstd && gamma && beta && acc_bn && dx, "outconv_bwd_bn: null pointer");
  return launch_outconv_bwd(z, cin, w, dlogits_nchw, nc, batch, H, W, dx, acc_w, acc_b, mean_invstd, gamma, beta, acc_bn, false,
                            nullptr, 0, stream);
}

namespace {
// ------------------------------------------------------------------ ResNetSTN backward pieces
// MaxPool2d(3, stride 2, padding 1) backward: every input pixel looks at the (up to 4) windows that
// contain it and takes their gradient when it is the window's first maximum in scan order.
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               int H, int W, int C, int Ho, int Wo, long total4,
                                                               float* __restrict__ dx) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const int cq = C >> 2;
  const int q = (int)(idx % cq);
  long r = idx / cq;
  const int xi = (int)(r % W); r /= W;
  const int yi = (int)(r % H);
  const long b = r / H;
  const float* xb = x + b * (long)H * W * C + 4 * q;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  for (int yo = yi / 2; yo <= (yi + 1) / 2; ++yo) {   // windows with 2*yo-1 <= yi <= 2*yo+1
    if (yo >= Ho) continue;
    for (int xo = xi / 2; xo <= (xi + 1) / 2; ++xo) {
      if (xo >= Wo) continue;
      f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int by[4] = {-1, -1, -1, -1}, bx[4] = {-1, -1, -1, -1};
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = 2 * yo - 1 + ky;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = 2 * xo - 1 + kx;
          if (xx < 0 || xx >= W) continue;
          const f32x4 v = *reinterpret_cast<const f32x4*>(xb + ((long)yy * W + xx) * C);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (v[j] > best[j] || by[j] < 0) { best[j] = v[j]; by[j] = yy; bx[j] = xx; }
        }
      }
      const f32x4 d = *reinterpret_cast<const f32x4*>(dy + ((b * Ho + yo) * (long)Wo + xo) * C + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (by[j] == yi && bx[j] == xi) g[j] += d[j];
    }
  }
  reinterpret_cast<f32x4*>(dx)[idx] = g;
}
}  // namespace

extern "C" int sfh_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int batch, int H, int W, int C,
                                    void* stream) {
  SFH_REQUIRE(x && dy && dx && batch > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "maxpool3x3s2_bwd: bad argument");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const long total4 = (long)batch * H * W * (C / 4);
  hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, x, dy, H, W, C, Ho, Wo, total4, dx);
  return sfh_check_launch("maxpool3x3s2_bwd_kernel");
}

namespace {
// AdaptiveAvgPool2d(1) + Linear backward; one block per frame.
// dx[b,p,c] = (sum_j dout[b][j] w[j][c]) / HW;  acc_w[j][c] += dout[b][j] * mean_p x[b,p,c];  acc_b[j] += dout[b][j]
template <bool DET = false>
__global__ __launch_bounds__(256) void avgpool_linear_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ dout, int HW, int C, int nout,
                                                                 float* __restrict__ dx, double* __restrict__ acc_w,
                                                                 double* __restrict__ acc_b) {
  const int b = blockIdx.x;
  if constexpr (DET) {   // acc_w = the workspace: frame b's slab is [nout][C] weight terms, then [nout] bias terms
    acc_w += det_slab_offset(b, det_avgpool_elems(nout, C));
    acc_b = acc_w + (long)nout * C;
  }
  const float* xb = x + (long)b * HW * C;
  float* dxb = dx + (long)b * HW * C;
  const float inv = 1.0f / (float)HW;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += xb[(long)i * C + c];
    const float mean = s * inv;
    float df = 0.f;
    for (int j = 0; j < nout; ++j) {
      const float d = dout[b * nout + j];
      df += d * w[j * C + c];
      det_add<DET>(&acc_w[(long)j * C + c], (double)d * (double)mean);
    }
    df *= inv;
    for (int i = 0; i < HW; ++i) dxb[(long)i * C + c] = df;
  }
  if (threadIdx.x < nout) det_add<DET>(&acc_b[threadIdx.x], (double)dout[b * nout + threadIdx.x]);
}
}  // namespace

static int avgpool_linear_bwd_impl(const float* x, const float* w, const float* dout, int batch, int H, int W, int C, int nout,
                                   float* dx, double* acc_w, double* acc_b, bool det, void* workspace, long long workspace_bytes,
                                   void* stream) {
  const char* who = det ? "avgpool_linear_bwd_det" : "avgpool_linear_bwd";
  const DetPlan p = det_avgpool_plan(batch, C, nout);
  SFH_REQUIRE(x && w && dout && dx && acc_w && acc_b && p.ok && H > 0 && W > 0, "%s: bad argument", who);
  if (det) SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  double* ws = (double*)workspace;   // the store pass finds both parts of its slab from the workspace's base
  SFH_LAUNCH_DET(avgpool_linear_bwd_kernel, det, dim3((unsigned)p.slabs), dim3(256), stream, x, w, dout, H * W, C, nout, dx,
                 det ? ws : acc_w, det ? ws : acc_b);
  if (int rc = sfh_check_launch(det ? "avgpool_linear_bwd_kernel (deterministic)" : "avgpool_linear_bwd_kernel")) return rc;
  if (!det) return SFH_OK;
  if (int rc = sfh_det_reduce_f64(ws, p.slabs, p.elems, (long)nout * C, nout * C, acc_w, nout * C, stream)) return rc;
  return sfh_det_reduce_f64(ws + (long)nout * C, p.slabs, p.elems, nout, nout, acc_b, nout, stream);
}

extern "C" int sfh_avgpool_linear_bwd(const float* x, const float* w, const float* dout, int batch, int H, int W,
                                      int C, int nout, float* dx, double* acc_w, double* acc_b, void* stream) {
  return avgpool_linear_bwd_impl(x, w, dout, batch, H, W, C, nout, dx, acc_w, acc_b, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_avgpool_linear_bwd_det_bytes(int batch, int C, int nout) {
  return det_bytes(det_avgpool_plan(batch, C, nout));
}

extern "C" int sfh_avgpool_linear_bwd_det(const float* x, const float* w, const float* dout, int batch, int H, int W, int C,
                                          int nout, float* dx, double* acc_w, double* acc_b, void* workspace,
                                          long long workspace_bytes, void* stream) {
  return avgpool_linear_bwd_impl(x, w, dout, batch, H, W, C, nout, dx, acc_w, acc_b, true, workspace, workspace_bytes, stream);
}

namespace {
// Backward-data of the 7x7 stride-2 pad-3 stem (models/resnet.py:172) for the first `nc` input channels
// (the logits inside cat((logits, x), 1)): dlogits[b][c][y][x] += sum_{co,ky,kx} dz[b][Y][X][co] *
// w[co][c][ky][kx] with 2Y + ky - 3 = y, 2X + kx - 3 = x.  One thread per input pixel; the weights of
// the nc channels sit in LDS as [ky][kx][co][4].
template <int NC4>
__global__ __launch_bounds__(256) void stem_bwd_data_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                            int cin, int c_off, int nc, int H, int W, int Ho, int Wo,
                                                            float* __restrict__ dlogits, int batch) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [49][64][4*NC4]
  for (int i = threadIdx.x; i < 49 * 64 * 4 * NC4; i += 256) {
    const int c = i % (4 * NC4), co = (i / (4 * NC4)) % 64, t = i / (4 * NC4 * 64);
    wl[i] = c < nc ? w[((long)co * cin + c_off + c) * 49 + t] : 0.f;
  }
  __syncthreads();
  // a thread owns the pixels x and x + 64 of a row: same column parity, i.e. the same taps (ky, kx) and the same weights -
  // every 16-byte LDS read of a weight quad feeds two pixels (the kernel was bound by those reads: one per four FMAs).
  // (Round 4: FOUR pixels per thread measured slower, 1.28 -> 1.36 ms; waves of ONE column parity - wave-uniform tap loops,
  // broadcast weight reads - slower still, 1.23 -> 1.88 ms: with lane -> every second column each dz load instruction touches
  // 64 cache lines instead of 32; the kernel is bound by that gather, not by the LDS weight reads.)
  // Workgroups reach the 8 XCDs round-robin in launch order.  Round 6 (profiles/r06_tcc_train_per_launch.txt): with (x tile, 4-row
  // band, frame) = blockIdx the neighbouring bands - which gather the same dz rows - sat on different XCDs: 1.78 GB of L2 misses for
  // 0.3 GB of tensors.  XCD x now owns the contiguous range [x * chunk, (x + 1) * chunk) of the (frame, band, x tile) order.
  // (1-D launch of 8 * chunk workgroups; gx x gy x batch tiles)
  const int gx = (W + 127) >> 7, gy = (H + 3) >> 2;
  const long total = (long)gx * gy * batch;
  const long chunk = (total + 7) >> 3;
  const long own = (long)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
  if (own >= total) return;                                // (uniform per workgroup; the weights' barrier is behind us)
  const int bx = (int)(own % gx), by = (int)((own / gx) % gy);
  const int x = bx * 128 + (threadIdx.x & 63);
  const int y = by * 4 + (threadIdx.x >> 6);
  const int b = (int)(own / ((long)gx * gy));
  if (x >= W || y >= H) return;
  const bool two = x + 64 < W;
  float acc[2][4 * NC4];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int c = 0; c < 4 * NC4; ++c) acc[p][c] = 0.f;
  for (int ky = (y + 3) & 1; ky < 7; ky += 2) {
    const int Y = (y + 3 - ky) >> 1;
    if (Y < 0 || Y >= Ho) continue;
    for (int kx = (x + 3) & 1; kx < 7; kx += 2) {
      const int X0 = (x + 3 - kx) >> 1, X1 = X0 + 32;
      const bool ok0 = X0 >= 0 && X0 < Wo, ok1 = two && X1 >= 0 && X1 < Wo;
      if (!ok0 && !ok1) continue;
      const float* dp0 = dz + (((long)b * Ho + Y) * Wo + (ok0 ? X0 : 0)) * 64;
      const float* dp1 = dz + (((long)b * Ho + Y) * Wo + (ok1 ? X1 : 0)) * 64;
      const float* wp = wl + (ky * 7 + kx) * 64 * 4 * NC4;
#pragma unroll 4
      for (int co4 = 0; co4 < 16; ++co4) {
        f32x4 d0 = *reinterpret_cast<const f32x4*>(dp0 + 4 * co4), d1 = *reinterpret_cast<const f32x4*>(dp1 + 4 * co4);
        if (!ok0) d0 = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (!ok1) d1 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int q = 0; q < NC4; ++q) {
            const f32x4 ww = *reinterpret_cast<const f32x4*>(wp + ((4 * co4 + j) * NC4 + q) * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              acc[0][4 * q + c] += d0[j] * ww[c];
              acc[1][4 * q + c] += d1[j] * ww[c];
            }
          }
        }
      }
    }
  }
  for (int c = 0; c < nc; ++c) {
    dlogits[(((long)b * nc + c) * H + y) * W + x] += acc[0][c];
    if (two) dlogits[(((long)b * nc + c) * H + y) * W + x + 64] += acc[1][c];
  }
}
}  // namespace

extern "C" int sfh_stem_bwd_data(const float* dz, const float* w, int cin, int c_off, int nc, int batch, int H,
                                 int W, float* dlogits_nchw, void* stream) {
  SFH_REQUIRE(dz && w && dlogits_nchw && batch > 0 && batch <= 65535 && H > 0 && W > 0, "stem_bwd_data: bad argument");
  SFH_REQUIRE(nc >= 1 && nc <= 8 && c_off >= 0 && c_off + nc <= cin, "stem_bwd_data: c_off=%d nc=%d cin=%d", c_off, nc, cin);
  const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
  // 1-D launch: the kernel maps workgroup -> (frame, 4-row band, 128-column tile) so that an XCD owns a contiguous range
  const long total = (long)sfh_cdiv(W, 128) * sfh_cdiv(H, 4) * batch;
  SFH_REQUIRE(total < (1L << 28), "stem_bwd_data: grid too large");
  const dim3 grid((unsigned)(((total + 7) >> 3) << 3));
  if (nc <= 4) {
    hipLaunchKernelGGL(stem_bwd_data_kernel<1>, grid, dim3(256), 49 * 64 * 4 * sizeof(float), (hipStream_t)stream, dz, w,
                       cin, c_off, nc, H, W, Ho, Wo, dlogits_nchw, batch);
  } else {
    sfh_allow_big_lds(reinterpret_cast<const void*>(&stem_bwd_data_kernel<2>));
    hipLaunchKernelGGL(stem_bwd_data_kernel<2>, grid, dim3(256), 49 * 64 * 8 * sizeof(float), (hipStream_t)stream, dz, w,
                       cin, c_off, nc, H, W, Ho, Wo, dlogits_nchw, batch);
  }
  return sfh_check_launch("stem_bwd_data_kernel");
}
