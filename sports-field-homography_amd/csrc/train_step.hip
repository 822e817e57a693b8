// train_step.hip - the kernels that open and close a training step: the losses with their gradients,
// clip_grad_value_ + the three optimizers, the multi-tensor copy and the gradient scale of the backward pass.
//
// Replaces train.py:181-224 + models/losses.py and train.py:88-92,234-237.
// (An accumulating entry, its _det sibling and its _det_bytes query: the rule stands above bn_stats_impl, train_bn.hip.)

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "common.h"
#include "det_core.h"   // the loss plans and det_add: the deterministic mode's slabs

namespace {
// ------------------------------------------------------------------ losses of the training step
// train.py:181-224 + models/losses.py in one pass over the pixels: segmentation CE (per-sample
// weighted), SmoothL1 between the bilinear warp and gt/nc (per-sample weighted), consistency CE against
// trunc(warp * nc).  Writes d loss / d logits (NCHW) and d loss / d warp, accumulates the three loss
// values in fp64.  loss[0] = seg, [1] = rec, [2] = consistency (already scaled by their lambdas).
struct LossArgs {
  const float* logits; const long* gt; const float* weight; const float* warp;
  int nc, HW; long npix; int batch;
  float l_seg, l_rec, l_cons;   // lambda (0 = loss disabled)
  int rec_mse;                  // 1: nn.MSELoss, 0: nn.SmoothL1Loss (train.py:113-118)
  int seg_focal, cons_focal;    // 1: kornia FocalLoss(alpha=1, gamma=2) instead of CE (train.py:101,126)
  float* dlogits; float* dwarp; double* loss;
};

// one classification loss term at a pixel: CE (lse - l[tgt]) or Kornia's focal loss with alpha 1, gamma 2
// (train.py:101,126): sum_k (onehot_k + 1e-6) * -(1 - q_k)^2 log q_k, q = softmax + 1e-8; adds coef * dL/dl to dl
template <int NC>
__device__ __forceinline__ float cls_loss(const float (&l)[NC], const float (&pr)[NC], float lse, int tgt, bool focal,
                                          float coef, float (&dl)[NC]) {
  if (!focal) {
    float lt = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (k == tgt) lt = l[k];
      dl[k] += coef * (pr[k] - (k == tgt ? 1.f : 0.f));
    }
    return lse - lt;
  }
  float dLdp[NC], dot = 0.f, loss = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float q = pr[k] + 1e-8f, t = (k == tgt ? 1.f : 0.f) + 1e-6f;
    const float om = 1.f - q, lg = logf(q);
    loss += t * (-om * om * lg);
    dLdp[k] = t * (2.f * om * lg - om * om / q);
    dot += dLdp[k] * pr[k];
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) dl[k] += coef * pr[k] * (dLdp[k] - dot);
  return loss;
}

template <int NC, bool DET = false>
__global__ __launch_bounds__(256) void train_losses_kernel(const LossArgs a) {
  __shared__ double sh[256];
  double s_seg = 0.0, s_rec = 0.0, s_cons = 0.0;
  const float inv = 1.0f / ((float)a.HW * (float)a.batch);
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < a.npix; p += (long)gridDim.x * 256) {
    const long b = p / a.HW, i = p - b * a.HW;
    float l[NC], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NC; ++k) { l[k] = a.logits[(b * NC + k) * a.HW + i]; mx = fmaxf(mx, l[k]); }
    float se = 0.f, pr[NC], dl[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) { pr[k] = expf(l[k] - mx); se += pr[k]; dl[k] = 0.f; }
    const float lse = logf(se) + mx, rs = 1.0f / se;
#pragma unroll
    for (int k = 0; k < NC; ++k) pr[k] *= rs;
    const int gt = (int)a.gt[p];
    const float wb = a.weight[b];
    const float wv = a.warp ? a.warp[p] : 0.f;
    const int tc = min(max((int)(wv * (float)NC), 0), NC - 1);   // (warp_mask * nc).to(long)
    if (a.l_seg != 0.f) s_seg += (double)(wb * cls_loss<NC>(l, pr, lse, gt, a.seg_focal != 0, a.l_seg * wb * inv, dl));
    if (a.l_cons != 0.f) s_cons += (double)cls_loss<NC>(l, pr, lse, tc, a.cons_focal != 0, a.l_cons * inv, dl);
#pragma unroll
    for (int k = 0; k < NC; ++k) a.dlogits[(b * NC + k) * a.HW + i] = dl[k];
    if (a.warp) {
      const float d = wv - (float)gt / (float)NC;
      const float ad = fabsf(d);
      if (a.rec_mse) {
        s_rec += (double)(wb * d * d);
        if (a.dwarp) a.dwarp[p] = a.l_rec * wb * inv * 2.f * d;
      } else {
        s_rec += (double)(wb * (ad < 1.f ? 0.5f * d * d : ad - 0.5f));
        if (a.dwarp) a.dwarp[p] = a.l_rec * wb * inv * (ad < 1.f ? d : (d > 0.f ? 1.f : -1.f));
      }
    }
  }
  double v[3] = {s_seg * a.l_seg, s_rec * a.l_rec, s_cons * a.l_cons};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __syncthreads();
    sh[threadIdx.x] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) det_add<DET>(&a.loss[DET ? det_slab_offset(blockIdx.x, 3) + k : k], sh[0] * (double)inv);
  }
}
}  // namespace

static int train_losses_impl(const float* logits_nchw, const int64_t* gt_mask, const float* weight, const float* warp_mask,
                             int nc, int batch, int H, int W, float lambda_seg, float lambda_rec, int rec_mse,
                             float lambda_cons, int focal_flags, float* dlogits_nchw, float* dwarp, double* loss3, bool det,
                             void* workspace, long long workspace_bytes, void* stream) {
  const char* who = det ? "train_losses_det" : "train_losses";
  const DetPlan p = det_losses_plan(batch, H, W);
  SFH_REQUIRE(logits_nchw && gt_mask && weight && dlogits_nchw && loss3 && p.ok, "%s: bad argument", who);
  SFH_REQUIRE(nc >= 2 && nc <= 8, "%s: nc=%d unsupported (2..8)", who, nc);
  SFH_REQUIRE(warp_mask || (lambda_rec == 0.f && lambda_cons == 0.f), "%s: rec/consistency need the warp mask", who);
  LossArgs a;
  a.logits = logits_nchw; a.gt = (const long*)gt_mask; a.weight = weight; a.warp = warp_mask;
  a.nc = nc; a.HW = H * W; a.npix = (long)batch * H * W; a.batch = batch;
  a.l_seg = lambda_seg; a.l_rec = lambda_rec; a.l_cons = lambda_cons; a.rec_mse = rec_mse;
  a.seg_focal = focal_flags & 1; a.cons_focal = (focal_flags >> 1) & 1;
  a.dlogits = dlogits_nchw; a.dwarp = dwarp; a.loss = loss3;
  const long nb = p.slabs;   // blocks
  if (det) {
    SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
    a.loss = (double*)workspace;
  }
#define SFH_TL(N)                                                                                                  \
  case N:                                                                                                          \
    if (det)                                                                                                       \
      hipLaunchKernelGGL((train_losses_kernel<N, true>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a); \
    else                                                                                                           \
      hipLaunchKernelGGL((train_losses_kernel<N>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);       \
    break;
  switch (nc) { SFH_TL(2) SFH_TL(3) SFH_TL(4) SFH_TL(5) SFH_TL(6) SFH_TL(7) SFH_TL(8) }
#undef SFH_TL
  if (int rc = sfh_check_launch(det ? "train_losses_kernel (deterministic)" : "train_losses_kernel")) return rc;
  return det ? sfh_det_reduce_f64((const double*)workspace, nb, 3, 3, 3, loss3, 3, stream) : SFH_OK;
}

extern "C" int sfh_train_losses(const float* logits_nchw, const int64_t* gt_mask, const float* weight,
                                const float* warp_mask, int nc, int batch, int H, int W, float lambda_seg,
                                float lambda_rec, int rec_mse, float lambda_cons, int focal_flags,
                                float* dlogits_nchw, float* dwarp, double* loss3, void* stream) {
  return train_losses_impl(logits_nchw, gt_mask, weight, warp_mask, nc, batch, H, W, lambda_seg, lambda_rec, rec_mse,
                           lambda_cons, focal_flags, dlogits_nchw, dwarp, loss3, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_train_losses_det_bytes(int batch, int H, int W) {
  return det_bytes(det_losses_plan(batch, H, W));
}

extern "C" int sfh_train_losses_det(const float* logits_nchw, const int64_t* gt_mask, const float* weight,
                                    const float* warp_mask, int nc, int batch, int H, int W, float lambda_seg,
                                    float lambda_rec, int rec_mse, float lambda_cons, int focal_flags, float* dlogits_nchw,
                                    float* dwarp, double* loss3, void* workspace, long long workspace_bytes, void* stream) {
  return train_losses_impl(logits_nchw, gt_mask, weight, warp_mask, nc, batch, H, W, lambda_seg, lambda_rec, rec_mse,
                           lambda_cons, focal_flags, dlogits_nchw, dwarp, loss3, true, workspace, workspace_bytes, stream);
}

namespace {
// models/losses.py:6-19 (reduction 'mean') and its gradient wrt the projected points; one thread per frame.
// DET: the 64 frames of a block (frames past the batch: zeros) are added in frame order and stored into the block's slab (one
// word).  The frame's body stands twice: shared through a device function, the default instantiation compiled to another
// instruction stream than the one it was.
template <bool DET = false>
__global__ void reproj_loss_kernel(const float* __restrict__ poi, const float* __restrict__ gt,
                                   const float* __restrict__ nonzeros, const float* __restrict__ num_nonzero,
                                   int batch, int npts, float lambda, float* __restrict__ dpoi, double* __restrict__ loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (DET) {
    __shared__ double sh[64];
    double term = 0.0;
    if (b < batch) {
      double s = 0.0;
      const float sc = lambda / (num_nonzero[b] * (float)batch);
      for (int n = 0; n < npts; ++n) {
        const long o = ((long)b * npts + n) * 2;
        const float dx = gt[o] - poi[o], dy = gt[o + 1] - poi[o + 1];
        const float dist = sqrtf(dx * dx + dy * dy);
        const float nz = nonzeros[(long)b * npts + n];
        s += (double)(dist * nz);
        const float g = dist > 0.f ? nz * sc / dist : 0.f;
        dpoi[o] = -g * dx;
        dpoi[o + 1] = -g * dy;
      }
      term = s * (double)sc;
    }
    sh[threadIdx.x] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int l = 0; l < 64; ++l) t += sh[l];
      loss[blockIdx.x] = t;
    }
    return;
  }
  if (b >= batch) return;
  double s = 0.0;
  const float sc = lambda / (num_nonzero[b] * (float)batch);
  for (int n = 0; n < npts; ++n) {
    const long o = ((long)b * npts + n) * 2;
    const float dx = gt[o] - poi[o], dy = gt[o + 1] - poi[o + 1];
    const float dist = sqrtf(dx * dx + dy * dy);
    const float nz = nonzeros[(long)b * npts + n];
    s += (double)(dist * nz);
    const float g = dist > 0.f ? nz * sc / dist : 0.f;   // torch propagates NaN at dist == 0; 0 here
    dpoi[o] = -g * dx;
    dpoi[o + 1] = -g * dy;
  }
  unsafeAtomicAdd(loss, s * (double)sc);
}
}  // namespace

static int reproj_loss_impl(const float* poi, const float* gt_poi, const float* nonzeros, const float* num_nonzero, int batch,
                            int npts, float lambda, float* dpoi, double* loss, bool det, void* ws, long long ws_bytes,
                            void* stream) {
  const char* who = det ? "reproj_loss_det" : "reproj_loss";
  const DetPlan p = det_reproj_plan(batch);
  SFH_REQUIRE(poi && gt_poi && nonzeros && num_nonzero && dpoi && loss && p.ok && npts > 0, "%s: bad argument", who);
  if (det) SFH_REQUIRE_WS(who, ws, ws_bytes, p);
  SFH_LAUNCH_DET(reproj_loss_kernel, det, dim3((unsigned)p.slabs), dim3(64), stream, poi, gt_poi, nonzeros, num_nonzero, batch,
                 npts, lambda, dpoi, det ? (double*)ws : loss);
  if (int rc = sfh_check_launch(det ? "reproj_loss_kernel (deterministic)" : "reproj_loss_kernel")) return rc;
  return det ? sfh_det_reduce_f64((const double*)ws, p.slabs, 1, 1, 1, loss, 1, stream) : SFH_OK;
}

extern "C" int sfh_reproj_loss(const float* poi, const float* gt_poi, const float* nonzeros,
                               const float* num_nonzero, int batch, int npts, float lambda, float* dpoi,
                               double* loss, void* stream) {
  return reproj_loss_impl(poi, gt_poi, nonzeros, num_nonzero, batch, npts, lambda, dpoi, loss, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_reproj_loss_det_bytes(int batch) { return det_bytes(det_reproj_plan(batch)); }

extern "C" int sfh_reproj_loss_det(const float* poi, const float* gt_poi, const float* nonzeros, const float* num_nonzero,
                                   int batch, int npts, float lambda, float* dpoi, double* loss, void* workspace,
                                   long long workspace_bytes, void* stream) {
  return reproj_loss_impl(poi, gt_poi, nonzeros, num_nonzero, batch, npts, lambda, dpoi, loss, true, workspace, workspace_bytes,
                          stream);
}

namespace {
// train.py:136-144,203-208: per_sample_weighted_criterion(MSELoss / SmoothL1Loss(reduction='none'), uv, gt_uv, weights) *
// lambda on (B,2,H,W) tensors.  models/losses.py:33-41 takes torch.mean(loss, dim=(1, 2)) - on a 4-D map that is the mean
// over CHANNEL and ROW, leaving (B, W) - and multiplies by the (B,) weights, which broadcasts along the LAST axis: the
// weight of column w is weights[w] (legal only for B == W) or weights[0] (B == 1).  Restated as written: `wcol` = 1 picks
// weights[w], 0 weights[0].  loss += lambda * mean_{b,w}(weight * mean_{c,h} l); duv = its gradient.
template <bool DET = false>
__global__ __launch_bounds__(256) void uv_loss_kernel(const float* __restrict__ uv, const float* __restrict__ gt,
                                                      const float* __restrict__ weight, int wcol, int C, int H, int W,
                                                      long total, float lambda, int mse, float* __restrict__ duv,
                                                      double* __restrict__ loss, float inv) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int w = (int)(p % W);
    const float wb = weight[wcol ? w : 0];
    const float d = uv[p] - gt[p];
    const float ad = fabsf(d);
    if (mse) {
      s += (double)(wb * d * d);
      duv[p] = lambda * wb * inv * 2.f * d;
    } else {
      s += (double)(wb * (ad < 1.f ? 0.5f * d * d : ad - 0.5f));
      duv[p] = lambda * wb * inv * (ad < 1.f ? d : (d > 0.f ? 1.f : -1.f));
    }
  }
  __syncthreads();
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) det_add<DET>(DET ? loss + blockIdx.x : loss, sh[0] * (double)lambda * (double)inv);
}
}  // namespace

static int uv_loss_impl(const float* uv, const float* gt_uv, const float* weight, int nweights, int batch, int C, int H, int W,
                        float lambda, int mse, float* duv, double* loss, bool det, void* workspace, long long workspace_bytes,
                        void* stream) {
  const char* who = det ? "uv_loss_det" : "uv_loss";
  const DetPlan p = det_uv_plan(batch, C, H, W);
  SFH_REQUIRE(uv && gt_uv && weight && duv && loss && p.ok, "%s: bad argument", who);
  SFH_REQUIRE(nweights == 1 || nweights == W,
              "%s: %d per-sample weights cannot be broadcast along the last axis of the (B, W) = (%d, %d) loss map "
              "(models/losses.py:38-39 multiplies torch.mean(loss, dim=(1, 2)) of a 4-D map by the weights)", who, nweights, batch, W);
  const long total = (long)batch * C * H * W;
  const int wcol = nweights == W && nweights != 1 ? 1 : 0;
  const float inv = 1.0f / ((float)batch * (float)C * (float)H * (float)W);
  if (det) SFH_REQUIRE_WS(who, workspace, workspace_bytes, p);
  SFH_LAUNCH_DET(uv_loss_kernel, det, dim3((unsigned)p.slabs), dim3(256), stream, uv, gt_uv, weight, wcol, C, H, W, total, lambda,
                 mse, duv, det ? (double*)workspace : loss, inv);
  if (int rc = sfh_check_launch(det ? "uv_loss_kernel (deterministic)" : "uv_loss_kernel")) return rc;
  return det ? sfh_det_reduce_f64((const double*)workspace, p.slabs, 1, 1, 1, loss, 1, stream) : SFH_OK;
}

extern "C" int sfh_uv_loss(const float* uv, const float* gt_uv, const float* weight, int nweights, int batch, int C, int H,
                           int W, float lambda, int mse, float* duv, double* loss, void* stream) {
  return uv_loss_impl(uv, gt_uv, weight, nweights, batch, C, H, W, lambda, mse, duv, loss, false, nullptr, 0, stream);
}

extern "C" int64_t sfh_uv_loss_det_bytes(int batch, int C, int H, int W) {
  return det_bytes(det_uv_plan(batch, C, H, W));
}

extern "C" int sfh_uv_loss_det(const float* uv, const float* gt_uv, const float* weight, int nweights, int batch, int C, int H,
                               int W, float lambda, int mse, float* duv, double* loss, void* workspace,
                               long long workspace_bytes, void* stream) {
  return uv_loss_impl(uv, gt_uv, weight, nweights, batch, C, H, W, lambda, mse, duv, loss, true, workspace, workspace_bytes, stream);
}

namespace {
// ------------------------------------------------------------------ clip_grad_value_ + RMSprop
// train.py:88,234-237: g = clamp(grad, -clip, clip); g += wd * p; sq = alpha*sq + (1-alpha)*g*g;
// buf = mu*buf + g / (sqrt(sq) + eps); p -= lr * buf   (torch.optim.RMSprop, centered=False).
// Multi-tensor: `table` holds per tensor {param, grad, square_avg, momentum_buf} pointers and `chunks`
// {tensor index, element offset, count}; one block per chunk.
struct OptTensor { float* p; const float* g; float* sq; float* buf; };
struct OptChunk { int tensor; int count; long offset; };

// clamp_ as clip_grad_value_ applies it: a NaN gradient stays NaN (both compares are false) and poisons the weight as it does
// in torch - fminf(fmaxf(g, -clip), clip) turned it into -clip; every other input, +-inf and -0 included, gives the same bits
__device__ __forceinline__ float opt_clip(float g, float clip) { return g < -clip ? -clip : (g > clip ? clip : g); }

__global__ __launch_bounds__(256) void rmsprop_kernel(const OptTensor* __restrict__ table, const OptChunk* __restrict__ chunks,
                                                      float lr, float alpha, float eps, float wd, float mu, float clip,
                                                      float gscale) {
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = table[c.tensor];
  for (int i = threadIdx.x; i < c.count; i += 256) {
    const long o = c.offset + i;
    float g = t.g[o] * gscale;   // 1/world: data-parallel mean of the all-reduced sum
    if (clip > 0.f) g = opt_clip(g, clip);
    const float p = t.p[o];
    g = g + wd * p;
    const float sq = alpha * t.sq[o] + (1.0f - alpha) * g * g;
    t.sq[o] = sq;
    const float avg = sqrtf(sq) + eps;
    float step = g / avg;
    if (mu > 0.f) {
      step = mu * t.buf[o] + step;
      t.buf[o] = step;
    }
    t.p[o] = p - lr * step;
  }
}
}  // namespace

extern "C" int sfh_rmsprop_step(const void* tensor_table, const void* chunk_table, int nchunks, float lr,
                                float alpha, float eps, float weight_decay, float momentum, float clip_value,
                                float grad_scale, void* stream) {
  SFH_REQUIRE(tensor_table && chunk_table && nchunks > 0, "rmsprop_step: bad argument");
  hipLaunchKernelGGL(rmsprop_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                     (const OptTensor*)tensor_table, (const OptChunk*)chunk_table, lr, alpha, eps, weight_decay,
                     momentum, clip_value, grad_scale);
  return sfh_check_launch("rmsprop_kernel");
}

namespace {
// train.py:90: torch.optim.SGD(lr, momentum, weight_decay) (dampening 0, no Nesterov) behind clip_grad_value_:
// g = clamp(grad); g += wd * p; buf = mu * buf + g (a zero-filled buffer gives torch's first step, buf = g); p -= lr * buf.
__global__ __launch_bounds__(256) void sgd_kernel(const OptTensor* __restrict__ table, const OptChunk* __restrict__ chunks,
                                                  float lr, float wd, float mu, float clip, float gscale) {
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = table[c.tensor];
  for (int i = threadIdx.x; i < c.count; i += 256) {
    const long o = c.offset + i;
    float g = t.g[o] * gscale;
    if (clip > 0.f) g = opt_clip(g, clip);
    const float p = t.p[o];
    g = g + wd * p;
    if (mu > 0.f) {
      g = mu * t.buf[o] + g;
      t.buf[o] = g;
    }
    t.p[o] = p - lr * g;
  }
}
}  // namespace

extern "C" int sfh_sgd_step(const void* tensor_table, const void* chunk_table, int nchunks, float lr, float weight_decay,
                            float momentum, float clip_value, float grad_scale, void* stream) {
  SFH_REQUIRE(tensor_table && chunk_table && nchunks > 0, "sgd_step: bad argument");
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const OptTensor*)tensor_table,
                     (const OptChunk*)chunk_table, lr, weight_decay, momentum, clip_value, grad_scale);
  return sfh_check_launch("sgd_kernel");
}

namespace {
// train.py:92: torch.optim.Adam(lr, betas, weight_decay) (L2 form, no amsgrad) behind clip_grad_value_, in torch's own
// operation order: m = lerp(m, g, 1 - b1); v = b2 * v + (1 - b2) * g * g; denom = sqrt(v) / sqrt(1 - b2^t) + eps;
// p -= (lr / (1 - b1^t)) * m / denom.  `buf` holds exp_avg, `sq` exp_avg_sq; the two bias corrections come from the host.
__global__ __launch_bounds__(256) void adam_kernel(const OptTensor* __restrict__ table, const OptChunk* __restrict__ chunks,
                                                   float step_size, float b1, float b2, float eps, float wd, float clip,
                                                   float gscale, float bias2_sqrt) {
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = table[c.tensor];
  for (int i = threadIdx.x; i < c.count; i += 256) {
    const long o = c.offset + i;
    float g = t.g[o] * gscale;
    if (clip > 0.f) g = opt_clip(g, clip);
    const float p = t.p[o];
    g = g + wd * p;
    float m = t.buf[o];
    m = m + (1.0f - b1) * (g - m);
    t.buf[o] = m;
    const float v = b2 * t.sq[o] + (1.0f - b2) * g * g;
    t.sq[o] = v;
    const float denom = sqrtf(v) / bias2_sqrt + eps;
    t.p[o] = p - step_size * (m / denom);
  }
}
}  // namespace

extern "C" int sfh_adam_step(const void* tensor_table, const void* chunk_table, int nchunks, float lr, float beta1, float beta2,
                             float eps, float weight_decay, float clip_value, float grad_scale, int step, void* stream) {
  SFH_REQUIRE(tensor_table && chunk_table && nchunks > 0 && step >= 1, "adam_step: bad argument (step counts from 1)");
  SFH_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam_step: betas must lie in [0, 1)");
  const double bias1 = 1.0 - pow((double)beta1, (double)step), bias2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const OptTensor*)tensor_table,
                     (const OptChunk*)chunk_table, (float)((double)lr / bias1), beta1, beta2, eps, weight_decay, clip_value,
                     grad_scale, (float)sqrt(bias2));
  return sfh_check_launch("adam_kernel");
}

namespace {
// ------------------------------------------------------------------ multi-tensor copy
// dst_t (contiguous) = src_t (up to 4-D, any strides) [* scale] for many tensors in ONE launch: the gradient assembly of a
// training step (182 tensors, the weight gradients as permuted views of the backward-filter buffers, times 1 / the
// power-of-two gradient scale) and the BatchNorm statistics snapshot (162 buffers) were one hipMemcpy each.
// 4-byte elements; SCALE = false moves the words untouched (integer buffers).
struct CopyTensor { void* dst; const void* src; int d1, d2, d3, pad; long s0, s1, s2, s3; };

template <bool SCALE>
__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyTensor* __restrict__ table, const OptChunk* __restrict__ chunks,
                                                         float scale, const float* __restrict__ scale_dev = nullptr) {
  if (SCALE && scale_dev) scale = *scale_dev;     // (the factor lives on the device: sfh_multi_copy_dscale)
  const OptChunk c = chunks[blockIdx.x];
  const CopyTensor t = table[c.tensor];
  const bool contiguous = t.s3 == 1 && t.s2 == t.d3 && t.s1 == (long)t.d2 * t.d3 && t.s0 == (long)t.d1 * t.d2 * t.d3;
  for (int i = threadIdx.x; i < c.count; i += 256) {
    const long o = c.offset + i;
    long so = o;
    if (!contiguous) {
      const long i3 = o % t.d3;
      long r = o / t.d3;
      const long i2 = r % t.d2;
      r /= t.d2;
      const long i1 = r % t.d1, i0 = r / t.d1;
      so = i0 * t.s0 + i1 * t.s1 + i2 * t.s2 + i3 * t.s3;
    }
    if (SCALE) reinterpret_cast<float*>(t.dst)[o] = reinterpret_cast<const float*>(t.src)[so] * scale;
    else reinterpret_cast<unsigned*>(t.dst)[o] = reinterpret_cast<const unsigned*>(t.src)[so];
  }
}
}  // namespace

extern "C" int sfh_multi_copy(const void* tensor_table, const void* chunk_table, int nchunks, float scale, void* stream) {
  SFH_REQUIRE(tensor_table && chunk_table && nchunks > 0, "multi_copy: bad argument");
  if (scale == 1.f)
    hipLaunchKernelGGL(multi_copy_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CopyTensor*)tensor_table, (const OptChunk*)chunk_table, 1.f);
  else
    hipLaunchKernelGGL(multi_copy_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CopyTensor*)tensor_table, (const OptChunk*)chunk_table, scale);
  return sfh_check_launch("multi_copy_kernel");
}

extern "C" int sfh_multi_copy_dscale(const void* tensor_table, const void* chunk_table, int nchunks, const float* scale_dev,
                                     void* stream) {
  SFH_REQUIRE(tensor_table && chunk_table && nchunks > 0 && scale_dev, "multi_copy_dscale: bad argument");
  hipLaunchKernelGGL(multi_copy_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                     (const CopyTensor*)tensor_table, (const OptChunk*)chunk_table, 1.f, scale_dev);
  return sfh_check_launch("multi_copy_kernel");
}

// The power-of-two scale a training step's backward pass is carried with in the two-plane fp16 format, chosen ON THE DEVICE from
// the largest head / theta gradient (words of sfh_multi_absminmax: nheads head tensors, then theta if has_theta) - what
// training.run_backward computed on the host behind a read-back until round 6.  Same rule: the largest head gradient goes to
// [2^(1+shift), 2^(2+shift)) (without heads: theta's to [2^(12+shift), 2^(13+shift))); if theta's gradient would then sit below
// 2^-16 the scale is raised until it does not, provided the head gradients stay below 2^6.  scale2 = {S, 1 / S}.  Raises bit 1
// of *overflow for a non-finite seed and bit 2 if no scale fits both (the caller reads the word at the end of the step).
__global__ void grad_scale_kernel(const uint32_t* __restrict__ words, int nheads, int has_theta, int shift,
                                  float* __restrict__ scale2, uint32_t* __restrict__ overflow) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float mh = 0.f, mt = 0.f;
  bool finite = true;
  for (int i = 0; i < nheads; ++i) {
    const uint32_t b = words[2 * i];
    finite &= b < 0x7F800000u;
    mh = fmaxf(mh, __uint_as_float(b));
  }
  if (has_theta) {
    const uint32_t b = words[2 * nheads];
    finite &= b < 0x7F800000u;
    mt = __uint_as_float(b);
  }
  float S = 1.f;
  if (!finite) {
    atomicOr(overflow, 2u);
  } else {
    const float m = nheads > 0 ? mh : mt;
    const int target = (nheads > 0 ? 2 : 13) + shift;
    int e = 0;
    if (m > 0.f) {
      (void)frexpf(m, &e);                    // m = f * 2^e, 0.5 <= f < 1  ->  m * S in [2^(target-1), 2^target)
      S = ldexpf(1.f, target - e);
    }
    if (nheads > 0 && mt > 0.f && mt * S < 1.52587890625e-05f) {
      (void)frexpf(mt, &e);
      const float S2 = ldexpf(1.f, -16 - e + 1);
      if (mh * S2 >= 64.f) atomicOr(overflow, 4u);
      else S = S2;
    }
  }
  scale2[0] = S;
  scale2[1] = 1.f / S;
}

extern "C" int sfh_grad_scale(const uint32_t* words, int nheads, int has_theta, int shift, float* scale2, uint32_t* overflow,
                              void* stream) {
  SFH_REQUIRE(words && scale2 && overflow && nheads >= 0 && (nheads > 0 || has_theta), "grad_scale: bad argument");
  hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, words, nheads, has_theta, shift, scale2,
                     overflow);
  return sfh_check_launch("grad_scale_kernel");
}
