// bn_math.h - the per-element arithmetic of training-mode BatchNorm, stated once.
//
// THE CONTRACT.  The training path stores neither the ReLU mask nor the normalised activation of a layer: every backward
// kernel reads them back out of the layer's conv output z.  That is sound only if each of them rounds y = xhat * gamma +
// beta, xhat = (z - mean) * invstd, exactly as the forward did - one fp32 rounding per operation, in this grouping, no
// contraction (build.py compiles every translation unit with -ffp-contract=off) - and gates with the strict y > 0.  So no
// kernel writes these expressions out; all of them call the functions below:
//   train_bn.hip     bn_apply_kernel, bn_bwd_reduce_kernel, bn_bwd_apply_kernel, bn_apply_s3_kernel, bn_bwd_apply_s3_kernel,
//                    bn_apply_pool_s3_kernel, pool2_bwd_bn_reduce_kernel
//   train_heads.hip  outconv_bwd_kernel<NC, true>
//   train_wgrad.hip  wgrad_c4_kernel<TH, TW, true>
//   conv_epilogue.h  the backward-sums branch of the conv epilogue
// tests/bn_math_host_main.cpp runs this file on the CPU against the fp32 / fp64 restatements of
// tests/test_train_kernel_host.py, bit for bit.
//
// Plain C++, no HIP header: SFH_BN_FN marks what the device runs too.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SFH_BN_FN __host__ __device__ __forceinline__
#else
#define SFH_BN_FN inline
#endif

// the forward's ReLU, with torch's NaN behaviour (relu(NaN) = NaN; v_max_f32 would return the other operand)
SFH_BN_FN float sfh_relu(float v) { return v < 0.f ? 0.f : v; }

SFH_BN_FN float bn_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
// the pre-activation (before a residual and the ReLU)
SFH_BN_FN float bn_y(float xhat, float gamma, float beta) { return xhat * gamma + beta; }
// the ReLU lets a gradient through where y > 0, strictly (y: the pre-activation or the activation - both are > 0 at the same
// elements), and g is the gradient behind it
SFH_BN_FN bool bn_relu_open(float y) { return y > 0.f; }
SFH_BN_FN float bn_gate(float y, float g) { return bn_relu_open(y) ? g : 0.f; }
// 1 / N and the two batch means of the backward, mg = sum g / N and mgx = sum g * xhat / N, from the fp64 sums
SFH_BN_FN float bn_inv_n(long npix) { return 1.0f / (float)npix; }
SFH_BN_FN float bn_mean_of(double sum, float inv_n) { return (float)sum * inv_n; }
SFH_BN_FN float bn_dz(float gamma, float invstd, float g, float mg, float xhat, float mgx) {
  return (gamma * invstd) * ((g - mg) - xhat * mgx);
}

// The per-channel terms of N consecutive channels.
template <int N>
struct BnChannels {
  float mean[N], invstd[N], gamma[N], beta[N], mg[N], mgx[N];
  SFH_BN_FN float xhat(int j, float z) const { return bn_xhat(z, mean[j], invstd[j]); }
  SFH_BN_FN float y(int j, float z) const { return bn_y(xhat(j, z), gamma[j], beta[j]); }
  SFH_BN_FN float dz(int j, float z, float g) const { return bn_dz(gamma[j], invstd[j], g, mg[j], xhat(j, z), mgx[j]); }
};

// Channels c .. c + N - 1 of a layer with C channels (mean_invstd = [mean | invstd]; channels past `last` read channel
// `last`).  BWD: with mg and mgx from acc = [sum g | sum g * xhat].  with_y == false: y() will not be called - beta, and
// outside BWD gamma, may be NULL and are not read.
template <int N, bool BWD = false>
SFH_BN_FN BnChannels<N> bn_load(const float* mean_invstd, const float* gamma, const float* beta, int C, int c,
                                bool with_y = true, const double* acc = nullptr, float inv_n = 0.f, int last = 0x7fffffff) {
  BnChannels<N> k;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < N; ++j) {
    const int i = c + j < last ? c + j : last;
    k.mean[j] = mean_invstd[i];
    k.invstd[j] = mean_invstd[C + i];
    k.gamma[j] = (BWD || with_y) ? gamma[i] : 1.f;
    k.beta[j] = with_y ? beta[i] : 0.f;
    k.mg[j] = BWD ? bn_mean_of(acc[i], inv_n) : 0.f;
    k.mgx[j] = BWD ? bn_mean_of(acc[C + i], inv_n) : 0.f;
  }
  return k;
}

// One channel's batch statistics from its fp64 sums s0 = sum z, s1 = sum z^2 over npix pixels: mean and invstd (variance
// E[z^2] - mean^2, clamped at 0) into mean_invstd[c], [C + c]; the running pair, where there is one, takes the unbiased
// variance (nn.BatchNorm2d).  Every operation in fp64, rounded to fp32 once at the store.
SFH_BN_FN void bn_finalize_channel(double s0, double s1, long npix, float eps, float momentum, int C, int c,
                                   float* mean_invstd, float* running_mean, float* running_var) {
  const double n = (double)npix;
  const double mean = s0 / n;
  double var = s1 / n - mean * mean;
  var = var > 0.0 ? var : 0.0;
  mean_invstd[c] = (float)mean;
  mean_invstd[C + c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = npix > 1 ? var * n / (n - 1.0) : var;
    running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
    running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
  }
}
