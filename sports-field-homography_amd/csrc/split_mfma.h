// split_mfma.h - what the split-operand kernels (conv_s3.hip, conv_small.hip, conv_upfused.hip, conv_inc_fused.hip,
// conv_c4h2.hip, stem.hip, wgrad_s3.hip) share on the device: the 16-byte vector types, the kept plane products and their
// order, the packed-weight strides and the split tensors' pixel offsets.  NP = planes per operand: 2 = H2 (fp16, "f16x3"),
// 3 = S3 (bf16, "bf16x6"); formats in include/sfh_amd.h, the arithmetic in conv_s3.hip's header.
#pragma once
#include "common.h"
#include "conv_geom.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The kept partial products of w * x, product k = plane PW[k] of the weights (first operand) x plane PX[k] of the
// activations (second operand):  H2  w0 x1 + w1 x0 + w0 x0;  S3  w0 x2 + w1 x1 + w2 x0 + w0 x1 + w1 x0 + w0 x0.
// Smallest first: the fp32 accumulator takes the low-order terms while it is still small, and every kernel adds them in
// THIS order per (stage, tap) - which is what the "bit-identical to sfh_conv_s3_fwd" promises of the other kernels rest on.
template <int NP>
struct SplitProducts {
  static_assert(NP == 2 || NP == 3, "two fp16 planes or three bf16 planes");
  static constexpr int N = NP == 3 ? 6 : 3;
  static constexpr int PW[6] = {0, 1, NP == 3 ? 2 : 0, 0, 1, 0};
  static constexpr int PX[6] = {NP == 3 ? 2 : 1, NP == 3 ? 1 : 0, 0, 1, 0, 0};
};

// one product: acc += w x on the 16-bit matrix core of the format (v_mfma_f32_16x16x32_bf16 / _f16); V: any 16-byte vector
template <int NP, class V>
__device__ __forceinline__ f32x4 split_mfma(const V& w, const V& x, const f32x4& acc) {
  if constexpr (NP == 3)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x), acc, 0, 0, 0);
}

// Packed weights (sfh_pack_h2_weights / sfh_pack_s3_weights), per 64 couts: [stage][tap][plane NP][cout group 4][lane 64]
// [8 x 16 bit] - byte strides
template <int NP>
struct SplitWeights {
  static constexpr unsigned GROUP = 1024u;         // one 16-cout group: 64 lanes x 16 bytes
  static constexpr unsigned PLANE = 4u * GROUP;
  static constexpr unsigned TAP = NP * PLANE;      // one (stage, tap)
};

// Split tensors are (B, H, cs/32, NP planes, 4 groups of 8 channels, W, 8) 16-bit values: every (plane, group) of an image
// row is a contiguous run of W x 16 bytes.  Byte offset of pixel x in run plg = plane * 4 + group of the FIRST 32-channel
// block of image row `row` = b * H + y (nblk = cs / 32 blocks; the next block is 4 * NP runs on).
template <int NP>
__device__ __forceinline__ unsigned split_pixel_offset(unsigned row, unsigned nblk, unsigned plg, unsigned W, unsigned x) {
  return ((row * (nblk * (4u * NP)) + plg) * W + x) * 16u;
}
// ... and of pixel (b, y, x) of a 16-bytes-per-pixel frame (fp32 NHWC with 4 stored channels, FH2)
__device__ __forceinline__ unsigned frame_pixel_offset(int b, int y, int x, int H, int W) {
  return (unsigned)((b * H + y) * W + x) * 16u;
}
