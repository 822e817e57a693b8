/*
 * sfh_amd.h - C ABI of libsfh_amd.so: the MI355X (gfx950) hot path of
 * darkAlert/sports-field-homography.
 *
 * The reference has no FFI layer: its operator boundary is the Python class
 * models.Reconstructor (models/reconstructor.py:30-247), which delegates every
 * device operation to ATen/cuDNN and Kornia.  Each entry point below replaces the
 * ATen/Kornia call(s) named in its comment (paths relative to the reference root).
 * The Python mirror of the class (sports-field-homography_amd/reconstructor.py)
 * binds these symbols with ctypes; INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - all pointers are DEVICE pointers (hipMalloc'd / torch CUDA tensors) unless named
 *    host_*; activations are fp32 NHWC ("channels last"), checkpoint tensors keep the
 *    reference layouts (OIHW conv weights, IOHW transposed-conv weights);
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*), allocates
 *    nothing, keeps no pointer and no global mutable state;
 *  - return value: 0 = success, negative = SFH_E_* (message via sfh_last_error()).
 */
#ifndef SFH_AMD_H
#define SFH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFH_OK 0
#define SFH_E_ARG (-1)     /* invalid argument / unsupported shape */
#define SFH_E_LAUNCH (-2)  /* HIP launch error */

/* Tile shapes of the implicit-GEMM conv kernel (output pixels per workgroup). */
#define SFH_TILE_8x32 0   /* 8 rows x 32 cols, MFMA pixel groups of 1x16 */
#define SFH_TILE_16x16 1  /* 16 rows x 16 cols, 1x16 groups              */
#define SFH_TILE_32x8 2   /* 32 rows x 8 cols, 2x8 groups (narrow maps)  */
#define SFH_TILE_8x16 3   /* 8 rows x 16 cols, 1x16 groups (split-bf16 kernel: small maps, stride 2) */
#define SFH_TILE_16x8 4   /* 16 rows x 8 cols, 2x8 groups  (split-bf16 kernel: small maps, stride 2) */

/* Tensor formats of conv sources / destinations.
 * F32: fp32 NHWC (B,H,W,cs).
 * S3 : "split-3" bf16 (B, H, cs/32, 3 planes, 4 groups, W, 8): v = plane0 + plane1 + plane2 exactly,
 *      plane0 = bf16(v), plane1 = bf16(v - plane0), plane2 = bf16(v - plane0 - plane1); channel c of
 *      pixel (y, x) lives in block c/32, group (c%32)/8, lane c%8 - each (block, plane, group) of an
 *      image row is W x 16 contiguous bytes.
 * H2 : "split-2" fp16 (B, H, cs/32, 2 planes, 4 groups, W, 8), the same layout with two planes:
 *      u = v * 2^e saturated to +-65504, plane0 = f16(u), plane1 = f16(u - plane0) (both RNE):
 *      22 significand bits of v while plane1 is a normal fp16 number (|u| >= 2^-3), an absolute error
 *      <= 2^-25 * 2^-e below that (fp16 subnormals are honoured by the conversions and by the MFMA).  The
 *      exponent e belongs to the TENSOR and is chosen by the caller (sfh_conv_desc.h2_exp_dst of the producer =
 *      h2_exp_src / h2_exp_res of its consumers); |v| must stay below 65504 * 2^-e: the producing kernel
 *      saturates, raises sfh_conv_desc.h2_overflow and records the largest |u| it saw in sfh_conv_desc.h2_range,
 *      from which the caller picks a smaller exponent.  The exponent trades range against the absolute error
 *      floor; end to end the result does not depend on it over a span of 2^6 (tests/probes/f16x3_error_probe.py).
 *      SFH_H2_ACT_EXP (2: |v| < 16376) is the conventional default - 4x the largest activation the synthetic
 *      ResNet-STN checkpoints of the tests produce - and what the training kernels use throughout. */
#define SFH_FMT_F32 0
#define SFH_FMT_S3 1
#define SFH_FMT_H2 2
#define SFH_FMT_FH2 3 /* the frame tensor of sfh_frame_to_h2 (16 bytes per pixel: two fp16 planes of channels 0..3); the only
                         source format sfh_conv3x3_c4h2_fwd takes, and only that entry takes it */
#define SFH_H2_ACT_EXP 2

/* Output modes of sfh_conv_fwd. */
#define SFH_OUT_NHWC 0        /* dst[b][y][x][co]                                        */
#define SFH_OUT_UPSCATTER2 1  /* transposed conv k2 s2: virtual cout = (dy*2+dx)*Cout+co; with ksize 2
                                 (sfh_conv_s3_fwd only): the 2x2 window of quadrant (dy,dx) starts at
                                 (y + dy - 1, x + dx - 1) - the composed ConvTranspose2d + conv3x3 of
                                 sfh_compose_up_weights */

typedef struct sfh_conv_desc {
  /* source 0: channels [0, c0) of the conv input; physical NHWC tensor (B, h0, w0, cs0). */
  const float* src0;
  int32_t c0, cs0, h0, w0;
  int32_t pool0;  /* 1: 2x2/stride-2 max-pool applied on load (h0 >= 2*H, w0 >= 2*W) */
  /* source 1 (optional, NULL if absent): channels [c0, c0+c1); physical (B, h1, w1, cs1),
   * placed at (pad_top1, pad_left1) inside the H x W input frame, zero elsewhere.       */
  const float* src1;
  int32_t c1, cs1, h1, w1, pad_top1, pad_left1;
  /* geometry */
  int32_t batch, H, W;  /* conv input frame */
  int32_t ksize;        /* 3 (pad 1), 1 (pad 0) or 4 (pad 2 before, 1 after; stem) */
  int32_t stride;       /* 1 or 2 */
  int32_t tile;         /* SFH_TILE_* */
  /* weights packed by sfh_pack_conv_weights for this (ksize, c0, c1); per-channel epilogue */
  const float* wpacked;
  const float* scale;  /* [cout_virtual] */
  const float* shift;  /* [cout_virtual] */
  int32_t cout;        /* virtual output channels, multiple of 64 */
  int32_t relu;
  /* optional residual added before ReLU: NHWC tensor with the geometry of dst */
  const float* residual;
  /* destination */
  float* dst;
  int32_t dst_cs;   /* channel stride (elements per pixel and plane) of dst */
  int32_t out_mode; /* SFH_OUT_* */
  /* formats (SFH_FMT_*): both sources share src_fmt; residual and dst_pool share dst_fmt */
  int32_t src_fmt, dst_fmt;
  /* optional second output: MaxPool2d(2) (floor) of dst, (B, Ho/2, Wo/2, pool_cs) */
  float* dst_pool;
  int32_t pool_cs;
  /* 1: `residual` is fp32 NHWC (channel stride dst_cs) even though dst is S3 (sfh_conv_s3_fwd) */
  int32_t residual_f32;
  /* optional [16][cout] shift table replacing `shift`, indexed by the border class of the OUTPUT pixel
   * (4*(row class) + (col class), see sfh_compose_up_weights): the up-sampling fusion below needs it */
  const float* shift_border;
  /* 2x2 up-scatter conv only: size of the destination frame when the up-sampled tensor is one row /
   * column short of it (F.pad in Up, unet/unet_parts.py:59-63, with diff 1: pad 0 before, 1 after);
   * 0 = 2*Ho x 2*Wo.  The conv frame (H, W) is then source rows/cols + 1, the extra source row reads 0. */
  int32_t up_dst_h, up_dst_w;
  /* 1: walk the pixel tiles from the last to the first (sfh_conv_s3_fwd).  Alternating the direction from
   * one layer to the next makes a layer start on the part of its input that the previous launch wrote
   * last, i.e. the part still resident in L2 / Infinity Cache. */
  int32_t reverse_tiles;
  /* OutConv fused behind the last 3x3 conv (sfh_conv_s3_fwd, cout == 64, plain output): with head_w set the
   * launch also computes logits = head_w (head_nc x 64) . y + head_b for its pixels and writes them NCHW to
   * head_logits (B,head_nc,H,W) and, if head_stn is set, cat((logits, frame)) zero-padded to cs channels to
   * head_stn (B,H,W,cs), cs = (head_nc + 3) rounded up to 4: 8 up to 5 classes, 12 for 6..8 (frame: head_frame, fp32
   * NHWC with 4 stored channels) - what sfh_outconv_fwd does in a second pass over y.  head_skip_dst != 0: y itself
   * is not stored. */
  const float* head_w;
  const float* head_b;
  int32_t head_nc, head_skip_dst;
  float* head_logits;
  float* head_stn;
  const float* head_frame;
  /* H2 destinations: device word that is OR-ed with 1 when a value had to be saturated to the fp16 range
   * (optional).  The caller zeroes it and reads it back after the last launch of a forward pass. */
  uint32_t* h2_overflow;
  /* Exponents of the H2 tensors of this launch (see SFH_FMT_H2; every H2 tensor stores v * 2^e):
   * h2_exp_src - both sources (folded by the CALLER into `scale` together with the weight exponent; the
   *              kernels that split an fp32 source themselves, sfh_stem7x7_fwd, read it);
   * h2_exp_dst - dst and dst_pool;  h2_exp_res - an H2 residual.  Range -64 .. 64. */
  int32_t h2_exp_src, h2_exp_dst, h2_exp_res;
  /* H2 destinations (optional): device word that receives, by atomic max, the largest bit pattern of
   * |v * 2^h2_exp_dst| this launch produced BEFORE saturation (bit patterns of non-negative floats order like
   * the floats; an Inf / NaN reads >= 0x7F800000).  > 0x477FE000 (65504.f) means the tensor was saturated; the
   * value tells the caller which exponent would have fitted.  Never reset by the library. */
  uint32_t* h2_range;
  /* sfh_conv_s3_fwd, H2 sources: couts per workgroup. 0 = chosen by the launcher, 64 = the 4-wave workgroup
   * (256 pixels x 64 couts, two per CU), 128 = the 8-wave workgroup (256 pixels x 128 couts, one per CU, two LDS
   * buffers; needs stride 1, ksize 3 or 2, cout % 128 == 0 - per quadrant for the up-scatter conv -, at least 128
   * input channels, no fused head).  Every other entry point (sfh_conv_small_fwd and sfh_conv_upfused_fwd included) ignores it. */
  int32_t wg_couts;
  /* kernels that split an fp32 source themselves (sfh_stem7x7_fwd): 0 or SFH_FMT_S3 = three bf16 planes, six products;
   * SFH_FMT_H2 = two fp16 planes, three products (weights from sfh_pack_stem_weights with the same format). */
  int32_t split_arith;
  /* split-K (sfh_conv_s3_fwd): ksplit > 1 launches ksplit copies of the grid; copy k accumulates its share of the
   * 32-channel stages of the K loop and writes acc * scale + shift as fp32 NHWC into slab k of dst, slabs
   * ksplit_stride BYTES apart - for layers whose (tile, cout block) grid alone leaves most of the chip idle (ResNet
   * layer3 / layer4 at batch 16).  Needs a single source, dst_fmt F32, no ReLU / residual / dst_pool / head; pass an
   * all-zero `shift` and let sfh_splitk_finish add the slabs, the real shift, the residual and the activation. */
  int32_t ksplit;
  int64_t ksplit_stride;
  /* sfh_conv_s3_fwd, 3x3 stride 1, plain output (optional): fp32 NHWC tensor (B, H, W, cout) the accumulators START from,
   * in accumulator units - i.e. a residual r enters as r / scale[c], which the caller arranges in the producer of that
   * tensor (the fused Up block: the composed 2x2 conv writes its partial divided by the skip-half conv's scale).  Loaded
   * in the prologue instead of sixteen dependent reads in the epilogue. */
  const float* acc_init;
  /* sfh_conv_s3_fwd, H2 sources, 3x3 or 1x1 stride 1, plain fp32 destination without ReLU / residual (the raw z = conv + bias of
   * a training-mode layer; optional): batch-statistics BatchNorm sums from the epilogue.  stats_partial = float64 table
   * [stats_rows][2][cout], zero before the launch; every wave ADDS (fp64 sums, fp64 atomics) the sums of z and of z * z
   * over its in-frame pixels into row (wave's tile slot) % stats_rows.  sfh_bn_stats_partials then adds the rows up
   * - the separate statistics pass over z (sfh_bn_stats) is not needed.  stats_rows: a power of two, 64 .. 65536. */
  double* stats_partial;
  int32_t stats_rows;
  /* backward mode of the same table (optional, with stats_partial): this launch is the backward-data conv whose fp32 output
   * dy is the ONLY gradient of a BatchNorm (+ReLU) layer; bwd_z = that layer's pre-BatchNorm tensor (fp32 NHWC, the shape of
   * dst, dst_cs == cout), bwd_mi = its mean | invstd (2 * cout floats), bwd_gamma / bwd_beta = its affine parameters (both
   * NULL: the layer has no ReLU).  The table then receives sum g and sum g * xhat with g = dy * (y > 0),
   * y = (z - mean) * invstd * gamma + beta exactly as sfh_bn_apply computes it: sfh_bn_bwd_reduce is not needed. */
  const float* bwd_z;
  const float* bwd_mi;
  const float* bwd_gamma;
  const float* bwd_beta;
  /* sfh_conv_upfused_fwd only: the packed weights (sfh_pack_h2_weights, ksize 2, 4 * cout virtual couts) and the 4 * cout
   * epilogue scales of the composed 2x2 conv of a fused Up block (its border-class shifts ride in shift_border). */
  const float* up_wpacked;
  const float* up_scale;
} sfh_conv_desc;

const char* sfh_last_error(void);
int sfh_version(void);

/* conv3x3+BN+ReLU, 1x1 conv, ConvTranspose2d k2 s2 - fp32 MFMA implicit GEMM.
 * Replaces nn.Conv2d/BatchNorm2d/ReLU of DoubleConv (unet/unet_parts.py:14-21), the
 * MaxPool2d of Down (unet/unet_parts.py:33, via pool0), F.pad + torch.cat of Up
 * (unet/unet_parts.py:59-67, via src1), nn.ConvTranspose2d of Up (unet/unet_parts.py:52),
 * and the conv/BN/ReLU/residual of BasicBlock (models/resnet.py:64-82).                  */
int sfh_conv_fwd(const sfh_conv_desc* d, void* stream);

/* fp32-accurate convolution on the bf16 matrix cores: sources in S3 format, weights packed by
 * sfh_pack_s3_weights, six bf16 MFMAs per 32 k (w0x2 + w1x1 + w2x0 + w0x1 + w1x0 + w0x0) with fp32
 * accumulation.  Same descriptor and epilogue as sfh_conv_fwd; ksize 1, 3 (stride 1 or 2) or 4 (stem),
 * c0/c1 multiples of 32, no pool0 (use the producer's dst_pool).  Replaces the same reference calls. */
int sfh_conv_s3_fwd(const sfh_conv_desc* d, void* stream);
int64_t sfh_packed_s3_weight_bytes(int ksize, int c0, int c1, int cout_virtual);
/* mode 0: OIHW conv weight; mode 1: IOHW ConvTranspose2d weight (ksize 1, cout_virtual = 4*cout);
 * mode 2: the 7x7 s2 stem as a 4x4 conv over the space-to-depth input (ksize 4, aux = real cin),
 * mode 3 / 4: backward-data of Conv2d / ConvTranspose2d; all as in sfh_pack_conv_weights. */
int sfh_pack_s3_weights(const float* w, void* packed, int ksize, int c0, int c1, int cout_virtual,
                        int mode, int aux, void* stream);
/* fp32 NHWC (rows = B*H, W, cs) <-> S3 (rows, cs/32, 3, 4, W, 8) conversion */
int sfh_f32_to_s3(const float* src, void* dst, int64_t rows, int W, int cs, void* stream);
int sfh_s3_to_f32(const void* src, float* dst, int64_t rows, int W, int cs, void* stream);

/* The same convolution with TWO fp16 planes per operand ("f16x3": sources in H2 format, src_fmt = SFH_FMT_H2 in
 * the descriptor of sfh_conv_s3_fwd): three fp16 MFMAs per 32 k (w0x1 + w1x0 + w0x0, fp32 accumulation) instead
 * of six bf16 ones.  Operands carry 22 significand bits; the dropped product is <= 2^-22 of the full one.  Measured
 * end to end (tests/probes/f16x3_error_probe.py) the representation error is below half of what the fp32
 * accumulation order already costs.  Weights are packed as planes of w * 2^wexp (wexp chosen by the caller so
 * that max |w| * 2^wexp lies in [2^13, 2^14)): the caller multiplies the layer's `scale` by 2^-(wexp +
 * h2_exp_src).  Modes and geometry as sfh_pack_s3_weights; packed size = 2/3 of the S3 size. */
int64_t sfh_packed_h2_weight_bytes(int ksize, int c0, int c1, int cout_virtual);
int sfh_pack_h2_weights(const float* w, void* packed, int ksize, int c0, int c1, int cout_virtual,
                        int mode, int aux, int wexp, void* stream);
/* fp32 NHWC (rows = B*H, W, cs) <-> H2 (rows, cs/32, 2, 4, W, 8) with the tensor's exponent act_exp (-64 .. 64);
 * overflow: optional device word, OR-ed with 1 when a value was saturated; range: optional device word, atomic
 * max of the bit patterns of |v * 2^act_exp| (as sfh_conv_desc.h2_range). */
int sfh_f32_to_h2(const float* src, void* dst, int64_t rows, int W, int cs, int act_exp, uint32_t* overflow,
                  uint32_t* range, void* stream);
int sfh_h2_to_f32(const void* src, float* dst, int64_t rows, int W, int cs, int act_exp, void* stream);

/* The same 3x3 stride-1 convolution on two-plane fp16 operands for launches whose grid of 256-pixel x 64-cout workgroups
 * leaves the chip under-filled (ResNet layer4 at batch 16, small batches): tiles of 12 x 20 pixels x 32 couts, halo and weight
 * fragments through LDS.  Same descriptor, same packed weights (sfh_pack_h2_weights), same accumulation order per output -
 * results are bit-identical to sfh_conv_s3_fwd's.  Restrictions: src_fmt H2, one source, ksize 3, stride 1, plain NHWC output
 * (H2 or fp32), optional residual of the destination's format + ReLU, no pooled output / head / acc_init / split-K / statistics. */
int sfh_conv_small_fwd(const sfh_conv_desc* d, void* stream);

/* The first conv of a fused Up block - conv3x3(cat([skip, ConvTranspose2d(x)])) + BatchNorm + ReLU, unet/unet_parts.py:52-68 - as ONE
 * launch (round 5 experiment; the two-launch form is sfh_conv_s3_fwd with ksize 2 / SFH_OUT_UPSCATTER2 writing an fp32 partial +
 * sfh_conv_s3_fwd with acc_init): src0 = the skip tensor (B,H,W,cs0) H2, src1 = the low-resolution x (B,h1,w1,cs1) H2 with
 * H in {2*h1, 2*h1+1}, W alike; wpacked / scale / shift / relu = the skip-half 3x3 conv's (c0 -> cout); up_wpacked / up_scale /
 * shift_border = the composed 2x2 conv's (c1 -> 4*cout virtual couts), scale and border shifts expressed in the skip-half's
 * accumulator units (what the two-launch form passes to its first launch); dst H2 (B,H,W,dst_cs).  Same products in the same
 * order per output as the two-launch form: bit-identical results.                                                        */
int sfh_conv_upfused_fwd(const sfh_conv_desc* d, void* stream);

/* First UNet layer (inc.double_conv.0, unet/unet_parts.py:15; 3 input channels stored as 4):
 * tap-packed fp32 MFMA kernel, k = channel, one MFMA k-step per tap.  Same descriptor/epilogue as
 * sfh_conv_fwd; wpacked from sfh_pack_c4_weights ((cout/64)*9*256 floats), w is OIHW (cout,cin<=4,3,3). */
int sfh_conv3x3_c4_fwd(const sfh_conv_desc* d, void* stream);
int sfh_pack_c4_weights(const float* w, float* packed, int cin, int cout, void* stream);

/* The same first layer on the fp16 matrix cores ("f16x3": two fp16 planes per operand, three products, fp32 accumulation;
 * unet/unet_parts.py:15).  The frame is split ONCE by sfh_frame_to_h2 into the FH2 frame tensor, 16 bytes per pixel =
 * [fp16 plane 0 of channels 0..3 | fp16 plane 1 of channels 0..3] of x * 2^act_exp (format as SFH_FMT_H2: saturating,
 * `range` receives the largest |x * 2^act_exp|, `overflow` is OR-ed with 1 on saturation; both optional; +-Inf saturate to
 * +-65504, a NaN becomes -65504 with plane 1 at +0, and `range` then reads the non-finite bit pattern, >= 0x7F800000); dst_nhwc4
 * (optional) receives the fp32 NHWC copy with 4 stored channels that sfh_nchw_to_nhwc would write.
 * sfh_conv3x3_c4h2_fwd: src0 = the FH2 tensor (B,H,W) x 16 bytes (src_fmt = SFH_FMT_FH2, c0 <= 4, cs0 = 4; a plain fp32 NHWC4
 * frame - src_fmt SFH_FMT_F32, the source of sfh_conv3x3_c4_fwd - is rejected), h2_exp_src = act_exp, wpacked from sfh_pack_c4h2_weights (planes of
 * w * 2^wexp; the caller multiplies `scale` by 2^-(wexp + act_exp)), dst H2 or fp32; descriptor fields as sfh_conv_fwd. */
int sfh_frame_to_h2(const float* src_nchw, float* dst_nhwc4, void* dst_fh2, int batch, int C, int H, int W, int act_exp,
                    uint32_t* overflow, uint32_t* range, void* stream);
int64_t sfh_packed_c4h2_weight_bytes(int cout);
int sfh_pack_c4h2_weights(const float* w, void* packed, int cin, int cout, int wexp, void* stream);
int sfh_conv3x3_c4h2_fwd(const sfh_conv_desc* d, void* stream);

/* The UNet's first DoubleConv in "f16x3" arithmetic - conv3x3(<= 4 -> 64) + BatchNorm + ReLU + conv3x3(64 -> 64) + BatchNorm +
 * ReLU, unet/unet_parts.py:14-21 - as ONE launch: the 64-channel intermediate is produced and consumed in LDS and never
 * written to memory.  inc0 = the descriptor sfh_conv3x3_c4h2_fwd would take for the first conv (FH2 frame source, cout 64,
 * dst_fmt H2; h2_exp_dst = the intermediate's exponent, h2_range / h2_overflow = the intermediate's words, which receive what
 * that launch would leave; dst is not used), inc3 = the descriptor sfh_conv_s3_fwd would take for the second conv (H2, ksize 3,
 * stride 1, c0 = cout = 64, tile SFH_TILE_8x32, h2_exp_src = inc0's h2_exp_dst, optional dst_pool, reverse_tiles; no second
 * source / residual / head / acc_init / split-K / statistics; src0 is not used).  Same products in the same order per output
 * element as the two launches: dst, dst_pool and all four range / overflow words are bit-identical. */
int sfh_conv_inc_fused_fwd(const sfh_conv_desc* inc0, const sfh_conv_desc* inc3, void* stream);

/* Number of floats of the packed weight buffer for a conv with the given geometry. */
int64_t sfh_packed_weight_floats(int ksize, int c0, int c1, int cout_virtual);

/* Re-layout checkpoint weights into MFMA fragment order.
 * mode = 0: w is OIHW (cout, c0+c1, k, k)  (nn.Conv2d), ksize 1 or 3
 * mode = 1: w is IOHW (cin, cout, 2, 2)    (nn.ConvTranspose2d), ksize must be 1 and
 *           cout_virtual = 4*cout.
 * mode = 2: w is OIHW (cout, aux, 7, 7), the stride-2 pad-3 stem of ResNetSTN
 *           (models/resnet.py:172), re-expressed as a 4x4 conv (pad 2 before / 1 after) over
 *           the 2x2 space-to-depth input produced by sfh_space_to_depth2; ksize = 4,
 *           c0 = 4 * (padded channels of the un-shuffled tensor), aux = real cin.
 * mode = 3: backward-data of a stride-1 Conv2d: w is OIHW (c0, aux, k, k); the packed conv maps dz
 *           (c0 = the layer's cout) to dx (cout_virtual >= aux = the layer's cin) with the taps
 *           flipped and in/out channels swapped.
 * mode = 4: backward-data of ConvTranspose2d k2 s2: w is IOHW (cout_virtual, aux, 2, 2); a 1x1 conv
 *           over sfh_space_to_depth2(dY) (c0 = 4*aux channels) producing dx.                      */
int sfh_pack_conv_weights(const float* w, float* packed, int ksize, int c0, int c1,
                          int cout_virtual, int mode, int aux, void* stream);

/* (B,H,W,cs) -> (B,ceil(H/2),ceil(W/2),4*cs): out[Y][X][(py*2+px)*cs + c] = in[2Y+py][2X+px][c], bit for bit
 * (+0.0 where 2Y+py >= H or 2X+px >= W: the odd row / column).  cs a multiple of 4. */
int sfh_space_to_depth2(const float* src, float* dst, int batch, int H, int W, int cs, void* stream);

/* scale = gamma / sqrt(var + eps); shift = (conv_bias - mean) * scale + beta
 * (eval-mode BatchNorm2d folded behind the conv; conv_bias may be NULL).
 * With gamma == NULL: scale = 1, shift = conv_bias (plain bias epilogue).
 * `repeat` replicates the n-vector (transposed conv: 4 sub-positions): element i < n * repeat holds channel i % n.
 * Evaluated as gamma * (1 / sqrtf(var + eps)) in fp32; with gamma == NULL scale is exactly 1 and shift exactly the bias
 * (+0.0 without one).                                                                       */
int sfh_fold_bn(const float* conv_bias, const float* gamma, const float* beta,
                const float* mean, const float* var, float eps, int n, int repeat,
                float* scale, float* shift, void* stream);

/* Decoded frames uint8 (B,H,W,C) -> float32 (B,C,H,W) = value/255: the dataset's preprocessing
 * (utils/dataset.py:154-159, :323-330: `img.transpose((2,0,1)) / 255` -> FloatTensor) on the GPU. */
int sfh_u8hwc_to_f32nchw(const uint8_t* src, float* dst, int batch, int C, int H, int W, void* stream);

/* Same with the video path's 2x downscale in front (utils/dataset.py:312-316: frames wider than the target
 * go through cv2.resize(..., INTER_AREA)): src uint8 (B,2H,2W,C) -> dst (B,C,H,W) = ((a+b+c+d+2)>>2)/255,
 * OpenCV's 2x2 area fast path.  Other scale factors are not covered. */
int sfh_u8hwc_area2_to_f32nchw(const uint8_t* src, float* dst, int batch, int C, int H, int W, void* stream);

/* Any integer downscale factor k = 2 .. 16 of the same call (1920x1080 -> 640x360 is k = 3): src uint8 (B,kH,kW,C) ->
 * dst (B,C,H,W).  k = 2 is the special case above; otherwise OpenCV's resizeAreaFast_ rule: the k x k block summed in int,
 * times the float 1.f / (k * k), rounded half to even, saturated to 0 .. 255, then / 255 (utils/dataset.py:312-330). */
int sfh_u8hwc_areak_to_f32nchw(const uint8_t* src, float* dst, int batch, int C, int H, int W, int k, void* stream);
/* Integer factors that differ per axis, or exceed 16 (kx horizontal, ky vertical, 1 .. 64 each): the same resizeAreaFast_ rule
 * with a kx x ky block - the block summed in int, times the float 1.f / (kx * ky), rounded half to even.  src (B,ky*H,kx*W,C). */
int sfh_u8hwc_areaxy_to_f32nchw(const uint8_t* src, float* dst, int batch, int C, int H, int W, int kx, int ky, void* stream);

/* The same call for ANY downscale (both factors >= 1, at least one not an integer: e.g. 1920x1080 -> 1024x576): OpenCV's
 * generic INTER_AREA path, resizeArea_ over the per-axis tables of computeResizeAreaTab (published imgproc/resize.cpp): every
 * destination pixel is sum_j beta_j * (sum_k alpha_k * S[sy_j][sx_k]) in float, products and sums individually rounded in
 * table order, then rounded half to even, saturated to 0 .. 255, / 255.
 * sfh_resize_area_tab (HOST code, no GPU): the table of one axis - for destination index d the entries ofs[d] .. ofs[d+1]-1 give
 * source index si[] and weight alpha[]; ofs has dsize + 1 ints, si / alpha room for `cap` entries (2 * dsize + ssize always
 * suffices); returns the number of entries, or -1 (bad sizes, dsize > ssize, cap too small).
 * sfh_u8hwc_area_to_f32nchw: src uint8 (B,Hs,Ws,C) -> dst float32 (B,C,Hd,Wd); the six table arrays are DEVICE pointers. */
int sfh_resize_area_tab(int ssize, int dsize, int32_t* ofs, int32_t* si, float* alpha, int cap);
int sfh_u8hwc_area_to_f32nchw(const uint8_t* src, float* dst, int batch, int C, int Hs, int Ws, int Hd, int Wd,
                              const int32_t* xofs, const int32_t* xsi, const float* xalpha, const int32_t* yofs,
                              const int32_t* ysi, const float* ybeta, void* stream);

/* (B, C, H, W) fp32 -> (B, H, W, cs) fp32; cs >= C, a multiple of 4.  Every value is moved bit for bit; the padding lanes
 * C .. cs-1 of every pixel are written as +0.0. */
int sfh_nchw_to_nhwc(const float* src, float* dst, int batch, int C, int H, int W, int cs,
                     void* stream);
/* (B, H, W, cs) -> (B, C, H, W), bit for bit; what the padding lanes C .. cs-1 hold does not enter the result. */
int sfh_nhwc_to_nchw(const float* src, float* dst, int batch, int C, int H, int W, int cs,
                     void* stream);

/* F.interpolate on NCHW planes (planes = B*C): mode 1 = 'bilinear' (align_corners as given; the input
 * resize of forward_unet, models/reconstructor.py:136, uses False), mode 0 = 'nearest' (the logits / uv
 * resize, models/reconstructor.py:153,156).
 * Index rules, decided in fp32 as ATen decides them:
 *   nearest:  source index min(floor(fl32(o * fl32(fl32(in) / fl32(out)))), in - 1) per axis - not floor(o * in / out): 26 -> 22
 *             reads source 12 at o = 11 where the exact quotient is 13.  A gather, bit for bit; align_corners is ignored.
 *   bilinear: src = o * fl32((in - 1) / (out - 1)) with align_corners (0 for out = 1), otherwise
 *             max(0, fl32(in / out) * (o + 0.5) - 0.5); i0 = min(trunc(src), in - 1), i1 = i0 + (i0 < in - 1), l = src - i0;
 *             value = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11), every operation rounded
 *             (no multiply-add contraction).  The fp32 src carries a few u * src, and the weights with it.
 * sfh_upsample2x_bilinear_nhwc is the bilinear rule with align_corners and out = 2 * in on NHWC; C a multiple of 4. */
int sfh_resize_nchw(const float* src, float* dst, int64_t planes, int hs, int ws, int hd, int wd, int mode,
                    int align_corners, void* stream);
/* nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) of the bilinear Up variant
 * (unet/unet_parts.py:49) on fp32 NHWC: (B,H,W,C) -> (B,2H,2W,C). */
int sfh_upsample2x_bilinear_nhwc(const float* src, float* dst, int batch, int H, int W, int C, void* stream);

/* OutConv (unet/unet_parts.py:74-77): 1x1 conv cin -> nc (nc <= 8) + bias.
 * x: NHWC (B,H,W,cin), w: (nc,cin,1,1), logits_nchw: (B,nc,H,W) or NULL.
 * Optional fused consumers:
 *   argmax_u8 (B,H,W): argmax over classes == preds_to_masks (utils/postprocess.py:7-18);
 *   stn_in  (B,H,W,stn_cs): [logits(nc), frame channels (3, read from frame_nhwc with
 *   stride frame_cs), zero padding] == torch.cat((logits, x), 1) of
 *   models/reconstructor.py:179,214 in NHWC.
 * cin a multiple of 8 (<= 1024); stn_cs a multiple of 4 with nc + 3 <= stn_cs <= 16, frame_cs >= 3.
 * stn_in lanes: the logits' own bits, then the frame's first three channels' bits, then +0.0 up to stn_cs; nothing beyond.
 * argmax rule: best = 0; for k = 1 .. nc-1: if logit[k] > logit[best] then best = k - on the fp32 logits the kernel stores.
 * A tie goes to the FIRST index.  Non-finite logits: a NaN never compares greater, so a NaN at class 0 stays the answer and
 * a NaN elsewhere is skipped; +inf wins like any large value.  This differs from the reference's argmax(softmax(.)), which
 * answers 0 for every pixel that holds a NaN or a +inf ([1, nan, 3, .5] and [1, 2, inf, 0]: 2 here, 0 there) and from it
 * only there and inside a top-2 margin of 1.2e-7.  The fused head epilogue and sfh_mask_format_fwd share this rule.      */
int sfh_outconv_fwd(const float* x, int cin, const float* w, const float* bias, int nc,
                    int batch, int H, int W, float* logits_nchw, uint8_t* argmax_u8,
                    float* stn_in, int stn_cs, const float* frame_nhwc, int frame_cs,
                    void* stream);

/* Homography warp of the court template == kornia HomographyWarper(h, w, mode,
 * normalized_coordinates=True)(template, theta) as called by Reconstructor.warp
 * (models/reconstructor.py:109-118), fused with the predict-mode epilogue
 * `* mask_classes` and `.type(int32)` (models/reconstructor.py:223,240).
 * theta: (B,3,3); tmpl: (.,1,ht,wt) with batch stride tmpl_bstride floats (0 = one shared
 * image); out_f32 (B,h,w) and/or out_i32 (B,h,w) = trunc(value * out_scale).
 * mode: 0 nearest, 1 bilinear.                                                            */
int sfh_homography_warp_fwd(const float* theta, const float* tmpl, int64_t tmpl_bstride,
                            int ht, int wt, int batch, int h, int w, int mode,
                            float out_scale, float* out_f32, int32_t* out_i32, void* stream);
/* Test hook (never on the product path): exhaustive GPU sweep of the two exact-division shortcuts of the
 * warp kernel against the IEEE divisions they replace - 1/z for every float with 2^-64 <= |z| <= 2^64, and
 * create_meshgrid's (i/(n-1) - 0.5)*2 for every 0 <= i < n <= 16385.  mismatches: DEVICE int64[2].        */
int sfh_selftest_warp_arith(int64_t* mismatches, void* stream);

/* transform_poi (models/reconstructor.py:120-130): inverse(theta) applied to the court
 * points, then p/2 + 0.5 if normalize.  theta (B,3,3), poi (B,N,2) -> out (B,N,2).        */
int sfh_poi_project_fwd(const float* theta, const float* poi, int batch, int npts,
                        int normalize, float* out, void* stream);

/* Consistency score (models/reconstructor.py:226-238): mean over pixels of
 * cross_entropy(logits[:, :, y, x], mask[y, x]).  logits NCHW (B,nc,H,W), mask int32
 * (B,hm,wm) (nearest-resized to HxW when sizes differ), partial: workspace of
 * sfh_ce_workspace_floats(batch, H, W) floats, score: (B).
 * Mask resize rule: F.interpolate(mode='nearest') in fp32 per axis, source row min(floor(fl32(y * fl32(hm / H))), hm - 1) and
 * the same with wm / W for the column (the nearest rule of sfh_resize_nchw).  One partial per 2048 pixels of a frame, summed
 * in a fixed order: a second launch gives the same bits.                                  */
int64_t sfh_ce_workspace_floats(int batch, int H, int W);
int sfh_consistency_ce_fwd(const float* logits, const int32_t* mask, int batch, int nc, int H,
                           int W, int hm, int wm, float* partial, float* score, void* stream);

/* The two calls above fused for predict()'s usual cases (nearest mode, 4, 7 or 8 classes; the logits (B,nc,hl,wl) have the warp's size,
 * or exactly half of it in both directions - predict.py's default geometry, where the reference scores through the nearest-
 * resized mask, i.e. logit pixel (y, x) against mask pixel (2y, 2x); models/reconstructor.py:223-240): out_i32 (B,h,w) = trunc(warp * out_scale) bit-identical to sfh_homography_warp_fwd, and
 * score (B) = mean over the pixels of cross_entropy(logits[:, :, y, x], out_i32[y, x]) - every wave scores the pixels it warps
 * while the class ids are still in registers, the logits (B,nc,h,w) are streamed once, the mask is never read back.  Two
 * launches (the fused kernel + a one-wave-per-frame sum of its partials in fp64, fixed order: deterministic) instead of three.
 * partial: workspace of sfh_warp_consistency_workspace_floats(batch, h, w) floats.  Other class counts / a mask of another
 * size: the two separate entries.                                                                                       */
int64_t sfh_warp_consistency_workspace_floats(int batch, int h, int w);
int sfh_warp_consistency_fwd(const float* theta, const float* tmpl, int64_t tmpl_bstride, int ht, int wt, int batch, int h,
                             int w, float out_scale, const float* logits, int nc, int hl, int wl, int32_t* out_i32,
                             float* partial, float* score, void* stream);

/* Output masks as predict.py writes them (predict.py:286-315; utils/postprocess.py:7-61):
 * src is int32 class ids (src_kind 0, e.g. predict()'s warp_mask), uint8 ids (1) or fp32 logits
 * NCHW (2: argmax over nc classes, first maximum wins); nearest resize (hs,ws)->(hd,wd) with
 * OpenCV's INTER_NEAREST index rule; mode 0 gray (ids), 1 bin ((id>0)*255), 2 rgb (palette:
 * HOST pointer to 8x3 bytes, colour of class k at palette[3k..3k+2]; out is (B,hd,wd,3)).   */
int sfh_mask_format_fwd(const void* src, int src_kind, int nc, int batch, int hs, int ws, int hd,
                        int wd, int mode, const uint8_t* palette, uint8_t* out, void* stream);

/* ResNetSTN pieces (models/resnet.py:235-254). */
/* MaxPool2d(kernel 3, stride 2, padding 1) on NHWC (B,H,W,C) -> (B,Ho,Wo,C), C a multiple of 4.  A selection, bit for bit;
 * a NaN anywhere in the window is the result (torch's rule), the padding never wins (a window of -inf gives -inf). */
int sfh_maxpool3x3s2_fwd(const float* x, float* y, int batch, int H, int W, int C, void* stream);
/* The same pooling written straight into a split tensor (dst_fmt SFH_FMT_H2 with exponent act_exp + the optional overflow /
 * range words of the format, or SFH_FMT_S3): what sfh_maxpool3x3s2_fwd followed by sfh_f32_to_h2 / sfh_f32_to_s3 gives, in
 * one pass.  C a multiple of 32. */
int sfh_maxpool3x3s2_split_fwd(const float* x, void* y, int batch, int H, int W, int C, int dst_fmt, int act_exp,
                               uint32_t* overflow, uint32_t* range, void* stream);
/* AdaptiveAvgPool2d(1) + flatten + Linear(C -> nout): x NHWC (B,H,W,C), w (nout,C), feat (B,C) = the
 * pooled features (workspace / second output), out (B,nout). */
int sfh_avgpool_linear_fwd(const float* x, const float* w, const float* bias, int batch, int H,
                           int W, int C, int nout, float* feat, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training mode (Reconstructor.forward under net.train() + loss.backward(), train.py:170,233).
 * Activations fp32 NHWC with channel stride == C; reductions over pixels accumulate in fp64 into
 * caller-zeroed `acc` buffers.
 * --------------------------------------------------------------------------------------------- */
/* nn.BatchNorm2d(training=True) (unet/unet_parts.py:16,19; models/resnet.py:174 etc.):
 * acc[0][c] += sum_p z[p][c], acc[1][c] += sum_p z[p][c]^2   (acc: 2*C doubles)                  */
int sfh_bn_stats(const float* z, int64_t npix, int C, double* acc, void* stream);
/* the same sums from the table a convolution's epilogue left (sfh_conv_desc.stats_partial: [rows][2][C] float64):
 * acc[0][c] += sum_r partial[r][0][c], acc[1][c] += sum_r partial[r][1][c].                                */
int sfh_bn_stats_partials(const double* partial, int rows, int C, double* acc, void* stream);
/* mean_invstd[0][c] = mean, [1][c] = 1/sqrt(biased var + eps); running stats (optional pair) updated
 * with `momentum` and the unbiased variance like torch.                                           */
int sfh_bn_finalize(const double* acc, int64_t npix, int C, float eps, float momentum, float* running_mean,
                    float* running_var, float* mean_invstd, int64_t* num_batches_tracked, void* stream);

/* sfh_bn_stats_partials + sfh_bn_finalize in one launch (round 6): `partial` = the (rows, 2, C) float64 table of per-wave sums of
 * z and z^2 that a conv epilogue left (sfh_conv_desc.stats_partial); summed in a fixed order (no atomics), then finished exactly
 * as sfh_bn_finalize does.                                                                                              */
int sfh_bn_finalize_partials(const double* partial, int rows, int64_t npix, int C, float eps, float momentum,
                             float* running_mean, float* running_var, float* mean_invstd, int64_t* num_batches_tracked,
                             void* stream);   /* num_batches_tracked
                    (optional): nn.BatchNorm2d's int64 step counter, incremented by one */
/* y = [relu]((z - mean) * invstd * gamma + beta [+ residual]); y_s3 (optional, C % 32 == 0, W = row
 * length of the (rows, W, C) tensor): the same values again in the split layout split_fmt (SFH_FMT_S3 or
 * SFH_FMT_H2; H2: `overflow` as in sfh_f32_to_h2) for the next convolution.  With y_s3, y may be NULL (only the
 * split copy is written: a layer whose consumers all read the split copy moves a third less). */
int sfh_bn_apply(const float* z, const float* mean_invstd, const float* gamma, const float* beta,
                 const float* residual, int relu, int64_t npix, int C, float* y, void* y_s3, int W,
                 int split_fmt, uint32_t* overflow, void* stream);
/* backward of bn_apply: with g = dy * (y > 0) (or dy when relu == 0; y == NULL with relu: the layer has no residual and
 * the sign of y is recomputed from z, gamma, beta - 8 instead of 12 bytes read per element), acc[0][c] += sum g,
 * acc[1][c] += sum g * xhat  (= dbeta, dgamma);  then
 * dz = gamma * invstd * (g - acc[0]/N - xhat * acc[1]/N), and dres = g (gradient of the residual
 * branch, optional).                                                                              */
int sfh_bn_bwd_reduce(const float* dy, const float* y, const float* z, const float* mean_invstd,
                      const float* gamma, const float* beta, int relu, int64_t npix, int C, double* acc, void* stream);
int sfh_bn_bwd_apply(const float* dy, const float* y, const float* z, const float* mean_invstd,
                     const float* gamma, const float* beta, const double* acc, int relu, int64_t npix, int C,
                     float* dz, float* dres, void* dz_s3, int W, int split_fmt, uint32_t* overflow, float* acc_f32,
                     void* stream);   /* dz_s3: optional split copy of dz (split_fmt, overflow: as sfh_bn_apply; with it dz may be NULL); acc_f32 (optional,
                                         2*C floats): acc as float32 = dbeta | dgamma for the caller */
/* acc[c] += sum_p x[p][c] over a channel slice of a (npix, cs) tensor: conv / transposed-conv bias
 * gradients.                                                                                       */
int sfh_colsum(const float* x, int64_t npix, int C, int cs, double* acc, void* stream);
/* First pass of nn.ConvTranspose2d(c, c/2, 2, stride=2).backward (unet/unet_parts.py:52, called from train.py:233):
 * du (B, 2h, 2w, cout) fp32 -> the space-to-depth tensor s (B, h, w, 4*cout), s[(py*2+px)*cout + co] at (y, x) =
 * du[2y+py][2x+px][co], written in the split format only (split_fmt SFH_FMT_S3 / SFH_FMT_H2 at the default exponent;
 * overflow as sfh_bn_apply), and the column sums of du (fp64, the bias gradient) - one pass instead of
 * sfh_colsum + sfh_space_to_depth2 + sfh_f32_to_h2.  acc = [acc_rows][cout] doubles, zeroed by the caller: a workgroup adds
 * its sums into row (its index) % acc_rows - same-address fp64 atomics are slow, 32 rows take them out of the way - and the
 * caller adds the rows up (sfh_bn_stats_partials with C = cout / 2; acc_rows = 1: acc is the result).  cout % 8 == 0.   */
int sfh_s2d_split_colsum(const float* du, int batch, int h, int w, int cout, void* s_split, int split_fmt,
                         double* acc, int acc_rows, uint32_t* overflow, void* stream);
/* nn.MaxPool2d(2) (unet/unet_parts.py:33) on NHWC, forward (floor) and backward: the gradient goes to
 * the first maximum of each window in scan order, like ATen; accumulate != 0 adds into dx.          */
int sfh_maxpool2_fwd(const float* x, float* y, int batch, int H, int W, int C, void* stream);
int sfh_maxpool2_bwd(const float* x, const float* dy, float* dx, int batch, int H, int W, int C,
                     int accumulate, void* stream);
/* The encoder's skip tensors in training mode (DoubleConv -> [MaxPool2d(2), Up], unet/unet_parts.py:16-20,33; split formats):
 * sfh_bn_apply_pool: y = relu(bn(z)) with the statistics in mean_invstd AND maxpool2(y) from one pass over z, both written in
 *   the split format only (y_s3: (B,H,W,C), pool_s3: (B,H/2,W/2,C); split_fmt / overflow as sfh_bn_apply) - bit for bit the
 *   planes of sfh_bn_apply -> sfh_maxpool2_fwd -> sfh_f32_to_h2.  C % 32 == 0.
 * sfh_pool2_bwd_bn_reduce: dx (+)= max-pool routing of dpool (window values recomputed from z; accumulate != 0: dx holds the
 *   gradient from y's other consumer) and, dx being the layer's total gradient then, acc (2*C doubles, zeroed by the caller)
 *   += [sum g | sum g * xhat], g = dx * (y > 0): sfh_maxpool2_bwd + sfh_bn_bwd_reduce in one pass.                       */
int sfh_bn_apply_pool(const float* z, const float* mean_invstd, const float* gamma, const float* beta, int batch, int H,
                      int W, int C, void* y_s3, void* pool_s3, int split_fmt, uint32_t* overflow, void* stream);
int sfh_pool2_bwd_bn_reduce(const float* z, const float* mean_invstd, const float* gamma, const float* beta,
                            const float* dpool, int batch, int H, int W, int C, int accumulate, float* dx, double* acc,
                            void* stream);
/* dst (B,h,w,C) (+)= src[b, y+oy, x+ox, c_off:c_off+C], src (B,Hs,Ws,cs), zero outside: the backward of
 * torch.cat / F.pad in Up (unet/unet_parts.py:59-67).                                              */
int sfh_slice_add(const float* src, int Hs, int Ws, int cs, int c_off, int oy, int ox, float* dst,
                  int batch, int h, int w, int C, int accumulate, void* stream);
/* dst (B,H,W,C): dst[2j][2i] = src[j][i], zero elsewhere - turns the backward of a stride-2 conv into
 * a stride-1 problem (models/resnet.py:56,172 stride-2 convs).                                     */
int sfh_zero_stuff2(const float* src, float* dst, int batch, int ho, int wo, int H, int W, int C,
                    void* stream);
/* Weight gradient of a stride-1 conv on the fp32 matrix cores (backward-filter):
 *   raw[m][tap][n_off + n] += sum_{b,y,x} dz[b][y][x][m] * xin[b][y + ky - pad][x + kx - pad][n]
 * dz (B,H,W,dz_cs) with M channels used; x (B,xh,xw,x_cs) with N channels, placed at (pad_top,pad_left)
 * inside the HxW conv input frame (second source of a concat), zero outside; ksize 1, 3 (pad 1) or
 * 4 (pad 2 before / 1 after: the space-to-depth stem, N <= 32); raw is (M, ksize^2, raw_n) fp32,
 * caller-zeroed, accumulated with atomics.                                                          */
int sfh_conv_wgrad(const float* dz, int dz_cs, int M, const float* x, int x_cs, int xh, int xw, int N,
                   int pad_top, int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n,
                   int n_off, void* stream);
/* The UNet's first layer (3 input channels stored as 4; unet/unet_parts.py:15-17) with its BatchNorm backward applied while
 * the gradient tiles are loaded: dy = gradient of the BatchNorm + ReLU output, z = the conv output, acc = the finished sums
 * [sum g | sum g * xhat] (sfh_bn_bwd_reduce, or the consumer's backward-data epilogue); raw as sfh_conv_wgrad (M, 9, raw_n).
 * Same values as sfh_bn_bwd_apply followed by sfh_conv_wgrad, without writing and re-reading dz.                        */
int sfh_conv_wgrad_c4_bn(const float* dy, const float* z, const float* mean_invstd, const float* gamma, const float* beta,
                         const double* acc, int M, const float* x, int N, int batch, int H, int W, float* raw, int raw_n,
                         void* stream);

/* The same weight gradient for 3x3 (pad 1) and 1x1 stride-1 convs on the 16-bit matrix cores, fp32-equivalent ("bf16x6",
 * six bf16 MFMA products per fp32 product, as sfh_conv_s3_fwd): dz and the layer input are S3 (split-bf16)
 * tensors - dz (B,H,M/32,3,4,W,8) with M a multiple of 64; x (B,xh,x_channels/32,3,4,xw,8) of which the
 * first N channels (multiple of 32) are used.  raw (M, ksize^2, raw_n) fp32, caller-zeroed, atomics.    */
int sfh_conv_wgrad_s3(const void* dz_s3, int M, const void* x_s3, int x_channels, int xh, int xw, int N,
                      int pad_top, int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n, int n_off,
                      int fmt, void* stream);   /* fmt: SFH_FMT_S3, or SFH_FMT_H2 (both tensors two-plane fp16, three
                                                   fp16 MFMA products per product) */

/* Grouped 3x3 convolution, padding 1, no bias: nn.Conv2d(C, C, 3, stride, 1, groups=G, bias=False) with C = G * cg, the
 * conv2 of the ResNeXt Bottleneck (models/resnet.py:108-112, groups = 32).  fp32 NHWC in and out, plain fp32 multiply-add
 * (one rounding per product and per add; csrc/conv_grouped.hip), group g owning channels [g*cg, (g+1)*cg) of both tensors.
 * Admitted: cg in {4, 8, 16, 32, 64}, stride 1 or 2, any groups >= 1; anything else returns SFH_E_ARG, nothing launched.
 *
 * sfh_pack_grouped_weights: w (G*cg, cg, 3, 3) OIHW -> packed (sfh_packed_grouped_weight_floats(G, cg) floats, -1 for a
 *   refused geometry).  mode 0: the forward layout; mode 1: the backward-data layout (inside each group output and input
 *   channel swapped, both taps flipped), with which sfh_conv_grouped_fwd at stride 1 maps dz -> dx.
 * sfh_conv_grouped_fwd: src (B,H,W,C) -> dst (B,Ho,Wo,C), Ho = (H-1)/stride + 1; scale / shift per channel, both NULL
 *   (dst = the raw accumulator) or both given: dst = [relu](acc * scale + shift), sfh_fold_bn's pair.  The terms of one
 *   output are added in one fixed order (csrc/conv_grouped_core.h): two calls give the same bits.  wpacked, dst, scale and
 *   shift 16-byte aligned.  A stride-2 backward-data goes through sfh_zero_stuff2 + the stride-1 call.
 * sfh_conv_grouped_wgrad: raw (C, 9, cg) fp32, raw[o][tap][c] += sum_p dz[p][o] * src[p*stride + tap - 1][g(o)*cg + c] over
 *   all B*Ho*Wo output pixels p; dz (B,Ho,Wo,C), src (B,H,W,C) read at its stride directly.  fp32 partial sums per
 *   workgroup tile, one fp32 atomic add per element and workgroup (their order is free, as in sfh_conv_wgrad).          */
int64_t sfh_packed_grouped_weight_floats(int groups, int cg);
int sfh_pack_grouped_weights(const float* w, float* packed, int groups, int cg, int mode, void* stream);
int sfh_conv_grouped_fwd(const float* src, const float* wpacked, const float* scale, const float* shift, int relu,
                         float* dst, int batch, int H, int W, int groups, int cg, int stride, void* stream);
int sfh_conv_grouped_wgrad(const float* dz, const float* src, float* raw, int batch, int H, int W, int groups, int cg,
                           int stride, void* stream);

/* Backward of OutConv (unet/unet_parts.py:74-77): dlogits NCHW (B,nc,H,W), x NHWC (B,H,W,cin);
 * dx NHWC (optional), acc_w (nc*cin doubles) += dW, acc_b (nc doubles) += db (caller-zeroed).        */
int sfh_outconv_bwd(const float* x, int cin, const float* w, const float* dlogits_nchw, int nc, int batch,
                    int H, int W, float* dx, double* acc_w, double* acc_b, void* stream);
/* The same pass when x is the BatchNorm + ReLU output of the layer in front and the head is its only consumer (up4.conv.3 ->
 * OutConv, unet/unet_model.py): x is recomputed from that layer's conv output z (mean_invstd, gamma, beta: sfh_bn_apply's
 * arithmetic, same bits) instead of read, and acc_bn (2 * cin doubles, zeroed by the caller) += [sum g | sum g * xhat] with
 * g = dx * (x > 0) - the layer's BatchNorm backward sums, without sfh_bn_bwd_reduce's pass over dx and z.                  */
int sfh_outconv_bwd_bn(const float* z, const float* mean_invstd, const float* gamma, const float* beta, int cin,
                       const float* w, const float* dlogits_nchw, int nc, int batch, int H, int W, float* dx,
                       double* acc_w, double* acc_b, double* acc_bn, void* stream);

/* ResNetSTN backward pieces (models/resnet.py:235-254).
 * MaxPool2d(3, stride 2, padding 1) on NHWC: dx (B,H,W,C) from dy (B,Ho,Wo,C), first maximum wins. */
int sfh_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int batch, int H, int W, int C,
                         void* stream);
/* AdaptiveAvgPool2d(1) + Linear: dx (B,H,W,C); acc_w (nout*C doubles) += dW, acc_b (nout) += db.     */
int sfh_avgpool_linear_bwd(const float* x, const float* w, const float* dout, int batch, int H, int W, int C,
                           int nout, float* dx, double* acc_w, double* acc_b, void* stream);
/* Backward-data of the 7x7 s2 p3 stem for input channels [c_off, c_off+nc), nc <= 8 - the logits
 * (or the uv map) inside torch.cat((logits, x[, uv]), 1) (models/reconstructor.py:174-183):
 * dlogits_nchw (B,nc,H,W) += ...; dz (B,Ho,Wo,64) NHWC, w OIHW (64,cin,7,7).                          */
int sfh_stem_bwd_data(const float* dz, const float* w, int cin, int c_off, int nc, int batch, int H, int W,
                      float* dlogits_nchw, void* stream);
/* d loss / d theta of the bilinear homography warp (sfh_homography_warp_fwd mode 1): acc (B*9 doubles,
 * caller-zeroed) += sum over pixels; dout (B,h,w).                                                   */
int sfh_homography_warp_bwd_theta(const float* theta, const float* tmpl, int64_t tmpl_bstride, int ht, int wt,
                                  int batch, int h, int w, const float* dout, double* acc, void* stream);
/* d loss / d theta of sfh_poi_project_fwd: dout (B,N,2) -> dtheta (B,9).                              */
int sfh_poi_project_bwd_theta(const float* theta, const float* poi, int batch, int npts, int normalize,
                              const float* dout, float* dtheta, void* stream);

/* Losses of the training step (train.py:181-224, models/losses.py:33-41) in one pass: segmentation
 * CE(logits, gt) and SmoothL1 (rec_mse = 0) or MSE (rec_mse = 1) of (warp, gt/nc), both averaged per frame, weighted by weight[b] and averaged
 * over the batch, and the consistency CE(logits, trunc(warp*nc)) averaged over all pixels; each times its
 * lambda (0 disables).  focal_flags bit 0 / bit 1: the segmentation / consistency term is
 * kornia.losses.FocalLoss(alpha=1, gamma=2) instead of CE (train.py:101,126; Kornia 0.5/0.6 formula:
 * sum_k (onehot_k + 1e-6) * -(1 - q_k)^2 log q_k with q = softmax + 1e-8).  gt_mask int64 (B,H,W); outputs d/dlogits (NCHW), d/dwarp (B,H,W, optional) and
 * loss3[0..2] += seg, rec, consistency (fp64, caller-zeroed).
 * The consistency target is clamp(trunc(fl32(warp * fl32(nc))), 0, nc - 1): the fp32 product is the reference's own
 * (warp_mask * nc).to(long); the clamp is this project's addition - torch raises at warp = 1 (and below 0), here such a pixel
 * takes class nc - 1 (0).  The reconstruction target is fl32(fl32(gt) / fl32(nc)); SmoothL1 branches on |d| < 1.           */
int sfh_train_losses(const float* logits_nchw, const int64_t* gt_mask, const float* weight,
                     const float* warp_mask, int nc, int batch, int H, int W, float lambda_seg,
                     float lambda_rec, int rec_mse, float lambda_cons, int focal_flags, float* dlogits_nchw,
                     float* dwarp, double* loss3, void* stream);
/* ReprojectionLoss (models/losses.py:6-31), reduction 'mean', times lambda: *loss += value; dpoi (B,N,2).
 * A point with dist == 0 gets the gradient 0, where torch propagates NaN (0 / 0 in the square root's backward). */
int sfh_reproj_loss(const float* poi, const float* gt_poi, const float* nonzeros, const float* num_nonzero,
                    int batch, int npts, float lambda, float* dpoi, double* loss, void* stream);
/* nn.utils.clip_grad_value_(clip) + torch.optim.RMSprop step (train.py:88,234-237) over many tensors in
 * one launch.  tensor_table: device array of {float* param; const float* grad; float* square_avg;
 * float* momentum_buf;}; chunk_table: device array of {int32 tensor; int32 count; int64 offset;}, one
 * workgroup per chunk.  clip_value <= 0 disables clipping, momentum == 0 skips the buffer; the gradient
 * is multiplied by grad_scale first (1/world after a data-parallel all-reduce sum, else 1).
 * The clip is clamp_ as clip_grad_value_ applies it, in all three optimizers: a NaN gradient stays NaN and poisons the weight
 * and the states it touches, as in torch; +-inf go to +-clip_value.
 * alpha (and Adam's beta1, beta2) as received; the complement 1 - alpha is formed in fp32 from that float and is exact; torch
 * rounds 1 - alpha_double to fp32 separately, a relative difference of the gain of at most 2^-24 / (1 - alpha) (the roundings of
 * alpha and of torch's complement, 2^-24 in all, seen from the complement): 10 ulps (9.3e-7) at alpha 0.99, 3 ulps (2.2e-7) at beta1 0.9, 111 ulps (1.29e-5) at
 * beta2 0.999.  tests/test_step_tail_host.py carries that difference through the recursion and states the distance to
 * torch.optim per element and state tensor.                                                             */
int sfh_rmsprop_step(const void* tensor_table, const void* chunk_table, int nchunks, float lr, float alpha,
                     float eps, float weight_decay, float momentum, float clip_value, float grad_scale,
                     void* stream);

/* The reference's other two optimizers (train.py:89-92) behind clip_grad_value_(clip), same tables as sfh_rmsprop_step:
 * sfh_sgd_step  = torch.optim.SGD(lr, momentum, weight_decay): buf (4th table pointer) = momentum buffer, zero-filled at first;
 * sfh_adam_step = torch.optim.Adam(lr, (beta1, beta2), eps, weight_decay): buf = exp_avg, sq (3rd pointer) = exp_avg_sq, both
 *                 zero-filled at first; `step` counts from 1 (bias corrections 1 - beta^step, evaluated in double on the host). */
int sfh_sgd_step(const void* tensor_table, const void* chunk_table, int nchunks, float lr, float weight_decay, float momentum,
                 float clip_value, float grad_scale, void* stream);
int sfh_adam_step(const void* tensor_table, const void* chunk_table, int nchunks, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float clip_value, float grad_scale, int step, void* stream);

/* UV-head loss (train.py:136-144,203-208): loss[0] += lambda * per_sample_weighted_criterion(MSELoss | SmoothL1Loss, uv, gt_uv,
 * weight) on (B,C,H,W) tensors and duv = its gradient.  models/losses.py:38-39 reduces a 4-D loss map with
 * torch.mean(loss, dim=(1, 2)) - over channel and row, leaving (B, W) - and multiplies by the weights, which broadcasts along
 * the LAST axis: nweights must be 1 (weight[0] everywhere; the B == 1 case) or W (column w takes weight[w]; the B == W case);
 * anything else is the reference's shape error and returns SFH_E_ARG.  mse: 1 = MSELoss, 0 = SmoothL1Loss(beta 1).          */
int sfh_uv_loss(const float* uv, const float* gt_uv, const float* weight, int nweights, int batch, int C, int H, int W,
                float lambda, int mse, float* duv, double* loss, void* stream);

/* Many small copies in one launch (training: the assembly of all parameter gradients into the flat gradient buffer -
 * weight gradients are permuted views of the backward-filter buffers - and the copy of the BatchNorm statistics a repeated
 * step starts from; torch issues one copy per tensor).  tensor_table: device array of {void* dst (contiguous); const
 * void* src; int32 d1, d2, d3, pad; int64 s0, s1, s2, s3} = logical shape (d0,d1,d2,d3) with the source's element strides,
 * 4-byte elements; chunk_table as sfh_rmsprop_step ({int32 tensor; int32 count; int64 offset}, one workgroup per chunk of
 * dst).  scale != 1: dst = src * scale (float32); scale == 1: the words are moved untouched.                     */
int sfh_multi_copy(const void* tensor_table, const void* chunk_table, int nchunks, float scale, void* stream);

/* sfh_multi_copy with the factor read from device memory (*scale_dev), float32 tensors.                                    */
int sfh_multi_copy_dscale(const void* tensor_table, const void* chunk_table, int nchunks, const float* scale_dev, void* stream);

/* The power-of-two scale of a training step's backward pass (two-plane fp16 gradients), chosen on the device: words = the output
 * of sfh_multi_absminmax over the nheads head-gradient tensors followed by the theta gradient (if has_theta); the largest head
 * gradient goes to [2^(1+shift), 2^(2+shift)) (no heads: theta's to [2^(12+shift), 2^(13+shift))), raised if theta's gradient
 * would sit below 2^-16 while the heads stay below 2^6.  scale2[0] = S, scale2[1] = 1 / S.  *overflow |= 2 for a non-finite
 * seed, |= 4 if no scale fits both (train.py:233: loss.backward() has no such limit - the caller then repeats the step with
 * three-plane bf16 operands).  No host read-back: the following launches take S through the pointer.                      */
int sfh_grad_scale(const uint32_t* words, int nheads, int has_theta, int shift, float* scale2, uint32_t* overflow, void* stream);

/* Backward of sfh_upsample2x_bilinear_nhwc (the bilinear Up variant, unet/unet_parts.py:49): dy (B,2H,2W,C)
 * -> dx (B,H,W,C).                                                                                        */
int sfh_upsample2x_bilinear_nhwc_bwd(const float* dy, float* dx, int batch, int H, int W, int C, void* stream);
/* Backward of sfh_resize_nchw mode 0 ('nearest': the logits / uv resize, models/reconstructor.py:153,156):
 * dy (planes,hd,wd) -> dx (planes,hs,ws).                                                                */
int sfh_resize_nearest_nchw_bwd(const float* dy, float* dx, int64_t planes, int hs, int ws, int hd, int wd,
                                void* stream);

/* Up block fusion (unet/unet_parts.py:52,59-67 + the first conv of DoubleConv): the u-half of
 *   conv3x3(cat([skip, ConvTranspose2d(x)]))  =  a 2x2 conv over the LOW-resolution x per output parity.
 * wconv OIHW (cout, c0+c1, 3, 3), wt IOHW (cx, c1, 2, 2), bt (c1); scale4 / shift4 (4*cout) = the folded
 * BatchNorm epilogue of the conv repeated per quadrant:
 *   w2 (4*cout, cx, 2, 2): virtual cout (py*2+px)*cout + co, tap (a,b) reads x[Y + py - 1 + a][X + px - 1 + b];
 *   shift_border (16, 4*cout): shift4 + scale4 * (what the transposed conv's bias contributes through the conv
 *   taps that fall inside the up-sampled tensor), per class of the output pixel: 4*(row class) + (col class),
 *   class 0: first row/col of the up-sampled tensor, 2: its last, 3: the padded row/col after it (F.pad with
 *   diff 1), 1: everything else (sfh_conv_desc.shift_border).                                             */
int sfh_compose_up_weights(const float* wconv, int cout, int c0, int c1, const float* wt, int cx,
                           const float* bt, const float* scale4, const float* shift4, float* w2,
                           float* shift_border, void* stream);

/* Second half of a split-K convolution (sfh_conv_desc.ksplit): y = [relu](sum_k slab_k + shift[c] [+ residual]) over
 * (npix, C) fp32 NHWC slabs slab_stride bytes apart -> dst in dst_fmt (F32 NHWC, S3 or H2 with exponent exp_dst; W =
 * row length of the split layouts).  residual (optional): same geometry, res_fmt / exp_res.  overflow / range: as
 * sfh_f32_to_h2.  Replaces the BatchNorm shift + residual add + ReLU of BasicBlock (models/resnet.py:74-80) that
 * sfh_conv_s3_fwd applies in its epilogue when the K loop is not split. */
int sfh_splitk_finish(const float* slabs, int nslabs, int64_t slab_stride, const float* shift, const void* residual,
                      int res_fmt, int exp_res, int relu, int64_t rows, int W, int C, void* dst, int dst_fmt,
                      int exp_dst, uint32_t* overflow, uint32_t* range, void* stream);

/* The ResNetSTN stem (models/resnet.py:172,241-243: 7x7 stride-2 pad-3 conv + BatchNorm + ReLU, <= 8 input
 * channels -> 64) with the split-bf16 arithmetic, K packed by tap (4 taps x 8 channels per MFMA): d->src0 fp32
 * NHWC (B,H,W,8) = cat((logits, frame)) zero-padded, d->wpacked from sfh_pack_stem_weights (w OIHW
 * (64,cin,7,7)), d->dst fp32 NHWC (B,Ho,Wo,64), scale/shift/relu as in sfh_conv_fwd; the other descriptor
 * fields must describe a plain single-source launch.                                                    */
int sfh_stem7x7_fwd(const sfh_conv_desc* d, void* stream);
int64_t sfh_packed_stem_weight_bytes(void);
int sfh_pack_stem_weights(const float* w, void* packed, int cin, int fmt, int wexp, void* stream);   /* fmt: SFH_FMT_S3, or
    SFH_FMT_H2 (planes of w * 2^wexp; the caller folds 2^-(wexp + h2_exp_src) into the layer's scale) */
/* 9..16 input channels (6..8 mask classes + frame, img+mask+uv): the same entry with d->cs0 = 12 or 16 stored channels
 * (d->c0 <= d->cs0, stored channels >= c0 zero) runs the 16-channel instance - 2 taps x 16 channels per MFMA, 25 k-steps - on
 * weights packed by sfh_pack_stem16_weights (cin <= 16, otherwise as sfh_pack_stem_weights) into
 * sfh_packed_stem16_weight_bytes() bytes.  Any other cs0, or c0 > cs0, is refused before anything is launched. */
int64_t sfh_packed_stem16_weight_bytes(void);
int sfh_pack_stem16_weights(const float* w, void* packed, int cin, int fmt, int wexp, void* stream);

/* Device calibration probe (bench.py `device_calibration`; not on the hot path): `workgroups` x 4 waves each run `iters` x 64
 * register-resident v_mfma_f32_16x16x32_f16 (fp16 operands with random mantissas): executed FLOPs = workgroups * 4 * iters *
 * 64 * 2 * 16 * 16 * 32.  out: workgroups * 256 floats (sink); clk: two 64-bit words zeroed by the caller - sums of the
 * shader-clock cycles (s_memtime) and of the 100 MHz ticks (s_memrealtime) the sampled waves spent in the loop, so the clock
 * the chip HELD inside the kernel is 100 MHz * clk[0] / clk[1].  The caller times the launch with events on `stream`. */
int sfh_probe_mfma_f16(int iters, int workgroups, float* out, uint64_t* clk, void* stream);

/* ---- engine-build helpers (csrc/hostprep.hip, round 6): what an engine needs while it packs a checkpoint, so that no stock
 * torch kernel runs on the predict path (the reference does this work inside nn.Module construction / cuDNN descriptors).
 *
 * sfh_multi_absminmax: ONE launch over `ntensors` float32 tensors - table = device array of {const float* ptr; int64 numel}
 * pairs - leaves in words[2 t] the bit pattern of max |x| of tensor t and in words[2 t + 1] 0x7FFFFFFF - (bit pattern of min
 * |x|); `words` must be zero-filled by the caller (zero is the identity of both).  A NaN / Inf element shows as a pattern >=
 * 0x7F800000.  The exponent of every two-plane fp16 weight tensor of a model comes from one call and one read-back
 * (replaces a torch abs().max() + host sync per layer); the min leg answers "does any folded BatchNorm scale vanish".      */
int sfh_multi_absminmax(const void* table, int ntensors, uint32_t* words, void* stream);

/* dst[i] = a[i] * factor (op 0), a[i] / b[i % nb] (op 1; factor applied after the division when != 1) or a[i] * b[i % nb] *
 * factor (op 2), float32, n elements; dst may alias a.  The folded scale / shift vectors of a layer (<= 16 K floats).    */
int sfh_vec_op(int op, const float* a, const float* b, int64_t n, int nb, float factor, float* dst, void* stream);

/* Pitched copy of 4-byte words: rows x width, pitches in words (channel slices of OIHW weights: the skip half of an Up
 * block's first conv, unet/unet_parts.py:67).                                                                           */
int sfh_copy2d_words(const void* src, int64_t src_pitch, void* dst, int64_t dst_pitch, int width, int64_t rows, void* stream);

/* dst[0 .. n) = value (4-byte words): range words, flags, constant scale / shift vectors.                                 */
int sfh_fill_words(void* dst, int64_t n, uint32_t value, void* stream);

/* *flag |= 1 (flag zero-filled by the caller) if any of rows 1 .. rows-1 of a (rows, row_words) array of 4-byte words differs
 * from row 0: "is the court template ONE image replicated over the batch" (utils/dataset.py:59), asked once per template. */
int sfh_rows_differ(const void* x, int64_t row_words, int rows, uint32_t* flag, void* stream);

/* ResNet-STN input for the modes the fused OutConv epilogue does not assemble (models/reconstructor.py:174-183,214: "img",
 * "mask", "img+mask+uv", and "img+mask" with resized logits): dst (B,H,W,cs) NHWC = cat((logits (B,nc,H,W), frame (B,cf,H,W),
 * uv (B,cu,H,W)), channel), zero-padded to cs; a source with 0 channels may be NULL.  Replaces torch.cat + a layout pass. */
int sfh_stn_input_assemble(const float* logits, int nc, const float* frame, int cf, const float* uv, int cu, int batch, int H,
                           int W, int cs, float* dst, void* stream);

/* Validation scores (eval.py:142-234, eval_reconstructor): slots of the fp64 accumulator vector that sfh_eval_batch adds one
 * batch into.  The caller zero-fills it once per evaluation and writes len(loader) into SFH_EVAL_NBATCH; sfh_uv_loss (lambda
 * 1) adds the uv score into SFH_EVAL_UV; SFH_EVAL_BAD mirrors the error flag.  Summed over ranks as one vector.            */
#define SFH_EVAL_SEG 0
#define SFH_EVAL_REC 1
#define SFH_EVAL_UV 2
#define SFH_EVAL_REPROJ 3
#define SFH_EVAL_REPROJ_PX 4
#define SFH_EVAL_CONSIST 5
#define SFH_EVAL_NBATCH 6
#define SFH_EVAL_FRAMES 7
#define SFH_EVAL_BAD 8
#define SFH_EVAL_SLOTS 9

/* Workspace of sfh_eval_batch in doubles: 5 per frame row plus 7 per frame; -1 for a bad shape.                          */
int64_t sfh_eval_workspace_doubles(int batch, int H, int W);

/* One validation batch into acc (SFH_EVAL_* slots), deterministic (fixed-order fp64 sums, no atomics on any sum), no host
 * synchronisation.  logits NCHW (B,nc,H,W) fp32, mask int64 (B,H,W), warp_mask fp32 (B,H,W); logits or warp_mask may be NULL
 * (that score is skipped), the mask may be NULL only if both are.  Per pixel, lse = logsumexp over the nc logits:
 *   seg     = lse - L[g], 0 and not counted where g == -100 (F.cross_entropy's ignore_index);
 *   rec     = (warp - fp32(g) / nc)^2;
 *   consist = lse - L[trunc(fp32(warp * nc))], 0 and not counted where that class is -100.
 * weight (B) fp32 non-NULL: acc[SEG] += mean_b(weight_b * mean_px seg), acc[REC] likewise (models/losses.py:33-41); NULL:
 * acc[SEG] += sum seg / counted pixels, acc[REC] += mean rec.  acc[CONSIST] += sum consist / counted pixels (if both logits and
 * warp).  poi, gt_poi (B,npts,2), nonzeros (B,npts), num_nonzero (B), all fp32, all NULL or none: acc[REPROJ] += sum_b
 * sum_n ||gt - poi|| * nonzeros / num_nonzero (models/losses.py:6-19, reduction 'sum') and acc[REPROJ_PX] += the same with x
 * scaled by target_w and y by target_h in fp32 (eval.py:205-215).  acc[FRAMES] += B.  A mask id outside [0, nc) other than
 * -100 ORs 1, a consistency class outside [0, nc) other than -100 (NaN included) ORs 2 into *flag (caller-zeroed, sticky;
 * torch raises on both); acc[BAD] = *flag after the batch.  workspace: sfh_eval_workspace_doubles(batch, H, W); nc 1 .. 8. */
int sfh_eval_batch(const float* logits, const int64_t* mask, const float* warp_mask, const float* weight, int nc, int batch,
                   int H, int W, const float* poi, const float* gt_poi, const float* nonzeros, const float* num_nonzero, int npts,
                   float target_w, float target_h, double* workspace, uint32_t* flag, double* acc, void* stream);

/* Training augmentation of a batch on the device (utils/augmentation.py: torchvision ColorJitter, GaussianBlur,
 * RandomResizedCrop, RandomHorizontalFlip, UVHorizontalFlip, PoIHorizontalFlip), csrc/augment.hip.  Every random decision is
 * made by the caller and arrives in `params`: device int32 (B,16) per sample = order[4] (the jitter op of slot 0..3: 0
 * brightness, 1 contrast, 2 saturation, 3 hue), factor[4] per op (fp32 bits), enabled (bit op), sigma (fp32 bits, 0 = no
 * blur), crop i, j, h, w, flip, 0.  The caller validates it (a permutation, finite factors, the crop inside the frame); the
 * kernels clamp the crop so that no block can address outside the frame.  No atomics: results are bit-reproducible.      */

/* Row partials of sfh_aug_gray_mean in doubles (batch * H); -1 for a bad shape.                                          */
int64_t sfh_aug_workspace_doubles(int batch, int H);

/* Contrast's mean, first stage (needed only when some sample has contrast enabled): per frame row, the sum in fp64 of
 * gray = 0.2989 r + 0.587 g + 0.114 b of the frame (uint8 (B,H,W,3), / 255) after the ops that precede contrast in that
 * sample's order -> workspace[b * H + y] (0 for a sample without contrast).                                               */
int sfh_aug_gray_mean(const uint8_t* frames, const int32_t* params, int batch, int H, int W, double* workspace, void* stream);

/* The fused pass: frames uint8 (B,H,W,3) -> image fp32 (B,3,H,W) = flip(resize(crop(blur(jitter(frames / 255))))) with
 * torchvision.transforms.functional's tensor arithmetic in fp32: the jitter ops in the sample's order (contrast against the
 * mean of the whole frame: the fixed-order sum of `workspace` / (H * W); workspace NULL = no sample has contrast on), a
 * blur_k x blur_k Gaussian of the sample's sigma with reflect padding at the frame border (blur_k odd, 1 .. 11; 1 = none),
 * bilinear align_corners=False resize of the crop to (H,W), horizontal flip.  masks uint8 (B,H,W) -> mask_out int64 and uv
 * fp32 (B,uv_channels,H,W) -> uv_out through the same crop with legacy nearest (src = min(floor(dst * (float)in / out),
 * in - 1)) and flip, uv channel 0 becoming (u > 0) - u under a flip; either pair may be NULL.  mean_out (B) fp32 or NULL:
 * the contrast mean used per sample (0 where contrast is off).                                                            */
int sfh_aug_apply(const uint8_t* frames, const uint8_t* masks, const float* uv, const int32_t* params, const double* workspace,
                  int batch, int H, int W, int blur_k, int uv_channels, float* image, int64_t* mask_out, float* uv_out,
                  float* mean_out, void* stream);

/* poi (B,npts,2) / nonzeros (B,npts) fp32 of flipped samples through the involution perm (int32, npts): out[n] =
 * (1 - poi[perm[n]].x, poi[perm[n]].y), nonzeros_out[n] = nonzeros[perm[n]]; other samples are copied.  nonzeros may be NULL. */
int sfh_aug_poi_flip(const float* poi, const float* nonzeros, const int32_t* perm, const int32_t* params, int batch, int npts,
                     float* poi_out, float* nonzeros_out, void* stream);

/* Court overlay frames (viz_preds.py:117-146, utils/postprocess.py:21-65), csrc/overlay.hip.  `source` of both entries:   */
#define SFH_OVERLAY_AUTO 0   /* per frame from score[b]: warp leg where score[b] < score_threshold, else segmentation leg */
#define SFH_OVERLAY_WARP 1   /* every frame takes the warp leg (score may be NULL)                                         */
#define SFH_OVERLAY_SEGM 2   /* every frame takes the segmentation leg (score may be NULL)                                 */
#define SFH_OVERLAY_LABEL_MAX 32   /* glyphs of a label row (the L of sfh_overlay_annotate) at most                        */

/* ONE launch: frames uint8 (B,H,W,3) -> out uint8 (B,H,W,3), out == frames allowed (a pixel depends on its own frame pixel
 * only).  Per frame a class-id mask comes from one of two legs, chosen on the device:
 *   warp leg: trunc(nearest homography warp of tmpl (ht x wt, batch stride tmpl_bstride floats, 0 = one shared image) by
 *             theta[b] at (H,W) * out_scale) - the ids of sfh_homography_warp_fwd(mode 0, out_i32) for the same arguments;
 *   segmentation leg: segm (B,hs,ws) int32 ids (segm_kind 0) / uint8 ids (1) or fp32 NCHW logits (B,nc,hs,ws) (2, first
 *             maximum wins), resized to (H,W) with sfh_mask_format_fwd's INTER_NEAREST index rule; segm NULL: no mask.
 * palette: HOST pointer to 8 x 3 bytes, ids outside 0..7 count as 0.  A pixel whose colour is (0,0,0) keeps the frame bytes,
 * any other becomes (colour_c + frame_c) >> 1 per channel (= the reference's float64 colour * 0.5 + frame * 0.5 truncated).
 * The blend is applied when the frame has a mask and (use_overlay_threshold == 0 or score[b] < overlay_threshold); otherwise
 * the frame is copied.  score: device fp32 (B); required for SFH_OVERLAY_AUTO and with an overlay threshold.  A NaN score
 * compares false everywhere.  theta / tmpl may be NULL for SFH_OVERLAY_SEGM.                                              */
int sfh_overlay_render(const uint8_t* frames, uint8_t* out, int batch, int H, int W, const float* theta, const float* tmpl,
                       int64_t tmpl_bstride, int ht, int wt, float out_scale, const void* segm, int segm_kind, int nc, int hs,
                       int ws, const float* score, float score_threshold, int source, int use_overlay_threshold,
                       float overlay_threshold, const uint8_t* palette, void* stream);

/* ONE launch over out uint8 (B,H,W,3): POI markers and a label per frame; either part may be absent (poi / labels NULL).
 * Markers: poi (B,npts,2) fp32 in [0,1]; centre = (rint(x * W), rint(y * H)), the product exact in fp64, ties to even; a
 * filled disc dx^2 + dy^2 <= radius^2 of marker_color (HOST pointer, 3 bytes) clipped at the frame border; a NaN / inf
 * centre draws nothing; radius 0 draws no markers.  Label: labels int8 (B,L) glyph codes of the 5x7 font in csrc/overlay.hip
 * (0-9 digits, 10 '.', 11 '-', 12 '+', 13 'e', 14 ' ', 15 'n', 16 'a', 17 'i', 18 'f'; a negative code ends the row), L <=
 * SFH_OVERLAY_LABEL_MAX, glyph cells of 6 x 7 font pixels of label_scale x label_scale frame pixels, top-left at (label_x,
 * label_y), clipped; colour (0,255,0) where score[b] < score_threshold, else (0,0,255); with score NULL (forced source
 * only) (0,255,0) for SFH_OVERLAY_WARP and (0,0,255) for SFH_OVERLAY_SEGM.  Deterministic: a later point index wins over an
 * earlier one and the label is drawn last - every pixel has exactly one writer.                                           */
int sfh_overlay_annotate(uint8_t* out, int batch, int H, int W, const float* poi, int npts, int radius,
                         const uint8_t* marker_color, const int8_t* labels, int L, int label_x, int label_y, int label_scale,
                         const float* score, float score_threshold, int source, void* stream);

/* Training labels from manual POI annotations (dataset_utils/preparation.py), csrc/prepare.hip.                           */
#define SFH_PREP_MAX_POINTS 256   /* template points of a fit at most                                                       */
#define SFH_PREP_JACOBI_SWEEPS 12 /* cyclic Jacobi sweeps over the 9 x 9 normal matrix                                      */

/* ONE launch for any batch, everything fp64: per frame the homography court -> frame from the point pairs (court_poi[i] in
 * [-1,1], 2 * manual_poi[b][i] - 1) of every point with manual x != -1 and y != -1 (calculate_homography's test).  Rule:
 * Hartley normalisation of both sets (centroid to the origin, mean distance sqrt 2), the 9 x 9 matrix L^T L of the DLT rows
 * (-x,-y,-1,0,0,0,ux,uy,u), (0,0,0,-x,-y,-1,vx,vy,v), its eigenvector of the smallest eigenvalue by SFH_PREP_JACOBI_SWEEPS
 * cyclic Jacobi sweeps, denormalised and divided by h33; then `refine` damped Gauss-Newton steps on h11..h32 against the
 * summed squared forward reprojection error in normalised frame coordinates (Marquardt scaling, lambda 1e-3, / 10 after an
 * accepted and * 10 after a rejected step; a step is accepted only when it lowers the cost).  Sums over points: slot
 * l = i mod 64 adds its points in index order, the 64 slots are combined by the butterfly l ^ 32, 16, 8, 4, 2, 1 - no
 * atomics, the same bits every run.  Outputs per frame: theta_c2f (9, h33 = 1), theta = inverse(theta_c2f) / its last entry
 * (frame -> court: Reconstructor.warp's convention), theta_f32 = theta rounded once (may be NULL), poi (npts,3): court
 * points through theta_c2f with Kornia's s = 1 / (z + 1e-8) (|z| > 1e-8, else 1), then / 2 + 0.5, third column the flag of
 * find_nonzero_points (0 where ignore_mask[i] != 0 or manual == (-1,-1)); num_nonzero = number of flags; rmse =
 * sum(flag * |poi * norm - manual * norm|) / num_nonzero (calculate_reprojection_rmse; norm_w = norm_h = 1 for none);
 * status 1, or 0 with every other output of the frame zero when fewer than 4 points are usable.  ignore_mask: device uint8
 * (npts) or NULL.  npts <= SFH_PREP_MAX_POINTS.                                                                            */
int sfh_prep_fit(const double* court_poi, const double* manual_poi, const uint8_t* ignore_mask, int batch, int npts,
                 double norm_w, double norm_h, int refine, double* theta_c2f, double* theta, float* theta_f32, double* poi,
                 int32_t* num_nonzero, double* rmse, int32_t* status, void* stream);

/* ONE launch: the class-id label mask (B,H,W) uint8 of theta (B,9) fp32 - pixel = ids[tap], the tap being exactly the
 * nearest tap of sfh_homography_warp_fwd(mode 0) on an hs x ws template (zero outside) - and, with want_uv, uv (B,H,W,3)
 * uint16 = (id, u_tab[tap x], v_tab[tap y]), zero outside.  ids uint8 (hs,ws), u_tab uint16 (ws), v_tab uint16 (hs): device
 * pointers.  W must be a multiple of 4 (every lane stores four pixels at once).                                            */
int sfh_prep_render(const float* theta, const uint8_t* ids, int hs, int ws, const uint16_t* u_tab, const uint16_t* v_tab,
                    int batch, int H, int W, int want_uv, uint8_t* mask, uint16_t* uv, void* stream);

/* convert_rgb_to_onehot / generate_onehot: npix pixels of 3 bytes -> one byte each: k where the pixel equals colour k of
 * the num_classes (4, 7, 8) table of sfh_mask_format_fwd's rgb mode (k >= 1), else the pixel's byte 0.                     */
int sfh_prep_rgb_to_ids(const uint8_t* rgb, int64_t npix, int num_classes, uint8_t* ids, void* stream);

/* Frame -> court mapping and top-view rectification (utils/transform.py, utils/court.py, utils/mapping_example.py),
 * csrc/mapping.hip.  theta is frame -> court in the model's convention (Reconstructor.warp samples the court template into the
 * frame with it); theta_c2f, its inverse, samples the frame into the court view and maps court points into the frame.     */

/* theta (B,3,3) fp32 -> theta_c2f (B,3,3) fp32: the fp64 adjugate times the fp64 reciprocal of the determinant, every operation
 * individually rounded, each entry rounded once to fp32 - the matrix sfh_poi_project_fwd applies.  status (B) uint8: 1 when
 * every entry of theta is finite and the determinant is finite and non-zero; otherwise 0 and theta_c2f of that frame is all
 * zeros.                                                                                                                   */
int sfh_theta_invert(const float* theta, int batch, float* theta_c2f, uint8_t* status, void* stream);

/* ONE launch: frames uint8 (B,H,W,3) -> top_view uint8 (B,hc,wc,3) and valid uint8 (B,hc,wc).  Court pixel (y, x) samples
 * the frame at unnorm(apply_h(theta_c2f[b], norm_axis(x, wc), norm_axis(y, hc)), frame size): the pinned fp32 coordinate
 * arithmetic of sfh_homography_warp_fwd with the frame as the sampled image.  mode 0: the nearest tap (round half to even;
 * the reference's Warper); mode 1: the four bilinear taps blended in fp32 in the order ((t00 w00 + t01 w01) + t10 w10) + t11
 * w11, rounded half to even and clamped to a byte.  Taps outside the frame give zero.  valid = 255 where the NEAREST tap lies
 * inside the frame (both modes), else 0.  A frame with status[b] == 0, or, with score non-NULL, a score[b] that is NaN or
 * above max_score, gives zeros and valid 0: decided on the device, no host read-back.  score (B) fp32 may be NULL (no gate).
 * H * W < 2^24; hc, wc 2 .. 16384.                                                                                         */
int sfh_topview_render(const uint8_t* frames, int batch, int H, int W, const float* theta_c2f, const uint8_t* status,
                       const float* score, float max_score, int hc, int wc, int mode, uint8_t* top_view, uint8_t* valid,
                       void* stream);

/* ONE launch: the court mosaic of a clip.  For every used frame (the rule of sfh_topview_render) in batch order, the bytes of
 * the nearest tap of every court pixel whose tap is valid are added to sum uint32 (hc,wc,3) and 1 to count uint32 (hc,wc);
 * both persist across calls (the caller zeroes them once).  One thread owns one court pixel: no atomics, and the integer
 * sums do not depend on how a clip is split into calls.  Limit: a pixel's count must stay below 2^32 / 255 frames.        */
int sfh_topview_accumulate(const uint8_t* frames, int batch, int H, int W, const float* theta_c2f, const uint8_t* status,
                           const float* score, float max_score, int hc, int wc, uint32_t* sum, uint32_t* count, void* stream);

/* image uint8 (hc,wc,3) = (2 * sum + count) / (2 * count) in integers (the mean, halves up); 0 where count == 0.            */
int sfh_topview_finish(const uint32_t* sum, const uint32_t* count, int hc, int wc, uint8_t* image, void* stream);

/* ONE launch for any n: points (n,2) fp32 through thetas[frame_index[i]] of a table (nframes,3,3) fp32 holding theta (frame ->
 * court) or theta_c2f (court -> frame): the caller picks the direction.  frame_index int32 (n), or NULL: every point uses
 * row frame0.  Per point: (1) with in_w, in_h != 0 the normalisation (p / size - 0.5) * 2 in fp32 (utils/transform.py:38-39 on
 * its float32 array; 0, 0 = already normalised); (2) X, Y, W = ((t0 x + t1 y) + t2) ... in fp64; (3) w' = 1 / W if |W| >
 * FLT_EPSILON else 0 (cv2.perspectiveTransform's rule); (4) ((X w') / 2 + 0.5) * out_sx, likewise y with out_sy, rounded once
 * to fp32.  Every fp64 operation is individually rounded.  flag (n) uint8: 0, with out = (0, 0), for a frame index outside
 * [0, nframes), w' == 0 or a non-finite result; else 1.                                                                    */
int sfh_map_points(const float* points, const int32_t* frame_index, int frame0, int64_t n, const float* thetas, int nframes,
                   float in_w, float in_h, double out_sx, double out_sy, float* out, uint8_t* flag, void* stream);

/* Standard PNG files from uint8 device images, csrc/pngenc.hip (the byte-exact rule: tests/pngenc_ref.py).  8-bit gray
 * (C = 1) or RGB (C = 3), non-interlaced; every scanline filter 1 (Sub); the filtered stream cut into strips of
 * max(1, min(SFH_PNG_STRIP_ROWS, SFH_PNG_MAX_ROW / (1 + W C))) rows, each strip one deflate block (fixed Huffman: maximal runs
 * of equal bytes as a literal + distance-1 matches; or stored when that would be longer than the strip + 5 bytes) in one
 * IDAT chunk; strips that are not the last end with an empty stored block so that they concatenate on byte boundaries.   */
#define SFH_PNG_MAX_ROW 32768   /* bytes of a filtered scanline, 1 + W C, at most                                           */
#define SFH_PNG_STRIP_ROWS 16   /* rows of a strip at most                                                                  */

/* Upper bound of the file size of an H x W x C image: 8 + 25 + 12 + strips * (12 + 5) + H (1 + W C) + 2 + 4.  -1 for
 * C other than 1, 3, non-positive sizes or a scanline above SFH_PNG_MAX_ROW.                                               */
int64_t sfh_png_capacity(int H, int W, int C);
/* bytes of the scratch buffer of sfh_png_encode / sfh_png_pack (16-byte aligned): per strip a 16-byte record and a slot  */
int64_t sfh_png_scratch_bytes(int batch, int H, int W, int C);

/* ONE launch, one workgroup per (image, strip): images uint8 (B,H,W) or (B,H,W,3) -> every strip's finished IDAT chunk
 * (length, tag, data, CRC-32) in its slot of scratch, its byte count and Adler-32 partial sums in its record.  bgr != 0: a
 * 3-channel image is BGR in memory (RGB in the file, cv2's convention); 0: RGB in memory.  No atomics on global memory.  */
int sfh_png_encode(const uint8_t* images, int batch, int H, int W, int C, int bgr, uint8_t* scratch, int64_t scratch_bytes,
                   void* stream);

/* ONE launch, one workgroup per image: scratch of sfh_png_encode (same batch, H, W, C) -> the files.  compact == 0: file b
 * starts at out + b * sfh_png_capacity; != 0: the files lie back to back.  offsets int64 (B + 1): start of every file,
 * offsets[B] the end of the last (compact) or B * capacity; sizes int32 (B).  out_bytes >= B * capacity in both modes;
 * nothing is written at or beyond offsets[b] + capacity of any file.                                                      */
int sfh_png_pack(const uint8_t* scratch, int64_t scratch_bytes, int batch, int H, int W, int C, int compact, uint8_t* out,
                 int64_t out_bytes, int64_t* offsets, int32_t* sizes, void* stream);

/* Baseline JFIF files from uint8 device images, csrc/jpegenc.hip (the byte-exact rule is libjpeg's with a restart interval of
 * one MCU row, restated in tests/jpegenc_ref.py): gray (C = 1) or 4:2:0 YCbCr (C = 3), Annex K quantisation tables scaled by
 * `quality` (1 .. 100, libjpeg's rule), Annex K Huffman tables, integer arithmetic only.                                  */
#define SFH_JPEG_MAX_WIDTH 2048   /* pixels of an image row at most: an MCU row is encoded in one workgroup's LDS             */

/* Upper bound of the file size of an H x W x C image: the header (334 bytes gray, 629 colour) + per MCU row (8 pixel rows
 * gray, 16 colour) 2 * ceil(blocks * 1660 / 8) + 2, where 1660 = 22 + 63 * 26 bits is the longest code of a block (DC: an
 * 11-bit code + 11 bits; every AC coefficient: a 16-bit code + 10 bits), the factor 2 is every byte stuffed and the 2 bytes
 * are the RSTm / EOI marker.  -1 for C other than 1, 3, non-positive sizes, W above SFH_JPEG_MAX_WIDTH or H above 65535.   */
int64_t sfh_jpeg_capacity(int H, int W, int C);
/* bytes of the scratch buffer of sfh_jpeg_encode / sfh_jpeg_pack (16-byte aligned): per MCU row an 8-byte record
 * {bytes, passes} and a slot of the interval's capacity                                                                    */
int64_t sfh_jpeg_scratch_bytes(int batch, int H, int W, int C);

/* ONE launch, one workgroup per (image, MCU row): images uint8 (B,H,W) or (B,H,W,3) -> every restart interval's entropy-coded
 * bytes, stuffed, 1-padded and closed by RSTm (EOI in the last), in its slot of scratch.  bgr != 0: a 3-channel image is BGR
 * in memory (cv2's convention); 0: RGB.  window_dwords: 0, or (tests only) the size of the LDS bit window, which an interval
 * longer than it is emitted through in several passes; the record's second word counts them.  No atomics on global memory. */
int sfh_jpeg_encode(const uint8_t* images, int batch, int H, int W, int C, int bgr, int quality, uint8_t* scratch,
                    int64_t scratch_bytes, int window_dwords, void* stream);

/* ONE launch, one workgroup per image: scratch of sfh_jpeg_encode (same batch, H, W, C, quality) -> the files.  compact == 0:
 * file b starts at out + b * sfh_jpeg_capacity; != 0: the files lie back to back.  offsets int64 (B + 1), sizes int32 (B) as
 * sfh_png_pack's.  out_bytes >= B * capacity in both modes; nothing is written at or beyond offsets[b] + capacity.        */
int sfh_jpeg_pack(const uint8_t* scratch, int64_t scratch_bytes, int batch, int H, int W, int C, int quality, int compact,
                  uint8_t* out, int64_t out_bytes, int64_t* offsets, int32_t* sizes, void* stream);

/* Baseline JFIF files -> uint8 device frames, csrc/jpegdec.hip with the decode core csrc/jpegdec_core.h (the byte-exact rule is
 * libjpeg's - jidctint's "islow" IDCT, the triangle h2v2 upsampler, the 16-bit fixed-point YCbCr -> RGB tables - restated in
 * tests/jpegdec_ref.py, which tests/test_jpegdec_host.py holds to PIL's bytes).  Admitted: SOF0, 8 bits, one interleaved scan
 * (Ss, Se, Ah/Al = 0, 63, 0), gray or YCbCr at 4:2:0 or 4:4:4, any 8-bit quantisation and any Huffman tables, any restart
 * interval.  Everything else is refused on the host, with nothing launched: -1 and one of the reasons below; a reason of 100 or
 * more names a well-formed file that needs something not built.                                                              */
#define SFH_JPEG_R_OK 0
#define SFH_JPEG_R_TRUNCATED 1        /* the bytes end inside the header                                                       */
#define SFH_JPEG_R_NOT_JPEG 2         /* no SOI                                                                                */
#define SFH_JPEG_R_MARKER 3           /* a marker that may not stand where it stands, or fill bytes inside entropy-coded data  */
#define SFH_JPEG_R_BAD_SOF 4
#define SFH_JPEG_R_BAD_TABLE 5        /* a DQT / DHT segment that defines no valid table, or a table used but not defined      */
#define SFH_JPEG_R_BAD_SOS 6
#define SFH_JPEG_R_RESTART 7          /* RSTm out of sequence, or not as many as the restart interval asks for                 */
#define SFH_JPEG_R_SIZE 8             /* width, height or channels other than the decoder's                                    */
#define SFH_JPEG_R_TOO_LONG 9         /* more bytes than the decoder's max_file_bytes                                          */
#define SFH_JPEG_R_PROGRESSIVE 100
#define SFH_JPEG_R_ARITHMETIC 101
#define SFH_JPEG_R_PRECISION 102      /* 12-bit samples                                                                        */
#define SFH_JPEG_R_DQT16 103          /* 16-bit quantisation tables                                                            */
#define SFH_JPEG_R_COMPONENTS 104     /* 2 or 4 components                                                                     */
#define SFH_JPEG_R_COLORSPACE 105     /* 3 components that are RGB by libjpeg's rule                                           */
#define SFH_JPEG_R_SAMPLING 106       /* 4:2:2, 4:4:0, 4:1:1, ...                                                              */
#define SFH_JPEG_R_NONINTERLEAVED 107 /* more than one scan                                                                    */
#define SFH_JPEG_R_DNL 108            /* DNL, or a height of 0                                                                 */
#define SFH_JPEG_R_SOF_TYPE 109       /* extended sequential, lossless, hierarchical                                           */

/* One Huffman table in the form the kernel reads: look[b] = length << 8 | symbol of the code of at most 8 bits that the byte b
 * starts with (0: none); a longer code c of length l is valid iff c <= maxcode[l] (-1: no code of that length) and its symbol
 * is vals[c + valoff[l]]; maxcode[0] = -1, maxcode[17] = INT32_MAX; vals in code order.                                      */
typedef struct sfh_jpeg_hufftab {
  uint16_t look[256];
  int32_t maxcode[18];
  int32_t valoff[18];
  uint8_t vals[256];
} sfh_jpeg_hufftab;

/* The parse of one file (7920 bytes).  hsamp, vsamp: sampling of component 0 (2, 2: 4:2:0; 1, 1: 4:4:4 and gray).  qsel / dcsel /
 * acsel: table of every component.  quant: natural (row-major) order.  scan_begin / scan_end: the entropy-coded bytes.
 * file_pos, file_bytes, seg_pos, nsub: filled by sfh_jpeg_dec_stage only - where the file and its segment table lie in the
 * staging buffer and the subsequences of its segments together.                                                             */
typedef struct sfh_jpeg_info {
  int32_t width, height, ncomp, hsamp, vsamp;
  int32_t mcus_x, mcus_y, blocks_per_mcu;
  int32_t restart_interval, nsegments;
  int32_t scan_begin, scan_end;
  int32_t reason;
  int32_t qsel[3], dcsel[3], acsel[3];
  int32_t file_pos, file_bytes, seg_pos, nsub;
  int32_t reserved[2];
  uint16_t quant[4][64];
  sfh_jpeg_hufftab dc[4], ac[4];
} sfh_jpeg_info;

/* Host code, no device: walks the markers of host_bytes[0, n) -> host_info, and the segments of the scan (the bytes between
 * RSTm markers, found by a scan for FF D0..D7; a file without DRI is one segment) as int32 quadruples {first byte, end byte,
 * first MCU, 0} in host_segs, as many as seg_cap admits (host_segs may be NULL with seg_cap 0); host_info->nsegments counts all.
 * 0, or -1 with host_info->reason = SFH_JPEG_R_*.                                                                            */
int sfh_jpeg_parse(const uint8_t* host_bytes, int64_t n, sfh_jpeg_info* host_info, int32_t* host_segs, int64_t seg_cap);

/* bytes of the staging buffer (pinned host memory and its device copy, 16-byte aligned) and of the device scratch buffer of a
 * decoder of `batch` H x W x C files of at most max_file_bytes; -1 for bad arguments (subseq_bits: a multiple of 32 in
 * 32 .. 65536) and for buffers of 2 GiB or more.                                                                             */
int64_t sfh_jpeg_dec_staging_bytes(int batch, int H, int W, int C, int64_t max_file_bytes);
int64_t sfh_jpeg_dec_scratch_bytes(int batch, int H, int W, int C, int64_t max_file_bytes, int subseq_bits);

/* Host code, no device: parses `batch` files and packs the batch into host_staging - a 64-byte head {magic, batch, largest
 * segment count, subseq_bits, used bytes}, the sfh_jpeg_info of every file, every file's segment table (the fourth word of a
 * quadruple: the segment's first subsequence slot), the files at 16-byte aligned positions - for ONE copy to the device.
 * Returns the bytes used, or -1 with *host_reason = SFH_JPEG_R_* and *host_index = the file refused (a file whose size or
 * channels are not H, W, C: SFH_JPEG_R_SIZE; longer than max_file_bytes: SFH_JPEG_R_TOO_LONG).                               */
int64_t sfh_jpeg_dec_stage(const uint8_t* const* host_files, const int64_t* host_sizes, int batch, int H, int W, int C,
                           int64_t max_file_bytes, int subseq_bits, uint8_t* host_staging, int64_t staging_bytes,
                           int32_t* host_reason, int32_t* host_index);

/* One hipMemsetAsync (coefficients and segment records) and ONE launch, one workgroup per (image, segment): `staged`, the device
 * copy of host_staging (which is read here for its head only) -> the quantised coefficients of every block as int16 in natural
 * order, MCU order, in scratch, and per segment a record {rounds, status}.  The segment's bits are cut into subsequences of
 * subseq_bits bits; a bounded fixed-point iteration over their exit states (bit position, block in the MCU, zig-zag index) finds
 * every subsequence's true entry state in at most as many rounds as there are subsequences, whatever the bytes are; a last pass
 * scatters the coefficients.  Reads are clamped to the segment's bytes, writes to its blocks; status != 0 (JD_E_* of
 * csrc/jpegdec_core.h): an invalid code, a run past coefficient 63, bits that end early, blocks left over.  No global atomics,
 * no waiting between workgroups.                                                                                             */
int sfh_jpeg_entropy_decode(const uint8_t* host_staging, const uint8_t* staged, int64_t staged_bytes, int batch, int H, int W,
                            int C, int64_t max_file_bytes, int subseq_bits, uint8_t* scratch, int64_t scratch_bytes, void* stream);

/* THREE launches (two for gray): the segment records -> status int32 (B) (the OR over the image's segments) and rounds int32 (B)
 * (their largest round count); dequantisation and jidctint's IDCT of every block into planes in scratch (gray: into out); the
 * h2v2 triangle upsampling and YCbCr -> RGB into out uint8 (B,H,W,3) (bgr != 0: BGR in memory) or (B,H,W).  An image whose
 * status is not 0 comes back as zeros.                                                                                       */
int sfh_jpeg_decode_pixels(const uint8_t* staged, int batch, int H, int W, int C, int hsamp, int bgr, int64_t max_file_bytes,
                           int subseq_bits, uint8_t* scratch, int64_t scratch_bytes, uint8_t* out, int32_t* status,
                           int32_t* rounds, void* stream);

/* Standard PNG files -> uint8 device images, csrc/pngdec.hip with the decode core csrc/pngdec_core.h (the pixels are those of
 * outputs.decode_png, which tests/test_pngdec_host.py holds to PIL's).  Admitted: non-interlaced 8-bit files of colour type 0, 2
 * and 6, all five scanline filters, any number of IDAT chunks cut anywhere, stored, fixed and dynamic blocks, a zlib header with
 * CM = 8, a window of at most 32 KB and no preset dictionary; ancillary chunks are skipped.  Everything else is refused on the
 * host, with nothing launched: -1 and one of the reasons below; a reason of 100 or more names a well-formed file that needs
 * something not built.                                                                                                       */
#define SFH_PNG_R_OK 0
#define SFH_PNG_R_TRUNCATED 1         /* the bytes end before IHDR is complete                                                 */
#define SFH_PNG_R_NOT_PNG 2           /* no PNG signature                                                                      */
#define SFH_PNG_R_CRC 3               /* a chunk whose CRC-32 is not the one stored                                            */
#define SFH_PNG_R_BAD_IHDR 4          /* IHDR missing, not first, repeated, or with values the format does not have            */
#define SFH_PNG_R_IDAT_ORDER 5        /* IDAT chunks that are not consecutive                                                  */
#define SFH_PNG_R_NO_IDAT 6
#define SFH_PNG_R_NO_IEND 7           /* the chunks end without IEND                                                           */
#define SFH_PNG_R_ZLIB 8              /* a zlib header that is not CM 8, window <= 32 KB, check bits right                      */
#define SFH_PNG_R_ZLIB_DICT 9         /* a preset dictionary                                                                   */
#define SFH_PNG_R_CRITICAL 10         /* a critical chunk that is not IHDR, PLTE, IDAT, IEND                                   */
#define SFH_PNG_R_SIZE 11             /* width, height or channels other than the decoder's                                    */
#define SFH_PNG_R_TOO_LONG 12         /* more bytes than the decoder's max_file_bytes                                          */
#define SFH_PNG_R_BIT_DEPTH 100       /* 1, 2, 4 or 16 bits                                                                    */
#define SFH_PNG_R_PALETTE 101
#define SFH_PNG_R_GRAY_ALPHA 102
#define SFH_PNG_R_INTERLACE 103       /* Adam7                                                                                 */
#define SFH_PNG_R_APNG 104
#define SFH_PNG_DEC_MAX_SEGMENTS 1024 /* IDAT chunks of a file that the segmented leg is tried on at most                      */

/* The parse of one file (64 bytes).  channels: 1, 3, 4.  idat_bytes: of all IDAT bodies together; cmf, flg: their first two
 * bytes; adler: their last four, big endian.  file_pos, file_bytes, range_pos, joined_pos: filled by sfh_png_dec_stage only -
 * where the file, its range table and the table of every body's offset in the joined bodies lie in the staging buffer.      */
typedef struct sfh_png_info {
  int32_t width, height, channels, bit_depth, color_type, interlace;
  int32_t nidat, idat_bytes, cmf, flg;
  uint32_t adler;
  int32_t reason;
  int32_t file_pos, file_bytes, range_pos, joined_pos;
} sfh_png_info;

/* Host code, no device: checks the signature, walks the chunks of host_bytes[0, n) and verifies every chunk's CRC-32 with a
 * table, reads IHDR and the zlib header -> host_info, and the IDAT bodies as int32 pairs {first byte, end byte} in host_ranges,
 * as many as range_cap admits (host_ranges may be NULL with range_cap 0); host_info->nidat counts all.  0, or -1 with
 * host_info->reason = SFH_PNG_R_*.                                                                                           */
int sfh_png_parse(const uint8_t* host_bytes, int64_t n, sfh_png_info* host_info, int32_t* host_ranges, int64_t range_cap);

/* bytes of the staging buffer (pinned host memory and its device copy, 16-byte aligned) and of the device scratch buffer of a
 * decoder of `batch` H x W x C files (C = 1, 3, 4) of at most max_file_bytes; -1 for bad arguments, a filtered stream
 * H (1 + W C) of 2 GiB or more and for buffers of 2 GiB (staging) / 4 GiB (scratch) or more.                                 */
int64_t sfh_png_dec_staging_bytes(int batch, int H, int W, int C, int64_t max_file_bytes);
int64_t sfh_png_dec_scratch_bytes(int batch, int H, int W, int C);

/* Host code, no device: parses `batch` files and packs the batch into host_staging - a 64-byte head {magic, batch, largest
 * IDAT count, used bytes}, the sfh_png_info of every file, every file's range table and joined offsets, the files at 16-byte
 * aligned positions - for ONE copy to the device.  Returns the bytes used, or -1 with *host_reason = SFH_PNG_R_* and
 * *host_index = the file refused.                                                                                           */
int64_t sfh_png_dec_stage(const uint8_t* const* host_files, const int64_t* host_sizes, int batch, int H, int W, int C,
                          int64_t max_file_bytes, uint8_t* host_staging, int64_t staging_bytes, int32_t* host_reason,
                          int32_t* host_index);

/* `staged`, the device copy of host_staging (which is read here for its head only) -> out uint8 (B,H,W) or (B,H,W,C) (bgr != 0:
 * BGR(A) in memory), status int32 (B) (the PD_E_* bits of csrc/pngdec_core.h; such an image comes back as zeros) and segmented
 * int32 (B) (1: the image's filtered stream came from the segmented leg).  One small memset, then: when a file of the batch has
 * 2 .. SFH_PNG_DEC_MAX_SEGMENTS IDAT chunks and serial_only == 0, the segmented leg - count pass, one workgroup per (image,
 * chunk); acceptance, on the device; write pass; Adler-32 partials; verdict - and then always the serial leg - inflate, one
 * workgroup per image, which exits at once for an accepted image; Adler-32 partials; verdict - and the two unfilter kernels, of
 * which exactly one does an image's work.  5 or 10 launches, no global atomics, no workgroup waits for another, no host
 * synchronisation.                                                                                                           */
int sfh_png_decode(const uint8_t* host_staging, const uint8_t* staged, int64_t staged_bytes, int batch, int H, int W, int C,
                   int bgr, int64_t max_file_bytes, int serial_only, uint8_t* scratch, int64_t scratch_bytes, uint8_t* out,
                   int32_t* status, int32_t* segmented, void* stream);

/* Pillow's 8-bit image resize, csrc/resample.hip (the byte-exact rule is libImaging/Resample.c's, restated in
 * tests/resample_ref.py): `Image.resize(size, filter)` of L and RGB images for the antialiased filters below - per axis a table
 * of (xmin, n) and n coefficients in 22-bit fixed point per output index, a horizontal pass into uint8, then a vertical pass,
 * each clamp((2^21 + sum pixel * k) >> 22, 0, 255) in 32-bit int - and the nearest resizes of the label side.                */
#define SFH_FILTER_BOX 4        /* Pillow's numbering of Image.BOX, BILINEAR, BICUBIC                                           */
#define SFH_FILTER_BILINEAR 2
#define SFH_FILTER_BICUBIC 3
#define SFH_NEAREST_PIL 0       /* Image.resize(.., NEAREST): a running fp64 sum x = a / 2, x += a with a = in / out            */
#define SFH_NEAREST_CV2 1       /* cv2.INTER_NEAREST: min(floor(i * (1 / (out / in))), in - 1)                                  */
#define SFH_RESAMPLE_MAX_TAPS 64   /* coefficients of one output index at most (bicubic: downscales up to 16x)                  */
#define SFH_RESAMPLE_MAX_ROWS 64   /* source rows of one tile's uint8 intermediate in LDS                                       */

/* SFH_RESAMPLE_MAX_TAPS, for callers that cannot read this header                                                            */
int sfh_resample_max_taps(void);
/* Host code, no device: the table of one axis.  bounds int32 (out, 2) = (xmin, n); coef int32 (out, ksize), row xx holding its
 * n coefficients then zeros; returns the row stride ksize = 2 ceil(support * max(in / out, 1)) + 1 (Pillow's), or -1 for
 * sizes <= 0, an unknown filter, a null pointer or cap < out * ksize (cap: the int32 elements `coef` has room for).         */
int sfh_resample_tab(int in, int out, int filter, int32_t* bounds, int32_t* coef, int cap);
/* Host code: output rows per tile for the vertical axis in -> out (16, 8, 4, 2 or 1: the largest whose source rows fit
 * SFH_RESAMPLE_MAX_ROWS); -1 for bad arguments or when an output index has more than SFH_RESAMPLE_MAX_TAPS taps.            */
int sfh_resample_tile_rows(int in, int out, int filter);
/* Host code: idx int32 (out) = the source index of every output index under `rule`; returns out, or -1 for sizes <= 0, an
 * unknown rule, a null pointer or cap < out.                                                                                */
int sfh_nearest_tab(int in, int out, int rule, int32_t* idx, int cap);

/* ONE launch, one workgroup per tile of tile_rows x 64 output pixels of one image, no atomics: src uint8 (B,Hs,Ws,C), C = 1 | 3
 * -> dst_u8 uint8 (B,Hd,Wd,C) and / or dst_f32 float32 (B,C,Hd,Wd) = byte / 255 (sfh_u8hwc_to_f32nchw's rule), whichever is not
 * NULL.  x* / y*: DEVICE copies of the tables of sfh_resample_tab for Ws -> Wd / Hs -> Hd with their row strides and the largest
 * n of the axis (x*taps); an axis whose sizes are equal is skipped and its table may be NULL; equal sizes on both axes give a
 * copy.  tile_rows: sfh_resample_tile_rows(Hs, Hd, filter).  -1 with nothing launched for null pointers, bad shapes and an
 * axis with more than SFH_RESAMPLE_MAX_TAPS taps.                                                                            */
int sfh_resample_u8(const uint8_t* src, uint8_t* dst_u8, float* dst_f32, int batch, int C, int Hs, int Ws, int Hd, int Wd,
                    const int32_t* xbounds, const int32_t* xcoef, int xstride, int xtaps, const int32_t* ybounds,
                    const int32_t* ycoef, int ystride, int ytaps, int tile_rows, void* stream);

/* ONE launch: nearest resize through two DEVICE index tables (sfh_nearest_tab): src (B,Hs,Ws,C) -> dst (B,Hd,Wd,C) of uint8
 * (elem_bytes 1, C = 1 | 3) or uint16 (elem_bytes 2, C = 3: the UV label).                                                   */
int sfh_resize_gather(const void* src, void* dst, int batch, int C, int elem_bytes, int Hs, int Ws, int Hd, int Wd,
                      const int32_t* yidx, const int32_t* xidx, void* stream);

/* 8- and 16-bit TIFF files (the UV labels) <-> device images, csrc/tiffdec.hip and csrc/tiffenc.hip with the core
 * csrc/tiff_core.h (the rule: outputs.decode_tiff / outputs.encode_tiff).  Admitted: classic TIFF, the first IFD, II and MM,
 * strips, chunky, FillOrder 1, unsigned samples of 8 or 16 bits, 1 (BlackIsZero) or 3 (RGB) per pixel, Compression 1 and 5 (TIFF
 * 6.0 LZW), Predictor 1 and 2, any RowsPerStrip.  Everything else is refused on the host before anything is launched: reasons
 * below 100 for a malformed or unfit file, from 100 on for a well-formed file that needs something not built.               */
#define SFH_TIFF_R_OK 0
#define SFH_TIFF_R_TRUNCATED 1        /* the bytes end inside the 8-byte header                                                */
#define SFH_TIFF_R_NOT_TIFF 2         /* no II / MM byte-order mark or a magic number other than 42 (43: SFH_TIFF_R_BIGTIFF)     */
#define SFH_TIFF_R_BAD_IFD 3          /* the first IFD reaches outside the file                                                */
#define SFH_TIFF_R_BAD_TAG 4          /* a tag whose type is not BYTE, SHORT or LONG, or whose array reaches outside the file    */
#define SFH_TIFF_R_STRIP 5            /* a strip that reaches outside the file                                                 */
#define SFH_TIFF_R_STRIP_TABLE 6      /* StripOffsets or StripByteCounts with another length than ceil(H / RowsPerStrip)       */
#define SFH_TIFF_R_MISSING_TAG 7      /* no ImageWidth, ImageLength, PhotometricInterpretation, StripOffsets or StripByteCounts */
#define SFH_TIFF_R_BAD_VALUE 8        /* a zero or absurd size, RowsPerStrip 0, a BitsPerSample count other than the samples'   */
#define SFH_TIFF_R_SIZE 11            /* width, height, channels or bits other than the decoder's                              */
#define SFH_TIFF_R_TOO_LONG 12        /* more bytes than the decoder's max_file_bytes                                          */
#define SFH_TIFF_R_BIGTIFF 100
#define SFH_TIFF_R_TILES 101
#define SFH_TIFF_R_PLANAR 102         /* PlanarConfiguration 2                                                                 */
#define SFH_TIFF_R_FILL_ORDER 103     /* FillOrder 2                                                                           */
#define SFH_TIFF_R_COMPRESSION 104    /* anything but 1 (none) and 5 (LZW)                                                     */
#define SFH_TIFF_R_PREDICTOR 105      /* anything but 1 and 2                                                                  */
#define SFH_TIFF_R_BIT_DEPTH 106      /* anything but 8 or 16 bits, or samples of different depths                              */
#define SFH_TIFF_R_SAMPLE_FORMAT 107  /* signed, float or undefined samples                                                    */
#define SFH_TIFF_R_SAMPLES 108        /* SamplesPerPixel other than 1 and 3                                                    */
#define SFH_TIFF_R_PHOTOMETRIC 109    /* palette images; anything but BlackIsZero for one sample and RGB for three              */
#define SFH_TIFF_R_OLD_LZW 110        /* the bit-reversed LZW of old writers (a strip that starts 00 01, libtiff's test)         */

/* The parse of one file (64 bytes).  file_pos, file_bytes, table_pos: filled by sfh_tiff_dec_stage only - where the file and its
 * strip table lie in the staging buffer.                                                                                     */
typedef struct sfh_tiff_info {
  int32_t width, height, channels, bits, compression, predictor, big_endian, rows_per_strip, nstrips, photometric;
  int32_t reason;
  int32_t file_pos, file_bytes, table_pos;
  int32_t reserved[2];
} sfh_tiff_info;

/* Host code, no device: the header and the first IFD of host_bytes[0, n) -> host_info, and the strip table as int32 records
 * {offset, byte count, first row, rows} in host_strips, as many as strip_cap admits (host_strips may be NULL with strip_cap 0);
 * host_info->nstrips counts all.  Every offset of the file is checked against n.  0, or -1 with host_info->reason =
 * SFH_TIFF_R_*.                                                                                                              */
int sfh_tiff_parse(const uint8_t* host_bytes, int64_t n, sfh_tiff_info* host_info, int32_t* host_strips, int64_t strip_cap);

/* bytes of the staging buffer and of the device scratch buffer (the decoded strips of every image, a status word per strip) of
 * a decoder of `batch` H x W x C files of `bits` bits of at most max_file_bytes; -1 for bad arguments and for buffers of 2 GiB
 * (staging) / 4 GiB (scratch) or more.                                                                                       */
int64_t sfh_tiff_dec_staging_bytes(int batch, int H, int W, int C, int bits, int64_t max_file_bytes);
int64_t sfh_tiff_dec_scratch_bytes(int batch, int H, int W, int C, int bits);

/* Host code, no device: parses `batch` files and packs the batch into host_staging - a 64-byte head {magic, batch, largest strip
 * count, used bytes}, the sfh_tiff_info of every file, every file's strip table, the files at 16-byte aligned positions - for
 * ONE copy to the device.  Returns the bytes used, or -1 with *host_reason = SFH_TIFF_R_* and *host_index = the file refused. */
int64_t sfh_tiff_dec_stage(const uint8_t* const* host_files, const int64_t* host_sizes, int batch, int H, int W, int C, int bits,
                           int64_t max_file_bytes, uint8_t* host_staging, int64_t staging_bytes, int32_t* host_reason,
                           int32_t* host_index);

/* `staged`, the device copy of host_staging (which is read here for its head only) -> out (B,H,W) or (B,H,W,3) of uint8 (bits 8)
 * or uint16 (bits 16); bgr != 0: the file's three samples reversed in memory.  status int32 (B): the OR of the TD_E_* bits of
 * the image's strips (csrc/tiff_core.h); such an image comes back as zeros.  Three launches: tiff_lzw_kernel, one wave per
 * (image, strip); tiff_verdict_kernel; tiff_unpredict_kernel (byte order, the predictor's prefix sum per row and channel, the
 * channel order).  No global atomics, no workgroup waits for another, no host synchronisation.                                */
int sfh_tiff_decode(const uint8_t* host_staging, const uint8_t* staged, int64_t staged_bytes, int batch, int H, int W, int C,
                    int bits, int bgr, int64_t max_file_bytes, uint8_t* scratch, int64_t scratch_bytes, void* out, int32_t* status,
                    void* stream);

/* The encoder.  compression 1 | 5, predictor 1 | 2, rows_per_strip 0 (max(1, 8192 / bytes per row), clamped to H) or 1 .. H.
 * sfh_tiff_strip_capacity: the most bytes a strip of n bytes encodes to (derived in csrc/tiff_core.h).  sfh_tiff_capacity: the
 * upper bound of one file, which sizes every buffer; -1 for bad arguments.                                                   */
int64_t sfh_tiff_strip_capacity(int64_t n, int compression);
int64_t sfh_tiff_capacity(int H, int W, int C, int bits, int compression, int rows_per_strip);
int64_t sfh_tiff_scratch_bytes(int batch, int H, int W, int C, int bits, int compression, int rows_per_strip);
/* ONE launch, one wave per (image, strip): images (B,H,W[,3]) of uint8 / uint16 (bgr != 0: the three samples are written in
 * reverse order) -> every strip, differenced and LZW-compressed, in its fixed-stride slot of `scratch`, and its byte count.   */
int sfh_tiff_encode(const void* images, int batch, int H, int W, int C, int bits, int bgr, int compression, int predictor,
                    int rows_per_strip, uint8_t* scratch, int64_t scratch_bytes, void* stream);
/* ONE launch, one workgroup per image: the scratch of sfh_tiff_encode (same arguments) -> the files, II: the 8-byte header, the
 * strips each on an even offset, the tag arrays, the IFD.  compact, out, offsets, sizes: as sfh_png_pack.                     */
int sfh_tiff_pack(const uint8_t* scratch, int64_t scratch_bytes, int batch, int H, int W, int C, int bits, int compression,
                  int predictor, int rows_per_strip, int compact, uint8_t* out, int64_t out_bytes, int64_t* offsets, int32_t* sizes,
                  void* stream);

/* -------------------------------------------------------------------------------------------------
 * Deterministic training mode: fixed-order slab sums (csrc/det_core.h states the arithmetic once).
 *
 * Every entry above that finishes a sum across workgroups with float atomics (their arrival order is free, so two runs
 * differ in the last bits) has a sibling NAME_det with the same arguments + (workspace, workspace_bytes) in front of the
 * stream, and a size query NAME_det_bytes that runs without a device (-1 for a refused geometry: the rule is the sibling's
 * own - entry, sibling and query read one plan, csrc/det_core.h - so the query answers -1 exactly where NAME and NAME_det
 * return SFH_E_ARG for the arguments the query sees.  For sfh_conv_wgrad_det_bytes that includes a source that does not
 * fit the frame (pad_top + xh > H, pad_left + xw > W, a negative pad), xh or xw <= 0, x_cs < N and x_cs % 4 != 0; for
 * sfh_conv_wgrad_s3_det_bytes a launch of 2^31 workgroups or more).  A sibling computes what
 * its entry computes, in two launches on the caller's stream:
 *
 *   store pass: the entry's kernel stores what it would have added into its own SLAB of the workspace.  Slab r is elements
 *     [r * E, (r + 1) * E) of the workspace, in the accumulator's type (float for raw, double for the fp64 accumulators);
 *     every element of every slab is written exactly once with a plain store (an empty share of the work stores zeros),
 *     so the workspace needs no memset and may be reused by the next call on the same stream.
 *   sum pass (sfh_det_reduce_f32 / _f64): dst[e] = (...((dst[e] + p_0[e]) + p_1[e]) + ...) + p_{R-1}[e] - the ascending
 *     chain over the R slabs, starting from what the destination held, in the accumulator's own precision.
 *
 *   entry                              slab r = the share of        R                                   E (layout)
 *   sfh_conv_wgrad_det                 pixel split r                split count of the launch           M * ksize^2 * N  [m][tap][n], n from 0
 *   sfh_conv_wgrad_s3_det              pixel split r                split count of the launch           M * ksize^2 * N  [m][tap][n], n from 0
 *   sfh_conv_grouped_wgrad_det         output tile r                tiles of 8 (stride 2: 4) x 16       C * 9 * cg       raw's own layout
 *   sfh_bn_stats_det, bn_bwd_reduce    reduction block r            min(1024, ceil(npix / 256))         2 * C            [row][c]
 *   sfh_colsum_det                     reduction block r            min(1024, ceil(npix / 256))         C
 *   sfh_outconv_bwd_det                block r of ppb pixels        ceil(npix / ppb)                    nc * cin + nc    [k][ci], then [k]
 *   sfh_avgpool_linear_bwd_det         frame r                      batch                               nout * C + nout  [j][c], then [j]
 *   sfh_train_losses_det               block r                      min(2048, ceil(npix / 256))         3
 *   sfh_uv_loss_det                    block r                      min(1024, ceil(B*C*H*W / 256))      1
 *   sfh_reproj_loss_det                block r of 64 frames         ceil(batch / 64)                    1   (the 64 frames added in frame order)
 *   sfh_homography_warp_bwd_theta_det  block (x, y): r = y * gx + x ceil(w / 256) * ceil(h / 4)         9 * batch        [b][k]
 *   (ppb = max(1024, 256 * ceil(floor(npix / 1024) / 256)).  The backward-filter slabs are compact: the sum pass places
 *   them at columns [n_off, n_off + N) of raw.)
 *
 * workspace_bytes >= NAME_det_bytes(...) = R * E * sizeof(element); a workspace that is NULL or smaller returns SFH_E_ARG
 * with nothing launched.  The library allocates nothing and keeps no pointer.  Same library build, device model, shapes and
 * operands -> the same bits, whatever else runs on the device; not across batch sizes or devices (the partition depends on
 * the geometry).  The one-pass forms (sfh_s2d_split_colsum, sfh_pool2_bwd_bn_reduce, sfh_outconv_bwd_bn,
 * sfh_conv_wgrad_c4_bn, sfh_bn_stats_partials, sfh_conv_desc.stats_partial) have no sibling: the mode takes their plain legs. */
/* dst[(e / ncol) * dst_row_stride + e % ncol] += sum over r < slabs of partial[r * slab_stride + e], e < elems, in the order
 * above.  elems % ncol == 0, slab_stride >= elems, dst_row_stride >= ncol.                                                 */
int sfh_det_reduce_f32(const float* partial, int64_t slabs, int64_t slab_stride, int64_t elems, int ncol, float* dst,
                       int64_t dst_row_stride, void* stream);
int sfh_det_reduce_f64(const double* partial, int64_t slabs, int64_t slab_stride, int64_t elems, int ncol, double* dst,
                       int64_t dst_row_stride, void* stream);
int64_t sfh_conv_wgrad_det_bytes(int M, int x_cs, int xh, int xw, int N, int pad_top, int pad_left, int batch, int H, int W,
                                 int ksize);
int sfh_conv_wgrad_det(const float* dz, int dz_cs, int M, const float* x, int x_cs, int xh, int xw, int N, int pad_top,
                       int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n, int n_off, void* workspace,
                       long long workspace_bytes, void* stream);
int64_t sfh_conv_wgrad_s3_det_bytes(int M, int N, int batch, int H, int W, int ksize);
int sfh_conv_wgrad_s3_det(const void* dz_s3, int M, const void* x_s3, int x_channels, int xh, int xw, int N, int pad_top,
                          int pad_left, int batch, int H, int W, int ksize, float* raw, int raw_n, int n_off, int fmt,
                          void* workspace, long long workspace_bytes, void* stream);
int64_t sfh_conv_grouped_wgrad_det_bytes(int batch, int H, int W, int groups, int cg, int stride);
int sfh_conv_grouped_wgrad_det(const float* dz, const float* src, float* raw, int batch, int H, int W, int groups, int cg,
                               int stride, void* workspace, long long workspace_bytes, void* stream);
int64_t sfh_bn_stats_det_bytes(int64_t npix, int C);
int sfh_bn_stats_det(const float* z, int64_t npix, int C, double* acc, void* workspace, long long workspace_bytes, void* stream);
int64_t sfh_bn_bwd_reduce_det_bytes(int64_t npix, int C);
int sfh_bn_bwd_reduce_det(const float* dy, const float* y, const float* z, const float* mean_invstd, const float* gamma,
                          const float* beta, int relu, int64_t npix, int C, double* acc, void* workspace,
                          long long workspace_bytes, void* stream);
int64_t sfh_colsum_det_bytes(int64_t npix, int C);
int sfh_colsum_det(const float* x, int64_t npix, int C, int cs, double* acc, void* workspace, long long workspace_bytes,
                   void* stream);
int64_t sfh_outconv_bwd_det_bytes(int cin, int nc, int batch, int H, int W);
int sfh_outconv_bwd_det(const float* x, int cin, const float* w, const float* dlogits_nchw, int nc, int batch, int H, int W,
                        float* dx, double* acc_w, double* acc_b, void* workspace, long long workspace_bytes, void* stream);
int64_t sfh_avgpool_linear_bwd_det_bytes(int batch, int C, int nout);
int sfh_avgpool_linear_bwd_det(const float* x, const float* w, const float* dout, int batch, int H, int W, int C, int nout,
                               float* dx, double* acc_w, double* acc_b, void* workspace, long long workspace_bytes,
                               void* stream);
int64_t sfh_train_losses_det_bytes(int batch, int H, int W);
int sfh_train_losses_det(const float* logits_nchw, const int64_t* gt_mask, const float* weight, const float* warp_mask, int nc,
                         int batch, int H, int W, float lambda_seg, float lambda_rec, int rec_mse, float lambda_cons,
                         int focal_flags, float* dlogits_nchw, float* dwarp, double* loss3, void* workspace,
                         long long workspace_bytes, void* stream);
int64_t sfh_reproj_loss_det_bytes(int batch);
int sfh_reproj_loss_det(const float* poi, const float* gt_poi, const float* nonzeros, const float* num_nonzero, int batch,
                        int npts, float lambda, float* dpoi, double* loss, void* workspace, long long workspace_bytes,
                        void* stream);
int64_t sfh_uv_loss_det_bytes(int batch, int C, int H, int W);
int sfh_uv_loss_det(const float* uv, const float* gt_uv, const float* weight, int nweights, int batch, int C, int H, int W,
                    float lambda, int mse, float* duv, double* loss, void* workspace, long long workspace_bytes, void* stream);
int64_t sfh_homography_warp_bwd_theta_det_bytes(int batch, int h, int w);
int sfh_homography_warp_bwd_theta_det(const float* theta, const float* tmpl, int64_t tmpl_bstride, int ht, int wt, int batch,
                                      int h, int w, const float* dout, double* acc, void* workspace,
                                      long long workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Homography refinement against the segmentation (csrc/refine.hip): direct alignment of the court template to the UNet's
 * class probabilities, a few damped Gauss-Newton steps per frame, coarse to fine.  THE RULE, stated here once; the kernels
 * and the numpy restatement tests/refine_ref.py follow it.
 *
 * Planes.  For a class count nc in 2..8 the foreground planes are c = 1 .. nc-1; plane c is channel c-1 of a channel-last
 *   tensor of CP channels, CP = 4 for nc <= 5 and 8 otherwise; the pad channels are 0.
 *   Template plane at level f:  Tf[c] = (count over the f x f block of (id == c)) / f^2 in fp32, id = rint(fl32(v * nc)) of the
 *     template (N,1,ht,wt) valued k/nc.
 *   Evidence plane at level f:  Ef[c] = (sum over the f x f block, row by row, of softmax(logits)[c]) / f^2, all fp32;
 *     softmax(l)[c] = e_c / (e_0 + e_1 + ... + e_{nc-1}) in that order, e_k = expf(l_k - max l), one IEEE division.
 *   f must divide ht, wt, hl and wl; otherwise the call is refused and nothing is launched.
 *   Background is not a plane: a tap outside the template reads 0 in every plane, and 0 is what background is.
 * Coordinates.  theta addresses the model's warp grid (H, W) (Reconstructor.warp's).  Evidence column j of level f over
 *   logits of width wl has xn = fmaf(ax, j, cx), ax = 2 f W / (wl (W-1)), cx = (f W / wl - 1) / (W-1) - 1, both evaluated in
 *   fp64 on the host and rounded once to fp32 (sfh_refine_axis): the centre of the averaged pixel in create_meshgrid's
 *   convention.  Rows alike with H and hl.  With f = 1 and wl = W this grid is the warp's own up to rounding; it is NOT
 *   required to be bit-equal to the warp kernels' (i / (W-1) - 0.5) * 2.
 *   Then X, Y, Z, s, u = s X, v = s Y exactly as the warp (s = 1 / (Z + 1e-8) where |Z| > 1e-8, else 1), px = fma(u + 1,
 *   (wt/f) / 2, -0.5), py alike with ht/f; bilinear taps with zero padding at (floor px, floor py).  The weights wx1 = px -
 *   floor px, wx0 = 1 - wx1 (wy alike), the value ((t00 wy0 wx0 + t01 wy0 wx1) + t10 wy1 wx0) + t11 wy1 wx1 and the tap
 *   differences duf = wy0 (t01 - t00) + wy1 (t11 - t10), dvf = wx0 (t10 - t00) + wx1 (t11 - t01) are fp32, every operation
 *   rounded; everything behind them is fp64 (the staging of sfh_homography_warp_bwd_theta).
 * Cost and normal equations.  r_c(p) = value_c(p) - Ef[c](p), cost = sum_p sum_c r_c^2.  theta[8] is held fixed; per pixel
 *   J_c = du_c a + dv_c b with du_c = duf_c (wt/f) / 2, dv_c = dvf_c (ht/f) / 2, a = du/dtheta = (s xn, s yn, s, 0, 0, 0, gu xn,
 *   gu yn), b = dv/dtheta = (0, 0, 0, s xn, s yn, s, gv xn, gv yn), gu = -X s^2, gv = -Y s^2 (0 where |Z| <= 1e-8).
 *   SFH_REFINE_SUMS = 45 sums per frame, the layout of sfh_prep_fit's step: the upper triangle of J^T J row by row
 *   (36), J^T r (8), the cost (1).
 * Step (Levenberg-Marquardt, the rule of sfh_prep_fit).  Solve (J^T J + lambda diag(J^T J)) delta = -J^T r by Cholesky in
 *   fp64 - the operation order is stated once, in csrc/chol8.h, for this step, sfh_prep_fit's and sfh_uvfit_step's.  The
 *   candidate is fl32(theta_k + delta_k), k < 8 (the accepted theta itself when a pivot is not > 0).  It is accepted
 *   iff every pivot was > 0 and cost(candidate) < cost(accepted) - a NaN cost rejects.  Accepted: lambda / 10; rejected:
 *   lambda * 10; lambda = 1e-3 at the start of every level.  Schedule: the levels from coarse to fine, `iters` steps each.
 *
 * One level = sfh_refine_accumulate(theta) + sfh_refine_step(first = 1), then `iters` times sfh_refine_accumulate(candidate)
 * + sfh_refine_step(first = 0), the last of them with last = 1.  The library allocates nothing and keeps no pointer. */
#define SFH_REFINE_SUMS 45
/* a[0] = ax, a[1] = cx of an axis of n warp-grid points seen through nl logits at level f (HOST pointer; no device call) */
int sfh_refine_axis(int f, int n, int nl, float* a);
/* tmpl (n,1,ht,wt) float -> planes (n, ht/f, wt/f, CP) float */
int sfh_refine_template_planes(const float* tmpl, int n, int ht, int wt, int nc, int f, float* planes, void* stream);
/* logits (batch,nc,hl,wl) float NCHW -> planes (batch, hl/f, wl/f, CP) float */
int sfh_refine_evidence_planes(const float* logits, int batch, int nc, int hl, int wl, int f, float* planes, void* stream);
/* bytes of the partial sums of sfh_refine_accumulate for an evidence grid of h x w (the finest level's serves every coarser
 * one): ceil(w / 64) * ceil(h / 64) * batch * 45 doubles; -1 for batch outside 1..65535 or h, w < 1 */
int64_t sfh_refine_workspace_bytes(int batch, int h, int w);
/* The 45 sums of theta (batch,9) per workgroup: tplanes (n, ht/f, wt/f, CP) with tplanes_bstride floats from frame to frame (0:
 * one template for every frame; else a multiple of 4), eplanes (batch, hl/f, wl/f, CP), both 16-byte aligned (they are read with
 * 16-byte loads; anything else returns SFH_E_ARG); H, W the warp grid.  Workgroup (x, y) covers 64 columns x
 * 64 rows of the evidence grid and stores its sums of frame b at workspace[((y * gx + x) * batch + b) * 45 + e], one plain
 * store per sum (wave shuffle, then LDS; no atomics).  A workspace that is NULL or short returns SFH_E_ARG, nothing launched. */
int sfh_refine_accumulate(const float* theta, const float* tplanes, int64_t tplanes_bstride, int ht, int wt,
                          const float* eplanes, int batch, int nc, int hl, int wl, int H, int W, int f, void* workspace,
                          long long workspace_bytes, void* stream);
/* One wave per frame: sums the `slabs` partials [slab][batch][45] of theta_eval (batch,9) in ascending slab order from 0 and
 * applies the step rule against the per-frame state: theta_acc (batch,9) float, sums_acc (batch,45) double, lambda (batch)
 * double, pivots_ok (batch) int32.  first != 0: theta_eval is adopted as the level's start, lambda = 1e-3,
 * accepted[b * nlevels + level] = 0 and cost[(b * nlevels + level) * 2] = its cost.  Otherwise accept / reject as above
 * (accepted is incremented).  Every call writes cost[(b * nlevels + level) * 2 + 1] = the accepted cost and theta_next
 * (batch,9): the next candidate, or the accepted theta when last != 0.  theta_next may be theta_eval. */
int sfh_refine_step(const double* partial, int64_t slabs, int batch, int first, int last, const float* theta_eval,
                    float* theta_acc, double* sums_acc, double* lambda, int32_t* pivots_ok, float* theta_next, double* cost,
                    int32_t* accepted, int level, int nlevels, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Registration metrics (csrc/metrics.hip): how good a homography is against a labelled one, per frame, in the terms the
 * sports-field registration literature reports - per-class segmentation IoU, IoU_part, IoU_whole, the projection error on the
 * court and the reprojection error in the frame.  THE RULES, stated here once; the kernels and the numpy restatement
 * tests/metrics_ref.py follow them.  The reference project has no counterpart.  theta maps the normalised frame to the
 * normalised court (Reconstructor.warp's matrix); every entry launches on `stream`, synchronises nothing, reads nothing back,
 * allocates nothing and OVERWRITES its outputs (the caller zero-fills the sticky flag only).
 *
 * Matrix of a theta.  m = the nine fp32 entries converted to fp64.  adj(theta) is the fp64 adjugate, the nine expressions of
 *   inverse_h33 (csrc/warp_coords.h) WITHOUT the multiplication by 1 / det:
 *     a0 = m4 m8 - m5 m7   a1 = m2 m7 - m1 m8   a2 = m1 m5 - m2 m4
 *     a3 = m5 m6 - m3 m8   a4 = m0 m8 - m2 m6   a5 = m2 m3 - m0 m5
 *     a6 = m3 m7 - m4 m6   a7 = m1 m6 - m0 m7   a8 = m0 m4 - m1 m3          det = (m0 a0 + m1 a3) + m2 a6
 *   every product and difference individually rounded.  A theta is USABLE iff det is finite and != 0 (a non-finite entry
 *   makes det non-finite).  Where a theta is not usable, theta and adj(theta) both read as the zero matrix in everything below.
 * Predicate.  in(M, q) for a 3 x 3 fp64 matrix M (row-major) and q = (a, b, c):  X = (M0 a + M1 b) + M2 c, Y and W likewise
 *   with rows 1 and 2, every operation individually rounded;  in  iff  |W| > 0  and  |X| <= |W|  and  |Y| <= |W|.  A NaN
 *   anywhere makes it false; the zero matrix makes it false.  The predicate is BLIND TO THE SIGN OF W, on purpose: the warp
 *   kernel divides by Z whatever its sign, so the predicate selects exactly the points that the model's own warp would draw
 *   into the square, the ones behind the horizon included.
 *
 * sfh_metrics_confusion.  out int64 (B,nc,nc): out[b][g][p] = the number of pixels of frame b with ground-truth class g and
 *   predicted class p; nc 2 .. 8, H * W < 2^31.  gt int64 (B,H,W); a pixel whose gt is -100 is counted nowhere.  pred by
 *   pred_kind: 0 int32 ids (B,H,W); 1 uint8 ids (B,H,W); 2 fp32 logits NCHW (B,nc,H,W), the class by the argmax rule stated
 *   above sfh_outconv_fwd (ties, NaN and +inf as stated there); 3 fp32 (B,H,W) warp mask valued k / nc, class =
 *   trunc(fl32(v * fl32(nc))), the rule of sfh_eval_batch, valid iff -1 < fl32(v * fl32(nc)) < nc.  *flag (caller-zeroed,
 *   sticky): bit 1 is ORed for a gt id outside [0, nc) other than -100, bit 2 for a predicted class outside [0, nc) (a
 *   non-finite kind-3 value included; at a pixel whose gt is -100 too); a pixel with either defect is counted nowhere.
 *   Two launches: a clear of out, then the count - per wave one step per DISTINCT (g, p) key present (ballot, popcount; lane k
 *   of a wave keeps the count of key k in a register), per workgroup one LDS word per key, across workgroups 64-bit integer
 *   atomic adds onto the cleared output (integer addition: the same bits in any order).
 *
 * sfh_metrics_region.  out int64 (B,3) = [nA, nB, nAB]: the canvas pixels where in(A, q), in(B, q), and both hold.  The
 *   canvas is the court raster wc x hc (both >= 2) extended by mx, my >= 0 pixels on each side: x = -mx .. wc-1+mx, y = -my ..
 *   hc-1+my, fewer than 2^31 pixels, wc, hc, mx, my <= 2^20.  Pixel (x, y) is the homogeneous court point
 *     q = ((2x - (wc-1)) (hc-1),  (2y - (hc-1)) (wc-1),  (wc-1) (hc-1)),   exact integers (below 2^53) converted to fp64:
 *   create_meshgrid's (i / (n-1) - 0.5) * 2 raster of sfh_topview_render without its division.
 *     mode 0 (part):  A = adj(theta_pred), B = adj(theta_gt) - the court pixels from which the frame is visible under each
 *       theta (use mx = my = 0);  IoU_part = nAB / (nA + nB - nAB).
 *     mode 1 (whole): A = theta_gt * adj(theta_pred), entry (i, j) = (g[i][0] a[0][j] + g[i][1] a[1][j]) + g[i][2] a[2][j] in
 *       fp64, and the zero matrix unless both thetas are usable; B = the identity - the image of the court rectangle under
 *       theta_pred * theta_gt^-1 against the rectangle itself;  IoU_whole by the same formula.  The margin bounds what is
 *       counted of the image outside the court: that is part of the rule.
 *   A theta that is not usable gives 0 for the counts that depend on it.  The matrices are formed once per workgroup.
 *
 * sfh_metrics_points.  out double (B,4) = [reproj_mean, n_pts, proj_mean, n_lattice], all fp64, one wave per frame.
 *   Reprojection (frame): court point n = (u, v) of court_pts double (N,2), normalised court coordinates shared by the
 *     batch, is counted iff in(adj(theta_gt), (u, v, 1)) - it is visible in the ground truth.  With (Xg, Yg, Wg) and (Xp, Yp,
 *     Wp) its images under adj(theta_gt) and adj(theta_pred) by the predicate's expressions, dx = (Xp / Wp - Xg / Wg)
 *     frame_sx, dy alike with frame_sy, error = sqrt(dx dx + dy dy).  frame_sx, frame_sy: pixels per normalised frame unit
 *     (target_w / 2, target_h / 2).
 *   Projection (court): the frame lattice x_k = -1 + (2k + 1) / gx, k = 0 .. gx-1, y_l alike with gy (1 <= gx, gy <= 4096).
 *     A lattice point is counted iff in(theta_gt, (x, y, 1)) - it lies on the court.  Its error is the same expression with
 *     theta_gt and theta_pred in place of the adjugates and court_sx, court_sy (court units per normalised court unit, e.g.
 *     metres / 2) in place of the frame's.
 *   Lane l sums the errors of its points l, l + 64, ... in that order, the lanes are added by the fixed shuffle tree of
 *   sfh_eval_batch; mean = sum / n, so 0 / 0 is written as NaN (no counted point).  A theta_pred that is not usable, or whose
 *   Wp is 0 at a counted point, yields a non-finite mean: the caller counts such frames instead of hiding them.           */
int sfh_metrics_confusion(const void* pred, int pred_kind, const int64_t* gt, int nc, int batch, int H, int W, int64_t* out,
                          uint32_t* flag, void* stream);
int sfh_metrics_region(const float* theta_pred, const float* theta_gt, int batch, int mode, int wc, int hc, int mx, int my,
                       int64_t* out, void* stream);
int sfh_metrics_points(const float* theta_pred, const float* theta_gt, int batch, const double* court_pts, int npts, int gx,
                       int gy, double frame_sx, double frame_sy, double court_sx, double court_sy, double* out, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Homography fit from the UV head (csrc/uvfit.hip).  The UV map is a dense set of frame -> court correspondences, one per
 * court pixel in view; a homography fitted to them is an estimate of theta that owes nothing to the STN's nine regressed
 * numbers, with a quality figure in court pixels.  Iteratively reweighted least squares: every pass is one linear 8 x 8 solve.
 * THE RULE, stated here once; the kernels and the numpy restatement tests/uvfit_ref.py follow it.  The reference project has
 * no counterpart.
 *
 * Inputs per frame.  uv (2,h,w) fp32 NCHW (the head's output, or a label through preparation.split_uv); optionally logits
 *   (nc,h,w) and a start theta0 (9) fp32.  (wt, ht): the court raster the UV labels were rendered from (LabelMaker's court_ids
 *   size; it need not be the court template's).  (W, H): the warp grid theta addresses.
 * Gate.  Pixel (i, j) counts iff u > u_min and v > v_min, u_min = 0.5 / wt and v_min = 0.5 / ht evaluated in fp64 on the host
 *   and rounded once to fp32 (a NaN fails; in the labels 0 means "no court here") and, with logits, its class is not 0 by the
 *   argmax rule stated above sfh_outconv_fwd (strict > scan, first maximum).
 * Coordinates.  Frame: x = fmaf(ax, j, cx0), y = fmaf(ay, i, cy0) in fp32 with (ax, cx0) = sfh_refine_axis(1, W, w) and (ay,
 *   cy0) = sfh_refine_axis(1, H, h): the pixel centres on the grid theta addresses; then widened to fp64.  Court: cx = 2 u - kx,
 *   cy = 2 v - ky in fp64 (u, v widened; 2 u is exact), kx = 1 + 1 / wt, ky = 1 + 1 / ht evaluated in fp64 on the host:
 *   generate_uv_template gives court column c the value (c + 1) / wt, and the warp's tap rule is px = (cx + 1) wt / 2 - 0.5.
 * Residual under a theta (its nine fp32 entries widened; theta[8] is used as read):  X = (t0 x + t1 y) + t2, Y and Wd alike
 *   with rows 1 and 2;  ex = (X / Wd - cx) (wt / 2), ey = (Y / Wd - cy) (ht / 2), r2 = ex ex + ey ey, all fp64, every operation
 *   individually rounded (no contraction).
 * Weight.  c = 1 + r2 / d2 with d2 = delta delta (delta in court pixels), omega = (1 / c) / (Wd Wd): the Cauchy weight times the
 *   factor that turns the algebraic residual into the geometric one to first order.  omega = 0 where |Wd| <= 1e-8 or r2 is not
 *   finite.  Without a theta (first pass, no theta0): omega = 1.  A pixel with omega == 0 adds nothing to the moments.
 * Sums.  SFH_UVFIT_SUMS = 27 per frame, fp64, over the gated pixels; with wx = omega x, wy = omega y, m = {wx x, wx y, wy y,
 *   wx, wy, omega} (the weighted {x^2, xy, y^2, x, y, 1}) and q = cx cx + cy cy:
 *     0..5    m[0..5]                    6..10   cx m[0..4]              11..15  cy m[0..4]
 *     16..18  q m[0..2]                  19, 20  omega cx, omega cy      21, 22  q wx, q wy          23  omega q
 *     24      n: the gated pixels        25      the gated pixels with r2 <= d2
 *     26      sum of r2 / c over the gated pixels with omega != 0         (25 and 26 are 0 without a theta)
 * Assembly.  With theta[8] fixed at 1 a pixel gives the rows r1 = [x, y, 1, 0, 0, 0, -cx x, -cx y | cx] and r2 = [0, 0, 0, x,
 *   y, 1, -cy x, -cy y | cy];  A = sum omega (r1^T r1 + r2^T r2) and g = sum omega (r1^T cx + r2^T cy) are, by sum index,
 *     A[0..2][0..2] = A[3..5][3..5] = [[0, 1, 3], [1, 2, 4], [3, 4, 5]]      A[0..2][3..5] = 0
 *     A[0..2][6] = -[6, 7, 9]     A[0..2][7] = -[7, 8, 10]     A[3..5][6] = -[11, 12, 14]     A[3..5][7] = -[12, 13, 15]
 *     A[6][6] = 16   A[6][7] = 17   A[7][7] = 18   (symmetric)              g = [9, 10, 19, 14, 15, 20, -21, -22]
 *   and the algebraic cost of an h is  (h^T A h - 2 h^T g) + S23,  h^T A h = sum_i h_i (sum_k A[i][k] h_k), both sums ascending.
 * Step.  A h = g by Cholesky in fp64, the operation order of csrc/chol8.h; no damping, no accept / reject: each pass is a
 *   linear solve.  theta_next = (fl32(h_0) .. fl32(h_7), 1).  The solve FAILS when a pivot is not > 0, when n < 4 or when one of
 *   the 27 sums is not finite; a frame whose solve failed is DEAD from then on (status < pass says so).  A frame that fails or
 *   is dead gets theta_next = theta_eval: the last solved theta, else theta0, else nine NaNs (no theta_eval).  status = the
 *   number of solves that succeeded.
 * Schedule.  sfh_uvfit_accumulate(theta0 or NULL) + sfh_uvfit_step(pass 0), then `iters` times accumulate(candidate) + step
 *   (pass 1 ..), then one accumulate + step with last = 1, which solves nothing, passes theta_eval through and writes the
 *   statistics of that final theta: 2 (iters + 2) launches on the caller's stream, no synchronisation, no read-back.  Every
 *   output is overwritten; the library allocates nothing and keeps no pointer. */
#define SFH_UVFIT_SUMS 27
/* bytes of the partial sums of sfh_uvfit_accumulate: ceil(w / 64) * ceil(h / 64) * batch * 27 doubles; -1 for batch outside
 * 1..65535 or h, w < 2 */
int64_t sfh_uvfit_workspace_bytes(int batch, int h, int w);
/* The 27 sums per workgroup: uv (batch,2,h,w), logits (batch,nc,h,w) or NULL (then nc is not read; else 2..8), theta (batch,9)
 * or NULL.  Workgroup (x, y) covers 64 columns x 64 rows of the grid (any h, w >= 2; a tile may be partly outside) and stores
 * its sums of frame b at workspace[((y * gx + x) * batch + b) * 27 + e], one plain store per sum (wave shuffle, then LDS; no
 * atomics: the same bits every run).  H, W, wt, ht >= 2, delta > 0; a workspace that is NULL or short returns SFH_E_ARG, as
 * every refusal does, with nothing launched. */
int sfh_uvfit_accumulate(const float* uv, const float* logits, int nc, const float* theta, int batch, int h, int w, int H, int W,
                         int wt, int ht, float u_min, float v_min, double kx, double ky, double delta, void* workspace,
                         long long workspace_bytes, void* stream);
/* One wave per frame: sums the `slabs` partials [slab][batch][27] in ascending slab order from 0, assembles, solves and applies
 * the dead-frame rule.  pass: the number of step calls of this schedule before this one (0: status is not read); last != 0:
 * nothing is solved.  theta_eval (batch,9): the theta the partials were accumulated under, NULL only on pass 0 without a
 * theta0; theta_next (batch,9) may be theta_eval.  status (batch) int32.  stats (batch,4) double = [n, inliers (S25),
 * sqrt(S26 / n), the algebraic cost of theta_next's first eight entries], written on every call. */
int sfh_uvfit_step(const double* partial, int64_t slabs, int batch, int pass, int last, const float* theta_eval,
                   float* theta_next, int32_t* status, double* stats, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Inter-frame homography tracking (csrc/track.hip).  M_t is the homography under which frame t lines up with frame t - 1,
 * estimated from the pixels themselves by direct photometric alignment - coarse to fine, a few robust Levenberg-Marquardt
 * steps per pair - and theta is carried across it: theta_t = theta_{t-1} M_t (theta maps the normalised frame to the
 * normalised court, Reconstructor.warp's matrix; M maps the normalised coordinates of the CURRENT frame of a pair to those of
 * its PREVIOUS frame).  THE RULE, stated here once; the kernels and the numpy restatement tests/track_ref.py follow it.  The
 * reference project has no counterpart.
 *
 * Planes.  Luma of a pixel: y = (19595 r + 38470 g + 7471 b + 32768) >> 16 (csrc/ycc.h, the JPEG encoder's Y); frames are
 *   uint8 (B,H,W,3), channel 0 is r, or with bgr != 0 channel 2 is.  Plane of level f:  P_f[I][J] = fl32(S) / fl32(255 f f),
 *   S the exact integer sum of y over the f x f block, one IEEE fp32 division; a scalar plane (B, H/f, W/f).  f in 1..16
 *   must divide H and W (and an alignment needs planes of at least 2 x 2 pixels); otherwise the call is refused and nothing
 *   is launched.
 * Coordinates.  Plane column J of level f has xn = fmaf(ax, J, cx), (ax, cx) = sfh_refine_axis(f, W, W): the centre of the
 *   averaged block on the full-resolution grid 2 j / (W-1) - 1.  Rows alike with H.  X, Y, Z, s, u = s X, v = s Y exactly as
 *   the warp and the refinement form them from M (fp32, every operation rounded; s = 1 / (Z + 1e-8) where |Z| > 1e-8, else the
 *   pixel is not counted).  Back to the previous frame's plane:  px = fmaf(u + 1, kx, -ox),  kx = (W-1) / (2 f),  ox = (f-1) /
 *   (2 f), evaluated in fp64 on the host and rounded once to fp32 (sfh_track_axis; csrc/track_core.h); py alike with H.  Under
 *   the identity px = J up to rounding, at every level.  (The refinement's (u + 1) wt / 2 - 0.5 is NOT this: it mixes the warp
 *   grid with a template raster.)
 * Residual.  Bilinear taps at (x0, y0) = (floor px, floor py) of the previous frame's plane.  A pixel COUNTS iff |Z| > 1e-8
 *   and all four taps lie inside the plane: 0 <= x0, x0 + 1 <= wl - 1, 0 <= y0, y0 + 1 <= hl - 1 (fp32 comparisons; a NaN
 *   fails).  No zero padding: outside the previous frame there is no evidence.  The weights wx1 = px - x0, wx0 = 1 - wx1 (wy
 *   alike), the value ((t00 wy0 wx0 + t01 wy0 wx1) + t10 wy1 wx0) + t11 wy1 wx1 and the tap differences duf = wy0 (t01 - t00) +
 *   wy1 (t11 - t10), dvf = wx0 (t10 - t00) + wx1 (t11 - t01) are fp32, operation for operation as the refinement states them;
 *   everything behind them is fp64.  r = value - P_cur[I][J].
 * Robust weight and cost (Geman-McClure).  q = r r / d2 with d2 = delta delta formed on the host, c = 1 + q, ic = 1 / c,
 *   rho = (r r) ic, omega = ic ic: two fp64 divisions, no transcendental function.  du = duf kx, dv = dvf ky (the fp32 kx, ky
 *   widened).  With a = (s xn, s yn, s, 0, 0, 0, gu xn, gu yn), b = (0, 0, 0, s xn, s yn, s, gv xn, gv yn), gu = -(X s) s, gv =
 *   -(Y s) s, all fp64 from the widened fp32 values:  J_k = du a_k (k = 0..2),  dv b_k (k = 3..5),  du a_k + dv b_k (k = 6, 7).
 *   SFH_TRACK_SUMS = 46 sums per pair over the counted pixels:  the upper triangle of sum (omega J_i) J_j row by row (36),
 *   sum (omega J_i) r (8), sum rho (index 44), n = the counted pixels (index 45; exact as a double).
 * Step.  M[8] is held as given (sfh_amd.track starts it at 1).  Solve (A + lambda diag A) d = -g by csrc/chol8.h; the
 *   candidate is fl32(M_k + d_k), k < 8 (the accepted M itself when a pivot is not > 0).  It is accepted iff every pivot was
 *   > 0, n_cand >= nmin, and cost_cand / n_cand < cost_acc / n_acc - two fp64 divisions; a NaN rejects.  The MEAN is compared
 *   because the overlap changes with M: a plain sum would reward sliding the frames apart.  lambda = 1e-3 at the start of
 *   every level, / 10 on accept, * 10 on reject.  nmin = ceil(min_overlap hl wl) per level, from the host.  A pair whose first
 *   evaluation at a level has n < nmin or a sum that is not finite is DEAD from then on: it keeps its last accepted M (the
 *   start of the schedule if there is none), later steps change nothing of it.  ok = 1 iff the pair is not dead, the accepted
 *   M is finite and (max_cost <= 0 or the accepted mean cost <= max_cost): the cut / failure flag, with no read-back.
 * Schedule per level.  sfh_track_accumulate(M) + sfh_track_step(first = 1), then `iters` times sfh_track_accumulate(
 *   candidate) + sfh_track_step(first = 0), the last of them with last = 1.  No synchronisation.
 * Carrying theta (sfh_track_propagate).  theta (F,9), optional score (F) with max_score, M (F,9) and link (F) int32: entry t
 *   belongs to the pair (t - 1, t), entry 0 is not read.  Frame t is GOOD iff theta_t is usable (det of its fp64 copy finite
 *   and != 0, the expressions stated above sfh_metrics_region) and, with a score array, score_t <= max_score (a NaN fails).
 *   Good: the output bits are the input's, source[t] = t.  Bad: walk back to the nearest good k < t with t - k <= max_gap and
 *   every link[k+1 .. t] != 0, walk forward alike (link[t+1 .. k]); the nearer anchor is taken, a tie goes back.  Back: P =
 *   theta_k, then P = P M_j for j = k+1 .. t ascending.  Forward: P = theta_k, then P = P adj(M_j) for j = k .. t+1
 *   descending (adj: the nine expressions above sfh_metrics_region).  Products in fp64, entry (i, j) = (p[i][0] m[0][j] +
 *   p[i][1] m[1][j]) + p[i][2] m[2][j], every operation rounded.  Output fl32(P_i / P_8), entry 8 = 1, source[t] = k.  No
 *   anchor, or a P_8 that is zero or not finite: nine NaNs, source[t] = -1.  One thread per frame, O(max_gap) work each.
 *
 * Every entry launches on the caller's stream, allocates nothing, keeps no pointer and overwrites its outputs; every refusal
 * returns SFH_E_ARG before anything is launched. */
#define SFH_TRACK_SUMS 46
/* a[0] = kx, a[1] = ox of an axis of n frame pixels at level f (HOST pointer; no device call) */
int sfh_track_axis(int f, int n, float* a);
/* frames (batch,H,W,3) uint8 -> planes (batch, H/f, W/f) float */
int sfh_track_planes(const uint8_t* frames, int batch, int H, int W, int f, int bgr, float* planes, void* stream);
/* bytes of the partial sums of sfh_track_accumulate for planes of h x w (the finest level's serves every coarser one):
 * ceil(w / 64) * ceil(h / 64) * pairs * 46 doubles; -1 for pairs outside 1..65535 or h, w < 2 */
int64_t sfh_track_workspace_bytes(int pairs, int h, int w);
/* The 46 sums of M (pairs,9) per workgroup.  planes (nframes, H/f, W/f) of level f; ia, ib (pairs) int32 DEVICE arrays: pair
 * p aligns the current frame ib[p] with the previous frame ia[p] (a pair with an index outside [0, nframes) counts no pixel).
 * Workgroup (x, y) covers 64 columns x 64 rows of the current plane, a lane per column, and stores its sums of pair p at
 * workspace[((y * gx + x) * pairs + p) * 46 + e], one plain store per sum (wave shuffle, then LDS; no atomics).  delta > 0.
 * A workspace that is NULL or short is refused. */
int sfh_track_accumulate(const float* M, const float* planes, int nframes, const int32_t* ia, const int32_t* ib, int pairs,
                         int H, int W, int f, double delta, void* workspace, long long workspace_bytes, void* stream);
/* One wave per pair: sums the `slabs` partials [slab][pairs][46] of M_eval (pairs,9) in ascending slab order from 0 and
 * applies the step rule against the per-pair state: M_acc (pairs,9) float, sums_acc (pairs,46) double, lambda (pairs) double,
 * pivots_ok (pairs) int32, dead (pairs) int32.  first != 0: M_eval is adopted as the level's start, lambda = 1e-3,
 * accepted[p * nlevels + level] = 0, stats[(p * nlevels + level) * 3] = its mean cost, and the dead rule is applied (dead is
 * not read when level == 0).  Otherwise accept / reject as above.  Every call writes stats[(p * nlevels + level) * 3 + 1] =
 * the accepted mean cost (cost / n: NaN for n = 0), [.. + 2] = the accepted n, ok (pairs) int32 as if the schedule ended
 * here, and M_next (pairs,9): the next candidate, or the accepted M when last != 0 or the pair is dead.  M_next may be
 * M_eval.  nmin: a whole number as a double. */
int sfh_track_step(const double* partial, int64_t slabs, int pairs, int first, int last, const float* M_eval, float* M_acc,
                   double* sums_acc, double* lambda, int32_t* pivots_ok, int32_t* dead, float* M_next, double* stats,
                   int32_t* accepted, int32_t* ok, int level, int nlevels, double nmin, double max_cost, void* stream);
/* theta, M (frames,9) float, score (frames) float or NULL, link (frames) int32 -> theta_out (frames,9) float, source
 * (frames) int32.  max_gap >= 0.  theta_out must not overlap theta. */
int sfh_track_propagate(const float* theta, const float* score, float max_score, const float* M, const int32_t* link,
                        int frames, int max_gap, float* theta_out, int32_t* source, void* stream);
/* Motion-compensated temporal smoothing of theta (sfh_track_smooth).  Under theta_t = theta_{t-1} M_t every good neighbour k of
 * frame t holds a second, independent estimate of theta_t: theta_k carried to t.  The estimates of one frame are combined
 * robustly - not a low-pass over time, so no lag - which averages the regression noise down, outvotes an isolated bad theta
 * that passed the score gate, and fills gaps as sfh_track_propagate does.  THE RULE, stated here once; csrc/smooth_core.h and
 * track_smooth_kernel run it, tests/smooth_ref.py restates it in numpy.  The reference project has no counterpart.
 *
 * Members.  The window of frame t is k in [t - back, t + ahead] within [0, frames), back and ahead in 0..31 (ahead = 0: the
 *   causal form).  Frame k is a MEMBER iff it is GOOD by sfh_track_propagate's definition (usable theta, optional score gate)
 *   and every link between k and t is non-zero: link[k+1 .. t] for a back member, link[t+1 .. k] for a forward one; frame t
 *   itself iff it is good.
 * Transport.  The chains and the fp64 product of sfh_track_propagate: back, P = theta_k then P = P M_j for j = k+1 .. t
 *   ascending; forward, P = theta_k then P = P adj(M_j) for j = k .. t+1 descending.  P is not normalised.
 * Control points.  ctrl (4,2) fp32, points (x, y) of the normalised frame; the default (ctrl = NULL) is (-1, 0.2), (1, 0.2),
 *   (1, 1), (-1, 1): the lower three fifths of the frame, where the court is (corners above it can lie at the ground plane's
 *   horizon).  Member k sees point p at q_k[2p], q_k[2p+1] = X / W, Y / W in normalised court units, fp64, with X, Y, W formed
 *   from P and (x, y, 1) as the predicate in() above sfh_metrics_region forms them.  A member is DROPPED unless all eight
 *   values are finite and its four W are non-zero and of one sign (a mixed sign: the horizon crosses the quadrilateral).
 *   members[t] = the members that remain.
 * Combination.  g_k = (R + 1 - |t - k|) / (R + 1), R = back for k <= t and ahead for k > t: the integers converted to fp64, one
 *   division (g_t = 1).  The reference member is the one nearest to t, a tie goes back; c0 = its eight values, d_k = q_k - c0.
 *   Pass 0 takes omega_k = 1; each of the `iters` passes after it takes r2_k = the eight squared components of q_k - c added
 *   in index order from the first, omega_k = ic ic with ic = 1 / (1 + r2_k / d2), d2 = delta delta formed on the host
 *   (sfh_track_accumulate's Geman-McClure weight).  Every pass: w_k = g_k omega_k, S = sum w_k, c_i = c0_i + (sum w_k d_k,i) /
 *   S.  The nine sums of a pass are the xor butterfly 32 .. 1 over the 64 lanes of a wave (wave_sum_all, csrc/common.h),
 *   lane l holding frame k = t - back + l and a lane without a member +0.0: that is the summation order.  Members that agree
 *   exactly give c = c0 exactly.
 * Refit.  The homography h with h8 = 1 that takes ctrl to c: rows 2p = [x y 1 0 0 0 -(u x) -(u y) | u] and 2p + 1 = [0 0 0 x y
 *   1 -(v x) -(v y) | v] of A h = b for point p, (u, v) = (c_2p, c_2p+1).  N = A^T A (lower triangle) and A^T b in fp64, each
 *   entry summed over the rows 0 .. 7 ascending from +0.0; N h = A^T b by csrc/chol8.h.  theta_out = (fl32(h_0) .. fl32(h_7), 1).
 * Statistics.  stats (frames,3) fp64 = [S of the last pass;  sqrt((sum w_k r2_k) / S) with the last pass's w and r2_k against
 *   the final c (one more butterfly);  sqrt(r2_t) of frame t's own theta against the final c, NaN when t is not a member - how
 *   far a frame's theta disagrees with the measured motion, readable without ground truth].
 * Nine NaNs and three NaN statistics where members[t] < min_members (>= 1), a c_i is not finite, or a pivot of the solve is
 *   not > 0; members[t] is written all the same.
 * One wave per frame, O(back + ahead) matrix products per lane, no workspace.  ctrl is a HOST pointer (or NULL), read before
 * the launch.  frames = 0 launches nothing.  theta_out must not overlap theta. */
int sfh_track_smooth(const float* theta, const float* score, float max_score, const float* M, const int32_t* link, int frames,
                     int back, int ahead, int iters, double delta, int min_members, const float* ctrl, float* theta_out,
                     int32_t* members, double* stats, void* stream);
/* Coarse shift search (sfh_track_search).  The Levenberg-Marquardt descent of the tracker converges from a start within about
 * 20 full-resolution pixels of the truth (256 x 144, factors 8, 4, 2); a faster pan leaves it in a wrong minimum with ok = 1.
 * The search tries every whole-pixel shift of the coarsest plane within a radius, scores each by the tracker's own robust
 * mean cost and hands the best one to the alignment as its start.  THE RULE, stated here once; csrc/search_core.h and the two
 * track_search kernels run it, tests/search_ref.py restates it in numpy.  The reference project has no counterpart.
 *
 * Inputs and candidates.  Level f, planes (nframes, hl, wl) as sfh_track_planes writes them, hl = H / f, wl = W / f; pair p =
 *   previous ia[p], current ib[p].  Radii rx, ry in 0..32.  Candidates (dx, dy) with |dx| <= rx, |dy| <= ry; candidate index
 *   c = (dy + ry) (2 rx + 1) + (dx + rx).
 * Counted pixels.  The current pixels (I, J) with 0 <= I + dy < hl and 0 <= J + dx < wl.  n = max(0, hl - |dy|) max(0, wl -
 *   |dx|): analytic, exact as a double; nothing is counted at run time.
 * Per-pixel cost.  r = (double)P_prev[I+dy][J+dx] - (double)P_cur[I][J]; q = r r / d2 with d2 = delta delta formed on the
 *   host, c = 1 + q, ic = 1 / c, rho = (r r) ic: sfh_track_accumulate's Geman-McClure cost, operation for operation.
 * Summation order, part of the rule.  One wave per candidate.  Lane l starts at +0.0 and adds rho of its counted pixels for
 *   I ascending and, within a row, J = l, l + 64, .. ascending; the 64 lane sums go through the xor butterfly 32 .. 1
 *   (wave_sum_all, csrc/common.h); mean = cost / n, one fp64 division (n = 0: NaN).  Every candidate of a pair with an index
 *   outside [0, nframes) has the mean NaN.  The table of means, workspace[p (2 rx + 1)(2 ry + 1) + c], is an output.
 * Admissibility and choice.  A candidate is admissible iff n >= nmin and its mean is finite; nmin = ceil(min_overlap hl wl)
 *   from the host, the aligner's own number.  Among the admissible candidates the smallest key (mean, dx dx + dy dy, dy, dx),
 *   compared lexicographically, is taken: ties prefer the identity, and a flat scene gives (0, 0).
 * Outputs per pair.  shift (2) int32 = (dx, dy); found int32 = 1; m0 (9) fp32 = [1, 0, tx, 0, 1, ty, 0, 0, 1] with tx =
 *   fl32(dx 2 f / (W - 1)), ty = fl32(dy 2 f / (H - 1)), each evaluated in fp64 as one exact integer product and one division and
 *   rounded once: under m0 sfh_track_accumulate's px is J + dx up to rounding.  sstats (3) fp64 = [the best mean, the mean
 *   of (0, 0) or NaN if that candidate is inadmissible, n of the best].
 * No admissible candidate (a pair index outside the frames, too small an overlap everywhere, a NaN plane): shift = (0, 0),
 *   found = 0, m0 = the identity, sstats = NaN, NaN, 0. */
/* bytes of the table of means: pairs (2 rx + 1)(2 ry + 1) doubles; -1 for pairs outside 1..65535 or a radius outside 0..32 */
int64_t sfh_track_search_workspace_bytes(int pairs, int rx, int ry);
/* Two launches on the caller's stream.  The cost kernel: grid (ceil(candidates / 4), pairs), a wave per candidate, an fp64
 * accumulator per lane, one plain store per (pair, candidate) into the workspace; no atomics.  The choice kernel: one wave per
 * pair walks the table in candidate order, each lane keeps its best key, a fixed butterfly over keys, lane 0 stores.  Refused
 * before any launch: a NULL pointer, nframes, H or W < 1, pairs outside 1..65535, f outside 1..16 or not dividing H and W,
 * planes below 2 x 2, a radius outside 0..32, delta not > 0 or not finite, nmin < 1 (a whole number as a double), a workspace
 * that is NULL or short.  ia, ib (pairs) int32 DEVICE arrays as sfh_track_accumulate takes them. */
int sfh_track_search(const float* planes, int nframes, const int32_t* ia, const int32_t* ib, int pairs, int H, int W, int f,
                     int rx, int ry, double delta, double nmin, void* workspace, long long workspace_bytes, int32_t* shift,
                     int32_t* found, float* m0, double* sstats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFH_AMD_H */
