// conv_grouped_core.h - the index arithmetic of the grouped 3x3 convolution (csrc/conv_grouped.hip), stated once.
//
// The layer: nn.Conv2d(C, C, 3, stride, padding 1, groups = G, bias = False) with C = G * cg; fp32 NHWC tensors; group g owns
// channels [g * cg, (g + 1) * cg) of source and destination.  Everything below is plain integer arithmetic that host and
// device evaluate alike: tests/grouped_conv_host_main.cpp runs forward, backward-data and backward-filter output by output
// through these functions, in the kernels' order.
//
// THE ORDER OF ONE OUTPUT'S TERMS (forward and backward-data; K = 9 * cg products, each rounded once, each add rounded once,
// no contraction - build.py compiles with -ffp-contract=off):
//   acc = 0
//   for chunk in 0 .. cg / gc_chunk(cg) - 1:                 (one chunk for cg <= 32, two for cg = 64)
//     for tap in 0 .. 8:                                     (tap = 3 * ky + kx)
//       for c in chunk * gc_chunk(cg) .. (chunk + 1) * gc_chunk(cg) - 1:
//         acc += x[source pixel of tap, g * cg + c] * w[o, c, tap]       (x = 0 where the tap lies in the padding)
// Two launches over the same operands therefore give the same bits.
//
// Plain C++, no HIP header: SFH_GC_FN marks what the device runs too.
#pragma once

#if defined(__HIPCC__)
#define SFH_GC_FN __host__ __device__ __forceinline__
#else
#define SFH_GC_FN inline
#endif

// workgroup tile of OUTPUT pixels: GC_TW columns x gc_tile_h(stride) rows (stride 2: half the rows, the halo is twice as wide)
#define GC_TW 16
SFH_GC_FN int gc_tile_h(int stride) { return stride == 1 ? 8 : 4; }
// rows / columns of source pixels a tile of th x GC_TW outputs reads
SFH_GC_FN int gc_halo(int n_out, int stride) { return (n_out - 1) * stride + 3; }

SFH_GC_FN bool gc_cg_ok(int cg) { return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64; }
// output channels one forward workgroup computes: whole groups, 32 channels (cg = 64: the one group)
SFH_GC_FN int gc_cb(int cg) { return cg < 32 ? 32 : cg; }
// input channels of a group that are resident in LDS at a time
SFH_GC_FN int gc_chunk(int cg) { return cg < 32 ? cg : 32; }
SFH_GC_FN int gc_out_size(int n, int stride) { return (n - 1) / stride + 1; }

// output coordinate o (or a tile's first output coordinate) + offset k (tap 0..2, or a halo row / column) -> source
// coordinate, or -1 for the padding zero; n = source extent.  The one place a source coordinate is made: a caller loads
// only where this is >= 0, so every load is inside the tensor.
SFH_GC_FN int gc_src_coord(int o, int k, int stride, int n) {
  const int s = o * stride + k - 1;
  return (s >= 0 && s < n) ? s : -1;
}

// NHWC element offset of channel c of group g at pixel index `pixel` (= (b * H + y) * W + x) of a C-channel tensor
SFH_GC_FN long gc_nhwc(long pixel, int C, int cg, int g, int c) { return pixel * (long)C + (long)g * cg + c; }

// Packed weights: [channel block of gc_cb outputs][chunk][tap][c in chunk][output in block], zero where the block reaches past
// the last channel - what one forward workgroup reads as one contiguous run per chunk.
SFH_GC_FN long gc_packed_floats(int groups, int cg) {
  const int cb = gc_cb(cg);
  return (long)((groups * cg + cb - 1) / cb) * 9 * cg * cb;
}
// oc: output channel (global); c: input channel inside oc's group
SFH_GC_FN long gc_packed_index(int cg, int oc, int tap, int c) {
  const int cb = gc_cb(cg), kc = gc_chunk(cg);
  return ((((long)(oc / cb) * (cg / kc) + c / kc) * 9 + tap) * kc + c % kc) * cb + oc % cb;
}
// The OIHW element of the (G * cg, cg, 3, 3) checkpoint weight that packed element (oc, tap, c) holds.
//   mode 0, forward:        w[oc][c][tap]
//   mode 1, backward-data:  the conv that maps dz -> dx: its output channel oc = g * cg + (input channel of the layer), its
//                           input channel c = (output channel of the layer inside g), both taps flipped:
//                           w[g * cg + c][oc % cg][8 - tap]
SFH_GC_FN long gc_weight_index(int mode, int cg, int oc, int tap, int c) {
  if (mode == 0) return ((long)oc * cg + c) * 9 + tap;
  return ((long)((oc / cg) * cg + c) * cg + oc % cg) * 9 + (8 - tap);
}

// Backward-filter: raw (G * cg, 9, cg), raw[o][tap][c] += sum_p dz[p, o] * x[p * stride + tap - 1, g(o) * cg + c].
SFH_GC_FN long gc_raw_index(int cg, int o, int tap, int c) { return ((long)o * 9 + tap) * cg + c; }
// The accumulation plan of one raw element (csrc/conv_grouped.hip, conv_grouped_wgrad_kernel), all in fp32:
//   a workgroup owns one tile of gc_tile_h x GC_TW output pixels; gc_wgrad_lanes(cg) threads share an element: lane l adds the
//   products of the tile's pixels l, l + lanes, l + 2 * lanes, ... (row-major inside the tile, pixels outside the map count
//   as zeros) in that order, starting from 0; the lanes' partial sums are added in lane order; the workgroup adds the result
//   to raw with ONE atomic add.  The order of the workgroups' atomic adds is free.
SFH_GC_FN int gc_wgrad_lanes(int cg) { return 256 / (32 * (gc_chunk(cg) / 4)); }
