// block_scan.h - the exclusive scan over a 256-thread workgroup that the encoders (pngenc.hip, jpegenc.hip) share.
// Everything lives in namespace blockscan; a translation unit pulls it into its own anonymous namespace.
#pragma once

namespace blockscan {

constexpr int kScanThreads = 256;

enum { OP_SUM, OP_MAX, OP_MIN };
template <int OP>
__device__ __forceinline__ int op_apply(int a, int b) {
  return OP == OP_SUM ? a + b : (OP == OP_MAX ? (a > b ? a : b) : (a < b ? a : b));
}

// exclusive scan over the 256 threads in thread order (REV: in reverse thread order); total: over all of them.
// tmp: 4 ints of LDS.  Wave step: the 64-lane shuffle forms, then the four wave results through LDS.
template <int OP, bool REV>
__device__ __forceinline__ int block_scan_excl(int v, int ident, int* tmp, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = REV ? __shfl_down(inc, d) : __shfl_up(inc, d);
    const bool ok = REV ? (lane + d < 64) : (lane >= d);
    if (ok) inc = op_apply<OP>(inc, o);
  }
  int ex = REV ? __shfl_down(inc, 1) : __shfl_up(inc, 1);
  if (lane == (REV ? 63 : 0)) ex = ident;
  __syncthreads();
  if (lane == (REV ? 0 : 63)) tmp[wv] = inc;
  __syncthreads();
  int pre = ident;
  total = ident;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const int x = tmp[w];
    total = op_apply<OP>(total, x);
    if (REV ? (w > wv) : (w < wv)) pre = op_apply<OP>(pre, x);
  }
  return op_apply<OP>(pre, ex);
}

}  // namespace blockscan
