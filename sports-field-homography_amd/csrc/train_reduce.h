// train_reduce.h - the end of a per-channel pixel reduction, shared by the training kernels of train_bn.hip and
// train_heads.hip (outconv_bwd_kernel).
#pragma once

#include "det_core.h"   // det_add: the default mode's atomic or the deterministic mode's store

// ------------------------------------------------------------------ per-channel reductions
// rows = pixels, C channels (multiple of 4).  A block of 256 threads = (256/cq) pixel lanes x cq
// channel quads strides over the pixels (grid-stride, at most RED_BLOCKS blocks so that the fp64
// atomics on the few accumulator addresses stay cheap) and adds its partials to fp64 accumulators;
// C > 1024 is processed in chunks of 1024 channels.
// (det_core.h, det_red_blocks: DET_RED_ROWS = 256 pixels per block below which no further blocks are launched,
// DET_RED_BLOCKS = 1024, 4 per CU)

// DET (every accumulating kernel below): the store pass of the deterministic mode (det_core.h).  `acc` is then the workspace,
// the block moves it to its own slab and the last add of every element is a plain store; DET = false is the kernel as it was.

// The end of such a block: thread (pixel lane pl, channel quad q) = threadIdx.x = pl * cq + q holds NV partial sums, NV / 4
// rows of its quad's four channels (s[4 * r + i]: row r, channel 4 * q + i; `live`: pl < 256 / cq).  One value at a time goes
// through sh[256], the first cq threads add the lanes up and acc[r * row_stride + 4 * q + i] takes the sum in one atomic.
template <bool DET = false, int NV>
__device__ __forceinline__ void red_tail(const double (&s)[NV], bool live, int cq, double* sh, double* __restrict__ acc,
                                         long row_stride) {
  const int lanes = 256 / cq;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    __syncthreads();
    sh[threadIdx.x] = live ? s[j] : 0.0;
    __syncthreads();
    if (threadIdx.x < cq) {
      double t = 0.0;
      for (int l = 0; l < lanes; ++l) t += sh[l * cq + threadIdx.x];
      det_add<DET>(&acc[(long)(j >> 2) * row_stride + 4 * threadIdx.x + (j & 3)], t);
    }
  }
}
