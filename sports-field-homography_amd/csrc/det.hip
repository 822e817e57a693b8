// det.hip - the sum pass of the deterministic training mode (csrc/det_core.h states the rule).
//
//   dst[o(e)] = (...((dst[o(e)] + p_0[e]) + p_1[e]) + ...) + p_{R-1}[e],   p_r = partial + r * slab_stride
//
// One thread per element, the R slabs in ascending order, in the accumulator's own precision: the result is a function of
// (R, e) and the values alone.  Consecutive threads read consecutive elements of a slab, so every load of a wave is one
// contiguous run; the chain of a thread is R dependent adds behind R independent loads.
#include "common.h"
#include "det_core.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void det_reduce_kernel(const T* __restrict__ partial, long slabs, long slab_stride, long elems,
                                                         int ncol, T* __restrict__ dst, long dst_row_stride) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  T* d = dst + det_dst_offset(e, ncol, dst_row_stride);
  *d = det_sum(*d, partial, slabs, slab_stride, e);
}

template <typename T>
int launch_reduce(const T* partial, int64_t slabs, int64_t slab_stride, int64_t elems, int ncol, T* dst, int64_t dst_row_stride,
                  void* stream) {
  SFH_REQUIRE(partial && dst, "det_reduce: null pointer");
  SFH_REQUIRE(slabs > 0 && elems > 0 && slab_stride >= elems && ncol > 0 && elems % ncol == 0 && dst_row_stride >= ncol,
              "det_reduce: slabs=%lld slab_stride=%lld elems=%lld ncol=%d dst_row_stride=%lld", (long long)slabs,
              (long long)slab_stride, (long long)elems, ncol, (long long)dst_row_stride);
  const long nblk = ((long)elems + 255) / 256;
  SFH_REQUIRE(nblk < (1L << 31), "det_reduce: %lld elements are too many for one launch", (long long)elems);
  hipLaunchKernelGGL(det_reduce_kernel<T>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, partial, (long)slabs,
                     (long)slab_stride, (long)elems, ncol, dst, (long)dst_row_stride);
  return sfh_check_launch("det_reduce_kernel");
}

}  // namespace

extern "C" int sfh_det_reduce_f32(const float* partial, int64_t slabs, int64_t slab_stride, int64_t elems, int ncol, float* dst,
                                  int64_t dst_row_stride, void* stream) {
  return launch_reduce<float>(partial, slabs, slab_stride, elems, ncol, dst, dst_row_stride, stream);
}

extern "C" int sfh_det_reduce_f64(const double* partial, int64_t slabs, int64_t slab_stride, int64_t elems, int ncol, double* dst,
                                  int64_t dst_row_stride, void* stream) {
  return launch_reduce<double>(partial, slabs, slab_stride, elems, ncol, dst, dst_row_stride, stream);
}
