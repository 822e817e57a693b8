// codec_pack.h - the three pieces png_pack_kernel (pngenc.hip) and jpeg_pack_kernel (jpegenc.hip) share.  Both have one
// 256-thread workgroup per image; the first launch left every piece of the file (a strip's IDAT chunk, a restart interval) in
// a fixed-stride SLOT of the scratch buffer and its byte count in the first word of a META record.
#pragma once
#include "block_scan.h"

namespace codecpack {

using namespace blockscan;

// compact mode: the byte counts of the `nbefore` slots of the images before this one, summed by the workgroup for itself - no
// third launch and no workgroup that the others wait for.  META: words of a meta record.  tmp: 4 ints of LDS.
template <int META>
__device__ __forceinline__ int bytes_before(const uint32_t* __restrict__ meta, int nbefore, int* tmp) {
  int part = 0, total;
  for (int i = threadIdx.x; i < nbefore; i += kScanThreads) part += (int)meta[(size_t)i * META];
  block_scan_excl<OP_SUM, false>(part, 0, tmp, total);
  return total;
}

// a wave copies a slot: slot j of the `nhere` slots from `src` on (`stride` bytes apart) goes to dst + off_s[j], cnt_s[j] bytes
// of it.  The destination has any alignment: up to 3 head bytes, aligned dword stores from byte loads, the tail.
__device__ __forceinline__ void copy_slots(const uint8_t* src, size_t stride, int nhere, uint8_t* dst, const int* off_s,
                                           const int* cnt_s) {
  const int lane = threadIdx.x & 63;
  for (int j = threadIdx.x >> 6; j < nhere; j += kScanThreads / 64) {
    const uint8_t* s = src + j * stride;
    uint8_t* d = dst + off_s[j];
    const int n = cnt_s[j];
    int headb = (int)((4u - (uint32_t)(uintptr_t)d) & 3u);
    if (headb > n) headb = n;
    if (lane < headb) d[lane] = s[lane];
    const int nw = (n - headb) / 4;
    for (int w = lane; w < nw; w += 64) {
      const uint8_t* sp = s + headb + 4 * w;
      *reinterpret_cast<uint32_t*>(d + headb + 4 * w) =
          (uint32_t)sp[0] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[2] << 16) | ((uint32_t)sp[3] << 24);
    }
    const int done = headb + 4 * nw;
    if (lane < n - done) d[done + lane] = s[done + lane];
  }
}

// one thread closes image b: its size, where it starts, and behind the last image where the batch ends
__device__ __forceinline__ void write_index(int b, int batch, int base, int size, int capacity, int compact,
                                            int64_t* __restrict__ offsets, int32_t* __restrict__ sizes) {
  sizes[b] = size;
  offsets[b] = base;
  if (b == batch - 1) offsets[batch] = compact ? (int64_t)base + size : (int64_t)batch * capacity;
}

}  // namespace codecpack
