// tiffenc.hip - device images to 8- and 16-bit TIFF files (sfh_amd.tiffenc; the byte-exact rule is outputs.encode_tiff, which
// tests/test_tiff_host.py holds to libtiff's strips).  The encode of one strip - the bytes as the file holds them, differenced
// with predictor 2, and the greedy LZW - is csrc/tiff_core.h, shared with tests/tiff_host_main.cpp.  Integers only.
//
// * tiff_encode_kernel, one workgroup (one wave) per (image, strip): the strip's bytes are formed 4 KB at a time in LDS by all
//   lanes, straight from the image; the LZW itself is serial - the wave runs it as uniform code, lane 0 stores - with the
//   dictionary as a hash table of 32 KB in LDS.  The strip goes to its fixed-stride slot, its byte count to a meta word.
// * tiff_pack_kernel, one workgroup per image, with codec_pack.h's pieces: the running sum of the even-aligned strip sizes, then
//   the header, the strips, the tag arrays and the IFD into the TiffBatch.  In compact mode every workgroup sums the sizes of the
//   images before its own for itself.
// No global atomics; no workgroup waits for another; no host synchronisation.
#include "common.h"
#include "block_scan.h"
#include "codec_host.h"
#include "codec_pack.h"
#include "tiff_core.h"

namespace {

using namespace codecpack;
constexpr int kThreads = kScanThreads;
constexpr int kIfdEntries = 12;
constexpr int kIfdBytes = 2 + 12 * kIfdEntries + 4;

struct EncGeom {
  int R, nstrips, stride;          // rows of a strip, strips of an image, bytes between two slots
  int fixed;                       // bytes of a file that are not strips: header, tag arrays, IFD
  int64_t capacity, slots, bytes;  // of a file; scratch: where the slots start, all of it
};

bool enc_geom(int batch, int H, int W, int C, int bits, int compression, int predictor, int rows_per_strip, EncGeom* g) {
  if (batch < 1 || H < 1 || W < 1 || (C != 1 && C != 3) || (bits != 8 && bits != 16) || (compression != 1 && compression != 5) ||
      (predictor != 1 && predictor != 2) || (compression == 1 && predictor != 1) || rows_per_strip < 0 || rows_per_strip > H)
    return false;
  const int64_t rowbytes = (int64_t)W * C * (bits / 8);
  if ((int64_t)H * rowbytes >= ((int64_t)1 << 31) - 65536) return false;
  g->R = rows_per_strip ? rows_per_strip : te_default_rows(H, W, C, bits);
  g->nstrips = sfh_cdiv(H, g->R);
  const int64_t cap = te_strip_capacity(g->R * rowbytes, compression);
  g->stride = (int)round16(cap);
  g->fixed = 8 + (C == 3 ? 12 : 0) + (g->nstrips > 1 ? 8 * g->nstrips : 0) + kIfdBytes;
  g->capacity = round16((int64_t)g->fixed + (int64_t)g->nstrips * (cap + 1));
  g->slots = round16((int64_t)batch * g->nstrips * 4);
  g->bytes = g->slots + (int64_t)batch * g->nstrips * g->stride;
  return g->capacity < ((int64_t)1 << 31);
}

__global__ __launch_bounds__(kTdLanes) void tiff_encode_kernel(const uint8_t* __restrict__ images, TeGeom tg, int R, int nstrips,
                                                               int compression, int stride, uint32_t* __restrict__ meta,
                                                               uint8_t* __restrict__ slots) {
  __shared__ TeShared sh;
  const int s = blockIdx.x, b = blockIdx.y;
  const uint8_t* img = images + (int64_t)b * tg.H * tg.W * tg.C * (tg.bits / 8);
  const int row0 = s * R, rows = tg.H - row0 < R ? tg.H - row0 : R;
  const size_t sidx = (size_t)b * nstrips + s;
  const int32_t n = te_encode_strip(img, tg, row0, rows, compression, sh, slots + sidx * (size_t)stride, stride);
  if (threadIdx.x == 0) meta[sidx] = (uint32_t)n;
}

__device__ __forceinline__ void put_le16(uint8_t* o, uint32_t v) {
  o[0] = (uint8_t)v;
  o[1] = (uint8_t)(v >> 8);
}
__device__ __forceinline__ void put_le32(uint8_t* o, uint32_t v) {
  put_le16(o, v);
  put_le16(o + 2, v >> 16);
}
// an IFD entry whose value (or offset) is one LONG or one SHORT
__device__ __forceinline__ uint8_t* put_entry(uint8_t* o, int tag, int type, uint32_t count, uint32_t value) {
  put_le16(o, (uint32_t)tag);
  put_le16(o + 2, (uint32_t)type);
  put_le32(o + 4, count);
  put_le32(o + 8, value);                                  // a SHORT sits in the low half, the high half is zero
  return o + 12;
}

__device__ __forceinline__ int even_up(int v) { return (v + 1) & ~1; }

__global__ __launch_bounds__(kThreads) void tiff_pack_kernel(const uint32_t* __restrict__ meta, const uint8_t* __restrict__ slots,
                                                             int batch, int H, int W, int C, int bits, int compression, int predictor,
                                                             int R, int nstrips, int stride, int fixed, int capacity, int compact,
                                                             uint8_t* __restrict__ out, int64_t* __restrict__ offsets,
                                                             int32_t* __restrict__ sizes) {
  __shared__ int tmp[4];
  __shared__ int off_s[kThreads], cnt_s[kThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  // where the image starts: the even-aligned strips of the images before it and their fixed parts
  int base = b * capacity;
  if (compact) {
    int part = 0, before;
    for (int i = t; i < b * nstrips; i += kThreads) part += even_up((int)meta[i]);
    block_scan_excl<OP_SUM, false>(part, 0, tmp, before);
    base = before + b * fixed;
  }
  const uint32_t* m = meta + (size_t)b * nstrips;
  int part = 0, strips_bytes;
  for (int i = t; i < nstrips; i += kThreads) part += even_up((int)m[i]);
  block_scan_excl<OP_SUM, false>(part, 0, tmp, strips_bytes);
  uint8_t* dst = out + base;
  const int arrays = 8 + strips_bytes;                     // BitsPerSample, SampleFormat (C == 3), then the two strip tables
  const int tables = arrays + (C == 3 ? 12 : 0);
  const int ifd = tables + (nstrips > 1 ? 8 * nstrips : 0);
  int pos = 8;
  for (int s0 = 0; s0 < nstrips; s0 += kThreads) {
    const int s = s0 + t;
    const bool live = s < nstrips;
    const int cnt = live ? (int)m[s] : 0;
    int tot;
    const int off = pos + block_scan_excl<OP_SUM, false>(even_up(cnt), 0, tmp, tot);
    __syncthreads();
    off_s[t] = off;
    cnt_s[t] = cnt;
    __syncthreads();
    const int nhere = nstrips - s0 < kThreads ? nstrips - s0 : kThreads;
    copy_slots(slots + ((size_t)b * nstrips + s0) * (size_t)stride, (size_t)stride, nhere, dst, off_s, cnt_s);
    if (live) {
      if (cnt & 1) dst[off + cnt] = 0;
      if (nstrips > 1) {
        put_le32(dst + tables + 4 * s, (uint32_t)off);
        put_le32(dst + tables + 4 * nstrips + 4 * s, (uint32_t)cnt);
      }
    }
    pos += tot;
  }
  if (t == 0) {
    dst[0] = 'I';
    dst[1] = 'I';
    put_le16(dst + 2, 42);
    put_le32(dst + 4, (uint32_t)ifd);
    if (C == 3)
      for (int k = 0; k < 3; ++k) {
        put_le16(dst + arrays + 2 * k, (uint32_t)bits);
        put_le16(dst + arrays + 6 + 2 * k, 1);
      }
    uint8_t* o = dst + ifd;
    put_le16(o, kIfdEntries);
    o += 2;
    o = put_entry(o, 256, 4, 1, (uint32_t)W);
    o = put_entry(o, 257, 4, 1, (uint32_t)H);
    o = put_entry(o, 258, 3, (uint32_t)C, C == 3 ? (uint32_t)arrays : (uint32_t)bits);
    o = put_entry(o, 259, 3, 1, (uint32_t)compression);
    o = put_entry(o, 262, 3, 1, C == 3 ? 2u : 1u);
    o = put_entry(o, 273, 4, (uint32_t)nstrips, nstrips > 1 ? (uint32_t)tables : 8u);
    o = put_entry(o, 277, 3, 1, (uint32_t)C);
    o = put_entry(o, 278, 4, 1, (uint32_t)R);
    o = put_entry(o, 279, 4, (uint32_t)nstrips, nstrips > 1 ? (uint32_t)(tables + 4 * nstrips) : m[0]);
    o = put_entry(o, 284, 3, 1, 1);
    o = put_entry(o, 317, 3, 1, (uint32_t)predictor);
    o = put_entry(o, 339, 3, (uint32_t)C, C == 3 ? (uint32_t)(arrays + 6) : 1u);
    put_le32(o, 0);
    write_index(b, batch, base, ifd + kIfdBytes, capacity, compact, offsets, sizes);
  }
}

int tiff_enc_check(const char* who, int batch, int H, int W, int C, int bits, int compression, int predictor, int rows_per_strip,
                   EncGeom* g) {
  SFH_REQUIRE(enc_geom(batch, H, W, C, bits, compression, predictor, rows_per_strip, g),
              "%s: batch %d image %dx%dx%d of %d bits, compression %d, predictor %d, %d rows per strip", who, batch, W, H, C, bits,
              compression, predictor, rows_per_strip);
  return enc_batch_check(who, batch, H, W, C, g->capacity, g->bytes);
}

}  // namespace

extern "C" int64_t sfh_tiff_strip_capacity(int64_t n, int compression) {
  if (n < 0 || (compression != 1 && compression != 5)) {
    sfh_set_error("tiff_strip_capacity: %lld bytes, compression %d", (long long)n, compression);
    return -1;
  }
  return te_strip_capacity(n, compression);
}

extern "C" int64_t sfh_tiff_capacity(int H, int W, int C, int bits, int compression, int rows_per_strip) {
  EncGeom g;
  if (!enc_geom(1, H, W, C, bits, compression, 1, rows_per_strip, &g)) {
    sfh_set_error("tiff_capacity: image %dx%dx%d of %d bits, compression %d, %d rows per strip", W, H, C, bits, compression,
                  rows_per_strip);
    return -1;
  }
  return g.capacity;
}

extern "C" int64_t sfh_tiff_scratch_bytes(int batch, int H, int W, int C, int bits, int compression, int rows_per_strip) {
  EncGeom g;
  if (!enc_geom(batch, H, W, C, bits, compression, 1, rows_per_strip, &g)) {
    sfh_set_error("tiff_scratch_bytes: batch %d image %dx%dx%d of %d bits, compression %d, %d rows per strip", batch, W, H, C, bits,
                  compression, rows_per_strip);
    return -1;
  }
  return g.bytes;
}

extern "C" int sfh_tiff_encode(const void* images, int batch, int H, int W, int C, int bits, int bgr, int compression, int predictor,
                               int rows_per_strip, uint8_t* scratch, int64_t scratch_bytes, void* stream) {
  EncGeom g;
  if (int rc = tiff_enc_check("tiff_encode", batch, H, W, C, bits, compression, predictor, rows_per_strip, &g)) return rc;
  SFH_REQUIRE(images && scratch, "tiff_encode: null pointer (images, scratch)");
  if (int rc = enc_scratch_check("tiff_encode", scratch, scratch_bytes, g.bytes)) return rc;
  TeGeom tg;
  tg.H = H;
  tg.W = W;
  tg.C = C;
  tg.bits = bits;
  tg.bgr = bgr ? 1 : 0;
  tg.predictor = predictor;
  hipLaunchKernelGGL(tiff_encode_kernel, dim3((unsigned)g.nstrips, (unsigned)batch), dim3(kTdLanes), 0, (hipStream_t)stream,
                     static_cast<const uint8_t*>(images), tg, g.R, g.nstrips, compression, g.stride,
                     reinterpret_cast<uint32_t*>(scratch), scratch + g.slots);
  return sfh_check_launch("tiff_encode_kernel");
}

extern "C" int sfh_tiff_pack(const uint8_t* scratch, int64_t scratch_bytes, int batch, int H, int W, int C, int bits, int compression,
                             int predictor, int rows_per_strip, int compact, uint8_t* out, int64_t out_bytes, int64_t* offsets,
                             int32_t* sizes, void* stream) {
  EncGeom g;
  if (int rc = tiff_enc_check("tiff_pack", batch, H, W, C, bits, compression, predictor, rows_per_strip, &g)) return rc;
  SFH_REQUIRE(scratch && out && offsets && sizes, "tiff_pack: null pointer (scratch, out, offsets, sizes)");
  if (int rc = enc_scratch_check("tiff_pack", scratch, scratch_bytes, g.bytes)) return rc;
  SFH_REQUIRE(out_bytes >= g.capacity * batch, "tiff_pack: output of %lld bytes, %lld needed (batch * tiff_capacity)",
              (long long)out_bytes, (long long)(g.capacity * batch));
  hipLaunchKernelGGL(tiff_pack_kernel, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(scratch), scratch + g.slots, batch, H, W, C, bits, compression, predictor, g.R,
                     g.nstrips, g.stride, g.fixed, (int)g.capacity, compact ? 1 : 0, out, offsets, sizes);
  return sfh_check_launch("tiff_pack_kernel");
}
