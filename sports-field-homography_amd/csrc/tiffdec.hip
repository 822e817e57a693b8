// tiffdec.hip - 8- and 16-bit TIFF files to device images (sfh_amd.tiffdec; the pixels are those of outputs.decode_tiff, which
// tests/test_tiff_host.py holds to libtiff's strips and to Pillow).  The core - the parse of the header and the IFD, the LZW decode
// of one strip by one wave and its bounds rules, the arithmetic of one sample - is csrc/tiff_core.h, shared with the stand-alone
// host program tests/tiff_host_main.cpp.  Integers only.
//
// * Host: sfh_tiff_parse reads the header and the first IFD; sfh_tiff_dec_stage packs the parses, strip tables and files of a
//   batch into one staging buffer for one copy.  Every offset is checked against the file there; the kernel clamps them again.
// * tiff_lzw_kernel, one workgroup (one wave) per (image, strip): the strip decoded (or, uncompressed, copied) into its rows of
//   the image's decoded bytes in the scratch -> a status word per strip.  The dictionary, 24 KB, is in LDS; the bytes a code
//   copies are read back from the scratch, which the same workgroup wrote before an earlier workgroup barrier.
// * tiff_verdict_kernel, a thread per image: the OR of its strips' status words -> status.
// * tiff_unpredict_kernel, one workgroup per (image, 8 rows): the samples in the file's byte order, with predictor 2 their prefix
//   sum per channel modulo 2^bits (block_scan.h, a carry across tiles of 1024 pixels), the channel order, the (B,H,W[,C]) layout.
//   An image with a status: zeros.
// No global atomics; no workgroup waits for another; no host synchronisation.
#include "common.h"
#include "block_scan.h"
#include "codec_host.h"
#include "tiff_core.h"

namespace {

using namespace blockscan;
constexpr int kThreads = kScanThreads;
constexpr uint32_t kMagic = 0x54444543u;   // "TDEC"
constexpr int kRowsPerGroup = 8;
constexpr int kPixPerThread = 4;

struct TiffGeom {
  int64_t rowbytes, total, slot;   // bytes of a decoded row, of an image, of an image's slot in the scratch
  int64_t st, bytes;               // scratch: where the strips' status words start, all of it
  int64_t strip_cap, staging;
};

bool tiff_geom(int batch, int H, int W, int C, int bits, int64_t max_file_bytes, TiffGeom* g) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || (C != 1 && C != 3) || (bits != 8 && bits != 16)) return false;
  g->rowbytes = (int64_t)W * C * (bits / 8);
  g->total = (int64_t)H * g->rowbytes;
  if (g->total >= ((int64_t)1 << 31) - 65536) return false;
  g->slot = round16(g->total);
  g->st = (int64_t)batch * g->slot;
  g->bytes = g->st + round16((int64_t)batch * H * 4);
  if (g->bytes >= ((int64_t)1 << 32)) return false;
  g->strip_cap = H;                                        // RowsPerStrip is at least 1
  if (max_file_bytes < 0) return true;                     // the scratch alone
  if (max_file_bytes < 8 || max_file_bytes >= ((int64_t)1 << 28)) return false;
  g->staging = kStageHeadBytes + (int64_t)batch * ((int64_t)sizeof(sfh_tiff_info) + 16 * g->strip_cap + round16(max_file_bytes) + 32);
  return g->staging < ((int64_t)1 << 31);
}

struct TiffArgs {
  int H, W, C, bits, bgr;
  int64_t rowbytes, slot, st;
};

__device__ __forceinline__ const sfh_tiff_info* staged_info(const uint8_t* staged, int b) {
  return reinterpret_cast<const sfh_tiff_info*>(staged + kStageHeadBytes) + b;
}

// scratch is read back by the workgroup that wrote it: no __restrict__
__global__ __launch_bounds__(kTdLanes) void tiff_lzw_kernel(const uint8_t* __restrict__ staged, TiffArgs a, uint8_t* scratch) {
  __shared__ TdShared sh;
  const int s = blockIdx.x, b = blockIdx.y;
  const sfh_tiff_info* info = staged_info(staged, b);
  if (s >= info->nstrips || s >= a.H) return;            // uniform over the workgroup
  const int32_t* rec = reinterpret_cast<const int32_t*>(staged + info->table_pos) + 4 * (int64_t)s;
  int32_t off = rec[0], cnt = rec[1], row0 = rec[2], rows = rec[3];
  // the host checked all four; clamped again so that no read leaves the file and no store the image's slot
  off = off < 0 ? 0 : (off > info->file_bytes ? info->file_bytes : off);
  cnt = cnt < 0 ? 0 : (cnt > info->file_bytes - off ? info->file_bytes - off : cnt);
  row0 = row0 < 0 ? 0 : (row0 > a.H ? a.H : row0);
  rows = rows < 0 ? 0 : (rows > a.H - row0 ? a.H - row0 : rows);
  const uint8_t* src = staged + info->file_pos + off;
  uint8_t* out = scratch + (int64_t)b * a.slot + (int64_t)row0 * a.rowbytes;
  const int32_t total = (int32_t)(rows * a.rowbytes);
  const int st = info->compression == 5 ? td_lzw_strip(src, cnt, sh, out, total) : td_copy_strip(src, cnt, out, total);
  if (threadIdx.x == 0) reinterpret_cast<int32_t*>(scratch + a.st)[(int64_t)b * a.H + s] = st;
}

__global__ __launch_bounds__(kTdLanes) void tiff_verdict_kernel(const uint8_t* __restrict__ staged, TiffArgs a, int batch,
                                                                const uint8_t* __restrict__ scratch, int32_t* __restrict__ status) {
  const int b = blockIdx.x * kTdLanes + threadIdx.x;
  if (b >= batch) return;
  int n = staged_info(staged, b)->nstrips;
  n = n > a.H ? a.H : n;
  const int32_t* st = reinterpret_cast<const int32_t*>(scratch + a.st) + (int64_t)b * a.H;
  int all = 0;
  for (int s = 0; s < n; ++s) all |= st[s];
  status[b] = all;
}

template <class T>
__global__ __launch_bounds__(kThreads) void tiff_unpredict_kernel(const uint8_t* __restrict__ staged, TiffArgs a,
                                                                  const uint8_t* __restrict__ scratch,
                                                                  const int32_t* __restrict__ status, T* __restrict__ out) {
  __shared__ int tmp[4];
  const int t = threadIdx.x, b = blockIdx.y;
  const sfh_tiff_info* info = staged_info(staged, b);
  const bool bad = status[b] != 0;
  const bool sum_rows = !bad && info->predictor == 2;    // uniform
  const int be = info->big_endian;
  const int C = a.C, W = a.W, mask = (1 << a.bits) - 1;
  const uint8_t* dec = scratch + (int64_t)b * a.slot;
  int oc[3];
  for (int k = 0; k < 3; ++k) oc[k] = td_out_channel(k, C, a.bgr);
  const int y1 = (blockIdx.x + 1) * kRowsPerGroup < a.H ? (blockIdx.x + 1) * kRowsPerGroup : a.H;
  for (int y = blockIdx.x * kRowsPerGroup; y < y1; ++y) {
    const uint8_t* row = dec + (int64_t)y * a.rowbytes;
    int carry[3] = {0, 0, 0};
    for (int x0 = 0; x0 < W; x0 += kThreads * kPixPerThread) {   // uniform trip count
      const int xa = x0 + t * kPixPerThread;
      int v[kPixPerThread][3];
      int sum[3] = {0, 0, 0};
#pragma unroll
      for (int i = 0; i < kPixPerThread; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < C) {
            const int d = (!bad && xa + i < W) ? (int)td_sample(row, (int64_t)(xa + i) * C + k, a.bits, be) : 0;
            sum[k] += d;
            v[i][k] = sum_rows ? sum[k] : d;               // the inclusive sum within the thread
          }
      if (sum_rows) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < C) {
            int tot;
            const int ex = block_scan_excl<OP_SUM, false>(sum[k], 0, tmp, tot);   // <= 1024 * 65535
            const int add = carry[k] + ex;
#pragma unroll
            for (int i = 0; i < kPixPerThread; ++i) v[i][k] += add;
            carry[k] = (carry[k] + tot) & mask;
          }
      }
#pragma unroll
      for (int i = 0; i < kPixPerThread; ++i)
        if (xa + i < W) {
          T* p = out + (((int64_t)b * a.H + y) * W + xa + i) * C;
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (k < C) p[oc[k]] = (T)(v[i][k] & mask);
        }
    }
  }
}

}  // namespace

extern "C" int sfh_tiff_parse(const uint8_t* host_bytes, int64_t n, sfh_tiff_info* host_info, int32_t* host_strips, int64_t strip_cap) {
  SFH_REQUIRE(host_bytes && host_info && n >= 0 && strip_cap >= 0 && (host_strips || strip_cap == 0),
              "tiff_parse: null pointer or negative size");
  const int rc = td_parse(host_bytes, n, host_info, host_strips, strip_cap);
  if (rc) sfh_set_error("tiff_parse: refused, reason %d", host_info->reason);
  return rc;
}

extern "C" int64_t sfh_tiff_dec_staging_bytes(int batch, int H, int W, int C, int bits, int64_t max_file_bytes) {
  TiffGeom g;
  if (max_file_bytes < 0 || !tiff_geom(batch, H, W, C, bits, max_file_bytes, &g)) {
    sfh_set_error("tiff_dec_staging_bytes: batch %d image %dx%dx%d of %d bits, files of %lld bytes", batch, W, H, C, bits,
                  (long long)max_file_bytes);
    return -1;
  }
  return g.staging;
}

extern "C" int64_t sfh_tiff_dec_scratch_bytes(int batch, int H, int W, int C, int bits) {
  TiffGeom g;
  if (!tiff_geom(batch, H, W, C, bits, -1, &g)) {
    sfh_set_error("tiff_dec_scratch_bytes: batch %d image %dx%dx%d of %d bits", batch, W, H, C, bits);
    return -1;
  }
  return g.bytes;
}

extern "C" int64_t sfh_tiff_dec_stage(const uint8_t* const* host_files, const int64_t* host_sizes, int batch, int H, int W, int C,
                                      int bits, int64_t max_file_bytes, uint8_t* host_staging, int64_t staging_bytes,
                                      int32_t* host_reason, int32_t* host_index) {
  TiffGeom g;
  const int64_t need = max_file_bytes >= 0 && tiff_geom(batch, H, W, C, bits, max_file_bytes, &g) ? g.staging : -1;
  if (!stage_begin("tiff_dec_stage", host_files, host_sizes, host_staging, staging_bytes, need, host_reason, host_index)) return -1;
  sfh_tiff_info* infos = reinterpret_cast<sfh_tiff_info*>(host_staging + kStageHeadBytes);
  int64_t pos = kStageHeadBytes + (int64_t)batch * (int64_t)sizeof(sfh_tiff_info);
  int max_strips = 0;
  for (int b = 0; b < batch; ++b) {
    sfh_tiff_info* info = infos + b;
    int32_t* table = reinterpret_cast<int32_t*>(host_staging + pos);
    int reason = stage_file_reason(host_files[b], host_sizes[b], max_file_bytes, SFH_TIFF_R_TRUNCATED, SFH_TIFF_R_TOO_LONG);
    if (reason == SFH_TIFF_R_OK) {
      if (td_parse(host_files[b], host_sizes[b], info, table, g.strip_cap)) reason = info->reason;
      else if (info->width != W || info->height != H || info->channels != C || info->bits != bits || info->nstrips > g.strip_cap)
        reason = SFH_TIFF_R_SIZE;
    }
    if (reason != SFH_TIFF_R_OK) return stage_refuse_file("tiff_dec_stage", b, reason, host_reason, host_index);
    info->table_pos = (int32_t)pos;
    pos += 16 * (int64_t)info->nstrips;
    max_strips = info->nstrips > max_strips ? info->nstrips : max_strips;
  }
  pos = stage_copy_files(infos, host_files, host_sizes, batch, host_staging, pos);
  stage_head(host_staging, kMagic, batch, max_strips)[3] = (uint32_t)pos;
  return pos;
}

extern "C" int sfh_tiff_decode(const uint8_t* host_staging, const uint8_t* staged, int64_t staged_bytes, int batch, int H, int W, int C,
                               int bits, int bgr, int64_t max_file_bytes, uint8_t* scratch, int64_t scratch_bytes, void* out,
                               int32_t* status, void* stream) {
  TiffGeom g;
  SFH_REQUIRE(max_file_bytes >= 0 && tiff_geom(batch, H, W, C, bits, max_file_bytes, &g), "tiff_decode: batch %d image %dx%dx%d of %d bits",
              batch, W, H, C, bits);
  SFH_REQUIRE(out && status, "tiff_decode: null pointer (out, status)");
  if (int rc = decode_begin("tiff_decode", "sfh_tiff_dec_stage", host_staging, staged, staged_bytes, scratch, scratch_bytes, g.bytes,
                            kMagic, batch, g.strip_cap, 3))
    return rc;
  const uint32_t* head = reinterpret_cast<const uint32_t*>(host_staging);
  hipStream_t st = (hipStream_t)stream;
  TiffArgs a;
  a.H = H;
  a.W = W;
  a.C = C;
  a.bits = bits;
  a.bgr = bgr ? 1 : 0;
  a.rowbytes = g.rowbytes;
  a.slot = g.slot;
  a.st = g.st;
  hipLaunchKernelGGL(tiff_lzw_kernel, dim3(head[2], (unsigned)batch), dim3(kTdLanes), 0, st, staged, a, scratch);
  if (int rc = sfh_check_launch("tiff_lzw_kernel")) return rc;
  hipLaunchKernelGGL(tiff_verdict_kernel, dim3((unsigned)sfh_cdiv(batch, kTdLanes)), dim3(kTdLanes), 0, st, staged, a, batch, scratch,
                     status);
  if (int rc = sfh_check_launch("tiff_verdict_kernel")) return rc;
  const dim3 grid((unsigned)sfh_cdiv(H, kRowsPerGroup), (unsigned)batch);
  if (bits == 16)
    hipLaunchKernelGGL(tiff_unpredict_kernel<uint16_t>, grid, dim3(kThreads), 0, st, staged, a, scratch, status,
                       static_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL(tiff_unpredict_kernel<uint8_t>, grid, dim3(kThreads), 0, st, staged, a, scratch, status,
                       static_cast<uint8_t*>(out));
  return sfh_check_launch("tiff_unpredict_kernel");
}
