// pngdec.hip - standard PNG files to uint8 device images (sfh_amd.pngdec; the pixels are those of outputs.decode_png, which
// tests/test_pngdec_host.py holds to PIL's).  The decode core - chunk parse with CRC-32, the bit reader over the joined IDAT bodies,
// the code tables, the inflate of one deflate sequence by one wave and its bounds rules, the arithmetic of one pixel - is
// csrc/pngdec_core.h, shared with the stand-alone host program tests/pngdec_host_main.cpp.  Integers only.
//
// * Host: sfh_png_parse walks the chunks; sfh_png_dec_stage packs the parses, range tables and files of a batch into one staging
//   buffer for one copy.
// * The segmented leg, launched only when a file of the batch has 2 .. SFH_PNG_DEC_MAX_SEGMENTS IDAT chunks.  Every chunk
//   boundary is a candidate start of an independent deflate sequence.  png_segcount_kernel, one workgroup (one wave) per (image,
//   chunk): the chunk decoded stand-alone, nothing stored -> a record {bytes, status, saw BFINAL, ended exactly}.
//   png_segaccept_kernel: the image is accepted iff every record is clean and exact, only the last saw BFINAL and the counts sum
//   to H (1 + W C); a running sum gives the offsets.  png_segwrite_kernel: the accepted images' chunks decoded again, stored.
//   png_adler_kernel + png_verdict_kernel (pass 0): an accepted image whose Adler-32 or filter bytes are wrong is un-accepted.
// * The serial leg, always launched.  png_inflate_kernel, one workgroup (one wave) per image: exits at once for an accepted
//   image, else inflates the joined bodies.  png_adler_kernel, one workgroup per (image, 16 KB): partial sums and the two
//   facts about the filter bytes (one above 4; one above 1).  png_verdict_kernel, a thread per image: the partials combined in
//   order, compared with the file's; status, segmented and the unfilter kernel of the image.
// * png_unfilter_rows_kernel, one workgroup per (image, 8 rows): images whose rows are all None / Sub - Sub is a prefix sum
//   modulo 256 per channel.  png_unfilter_skew_kernel, one wave per image, every other image: bands of 64 rows, lane t on row
//   r0 + t and pixel s - t at step s, the pixel above and above left by a shuffle.  An image with a status: zeros.
// Scratch per image: the filtered stream, the Adler partials, the segment records and offsets, a control record.  LDS of the
// inflate kernels: PdShared (55852 bytes: the 48 KB ring, three tables, the code lengths, 64 token records).  No global atomics; no
// workgroup waits for another; no host synchronisation.
#include "common.h"
#include "block_scan.h"
#include "codec_host.h"
#include "pngdec_core.h"

namespace {

using namespace blockscan;
constexpr int kThreads = kScanThreads;
constexpr uint32_t kMagic = 0x50444543u;   // "PDEC"
constexpr int kAdlerChunk = 16384;         // bytes of one workgroup of png_adler_kernel: 256 threads x 64
constexpr int kRowsPerGroup = 8;
constexpr int kPixPerThread = 8;
constexpr int kCtlInts = 8;                // per image: accepted, serial status, mode, ...
enum { CTL_ACCEPTED = 0, CTL_SERIAL_STATUS = 1, CTL_MODE = 2 };

struct PngGeom {
  int64_t total;         // bytes of an image's filtered stream
  int64_t slot;          // ... rounded up
  int64_t nchunks;       // Adler partials of an image
  int64_t filt, part, rec, off, ctl, bytes;   // scratch offsets
  int64_t range_cap;     // IDAT chunks a file of max_file_bytes has at most
  int64_t staging;
};

bool png_geom(int batch, int H, int W, int C, int64_t max_file_bytes, PngGeom* g) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || (C != 1 && C != 3 && C != 4)) return false;
  g->total = (int64_t)H * (1 + (int64_t)W * C);
  if (g->total >= ((int64_t)1 << 31) - 65536) return false;
  g->slot = round16(g->total);
  g->nchunks = (g->total + kAdlerChunk - 1) / kAdlerChunk;
  int64_t o = 0;
  g->filt = o;
  o += (int64_t)batch * g->slot;
  g->part = o;
  o += round16((int64_t)batch * g->nchunks * 16);
  g->rec = o;
  o += (int64_t)batch * SFH_PNG_DEC_MAX_SEGMENTS * 16;
  g->off = o;
  o += (int64_t)batch * SFH_PNG_DEC_MAX_SEGMENTS * 4;
  g->ctl = o;
  o += round16((int64_t)batch * kCtlInts * 4);
  g->bytes = o;
  if (g->bytes >= ((int64_t)1 << 32)) return false;
  if (max_file_bytes < 0) return true;                   // the scratch alone
  if (max_file_bytes < 8 || max_file_bytes >= ((int64_t)1 << 28)) return false;
  g->range_cap = max_file_bytes / 12 + 1;
  g->staging = kStageHeadBytes + (int64_t)batch * ((int64_t)sizeof(sfh_png_info) + 12 * g->range_cap + 16 + round16(max_file_bytes) + 16);
  return g->staging < ((int64_t)1 << 31);
}

struct PngArgs {
  int H, W, C, bgr;
  int32_t total;
  int64_t slot, nchunks;
  int64_t filt, part, rec, off, ctl;
};

PngArgs png_args(const PngGeom& g, int H, int W, int C, int bgr) {
  PngArgs a;
  a.H = H;
  a.W = W;
  a.C = C;
  a.bgr = bgr;
  a.total = (int32_t)g.total;
  a.slot = g.slot;
  a.nchunks = g.nchunks;
  a.filt = g.filt;
  a.part = g.part;
  a.rec = g.rec;
  a.off = g.off;
  a.ctl = g.ctl;
  return a;
}

__device__ __forceinline__ const sfh_png_info* staged_info(const uint8_t* staged, int b) {
  return reinterpret_cast<const sfh_png_info*>(staged + kStageHeadBytes) + b;
}
__device__ __forceinline__ int32_t* ctl_of(uint8_t* scratch, const PngArgs& a, int b) {
  return reinterpret_cast<int32_t*>(scratch + a.ctl) + (int64_t)b * kCtlInts;
}
// chunks of the image that the segmented leg is tried on (0: none)
__device__ __forceinline__ int seg_count(const sfh_png_info* info) {
  return (info->nidat >= 2 && info->nidat <= SFH_PNG_DEC_MAX_SEGMENTS) ? info->nidat : 0;
}

__device__ __forceinline__ PdStream base_stream(const uint8_t* staged, const sfh_png_info* info) {
  PdStream s;
  s.file = staged + info->file_pos;
  s.file_bytes = info->file_bytes;
  s.ranges = reinterpret_cast<const int32_t*>(staged + info->range_pos);
  s.nranges = info->nidat;
  s.r0 = 0;
  s.skip = 2;
  s.len = info->idat_bytes - 6;
  return s;
}

// chunk `seg` as a stream of its own: its body without what it holds of the zlib header and of the Adler-32
__device__ __forceinline__ PdStream seg_stream(const uint8_t* staged, const sfh_png_info* info, int seg) {
  PdStream s = base_stream(staged, info);
  const int32_t* joined = reinterpret_cast<const int32_t*>(staged + info->joined_pos);
  const int32_t l0 = joined[seg], l1 = joined[seg] + (s.ranges[2 * seg + 1] - s.ranges[2 * seg]);
  const int32_t lo = l0 > 2 ? l0 : 2, hi = l1 < info->idat_bytes - 4 ? l1 : info->idat_bytes - 4;
  s.r0 = seg;
  s.skip = lo - l0;
  s.len = hi - lo;
  return s;
}

__global__ __launch_bounds__(kPdLanes) void png_segcount_kernel(const uint8_t* __restrict__ staged, PngArgs a,
                                                                uint8_t* __restrict__ scratch) {
  __shared__ PdShared sh;
  const int seg = blockIdx.x, b = blockIdx.y;
  const sfh_png_info* info = staged_info(staged, b);
  if (seg >= seg_count(info)) return;                    // uniform over the workgroup
  const PdStream s = seg_stream(staged, info, seg);
  PdResult res;
  pd_inflate(s, sh, nullptr, 0, a.total, res);
  if (threadIdx.x == 0) {
    int32_t* rec = reinterpret_cast<int32_t*>(scratch + a.rec) + ((int64_t)b * SFH_PNG_DEC_MAX_SEGMENTS + seg) * 4;
    rec[0] = res.produced;
    rec[1] = res.status;
    rec[2] = res.final_seen;
    rec[3] = res.exact;
  }
}

__global__ __launch_bounds__(kPdLanes) void png_segaccept_kernel(const uint8_t* __restrict__ staged, PngArgs a, int batch,
                                                                 uint8_t* __restrict__ scratch) {
  const int b = blockIdx.x * kPdLanes + threadIdx.x;
  if (b >= batch) return;
  const int nseg = seg_count(staged_info(staged, b));
  const int32_t* rec = reinterpret_cast<const int32_t*>(scratch + a.rec) + (int64_t)b * SFH_PNG_DEC_MAX_SEGMENTS * 4;
  int32_t* off = reinterpret_cast<int32_t*>(scratch + a.off) + (int64_t)b * SFH_PNG_DEC_MAX_SEGMENTS;
  bool ok = nseg > 0;
  int64_t sum = 0;
  for (int s = 0; s < nseg; ++s) {
    off[s] = (int32_t)(sum < a.total ? sum : a.total);
    ok = ok && rec[4 * s + 1] == 0 && rec[4 * s + 3] == 1 && rec[4 * s + 2] == (s == nseg - 1 ? 1 : 0);
    sum += rec[4 * s];
  }
  ctl_of(scratch, a, b)[CTL_ACCEPTED] = (ok && sum == a.total) ? 1 : 0;
}

__global__ __launch_bounds__(kPdLanes) void png_segwrite_kernel(const uint8_t* __restrict__ staged, PngArgs a,
                                                                uint8_t* __restrict__ scratch) {
  __shared__ PdShared sh;
  const int seg = blockIdx.x, b = blockIdx.y;
  const sfh_png_info* info = staged_info(staged, b);
  if (seg >= seg_count(info) || ctl_of(scratch, a, b)[CTL_ACCEPTED] == 0) return;
  const PdStream s = seg_stream(staged, info, seg);
  const int32_t off = (reinterpret_cast<const int32_t*>(scratch + a.off) + (int64_t)b * SFH_PNG_DEC_MAX_SEGMENTS)[seg];
  const int32_t n = (reinterpret_cast<const int32_t*>(scratch + a.rec) + ((int64_t)b * SFH_PNG_DEC_MAX_SEGMENTS + seg) * 4)[0];
  int32_t cap = a.total - off;                           // accepted: off + n <= total
  cap = cap < n ? cap : n;
  PdResult res;
  pd_inflate(s, sh, scratch + a.filt + (int64_t)b * a.slot + off, cap, n, res);
}

__global__ __launch_bounds__(kPdLanes) void png_inflate_kernel(const uint8_t* __restrict__ staged, PngArgs a,
                                                               uint8_t* __restrict__ scratch) {
  __shared__ PdShared sh;
  const int b = blockIdx.x;
  int32_t* ctl = ctl_of(scratch, a, b);
  if (ctl[CTL_ACCEPTED] != 0) return;
  const sfh_png_info* info = staged_info(staged, b);
  const PdStream s = base_stream(staged, info);
  PdResult res;
  pd_inflate(s, sh, scratch + a.filt + (int64_t)b * a.slot, a.total, a.total, res);
  if (threadIdx.x == 0) {
    int st = res.status;
    if (!st && !res.final_seen) st |= PD_E_EOF;
    if (!st && res.produced != a.total) st |= PD_E_SIZE;
    ctl[CTL_SERIAL_STATUS] = st;
  }
}

// pass 0: the images the segmented leg accepted; pass 1: the others
__global__ __launch_bounds__(kThreads) void png_adler_kernel(PngArgs a, int pass, uint8_t* __restrict__ scratch) {
  __shared__ int tmp[4];
  const int t = threadIdx.x, b = blockIdx.y;
  if ((ctl_of(scratch, a, b)[CTL_ACCEPTED] != 0) != (pass == 0)) return;
  const uint8_t* f = scratch + a.filt + (int64_t)b * a.slot;
  const int64_t c0 = (int64_t)blockIdx.x * kAdlerChunk;
  const int n = (int)(a.total - c0 < kAdlerChunk ? a.total - c0 : kAdlerChunk);   // bytes of this chunk
  const int i0 = t * 64;
  uint32_t sa = 0, sb = 0;
  if (i0 < n) {
    const int i1 = i0 + 64 < n ? i0 + 64 : n;
    if (i1 - i0 == 64) {                                   // c0 + i0 is a multiple of 16, and so is the slot
      const uint4* p = reinterpret_cast<const uint4*>(f + c0 + i0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 v = p[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const uint32_t d = (w[j >> 2] >> (8 * (j & 3))) & 255u;
          sa += d;
          sb += (uint32_t)(n - (i0 + 16 * q + j)) * d;   // <= 16384 * 255 * 64
        }
      }
    } else {
      for (int i = i0; i < i1; ++i) {
        const uint32_t d = f[c0 + i];
        sa += d;
        sb += (uint32_t)(n - i) * d;
      }
    }
    // the filter bytes among the thread's bytes
    const int64_t stride = 1 + (int64_t)a.W * a.C;
    const int64_t g0 = c0 + i0, g1 = c0 + i1;
    const int64_t r = g0 % stride;
    int flags = 0;
    for (int64_t g = r ? g0 + stride - r : g0; g < g1; g += stride) {
      const int v = f[g];
      flags |= (v > 4 ? 1 : 0) | (v > 1 ? 2 : 0);
    }
    sb = (sb % 65521u) | ((uint32_t)flags << 16);        // sums of 256 of these stay apart
  }
  int ta, tb;
  block_scan_excl<OP_SUM, false>((int)sa, 0, tmp, ta);  // <= 16384 * 255
  __syncthreads();
  block_scan_excl<OP_SUM, false>((int)(sb & 0xFFFFu), 0, tmp, tb);
  __syncthreads();
  int f1, f2;
  block_scan_excl<OP_MAX, false>((int)((sb >> 16) & 1u), 0, tmp, f1);
  __syncthreads();
  block_scan_excl<OP_MAX, false>((int)((sb >> 17) & 1u), 0, tmp, f2);
  if (t == 0) {
    uint32_t* part = reinterpret_cast<uint32_t*>(scratch + a.part) + ((int64_t)b * a.nchunks + blockIdx.x) * 4;
    part[0] = (uint32_t)ta % 65521u;
    part[1] = (uint32_t)tb % 65521u;
    part[2] = (uint32_t)n;
    part[3] = (uint32_t)(f1 | (f2 << 1));
  }
}

__global__ __launch_bounds__(kPdLanes) void png_verdict_kernel(const uint8_t* __restrict__ staged, PngArgs a, int batch, int pass,
                                                               uint8_t* __restrict__ scratch, int32_t* __restrict__ status,
                                                               int32_t* __restrict__ segmented) {
  const int b = blockIdx.x * kPdLanes + threadIdx.x;
  if (b >= batch) return;
  int32_t* ctl = ctl_of(scratch, a, b);
  if ((ctl[CTL_ACCEPTED] != 0) != (pass == 0)) return;
  const uint32_t* part = reinterpret_cast<const uint32_t*>(scratch + a.part) + (int64_t)b * a.nchunks * 4;
  uint32_t sa = 1, sb = 0, flags = 0;
  for (int64_t c = 0; c < a.nchunks; ++c) {              // in order; the arithmetic of sfh_png_pack
    const uint32_t n = part[4 * c + 2] % 65521u;
    sb = (sb + (uint32_t)(((uint64_t)n * sa) % 65521u) + part[4 * c + 1]) % 65521u;
    sa = (sa + part[4 * c]) % 65521u;
    flags |= part[4 * c + 3];
  }
  int st = pass == 0 ? 0 : ctl[CTL_SERIAL_STATUS];
  if (!st) {
    if (((sb << 16) | sa) != staged_info(staged, b)->adler) st |= PD_E_ADLER;
    if (flags & 1u) st |= PD_E_FILTER;
  }
  if (pass == 0 && st) {                                 // a false acceptance: the serial leg decides
    ctl[CTL_ACCEPTED] = 0;
    return;
  }
  ctl[CTL_MODE] = (flags & 2u) ? 1 : 0;
  status[b] = st;
  segmented[b] = pass == 0 ? 1 : 0;
}

__device__ __forceinline__ int64_t out_index(const PngArgs& a, int b, int y, int x) {
  return (((int64_t)b * a.H + y) * a.W + x) * a.C;
}

__global__ __launch_bounds__(kThreads) void png_unfilter_rows_kernel(PngArgs a, const uint8_t* __restrict__ scratch,
                                                                     const int32_t* __restrict__ status, uint8_t* __restrict__ out) {
  __shared__ int tmp[4];
  const int t = threadIdx.x, b = blockIdx.y;
  const bool bad = status[b] != 0;
  const int mode = (reinterpret_cast<const int32_t*>(scratch + a.ctl) + (int64_t)b * kCtlInts)[CTL_MODE];
  if (!bad && mode != 0) return;                         // uniform: the skew kernel's image
  const int C = a.C, W = a.W;
  const int64_t stride = 1 + (int64_t)W * C;
  const uint8_t* f = scratch + a.filt + (int64_t)b * a.slot;
  int oc[4];
  for (int k = 0; k < 4; ++k) oc[k] = pd_out_channel(k, C, a.bgr);
  const int y1 = (blockIdx.x + 1) * kRowsPerGroup < a.H ? (blockIdx.x + 1) * kRowsPerGroup : a.H;
  for (int y = blockIdx.x * kRowsPerGroup; y < y1; ++y) {
    const uint8_t* row = f + (int64_t)y * stride;
    const int ft = bad ? 0 : row[0];
    int carry[4] = {0, 0, 0, 0};
    for (int x0 = 0; x0 < W; x0 += kThreads * kPixPerThread) {   // uniform trip count
      const int xa = x0 + t * kPixPerThread;
      int v[kPixPerThread][4];
      int sum[4] = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < kPixPerThread; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < C) {
            const int d = (!bad && xa + i < W) ? row[1 + (int64_t)(xa + i) * C + k] : 0;
            sum[k] += d;
            v[i][k] = ft == 1 ? sum[k] : d;              // Sub: the inclusive sum within the thread
          }
      if (ft == 1) {                                       // uniform
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < C) {
            int tot;
            const int ex = block_scan_excl<OP_SUM, false>(sum[k], 0, tmp, tot);
            const int add = carry[k] + ex;
#pragma unroll
            for (int i = 0; i < kPixPerThread; ++i) v[i][k] += add;
            carry[k] = (carry[k] + tot) & 255;
          }
      }
#pragma unroll
      for (int i = 0; i < kPixPerThread; ++i)
        if (xa + i < W) {
          uint8_t* p = out + out_index(a, b, y, xa + i);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < C) p[oc[k]] = (uint8_t)(v[i][k] & 255);
        }
    }
  }
}

__device__ __forceinline__ uint32_t load_px(const uint8_t* p, int C) {
  uint32_t v = 0;
  for (int k = 0; k < C; ++k) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

__global__ __launch_bounds__(kPdLanes) void png_unfilter_skew_kernel(PngArgs a, const uint8_t* __restrict__ scratch,
                                                                     const int32_t* __restrict__ status, uint8_t* out) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const int mode = (reinterpret_cast<const int32_t*>(scratch + a.ctl) + (int64_t)b * kCtlInts)[CTL_MODE];
  if (status[b] != 0 || mode != 1) return;               // uniform
  const int C = a.C, W = a.W, H = a.H;
  const int64_t stride = 1 + (int64_t)W * C;
  const uint8_t* f = scratch + a.filt + (int64_t)b * a.slot;
  int oc[4];
  for (int k = 0; k < 4; ++k) oc[k] = pd_out_channel(k, C, a.bgr);
  for (int r0 = 0; r0 < H; r0 += kPdLanes) {
    const int y = r0 + lane;
    const bool live = y < H;
    const uint8_t* row = f + (int64_t)(live ? y : 0) * stride;
    const int ft = live ? row[0] : 0;
    uint32_t prev1 = 0, prev2 = 0, upc = 0;
    for (int s = 0; s < W + kPdLanes - 1; ++s) {
      const int x = s - lane;
      uint32_t pb = __shfl_up(prev1, 1), pc = __shfl_up(prev2, 1);
      if (lane == 0) {
        pc = upc;
        pb = 0;
        if (r0 > 0 && x < W) {                             // the last row of the band before, from the output
          const uint8_t* p = out + out_index(a, b, r0 - 1, x);
          for (int k = 0; k < C; ++k) pb |= (uint32_t)p[oc[k]] << (8 * k);
        }
        upc = pb;
      }
      uint32_t cur = 0;
      if (live && x >= 0 && x < W) {
        cur = pd_recon(ft, load_px(row + 1 + (int64_t)x * C, C), prev1, pb, pc, C);
        uint8_t* p = out + out_index(a, b, y, x);
        for (int k = 0; k < C; ++k) p[oc[k]] = (uint8_t)(cur >> (8 * k));
      }
      prev2 = prev1;
      prev1 = cur;
    }
    __syncthreads();                                       // the band's last row is read by lane 0 of the next
  }
}

}  // namespace

extern "C" int sfh_png_parse(const uint8_t* host_bytes, int64_t n, sfh_png_info* host_info, int32_t* host_ranges, int64_t range_cap) {
  SFH_REQUIRE(host_bytes && host_info && n >= 0 && range_cap >= 0 && (host_ranges || range_cap == 0),
              "png_parse: null pointer or negative size");
  const int rc = pd_parse(host_bytes, n, host_info, host_ranges, range_cap);
  if (rc) sfh_set_error("png_parse: refused, reason %d", host_info->reason);
  return rc;
}

extern "C" int64_t sfh_png_dec_staging_bytes(int batch, int H, int W, int C, int64_t max_file_bytes) {
  PngGeom g;
  if (max_file_bytes < 0 || !png_geom(batch, H, W, C, max_file_bytes, &g)) {
    sfh_set_error("png_dec_staging_bytes: batch %d image %dx%dx%d files of %lld bytes", batch, W, H, C, (long long)max_file_bytes);
    return -1;
  }
  return g.staging;
}

extern "C" int64_t sfh_png_dec_scratch_bytes(int batch, int H, int W, int C) {
  PngGeom g;
  if (!png_geom(batch, H, W, C, -1, &g)) {
    sfh_set_error("png_dec_scratch_bytes: batch %d image %dx%dx%d", batch, W, H, C);
    return -1;
  }
  return g.bytes;
}

extern "C" int64_t sfh_png_dec_stage(const uint8_t* const* host_files, const int64_t* host_sizes, int batch, int H, int W, int C,
                                     int64_t max_file_bytes, uint8_t* host_staging, int64_t staging_bytes, int32_t* host_reason,
                                     int32_t* host_index) {
  PngGeom g;
  const int64_t need = max_file_bytes >= 0 && png_geom(batch, H, W, C, max_file_bytes, &g) ? g.staging : -1;
  if (!stage_begin("png_dec_stage", host_files, host_sizes, host_staging, staging_bytes, need, host_reason, host_index)) return -1;
  sfh_png_info* infos = reinterpret_cast<sfh_png_info*>(host_staging + kStageHeadBytes);
  int64_t pos = kStageHeadBytes + (int64_t)batch * (int64_t)sizeof(sfh_png_info);
  int max_idat = 0;
  for (int b = 0; b < batch; ++b) {
    sfh_png_info* info = infos + b;
    int32_t* ranges = reinterpret_cast<int32_t*>(host_staging + pos);
    int reason = stage_file_reason(host_files[b], host_sizes[b], max_file_bytes, SFH_PNG_R_TRUNCATED, SFH_PNG_R_TOO_LONG);
    if (reason == SFH_PNG_R_OK) {
      if (pd_parse(host_files[b], host_sizes[b], info, ranges, g.range_cap)) reason = info->reason;
      else if (info->width != W || info->height != H || info->channels != C || info->nidat > g.range_cap) reason = SFH_PNG_R_SIZE;
    }
    if (reason != SFH_PNG_R_OK) return stage_refuse_file("png_dec_stage", b, reason, host_reason, host_index);
    info->range_pos = (int32_t)pos;
    pos += 8 * (int64_t)info->nidat;
    int32_t* joined = reinterpret_cast<int32_t*>(host_staging + pos);
    info->joined_pos = (int32_t)pos;
    int32_t at = 0;
    for (int r = 0; r < info->nidat; ++r) {
      joined[r] = at;
      at += ranges[2 * r + 1] - ranges[2 * r];
    }
    pos = round16(pos + 4 * (int64_t)info->nidat);
    max_idat = info->nidat > max_idat ? info->nidat : max_idat;
  }
  pos = stage_copy_files(infos, host_files, host_sizes, batch, host_staging, pos);
  stage_head(host_staging, kMagic, batch, max_idat)[3] = (uint32_t)pos;
  return pos;
}

extern "C" int sfh_png_decode(const uint8_t* host_staging, const uint8_t* staged, int64_t staged_bytes, int batch, int H, int W, int C,
                              int bgr, int64_t max_file_bytes, int serial_only, uint8_t* scratch, int64_t scratch_bytes, uint8_t* out,
                              int32_t* status, int32_t* segmented, void* stream) {
  PngGeom g;
  SFH_REQUIRE(max_file_bytes >= 0 && png_geom(batch, H, W, C, max_file_bytes, &g), "png_decode: batch %d image %dx%dx%d", batch, W, H, C);
  SFH_REQUIRE(out && status && segmented, "png_decode: null pointer (out, status, segmented)");
  if (int rc = decode_begin("png_decode", "sfh_png_dec_stage", host_staging, staged, staged_bytes, scratch, scratch_bytes, g.bytes,
                            kMagic, batch, g.range_cap, 3))
    return rc;
  const uint32_t* head = reinterpret_cast<const uint32_t*>(host_staging);
  hipStream_t st = (hipStream_t)stream;
  const PngArgs a = png_args(g, H, W, C, bgr ? 1 : 0);
  const hipError_t e = hipMemsetAsync(scratch + g.ctl, 0, (size_t)batch * kCtlInts * 4, st);
  if (e != hipSuccess) {
    sfh_set_error("png_decode: hipMemsetAsync: %s", hipGetErrorString(e));
    return SFH_E_LAUNCH;
  }
  const dim3 per_image((unsigned)sfh_cdiv(batch, kPdLanes));
  const dim3 adler_grid((unsigned)g.nchunks, (unsigned)batch);
  // the largest IDAT count of the batch decides whether the segmented leg is launched at all; files with more chunks than
  // SFH_PNG_DEC_MAX_SEGMENTS take the serial leg, so the grid stops there
  const unsigned nseg = head[2] > (uint32_t)SFH_PNG_DEC_MAX_SEGMENTS ? (unsigned)SFH_PNG_DEC_MAX_SEGMENTS : head[2];
  if (nseg >= 2 && !serial_only) {
    hipLaunchKernelGGL(png_segcount_kernel, dim3(nseg, (unsigned)batch), dim3(kPdLanes), 0, st, staged, a, scratch);
    if (int rc = sfh_check_launch("png_segcount_kernel")) return rc;
    hipLaunchKernelGGL(png_segaccept_kernel, per_image, dim3(kPdLanes), 0, st, staged, a, batch, scratch);
    if (int rc = sfh_check_launch("png_segaccept_kernel")) return rc;
    hipLaunchKernelGGL(png_segwrite_kernel, dim3(nseg, (unsigned)batch), dim3(kPdLanes), 0, st, staged, a, scratch);
    if (int rc = sfh_check_launch("png_segwrite_kernel")) return rc;
    hipLaunchKernelGGL(png_adler_kernel, adler_grid, dim3(kThreads), 0, st, a, 0, scratch);
    if (int rc = sfh_check_launch("png_adler_kernel")) return rc;
    hipLaunchKernelGGL(png_verdict_kernel, per_image, dim3(kPdLanes), 0, st, staged, a, batch, 0, scratch, status, segmented);
    if (int rc = sfh_check_launch("png_verdict_kernel")) return rc;
  }
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)batch), dim3(kPdLanes), 0, st, staged, a, scratch);
  if (int rc = sfh_check_launch("png_inflate_kernel")) return rc;
  hipLaunchKernelGGL(png_adler_kernel, adler_grid, dim3(kThreads), 0, st, a, 1, scratch);
  if (int rc = sfh_check_launch("png_adler_kernel")) return rc;
  hipLaunchKernelGGL(png_verdict_kernel, per_image, dim3(kPdLanes), 0, st, staged, a, batch, 1, scratch, status, segmented);
  if (int rc = sfh_check_launch("png_verdict_kernel")) return rc;
  hipLaunchKernelGGL(png_unfilter_rows_kernel, dim3((unsigned)sfh_cdiv(H, kRowsPerGroup), (unsigned)batch), dim3(kThreads), 0, st, a,
                     scratch, status, out);
  if (int rc = sfh_check_launch("png_unfilter_rows_kernel")) return rc;
  hipLaunchKernelGGL(png_unfilter_skew_kernel, dim3((unsigned)batch), dim3(kPdLanes), 0, st, a, scratch, status, out);
  return sfh_check_launch("png_unfilter_skew_kernel");
}
