// pngenc.hip - standard PNG files from uint8 device images in two launches (sfh_amd.pngenc; the rule is restated in
// tests/pngenc_ref.py and the two agree byte for byte).
//
// The format is built from pieces every inflater accepts: 8-bit gray / RGB, filter 1 (Sub) on every scanline, the filtered
// stream cut into STRIPS of R = max(1, min(16, 32768 / (1 + W C))) rows, each strip one fixed-Huffman deflate block whose tokens
// are the maximal runs of equal bytes (first byte a literal, the rest distance-1 matches of at most 258 while at least 3 remain,
// a remainder of 1 or 2 as literals).  A strip that is not the last ends with an empty stored block (the sync flush of parallel
// gzip writers), so every strip is a whole number of bytes and strips concatenate; a strip whose fixed form would be longer than
// its bytes + 5 is one stored block instead.  One IDAT chunk per strip.
//
// * png_encode_kernel, one workgroup per (image, strip): Sub in registers -> the strip in LDS; every thread owns a contiguous
//   segment of it (4 * odd bytes: consecutive threads start on different banks); run starts by neighbour comparison; run
//   extents by a forward max-scan of "last start" and a backward min-scan of "first start" over the workgroup; token bit lengths,
//   their prefix sum, then the code bits OR-ed into an LDS image of the whole chunk (disjoint bits: the result does not depend
//   on the order); fixed or stored is decided from the bit total BEFORE anything is written, so the LDS chunk never exceeds
//   strip + 5 + headers.  CRC-32 of the chunk: per-thread table CRCs of equal sub-segments (the message is thought left-padded
//   with zeros to 256 equal pieces: leading zeros do not change a CRC register that starts at 0), combined pairwise in fixed
//   order with x^(8 len) mod P.  The chunk goes to the strip's fixed-stride slot of the scratch buffer as dwords; its byte
//   count, the strip's Adler-32 partial sums and (last strip) the CRC register go to a 16-byte meta record.
// * png_pack_kernel, one workgroup per image: scan of the strip byte counts, signature + IHDR, the strips copied to their
//   offsets, the Adler partials combined in strip order (a scan, no serial walk), the last chunk's Adler-32 and CRC, IEND,
//   sizes[b], offsets[b].  compact: image b starts at the sum of the sizes of the images before it, which every workgroup
//   computes for itself from the meta records - no third launch, no communication between workgroups.
// No global atomics anywhere; the same bytes every run.
#include "common.h"
#include "codec_common.h"
#include "codec_host.h"
#include "codec_pack.h"

namespace {

using namespace codecpack;
constexpr int kThreads = kScanThreads;
constexpr int kMaxRow = SFH_PNG_MAX_ROW;
constexpr int kStripRows = SFH_PNG_STRIP_ROWS;
constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kAdler = 65521u;
constexpr int kFixedFile = 8 + 25 + 12;   // signature, IHDR, IEND

struct PngHead {
  uint8_t b[36];   // signature + IHDR chunk (33 bytes)
};

inline int strip_rows(int W, int C) {
  const int r = kMaxRow / (1 + W * C);
  return r < 1 ? 1 : (r > kStripRows ? kStripRows : r);
}
// a strip's slot in the scratch buffer: chunk header 8, zlib header 2, stored header 5, the bytes, Adler 4, CRC 4
inline int slot_stride(int R, int rowlen) { return round16(8 + 2 + 5 + R * rowlen + 4 + 4); }
inline int raw_lds_bytes(int R, int rowlen) { return round16(R * rowlen + 4); }
constexpr int kTableBytes = 256 * 4 + kThreads * 4 + 16;   // CRC table, CRC partials, the scans' four wave results

// a * b mod P over GF(2), reflected representation (x^0 = 0x80000000): the operator of zlib's crc32_combine
__device__ __forceinline__ uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (int i = 31; i >= 0; --i) {
    p ^= ((a >> i) & 1u) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  }
  return p;
}

// x^(8 n) mod P: what n zero bytes do to a CRC register
__device__ __forceinline__ uint32_t gf2_x8n(uint32_t n) {
  uint32_t r = 0x80000000u, base = 0x00800000u;   // x^0, x^8
  while (n) {
    if (n & 1u) r = gf2_mulmod(r, base);
    n >>= 1;
    if (n) base = gf2_mulmod(base, base);
  }
  return r;
}

__device__ __forceinline__ uint32_t crc_step_bits(uint32_t c, uint32_t byte) {
  c ^= byte;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kPoly : 0u);
  return c;
}

struct Tok {
  uint32_t code;   // bits in stream order, first bit in bit 0
  int nbits;
};

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, int n) { return __brev(v) >> (32 - n); }

__device__ __forceinline__ Tok lit_token(uint32_t v) {
  Tok t;
  if (v < 144u) {
    t.code = rev_bits(0x30u + v, 8);
    t.nbits = 8;
  } else {
    t.code = rev_bits(0x190u + (v - 144u), 9);
    t.nbits = 9;
  }
  return t;
}

// length 3 .. 258 at distance 1: length symbol, its extra bits, the 5-bit distance code 0
__device__ __forceinline__ Tok match_token(int len) {
  int sym, eb = 0;
  uint32_t extra = 0;
  if (len == 258) {
    sym = 285;
  } else if (len <= 10) {
    sym = 254 + len;
  } else {
    const int l = len - 3;                       // 8 .. 254
    eb = (31 - __clz(l)) - 2;
    sym = 261 + 4 * eb + ((l >> eb) & 3);
    extra = (uint32_t)l & ((1u << eb) - 1u);
  }
  Tok t;
  int hb;
  if (sym < 280) {
    t.code = rev_bits((uint32_t)(sym - 256), 7);
    hb = 7;
  } else {
    t.code = rev_bits(0xC0u + (uint32_t)(sym - 280), 8);
    hb = 8;
  }
  t.code |= extra << hb;
  t.nbits = hb + eb + 5;
  return t;
}

template <bool EMIT>
__device__ __forceinline__ void put(const Tok& t, uint32_t* chunk, uint32_t& bitpos) {
  if (EMIT) {
    const uint32_t w = bitpos >> 5, sh = bitpos & 31u;
    const uint64_t v = (uint64_t)t.code << sh;
    atomicOr(&chunk[w], (uint32_t)v);
    if ((uint32_t)(v >> 32)) atomicOr(&chunk[w + 1], (uint32_t)(v >> 32));
  }
  bitpos += (uint32_t)t.nbits;
}

// The tokens that START inside [seg0, seg1) of the strip raw[0, N), in stream order.  s_in: start of the run that holds byte
// seg0 - 1; e_out: first run start at or after seg1 (N if none).  Returns the bit position after the last token.
template <bool EMIT>
__device__ __forceinline__ uint32_t walk_tokens(const uint8_t* raw, int seg0, int seg1, int s_in, int e_out, uint32_t* chunk,
                                                uint32_t bitpos) {
  int p = seg0, s = s_in;
  while (p < seg1) {
    const uint32_t v = raw[p];
    if (p == 0 || raw[p - 1] != v) s = p;
    int q = p + 1;
    while (q < seg1 && raw[q] == v) ++q;
    const int e = q < seg1 ? q : e_out;          // the run is [s, e)
    const int n = e - s - 1;                     // bytes after the first
    const int k0 = p - s, k1 = q - s;            // this piece of the run, as offsets in the run
    if (k0 == 0) put<EMIT>(lit_token(v), chunk, bitpos);
    int nmatch = 0, tail = n;                    // match i starts at offset 1 + 258 i; `tail` literals end the run
    if (n >= 3) {
      const int full = n / 258, rem = n - full * 258;
      nmatch = full + (rem >= 3 ? 1 : 0);
      tail = rem >= 3 ? 0 : rem;
    }
    const int lo = k0 > 1 ? k0 : 1;
    for (int i = (lo - 1 + 257) / 258; i < nmatch && 1 + 258 * i < k1; ++i) {
      const int left = n - 258 * i;
      put<EMIT>(match_token(left < 258 ? left : 258), chunk, bitpos);
    }
    for (int k = n + 1 - tail; k <= n; ++k)
      if (k >= lo && k < k1) put<EMIT>(lit_token(v), chunk, bitpos);
    p = q;
  }
  return bitpos;
}

extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];

// meta record of a strip: {chunk bytes, Adler sum a, Adler sum b, CRC register (last strip: before the Adler bytes)}
__global__ __launch_bounds__(kThreads) void png_encode_kernel(const uint8_t* __restrict__ images, int H, int W, int C, int bgr,
                                                              int R, int nstrips, int raw_bytes, int stride,
                                                              uint32_t* __restrict__ meta, uint8_t* __restrict__ slots) {
  const int t = threadIdx.x;
  const int strip = blockIdx.x, b = blockIdx.y;
  const int rowlen = 1 + W * C;
  const int row0 = strip * R;
  const int rows = H - row0 < R ? H - row0 : R;
  const int N = rows * rowlen;                                   // 1 .. 32768
  const bool first = strip == 0, last = strip == nstrips - 1;
  uint8_t* raw = png_lds;
  uint32_t* chunk = reinterpret_cast<uint32_t*>(png_lds + raw_bytes);
  uint8_t* chunk8 = png_lds + raw_bytes;
  const int chunk_words = stride / 4 + 4;                        // + the word a token's upper half may touch
  // the tables follow the chunk in the dynamic region: a kernel with no static LDS may raise its dynamic limit to the whole 160 KB
  uint32_t* crc_tab = chunk + chunk_words;
  uint32_t* crc_part = crc_tab + 256;
  int* tmp = reinterpret_cast<int*>(crc_part + kThreads);

  {   // CRC table, a zeroed chunk image
    uint32_t c = (uint32_t)t;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kPoly : 0u);
    crc_tab[t] = c;
    for (int w = t; w < chunk_words; w += kThreads) chunk[w] = 0u;
  }

  // ---- 1. the strip's filtered bytes: four consecutive stream positions per lane and step, one LDS dword
  const uint8_t* img = images + ((size_t)b * H + row0) * (size_t)W * C;
  for (int p4 = t * 4; p4 < N; p4 += kThreads * 4) {
    int r = p4 / rowlen, c = p4 - r * rowlen;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (p4 + j < N) {
        uint32_t v = 1u;                                          // filter type Sub
        if (c > 0) {
          const int i = c - 1;
          const int x = C == 3 ? i / 3 : i, ch = C == 3 ? i - x * 3 : 0;
          const int sc = (C == 3 && bgr) ? 2 - ch : ch;
          const uint8_t* px = img + ((size_t)r * W + x) * C + sc;
          v = (uint32_t)px[0] - (x > 0 ? (uint32_t)px[-C] : 0u);
        }
        word |= (v & 255u) << (8 * j);
        if (++c == rowlen) {
          c = 0;
          ++r;
        }
      }
    }
    *reinterpret_cast<uint32_t*>(raw + p4) = word;
  }
  __syncthreads();

  // ---- 2. run starts in the thread's segment, Adler sums
  const int K = 4 * (((N + kThreads * 4 - 1) / (kThreads * 4)) | 1);      // 4 * odd >= N / 256
  const int seg0 = t * K < N ? t * K : N;
  const int seg1 = seg0 + K < N ? seg0 + K : N;
  int last_start = -1, first_start = N;
  uint32_t s1 = 0, s2 = 0;
  {
    uint32_t prev = seg0 > 0 ? raw[seg0 - 1] : 0u;
    for (int p = seg0; p < seg1; ++p) {
      const uint32_t d = raw[p];
      if (p == 0 || d != prev) {
        if (first_start == N) first_start = p;
        last_start = p;
      }
      prev = d;
      s1 += d;
      s2 += (uint32_t)(N - p) * d;                                // K * 255 * 32768 < 2^32
    }
  }
  int unused;
  const int s_in = block_scan_excl<OP_MAX, false>(last_start, -1, tmp, unused);
  const int e_out = block_scan_excl<OP_MIN, true>(first_start, N, tmp, unused);
  int adler_a, adler_b;
  block_scan_excl<OP_SUM, false>((int)s1, 0, tmp, adler_a);      // 32768 * 255 < 2^31
  block_scan_excl<OP_SUM, false>((int)(s2 % kAdler), 0, tmp, adler_b);

  // ---- 3. bit lengths and their prefix sum; fixed or stored
  const uint32_t mybits = walk_tokens<false>(raw, seg0, seg1, s_in, e_out, nullptr, 0u);
  int total_bits;
  const int bit_excl = block_scan_excl<OP_SUM, false>((int)mybits, 0, tmp, total_bits);
  const int hdr = 8 + (first ? 2 : 0);                            // chunk length, "IDAT", zlib header
  const int fixed_len = last ? (3 + total_bits + 7 + 7) / 8 : (3 + total_bits + 7 + 3 + 7) / 8 + 4;
  const bool fixed = fixed_len <= N + 5;
  const int body_len = fixed ? fixed_len : N + 5;
  const int data_len = (first ? 2 : 0) + body_len + (last ? 4 : 0);

  // ---- 4. the chunk image in LDS
  if (fixed) {
    walk_tokens<true>(raw, seg0, seg1, s_in, e_out, chunk, (uint32_t)(hdr * 8 + 3 + bit_excl));
    if (t == 0) atomicOr(&chunk[hdr / 4], ((last ? 1u : 0u) | 2u) << ((hdr & 3) * 8));   // BFINAL, BTYPE 01
  } else {
    for (int p = t; p < N; p += kThreads) chunk8[hdr + 5 + p] = raw[p];
  }
  __syncthreads();
  if (t == 0) {
    chunk8[0] = (uint8_t)(data_len >> 24);
    chunk8[1] = (uint8_t)(data_len >> 16);
    chunk8[2] = (uint8_t)(data_len >> 8);
    chunk8[3] = (uint8_t)data_len;
    chunk8[4] = 'I';
    chunk8[5] = 'D';
    chunk8[6] = 'A';
    chunk8[7] = 'T';
    if (first) {
      chunk8[8] = 0x78;
      chunk8[9] = 0x01;
    }
    if (fixed) {
      if (!last) {                                                // the empty stored block's LEN 0000 / NLEN FFFF
        chunk8[hdr + fixed_len - 2] = 0xFF;
        chunk8[hdr + fixed_len - 1] = 0xFF;
      }
    } else {
      chunk8[hdr] = last ? 1 : 0;
      chunk8[hdr + 1] = (uint8_t)N;
      chunk8[hdr + 2] = (uint8_t)(N >> 8);
      chunk8[hdr + 3] = (uint8_t)~N;
      chunk8[hdr + 4] = (uint8_t)(~N >> 8);
    }
  }
  __syncthreads();

  // ---- 5. CRC-32 over tag + data (the last strip: up to the Adler bytes, which the pack kernel appends)
  const int crc_len = 4 + (first ? 2 : 0) + body_len;
  const int m = 4 * (((crc_len + kThreads * 4 - 1) / (kThreads * 4)) | 1);
  {
    const int pad = kThreads * m - crc_len;
    int i0 = t * m - pad, i1 = i0 + m;
    if (i0 < 0) i0 = 0;
    uint32_t c = 0;
    for (int i = i0; i < i1; ++i) c = crc_tab[(c ^ chunk8[4 + i]) & 255u] ^ (c >> 8);
    crc_part[t] = c;
  }
  uint32_t pw = gf2_x8n((uint32_t)m);
  for (int d = 1; d < kThreads; d <<= 1) {
    __syncthreads();
    if ((t & (2 * d - 1)) == 0) crc_part[t] = gf2_mulmod(crc_part[t], pw) ^ crc_part[t + d];
    pw = gf2_mulmod(pw, pw);
  }
  __syncthreads();
  const uint32_t reg = gf2_mulmod(0xFFFFFFFFu, gf2_x8n((uint32_t)crc_len)) ^ crc_part[0];
  if (t == 0 && !last) {
    const uint32_t crc = ~reg;
    uint8_t* o = chunk8 + 4 + crc_len;
    o[0] = (uint8_t)(crc >> 24);
    o[1] = (uint8_t)(crc >> 16);
    o[2] = (uint8_t)(crc >> 8);
    o[3] = (uint8_t)crc;
  }
  __syncthreads();

  // ---- 6. chunk -> the strip's slot, meta record
  const size_t sidx = (size_t)b * nstrips + strip;
  uint32_t* slot = reinterpret_cast<uint32_t*>(slots + sidx * (size_t)stride);
  const int nbytes = 12 + data_len;                               // <= stride
  for (int w = t; w < (nbytes + 3) / 4; w += kThreads) slot[w] = chunk[w];
  if (t == 0) {
    uint32_t* mrec = meta + sidx * 4;
    mrec[0] = (uint32_t)nbytes;
    mrec[1] = (uint32_t)adler_a % kAdler;
    mrec[2] = (uint32_t)adler_b % kAdler;
    mrec[3] = reg;
  }
}

__global__ __launch_bounds__(kThreads) void png_pack_kernel(const uint32_t* __restrict__ meta, const uint8_t* __restrict__ slots,
                                                            int batch, int H, int rowlen, int R, int nstrips, int stride,
                                                            int capacity, int compact, PngHead head, uint8_t* __restrict__ out,
                                                            int64_t* __restrict__ offsets, int32_t* __restrict__ sizes) {
  __shared__ int tmp[4];
  __shared__ int off_s[kThreads], cnt_s[kThreads];
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  // where the image starts
  const int base = compact ? bytes_before<4>(meta, b * nstrips, tmp) + b * kFixedFile : b * capacity;
  uint8_t* dst = out + base;
  if (t < 33) dst[t] = head.b[t];
  int pos = 33;                                   // bytes of the file so far
  uint32_t A = 1u, Bsum = 0u;                     // Adler-32 of the filtered stream so far
  for (int s0 = 0; s0 < nstrips; s0 += kThreads) {
    const int s = s0 + t;
    const bool live = s < nstrips;
    const uint32_t* mrec = meta + ((size_t)b * nstrips + (live ? s : 0)) * 4;
    const int cnt = live ? (int)mrec[0] : 0;
    const int sa = live ? (int)mrec[1] : 0, sb = live ? (int)mrec[2] : 0;
    const int rows = live ? (H - s * R < R ? H - s * R : R) : 0;
    int tot, atot, btot;
    const int off = block_scan_excl<OP_SUM, false>(cnt, 0, tmp, tot);
    const int a_before = block_scan_excl<OP_SUM, false>(sa, 0, tmp, atot);       // 256 * 65521 < 2^31
    // after len bytes: B += len * A_before + sum((len - i) d_i)
    const uint32_t term = (uint32_t)((uint64_t)(uint32_t)(rows * rowlen) * ((A + (uint32_t)a_before) % kAdler) % kAdler) + (uint32_t)sb;
    block_scan_excl<OP_SUM, false>((int)(term % kAdler), 0, tmp, btot);
    A = (A + (uint32_t)atot) % kAdler;
    Bsum = (Bsum + (uint32_t)btot) % kAdler;
    __syncthreads();
    off_s[t] = pos + off;
    cnt_s[t] = (live && s == nstrips - 1) ? cnt - 8 : cnt;      // the last chunk's Adler and CRC are written below
    __syncthreads();
    const int nhere = nstrips - s0 < kThreads ? nstrips - s0 : kThreads;
    copy_slots(slots + ((size_t)b * nstrips + s0) * (size_t)stride, (size_t)stride, nhere, dst, off_s, cnt_s);
    pos += tot;
  }
  if (t == 0) {
    const uint32_t adler = (Bsum << 16) | A;
    uint32_t reg = meta[((size_t)b * nstrips + nstrips - 1) * 4 + 3];
    reg = crc_step_bits(reg, adler >> 24);
    reg = crc_step_bits(reg, (adler >> 16) & 255u);
    reg = crc_step_bits(reg, (adler >> 8) & 255u);
    reg = crc_step_bits(reg, adler & 255u);
    put_be32(dst + pos - 8, adler);
    put_be32(dst + pos - 4, ~reg);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) dst[pos + i] = iend[i];
    write_index(b, batch, base, pos + 12, capacity, compact, offsets, sizes);
  }
}

int png_check(const char* who, int batch, int H, int W, int C) {
  SFH_REQUIRE(C == 1 || C == 3, "%s: %d channels (1 gray, 3 colour)", who, C);
  SFH_REQUIRE(H > 0 && W > 0, "%s: image %dx%d", who, W, H);
  SFH_REQUIRE((int64_t)1 + (int64_t)W * C <= kMaxRow, "%s: a scanline of 1 + %d * %d bytes (at most %d)", who, W, C, kMaxRow);
  return enc_batch_check(who, batch, H, W, C, sfh_png_capacity(H, W, C), sfh_png_scratch_bytes(batch, H, W, C));
}

}  // namespace

extern "C" int64_t sfh_png_capacity(int H, int W, int C) {
  if ((C != 1 && C != 3) || H <= 0 || W <= 0 || (int64_t)1 + (int64_t)W * C > kMaxRow) {
    sfh_set_error("png_capacity: image %dx%dx%d (1 or 3 channels, a scanline of at most %d bytes)", W, H, C, kMaxRow);
    return -1;
  }
  const int rowlen = 1 + W * C;
  const int64_t strips = sfh_cdiv(H, strip_rows(W, C));
  return kFixedFile + strips * 17 + (int64_t)H * rowlen + 2 + 4;
}

extern "C" int64_t sfh_png_scratch_bytes(int batch, int H, int W, int C) {
  if (sfh_png_capacity(H, W, C) < 0 || batch <= 0) {
    sfh_set_error("png_scratch_bytes: batch %d image %dx%dx%d", batch, W, H, C);
    return -1;
  }
  const int R = strip_rows(W, C);
  const int64_t strips = (int64_t)batch * sfh_cdiv(H, R);
  return strips * 16 + strips * slot_stride(R, 1 + W * C);
}

extern "C" int sfh_png_encode(const uint8_t* images, int batch, int H, int W, int C, int bgr, uint8_t* scratch,
                              int64_t scratch_bytes, void* stream) {
  if (int rc = png_check("png_encode", batch, H, W, C)) return rc;
  SFH_REQUIRE(images && scratch, "png_encode: null pointer (images, scratch)");
  if (int rc = enc_scratch_check("png_encode", scratch, scratch_bytes, sfh_png_scratch_bytes(batch, H, W, C))) return rc;
  const int rowlen = 1 + W * C, R = strip_rows(W, C), nstrips = sfh_cdiv(H, R);
  const int stride = slot_stride(R, rowlen), raw_bytes = raw_lds_bytes(R, rowlen);
  const size_t lds = (size_t)raw_bytes + stride + 16 + kTableBytes;
  sfh_allow_big_lds(reinterpret_cast<const void*>(png_encode_kernel));
  uint32_t* meta = reinterpret_cast<uint32_t*>(scratch);
  uint8_t* slots = scratch + (size_t)batch * nstrips * 16;
  hipLaunchKernelGGL(png_encode_kernel, dim3((unsigned)nstrips, (unsigned)batch), dim3(kThreads), lds, (hipStream_t)stream, images,
                     H, W, C, bgr ? 1 : 0, R, nstrips, raw_bytes, stride, meta, slots);
  return sfh_check_launch("png_encode_kernel");
}

extern "C" int sfh_png_pack(const uint8_t* scratch, int64_t scratch_bytes, int batch, int H, int W, int C, int compact,
                            uint8_t* out, int64_t out_bytes, int64_t* offsets, int32_t* sizes, void* stream) {
  if (int rc = png_check("png_pack", batch, H, W, C)) return rc;
  SFH_REQUIRE(scratch && out && offsets && sizes, "png_pack: null pointer (scratch, out, offsets, sizes)");
  if (int rc = enc_scratch_check("png_pack", scratch, scratch_bytes, sfh_png_scratch_bytes(batch, H, W, C))) return rc;
  const int64_t cap = sfh_png_capacity(H, W, C);
  SFH_REQUIRE(out_bytes >= cap * batch, "png_pack: output of %lld bytes, %lld needed (batch * png_capacity)",
              (long long)out_bytes, (long long)(cap * batch));
  const int rowlen = 1 + W * C, R = strip_rows(W, C), nstrips = sfh_cdiv(H, R);
  PngHead head = {};
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  for (int i = 0; i < 8; ++i) head.b[i] = sig[i];
  uint8_t* p = head.b + 8;
  const uint8_t ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', 0, 0, 0, 0, 0, 0, 0, 0, 8, (uint8_t)(C == 1 ? 0 : 2), 0, 0, 0};
  for (int i = 0; i < 21; ++i) p[i] = ihdr[i];
  put_be32(p + 8, (uint32_t)W);
  put_be32(p + 12, (uint32_t)H);
  put_be32(p + 21, host_crc32(p + 4, 17));
  const uint32_t* meta = reinterpret_cast<const uint32_t*>(scratch);
  const uint8_t* slots = scratch + (size_t)batch * nstrips * 16;
  hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, meta, slots, batch, H, rowlen,
                     R, nstrips, slot_stride(R, rowlen), (int)cap, compact ? 1 : 0, head, out, offsets, sizes);
  return sfh_check_launch("png_pack_kernel");
}
