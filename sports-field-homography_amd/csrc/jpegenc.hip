// jpegenc.hip - baseline JFIF files from uint8 device images in two launches (sfh_amd.jpegenc; the rule is libjpeg's, restated in
// tests/jpegenc_ref.py, which tests/test_jpegenc_host.py holds to PIL's bytes; the three agree byte for byte).
//
// The file is the one libjpeg writes with a restart interval of one MCU row: 4:2:0 (Y 2x2, Cb / Cr 1x1) or gray, the Annex K
// quantisation tables scaled by quality, the Annex K Huffman tables.  A restart interval is byte aligned and predicts its DC
// values from 0, so MCU rows are encoded independently and concatenated.  Integers only, no floating point anywhere.
//
// * jpeg_encode_kernel, one workgroup per (image, MCU row): RGB -> YCbCr in libjpeg's 16-bit fixed point and the h2v2
//   downsample on load, into planar LDS (edges: the right edge replicated per sample before downsampling; the bottom row up to an
//   even height before, every component's last row after it); a thread per block (a contiguous run of blocks per thread, MCU
//   order): jfdctint's "islow" DCT in registers, division by 8 Q as a multiplication by a precomputed reciprocal (exact, see
//   quant_recip), zig-zag -> int16 coefficients in LDS at a stride of 33 dwords (consecutive lanes on different banks); dummy
//   blocks (beyond the component's ceil(size / 8) blocks) take the DC of the block before them; bit lengths per block with the
//   DC difference to the previous block of the component, their prefix sum over the workgroup.  The planar samples are dead by
//   then and their LDS becomes a bit WINDOW of `winw` dwords and a staging area: for every window of the interval's bit stream
//   the blocks that intersect it OR their code bits in (disjoint bits: the order does not matter), clipped to the window; the
//   window's bytes are scanned for 0xFF, stuffed into the staging area, which is aligned with the interval's slot in the scratch
//   buffer, and its whole dwords stored; up to 3 bytes carry over.  The last window pads with 1-bits and appends RSTm (m = MCU
//   row mod 8) or, in the last MCU row, EOI.  An interval of any size is written this way; what is short goes in one pass.
//   The meta record of the interval: {bytes, passes}.
// * jpeg_pack_kernel, one workgroup per image: scan of the interval byte counts, the header (built on the host, a kernel
//   argument), the intervals copied to their offsets, sizes[b], offsets[b].  compact: image b starts at the sum of the sizes of
//   the images before it, which every workgroup computes for itself from the meta records - no third launch.
// No global atomics anywhere; the same bytes every run.
#include "common.h"
#include "codec_common.h"
#include "codec_host.h"
#include "codec_pack.h"
#include "ycc.h"

namespace {

using namespace codecpack;
constexpr int kThreads = kScanThreads;
constexpr int kMaxWidth = SFH_JPEG_MAX_WIDTH;
constexpr int kCoefStride = 66;               // int16 per block: 64 coefficients, the block's bit length, one spare = 33 dwords
// The longest code of a block.  DC: a Huffman code of at most 11 bits (the chroma table's longest) + 11 magnitude bits.  Each of the
// 63 AC coefficients: a code of at most 16 bits + 10 magnitude bits; a block in which every coefficient is coded has neither ZRL
// nor EOB, and every zero coefficient only shortens it (a ZRL is 11 / 10 bits for 16 coefficients, EOB at most 4).
constexpr int kBlockMaxBits = 22 + 63 * 26;
constexpr int kMinRegion = 1536;              // bytes of the samples / window + staging region at least

constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K, tables K.3 - K.6: codes per length 1 .. 16, then the symbols in code order
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// what the kernels take as arguments: the tables of one quality, the encoder's code tables, the file header
struct JpegTables {
  uint32_t recip[2][64];   // natural order: floor(2^32 / (8 Q)) + 1
  uint16_t div[2][64];     // 8 Q
  uint32_t dc[2][12];      // category -> code | length << 16
  uint32_t ac[2][256];     // run << 4 | category -> code | length << 16 (0 where Annex K has no code)
};
constexpr int kTableWords = sizeof(JpegTables) / 4;
struct JpegHead {
  uint8_t b[640];
  int n;
};

// canonical codes of a DHT segment (Annex C)
void derive_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* tab) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) tab[vals[k++]] = code++ | ((uint32_t)len << 16);
    code <<= 1;
  }
}

// libjpeg's jpeg_quality_scaling and jpeg_add_quant_table with force_baseline
int quant_entry(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (base * s + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// (x * m) >> 32 == x / d for m = floor(2^32 / d) + 1 when x * (m d - 2^32) < 2^32; m d - 2^32 is in (0, d], so x < 2^32 / d
// suffices: d = 8 Q <= 2040 and x = |coefficient| + d / 2 < 2^17 (a DCT output is below 2^16)
uint32_t quant_recip(uint32_t d) { return (uint32_t)((1ull << 32) / d) + 1u; }

void make_tables(int quality, JpegTables* t) {
  *t = JpegTables{};
  for (int i = 0; i < 64; ++i) {
    const int q[2] = {quant_entry(kBaseLuma[i], quality), quant_entry(kBaseChroma[i], quality)};
    for (int c = 0; c < 2; ++c) {
      t->div[c][i] = (uint16_t)(8 * q[c]);
      t->recip[c][i] = quant_recip(8u * (uint32_t)q[c]);
    }
  }
  const uint8_t dcvals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  for (int c = 0; c < 2; ++c) {
    derive_codes(kDcBits[c], dcvals, t->dc[c]);
    derive_codes(kAcBits[c], kAcVals[c], t->ac[c]);
  }
}

inline int64_t meta_bytes(int64_t intervals) { return round16(intervals * 8); }   // {bytes, passes} per interval
inline int mcu_size(int C) { return C == 3 ? 16 : 8; }
inline int blocks_per_row(int W, int C) { return sfh_cdiv(W, mcu_size(C)) * (C == 3 ? 6 : 1); }
// bytes of an interval at most: its blocks at kBlockMaxBits, every byte stuffed, the marker
inline int interval_capacity(int W, int C) { return 2 * ((blocks_per_row(W, C) * kBlockMaxBits + 7) / 8) + 2; }
inline int slot_stride(int W, int C) { return round16(interval_capacity(W, C)); }
inline int header_bytes(int C) { return C == 3 ? 629 : 334; }
// the samples of an interval as planar bytes (colour: Y 16 x 16 mcus, Cb and Cr 8 x 8 mcus; gray: 8 x 8 mcus), at least kMinRegion
inline int region_bytes(int W, int C) {
  const int r = sfh_cdiv(W, mcu_size(C)) * (C == 3 ? 384 : 64);
  return r < kMinRegion ? kMinRegion : r;
}
// the window in dwords: the staging area behind it holds the window's bytes all stuffed, 3 carried bytes and the marker
inline int window_words(int region) { return (region - 8) / 12; }

uint8_t* put_segment(uint8_t* p, int marker, const uint8_t* body, int n) {
  *p++ = 0xFF;
  *p++ = (uint8_t)marker;
  *p++ = (uint8_t)((n + 2) >> 8);
  *p++ = (uint8_t)(n + 2);
  for (int i = 0; i < n; ++i) *p++ = body[i];
  return p;
}

void make_header(int H, int W, int C, int quality, JpegHead* h) {
  uint8_t* p = h->b;
  uint8_t body[200];
  *p++ = 0xFF;
  *p++ = 0xD8;
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p = put_segment(p, 0xE0, jfif, 14);
  for (int c = 0; c < (C == 3 ? 2 : 1); ++c) {
    body[0] = (uint8_t)c;
    for (int i = 0; i < 64; ++i) body[1 + i] = (uint8_t)quant_entry((c ? kBaseChroma : kBaseLuma)[kJpegNatural[i]], quality);
    p = put_segment(p, 0xDB, body, 65);
  }
  int n = 0;
  body[n++] = 8;
  body[n++] = (uint8_t)(H >> 8);
  body[n++] = (uint8_t)H;
  body[n++] = (uint8_t)(W >> 8);
  body[n++] = (uint8_t)W;
  body[n++] = (uint8_t)C;
  for (int c = 0; c < C; ++c) {
    body[n++] = (uint8_t)(c + 1);
    body[n++] = (C == 3 && c == 0) ? 0x22 : 0x11;
    body[n++] = c ? 1 : 0;
  }
  p = put_segment(p, 0xC0, body, n);
  for (int c = 0; c < (C == 3 ? 2 : 1); ++c) {
    body[0] = (uint8_t)c;
    for (int i = 0; i < 16; ++i) body[1 + i] = kDcBits[c][i];
    for (int i = 0; i < 12; ++i) body[17 + i] = (uint8_t)i;
    p = put_segment(p, 0xC4, body, 29);
    body[0] = (uint8_t)(0x10 | c);
    for (int i = 0; i < 16; ++i) body[1 + i] = kAcBits[c][i];
    for (int i = 0; i < 162; ++i) body[17 + i] = kAcVals[c][i];
    p = put_segment(p, 0xC4, body, 179);
  }
  const int mcus = sfh_cdiv(W, mcu_size(C));
  body[0] = (uint8_t)(mcus >> 8);
  body[1] = (uint8_t)mcus;
  p = put_segment(p, 0xDD, body, 2);
  n = 0;
  body[n++] = (uint8_t)C;
  for (int c = 0; c < C; ++c) {
    body[n++] = (uint8_t)(c + 1);
    body[n++] = c ? 0x11 : 0x00;
  }
  body[n++] = 0;
  body[n++] = 63;
  body[n++] = 0;
  p = put_segment(p, 0xDA, body, n);
  h->n = (int)(p - h->b);
}

// one pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2) over 8 values; FIRST: the row pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int n = FIRST ? 11 : 15;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d0 = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d4 = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  const int z1 = (t12 + t13) * 4433;
  d2 = descale(z1 + t13 * 6270, n);
  d6 = descale(z1 - t12 * 15137, n);
  const int z5 = (t4 + t6 + t5 + t7) * 9633;
  const int y1 = (t4 + t7) * -7373, y2 = (t5 + t6) * -20995, y3 = (t4 + t6) * -16069 + z5, y4 = (t5 + t7) * -3196 + z5;
  d7 = descale(t4 * 2446 + y1 + y3, n);
  d5 = descale(t5 * 16819 + y2 + y4, n);
  d3 = descale(t6 * 25172 + y2 + y3, n);
  d1 = descale(t7 * 12299 + y1 + y4, n);
}

// `n` bits (1 .. 27), first bit highest, at bit `pos` of the interval's stream, into the window of wn dwords that starts at dword
// w0 of the stream: the dwords outside the window are left alone (w wraps to a large value below the window)
__device__ __forceinline__ void put_bits(uint32_t val, int n, uint32_t pos, uint32_t* win, uint32_t w0, uint32_t wn) {
  const uint32_t w = (pos >> 5) - w0;
  const uint64_t v = (uint64_t)val << (64 - n - (int)(pos & 31u));
  const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
  if (w < wn && hi) atomicOr(&win[w], hi);
  if (w + 1u < wn && lo) atomicOr(&win[w + 1u], lo);
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }

// the codes of one block (zig-zag coefficients cf, DC prediction pred) from bit `pos` on -> the bit position behind them
template <bool EMIT>
__device__ __forceinline__ uint32_t walk_block(const int16_t* cf, int pred, const uint32_t* dc, const uint32_t* ac, uint32_t pos,
                                               uint32_t* win, uint32_t w0, uint32_t wn) {
  {
    const int diff = (int)cf[0] - pred;
    const int cat = category(diff);
    const uint32_t e = dc[cat];
    const int len = (int)(e >> 16) + cat;
    if (EMIT) put_bits(((e & 0xFFFFu) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u)), len, pos, win, w0, wn);
    pos += (uint32_t)len;
  }
  int run = 0;
  const uint32_t zrl = ac[0xF0];
  for (int k = 1; k < 64; ++k) {
    const int v = cf[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      if (EMIT) put_bits(zrl & 0xFFFFu, (int)(zrl >> 16), pos, win, w0, wn);
      pos += zrl >> 16;
      run -= 16;
    }
    const int cat = category(v);
    const uint32_t e = ac[(run << 4) | cat];
    const int len = (int)(e >> 16) + cat;
    if (EMIT) put_bits(((e & 0xFFFFu) << cat) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u)), len, pos, win, w0, wn);
    pos += (uint32_t)len;
    run = 0;
  }
  if (run > 0) {
    const uint32_t e = ac[0];
    if (EMIT) put_bits(e & 0xFFFFu, (int)(e >> 16), pos, win, w0, wn);
    pos += e >> 16;
  }
  return pos;
}

// libjpeg's rgb_ycc_convert: 16-bit fixed point, ONE_HALF on Y (ycc_y, ycc.h), CBCR_OFFSET + ONE_HALF - 1 on chroma
__device__ __forceinline__ int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16; }
__device__ __forceinline__ int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16; }

extern __shared__ __attribute__((aligned(16))) uint8_t jpeg_lds[];

// which component a block of the interval belongs to and where its samples are; block j in MCU order
struct BlockPos {
  int tab;        // 0 luma, 1 chroma tables
  int prev;       // the block whose DC predicts this one's, -1: none
  bool dummy;
  int offset, stride;   // of its 8 x 8 samples in the region
};

__device__ __forceinline__ BlockPos block_pos(int j, int C, int mcus, int row, int ybw, int ybh) {
  BlockPos p;
  if (C == 1) {
    p.tab = 0;
    p.prev = j - 1;
    p.dummy = false;
    p.offset = j * 8;
    p.stride = mcus * 8;
    return p;
  }
  const int m = j / 6, k = j - m * 6;
  const int Wp = mcus * 16, Cw = mcus * 8;
  if (k < 4) {
    const int bx = 2 * m + (k & 1), by = k >> 1;
    p.tab = 0;
    p.prev = k > 0 ? j - 1 : (m > 0 ? j - 3 : -1);
    p.dummy = bx >= ybw || 2 * row + by >= ybh;
    p.offset = by * 8 * Wp + bx * 8;
    p.stride = Wp;
  } else {
    p.tab = 1;
    p.prev = m > 0 ? j - 6 : -1;
    p.dummy = false;
    p.offset = 16 * Wp + (k - 4) * 8 * Cw + m * 8;
    p.stride = Cw;
  }
  return p;
}

__global__ __launch_bounds__(kThreads) void jpeg_encode_kernel(const uint8_t* __restrict__ images, int H, int W, int C, int bgr,
                                                               int mcus, int nrows, int region, int winw, int stride,
                                                               JpegTables tabs, uint32_t* __restrict__ meta,
                                                               uint8_t* __restrict__ slots) {
  const int t = threadIdx.x;
  const int row = blockIdx.x, b = blockIdx.y;
  const int nblocks = mcus * (C == 3 ? 6 : 1);
  uint8_t* smp = jpeg_lds;                                                    // phase 1, 2: the planar samples
  uint32_t* win = reinterpret_cast<uint32_t*>(jpeg_lds);                      // phase 4: the bit window ...
  uint8_t* stage = jpeg_lds + 4 * winw;                                       // ... and the stuffed bytes behind it
  int16_t* coef = reinterpret_cast<int16_t*>(jpeg_lds + region);
  uint32_t* ltab = reinterpret_cast<uint32_t*>(coef + (size_t)nblocks * kCoefStride);
  int* tmp = reinterpret_cast<int*>(ltab + kTableWords);
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&tabs);
    for (int i = t; i < kTableWords; i += kThreads) ltab[i] = src[i];
  }
  const JpegTables* lt = reinterpret_cast<const JpegTables*>(ltab);

  // ---- 1. samples -> planar LDS
  const uint8_t* img = images + (size_t)b * H * W * C;
  if (C == 3) {
    const int Wp = mcus * 16, Cw = mcus * 8;
    const int ro = bgr ? 2 : 0, bo = bgr ? 0 : 2;
    const int y0 = row * 16;
    for (int i = t; i < 8 * Cw; i += kThreads) {
      const int qy = i / Cw, qx = i - qy * Cw;
      const int xa = 2 * qx < W ? 2 * qx : W - 1, xb = 2 * qx + 1 < W ? 2 * qx + 1 : W - 1;
      const int ga = y0 + 2 * qy, ya = ga < H ? ga : H - 1, yb = ga + 1 < H ? ga + 1 : H - 1;
      // chroma: the bottom row replicated up to an even height, then the COMPONENT's last row
      const int qc = (ga >> 1) < ((H - 1) >> 1) ? (ga >> 1) : ((H - 1) >> 1);
      const int ca = 2 * qc, cb = 2 * qc + 1 < H ? 2 * qc + 1 : H - 1;
      const uint8_t* p00 = img + ((size_t)ya * W + xa) * 3;
      const uint8_t* p01 = img + ((size_t)ya * W + xb) * 3;
      const uint8_t* p10 = img + ((size_t)yb * W + xa) * 3;
      const uint8_t* p11 = img + ((size_t)yb * W + xb) * 3;
      const int y00 = ycc_y(p00[ro], p00[1], p00[bo]), y01 = ycc_y(p01[ro], p01[1], p01[bo]);
      const int y10 = ycc_y(p10[ro], p10[1], p10[bo]), y11 = ycc_y(p11[ro], p11[1], p11[bo]);
      *reinterpret_cast<uint16_t*>(smp + (2 * qy) * Wp + 2 * qx) = (uint16_t)(y00 | (y01 << 8));
      *reinterpret_cast<uint16_t*>(smp + (2 * qy + 1) * Wp + 2 * qx) = (uint16_t)(y10 | (y11 << 8));
      if (ca != ya || cb != yb) {
        p00 = img + ((size_t)ca * W + xa) * 3;
        p01 = img + ((size_t)ca * W + xb) * 3;
        p10 = img + ((size_t)cb * W + xa) * 3;
        p11 = img + ((size_t)cb * W + xb) * 3;
      }
      const int bias = 1 + (qx & 1);                                          // h2v2_downsample: 1, 2, 1, 2 along the row
      const int scb = ycc_cb(p00[ro], p00[1], p00[bo]) + ycc_cb(p01[ro], p01[1], p01[bo]) + ycc_cb(p10[ro], p10[1], p10[bo]) +
                      ycc_cb(p11[ro], p11[1], p11[bo]);
      const int scr = ycc_cr(p00[ro], p00[1], p00[bo]) + ycc_cr(p01[ro], p01[1], p01[bo]) + ycc_cr(p10[ro], p10[1], p10[bo]) +
                      ycc_cr(p11[ro], p11[1], p11[bo]);
      smp[16 * Wp + qy * Cw + qx] = (uint8_t)((scb + bias) >> 2);
      smp[16 * Wp + 8 * Cw + qy * Cw + qx] = (uint8_t)((scr + bias) >> 2);
    }
  } else {
    const int Wp = mcus * 8, W4 = mcus * 2;
    const int y0 = row * 8;
    for (int i = t; i < 8 * W4; i += kThreads) {
      const int y = i / W4, x4 = (i - y * W4) * 4;
      const int gy = y0 + y < H ? y0 + y : H - 1;
      const uint8_t* src = img + (size_t)gy * W;
      uint32_t word = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) word |= (uint32_t)src[x4 + k < W ? x4 + k : W - 1] << (8 * k);
      *reinterpret_cast<uint32_t*>(smp + y * Wp + x4) = word;
    }
  }
  __syncthreads();

  // ---- 2. DCT, quantisation, zig-zag: a contiguous run of blocks per thread
  const int per = (nblocks + kThreads - 1) / kThreads;
  const int j0 = t * per < nblocks ? t * per : nblocks;
  const int j1 = j0 + per < nblocks ? j0 + per : nblocks;
  const int ybw = (W + 7) >> 3, ybh = (H + 7) >> 3;
  for (int j = j0; j < j1; ++j) {
    const BlockPos bp = block_pos(j, C, mcus, row, ybw, ybh);
    int16_t* cf = coef + (size_t)j * kCoefStride;
    if (bp.dummy) {
#pragma unroll
      for (int i = 0; i < 32; ++i) reinterpret_cast<uint32_t*>(cf)[i] = 0u;
      continue;
    }
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t* s = reinterpret_cast<const uint32_t*>(smp + bp.offset + r * bp.stride);
      const uint32_t lo = s[0], hi = s[1];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        d[r * 8 + c] = (int)((lo >> (8 * c)) & 255u) - 128;
        d[r * 8 + 4 + c] = (int)((hi >> (8 * c)) & 255u) - 128;
      }
      fdct8<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
    const uint32_t* recip = lt->recip[bp.tab];
    const uint16_t* dv = lt->div[bp.tab];
#pragma unroll
    for (int z = 0; z < 64; ++z) {
      const int i = kJpegNatural[z];
      const int c = d[i];
      const uint32_t q = __umulhi((uint32_t)(c < 0 ? -c : c) + ((uint32_t)dv[i] >> 1), recip[i]);
      cf[z] = (int16_t)(c < 0 ? -(int)q : (int)q);
    }
  }
  __syncthreads();
  // a dummy block has the DC of the block before it in the MCU; block 0 of an MCU is never a dummy
  for (int j = j0; j < j1; ++j) {
    if (C != 3) break;
    const BlockPos bp = block_pos(j, C, mcus, row, ybw, ybh);
    if (!bp.dummy) continue;
    int src = j - 1;
    while (block_pos(src, C, mcus, row, ybw, ybh).dummy) --src;
    coef[(size_t)j * kCoefStride] = coef[(size_t)src * kCoefStride];
  }
  __syncthreads();

  // ---- 3. bit lengths, their prefix sum
  uint32_t mybits = 0;
  for (int j = j0; j < j1; ++j) {
    const BlockPos bp = block_pos(j, C, mcus, row, ybw, ybh);
    int16_t* cf = coef + (size_t)j * kCoefStride;
    const int pred = bp.prev >= 0 ? coef[(size_t)bp.prev * kCoefStride] : 0;
    const uint32_t n = walk_block<false>(cf, pred, lt->dc[bp.tab], lt->ac[bp.tab], 0u, nullptr, 0u, 0u);
    cf[64] = (int16_t)n;                                                      // <= kBlockMaxBits
    mybits += n;
  }
  int total_bits;
  const int bit_excl = block_scan_excl<OP_SUM, false>((int)mybits, 0, tmp, total_bits);   // 768 * 1660 < 2^31
  const int nbytes = (total_bits + 7) >> 3;                                   // of the interval before stuffing
  const int nwords = (nbytes + 3) >> 2;
  const bool last_row = row == nrows - 1;

  // ---- 4. windows of the bit stream -> stuffed bytes -> the slot
  const size_t sidx = (size_t)b * nrows + row;
  uint32_t* slot = reinterpret_cast<uint32_t*>(slots + sidx * (size_t)stride);
  int outw = 0;                      // dwords of the slot written
  int carry = 0;                     // bytes at the start of the staging area that belong to dword outw
  int passes = 0;
  for (int w0 = 0; w0 < nwords; w0 += winw) {
    ++passes;
    __syncthreads();                 // the previous flush has read the staging area; phase 2 has read the samples
    for (int w = t; w < winw; w += kThreads) win[w] = 0u;
    __syncthreads();
    {
      const uint32_t lo = (uint32_t)w0 * 32u, hi = lo + (uint32_t)winw * 32u;
      uint32_t pos = (uint32_t)bit_excl;
      for (int j = j0; j < j1; ++j) {
        const int16_t* cf = coef + (size_t)j * kCoefStride;
        const uint32_t n = (uint32_t)cf[64];
        if (pos < hi && pos + n > lo) {
          const BlockPos bp = block_pos(j, C, mcus, row, ybw, ybh);
          const int pred = bp.prev >= 0 ? coef[(size_t)bp.prev * kCoefStride] : 0;
          walk_block<true>(cf, pred, lt->dc[bp.tab], lt->ac[bp.tab], pos, win, (uint32_t)w0, (uint32_t)winw);
        }
        pos += n;
      }
      if (t == 0 && (total_bits & 7)) put_bits((1u << (8 - (total_bits & 7))) - 1u, 8 - (total_bits & 7), (uint32_t)total_bits, win,
                                               (uint32_t)w0, (uint32_t)winw);   // 1-padding of the last byte
    }
    __syncthreads();
    const int cnt = nbytes - 4 * w0 < 4 * winw ? nbytes - 4 * w0 : 4 * winw;  // bytes of this window
    const int seg = 4 * ((cnt + 4 * kThreads - 1) / (4 * kThreads));
    const int s0 = t * seg < cnt ? t * seg : cnt;
    const int s1 = s0 + seg < cnt ? s0 + seg : cnt;
    int nff = 0;
    for (int i = s0; i < s1; ++i) nff += ((win[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
    int total_ff;
    const int ff_before = block_scan_excl<OP_SUM, false>(nff, 0, tmp, total_ff);
    {
      uint8_t* o = stage + carry + s0 + ff_before;
      for (int i = s0; i < s1; ++i) {
        const uint32_t v = (win[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
        *o++ = (uint8_t)v;
        if (v == 255u) *o++ = 0;
      }
    }
    int len = carry + cnt + total_ff;                                         // bytes in the staging area
    const bool last = w0 + winw >= nwords;
    if (last) {
      if (t == 0) {
        stage[len] = 0xFF;
        stage[len + 1] = last_row ? 0xD9 : (uint8_t)(0xD0 + (row & 7));
      }
      len += 2;
    }
    __syncthreads();
    // the last flush rounds up to a whole dword: up to 3 stale bytes of the staging area follow the marker.  They stay inside
    // the slot (its stride is a multiple of 16) and behind the interval's byte count, so the pack kernel never copies them.
    const int nfull = last ? (len + 3) >> 2 : len >> 2;
    const uint32_t* st32 = reinterpret_cast<const uint32_t*>(stage);
    for (int w = t; w < nfull; w += kThreads) slot[outw + w] = st32[w];
    outw += nfull;
    carry = len - 4 * nfull;
    if (!last && nfull > 0) {
      __syncthreads();
      if (t == 0) reinterpret_cast<uint32_t*>(stage)[0] = st32[nfull];
    }
    if (last && t == 0) {
      meta[sidx * 2] = (uint32_t)(4 * (outw - nfull) + len);
      meta[sidx * 2 + 1] = (uint32_t)passes;
    }
  }
}

constexpr int kPackLdsBytes = (4 + 2 * kThreads) * (int)sizeof(int);

__global__ __launch_bounds__(kThreads) void jpeg_pack_kernel(const uint32_t* __restrict__ meta, const uint8_t* __restrict__ slots,
                                                             int batch, int nrows, int stride, int capacity, int compact,
                                                             JpegHead head, uint8_t* __restrict__ out,
                                                             int64_t* __restrict__ offsets, int32_t* __restrict__ sizes) {
  int* tmp = reinterpret_cast<int*>(jpeg_lds);                                // kPackLdsBytes of dynamic LDS: the scan's 4 ints,
  int* off_s = tmp + 4;                                                       // offset and byte count of kThreads intervals
  int* cnt_s = off_s + kThreads;
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int base = compact ? bytes_before<2>(meta, b * nrows, tmp) + b * head.n : b * capacity;
  uint8_t* dst = out + base;
  for (int i = t; i < head.n; i += kThreads) dst[i] = head.b[i];
  int pos = head.n;
  for (int s0 = 0; s0 < nrows; s0 += kThreads) {
    const int s = s0 + t;
    const int cnt = s < nrows ? (int)meta[((size_t)b * nrows + s) * 2] : 0;
    int tot;
    const int off = block_scan_excl<OP_SUM, false>(cnt, 0, tmp, tot);
    __syncthreads();
    off_s[t] = pos + off;
    cnt_s[t] = cnt;
    __syncthreads();
    const int nhere = nrows - s0 < kThreads ? nrows - s0 : kThreads;
    copy_slots(slots + ((size_t)b * nrows + s0) * (size_t)stride, (size_t)stride, nhere, dst, off_s, cnt_s);
    pos += tot;
  }
  if (t == 0) write_index(b, batch, base, pos, capacity, compact, offsets, sizes);
}

int jpeg_check(const char* who, int batch, int H, int W, int C, int quality) {
  SFH_REQUIRE(C == 1 || C == 3, "%s: %d channels (1 gray, 3 colour)", who, C);
  SFH_REQUIRE(H > 0 && W > 0 && H <= 65535, "%s: image %dx%d", who, W, H);
  SFH_REQUIRE(W <= kMaxWidth, "%s: width %d (at most %d)", who, W, kMaxWidth);
  SFH_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d (1 .. 100)", who, quality);
  return enc_batch_check(who, batch, H, W, C, sfh_jpeg_capacity(H, W, C), sfh_jpeg_scratch_bytes(batch, H, W, C));
}

}  // namespace

extern "C" int64_t sfh_jpeg_capacity(int H, int W, int C) {
  if ((C != 1 && C != 3) || H <= 0 || W <= 0 || H > 65535 || W > kMaxWidth) {
    sfh_set_error("jpeg_capacity: image %dx%dx%d (1 or 3 channels, at most %d wide and 65535 high)", W, H, C, kMaxWidth);
    return -1;
  }
  return header_bytes(C) + (int64_t)sfh_cdiv(H, mcu_size(C)) * interval_capacity(W, C);
}

extern "C" int64_t sfh_jpeg_scratch_bytes(int batch, int H, int W, int C) {
  if (sfh_jpeg_capacity(H, W, C) < 0 || batch <= 0) {
    sfh_set_error("jpeg_scratch_bytes: batch %d image %dx%dx%d", batch, W, H, C);
    return -1;
  }
  const int64_t rows = (int64_t)batch * sfh_cdiv(H, mcu_size(C));
  return meta_bytes(rows) + rows * slot_stride(W, C);
}

extern "C" int sfh_jpeg_encode(const uint8_t* images, int batch, int H, int W, int C, int bgr, int quality, uint8_t* scratch,
                               int64_t scratch_bytes, int window_dwords, void* stream) {
  if (int rc = jpeg_check("jpeg_encode", batch, H, W, C, quality)) return rc;
  SFH_REQUIRE(images && scratch, "jpeg_encode: null pointer (images, scratch)");
  if (int rc = enc_scratch_check("jpeg_encode", scratch, scratch_bytes, sfh_jpeg_scratch_bytes(batch, H, W, C))) return rc;
  const int region = region_bytes(W, C);
  const int winmax = window_words(region);
  SFH_REQUIRE(window_dwords >= 0 && window_dwords <= winmax, "jpeg_encode: window of %d dwords (0: the default, at most %d)",
              window_dwords, winmax);
  const int winw = window_dwords ? window_dwords : winmax;
  const int mcus = sfh_cdiv(W, mcu_size(C)), nrows = sfh_cdiv(H, mcu_size(C));
  const int nblocks = mcus * (C == 3 ? 6 : 1);
  JpegTables tabs;
  make_tables(quality, &tabs);
  const size_t lds = (size_t)region + (size_t)nblocks * kCoefStride * 2 + sizeof(JpegTables) + 16;
  sfh_allow_big_lds(reinterpret_cast<const void*>(jpeg_encode_kernel));
  uint32_t* meta = reinterpret_cast<uint32_t*>(scratch);
  uint8_t* slots = scratch + meta_bytes((int64_t)batch * nrows);
  hipLaunchKernelGGL(jpeg_encode_kernel, dim3((unsigned)nrows, (unsigned)batch), dim3(kThreads), lds, (hipStream_t)stream, images,
                     H, W, C, bgr ? 1 : 0, mcus, nrows, region, winw, slot_stride(W, C), tabs, meta, slots);
  return sfh_check_launch("jpeg_encode_kernel");
}

extern "C" int sfh_jpeg_pack(const uint8_t* scratch, int64_t scratch_bytes, int batch, int H, int W, int C, int quality,
                             int compact, uint8_t* out, int64_t out_bytes, int64_t* offsets, int32_t* sizes, void* stream) {
  if (int rc = jpeg_check("jpeg_pack", batch, H, W, C, quality)) return rc;
  SFH_REQUIRE(scratch && out && offsets && sizes, "jpeg_pack: null pointer (scratch, out, offsets, sizes)");
  if (int rc = enc_scratch_check("jpeg_pack", scratch, scratch_bytes, sfh_jpeg_scratch_bytes(batch, H, W, C))) return rc;
  const int64_t cap = sfh_jpeg_capacity(H, W, C);
  SFH_REQUIRE(out_bytes >= cap * batch, "jpeg_pack: output of %lld bytes, %lld needed (batch * jpeg_capacity)",
              (long long)out_bytes, (long long)(cap * batch));
  const int nrows = sfh_cdiv(H, mcu_size(C));
  JpegHead head = {};
  make_header(H, W, C, quality, &head);
  const uint32_t* meta = reinterpret_cast<const uint32_t*>(scratch);
  const uint8_t* slots = scratch + meta_bytes((int64_t)batch * nrows);
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)batch), dim3(kThreads), kPackLdsBytes, (hipStream_t)stream, meta, slots,
                     batch, nrows, slot_stride(W, C), (int)cap, compact ? 1 : 0, head, out, offsets, sizes);
  return sfh_check_launch("jpeg_pack_kernel");
}
