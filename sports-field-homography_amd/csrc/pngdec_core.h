// pngdec_core.h - the decode core of sfh_amd.pngdec as plain functions that compile for the host and for the device: the chunk
// parse with its CRC-32, the bit reader over the joined IDAT bodies, the canonical-code tables, the inflate of one deflate
// sequence by one wave, and the arithmetic of one unfiltered pixel.  csrc/pngdec.hip runs pd_inflate in a 64-thread workgroup;
// tests/pngdec_host_main.cpp runs it lane by lane under the sanitizers.  Nothing here includes a HIP header.
//
// Lanes.  pd_inflate is written once.  Code outside a lane section is UNIFORM: every lane of the wave runs it on the same values
// (every lane has its own copy of the reader and of the decode state, so nothing has to be broadcast); it never writes shared
// memory except one lane through PD_IS_LANE.  A lane section, PD_LANES_BEGIN(lane) ... PD_LANES_END, is the data-parallel part:
// on the device `lane` is the thread index and the section stands between two workgroup barriers; on the host it is a loop over
// the 64 lanes, one after the other - correct because no lane of a section reads what another lane of the same section writes.
//
// Streams.  The deflate bytes of a file are the joined IDAT bodies without the two bytes of the zlib header and the four of the
// Adler-32.  A PdStream is a run of `len` of those bytes that starts `skip` bytes into the body `r0` of the file's range table
// {first byte, end byte} (offsets in the file); the reader walks the table, so a stream crosses chunk boundaries at any bit.
//
// Bounds.  The bytes are not trusted.  A read outside the stream's bytes, or outside [0, file_bytes) of the file, gives zero and is
// counted; a decode that used such bits ends with PD_E_EOF.  Every store is guarded by the `cap` bytes of the stream's slot.  The
// ring is indexed modulo its size.  Every token uses at least one bit and every batch checks the bit count, so a decode ends.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/sfh_amd.h"
#include "codec_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PD_LANES_BEGIN(lane) \
  __syncthreads();           \
  {                          \
    const int lane = (int)threadIdx.x;
#define PD_LANES_END \
  }                  \
  __syncthreads();
#define PD_IS_LANE(i) ((int)threadIdx.x == (i))
#else
#define PD_LANES_BEGIN(lane) for (int lane = 0; lane < kPdLanes; ++lane) {
#define PD_LANES_END }
#define PD_IS_LANE(i) true
#endif

constexpr int kPdLanes = 64;
constexpr int kPdWindow = 32768;          // deflate's largest distance
// The ring holds more than the window: the literals of a batch are stored before its matches are copied, so a byte of the batch
// must not land on a slot that an earlier match of the same batch still reads.  A batch ends once it has kPdBatchBytes.
constexpr int kPdRing = 49152;
constexpr int kPdBatchBytes = kPdRing - kPdWindow - 258;

// status bits of an image (PngDecoder.status)
enum {
  PD_E_TABLE = 1,     // an over-subscribed or incomplete code-length set, no end-of-block code, a repeat with nothing to repeat
  PD_E_SYMBOL = 2,    // symbols 286 / 287, distance codes 30 / 31, bits that are no code, block type 3
  PD_E_DIST = 4,      // a distance beyond the bytes produced
  PD_E_STORED = 8,    // a stored block with LEN != ~NLEN
  PD_E_SIZE = 16,     // output short of or beyond H (1 + W C)
  PD_E_EOF = 32,      // the bits end early
  PD_E_FILTER = 64,   // a filter byte above 4
  PD_E_ADLER = 128    // the Adler-32 of the filtered stream is not the file's
};

// ------------------------------------------------------------------------------------------------------------ the host parse

// Host code: the parse of sfh_png_parse.  ranges: int32 pairs, as many as `cap` admits (may be null with cap 0).
inline int pd_parse(const uint8_t* d, int64_t n, sfh_png_info* info, int32_t* ranges, int64_t cap) {
  memset(info, 0, sizeof(*info));
  auto refuse = [&](int reason) {
    info->reason = reason;
    return -1;
  };
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (n >= ((int64_t)1 << 31)) return refuse(SFH_PNG_R_TOO_LONG);
  if (n < 8) return refuse(memcmp(d, sig, (size_t)(n > 0 ? n : 0)) ? SFH_PNG_R_NOT_PNG : SFH_PNG_R_TRUNCATED);
  if (memcmp(d, sig, 8)) return refuse(SFH_PNG_R_NOT_PNG);
  int64_t pos = 8;
  bool have_ihdr = false, have_iend = false, idat_closed = false;
  int later = 0;                                         // a reason found behind IHDR that a malformed chunk list outranks
  int32_t nidat = 0;
  int64_t idat_bytes = 0;
  uint8_t head[2] = {0, 0}, tail[4] = {0, 0, 0, 0};      // the first two and the last four bytes of the joined bodies
  while (!have_iend) {
    if (n - pos < 12) return refuse(have_ihdr ? SFH_PNG_R_NO_IEND : SFH_PNG_R_TRUNCATED);
    const uint32_t len = get_be32(d + pos);
    const uint8_t* tag = d + pos + 4;
    if (len > 0x7FFFFFFFu || (int64_t)len > n - pos - 12) return refuse(have_ihdr ? SFH_PNG_R_NO_IEND : SFH_PNG_R_TRUNCATED);
    const uint8_t* body = d + pos + 8;
    if (host_crc32(tag, 4 + (int64_t)len) != get_be32(body + len)) return refuse(SFH_PNG_R_CRC);
    const bool is_idat = !memcmp(tag, "IDAT", 4);
    if (!have_ihdr) {
      if (memcmp(tag, "IHDR", 4) || len != 13) return refuse(SFH_PNG_R_BAD_IHDR);
      have_ihdr = true;
      const uint32_t w = get_be32(body), h = get_be32(body + 4);
      const int depth = body[8], ctype = body[9], comp = body[10], filt = body[11], lace = body[12];
      if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || comp != 0 || filt != 0 || lace > 1 ||
          !(ctype == 0 || ctype == 2 || ctype == 3 || ctype == 4 || ctype == 6) ||
          !(depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16))
        return refuse(SFH_PNG_R_BAD_IHDR);
      info->width = (int32_t)w;
      info->height = (int32_t)h;
      info->bit_depth = depth;
      info->color_type = ctype;
      info->interlace = lace;
      info->channels = ctype == 0 ? 1 : (ctype == 2 ? 3 : (ctype == 6 ? 4 : 0));
      if (ctype == 3) later = SFH_PNG_R_PALETTE;
      else if (ctype == 4) later = SFH_PNG_R_GRAY_ALPHA;
      else if (depth != 8) later = SFH_PNG_R_BIT_DEPTH;
      else if (lace) later = SFH_PNG_R_INTERLACE;
    } else if (!memcmp(tag, "IHDR", 4)) {
      return refuse(SFH_PNG_R_BAD_IHDR);
    } else if (is_idat) {
      if (idat_closed) return refuse(SFH_PNG_R_IDAT_ORDER);
      if (nidat < cap) {
        ranges[2 * nidat] = (int32_t)(pos + 8);
        ranges[2 * nidat + 1] = (int32_t)(pos + 8 + len);
      }
      for (uint32_t i = 0; i < len && idat_bytes + i < 2; ++i) head[idat_bytes + i] = body[i];
      for (uint32_t i = len > 4 ? len - 4 : 0; i < len; ++i) {
        tail[0] = tail[1];
        tail[1] = tail[2];
        tail[2] = tail[3];
        tail[3] = body[i];
      }
      ++nidat;
      idat_bytes += len;
      if (idat_bytes >= ((int64_t)1 << 31)) return refuse(SFH_PNG_R_TOO_LONG);
    } else if (!memcmp(tag, "IEND", 4)) {
      have_iend = true;
    } else {
      if (!memcmp(tag, "acTL", 4) || !memcmp(tag, "fcTL", 4) || !memcmp(tag, "fdAT", 4)) later = later ? later : SFH_PNG_R_APNG;
      else if (!(tag[0] & 0x20) && memcmp(tag, "PLTE", 4)) return refuse(SFH_PNG_R_CRITICAL);   // a critical chunk nobody knows
    }
    if (nidat > 0 && !is_idat) idat_closed = true;
    pos += 12 + (int64_t)len;
  }
  if (later) return refuse(later);
  if (nidat == 0) return refuse(SFH_PNG_R_NO_IDAT);
  if (idat_bytes < 6) return refuse(SFH_PNG_R_ZLIB);
  info->nidat = nidat;
  info->idat_bytes = (int32_t)idat_bytes;
  info->cmf = head[0];
  info->flg = head[1];
  info->adler = ((uint32_t)tail[0] << 24) | ((uint32_t)tail[1] << 16) | ((uint32_t)tail[2] << 8) | tail[3];
  if ((head[0] & 15) != 8 || (head[0] >> 4) > 7 || ((head[0] << 8) | head[1]) % 31 != 0) return refuse(SFH_PNG_R_ZLIB);
  if (head[1] & 0x20) return refuse(SFH_PNG_R_ZLIB_DICT);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ the bit reader

struct PdStream {
  const uint8_t* file;      // the file's first byte
  int32_t file_bytes;
  const int32_t* ranges;    // {first byte, end byte} of every IDAT body
  int32_t nranges;
  int32_t r0;               // the body the stream starts in
  int32_t skip;             // bytes of that body before the stream
  int32_t len;              // bytes of the stream
};

struct PdReader {
  const PdStream* s;
  int32_t ri, p, e;         // the current body and the next byte in it, [p, e) clamped to the file
  int32_t left;             // bytes of the stream not fetched yet
  int32_t over;             // zero bytes fetched beyond the stream
  uint64_t buf;
  int32_t nbits;
};

SFH_HD void pd_enter_range(PdReader& r, int ri) {
  r.ri = ri;
  int32_t p = 0, e = 0;
  if (ri < r.s->nranges) {
    p = r.s->ranges[2 * ri];
    e = r.s->ranges[2 * ri + 1];
  }
  if (p < 0) p = 0;
  if (e > r.s->file_bytes) e = r.s->file_bytes;
  if (e < p) e = p;
  r.p = p;
  r.e = e;
}

// the reader `n` more bytes into the stream (n >= 0), nothing fetched
SFH_HD void pd_skip_bytes(PdReader& r, int64_t n) {
  if (n > r.left) n = r.left;
  r.left -= (int32_t)n;
  while (n > 0 && r.ri < r.s->nranges) {
    const int32_t have = r.e - r.p;
    if (n <= have) {
      r.p += (int32_t)n;
      return;
    }
    n -= have;
    pd_enter_range(r, r.ri + 1);
  }
}

SFH_HD void pd_reader_init(PdReader& r, const PdStream& s) {
  r.s = &s;
  r.left = s.len > 0 ? s.len : 0;
  r.over = 0;
  r.buf = 0;
  r.nbits = 0;
  pd_enter_range(r, s.r0 < 0 ? 0 : s.r0);
  const int32_t keep = r.left;
  r.left = 0x7FFFFFFF;
  pd_skip_bytes(r, s.skip > 0 ? s.skip : 0);
  r.left = keep;
}

SFH_HD uint32_t pd_next_byte(PdReader& r) {
  if (r.left > 0) {
    while (r.p >= r.e && r.ri < r.s->nranges) pd_enter_range(r, r.ri + 1);
    if (r.p < r.e) {
      --r.left;
      return r.s->file[r.p++];
    }
    r.left = 0;
  }
  ++r.over;
  return 0;
}

SFH_HD void pd_refill(PdReader& r) {
  while (r.nbits <= 56) {
    r.buf |= (uint64_t)pd_next_byte(r) << r.nbits;
    r.nbits += 8;
  }
}
SFH_HD uint32_t pd_bits(PdReader& r, int n) {              // n <= 16, the buffer filled
  const uint32_t v = (uint32_t)r.buf & ((1u << n) - 1u);
  r.buf >>= n;
  r.nbits -= n;
  return v;
}
SFH_HD bool pd_past_end(const PdReader& r) { return r.nbits < 8 * r.over; }
// bits of the stream used so far (valid while !pd_past_end)
SFH_HD int64_t pd_used_bits(const PdReader& r) {
  return 8 * ((int64_t)(r.s->len > 0 ? r.s->len : 0) - r.left + r.over) - r.nbits;
}

// ------------------------------------------------------------------------------------------------------------ the code tables

// A canonical code in the lookup form sfh_amd.jpegdec uses: look[low 9 bits of the stream] = length << 9 | symbol for a code of at
// most 9 bits (0: none); a longer code c of length l, read first bit highest, is valid iff c <= maxcode[l] (-1: none of that
// length) and its symbol is vals[c + valoff[l]]; vals in code order.
struct PdTable {
  uint16_t look[512];
  int32_t maxcode[16];
  int32_t valoff[16];
  int32_t first[16];      // first code of every length
  int32_t start[16];      // index in vals of the first symbol of every length
  uint16_t vals[288];
  int32_t nvals;
  int32_t err;
};

struct PdRec {
  int32_t pos;            // output offset in the stream's slot
  int32_t tok;            // a literal: the byte; a match: 256 | length << 9 ... see pd_inflate
  int32_t dist;           // 0: a literal
};

struct PdShared {
  uint8_t ring[kPdRing];
  PdTable lit, dst, cl;
  uint8_t lens[320];      // the code lengths of a block: literal / length, then distance
  uint8_t cl_lens[19];
  PdRec rec[kPdLanes];
};

SFH_HD uint32_t pd_rev(uint32_t v, int n) {               // the low n bits of v in reverse order, n <= 16
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
  v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
  return v >> (16 - n);
}

// one lane: counts, the completeness rule (zlib's: a set may be incomplete only if it is one code of one bit, or - literal /
// length and distance sets - empty), first codes, symbols in code order
SFH_HD void pd_table_prepare(PdTable& t, const uint8_t* lens, int n, bool is_cl) {
  int32_t count[16];
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int i = 0; i < n; ++i) ++count[lens[i] & 15];
  int32_t left = 1, maxlen = 0;
  t.err = 0;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - count[l];
    if (left < 0) {
      t.err = PD_E_TABLE;
      left = 0;
    }
    if (count[l]) maxlen = l;
  }
  if (left > 0 && (is_cl || maxlen > 1)) t.err = PD_E_TABLE;
  int32_t code = 0, idx = 0;
  t.maxcode[0] = -1;
  t.valoff[0] = t.first[0] = t.start[0] = 0;
  for (int l = 1; l < 16; ++l) {
    code <<= 1;
    t.first[l] = code;
    t.start[l] = idx;
    t.valoff[l] = idx - code;
    t.maxcode[l] = count[l] ? code + count[l] - 1 : -1;
    code += count[l];
    idx += count[l];
  }
  t.nvals = idx;
  int32_t next[16];
  for (int l = 0; l < 16; ++l) next[l] = t.start[l];
  for (int i = 0; i < n; ++i) {
    const int l = lens[i] & 15;
    if (l && next[l] < 288) t.vals[next[l]++] = (uint16_t)i;
  }
  if (t.err) {                                             // an over-subscribed set: nothing of it is used
    t.nvals = 0;
    for (int l = 0; l < 16; ++l) t.maxcode[l] = -1;
  }
}

// lens[0, n) -> t, by the wave
#define PD_BUILD_TABLE(t, lens_, n_, is_cl_)                                              \
  PD_LANES_BEGIN(lane)                                                                    \
  if (lane == 0) pd_table_prepare(t, lens_, n_, is_cl_);                                  \
  for (int i = lane; i < 512; i += kPdLanes) (t).look[i] = 0;                             \
  PD_LANES_END                                                                            \
  PD_LANES_BEGIN(lane)                                                                    \
  for (int i = lane; i < (t).nvals; i += kPdLanes) {                                      \
    const int sym = (t).vals[i];                                                          \
    const int l = (lens_)[sym] & 15;                                                      \
    if (l >= 1 && l <= 9) {                                                               \
      const uint32_t code = (uint32_t)((t).first[l] + (i - (t).start[l]));                \
      for (uint32_t j = pd_rev(code, l); j < 512; j += 1u << l) (t).look[j] = (uint16_t)((l << 9) | sym); \
    }                                                                                     \
  }                                                                                       \
  PD_LANES_END

// the code at the low end of `bits` -> its length (0: no such code) and symbol
SFH_HD int pd_code(const PdTable& t, uint32_t bits, int& sym) {
  const uint32_t e = t.look[bits & 511u];
  if (e) {
    sym = (int)(e & 511u);
    return (int)(e >> 9);
  }
  const uint32_t rev = pd_rev(bits & 0x7FFFu, 15);
  for (int l = 10; l <= 15; ++l) {
    const int32_t code = (int32_t)(rev >> (15 - l));
    if (code <= t.maxcode[l]) {
      const int32_t idx = code + t.valoff[l];
      sym = t.vals[(idx >= 0 && idx < 288) ? idx : 0];
      return l;
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ inflate

struct PdResult {
  int32_t produced;   // bytes of output
  int32_t status;     // PD_E_*
  int32_t final_seen; // a block with BFINAL ended the decode
  int32_t exact;      // the decode ended on a block boundary with exactly the stream's bits used (the last block: to the byte)
};

constexpr uint16_t kPdLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kPdLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kPdDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kPdDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr uint8_t kPdClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

SFH_HD void pd_put(PdShared& sh, uint8_t* out, int32_t cap, int32_t pos, uint8_t v) {
  sh.ring[(uint32_t)pos % (uint32_t)kPdRing] = v;
  if (pos < cap) out[pos] = v;
}

// One deflate sequence by one wave.  out: the stream's slot of `cap` bytes, or null to count only (nothing is stored, the ring is
// not used).  limit: the decode fails with PD_E_SIZE once it has produced more than `limit` bytes.  The decode ends at the end of
// a BFINAL block, or - whole_stream false - at the first block boundary at or beyond the stream's last bit.
SFH_HD void pd_inflate(const PdStream& s, PdShared& sh, uint8_t* out, int32_t cap, int32_t limit, PdResult& res) {
  PdReader r;
  pd_reader_init(r, s);
  const int64_t nbits_stream = 8 * (int64_t)(s.len > 0 ? s.len : 0);
  int32_t pos = 0, status = 0;
  bool final_seen = false, exact = false;
  for (;;) {
    pd_refill(r);
    const bool bfinal = pd_bits(r, 1) != 0;
    const uint32_t btype = pd_bits(r, 2);
    if (pd_past_end(r)) {
      status |= PD_E_EOF;
      break;
    }
    if (btype == 3) {
      status |= PD_E_SYMBOL;
      break;
    }
    if (btype == 0) {
      pd_bits(r, r.nbits & 7);                             // to the byte boundary
      pd_refill(r);
      const uint32_t len = pd_bits(r, 16);
      const uint32_t nlen = pd_bits(r, 16);
      if (pd_past_end(r)) {
        status |= PD_E_EOF;
        break;
      }
      if ((len ^ 0xFFFFu) != nlen) {
        status |= PD_E_STORED;
        break;
      }
      if ((int64_t)pos + len > limit) {
        status |= PD_E_SIZE;
        break;
      }
      // the buffer holds whole bytes: the block's first ones, then (beyond the stream's end) `over` zero bytes that are no data
      int32_t held = (r.nbits >> 3) - r.over;
      if ((uint32_t)held > len) held = (int32_t)len;
      const int32_t rest = (int32_t)len - held;
      if (rest > r.left) {
        status |= PD_E_EOF;
        break;
      }
      const uint64_t heldbits = r.buf;
      if (out && held > 0) {
        PD_LANES_BEGIN(lane)
        if (lane < held) pd_put(sh, out, cap, pos + lane, (uint8_t)(heldbits >> (8 * lane)));
        PD_LANES_END
      }
      if (rest > 0) {                                      // then straight from the bodies, 64 bytes a step; over == 0 here
        r.buf = 0;
        r.nbits = 0;
        if (out) {
          PD_LANES_BEGIN(lane)
          PdReader q = r;
          pd_skip_bytes(q, lane);
          for (int32_t j = lane; j < rest; j += kPdLanes) {
            pd_put(sh, out, cap, pos + held + j, (uint8_t)pd_next_byte(q));
            pd_skip_bytes(q, kPdLanes - 1);
          }
          PD_LANES_END
        }
        pd_skip_bytes(r, rest);
      } else {
        r.buf >>= 8 * held;
        r.nbits -= 8 * held;
      }
      pos += (int32_t)len;
    } else {
      // ---- the block's tables
      int nlit = 288, ndist = 32;
      if (btype == 1) {
        PD_LANES_BEGIN(lane)
        for (int i = lane; i < 320; i += kPdLanes) sh.lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : (i < 288 ? 8 : 5))));
        PD_LANES_END
      } else {
        nlit = 257 + (int)pd_bits(r, 5);
        ndist = 1 + (int)pd_bits(r, 5);
        const int ncl = 4 + (int)pd_bits(r, 4);
        for (int i = 0; i < 19; ++i) {
          pd_refill(r);
          const uint8_t v = i < ncl ? (uint8_t)pd_bits(r, 3) : (uint8_t)0;
          if (PD_IS_LANE(0)) sh.cl_lens[kPdClOrder[i]] = v;
        }
        if (pd_past_end(r)) {
          status |= PD_E_EOF;
          break;
        }
        if (nlit > 286 || ndist > 30) {
          status |= PD_E_TABLE;
          break;
        }
        PD_BUILD_TABLE(sh.cl, sh.cl_lens, 19, true)
        if (sh.cl.err) {
          status |= PD_E_TABLE;
          break;
        }
        int i = 0, prev = 0;
        while (i < nlit + ndist && !status) {
          pd_refill(r);
          int sym = 0;
          const int l = pd_code(sh.cl, (uint32_t)r.buf, sym);
          if (l == 0) {
            status |= PD_E_SYMBOL;
            break;
          }
          pd_bits(r, l);
          int rep = 1, v = sym;
          if (sym == 16) {
            if (i == 0) {
              status |= PD_E_TABLE;
              break;
            }
            v = prev;
            rep = 3 + (int)pd_bits(r, 2);
          } else if (sym == 17) {
            v = 0;
            rep = 3 + (int)pd_bits(r, 3);
          } else if (sym == 18) {
            v = 0;
            rep = 11 + (int)pd_bits(r, 7);
          }
          if (i + rep > nlit + ndist) {
            status |= PD_E_TABLE;
            break;
          }
          if (pd_past_end(r)) {
            status |= PD_E_EOF;
            break;
          }
          for (int k = 0; k < rep; ++k, ++i) {
            const int slot = i < nlit ? i : 288 + (i - nlit);
            if (PD_IS_LANE(0)) sh.lens[slot] = (uint8_t)v;
          }
          prev = v;
        }
        if (status) break;
        PD_LANES_BEGIN(lane)
        for (int k = nlit + lane; k < 288; k += kPdLanes) sh.lens[k] = 0;
        for (int k = 288 + ndist + lane; k < 320; k += kPdLanes) sh.lens[k] = 0;
        PD_LANES_END
      }
      PD_BUILD_TABLE(sh.lit, sh.lens, 288, false)
      PD_BUILD_TABLE(sh.dst, sh.lens + 288, 32, false)
      if (sh.lit.err || sh.dst.err || sh.lens[256] == 0) {
        status |= PD_E_TABLE;
        break;
      }
      // ---- batches of up to 64 tokens
      bool eob = false;
      while (!eob && !status) {
        const int32_t pos0 = pos;
        int n = 0;
        while (n < kPdLanes && pos - pos0 < kPdBatchBytes) {
          pd_refill(r);
          int sym = 0;
          int l = pd_code(sh.lit, (uint32_t)r.buf, sym);
          if (l == 0) {
            status |= PD_E_SYMBOL;
            break;
          }
          pd_bits(r, l);
          if (sym == 256) {
            eob = true;
            break;
          }
          int32_t tok = sym, dist = 0, adv = 1;
          if (sym > 256) {
            if (sym >= 286) {
              status |= PD_E_SYMBOL;
              break;
            }
            adv = kPdLenBase[sym - 257] + (int32_t)pd_bits(r, kPdLenExtra[sym - 257]);
            int dsym = 0;
            l = pd_code(sh.dst, (uint32_t)r.buf, dsym);
            if (l == 0 || dsym >= 30) {
              status |= PD_E_SYMBOL;
              break;
            }
            pd_bits(r, l);
            dist = kPdDistBase[dsym] + (int32_t)pd_bits(r, kPdDistExtra[dsym]);
            if (dist > pos) {
              status |= PD_E_DIST;
              break;
            }
            tok = adv;
          }
          if ((int64_t)pos + adv > limit) {
            status |= PD_E_SIZE;
            break;
          }
          if (PD_IS_LANE(n)) {
            sh.rec[n].pos = pos;
            sh.rec[n].tok = tok;
            sh.rec[n].dist = dist;
          }
          pos += adv;
          ++n;
        }
        if (pd_past_end(r)) {                              // the batch used bits that are not there: nothing of it is stored
          status |= PD_E_EOF;
          break;
        }
        if (out && n > 0) {
          PD_LANES_BEGIN(lane)
          if (lane < n && sh.rec[lane].dist == 0) pd_put(sh, out, cap, sh.rec[lane].pos, (uint8_t)sh.rec[lane].tok);
          PD_LANES_END
          for (int k = 0; k < n; ++k) {
            const int32_t dist = sh.rec[k].dist;
            if (dist == 0) continue;
            const int32_t at = sh.rec[k].pos, len = sh.rec[k].tok;
            PD_LANES_BEGIN(lane)
            for (int32_t j = lane; j < len; j += kPdLanes) {
              const int32_t src = at - dist + (j < dist ? j : j % dist);
              pd_put(sh, out, cap, at + j, sh.ring[(uint32_t)src % (uint32_t)kPdRing]);
            }
            PD_LANES_END
          }
        }
      }
      if (status) break;
    }
    // ---- a block boundary
    if (bfinal) {
      final_seen = true;
      exact = (pd_used_bits(r) + 7) / 8 * 8 == nbits_stream;
      break;
    }
    if (pd_used_bits(r) >= nbits_stream) {
      exact = pd_used_bits(r) == nbits_stream;
      break;
    }
  }
  res.produced = pos;
  res.status = status;
  res.final_seen = final_seen ? 1 : 0;
  res.exact = (exact && !status) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ unfiltering

SFH_HD int pd_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// One pixel, its bytes in one register (channel k in byte k): the filtered bytes `raw` under filter f (0 .. 4) with the pixel to
// the left a, the one above b and the one above left c -> the pixel.
SFH_HD uint32_t pd_recon(int f, uint32_t raw, uint32_t a, uint32_t b, uint32_t c, int C) {
  uint32_t v = 0;
  for (int k = 0; k < C; ++k) {
    const int sh = 8 * k;
    const int x = (raw >> sh) & 255, pa = (a >> sh) & 255, pb = (b >> sh) & 255, pc = (c >> sh) & 255;
    const int pred = f == 0 ? 0 : (f == 1 ? pa : (f == 2 ? pb : (f == 3 ? (pa + pb) >> 1 : pd_paeth(pa, pb, pc))));
    v |= (uint32_t)((x + pred) & 255) << sh;
  }
  return v;
}

// where channel k of the file lies in a pixel of the output
SFH_HD int pd_out_channel(int k, int C, int bgr) { return (bgr && C >= 3 && k < 3) ? 2 - k : k; }
