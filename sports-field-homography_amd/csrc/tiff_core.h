// tiff_core.h - the core of sfh_amd.tiffdec and sfh_amd.tiffenc as plain functions that compile for the host and for the device:
// the parse of a classic TIFF's header and first IFD, the TIFF 6.0 LZW decode of one strip by one wave, the copy of an
// uncompressed strip, the arithmetic of one sample (byte order, horizontal differencing), and the greedy LZW encode of one strip.
// csrc/tiffdec.hip and csrc/tiffenc.hip run the strip functions in a 64-thread workgroup; tests/tiff_host_main.cpp runs them lane
// by lane under the sanitizers.  Nothing here includes a HIP header.  The written-down rule both are held to is
// outputs.decode_tiff / outputs.encode_tiff.
//
// Lanes: the convention of pngdec_core.h.  Code outside a lane section is UNIFORM - every lane runs it on the same values and
// only one lane (TD_IS_LANE) stores; a lane section TD_LANES_BEGIN(lane) ... TD_LANES_END stands between two workgroup barriers
// on the device and is a loop over the 64 lanes on the host - correct because no lane of a section reads what another lane of
// the same section writes.  TD_SYNC() is the barrier alone.
//
// The decoder's dictionary.  Every LZW string is a substring of the bytes already decoded, so entry e is (position in the strip's
// decoded bytes, length) - 4096 x (u32 + u16) = 24 KB of LDS - and a code is a copy the whole wave performs, 64 bytes a step, from
// pos + (k mod dist) with dist = the write position - pos.  The entry a code adds is (where the previous code's string was
// written, its length + 1): the previous string and, next to it in the output, the first byte of this one.  For the code that
// equals the entry being added (KwKwK) dist is the previous length, and k mod dist wraps the last byte onto the first.
// The earlier bytes are read back from the strip's slot in global memory: the same workgroup stored them, in an earlier lane
// section, and the workgroup barrier between the sections orders that load behind the store.
//
// Bounds.  The bytes are not trusted.  A read at or past the strip's byte count gives zero; a decode that used such bits ends with
// TD_E_EOF.  Every store is guarded by the strip's `total` bytes.  Every code uses at least 9 bits, so a decode ends.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/sfh_amd.h"
#include "codec_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TD_LANES_BEGIN(lane) \
  __syncthreads();           \
  {                          \
    const int lane = (int)threadIdx.x;
#define TD_LANES_END \
  }                  \
  __syncthreads();
#define TD_IS_LANE(i) ((int)threadIdx.x == (i))
#define TD_SYNC() __syncthreads()
#else
#define TD_LANES_BEGIN(lane) for (int lane = 0; lane < kTdLanes; ++lane) {
#define TD_LANES_END }
#define TD_IS_LANE(i) true
#define TD_SYNC() \
  do {            \
  } while (0)
#endif

constexpr int kTdLanes = 64;
constexpr int kTdCodes = 4096;
constexpr int kTdClear = 256, kTdEoi = 257, kTdFirst = 258;

// status bits of an image (TiffDecoder.status): the OR over its strips
enum {
  TD_E_CODE = 1,    // a code above the next free code
  TD_E_FIRST = 2,   // a first code after Clear that is not a literal
  TD_E_SIZE = 4,    // output short of or beyond the strip's rows * W * C * bytes
  TD_E_EOF = 8      // the bits end early
};

// ------------------------------------------------------------------------------------------------------------ the host parse
inline uint32_t td_u16(const uint8_t* p, bool be) { return be ? ((uint32_t)p[0] << 8) | p[1] : ((uint32_t)p[1] << 8) | p[0]; }
inline uint32_t td_u32(const uint8_t* p, bool be) {
  return be ? get_be32(p) : ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
}

// an IFD entry of BYTE, SHORT or LONG values whose array lies inside the file
struct TdEntry {
  const uint8_t* base;   // the first value; nullptr: the tag is absent
  uint32_t count;
  int size;
};

inline uint32_t td_value(const TdEntry& e, uint32_t i, bool be) {
  const uint8_t* p = e.base + (size_t)e.size * i;
  return e.size == 1 ? p[0] : (e.size == 2 ? td_u16(p, be) : td_u32(p, be));
}

// Header and first IFD of a classic TIFF -> *info and, when host_strips is given, the first min(nstrips, strip_cap) records
// {offset, byte count, first row, rows} of the strip table.  0, or -1 with info->reason = SFH_TIFF_R_*.  Every offset the file
// states - the IFD, every tag array, every strip - is checked against the n bytes here.
inline int td_parse(const uint8_t* d, int64_t n, sfh_tiff_info* info, int32_t* host_strips, int64_t strip_cap) {
  memset(info, 0, sizeof(*info));
  auto refuse = [&](int reason) {
    info->reason = reason;
    return -1;
  };
  if (n >= ((int64_t)1 << 31)) return refuse(SFH_TIFF_R_TOO_LONG);
  if (n < 2) return refuse(SFH_TIFF_R_TRUNCATED);
  const bool be = d[0] == 'M' && d[1] == 'M';
  if (!be && !(d[0] == 'I' && d[1] == 'I')) return refuse(SFH_TIFF_R_NOT_TIFF);
  if (n < 4) return refuse(SFH_TIFF_R_TRUNCATED);
  const uint32_t magic = td_u16(d + 2, be);
  if (magic == 43) return refuse(SFH_TIFF_R_BIGTIFF);
  if (magic != 42) return refuse(SFH_TIFF_R_NOT_TIFF);
  if (n < 8) return refuse(SFH_TIFF_R_TRUNCATED);
  const int64_t ifd = td_u32(d + 4, be);
  if (ifd < 8 || ifd + 2 > n) return refuse(SFH_TIFF_R_BAD_IFD);
  const int64_t nent = td_u16(d + ifd, be);
  if (ifd + 2 + 12 * nent > n) return refuse(SFH_TIFF_R_BAD_IFD);

  enum { T_W, T_H, T_BITS, T_COMP, T_PHOTO, T_FILL, T_OFF, T_SPP, T_RPS, T_CNT, T_PLANAR, T_PRED, T_FMT, T_N };
  const int tags[T_N] = {256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 339};
  TdEntry e[T_N];
  for (int k = 0; k < T_N; ++k) e[k] = TdEntry{nullptr, 0, 0};
  bool tiles = false;
  for (int64_t i = 0; i < nent; ++i) {
    const uint8_t* p = d + ifd + 2 + 12 * i;
    const int tag = (int)td_u16(p, be);
    if (tag >= 322 && tag <= 325) tiles = true;
    for (int k = 0; k < T_N; ++k) {
      if (tag != tags[k]) continue;
      const int type = (int)td_u16(p + 2, be);
      const uint32_t count = td_u32(p + 4, be);
      const int size = type == 1 ? 1 : (type == 3 ? 2 : (type == 4 ? 4 : 0));
      if (!size || count < 1) return refuse(SFH_TIFF_R_BAD_TAG);
      const int64_t bytes = (int64_t)size * count;
      const uint8_t* base = p + 8;
      if (bytes > 4) {
        const int64_t off = td_u32(p + 8, be);
        if (off + bytes > n) return refuse(SFH_TIFF_R_BAD_TAG);
        base = d + off;
      }
      e[k] = TdEntry{base, count, size};
    }
  }
  if (tiles) return refuse(SFH_TIFF_R_TILES);
  if (!e[T_W].base || !e[T_H].base || !e[T_PHOTO].base || !e[T_OFF].base || !e[T_CNT].base) return refuse(SFH_TIFF_R_MISSING_TAG);
  auto first = [&](int k, uint32_t dflt) { return e[k].base ? td_value(e[k], 0, be) : dflt; };
  const uint32_t W = first(T_W, 0), H = first(T_H, 0);
  if (W < 1 || H < 1 || W >= (1u << 24) || H >= (1u << 24)) return refuse(SFH_TIFF_R_BAD_VALUE);
  const uint32_t spp = first(T_SPP, 1);
  if (spp != 1 && spp != 3) return refuse(SFH_TIFF_R_SAMPLES);
  const uint32_t bits = first(T_BITS, 1);
  if (bits != 8 && bits != 16) return refuse(SFH_TIFF_R_BIT_DEPTH);
  if (e[T_BITS].base && e[T_BITS].count != 1 && e[T_BITS].count != spp) return refuse(SFH_TIFF_R_BAD_VALUE);
  for (uint32_t i = 1; e[T_BITS].base && i < e[T_BITS].count; ++i)
    if (td_value(e[T_BITS], i, be) != bits) return refuse(SFH_TIFF_R_BIT_DEPTH);
  for (uint32_t i = 0; e[T_FMT].base && i < e[T_FMT].count; ++i)
    if (td_value(e[T_FMT], i, be) != 1) return refuse(SFH_TIFF_R_SAMPLE_FORMAT);
  const uint32_t comp = first(T_COMP, 1);
  if (comp != 1 && comp != 5) return refuse(SFH_TIFF_R_COMPRESSION);
  const uint32_t photo = first(T_PHOTO, 0);
  if (photo != (spp == 1 ? 1u : 2u)) return refuse(SFH_TIFF_R_PHOTOMETRIC);
  if (spp > 1 && first(T_PLANAR, 1) != 1) return refuse(SFH_TIFF_R_PLANAR);
  if (first(T_FILL, 1) != 1) return refuse(SFH_TIFF_R_FILL_ORDER);
  const uint32_t pred = first(T_PRED, 1);
  if (pred != 1 && pred != 2) return refuse(SFH_TIFF_R_PREDICTOR);
  uint32_t rps = first(T_RPS, 0xFFFFFFFFu);
  if (rps < 1) return refuse(SFH_TIFF_R_BAD_VALUE);
  if (rps > H) rps = H;
  const uint32_t nstrips = (H + rps - 1) / rps;
  if (e[T_OFF].count != nstrips || e[T_CNT].count != nstrips) return refuse(SFH_TIFF_R_STRIP_TABLE);
  info->width = (int32_t)W;
  info->height = (int32_t)H;
  info->channels = (int32_t)spp;
  info->bits = (int32_t)bits;
  info->compression = (int32_t)comp;
  info->predictor = comp == 5 ? (int32_t)pred : 1;       // libtiff applies a predictor inside its LZW codec only
  info->big_endian = be ? 1 : 0;
  info->rows_per_strip = (int32_t)rps;
  info->nstrips = (int32_t)nstrips;
  info->photometric = (int32_t)photo;
  for (uint32_t s = 0; s < nstrips; ++s) {
    const int64_t off = td_value(e[T_OFF], s, be), cnt = td_value(e[T_CNT], s, be);
    if (off + cnt > n) return refuse(SFH_TIFF_R_STRIP);
    // libtiff's test for the bit-reversed LZW of old writers: their Clear code puts 00 01 at the start of a strip
    if (comp == 5 && cnt >= 2 && d[off] == 0 && (d[off + 1] & 1)) return refuse(SFH_TIFF_R_OLD_LZW);
    if (host_strips && (int64_t)s < strip_cap) {
      int32_t* rec = host_strips + 4 * (int64_t)s;
      rec[0] = (int32_t)off;
      rec[1] = (int32_t)cnt;
      rec[2] = (int32_t)(s * rps);
      rec[3] = (int32_t)(H - s * rps < rps ? H - s * rps : rps);
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ one strip, decoded
struct TdShared {
  uint32_t pos[kTdCodes];
  uint16_t len[kTdCodes];
};

// an uncompressed strip: n file bytes -> the `total` bytes of its slot, 64 bytes a step
SFH_HD int td_copy_strip(const uint8_t* src, int32_t n, uint8_t* out, int32_t total) {
  const int32_t m = n < total ? n : total;
  TD_LANES_BEGIN(lane)
  for (int32_t i = lane; i < m; i += kTdLanes) out[i] = src[i];
  TD_LANES_END
  return n < total ? TD_E_SIZE : 0;
}

// a TIFF 6.0 LZW strip (MSB-first codes of 9 .. 12 bits, Clear 256, EOI 257, the early change of width): n file bytes -> the
// `total` bytes of its slot -> the TD_E_* bits.  The decode ends when the slot is complete: an EOI is not needed and whatever
// follows it inside the byte count is not read.
SFH_HD int td_lzw_strip(const uint8_t* src, int32_t n, TdShared& sh, uint8_t* out, int32_t total) {
  uint64_t acc = 0;
  int nbits = 0;
  int32_t ip = 0;
  int64_t used = 0;
  int width = 9, next = kTdFirst;
  bool fresh = true;                     // no code since the last Clear (a strip starts as after a Clear)
  int32_t o = 0, prev_o = 0, prev_len = 0;
  while (o < total) {
    while (nbits < width) {
      acc = (acc << 8) | (uint64_t)(ip < n ? src[ip] : 0);
      ++ip;
      nbits += 8;
    }
    const int code = (int)((acc >> (nbits - width)) & ((1u << width) - 1u));
    nbits -= width;
    used += width;
    if (used > 8 * (int64_t)n) return TD_E_EOF;
    if (code == kTdClear) {
      width = 9;
      next = kTdFirst;
      fresh = true;
      continue;
    }
    if (code == kTdEoi) return TD_E_SIZE;                  // o < total
    int32_t pos = o, len = 1;
    if (fresh) {
      if (code > 255) return TD_E_FIRST;
    } else {
      const bool room = next < kTdCodes;
      if (code > next || (code == next && !room)) return TD_E_CODE;
      if (code == next) {
        pos = prev_o;
        len = prev_len + 1;
      } else if (code > 255) {
        pos = (int32_t)sh.pos[code];
        len = (int32_t)sh.len[code];
      }
      if (room) {
        if (TD_IS_LANE(0)) {
          sh.pos[next] = (uint32_t)prev_o;
          sh.len[next] = (uint16_t)(prev_len + 1);           // at most 1 + the number of entries
        }
        ++next;
        if (next == (1 << width) - 1 && width < 12) ++width;   // the early change
      }
    }
    if (len > total - o) return TD_E_SIZE;
    const int32_t dist = o - pos;                          // 0 only for a literal
    TD_LANES_BEGIN(lane)
    if (code < 256) {
      if (lane == 0) out[o] = (uint8_t)code;
    } else {
      for (int32_t k = lane; k < len; k += kTdLanes) out[o + k] = out[pos + k % dist];
    }
    TD_LANES_END
    prev_o = o;
    prev_len = len;
    o += len;
    fresh = false;
  }
  return 0;
}

// sample s of a decoded row (the file's byte order) -> its value
SFH_HD uint32_t td_sample(const uint8_t* row, int64_t s, int bits, int big_endian) {
  if (bits == 8) return row[s];
  const uint8_t* p = row + 2 * s;
  return big_endian ? ((uint32_t)p[0] << 8) | p[1] : ((uint32_t)p[1] << 8) | p[0];
}

SFH_HD int td_out_channel(int k, int C, int bgr) { return (bgr && C == 3) ? 2 - k : k; }

// ------------------------------------------------------------------------------------------------------------ one strip, encoded
// Greedy LZW as libtiff writes it: Clear first; the longest match in the dictionary; the width grows when the next free code
// reaches 1 << width; Clear and restart when the next free code reaches 4094; the last code, then EOI at the width the decoder
// expects there; the final byte zero-padded.  The dictionary is a hash table keyed by (prefix code, byte): 8192 words of
// (key << 12 | code), linear probing, at most 3836 entries (load below 47 %).
constexpr int kTeHashBits = 13;
constexpr int kTeHash = 1 << kTeHashBits;
constexpr int kTeChunk = 4096;
constexpr int kTeFull = 4094;
constexpr uint32_t kTeEmpty = 0xFFFFFFFFu;

struct TeShared {
  uint32_t hash[kTeHash];
  uint8_t chunk[kTeChunk];
};

struct TeGeom {
  int H, W, C, bits, bgr, predictor;
};

// The slot of a strip of n bytes.  Uncompressed: n.  LZW: every code but Clear and EOI consumes at least one byte, so there are
// at most n data codes; a Clear opens the strip and follows every 3836 entries (codes 258 .. 4093), one entry per data code, so
// there are at most 1 + n / 3836 + 1 of them (the last: the post-encode step may clear as well); one EOI.  No code has more than
// 12 bits, and the last byte is padded: ceil(12 (n + n / 3836 + 3) / 8) bytes.  One code of slack on top.
SFH_HD int64_t te_strip_capacity(int64_t n, int compression) {
  return compression == 1 ? n : (12 * (n + n / 3836 + 4) + 7) / 8;
}

// byte i of the strip that starts at row0, as the file holds it before compression: the file's channel order, little endian,
// differenced at a stride of C samples modulo 2^bits with predictor 2
SFH_HD uint8_t te_raw_byte(const void* img, const TeGeom& g, int row0, int32_t i) {
  const int bps = g.bits / 8;
  const int32_t rowbytes = g.W * g.C * bps;
  const int y = row0 + i / rowbytes;
  const int32_t j = i % rowbytes;
  const int32_t s = j / bps;
  const int x = s / g.C, k = td_out_channel(s % g.C, g.C, g.bgr);
  const int64_t idx = ((int64_t)y * g.W + x) * g.C + k;
  uint32_t v, p = 0;
  if (g.bits == 16) {
    const uint16_t* im = static_cast<const uint16_t*>(img);
    v = im[idx];
    if (g.predictor == 2 && x > 0) p = im[idx - g.C];
  } else {
    const uint8_t* im = static_cast<const uint8_t*>(img);
    v = im[idx];
    if (g.predictor == 2 && x > 0) p = im[idx - g.C];
  }
  return (uint8_t)(((v - p) >> (8 * (j % bps))) & 255u);
}

SFH_HD void te_clear(TeShared& sh) {
  TD_LANES_BEGIN(lane)
  for (int i = lane; i < kTeHash; i += kTdLanes) sh.hash[i] = kTeEmpty;
  TD_LANES_END
}

// rows [row0, row0 + rows) of image `img` -> the strip's slot of `cap` bytes -> the strip's byte count (never more is stored
// than cap; te_strip_capacity is never exceeded)
SFH_HD int32_t te_encode_strip(const void* img, const TeGeom& g, int row0, int rows, int compression, TeShared& sh, uint8_t* slot,
                               int32_t cap) {
  const int32_t n = rows * g.W * g.C * (g.bits / 8);
  if (compression == 1) {
    TD_LANES_BEGIN(lane)
    for (int32_t i = lane; i < n && i < cap; i += kTdLanes) slot[i] = te_raw_byte(img, g, row0, i);
    TD_LANES_END
    return n;
  }
  uint32_t acc = 0;
  int nb = 0;
  int32_t op = 0;
  auto put = [&](int code, int width) {
    acc = ((acc << width) | (uint32_t)code) & 0xFFFFFu;    // nb < 8 before: at most 20 bits
    nb += width;
    while (nb >= 8) {
      if (TD_IS_LANE(0) && op < cap) slot[op] = (uint8_t)(acc >> (nb - 8));
      ++op;
      nb -= 8;
    }
  };
  int width = 9, next = kTdFirst, ent = -1;
  te_clear(sh);
  put(kTdClear, width);
  for (int32_t c0 = 0; c0 < n; c0 += kTeChunk) {
    const int32_t m = n - c0 < kTeChunk ? n - c0 : kTeChunk;
    TD_LANES_BEGIN(lane)
    for (int32_t i = lane; i < m; i += kTdLanes) sh.chunk[i] = te_raw_byte(img, g, row0, c0 + i);
    TD_LANES_END
    for (int32_t i = 0; i < m; ++i) {
      const int c = sh.chunk[i];
      if (ent < 0) {
        ent = c;
        continue;
      }
      const uint32_t key = ((uint32_t)ent << 8) | (uint32_t)c;
      uint32_t h = (key * 2654435761u) >> (32 - kTeHashBits);
      int found = -1;
      for (uint32_t v = sh.hash[h]; v != kTeEmpty; v = sh.hash[h]) {
        if ((v >> 12) == key) {
          found = (int)(v & 4095u);
          break;
        }
        h = (h + 1) & (kTeHash - 1);
      }
      if (found >= 0) {
        ent = found;
        continue;
      }
      put(ent, width);
      if (TD_IS_LANE(0)) sh.hash[h] = (key << 12) | (uint32_t)next;
      TD_SYNC();
      ++next;
      ent = c;
      if (next == kTeFull) {
        put(kTdClear, width);
        te_clear(sh);
        width = 9;
        next = kTdFirst;
      } else if (next > (1 << width) - 1) {
        ++width;
      }
    }
  }
  if (ent >= 0) {
    put(ent, width);
    ++next;
    if (next == kTeFull) {
      put(kTdClear, width);
      width = 9;
    } else if (next > (1 << width) - 1) {
      ++width;
    }
  }
  put(kTdEoi, width);
  if (nb > 0) {
    if (TD_IS_LANE(0) && op < cap) slot[op] = (uint8_t)((acc << (8 - nb)) & 255u);
    ++op;
  }
  return op;
}

// rows of a strip by default: about 8 KB, libtiff's choice
SFH_HD int te_default_rows(int H, int W, int C, int bits) {
  const int64_t rowbytes = (int64_t)W * C * (bits / 8);
  int64_t r = 8192 / rowbytes;
  r = r < 1 ? 1 : r;
  return (int)(r > H ? H : r);
}
