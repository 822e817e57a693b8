// jpegdec_core.h - the decode core of sfh_amd.jpegdec as plain functions that compile for the host and for the device: the marker
// parse, the bit reader, the code lookup, the state step, the per-lane phases of the subsequence algorithm and their bounds rules.
// csrc/jpegdec.hip runs the lane phases in a workgroup; tests/jpegdec_host_main.cpp runs them lane by lane under the sanitizers.
// Nothing here includes a HIP header.  The rule is restated in tests/jpegdec_ref.py.
//
// Positions.  A segment is the entropy-coded bytes between two markers, [lo, hi) of the buffer `data`.  A bit position p counts RAW
// bits from the segment's first byte, stuffed bytes included.  Byte k of the segment is a STUFFING byte iff it is 0x00 and byte
// k - 1 is 0xFF; a position never lies inside a stuffing byte (jd_normalise, jd_advance keep that).  Whether a byte is stuffing is a
// function of the bytes alone, so the serial decode and every speculative decode read the same bits at the same position.
//
// Bounds.  No byte outside [lo, hi) is ever used: jd_peek loads the aligned dwords that cover [lo + k, lo + k + 9) and zeroes
// the bytes at or beyond hi, so `data` must be 4-byte aligned and readable up to hi rounded up to a multiple of 4 (the staging
// layout guarantees both; a dword that starts at or beyond hi is not loaded).  Every coefficient store is guarded by the segment's
// block count.  Every step advances p by at least one bit, so a decode of [p, end) takes at most end - p steps.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/sfh_amd.h"
#include "codec_common.h"

enum { JD_E_CODE = 1, JD_E_RUN = 2, JD_E_EOF = 4, JD_E_BLOCKS = 8 };   // status bits of a segment

struct JdState {
  int32_t p;    // raw bit position in the segment
  int32_t st;   // block index within the MCU << 8 | zig-zag index of the next coefficient (0: the next code is a DC code)
};
struct JdExit {
  int32_t p, st;
  int32_t nblk;   // blocks completed by the decode that produced this exit
};
struct JdEvent {
  int32_t k;      // zig-zag index of the coefficient this step produced, -1: none (EOB, ZRL, an error)
  int32_t value;  // the coefficient (k == 0: the DC DIFFERENCE)
  int32_t done;   // the step completed a block
  int32_t err;    // JD_E_* of this step
};
struct JdCtx {
  const uint8_t* data;   // 4-byte aligned
  int32_t lo, hi;        // the segment's bytes
  int32_t nbits;         // (hi - lo) * 8
  int32_t bpm;           // blocks per MCU
  const sfh_jpeg_hufftab* dc;   // [4]
  const sfh_jpeg_hufftab* ac;   // [4]
  const uint8_t* blk_dc;        // [bpm] table of block j of an MCU
  const uint8_t* blk_ac;
};
struct JdPeek {
  uint32_t bits;    // the 32 data bits from p on, first bit highest
  uint32_t skips;   // nibble q: stuffing bytes between the byte of p and the q-th data byte after it
};

SFH_HD int jd_byte(const JdCtx& c, int32_t k) { return (k >= 0 && k < c.hi - c.lo) ? c.data[c.lo + k] : 0; }

// a guessed position: not inside a stuffing byte
SFH_HD int32_t jd_normalise(const JdCtx& c, int32_t p) {
  const int32_t k = p >> 3;
  return (k > 0 && jd_byte(c, k) == 0 && jd_byte(c, k - 1) == 0xFF) ? ((k + 1) << 3) : p;
}

SFH_HD JdPeek jd_peek(const JdCtx& c, int32_t p) {
  const int64_t a = (int64_t)c.lo + (p >> 3);           // absolute index of the byte of p
  const int64_t nv = (int64_t)c.hi - a;                 // bytes from there to the segment's end (may be <= 0)
  const int64_t w = a >> 2;
  const uint32_t* dw = reinterpret_cast<const uint32_t*>(c.data);
  uint32_t d[3];                                        // bytes a .. a + 8 lie in the dwords w, w + 1, w + 2
  for (int j = 0; j < 3; ++j) d[j] = (4 * (w + j) < (int64_t)c.hi && nv > 0) ? dw[w + j] : 0u;
  const int sh = 8 * (int)(a & 3);
  uint64_t r64 = (uint64_t)d[0] | ((uint64_t)d[1] << 32);
  if (sh) r64 = (r64 >> sh) | ((uint64_t)d[2] << (64 - sh));
  uint32_t r8 = (d[2] >> sh) & 255u;
  if (nv < 8) r64 = nv <= 0 ? 0ull : (r64 & ((1ull << (8 * nv)) - 1ull));
  if (nv < 9) r8 = 0u;
  uint64_t acc = 0;
  uint32_t skips = 0, ns = 0, prev = 0x100u;
  int nd = 0;
  for (int j = 0; j < 9; ++j) {
    const uint32_t b = j < 8 ? (uint32_t)((r64 >> (8 * j)) & 255u) : r8;
    if (j > 0 && prev == 0xFFu && b == 0u) {
      ++ns;
      prev = 0u;
      continue;
    }
    if (nd < 5) {
      acc = (acc << 8) | b;
      skips |= ns << (4 * nd);
      ++nd;
    }
    prev = b;
  }
  // 9 raw bytes hold at least 5 data bytes (a stuffing byte follows a data byte): acc has 40 bits
  JdPeek pk;
  pk.bits = (uint32_t)((acc << (24 + (p & 7))) >> 32);
  pk.skips = skips;
  return pk;
}

// p advanced by n data bits (n <= 31)
SFH_HD int32_t jd_advance(const JdPeek& pk, int32_t p, int n) {
  const int t = (p & 7) + n;
  const int q = t >> 3;   // <= 4
  return (((p >> 3) + q + (int32_t)((pk.skips >> (4 * q)) & 15u)) << 3) | (t & 7);
}

// the code at the top of b16 -> length (0: no such code) and symbol
SFH_HD int jd_code(const sfh_jpeg_hufftab& t, uint32_t b16, int& sym) {
  const uint32_t e = t.look[b16 >> 8];
  if (e) {
    sym = (int)(e & 255u);
    return (int)(e >> 8);
  }
  for (int l = 9; l <= 16; ++l) {
    const int32_t code = (int32_t)(b16 >> (16 - l));
    if (code <= t.maxcode[l]) {
      sym = t.vals[(code + t.valoff[l]) & 255];
      return l;
    }
  }
  return 0;
}

SFH_HD void jd_step(const JdCtx& c, JdState& s, JdEvent& e) {
  const JdPeek pk = jd_peek(c, s.p);
  int blk = s.st >> 8, zz = s.st & 255;
  const bool isdc = zz == 0;
  const sfh_jpeg_hufftab& t = isdc ? c.dc[c.blk_dc[blk] & 3] : c.ac[c.blk_ac[blk] & 3];
  e.k = -1;
  e.value = 0;
  e.done = 0;
  e.err = 0;
  int sym = 0;
  const int len = jd_code(t, pk.bits >> 16, sym);
  if (len == 0) {                                       // no such code: 16 bits on, the state as it was
    e.err = JD_E_CODE;
    s.p = jd_advance(pk, s.p, 16);
    if (s.p > c.nbits) e.err |= JD_E_EOF;
    return;
  }
  const int sz = sym & 15, run = isdc ? 0 : (sym >> 4);
  int v = 0;
  if (sz) {
    v = (int)((pk.bits << len) >> (32 - sz));
    if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
  }
  bool done = false;
  if (isdc) {
    e.k = 0;
    e.value = v;
    zz = 1;
  } else if (sz == 0) {
    if (run == 15) {                                    // ZRL
      zz += 16;
      if (zz > 64) e.err = JD_E_RUN;
      done = zz >= 64;
    } else {
      done = true;                                      // EOB
    }
  } else {
    zz += run;
    if (zz > 63) {
      e.err = JD_E_RUN;
      done = true;
    } else {
      e.k = zz;
      e.value = v;
      done = ++zz == 64;
    }
  }
  if (done) {
    blk = blk + 1 == c.bpm ? 0 : blk + 1;
    zz = 0;
    e.done = 1;
  }
  s.st = (blk << 8) | zz;
  s.p = jd_advance(pk, s.p, len + sz);
  if (s.p > c.nbits) e.err |= JD_E_EOF;
}

SFH_HD int32_t jd_sub_end(const JdCtx& c, int32_t i, int32_t subseq_bits) {
  const int64_t e = ((int64_t)i + 1) * subseq_bits;
  return e < c.nbits ? (int32_t)e : c.nbits;
}

SFH_HD int32_t jd_nsub(int32_t nbytes, int32_t subseq_bits) {
  const int64_t n = ((int64_t)nbytes * 8 + subseq_bits - 1) / subseq_bits;
  return n < 1 ? 1 : (int32_t)n;
}

// One round of the fixed-point iteration for lane `tid` of `nth`: subsequence i is decoded from the exit of i - 1 of the round
// before (`prev`), its exit goes to `cur`.  Round 0 starts subsequence 0 at the true start and every other one at a guess.
// lastin[i]: the state i was last decoded from - the same entry state gives the same exit, so that decode is not repeated.
// -> whether an exit of this lane changed.
SFH_HD bool jd_round_lane(const JdCtx& c, int32_t subseq_bits, int32_t nsub, int32_t round, int tid, int nth, const JdExit* prev,
                          JdExit* cur, JdState* lastin) {
  bool changed = false;
  for (int32_t i = tid; i < nsub; i += nth) {
    JdState in;
    if (round == 0) {
      in.p = i == 0 ? 0 : jd_normalise(c, (int32_t)((int64_t)i * subseq_bits));
      in.st = 0;
    } else if (i < round) {                             // correct since round i
      cur[i] = prev[i];
      continue;
    } else {
      in.p = prev[i - 1].p;
      in.st = prev[i - 1].st;
      if (in.p == lastin[i].p && in.st == lastin[i].st) {
        cur[i] = prev[i];
        continue;
      }
    }
    lastin[i] = in;
    const int32_t end = jd_sub_end(c, i, subseq_bits);
    JdState s = in;
    JdEvent e;
    int32_t nblk = 0;
    while (s.p < end) {
      jd_step(c, s, e);
      nblk += e.done;
    }
    if (round == 0 || s.p != prev[i].p || s.st != prev[i].st || nblk != prev[i].nblk) changed = true;
    cur[i].p = s.p;
    cur[i].st = s.st;
    cur[i].nblk = nblk;
  }
  return changed;
}

// The last pass for lane `tid`: every subsequence once more from its true entry state, its first block base[i]; coefficients of
// the segment's blocks [0, nblocks) go to coef (int16, natural order, the DC as a difference); -> JD_E_* of those blocks.
SFH_HD int jd_final_lane(const JdCtx& c, int32_t subseq_bits, int32_t nsub, int tid, int nth, const JdExit* exits,
                         const int32_t* base, int16_t* coef, int32_t nblocks) {
  int err = 0;
  for (int32_t i = tid; i < nsub; i += nth) {
    JdState s;
    s.p = i == 0 ? 0 : exits[i - 1].p;
    s.st = i == 0 ? 0 : exits[i - 1].st;
    int32_t ab = base[i];
    const int32_t end = jd_sub_end(c, i, subseq_bits);
    JdEvent e;
    while (s.p < end) {
      jd_step(c, s, e);
      if (ab >= 0 && ab < nblocks) {
        err |= e.err;
        if (e.k >= 0) coef[(int64_t)ab * 64 + kJpegNatural[e.k & 63]] = (int16_t)e.value;
      }
      ab += e.done;
    }
  }
  return err;
}

// ------------------------------------------------------------------------------------------------------------ the marker parse

namespace jdparse {

inline int fail(sfh_jpeg_info* info, int reason) {
  info->reason = reason;
  return -1;
}

// canonical codes of one DHT table (Annex C) in the lookup form jd_code reads; false: the counts overflow a length
inline bool build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, sfh_jpeg_hufftab* t) {
  memset(t, 0, sizeof(*t));
  for (int i = 0; i < nvals; ++i) t->vals[i] = vals[i];
  int32_t code = 0, k = 0;
  t->maxcode[0] = -1;
  for (int l = 1; l <= 16; ++l) {
    t->valoff[l] = k - code;
    const int n = bits[l - 1];
    if (n) {
      if (l <= 8)
        for (int i = 0; i < n; ++i)
          for (int f = 0; f < (1 << (8 - l)); ++f) {
            const int idx = ((code + i) << (8 - l)) + f;
            if (idx < 256) t->look[idx] = (uint16_t)((l << 8) | vals[k + i]);
          }
      k += n;
      code += n;
      if (code > (1 << l)) return false;
      t->maxcode[l] = code - 1;
    } else {
      t->maxcode[l] = -1;
    }
    code <<= 1;
  }
  t->maxcode[17] = 0x7FFFFFFF;
  return true;
}

}  // namespace jdparse

// bytes[0, n) -> info, and up to seg_cap segments {first byte, end byte, first MCU, 0} as int32 quadruples in segs (may be null
// when seg_cap is 0); info->nsegments counts all of them.  0, or -1 with info->reason = SFH_JPEG_R_*.
inline int jd_parse(const uint8_t* bytes, int64_t n, sfh_jpeg_info* info, int32_t* segs, int64_t seg_cap) {
  using namespace jdparse;
  memset(info, 0, sizeof(*info));
  if (!bytes || n < 4) return fail(info, SFH_JPEG_R_TRUNCATED);
  if (n >= ((int64_t)1 << 28)) return fail(info, SFH_JPEG_R_TOO_LONG);
  if (bytes[0] != 0xFF || bytes[1] != 0xD8) return fail(info, SFH_JPEG_R_NOT_JPEG);
  bool have_q[4] = {false, false, false, false}, have_dc[4] = {false, false, false, false}, have_ac[4] = {false, false, false, false};
  bool jfif = false, adobe = false, sof = false;
  int adobe_transform = -1;
  int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0};
  int64_t i = 2;
  for (;;) {
    if (i + 2 > n) return fail(info, SFH_JPEG_R_TRUNCATED);
    if (bytes[i] != 0xFF) return fail(info, SFH_JPEG_R_MARKER);
    while (i < n && bytes[i] == 0xFF) ++i;              // fill bytes
    if (i >= n) return fail(info, SFH_JPEG_R_TRUNCATED);
    const int m = bytes[i++];
    if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return fail(info, SFH_JPEG_R_MARKER);
    if (i + 2 > n) return fail(info, SFH_JPEG_R_TRUNCATED);
    const int len = get_be16(bytes + i);
    if (len < 2 || i + len > n) return fail(info, SFH_JPEG_R_TRUNCATED);
    const uint8_t* b = bytes + i + 2;
    const int bl = len - 2;
    if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) return fail(info, SFH_JPEG_R_PROGRESSIVE);
    if (m == 0xC9 || m == 0xCB || m == 0xCD || m == 0xCF || m == 0xCC) return fail(info, SFH_JPEG_R_ARITHMETIC);
    if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC7 || m == 0xDE || m == 0xDF) return fail(info, SFH_JPEG_R_SOF_TYPE);
    if (m == 0xDC) return fail(info, SFH_JPEG_R_DNL);
    if (m == 0xC0) {
      if (sof) return fail(info, SFH_JPEG_R_MARKER);
      if (bl < 6) return fail(info, SFH_JPEG_R_TRUNCATED);
      if (b[0] != 8) return fail(info, b[0] == 12 ? SFH_JPEG_R_PRECISION : SFH_JPEG_R_BAD_SOF);
      info->height = get_be16(b + 1);
      info->width = get_be16(b + 3);
      info->ncomp = b[5];
      if (info->width == 0) return fail(info, SFH_JPEG_R_BAD_SOF);
      if (info->height == 0) return fail(info, SFH_JPEG_R_DNL);
      if (info->ncomp == 4) return fail(info, SFH_JPEG_R_COMPONENTS);
      if (info->ncomp != 1 && info->ncomp != 3) return fail(info, info->ncomp == 2 ? SFH_JPEG_R_COMPONENTS : SFH_JPEG_R_BAD_SOF);
      if (bl != 6 + 3 * info->ncomp) return fail(info, SFH_JPEG_R_BAD_SOF);
      for (int c = 0; c < info->ncomp; ++c) {
        comp_id[c] = b[6 + 3 * c];
        comp_h[c] = b[7 + 3 * c] >> 4;
        comp_v[c] = b[7 + 3 * c] & 15;
        info->qsel[c] = b[8 + 3 * c];
        if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || info->qsel[c] > 3) return fail(info, SFH_JPEG_R_BAD_SOF);
      }
      sof = true;
    } else if (m == 0xDB) {
      int o = 0;
      while (o < bl) {
        const int pq = b[o] >> 4, tq = b[o] & 15;
        if (tq > 3 || pq > 1) return fail(info, SFH_JPEG_R_BAD_TABLE);
        if (pq == 1) return fail(info, SFH_JPEG_R_DQT16);
        if (o + 65 > bl) return fail(info, SFH_JPEG_R_TRUNCATED);
        for (int z = 0; z < 64; ++z) info->quant[tq][kJpegNatural[z]] = b[o + 1 + z];
        have_q[tq] = true;
        o += 65;
      }
    } else if (m == 0xC4) {
      int o = 0;
      while (o < bl) {
        const int tc = b[o] >> 4, th = b[o] & 15;
        if (tc > 1 || th > 3) return fail(info, SFH_JPEG_R_BAD_TABLE);
        if (o + 17 > bl) return fail(info, SFH_JPEG_R_TRUNCATED);
        int cnt = 0;
        for (int l = 0; l < 16; ++l) cnt += b[o + 1 + l];
        if (cnt > 256) return fail(info, SFH_JPEG_R_BAD_TABLE);
        if (o + 17 + cnt > bl) return fail(info, SFH_JPEG_R_TRUNCATED);
        if (tc == 0)
          for (int k = 0; k < cnt; ++k)
            if (b[o + 17 + k] > 15) return fail(info, SFH_JPEG_R_BAD_TABLE);
        if (!build_huff(b + o + 1, b + o + 17, cnt, tc ? &info->ac[th] : &info->dc[th])) return fail(info, SFH_JPEG_R_BAD_TABLE);
        (tc ? have_ac : have_dc)[th] = true;
        o += 17 + cnt;
      }
    } else if (m == 0xDD) {
      if (bl != 2) return fail(info, SFH_JPEG_R_MARKER);
      info->restart_interval = get_be16(b);
    } else if (m == 0xE0) {
      if (bl >= 5 && memcmp(b, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (bl >= 12 && memcmp(b, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = b[11];
      }
    } else if (m == 0xDA) {
      if (!sof) return fail(info, SFH_JPEG_R_MARKER);
      if (bl < 1) return fail(info, SFH_JPEG_R_TRUNCATED);
      const int ns = b[0];
      if (ns < 1 || ns > 4 || bl != 4 + 2 * ns) return fail(info, SFH_JPEG_R_BAD_SOS);
      if (ns != info->ncomp) return fail(info, SFH_JPEG_R_NONINTERLEAVED);
      for (int c = 0; c < ns; ++c) {
        if (b[1 + 2 * c] != comp_id[c]) return fail(info, SFH_JPEG_R_BAD_SOS);
        info->dcsel[c] = b[2 + 2 * c] >> 4;
        info->acsel[c] = b[2 + 2 * c] & 15;
        if (info->dcsel[c] > 3 || info->acsel[c] > 3) return fail(info, SFH_JPEG_R_BAD_SOS);
        if (!have_dc[info->dcsel[c]] || !have_ac[info->acsel[c]] || !have_q[info->qsel[c]]) return fail(info, SFH_JPEG_R_BAD_TABLE);
      }
      if (b[1 + 2 * ns] != 0 || b[2 + 2 * ns] != 63 || b[3 + 2 * ns] != 0) return fail(info, SFH_JPEG_R_BAD_SOS);
      i += len;
      break;
    } else if (!((m >= 0xE1 && m <= 0xEF) || m == 0xFE)) {
      return fail(info, SFH_JPEG_R_MARKER);
    }
    i += len;
  }
  // colour space by libjpeg's rule, sampling
  if (info->ncomp == 3) {
    if (adobe && adobe_transform == 0) return fail(info, SFH_JPEG_R_COLORSPACE);
    if (!jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return fail(info, SFH_JPEG_R_COLORSPACE);
    if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1 ||
        !((comp_h[0] == 2 && comp_v[0] == 2) || (comp_h[0] == 1 && comp_v[0] == 1)))
      return fail(info, SFH_JPEG_R_SAMPLING);
  } else if (comp_h[0] != 1 || comp_v[0] != 1) {
    return fail(info, SFH_JPEG_R_SAMPLING);
  }
  info->hsamp = comp_h[0];
  info->vsamp = comp_v[0];
  const int mcu = 8 * info->hsamp;
  info->mcus_x = (info->width + mcu - 1) / mcu;
  info->mcus_y = (info->height + mcu - 1) / mcu;
  info->blocks_per_mcu = info->ncomp == 1 ? 1 : info->hsamp * info->vsamp + 2;
  const int64_t total = (int64_t)info->mcus_x * info->mcus_y;
  const int64_t ri = info->restart_interval;
  const int64_t expected = ri ? (total + ri - 1) / ri : 1;
  // the scan: segments between RSTm markers, up to the first other marker or the end of the bytes
  info->scan_begin = (int32_t)i;
  int64_t nseg = 0, start = i;
  int64_t end = n;
  int after = -1;
  while (i < n) {
    if (bytes[i] != 0xFF) {
      ++i;
      continue;
    }
    int64_t j = i + 1;
    while (j < n && bytes[j] == 0xFF) ++j;
    if (j >= n) {                                       // the bytes end in 0xFF: no marker, the scan ends there
      end = i;
      break;
    }
    const int c = bytes[j];
    if (c == 0) {
      if (j != i + 1) return fail(info, SFH_JPEG_R_MARKER);   // fill bytes inside entropy-coded data
      i = j + 1;
      continue;
    }
    if (c >= 0xD0 && c <= 0xD7) {
      if (c != 0xD0 + (int)(nseg & 7)) return fail(info, SFH_JPEG_R_RESTART);
      if (nseg < seg_cap && segs) {
        segs[4 * nseg] = (int32_t)start;
        segs[4 * nseg + 1] = (int32_t)i;
        segs[4 * nseg + 2] = (int32_t)(nseg * ri);
        segs[4 * nseg + 3] = 0;
      }
      ++nseg;
      start = i = j + 1;
      continue;
    }
    end = i;
    after = c;
    break;
  }
  if (nseg < seg_cap && segs) {
    segs[4 * nseg] = (int32_t)start;
    segs[4 * nseg + 1] = (int32_t)end;
    segs[4 * nseg + 2] = (int32_t)(nseg * ri);
    segs[4 * nseg + 3] = 0;
  }
  ++nseg;
  info->scan_end = (int32_t)end;
  info->nsegments = (int32_t)nseg;
  if (after == 0xDC) return fail(info, SFH_JPEG_R_DNL);
  if (after == 0xDA) return fail(info, SFH_JPEG_R_NONINTERLEAVED);
  if (nseg != expected) return fail(info, SFH_JPEG_R_RESTART);
  return 0;
}
