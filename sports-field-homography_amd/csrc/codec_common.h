// codec_common.h - the small integer and byte helpers the four image codecs (pngenc.hip, jpegenc.hip, pngdec.hip, jpegdec.hip and
// the *_core.h decode cores) share, stated once.  Plain C++: the stand-alone host programs of tests/ compile it with clang++
// under the sanitizers, so nothing here includes a HIP header; SFH_HD marks what the device runs too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SFH_HD __host__ __device__ inline
#else
#define SFH_HD inline
#endif

template <class T>
constexpr T round16(T v) {
  return (v + 15) & ~(T)15;
}

// libjpeg's DESCALE: x / 2^n rounded to nearest (jfdctint.c in jpegenc.hip, jidctint.c in jpegdec.hip)
SFH_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// JPEG: zig-zag position -> natural (row-major) index
constexpr uint8_t kJpegNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// big-endian integers as PNG chunks and JPEG segments hold them
SFH_HD int get_be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }
SFH_HD uint32_t get_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
SFH_HD void put_be32(uint8_t* o, uint32_t v) {
  o[0] = (uint8_t)(v >> 24);
  o[1] = (uint8_t)(v >> 16);
  o[2] = (uint8_t)(v >> 8);
  o[3] = (uint8_t)v;
}

// CRC-32 (PNG chunks) on the host, by table
struct Crc32Table {
  uint32_t t[256];
  Crc32Table() {
    for (uint32_t n = 0; n < 256; ++n) {
      uint32_t c = n;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
      t[n] = c;
    }
  }
};

inline uint32_t host_crc32(const uint8_t* p, int64_t n) {
  static const Crc32Table tab;
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 255u] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}
