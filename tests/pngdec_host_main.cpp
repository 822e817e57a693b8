// pngdec_host_main.cpp - the decode core of sfh_amd.pngdec (csrc/pngdec_core.h) run on the host, lane by lane as the kernels of
// csrc/pngdec.hip run it, so that the sanitizers see every read and write of it.  Built and run by tests/test_pngdec_host.py with
// -fsanitize=address,undefined; it links nothing of the library.
//
//   pngdec_host_main FILE...
//
// prints one line per file: "refused <reason>" or "ok <status> <accepted> <same>" - status: the PD_E_* bits of the serial leg as
// png_inflate_kernel and png_verdict_kernel form them; accepted: whether the segmented leg - count pass, acceptance rule, write
// pass, Adler-32 - accepts the file; same: its filtered stream equals the serial leg's (1 when not accepted) - and, with a status
// of 0, writes the filtered stream to FILE.filt and the unfiltered pixels in the file's channel order to FILE.px.  Every file is
// copied into a heap block of exactly its size, and every buffer has exactly the size the kernels' have, so one byte too many
// is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sports-field-homography_amd/csrc/pngdec_core.h"

static bool dump(const char* path, const char* suffix, const std::vector<uint8_t>& v) {
  const std::string name = std::string(path) + suffix;
  FILE* f = fopen(name.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), 1, v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

static uint32_t adler32(const uint8_t* p, size_t n) {
  uint32_t a = 1, b = 0;
  for (size_t i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}

// what png_adler_kernel and png_verdict_kernel add to a clean inflate
static int checked(const sfh_png_info& info, const std::vector<uint8_t>& filt) {
  int st = 0;
  if (adler32(filt.data(), filt.size()) != info.adler) st |= PD_E_ADLER;
  const size_t stride = 1 + (size_t)info.width * info.channels;
  for (size_t y = 0; y < (size_t)info.height; ++y)
    if (filt[y * stride] > 4) st |= PD_E_FILTER;
  return st;
}

static int decode_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* data = static_cast<uint8_t*>(malloc(n > 0 ? (size_t)n : 1));
  if (!data || (n > 0 && fread(data, 1, (size_t)n, f) != (size_t)n)) {
    fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  fclose(f);

  sfh_png_info info;
  if (pd_parse(data, n, &info, nullptr, 0)) {
    printf("refused %d\n", info.reason);
    free(data);
    return 0;
  }
  std::vector<int32_t> ranges((size_t)info.nidat * 2);
  pd_parse(data, n, &info, ranges.data(), info.nidat);
  const int64_t total64 = (int64_t)info.height * (1 + (int64_t)info.width * info.channels);
  if (total64 >= ((int64_t)1 << 28)) {
    printf("refused %d\n", SFH_PNG_R_SIZE);
    free(data);
    return 0;
  }
  const int32_t total = (int32_t)total64;
  PdShared* sh = new PdShared;
  PdStream base;
  base.file = data;
  base.file_bytes = (int32_t)n;
  base.ranges = ranges.data();
  base.nranges = info.nidat;
  base.r0 = 0;
  base.skip = 2;
  base.len = info.idat_bytes - 6;

  // ---- the serial leg
  std::vector<uint8_t> filt((size_t)total, 0);
  PdResult res;
  pd_inflate(base, *sh, filt.data(), total, total, res);
  int status = res.status;
  if (!status && !res.final_seen) status |= PD_E_EOF;
  if (!status && res.produced != total) status |= PD_E_SIZE;
  if (!status) status |= checked(info, filt);

  // ---- the segmented leg
  int accepted = 0, same = 1;
  if (info.nidat >= 2 && info.nidat <= SFH_PNG_DEC_MAX_SEGMENTS) {
    std::vector<PdStream> segs((size_t)info.nidat, base);
    std::vector<PdResult> recs((size_t)info.nidat);
    std::vector<int32_t> off((size_t)info.nidat);
    int32_t joined = 0;
    for (int s = 0; s < info.nidat; ++s) {
      const int32_t l0 = joined, l1 = joined + (ranges[2 * s + 1] - ranges[2 * s]);
      const int32_t lo = l0 > 2 ? l0 : 2, hi = l1 < info.idat_bytes - 4 ? l1 : info.idat_bytes - 4;
      segs[s].r0 = s;
      segs[s].skip = lo - l0;
      segs[s].len = hi - lo;
      joined = l1;
      pd_inflate(segs[s], *sh, nullptr, 0, total, recs[s]);
    }
    bool ok = true;
    int64_t sum = 0;
    for (int s = 0; s < info.nidat; ++s) {
      off[s] = (int32_t)(sum < total ? sum : total);
      ok = ok && recs[s].status == 0 && recs[s].exact == 1 && recs[s].final_seen == (s == info.nidat - 1 ? 1 : 0);
      sum += recs[s].produced;
    }
    if (ok && sum == total) {
      std::vector<uint8_t> filt2((size_t)total, 0);
      for (int s = 0; s < info.nidat; ++s) {
        int32_t cap = total - off[s];
        cap = cap < recs[s].produced ? cap : recs[s].produced;
        PdResult again;
        pd_inflate(segs[s], *sh, filt2.data() + off[s], cap, recs[s].produced, again);
      }
      if (checked(info, filt2) == 0) {
        accepted = 1;
        same = (status == 0 && filt2 == filt) ? 1 : 0;
      }
    }
  }

  // ---- the pixels, row by row with the arithmetic of the unfilter kernels
  if (!status) {
    const int C = info.channels, W = info.width, H = info.height;
    const size_t stride = 1 + (size_t)W * C;
    std::vector<uint8_t> px((size_t)H * W * C, 0);
    for (int y = 0; y < H; ++y) {
      const uint8_t* row = filt.data() + (size_t)y * stride;
      uint32_t a = 0, c = 0;
      for (int x = 0; x < W; ++x) {
        uint32_t raw = 0, b = 0;
        for (int k = 0; k < C; ++k) {
          raw |= (uint32_t)row[1 + (size_t)x * C + k] << (8 * k);
          if (y > 0) b |= (uint32_t)px[((size_t)(y - 1) * W + x) * C + k] << (8 * k);
        }
        const uint32_t cur = pd_recon(row[0], raw, a, b, c, C);
        for (int k = 0; k < C; ++k) px[((size_t)y * W + x) * C + k] = (uint8_t)(cur >> (8 * k));
        a = cur;
        c = b;
      }
    }
    if (!dump(path, ".filt", filt) || !dump(path, ".px", px)) {
      fprintf(stderr, "cannot write next to %s\n", path);
      return 2;
    }
  }
  printf("ok %d %d %d\n", status, accepted, same);
  delete sh;
  free(data);
  return 0;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (int rc = decode_file(argv[i])) return rc;
  return 0;
}
