// tiff_host_main.cpp - the core of sfh_amd.tiffdec / sfh_amd.tiffenc (csrc/tiff_core.h) run on the host, lane by lane as the kernels
// of csrc/tiffdec.hip and csrc/tiffenc.hip run it, so that the sanitizers see every read and write of it.  Built and run by
// tests/test_tiff_host.py with -fsanitize=address,undefined; it links nothing of the library.
//
//   tiff_host_main decode BGR FILE...
//     one line per file: "refused <reason>" or "ok <status> <width> <height> <channels> <bits> <compression> <predictor>
//     <big endian> <rows per strip> <strips>" - status: the OR of the TD_E_* bits of the strips, as tiff_verdict_kernel forms it -
//     and, with a status of 0, the pixels (little endian, the channels reversed when BGR is 1) in FILE.px.
//   tiff_host_main encode FILE H W C BITS BGR COMPRESSION PREDICTOR ROWS_PER_STRIP
//     FILE: the image's samples, little endian -> FILE.enc: per strip a little-endian uint32 byte count and the strip's bytes.
//
// Every file is copied into a heap block of exactly its size, every strip is decoded into a heap block of exactly its rows' bytes
// and encoded into one of exactly te_strip_capacity bytes, so one byte too many is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sports-field-homography_amd/csrc/tiff_core.h"

static uint8_t* slurp(const char* path, long* n) {
  FILE* f = fopen(path, "rb");
  if (!f) return nullptr;
  fseek(f, 0, SEEK_END);
  *n = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* data = static_cast<uint8_t*>(malloc(*n > 0 ? (size_t)*n : 1));
  if (data && *n > 0 && fread(data, 1, (size_t)*n, f) != (size_t)*n) {
    free(data);
    data = nullptr;
  }
  fclose(f);
  return data;
}

static bool dump(const char* path, const char* suffix, const std::vector<uint8_t>& v) {
  const std::string name = std::string(path) + suffix;
  FILE* f = fopen(name.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), 1, v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

static int decode_file(const char* path, int bgr) {
  long n = 0;
  uint8_t* data = slurp(path, &n);
  if (!data) {
    fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  sfh_tiff_info info;
  if (td_parse(data, n, &info, nullptr, 0)) {
    printf("refused %d\n", info.reason);
    free(data);
    return 0;
  }
  std::vector<int32_t> table((size_t)info.nstrips * 4);
  td_parse(data, n, &info, table.data(), info.nstrips);
  const int H = info.height, W = info.width, C = info.channels, bps = info.bits / 8;
  const int64_t rowbytes = (int64_t)W * C * bps;
  if ((int64_t)H * rowbytes >= ((int64_t)1 << 28)) {
    printf("refused %d\n", SFH_TIFF_R_SIZE);
    free(data);
    return 0;
  }
  TdShared* sh = new TdShared;
  std::vector<uint8_t> dec((size_t)(H * rowbytes), 0);
  int status = 0;
  for (int s = 0; s < info.nstrips; ++s) {
    const int32_t off = table[4 * s], cnt = table[4 * s + 1], row0 = table[4 * s + 2], rows = table[4 * s + 3];
    const int32_t total = (int32_t)(rows * rowbytes);
    uint8_t* src = static_cast<uint8_t*>(malloc(cnt > 0 ? (size_t)cnt : 1));   // exactly the strip: a read past it is a report
    uint8_t* slot = static_cast<uint8_t*>(calloc((size_t)total, 1));
    memcpy(src, data + off, (size_t)cnt);
    status |= info.compression == 5 ? td_lzw_strip(src, cnt, *sh, slot, total) : td_copy_strip(src, cnt, slot, total);
    memcpy(dec.data() + (size_t)row0 * rowbytes, slot, (size_t)total);
    free(slot);
    free(src);
  }
  if (!status) {
    // the arithmetic of tiff_unpredict_kernel, one row and channel after the other
    std::vector<uint8_t> px((size_t)(H * rowbytes), 0);
    const uint32_t mask = (1u << info.bits) - 1u;
    for (int y = 0; y < H; ++y) {
      const uint8_t* row = dec.data() + (size_t)y * rowbytes;
      uint32_t acc[3] = {0, 0, 0};
      for (int x = 0; x < W; ++x)
        for (int k = 0; k < C; ++k) {
          const uint32_t d = td_sample(row, (int64_t)x * C + k, info.bits, info.big_endian);
          acc[k] = info.predictor == 2 ? (acc[k] + d) & mask : d;
          uint8_t* p = px.data() + (((size_t)y * W + x) * C + td_out_channel(k, C, bgr)) * bps;
          p[0] = (uint8_t)acc[k];
          if (bps == 2) p[1] = (uint8_t)(acc[k] >> 8);
        }
    }
    if (!dump(path, ".px", px)) {
      fprintf(stderr, "cannot write next to %s\n", path);
      return 2;
    }
  }
  printf("ok %d %d %d %d %d %d %d %d %d %d\n", status, W, H, C, info.bits, info.compression, info.predictor, info.big_endian,
         info.rows_per_strip, info.nstrips);
  delete sh;
  free(data);
  return 0;
}

static int encode_file(const char* path, int H, int W, int C, int bits, int bgr, int compression, int predictor, int R) {
  long n = 0;
  uint8_t* data = slurp(path, &n);
  const int64_t rowbytes = (int64_t)W * C * (bits / 8);
  if (!data || n != H * rowbytes || R < 1 || R > H) {
    fprintf(stderr, "cannot read %s as %dx%dx%d of %d bits\n", path, W, H, C, bits);
    return 2;
  }
  TeGeom g;
  g.H = H;
  g.W = W;
  g.C = C;
  g.bits = bits;
  g.bgr = bgr;
  g.predictor = predictor;
  TeShared* sh = new TeShared;
  std::vector<uint8_t> out;
  for (int row0 = 0; row0 < H; row0 += R) {
    const int rows = H - row0 < R ? H - row0 : R;
    const int64_t cap = te_strip_capacity(rows * rowbytes, compression);
    uint8_t* slot = static_cast<uint8_t*>(malloc((size_t)cap));
    const int32_t m = te_encode_strip(data, g, row0, rows, compression, *sh, slot, (int32_t)cap);
    if (m > cap) {
      fprintf(stderr, "strip at row %d: %d bytes, capacity %lld\n", row0, m, (long long)cap);
      return 3;
    }
    for (int i = 0; i < 4; ++i) out.push_back((uint8_t)((uint32_t)m >> (8 * i)));
    out.insert(out.end(), slot, slot + m);
    free(slot);
  }
  delete sh;
  free(data);
  if (!dump(path, ".enc", out)) return 2;
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "decode")) {
    for (int i = 3; i < argc; ++i)
      if (int rc = decode_file(argv[i], atoi(argv[2]))) return rc;
    return 0;
  }
  if (argc == 11 && !strcmp(argv[1], "encode"))
    return encode_file(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]),
                       atoi(argv[9]), atoi(argv[10]));
  fprintf(stderr, "usage: tiff_host_main decode BGR FILE... | encode FILE H W C BITS BGR COMPRESSION PREDICTOR ROWS\n");
  return 2;
}
