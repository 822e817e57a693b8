// jpegdec_host_main.cpp - the decode core of sfh_amd.jpegdec (csrc/jpegdec_core.h) run on the host, lane by lane as the kernel
// jpeg_entropy_kernel runs it, so that the sanitizers see every read and write of it.  Built and run by
// tests/test_jpegdec_host.py with -fsanitize=address,undefined; it links nothing of the library.
//
//   jpegdec_host_main [--subseq BITS] [--lanes N] FILE...
//
// prints one line per file: "ok <status> <checksum> <rounds>" (status: OR of the segments' JD_E_* bits; checksum: FNV-1a over
// the int16 coefficients of the image, little endian, DC values integrated; rounds: the largest round count) or
// "refused <reason>".  Every file is copied into a heap block of exactly its size rounded up to 4 bytes - the core's stated
// read contract - and every scratch array has exactly the size the kernel's has, so one byte too many is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sports-field-homography_amd/csrc/jpegdec_core.h"

static int decode_file(const char* path, int subseq_bits, int lanes) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  const size_t padded = ((size_t)n + 3) & ~(size_t)3;
  uint8_t* data = static_cast<uint8_t*>(malloc(padded ? padded : 1));   // malloc's blocks are 16-byte aligned
  if (!data || (n > 0 && fread(data, 1, (size_t)n, f) != (size_t)n)) {
    fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  fclose(f);
  memset(data + n, 0, padded - (size_t)n);

  sfh_jpeg_info* info = new sfh_jpeg_info;
  if (jd_parse(data, n, info, nullptr, 0)) {
    printf("refused %d\n", info->reason);
    delete info;
    free(data);
    return 0;
  }
  std::vector<int32_t> segs((size_t)info->nsegments * 4);
  if (jd_parse(data, n, info, segs.data(), info->nsegments)) {
    printf("refused %d\n", info->reason);
    delete info;
    free(data);
    return 0;
  }
  const int bpm = info->blocks_per_mcu;
  const int64_t total_mcus = (int64_t)info->mcus_x * info->mcus_y;
  std::vector<int16_t> coef((size_t)(total_mcus * bpm * 64), 0);
  uint8_t blk_dc[8], blk_ac[8], blk_comp[8];
  for (int t = 0; t < 8; ++t) {
    const int c = info->ncomp == 1 ? 0 : (t < bpm - 2 ? 0 : t - (bpm - 3));
    const int cc = c < 3 ? c : 0;
    blk_comp[t] = (uint8_t)cc;
    blk_dc[t] = (uint8_t)info->dcsel[cc];
    blk_ac[t] = (uint8_t)info->acsel[cc];
  }
  int status = 0, most = 0;
  for (int s = 0; s < info->nsegments; ++s) {
    const int64_t m0 = segs[4 * s + 2];
    int64_t nm = info->restart_interval ? info->restart_interval : total_mcus;
    if (m0 + nm > total_mcus) nm = total_mcus - m0;
    if (nm < 0) nm = 0;
    const int32_t nblocks = (int32_t)(nm * bpm);
    JdCtx c;
    c.data = data;
    c.lo = segs[4 * s];
    c.hi = segs[4 * s + 1];
    c.nbits = (c.hi - c.lo) * 8;
    c.bpm = bpm;
    c.dc = info->dc;
    c.ac = info->ac;
    c.blk_dc = blk_dc;
    c.blk_ac = blk_ac;
    const int32_t nsub = jd_nsub(c.hi - c.lo, subseq_bits);
    std::vector<JdExit> exa((size_t)nsub), exb((size_t)nsub);
    std::vector<JdState> lastin((size_t)nsub);
    std::vector<int32_t> base((size_t)nsub);
    JdExit* ex[2] = {exa.data(), exb.data()};
    int rounds = 0, cur = 0;
    for (int round = 0; round < nsub; ++round) {
      cur = round & 1;
      bool any = false;
      for (int t = 0; t < lanes; ++t) any |= jd_round_lane(c, subseq_bits, nsub, round, t, lanes, ex[cur ^ 1], ex[cur], lastin.data());
      ++rounds;
      if (!any) break;
    }
    const JdExit* exits = ex[cur];
    int32_t carry = 0;
    for (int32_t i = 0; i < nsub; ++i) {
      base[(size_t)i] = carry;
      carry += exits[i].nblk;
    }
    int16_t* cf = coef.data() + m0 * bpm * 64;
    int err = 0;
    for (int t = 0; t < lanes; ++t) err |= jd_final_lane(c, subseq_bits, nsub, t, lanes, exits, base.data(), cf, nblocks);
    if (carry < nblocks) err |= JD_E_BLOCKS;
    int run[3] = {0, 0, 0};
    for (int64_t u = 0; u < nm; ++u)
      for (int j = 0; j < bpm; ++j) {
        int16_t* p = cf + (u * bpm + j) * 64;
        run[blk_comp[j]] += *p;
        *p = (int16_t)run[blk_comp[j]];
      }
    status |= err;
    most = rounds > most ? rounds : most;
  }
  uint64_t h = 0xcbf29ce484222325ull;
  for (int16_t v : coef) {
    const uint16_t u = (uint16_t)v;
    h = (h ^ (u & 255u)) * 0x100000001b3ull;
    h = (h ^ (u >> 8)) * 0x100000001b3ull;
  }
  printf("ok %d %016llx %d\n", status, (unsigned long long)h, most);
  delete info;
  free(data);
  return 0;
}

int main(int argc, char** argv) {
  int subseq_bits = 1024, lanes = 256;
  int i = 1;
  while (i + 1 < argc && argv[i][0] == '-') {
    if (!strcmp(argv[i], "--subseq")) subseq_bits = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--lanes")) lanes = atoi(argv[i + 1]);
    else break;
    i += 2;
  }
  if (subseq_bits < 32 || (subseq_bits & 31) || lanes < 1) {
    fprintf(stderr, "bad --subseq / --lanes\n");
    return 2;
  }
  for (; i < argc; ++i)
    if (int rc = decode_file(argv[i], subseq_bits, lanes)) return rc;
  return 0;
}
