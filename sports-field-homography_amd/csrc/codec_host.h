// codec_host.h - the host-side refusals and the staging protocol the codecs' C entry points share (pngenc.hip, jpegenc.hip;
// pngdec.hip, jpegdec.hip).  Host code of the library only: it reports through sfh_set_error.
//
// Staging.  sfh_*_dec_stage packs a batch into one pinned buffer that travels in one copy: a 64-byte head of uint32 words
// {magic, batch, the largest table of the batch, codec words ...}, the parse of every file (sfh_*_info), every file's table, then
// the files themselves, each at a 16-byte position with zeroed padding of at least 16 bytes behind it (the bit readers load
// whole dwords).  The word order of each codec's head is documented in include/sfh_amd.h.
#pragma once
#include <string.h>

#include "codec_common.h"
#include "common.h"

constexpr int kStageHeadBytes = 64;

// ---- encoders

inline int enc_batch_check(const char* who, int batch, int H, int W, int C, int64_t capacity, int64_t scratch_bytes) {
  SFH_REQUIRE(batch > 0 && batch <= 65535, "%s: batch %d (1 .. 65535)", who, batch);
  SFH_REQUIRE(capacity * batch < ((int64_t)1 << 31) && scratch_bytes < ((int64_t)1 << 32),
              "%s: %d images of %dx%dx%d: encoded batch of 2 GiB or more", who, batch, W, H, C);
  return SFH_OK;
}

inline int enc_scratch_check(const char* who, const uint8_t* scratch, int64_t scratch_bytes, int64_t need) {
  SFH_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
  SFH_REQUIRE(scratch_bytes >= need, "%s: scratch of %lld bytes, %lld needed", who, (long long)scratch_bytes, (long long)need);
  return SFH_OK;
}

// ---- decoders: sfh_*_dec_stage

// the arguments of a stage call; need: the staging bytes of the batch's geometry, negative when the geometry itself was refused.
// false: refused (*host_reason is 0: no file is to blame)
inline bool stage_begin(const char* who, const uint8_t* const* host_files, const int64_t* host_sizes, const uint8_t* host_staging,
                        int64_t staging_bytes, int64_t need, int32_t* host_reason, int32_t* host_index) {
  if (!host_files || !host_sizes || !host_staging || !host_reason || !host_index || need < 0 || staging_bytes < need ||
      ((uintptr_t)host_staging & 15)) {
    sfh_set_error("%s: null pointer, bad shape or a staging buffer that is too small or not 16-byte aligned", who);
    if (host_reason) *host_reason = 0;
    return false;
  }
  *host_reason = 0;
  *host_index = -1;
  return true;
}

// the rungs every file climbs before its parse -> 0, or the codec's reason code for a missing and for an oversize file
inline int stage_file_reason(const uint8_t* file, int64_t size, int64_t max_file_bytes, int r_truncated, int r_too_long) {
  if (!file || size < 0) return r_truncated;
  return size > max_file_bytes ? r_too_long : 0;
}

inline int64_t stage_refuse_file(const char* who, int b, int reason, int32_t* host_reason, int32_t* host_index) {
  *host_reason = reason;
  *host_index = b;
  sfh_set_error("%s: file %d refused, reason %d", who, b, reason);
  return -1;
}

// the files behind the tables, from `pos` on -> the bytes of the staging buffer used
template <class Info>
inline int64_t stage_copy_files(Info* infos, const uint8_t* const* host_files, const int64_t* host_sizes, int batch,
                                uint8_t* host_staging, int64_t pos) {
  for (int b = 0; b < batch; ++b) {
    infos[b].file_pos = (int32_t)pos;
    infos[b].file_bytes = (int32_t)host_sizes[b];
    memcpy(host_staging + pos, host_files[b], (size_t)host_sizes[b]);
    const int64_t end = round16(pos + host_sizes[b]) + 16;
    memset(host_staging + pos + host_sizes[b], 0, (size_t)(end - pos - host_sizes[b]));
    pos = end;
  }
  return pos;
}

// the head's three common words -> the head, for the codec's own words
inline uint32_t* stage_head(uint8_t* host_staging, uint32_t magic, int batch, int largest) {
  uint32_t* head = reinterpret_cast<uint32_t*>(host_staging);
  memset(head, 0, kStageHeadBytes);
  head[0] = magic;
  head[1] = (uint32_t)batch;
  head[2] = (uint32_t)largest;
  return head;
}

// ---- decoders: what a decode entry point checks before it launches.  largest_cap: the bound of head word 2; used_word: the head
// word that holds the staged bytes
inline int decode_begin(const char* who, const char* stage_fn, const uint8_t* host_staging, const uint8_t* staged,
                        int64_t staged_bytes, const uint8_t* scratch, int64_t scratch_bytes, int64_t scratch_need, uint32_t magic,
                        int batch, int64_t largest_cap, int used_word) {
  SFH_REQUIRE(host_staging && staged && scratch, "%s: null pointer (host_staging, staged, scratch)", who);
  SFH_REQUIRE((((uintptr_t)staged | (uintptr_t)scratch) & 15) == 0, "%s: staged and scratch must be 16-byte aligned", who);
  const uint32_t* head = reinterpret_cast<const uint32_t*>(host_staging);
  SFH_REQUIRE(head[0] == magic && head[1] == (uint32_t)batch && head[2] >= 1 && (int64_t)head[2] <= largest_cap,
              "%s: host_staging is not what %s left for this batch", who, stage_fn);
  SFH_REQUIRE(staged_bytes >= (int64_t)head[used_word], "%s: staged buffer of %lld bytes, %lld used", who, (long long)staged_bytes,
              (long long)head[used_word]);
  SFH_REQUIRE(scratch_bytes >= scratch_need, "%s: scratch of %lld bytes, %lld needed", who, (long long)scratch_bytes,
              (long long)scratch_need);
  return SFH_OK;
}
