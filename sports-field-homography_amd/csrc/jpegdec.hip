// jpegdec.hip - baseline JFIF files to uint8 device frames (sfh_amd.jpegdec; the rule is libjpeg's, restated in
// tests/jpegdec_ref.py, which tests/test_jpegdec_host.py holds to PIL's bytes).  The decode core - parse, bit reader, code lookup,
// state step, the per-lane phases and their bounds rules - is csrc/jpegdec_core.h, shared with the stand-alone host program
// tests/jpegdec_host_main.cpp.  Integers only.
//
// * Host: sfh_jpeg_parse walks the markers; sfh_jpeg_dec_stage packs the parses, segment tables and files of a batch into one
//   staging buffer for one copy.
// * jpeg_entropy_kernel, one workgroup per (image, segment).  A segment (the bytes between two RSTm markers; the whole scan
//   without DRI) is a serial bit stream: it is cut into subsequences of subseq_bits bits, thread t owns t, t + 256, ...  Round 0
//   decodes subsequence 0 from the true start and every other one from a guessed state; round r decodes subsequence i from
//   the exit i - 1 had after round r - 1 (two exit buffers, read one, write the other: the same rounds every run) and skips the
//   decode when that entry state is the one it last decoded from.  After round r subsequences 0 .. r are right by induction,
//   whether or not the codes synchronise; the loop ends when a workgroup-wide OR says nothing changed, after nsub rounds at the
//   latest.  A scan of the block counts gives every subsequence its first block; a last pass decodes once more and scatters the
//   coefficients (int16, natural order, MCU order; cleared by the memset before the launch); a scan per component over the
//   segment turns the DC differences into values.  Record: {rounds, status}.
// * jpeg_status_kernel, one workgroup per image: OR of the statuses, max of the rounds.
// * jpeg_idct_kernel, a thread per block: dequantisation, jidctint's two passes -> planes in scratch (gray: the frame).
// * jpeg_color_kernel: 4:2:0, a thread per chroma sample = 2 x 2 pixels (triangle upsampling, then the 16-bit fixed-point
//   YCbCr -> RGB); 4:4:4, a thread per pixel.
// Scratch: [coefficients | records] (one memset), exits A, exits B, last entry states, first blocks, planes.  LDS: the file's
// sfh_jpeg_info (7920 bytes) and a few words.  No global atomics; no workgroup waits for another.
#include "common.h"
#include "block_scan.h"
#include "codec_host.h"
#include "jpegdec_core.h"

namespace {

using namespace blockscan;
constexpr int kThreads = kScanThreads;
constexpr uint32_t kMagic = 0x4a444543u;   // "JDEC"

struct DecGeom {
  int mcus_x16, mcus_y16, mcus_x8, mcus_y8;
  int64_t max_mcus;      // of an image, whichever sampling
  int64_t max_blocks;    // coefficient blocks of an image at most
  int64_t subcap;        // subsequence slots of an image
  int64_t plane;         // bytes of one plane
  // scratch offsets
  int64_t coef, rec, clear_bytes, exa, exb, lastin, base, planes, total;
  int64_t staging;
};

bool dec_geom(int batch, int H, int W, int C, int64_t max_file_bytes, int subseq_bits, DecGeom* g) {
  if (batch < 1 || batch > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return false;
  if (max_file_bytes < 4 || max_file_bytes >= ((int64_t)1 << 28) - 8192) return false;      // bit positions are int32
  if (subseq_bits < 32 || subseq_bits > 65536 || (subseq_bits & 31)) return false;
  g->mcus_x16 = sfh_cdiv(W, 16);
  g->mcus_y16 = sfh_cdiv(H, 16);
  g->mcus_x8 = sfh_cdiv(W, 8);
  g->mcus_y8 = sfh_cdiv(H, 8);
  g->max_mcus = (int64_t)g->mcus_x8 * g->mcus_y8;
  const int64_t b420 = (int64_t)g->mcus_x16 * g->mcus_y16 * 6, b444 = g->max_mcus * 3;
  g->max_blocks = C == 1 ? g->max_mcus : (b420 > b444 ? b420 : b444);
  g->subcap = (max_file_bytes * 8 + subseq_bits - 1) / subseq_bits + g->max_mcus;
  g->plane = C == 1 ? 0 : (int64_t)g->mcus_x16 * 16 * g->mcus_y16 * 16;
  int64_t o = 0;
  g->coef = o;
  o += round16((int64_t)batch * g->max_blocks * 128);
  g->rec = o;
  o += round16((int64_t)batch * g->max_mcus * 8);
  g->clear_bytes = o;
  g->exa = o;
  o += round16((int64_t)batch * g->subcap * 12);
  g->exb = o;
  o += round16((int64_t)batch * g->subcap * 12);
  g->lastin = o;
  o += round16((int64_t)batch * g->subcap * 8);
  g->base = o;
  o += round16((int64_t)batch * g->subcap * 4);
  g->planes = o;
  o += round16((int64_t)batch * 3 * g->plane);
  g->total = o;
  g->staging = kStageHeadBytes + (int64_t)batch * ((int64_t)sizeof(sfh_jpeg_info) + 16 * g->max_mcus + round16(max_file_bytes) + 16);
  return g->total < ((int64_t)1 << 31) * 2 && g->staging < ((int64_t)1 << 31);
}

struct DecArgs {
  int H, W, C, subseq_bits;
  int64_t max_blocks, max_mcus, subcap, plane;
  int64_t coef, rec, exa, exb, lastin, base, planes;
};

DecArgs dec_args(const DecGeom& g, int H, int W, int C, int subseq_bits) {
  DecArgs a;
  a.H = H;
  a.W = W;
  a.C = C;
  a.subseq_bits = subseq_bits;
  a.max_blocks = g.max_blocks;
  a.max_mcus = g.max_mcus;
  a.subcap = g.subcap;
  a.plane = g.plane;
  a.coef = g.coef;
  a.rec = g.rec;
  a.exa = g.exa;
  a.exb = g.exb;
  a.lastin = g.lastin;
  a.base = g.base;
  a.planes = g.planes;
  return a;
}

__device__ __forceinline__ const sfh_jpeg_info* staged_info(const uint8_t* staged, int b) {
  return reinterpret_cast<const sfh_jpeg_info*>(staged + kStageHeadBytes) + b;
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(const uint8_t* __restrict__ staged, DecArgs a,
                                                                uint8_t* __restrict__ scratch) {
  __shared__ sfh_jpeg_info info;
  __shared__ uint8_t blk_dc[8], blk_ac[8], blk_comp[8];
  __shared__ int tmp[4];
  __shared__ int flag;
  const int t = threadIdx.x;
  const int seg = blockIdx.x, b = blockIdx.y;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(staged_info(staged, b));
    uint32_t* dst = reinterpret_cast<uint32_t*>(&info);
    for (int i = t; i < (int)(sizeof(sfh_jpeg_info) / 4); i += kThreads) dst[i] = src[i];
  }
  __syncthreads();
  if (seg >= info.nsegments) return;                    // uniform over the workgroup
  const int bpm = info.blocks_per_mcu;
  if (t < 8) {
    const int c = info.ncomp == 1 ? 0 : (t < bpm - 2 ? 0 : t - (bpm - 3));
    const int cc = c < 3 ? c : 0;
    blk_comp[t] = (uint8_t)cc;
    blk_dc[t] = (uint8_t)info.dcsel[cc];
    blk_ac[t] = (uint8_t)info.acsel[cc];
  }
  __syncthreads();
  const int32_t* sq = reinterpret_cast<const int32_t*>(staged + info.seg_pos) + 4 * (int64_t)seg;
  const int64_t total_mcus = (int64_t)info.mcus_x * info.mcus_y;
  const int64_t m0 = sq[2];
  int64_t nm = info.restart_interval ? info.restart_interval : total_mcus;
  if (m0 + nm > total_mcus) nm = total_mcus - m0;
  if (nm < 0) nm = 0;
  const int32_t nblocks = (int32_t)(nm * bpm);
  JdCtx c;
  c.data = staged;
  c.lo = info.file_pos + sq[0];
  c.hi = info.file_pos + sq[1];
  if (c.hi > info.file_pos + info.file_bytes) c.hi = info.file_pos + info.file_bytes;
  if (c.hi < c.lo) c.hi = c.lo;
  c.nbits = (c.hi - c.lo) * 8;
  c.bpm = bpm;
  c.dc = info.dc;
  c.ac = info.ac;
  c.blk_dc = blk_dc;
  c.blk_ac = blk_ac;
  const int S = a.subseq_bits;
  int32_t nsub = jd_nsub(c.hi - c.lo, S);
  const int64_t slot0 = (int64_t)b * a.subcap + sq[3];
  if (sq[3] < 0 || sq[3] + (int64_t)nsub > a.subcap) nsub = 0;   // cannot happen with a staging buffer of sfh_jpeg_dec_stage
  JdExit* ex[2] = {reinterpret_cast<JdExit*>(scratch + a.exa) + slot0, reinterpret_cast<JdExit*>(scratch + a.exb) + slot0};
  JdState* lastin = reinterpret_cast<JdState*>(scratch + a.lastin) + slot0;
  int32_t* base = reinterpret_cast<int32_t*>(scratch + a.base) + slot0;
  int16_t* coef = reinterpret_cast<int16_t*>(scratch + a.coef) + ((int64_t)b * a.max_blocks + m0 * bpm) * 64;
  int32_t* rec = reinterpret_cast<int32_t*>(scratch + a.rec) + ((int64_t)b * a.max_mcus + seg) * 2;
  if (m0 * bpm + nblocks > a.max_blocks || nsub == 0) {
    if (t == 0) {
      rec[0] = 0;
      rec[1] = JD_E_BLOCKS;
    }
    return;
  }

  // ---- 1. the fixed-point iteration over the exit states
  int rounds = 0;
  int cur = 0;
  for (int round = 0; round < nsub; ++round) {
    cur = round & 1;
    if (t == 0) flag = 0;
    __syncthreads();
    const bool changed = jd_round_lane(c, S, nsub, round, t, kThreads, ex[cur ^ 1], ex[cur], lastin);
    if (changed) atomicOr(&flag, 1);
    __syncthreads();
    const int any = flag;
    ++rounds;
    __syncthreads();
    if (!any) break;
  }
  const JdExit* exits = ex[cur];

  // ---- 2. every subsequence's first block
  int carry = 0;
  for (int32_t i0 = 0; i0 < nsub; i0 += kThreads) {
    const int32_t i = i0 + t;
    const int n = i < nsub ? exits[i].nblk : 0;
    int tot;
    const int off = block_scan_excl<OP_SUM, false>(n, 0, tmp, tot);
    if (i < nsub) base[i] = carry + off;
    carry += tot;
    __syncthreads();
  }

  // ---- 3. the coefficients
  int err = jd_final_lane(c, S, nsub, t, kThreads, exits, base, coef, nblocks);
  if (t == 0 && carry < nblocks) err |= JD_E_BLOCKS;
  if (t == 0) flag = 0;
  __syncthreads();
  if (err) atomicOr(&flag, err);
  __syncthreads();
  if (t == 0) {
    rec[0] = rounds;
    rec[1] = flag;
  }

  // ---- 4. DC differences -> values: a contiguous run of MCUs per thread, a scan per component
  const int per = (int)((nm + kThreads - 1) / kThreads);
  const int64_t u0 = (int64_t)t * per < nm ? (int64_t)t * per : nm;
  const int64_t u1 = u0 + per < nm ? u0 + per : nm;
  int sum[3] = {0, 0, 0};
  for (int64_t u = u0; u < u1; ++u)
    for (int j = 0; j < bpm; ++j) {
      const int v = coef[(u * bpm + j) * 64];
      const int cc = blk_comp[j];
      sum[0] += cc == 0 ? v : 0;
      sum[1] += cc == 1 ? v : 0;
      sum[2] += cc == 2 ? v : 0;
    }
  int run[3];
  for (int k = 0; k < 3; ++k) {
    int tot;
    run[k] = block_scan_excl<OP_SUM, false>(sum[k], 0, tmp, tot);
    __syncthreads();
  }
  for (int64_t u = u0; u < u1; ++u)
    for (int j = 0; j < bpm; ++j) {
      int16_t* p = coef + (u * bpm + j) * 64;
      const int cc = blk_comp[j];
      const int v = (cc == 0 ? run[0] : (cc == 1 ? run[1] : run[2])) + *p;
      run[0] = cc == 0 ? v : run[0];
      run[1] = cc == 1 ? v : run[1];
      run[2] = cc == 2 ? v : run[2];
      *p = (int16_t)v;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_status_kernel(const uint8_t* __restrict__ staged, DecArgs a,
                                                               const uint8_t* __restrict__ scratch, int32_t* __restrict__ status,
                                                               int32_t* __restrict__ rounds) {
  __shared__ int tmp[4];
  const int t = threadIdx.x, b = blockIdx.x;
  const int nseg = staged_info(staged, b)->nsegments;
  const int32_t* rec = reinterpret_cast<const int32_t*>(scratch + a.rec) + (int64_t)b * a.max_mcus * 2;
  int st = 0, rd = 0;
  for (int s = t; s < nseg && s < a.max_mcus; s += kThreads) {
    rd = rec[2 * s] > rd ? rec[2 * s] : rd;
    st |= rec[2 * s + 1];
  }
  int rmax, any;
  block_scan_excl<OP_MAX, false>(rd, 0, tmp, rmax);
  __syncthreads();
  block_scan_excl<OP_MAX, false>(st != 0 ? 1 : 0, 0, tmp, any);
  // the OR itself: every status bit is below 16, so the max over bit k alone gives bit k
  int bits = 0;
  for (int k = 0; k < 4; ++k) {
    int m;
    __syncthreads();
    block_scan_excl<OP_MAX, false>((st >> k) & 1, 0, tmp, m);
    bits |= m << k;
  }
  if (t == 0) {
    status[b] = any ? bits : 0;
    rounds[b] = rmax;
  }
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one pass of jidctint.c (CONST_BITS 13, PASS1_BITS 2) over 8 values; N: the descale (11: the column pass, 18: the row pass)
template <int N>
__device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  int z2 = d2, z3 = d6;
  int z1 = (z2 + z3) * 4433;
  const int e2 = z1 + z3 * -15137, e3 = z1 + z2 * 6270;
  const int e0 = (d0 + d4) * 8192, e1 = (d0 - d4) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int o0 = d7, o1 = d5, o2 = d3, o3 = d1;
  z1 = o0 + o3;
  z2 = o1 + o2;
  z3 = o0 + o2;
  int z4 = o1 + o3;
  const int z5 = (z3 + z4) * 9633;
  o0 *= 2446;
  o1 *= 16819;
  o2 *= 25172;
  o3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  d0 = descale(t10 + o3, N);
  d7 = descale(t10 - o3, N);
  d1 = descale(t11 + o2, N);
  d6 = descale(t11 - o2, N);
  d2 = descale(t12 + o1, N);
  d5 = descale(t12 - o1, N);
  d3 = descale(t13 + o0, N);
  d4 = descale(t13 - o0, N);
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const uint8_t* __restrict__ staged, DecArgs a,
                                                             uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
                                                             const int32_t* __restrict__ status) {
  __shared__ int quant[3][64];
  __shared__ int geom[4];
  const int t = threadIdx.x, b = blockIdx.y;
  {
    const sfh_jpeg_info* info = staged_info(staged, b);
    if (t < 192) {
      const int c = t >> 6;
      quant[c][t & 63] = c < info->ncomp ? info->quant[info->qsel[c] & 3][t & 63] : 0;
    }
    if (t == 0) {
      geom[0] = info->mcus_x;
      geom[1] = info->mcus_y;
      geom[2] = info->blocks_per_mcu;
      geom[3] = info->hsamp;
    }
  }
  __syncthreads();
  const int mcus_x = geom[0], bpm = geom[2], hs = geom[3];
  const int64_t nblocks = (int64_t)mcus_x * geom[1] * bpm;
  const int64_t g = (int64_t)blockIdx.x * kThreads + t;
  if (g >= nblocks || g >= a.max_blocks) return;
  const int64_t mcu = g / bpm;
  const int j = (int)(g - mcu * bpm);
  const int mx = (int)(mcu % mcus_x), my = (int)(mcu / mcus_x);
  int comp, bx, by;
  if (a.C == 1 || hs == 1) {
    comp = j;
    bx = mx;
    by = my;
  } else if (j < 4) {
    comp = 0;
    bx = 2 * mx + (j & 1);
    by = 2 * my + (j >> 1);
  } else {
    comp = j - 3;
    bx = mx;
    by = my;
  }
  int d[64];
  const bool bad = status[b] != 0;
  {
    const uint32_t* cf = reinterpret_cast<const uint32_t*>(reinterpret_cast<const int16_t*>(scratch + a.coef) +
                                                           ((int64_t)b * a.max_blocks + g) * 64);
    const int* q = quant[comp];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const uint32_t w = cf[i];
      d[2 * i] = (int)(int16_t)(w & 0xFFFFu) * q[2 * i];
      d[2 * i + 1] = (int)(int16_t)(w >> 16) * q[2 * i + 1];
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col)
    idct8<11>(d[col], d[8 + col], d[16 + col], d[24 + col], d[32 + col], d[40 + col], d[48 + col], d[56 + col]);
#pragma unroll
  for (int r = 0; r < 8; ++r)
    idct8<18>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
  if (a.C == 1) {                                       // gray: the frame itself, cropped
    uint8_t* dst = out + (int64_t)b * a.H * a.W;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = by * 8 + r;
      if (y >= a.H) break;
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (bx * 8 + x < a.W) dst[(int64_t)y * a.W + bx * 8 + x] = bad ? 0 : (uint8_t)clamp255(d[r * 8 + x] + 128);
    }
    return;
  }
  const int pw = mcus_x * 8 * (comp == 0 ? hs : 1);     // the plane's row stride: a multiple of 8, so the stores are aligned
  if ((int64_t)(by * 8 + 8) * pw > a.plane) return;
  uint8_t* dst = scratch + a.planes + ((int64_t)b * 3 + comp) * a.plane + (int64_t)by * 8 * pw + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (uint32_t)clamp255(d[r * 8 + x] + 128) << (8 * x);
      hi |= (uint32_t)clamp255(d[r * 8 + 4 + x] + 128) << (8 * x);
    }
    *reinterpret_cast<uint2*>(dst + (int64_t)r * pw) = make_uint2(lo, hi);
  }
}

// libjpeg's ycc_rgb_convert: 16-bit fixed point
__device__ __forceinline__ void put_rgb(uint8_t* p, int y, int cb, int cr, int bgr) {
  const int r = clamp255(y + ((91881 * (cr - 128) + 32768) >> 16));
  const int bl = clamp255(y + ((116130 * (cb - 128) + 32768) >> 16));
  const int g = clamp255(y + ((-22554 * (cb - 128) - 46802 * (cr - 128) + 32768) >> 16));
  p[0] = (uint8_t)(bgr ? bl : r);
  p[1] = (uint8_t)g;
  p[2] = (uint8_t)(bgr ? r : bl);
}

__global__ __launch_bounds__(kThreads) void jpeg_color_kernel(const uint8_t* __restrict__ staged, DecArgs a, int bgr,
                                                              const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
                                                              const int32_t* __restrict__ status) {
  const int b = blockIdx.z;
  const sfh_jpeg_info* info = staged_info(staged, b);
  const int hs = info->hsamp, mcus_x = info->mcus_x;
  const bool bad = status[b] != 0;
  const int H = a.H, W = a.W;
  const uint8_t* py = scratch + a.planes + (int64_t)b * 3 * a.plane;
  const uint8_t* pcb = py + a.plane;
  const uint8_t* pcr = pcb + a.plane;
  uint8_t* dst = out + (int64_t)b * H * W * 3;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (hs == 1) {
    if (x >= W || y >= H) return;
    const int pw = mcus_x * 8;
    uint8_t* p = dst + ((int64_t)y * W + x) * 3;
    if (bad) {
      p[0] = p[1] = p[2] = 0;
      return;
    }
    const int64_t o = (int64_t)y * pw + x;
    put_rgb(p, py[o], pcb[o], pcr[o], bgr);
    return;
  }
  const int cw = (W + 1) >> 1, ch = (H + 1) >> 1;
  if (x >= cw || y >= ch) return;
  const int yw = mcus_x * 16, cwp = mcus_x * 8;
  const int xl = x > 0 ? x - 1 : 0, xr = x + 1 < cw ? x + 1 : cw - 1;
  const int yu = y > 0 ? y - 1 : 0, yd = y + 1 < ch ? y + 1 : ch - 1;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int oy = 2 * y + dy;
    if (oy >= H) break;
    const int yf = dy ? yd : yu;                        // the far row; the near row is y
    const uint8_t* nb = pcb + (int64_t)y * cwp;
    const uint8_t* fb = pcb + (int64_t)yf * cwp;
    const uint8_t* nr = pcr + (int64_t)y * cwp;
    const uint8_t* fr = pcr + (int64_t)yf * cwp;
    const int bl = 3 * nb[xl] + fb[xl], bt = 3 * nb[x] + fb[x], bn = 3 * nb[xr] + fb[xr];
    const int rl = 3 * nr[xl] + fr[xl], rt = 3 * nr[x] + fr[x], rn = 3 * nr[xr] + fr[xr];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int ox = 2 * x + dx;
      if (ox >= W) break;
      uint8_t* p = dst + ((int64_t)oy * W + ox) * 3;
      if (bad) {
        p[0] = p[1] = p[2] = 0;
        continue;
      }
      const int cb = dx ? (3 * bt + bn + 7) >> 4 : (3 * bt + bl + 8) >> 4;
      const int cr = dx ? (3 * rt + rn + 7) >> 4 : (3 * rt + rl + 8) >> 4;
      put_rgb(p, py[(int64_t)oy * yw + ox], cb, cr, bgr);
    }
  }
}

}  // namespace

extern "C" int sfh_jpeg_parse(const uint8_t* host_bytes, int64_t n, sfh_jpeg_info* host_info, int32_t* host_segs, int64_t seg_cap) {
  SFH_REQUIRE(host_bytes && host_info && n >= 0 && seg_cap >= 0 && (host_segs || seg_cap == 0),
              "jpeg_parse: null pointer or negative size");
  const int rc = jd_parse(host_bytes, n, host_info, host_segs, seg_cap);
  if (rc) sfh_set_error("jpeg_parse: refused, reason %d", host_info->reason);
  return rc;
}

extern "C" int64_t sfh_jpeg_dec_staging_bytes(int batch, int H, int W, int C, int64_t max_file_bytes) {
  DecGeom g;
  if (!dec_geom(batch, H, W, C, max_file_bytes, 1024, &g)) {
    sfh_set_error("jpeg_dec_staging_bytes: batch %d image %dx%dx%d files of %lld bytes", batch, W, H, C, (long long)max_file_bytes);
    return -1;
  }
  return g.staging;
}

extern "C" int64_t sfh_jpeg_dec_scratch_bytes(int batch, int H, int W, int C, int64_t max_file_bytes, int subseq_bits) {
  DecGeom g;
  if (!dec_geom(batch, H, W, C, max_file_bytes, subseq_bits, &g)) {
    sfh_set_error("jpeg_dec_scratch_bytes: batch %d image %dx%dx%d files of %lld bytes, subsequences of %d bits", batch, W, H, C,
                  (long long)max_file_bytes, subseq_bits);
    return -1;
  }
  return g.total;
}

extern "C" int64_t sfh_jpeg_dec_stage(const uint8_t* const* host_files, const int64_t* host_sizes, int batch, int H, int W, int C,
                                      int64_t max_file_bytes, int subseq_bits, uint8_t* host_staging, int64_t staging_bytes,
                                      int32_t* host_reason, int32_t* host_index) {
  DecGeom g;
  const int64_t need = dec_geom(batch, H, W, C, max_file_bytes, subseq_bits, &g) ? g.staging : -1;
  if (!stage_begin("jpeg_dec_stage", host_files, host_sizes, host_staging, staging_bytes, need, host_reason, host_index)) return -1;
  sfh_jpeg_info* infos = reinterpret_cast<sfh_jpeg_info*>(host_staging + kStageHeadBytes);
  int64_t pos = kStageHeadBytes + (int64_t)batch * (int64_t)sizeof(sfh_jpeg_info);
  int max_seg = 0, hsamp = 0;
  for (int b = 0; b < batch; ++b) {
    sfh_jpeg_info* info = infos + b;
    int32_t* segs = reinterpret_cast<int32_t*>(host_staging + pos);
    int reason = stage_file_reason(host_files[b], host_sizes[b], max_file_bytes, SFH_JPEG_R_TRUNCATED, SFH_JPEG_R_TOO_LONG);
    if (reason == SFH_JPEG_R_OK) {
      if (jd_parse(host_files[b], host_sizes[b], info, segs, g.max_mcus)) reason = info->reason;
      else if (info->width != W || info->height != H || info->ncomp != C || info->nsegments > g.max_mcus ||
               (b > 0 && info->hsamp != hsamp))
        reason = SFH_JPEG_R_SIZE;
    }
    if (reason != SFH_JPEG_R_OK) return stage_refuse_file("jpeg_dec_stage", b, reason, host_reason, host_index);
    hsamp = info->hsamp;
    int64_t nsub = 0;
    for (int s = 0; s < info->nsegments; ++s) {
      segs[4 * s + 3] = (int32_t)nsub;
      nsub += jd_nsub(segs[4 * s + 1] - segs[4 * s], subseq_bits);
    }
    info->nsub = (int32_t)nsub;                          // <= subcap: the segments' bytes are disjoint bytes of the file
    info->seg_pos = (int32_t)pos;
    pos += 16 * (int64_t)info->nsegments;
    max_seg = info->nsegments > max_seg ? info->nsegments : max_seg;
  }
  pos = stage_copy_files(infos, host_files, host_sizes, batch, host_staging, pos);
  uint32_t* head = stage_head(host_staging, kMagic, batch, max_seg);
  head[3] = (uint32_t)subseq_bits;
  head[4] = (uint32_t)pos;
  head[5] = (uint32_t)hsamp;
  return pos;
}

extern "C" int sfh_jpeg_entropy_decode(const uint8_t* host_staging, const uint8_t* staged, int64_t staged_bytes, int batch, int H,
                                       int W, int C, int64_t max_file_bytes, int subseq_bits, uint8_t* scratch,
                                       int64_t scratch_bytes, void* stream) {
  DecGeom g;
  SFH_REQUIRE(dec_geom(batch, H, W, C, max_file_bytes, subseq_bits, &g), "jpeg_entropy_decode: batch %d image %dx%dx%d", batch, W, H, C);
  if (int rc = decode_begin("jpeg_entropy_decode", "sfh_jpeg_dec_stage", host_staging, staged, staged_bytes, scratch, scratch_bytes,
                            g.total, kMagic, batch, g.max_mcus, 4))
    return rc;
  const uint32_t* head = reinterpret_cast<const uint32_t*>(host_staging);
  SFH_REQUIRE(head[3] == (uint32_t)subseq_bits, "jpeg_entropy_decode: host_staging was staged for subsequences of %u bits, not %d",
              head[3], subseq_bits);
  const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)g.clear_bytes, (hipStream_t)stream);
  if (e != hipSuccess) {
    sfh_set_error("jpeg_entropy_decode: hipMemsetAsync: %s", hipGetErrorString(e));
    return SFH_E_LAUNCH;
  }
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(head[2], (unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, staged,
                     dec_args(g, H, W, C, subseq_bits), scratch);
  return sfh_check_launch("jpeg_entropy_kernel");
}

extern "C" int sfh_jpeg_decode_pixels(const uint8_t* staged, int batch, int H, int W, int C, int hsamp, int bgr,
                                      int64_t max_file_bytes, int subseq_bits, uint8_t* scratch, int64_t scratch_bytes, uint8_t* out,
                                      int32_t* status, int32_t* rounds, void* stream) {
  DecGeom g;
  SFH_REQUIRE(dec_geom(batch, H, W, C, max_file_bytes, subseq_bits, &g), "jpeg_decode_pixels: batch %d image %dx%dx%d", batch, W, H, C);
  SFH_REQUIRE(staged && scratch && out && status && rounds, "jpeg_decode_pixels: null pointer");
  SFH_REQUIRE((((uintptr_t)staged | (uintptr_t)scratch) & 15) == 0, "jpeg_decode_pixels: staged and scratch must be 16-byte aligned");
  SFH_REQUIRE(scratch_bytes >= g.total, "jpeg_decode_pixels: scratch of %lld bytes, %lld needed", (long long)scratch_bytes,
              (long long)g.total);
  SFH_REQUIRE(hsamp == 1 || (hsamp == 2 && C == 3), "jpeg_decode_pixels: sampling %d (1, or 2 with 3 channels)", hsamp);
  const DecArgs a = dec_args(g, H, W, C, subseq_bits);
  hipLaunchKernelGGL(jpeg_status_kernel, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, staged, a, scratch, status,
                     rounds);
  if (int rc = sfh_check_launch("jpeg_status_kernel")) return rc;
  const int64_t blocks = C == 1 ? g.max_mcus : (hsamp == 2 ? (int64_t)g.mcus_x16 * g.mcus_y16 * 6 : g.max_mcus * 3);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + kThreads - 1) / kThreads), (unsigned)batch), dim3(kThreads), 0,
                     (hipStream_t)stream, staged, a, scratch, out, status);
  if (int rc = sfh_check_launch("jpeg_idct_kernel")) return rc;
  if (C == 1) return SFH_OK;
  const int gw = hsamp == 2 ? (W + 1) / 2 : W, gh = hsamp == 2 ? (H + 1) / 2 : H;
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)sfh_cdiv(gw, 64), (unsigned)sfh_cdiv(gh, 4), (unsigned)batch), dim3(kThreads),
                     0, (hipStream_t)stream, staged, a, bgr ? 1 : 0, scratch, out, status);
  return sfh_check_launch("jpeg_color_kernel");
}
