// overlay.hip - the annotated frame a person looks at: class-id mask -> colours -> blend over the video frame, POI markers
// and the score label (viz_preds.py:117-146 with utils/postprocess.py:21-65, predict.py:378-384).
//
// sfh_overlay_render is ONE pass over the frame bytes.  Per output pixel: the class id (one homography evaluation and one
// template tap - the warp leg - or one nearest-resized read of the segmentation source), a palette look-up and an integer
// blend with the three frame bytes.  Compulsory traffic: 3 B read + 3 B written per pixel, one template, 36 B of theta per
// frame.  Which leg a frame takes is decided on the device from score[b] (no host synchronisation); the frame index is
// blockIdx.y, so the choice is uniform in a workgroup.
//
// The warp leg restates warp.hip's nearest arithmetic in its plain IEEE form (apply_h / norm_axis / unnorm: individually
// rounded fp32 operations in the order of oracle/warp_ref.py; the file is built with -ffp-contract=off).  warp.hip's
// launch kernel replaces the divisions by Newton forms that its exhaustive self-test (sfh_selftest_warp_arith) shows to be
// the correctly rounded quotients, so both give the same ids bit for bit; the kernel here stays VALU-bound by those
// divisions, not by bandwidth.
//
// sfh_overlay_annotate is one small launch: one workgroup per (frame, marker) and one per (frame, label).  Every pixel has
// exactly ONE writer: a marker's workgroup leaves out the pixels that a later marker or the label covers, so "a later
// point index wins, the label is drawn last" holds without any ordering between workgroups and without a store race.
#include "common.h"

namespace {

struct Homog {
  float t[9];
};

__device__ __forceinline__ void apply_h(const Homog& H, float x, float y, float& u, float& v) {
  const float X = __fadd_rn(__fadd_rn(__fmul_rn(H.t[0], x), __fmul_rn(H.t[1], y)), H.t[2]);
  const float Y = __fadd_rn(__fadd_rn(__fmul_rn(H.t[3], x), __fmul_rn(H.t[4], y)), H.t[5]);
  const float Z = __fadd_rn(__fadd_rn(__fmul_rn(H.t[6], x), __fmul_rn(H.t[7], y)), H.t[8]);
  const float s = (fabsf(Z) > 1e-8f) ? __fdiv_rn(1.0f, __fadd_rn(Z, 1e-8f)) : 1.0f;
  u = __fmul_rn(s, X);
  v = __fmul_rn(s, Y);
}

__device__ __forceinline__ float norm_axis(int i, int n) {
  // create_meshgrid: (i/(n-1) - 0.5) * 2
  return __fmul_rn(__fsub_rn(__fdiv_rn((float)i, (float)(n - 1)), 0.5f), 2.0f);
}

__device__ __forceinline__ float unnorm(float c, int size) {
  // ATen CPU grid sampler, align_corners=False: fma(fl(c + 1), size/2, -0.5) (oracle/warp_ref.py:unnormalize)
  return __builtin_fmaf(__fadd_rn(c, 1.0f), 0.5f * (float)size, -0.5f);
}

__device__ __forceinline__ float fetch(const float* __restrict__ tm, float fx, float fy, int wt, int ht) {
  // fx, fy are integral-valued floats (or NaN/inf): in range -> template value, else 0 (grid_sample's zeros padding)
  if (fx >= 0.f && fx <= (float)(wt - 1) && fy >= 0.f && fy <= (float)(ht - 1))
    return tm[(int)fy * wt + (int)fx];
  return 0.f;
}

// class id -> colour, packed c0 | c1 << 8 | c2 << 16; 0 = "keep the frame"
struct OvPalette {
  uint32_t c[8];
};

// KIND 0: int32 ids, 1: uint8 ids, 2: fp32 logits NCHW (first maximum wins, as mask_format_kernel)
template <int KIND>
__device__ __forceinline__ int segm_id_at(const void* __restrict__ src, long b, int nc, int hs, int ws, int sy, int sx) {
  if (KIND == 0) return ((const int32_t*)src)[(b * hs + sy) * ws + sx];
  if (KIND == 1) return ((const uint8_t*)src)[(b * hs + sy) * ws + sx];
  const float* lg = (const float*)src + (b * nc * hs + sy) * (long)ws + sx;
  const long plane = (long)hs * ws;
  int best = 0;
  float bv = lg[0];
  for (int k = 1; k < nc; ++k) {
    const float v = lg[k * plane];
    if (v > bv) { bv = v; best = k; }
  }
  return best;
}

// per byte floor((a + b) / 2) of the three packed bytes
__device__ __forceinline__ uint32_t avg3(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0x00FEFEFEu) >> 1); }

__device__ __forceinline__ uint32_t blend_px(uint32_t frame, uint32_t colour) { return colour ? avg3(frame, colour) : frame; }

// One thread = four consecutive pixels of a row.  VEC: W % 4 == 0 and 4-byte aligned pointers - the 12 bytes are three
// dwords; otherwise bytes.  KIND 3: no segmentation source.
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void overlay_render_kernel(const uint8_t* frames, uint8_t* out, int H, int W,
                                                             const float* __restrict__ theta, const float* __restrict__ tmpl,
                                                             long tmpl_bstride, int ht, int wt, float out_scale,
                                                             const void* __restrict__ segm, int nc, int hs, int ws,
                                                             double ify, double ifx, const float* __restrict__ score,
                                                             float score_threshold, int source, int use_ot,
                                                             float overlay_threshold, OvPalette pal) {
  const int b = blockIdx.y;
  const int wq = (W + 3) >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= H * wq) return;
  const int y = t / wq;
  const int x0 = (t - y * wq) * 4;
  const int n = min(4, W - x0);
  const float sc = score ? score[b] : 0.f;
  // frame-uniform decisions (a NaN score compares false: segmentation leg, no blend under an overlay threshold)
  const bool use_warp = source == 1 || (source == 0 && sc < score_threshold);
  const bool has_mask = use_warp || KIND != 3;
  const bool blend = has_mask && (!use_ot || sc < overlay_threshold);
  const long off = (((long)b * H + y) * W + x0) * 3;
  const uint8_t* fp = frames + off;
  uint8_t* op = out + off;

  uint32_t col[4] = {0u, 0u, 0u, 0u};
  if (blend) {
    if (use_warp) {
      Homog Hm;
#pragma unroll
      for (int k = 0; k < 9; ++k) Hm.t[k] = theta[b * 9 + k];
      const float* tm = tmpl + (long)b * tmpl_bstride;
      const float yn = norm_axis(y, H);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          float u, v;
          apply_h(Hm, norm_axis(x0 + j, W), yn, u, v);
          const float val = fetch(tm, rintf(unnorm(u, wt)), rintf(unnorm(v, ht)), wt, ht);
          const int id = (int32_t)__fmul_rn(val, out_scale);
          col[j] = pal.c[(id >= 0 && id < 8) ? id : 0];
        }
      }
    } else if (KIND != 3) {
      const int sy = min((int)floor((double)y * ify), hs - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          const int sx = min((int)floor((double)(x0 + j) * ifx), ws - 1);
          const int id = segm_id_at<(KIND == 3 ? 0 : KIND)>(segm, b, nc, hs, ws, sy, sx);
          col[j] = pal.c[(id >= 0 && id < 8) ? id : 0];
        }
      }
    }
  } else if (out == frames) {
    return;   // nothing to draw on this frame and nothing to copy
  }

  if (VEC) {
    const uint32_t* f4 = (const uint32_t*)fp;
    const uint32_t d0 = f4[0], d1 = f4[1], d2 = f4[2];
    const uint32_t r0 = blend_px(d0 & 0x00FFFFFFu, col[0]);
    const uint32_t r1 = blend_px((d0 >> 24) | ((d1 & 0x0000FFFFu) << 8), col[1]);
    const uint32_t r2 = blend_px((d1 >> 16) | ((d2 & 0x000000FFu) << 16), col[2]);
    const uint32_t r3 = blend_px(d2 >> 8, col[3]);
    uint32_t* o4 = (uint32_t*)op;
    o4[0] = r0 | (r1 << 24);
    o4[1] = (r1 >> 8) | (r2 << 16);
    o4[2] = (r2 >> 16) | (r3 << 8);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
        const uint32_t f = (uint32_t)fp[3 * j] | ((uint32_t)fp[3 * j + 1] << 8) | ((uint32_t)fp[3 * j + 2] << 16);
        const uint32_t r = blend_px(f, col[j]);
        op[3 * j] = (uint8_t)r;
        op[3 * j + 1] = (uint8_t)(r >> 8);
        op[3 * j + 2] = (uint8_t)(r >> 16);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- markers and label
// The project's own 5x7 bitmap font (the reference stamps OpenCV's Hershey font, which is not reproduced): one byte per
// glyph row, top row first, bit 4 = leftmost column.  Glyph codes are indices into this table;
// sfh_amd/visualize.py holds the same table (tests/test_overlay_host.py compares the two).
#define SFH_OVERLAY_NGLYPHS 19
__constant__ uint8_t kGlyphs[SFH_OVERLAY_NGLYPHS][7] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E},  // 0
    {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},  // 1
    {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},  // 2
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},  // 3
    {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02},  // 4
    {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},  // 5
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E},  // 6
    {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},  // 7
    {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},  // 8
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C},  // 9
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C},  // .
    {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00},  // -
    {0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00},  // +
    {0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E},  // e
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00},  // space
    {0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11},  // n
    {0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F},  // a
    {0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E},  // i
    {0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08},  // f
};

constexpr int kGlyphW = 5, kGlyphH = 7, kGlyphAdvance = 6;   // one blank column between glyphs

// marker centre of a normalised point: rint (half to even) of the exact fp64 product; false = draws nothing
__device__ __forceinline__ bool marker_centre(const float* __restrict__ p, int H, int W, long& cx, long& cy) {
  const double x = rint((double)p[0] * (double)W), y = rint((double)p[1] * (double)H);
  if (!(fabs(x) < 1e9) || !(fabs(y) < 1e9)) return false;   // NaN, inf, or too far away to reach the frame
  cx = (long)x;
  cy = (long)y;
  return true;
}

// is pixel (x, y) lit by the frame's label?  codes: the frame's L glyph codes (LDS), len: glyphs before the terminator
__device__ __forceinline__ bool label_lit(const int8_t* codes, int len, int lx, int ly, int scale, int x, int y) {
  const int rx = x - lx, ry = y - ly;
  if (rx < 0 || ry < 0) return false;
  const int gx = rx / scale, gy = ry / scale;
  if (gy >= kGlyphH) return false;
  const int ci = gx / kGlyphAdvance, col = gx - ci * kGlyphAdvance;
  if (ci >= len || col >= kGlyphW) return false;
  const int code = codes[ci];
  if (code >= SFH_OVERLAY_NGLYPHS) return false;
  return (kGlyphs[code][gy] >> (kGlyphW - 1 - col)) & 1;
}

// grid (npts_drawn + has_label, B): item < npts_drawn is marker `item`, the last item the label
__global__ __launch_bounds__(256) void overlay_annotate_kernel(uint8_t* out, int H, int W, const float* __restrict__ poi,
                                                               int npts, int npts_drawn, int radius, uint32_t marker_colour,
                                                               const int8_t* __restrict__ labels, int L, int lx, int ly,
                                                               int scale, const float* __restrict__ score,
                                                               float score_threshold, int source) {
  __shared__ int8_t s_codes[SFH_OVERLAY_LABEL_MAX];
  __shared__ int s_len;
  __shared__ long s_cx[256], s_cy[256];
  __shared__ uint8_t s_ok[256];
  const int b = blockIdx.y, item = blockIdx.x, tid = threadIdx.x;
  if (tid < SFH_OVERLAY_LABEL_MAX) s_codes[tid] = (labels && tid < L) ? labels[(long)b * L + tid] : (int8_t)-1;
  __syncthreads();
  if (tid == 0) {
    int len = 0;
    while (len < L && s_codes[len] >= 0) ++len;
    s_len = len;
  }
  __syncthreads();
  const int len = s_len;
  uint8_t* fo = out + (long)b * H * W * 3;

  if (item < npts_drawn) {
    const float* pts = poi + (long)b * npts * 2;
    long cx, cy;
    if (!marker_centre(pts + 2 * item, H, W, cx, cy)) return;      // the whole workgroup: no barrier is left waiting
    const long r2 = (long)radius * radius;
    const int side = 2 * radius + 1;
    for (int p0 = 0; p0 < side * side; p0 += 256) {                // 256 pixels of the disc's bounding square per pass
      const int i = p0 + tid;
      long x = 0, y = 0;
      bool mine = false;
      if (i < side * side) {
        const int dy = i / side - radius, dx = i - (i / side) * side - radius;
        x = cx + dx;
        y = cy + dy;
        mine = (long)dx * dx + (long)dy * dy <= r2 && x >= 0 && x < W && y >= 0 && y < H &&
               !label_lit(s_codes, len, lx, ly, scale, (int)x, (int)y);
      }
      // a later marker over this pixel writes it instead: their centres go through LDS, 256 at a time
      for (int m0 = item + 1; m0 < npts_drawn; m0 += 256) {
        __syncthreads();
        long mx = 0, my = 0;
        const bool ok = m0 + tid < npts_drawn && marker_centre(pts + 2 * (m0 + tid), H, W, mx, my);
        s_cx[tid] = mx;
        s_cy[tid] = my;
        s_ok[tid] = ok;
        __syncthreads();
        const int cnt = min(256, npts_drawn - m0);
        for (int k = 0; k < cnt && mine; ++k)
          if (s_ok[k]) mine = (x - s_cx[k]) * (x - s_cx[k]) + (y - s_cy[k]) * (y - s_cy[k]) > r2;
      }
      if (mine) {
        uint8_t* o = fo + (y * W + x) * 3;
        o[0] = (uint8_t)marker_colour;
        o[1] = (uint8_t)(marker_colour >> 8);
        o[2] = (uint8_t)(marker_colour >> 16);
      }
    }
    return;
  }
  // the label: (0,255,0) where the frame took the warp leg's side of the score threshold, else (0,0,255)
  // (viz_preds.py:125,127, written into the array as given)
  const bool low = score ? score[b] < score_threshold : source == 1;
  const uint8_t c0 = 0, c1 = low ? 255 : 0, c2 = low ? 0 : 255;
  const int cell = scale * scale;
  const long total = (long)len * kGlyphH * kGlyphW * cell;
  for (long i = tid; i < total; i += 256) {
    const int sub = (int)(i % cell);
    const int bit = (int)(i / cell);
    const int ci = bit / (kGlyphH * kGlyphW), gy = (bit / kGlyphW) % kGlyphH, col = bit % kGlyphW;
    const int code = s_codes[ci];
    if (code >= SFH_OVERLAY_NGLYPHS || !((kGlyphs[code][gy] >> (kGlyphW - 1 - col)) & 1)) continue;
    const long x = (long)lx + (long)(ci * kGlyphAdvance + col) * scale + sub % scale;
    const long y = (long)ly + (long)gy * scale + sub / scale;
    if (x < 0 || x >= W || y < 0 || y >= H) continue;
    uint8_t* o = fo + (y * W + x) * 3;
    o[0] = c0;
    o[1] = c1;
    o[2] = c2;
  }
}

}  // namespace

extern "C" int sfh_overlay_render(const uint8_t* frames, uint8_t* out, int batch, int H, int W, const float* theta,
                                  const float* tmpl, int64_t tmpl_bstride, int ht, int wt, float out_scale, const void* segm,
                                  int segm_kind, int nc, int hs, int ws, const float* score, float score_threshold, int source,
                                  int use_overlay_threshold, float overlay_threshold, const uint8_t* palette, void* stream) {
  SFH_REQUIRE(frames && out && palette, "overlay_render: null pointer (frames, out, palette)");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 1 && W > 1 && (int64_t)H * ((W + 3) / 4) < (1LL << 31) - 256,
              "overlay_render: bad geometry b=%d h=%d w=%d", batch, H, W);
  SFH_REQUIRE(source >= SFH_OVERLAY_AUTO && source <= SFH_OVERLAY_SEGM, "overlay_render: source %d (0 auto, 1 warp, 2 segm)",
              source);
  SFH_REQUIRE(score || (source != SFH_OVERLAY_AUTO && !use_overlay_threshold),
              "overlay_render: source auto and an overlay threshold need a score (null pointer)");
  if (source != SFH_OVERLAY_SEGM) {
    SFH_REQUIRE(theta && tmpl, "overlay_render: the warp leg needs theta and a template (null pointer)");
    SFH_REQUIRE(ht > 0 && wt > 0 && (int64_t)ht * wt <= (1 << 22) && W <= (1 << 20) && H <= (1 << 20),
                "overlay_render: template %dx%d (at most 4 Mi pixels) or frame %dx%d too large", wt, ht, W, H);
    SFH_REQUIRE(tmpl_bstride == 0 || tmpl_bstride >= (int64_t)ht * wt, "overlay_render: bad template stride");
  }
  const bool use_segm = segm && source != SFH_OVERLAY_WARP;
  if (use_segm) {
    SFH_REQUIRE(segm_kind >= 0 && segm_kind <= 2, "overlay_render: segm_kind %d (0 int32 ids, 1 uint8 ids, 2 logits)", segm_kind);
    SFH_REQUIRE(hs > 0 && ws > 0, "overlay_render: segmentation source %dx%d", ws, hs);
    SFH_REQUIRE(segm_kind != 2 || nc >= 2, "overlay_render: logits need nc >= 2");
  }
  OvPalette pal;
  for (int k = 0; k < 8; ++k)   // host pointer, copied by value
    pal.c[k] = (uint32_t)palette[k * 3] | ((uint32_t)palette[k * 3 + 1] << 8) | ((uint32_t)palette[k * 3 + 2] << 16);
  const double ify = use_segm ? 1.0 / ((double)H / (double)hs) : 1.0, ifx = use_segm ? 1.0 / ((double)W / (double)ws) : 1.0;
  const bool vec = W % 4 == 0 && (((uintptr_t)frames | (uintptr_t)out) & 3) == 0;
  const dim3 grid((unsigned)sfh_cdiv(H * ((W + 3) / 4), 256), (unsigned)batch);
#define SFH_OV(K, V)                                                                                                     \
  hipLaunchKernelGGL((overlay_render_kernel<K, V>), grid, dim3(256), 0, (hipStream_t)stream, frames, out, H, W, theta, tmpl, \
                     (long)tmpl_bstride, ht, wt, out_scale, segm, nc, hs, ws, ify, ifx, score, score_threshold, source,    \
                     use_overlay_threshold ? 1 : 0, overlay_threshold, pal)
#define SFH_OV_K(K)                 \
  do {                              \
    if (vec) SFH_OV(K, true);       \
    else SFH_OV(K, false);          \
  } while (0)
  const int kind = use_segm ? segm_kind : 3;
  if (kind == 0) SFH_OV_K(0);
  else if (kind == 1) SFH_OV_K(1);
  else if (kind == 2) SFH_OV_K(2);
  else SFH_OV_K(3);
#undef SFH_OV_K
#undef SFH_OV
  return sfh_check_launch("overlay_render_kernel");
}

extern "C" int sfh_overlay_annotate(uint8_t* out, int batch, int H, int W, const float* poi, int npts, int radius,
                                    const uint8_t* marker_color, const int8_t* labels, int L, int label_x, int label_y,
                                    int label_scale, const float* score, float score_threshold, int source, void* stream) {
  SFH_REQUIRE(out, "overlay_annotate: null pointer (out)");
  SFH_REQUIRE(batch > 0 && batch <= 65535 && H > 0 && W > 0, "overlay_annotate: bad geometry b=%d h=%d w=%d", batch, H, W);
  SFH_REQUIRE(radius >= 0 && radius <= 1024, "overlay_annotate: radius %d (0 = no markers, at most 1024)", radius);
  if (poi) {
    SFH_REQUIRE(npts > 0 && npts <= 65535, "overlay_annotate: %d points", npts);
    SFH_REQUIRE(radius == 0 || marker_color, "overlay_annotate: markers need a colour of 3 bytes (null pointer)");
  }
  if (labels) {
    SFH_REQUIRE(L > 0 && L <= SFH_OVERLAY_LABEL_MAX, "overlay_annotate: label of %d glyphs (1 .. %d declared by SFH_OVERLAY_LABEL_MAX)",
                L, SFH_OVERLAY_LABEL_MAX);
    SFH_REQUIRE(label_scale >= 1 && label_scale <= 64, "overlay_annotate: label scale %d (1 .. 64)", label_scale);
    SFH_REQUIRE(source >= SFH_OVERLAY_AUTO && source <= SFH_OVERLAY_SEGM, "overlay_annotate: source %d (0 auto, 1 warp, 2 segm)",
                source);
    SFH_REQUIRE(score || source != SFH_OVERLAY_AUTO, "overlay_annotate: the label's colour needs a score or a forced source (null pointer)");
    SFH_REQUIRE(label_x > -(1 << 24) && label_x < (1 << 24) && label_y > -(1 << 24) && label_y < (1 << 24),
                "overlay_annotate: label position (%d, %d)", label_x, label_y);
  }
  const int drawn = (poi && radius > 0) ? npts : 0;
  const int items = drawn + (labels ? 1 : 0);
  if (items == 0) return SFH_OK;
  const uint32_t mc = marker_color ? ((uint32_t)marker_color[0] | ((uint32_t)marker_color[1] << 8) | ((uint32_t)marker_color[2] << 16)) : 0u;
  hipLaunchKernelGGL(overlay_annotate_kernel, dim3((unsigned)items, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, out, H, W,
                     poi, npts, drawn, radius, mc, labels, labels ? L : 0, label_x, label_y, labels ? label_scale : 1, score,
                     score_threshold, source);
  return sfh_check_launch("overlay_annotate_kernel");
}
