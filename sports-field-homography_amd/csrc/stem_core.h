// stem_core.h - the index arithmetic of the tap-packed 7x7 stride-2 stem (csrc/stem.hip), stated once for its two instances.
//
// One v_mfma_f32_16x16x32_{bf16,f16} contracts 32 k-slots: four lane groups (lane / 16) of 8 slots each.  An instance with CH
// channels per tap (CH = 8: up to 8 input channels; CH = 16: 9..16) spends CH / 8 lane groups on one tap, so a k-step covers
// 32 / CH taps and the 49 taps take ceil(49 * CH / 32) steps (13 / 25).  Lane group lg of step s owns
//   tap      st_tap(CH, s, lg)   = (32 / CH) * s + lg / (CH / 8)          (taps >= 49 are padding: zero weights)
//   channels st_chan0(CH, lg) .. + 7,  st_chan0 = 8 * (lg % (CH / 8))     (channels >= cin: zero weights)
// on BOTH operands: the weights are packed in that order, the kernel reads the pixel of that tap and that channel half.
//
// Plain C++, no HIP header: ST_FN marks what the device runs too (tests/stem_core_host_main.cpp walks every index).
#pragma once

#if defined(__HIPCC__)
#define ST_FN __host__ __device__ __forceinline__
#else
#define ST_FN inline
#endif

#define ST_TAPS 49
#define ST_COUT 64

ST_FN constexpr bool st_ch_ok(int ch) { return ch == 8 || ch == 16; }
// stored channels of the fp32 NHWC source an instance accepts
ST_FN constexpr bool st_cs_ok(int ch, int cs) { return ch == 8 ? cs == 8 : (cs == 12 || cs == 16); }
ST_FN constexpr int st_taps_per_step(int ch) { return 32 / ch; }
ST_FN constexpr int st_nstep(int ch) { return (ST_TAPS + st_taps_per_step(ch) - 1) / st_taps_per_step(ch); }
ST_FN constexpr int st_tap(int ch, int s, int lg) { return st_taps_per_step(ch) * s + lg / (ch / 8); }
ST_FN constexpr int st_chan0(int ch, int lg) { return 8 * (lg % (ch / 8)); }

// workgroup tile of OUTPUT pixels (rows x columns) and the halo of source pixels it stages
ST_FN constexpr int st_tile_h(int) { return 8; }
ST_FN constexpr int st_tile_w(int ch) { return ch == 8 ? 32 : 16; }
ST_FN constexpr int st_halo(int n_out) { return 2 * (n_out - 1) + 7; }
ST_FN constexpr int st_halo_h(int ch) { return st_halo(st_tile_h(ch)); }
ST_FN constexpr int st_halo_w(int ch) { return st_halo(st_tile_w(ch)); }
ST_FN constexpr int st_halo_pixels(int ch) { return st_halo_h(ch) * st_halo_w(ch); }
// pixels of one LDS plane (one 16-byte element = 8 channels of one pixel), rounded up to 16
ST_FN constexpr int st_halo_padded(int ch) { return (st_halo_pixels(ch) + 15) / 16 * 16; }
// halo pixel of output pixel (oy, ox) of the tile under tap t: the tap's offset is added to the pixel's
ST_FN constexpr int st_pixel_off(int ch, int oy, int ox) { return 2 * oy * st_halo_w(ch) + 2 * ox; }
// (a padding tap reads tap 48's pixel: its weights are zero, any staged address will do)
ST_FN constexpr int st_tap_off(int ch, int t) {
  return ((t < ST_TAPS ? t : ST_TAPS - 1) / 7) * st_halo_w(ch) + (t < ST_TAPS ? t : ST_TAPS - 1) % 7;
}
// LDS element (16 bytes) of plane p, channel half hf, halo pixel pix: [plane][half][padded pixel]
ST_FN constexpr int st_lds_elem(int ch, int p, int hf, int pix) { return (p * (ch / 8) + hf) * st_halo_padded(ch) + pix; }
ST_FN constexpr int st_lds_bytes(int ch, int np) { return np * (ch / 8) * st_halo_padded(ch) * 16; }

// Packed weights: [step][plane NP][cout subtile 4][lane 64][j 8] 16-bit words; cout = 16 * subtile + (lane & 15), the lane
// group lane >> 4 gives tap and channel half (above), channel = st_chan0 + j.
ST_FN constexpr long st_packed_elems(int ch, int np) { return (long)st_nstep(ch) * np * 4 * 64 * 8; }
ST_FN constexpr long st_packed_index(int np, int s, int p, int sub, int lane, int j) {
  return ((((long)(s * np + p)) * 4 + sub) * 64 + lane) * 8 + j;
}
