"""Launch plans for the HIP hot path: weight packing, NHWC workspaces and the sequence
of C-ABI calls that implements ``forward_unet`` / ``ResNetSTN`` / warp.

PyTorch is used here for device memory (``torch.empty``), the current HIP stream and the parameter storage only; every
arithmetic step is a call into ``libsfh_amd.so``.  Host-prep helpers and format / layout wrappers: ``ops.py``; H2 range
bookkeeping: ``h2ranges.py`` (both re-exported here).
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib
from ._lib import ConvDesc
from .h2ranges import FP16RangeExhausted, H2Ranges, _bits_to_float, _NoRanges  # noqa: F401
from .options import Options
from .ops import (PRECISIONS, _SPLIT, _SPLIT_DTYPES, _area_tab, _chan, _f32_to_split_into, _f32c,  # noqa: F401
                  _fmt_code, _fmt_of, _hw, _ptr, _split_to_f32_into, _stream, _stream_scope, absminmax, absminmax_words,
                  consistency_ce, f32_to_h2, f32_to_s3, f32_to_split, filled, frames_u8_to_input, h2_weight_exp,
                  nchw_to_nhwc, nhwc_to_nchw, poi_project, resize_nchw, resolve_wexp, rows_all_equal, s3_empty, s3_to_f32,
                  slice_in_channels, snapshot, split_empty, split_shape, stn_input_assemble, vec_op, weight_exps)

# (tile id, rows, cols) of the stride-1 workgroup tiles; stride-2 tiles have half the rows.
_TILES = ((_lib.TILE_8x32, 8, 32), (_lib.TILE_16x16, 16, 16), (_lib.TILE_32x8, 32, 8))

# half-size tiles of the split-bf16 kernel (8 pixel groups): small maps and stride 2
_TILES_S3_HALF = ((_lib.TILE_8x16, 8, 16), (_lib.TILE_16x8, 16, 8))
_WG_SLOTS = 512  # workgroups resident on the chip at two per CU


def _zero_rows(ksize, ho, split):
    """shared zero rows per frame of the flattened row space (csrc/conv_geom.h, sfh_zero_rows): the padding before the window;
    the split-operand kernels keep the rows per frame even (fused 2x2 pool windows never straddle a tile edge)"""
    zr = ksize // 2
    if split:
        zr += (ho + zr) & 1
    return zr


def _ntiles(batch, ho, wo, stride, zr, th, tw):
    """pixel tiles of th x tw outputs (csrc/conv_geom.h, sfh_conv_grid): stride 1 tiles the flattened rows of all frames,
    stride 2 every frame for itself"""
    ty = batch * -(-ho // th) if stride == 2 else -(-(batch * (ho + zr)) // th)
    return ty * -(-wo // tw)


def choose_tile(batch, ho, wo, stride, zrows=1):
    """fp32 kernel: pick the workgroup tile that wastes the fewest padded output pixels."""
    best = None
    for tid, th, tw in _TILES:
        if stride == 2:
            th //= 2
        cost = _ntiles(batch, ho, wo, stride, zrows, th, tw) * th * tw
        if best is None or cost < best[0]:
            best = (cost, tid)
    return best[1]


def choose_tile_s3(batch, ho, wo, stride, zrows, nblk, ksize=3, wg_slots=_WG_SLOTS):
    """split-bf16 kernel: estimated time = rounds of resident workgroups x pixels per tile; the
    half-size tiles win when the full-size grid would leave most of the chip idle (ResNet layer3/4)
    and are the only ones whose stride-2 halo fits LDS."""
    best = None
    if stride == 2:
        cands = _TILES_S3_HALF
    else:  # stride 1: full-size tiles (half-size tiles measured no faster on ResNet layer3/4)
        cands = _TILES
    for tid, th, tw in cands:
        ntiles = _ntiles(batch, ho, wo, stride, zrows, th, tw)
        rounds = -(-(ntiles * nblk) // wg_slots)
        # equal estimates: prefer the larger tile (less per-workgroup overhead, more operand reuse)
        cost = (rounds * th * tw, ntiles * th * tw, -th * tw)
        if best is None or cost < best[0]:
            best = (cost, tid)
    return best[1]


def choose_small_map(batch, ho, wo, zr, cout, tile_id, max_wgs=None):
    """Should a plain 3x3 stride-1 H2 launch take the small-map kernel (csrc/conv_small.hip: 12x20-pixel x 32-cout workgroups)
    instead of conv_s3_kernel with workgroup tile `tile_id`?  Yes when the standard grid is at most one workgroup per CU - one
    wave per SIMD: the launch then takes what its busiest SIMD takes, and only finer work units shorten it - AND the finer tiling
    gives at least 1.2x the workgroups.  At batch 16 and 640x360: ResNet layer4 (192 -> 256 workgroups: 79 -> 50 us) and layer3
    (240 -> 512: equal alone, better under the pipeline); at batch 1 most of the net."""
    th, tw = next((a, b) for t_, a, b in _TILES + _TILES_S3_HALF if t_ == tile_id)
    std = _ntiles(batch, ho, wo, 1, zr, th, tw) * (cout // 64)
    fine = _ntiles(batch, ho, wo, 2, 0, 12, 20) * (cout // 32)   # (tiles per frame, as at stride 2)
    return std <= (_SMALL_MAP_MAX if max_wgs is None else max_wgs) and fine * 5 >= std * 6


def choose_ksplit(batch, ho, wo, stride, cout, nstages, ksize=3, wg_slots=_WG_SLOTS):
    """Split-K factor for a conv whose (pixel tile, 64-cout block) grid fills at most a QUARTER of the chip's
    workgroup slots (small batches: one frame of 640x360 has 4-60 workgroups per ResNet layer): the largest factor
    that keeps the grid within one round of resident workgroups and leaves every split at least two 32-channel
    stages.  1 = no split.  Measured at batch 16 (profiles/r03_resnet_table_*.txt): layer3 (240 workgroups) 53 us
    unsplit against 49 + 10.5 us (conv x2 + finish), layer4 (192) 82 against 74 + 8 - grids of that size are bound
    by the weight stream every pixel tile pulls from L2, not by idle CUs, so they are left alone."""
    zr = _zero_rows(ksize, ho, True)
    cands = _TILES_S3_HALF if stride == 2 else _TILES
    ntiles = min(_ntiles(batch, ho, wo, stride, zr, th, tw) for tid, th, tw in cands)
    wgs = ntiles * (cout // 64)
    if wgs * 4 > wg_slots:
        return 1
    return max(1, min(wg_slots // (2 * wgs), nstages // 2, 8))


ConvRecord = namedtuple("ConvRecord", "tag work e0 e1 executed nbytes")


class ConvTimer:
    """Optional HIP-event timing of conv launches on the launch stream (used by bench.py for the
    live roofline figure).  Records ConvRecord(tag, algorithmic work, start event, end event, executed FLOPs, bytes):
    work = FLOPs of the conv launches, BYTES of the warp launches; executed / nbytes = None where a site has none."""

    def __init__(self, only=None):
        """only: set of tags to time (None = every launch).  bench.py times just the dominant kernel's launches inside the
        headline region - two event records per launch are not free (all 59 timed launches of a step: +0.2 ms) - and every
        group in the unpipelined pass behind it."""
        self.records = []
        self.only = None if only is None else set(only)

    def wants(self, tag):
        return self.only is None or tag in self.only

    def summary(self):
        """-> {tag: (launches, total work, total_ms)}; call after a device synchronize."""
        out = {}
        for rec in self.records:
            n, f, t = out.get(rec.tag, (0, 0.0, 0.0))
            out[rec.tag] = (n + 1, f + rec.work, t + rec.e0.elapsed_time(rec.e1))
        return out

    def traffic(self):
        """-> {tag: ALGORITHMIC HBM bytes of the launches}: every operand tensor read once, every result written once
        (sources at their stored width, packed weights, fp32 seed / residual where a launch has one) - the figure the
        counters' FETCH_SIZE + WRITE_SIZE are compared with (bench.py roofline.traffic_algorithmic)."""
        return self._total("nbytes")

    def executed(self):
        """-> {tag: FLOPs the launches EXECUTED} where that differs from the algorithmic work they are credited with
        (the composed 2x2 Up conv runs 4 taps x 2C channels for the reference's 9 taps x C)."""
        return self._total("executed")

    def _total(self, field):
        out = {}
        for rec in self.records:
            v = getattr(rec, field)
            if v is not None:
                out[rec.tag] = out.get(rec.tag, 0.0) + v
        return out


class _Timing:
    """One timed launch: created = start event recorded; stop() records the end event, add() appends the ConvRecord."""
    __slots__ = ("tm", "tag", "e0", "e1")

    def __init__(self, tm, tag):
        self.tm, self.tag = tm, tag
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def stop(self):
        self.e1.record()

    def add(self, work, executed=None, nbytes=None):
        self.tm.records.append(ConvRecord(self.tag, work, self.e0, self.e1, executed, nbytes))


def _timed(tag):
    """-> a started _Timing if the installed ConvTimer wants `tag`, else None (launch sites test `PackedConv.timer is
    not None` themselves first: the untimed path pays that one test and no call)"""
    tm = PackedConv.timer
    return _Timing(tm, tag) if (tm is not None and tm.wants(tag)) else None


def conv_work(batch, ho, wo, ksize, c0, c1, cout, cout_real, transposed=False, stem_cin=0, flops_per_out_pixel=None,
              src_bpe=4, dst_bpe=4, src0_hw=(0, 0), src1_hw=None, weight_bytes=0, dst_pixels=0, pooled=False, head_nc=0,
              extra_bytes=0):
    """Roofline accounting of one PackedConv launch from plain numbers -> (flops, executed, nbytes).  flops: 2 * MACs of the
    reference op (real cin, real taps); a fused Up conv (flops_per_out_pixel) is credited with the u-half of the reference's
    3x3 conv, `executed` = what the composed conv really multiplies (4 quadrants x 4 taps x all low-resolution channels, 8/9
    of the credit), else None.  nbytes: every operand read once, every result written once, at src_bpe / dst_bpe bytes per
    element (4 for split-K slabs); dst_pixels = B * H * W as dst is written (0: a fused head consumed it)."""
    kk = 49 if ksize == 4 else (4 if transposed else ksize * ksize)
    cin = stem_cin if ksize == 4 else c0 + c1
    flops, executed = 2.0 * batch * ho * wo * cout_real * kk * cin, None
    if flops_per_out_pixel is not None:
        executed = 2.0 * batch * ho * wo * cout * 4 * c0
        flops = flops_per_out_pixel * batch * (2 * ho) * (2 * wo)
    nbytes = batch * src0_hw[0] * src0_hw[1] * c0 * src_bpe + weight_bytes + dst_pixels * cout_real * dst_bpe + extra_bytes
    if src1_hw is not None:
        nbytes += batch * src1_hw[0] * src1_hw[1] * c1 * src_bpe
    if pooled:      # the 2x2 max-pooled copy the epilogue writes beside dst
        nbytes += batch * (ho // 2) * (wo // 2) * cout_real * dst_bpe
    if head_nc:     # the fused OutConv's fp32 logits
        nbytes += batch * ho * wo * head_nc * 4
    return flops, executed, float(nbytes)


def upfused_work(batch, H, W, skip_c0, cout, low_c0, low_hw, flops_per_out_pixel, weight_bytes):
    """conv_work's counterpart for run_upfused -> (flops, executed, nbytes).  Credited like the two launches it replaces:
    the whole reference conv over cat([skip, up]) (9 taps x (c_skip + c_up), c_up recovered from the composed conv's
    flops_per_out_pixel); executed: 9 taps x the skip channels + 4 taps x all low-resolution channels; H2 tensors, 4 B."""
    c_up = flops_per_out_pixel / (2.0 * cout * 9)
    nbytes = (batch * H * W * (skip_c0 + cout) + batch * low_hw[0] * low_hw[1] * low_c0) * 4 + weight_bytes
    return (2.0 * batch * H * W * cout * 9 * (skip_c0 + c_up), 2.0 * batch * H * W * cout * (9 * skip_c0 + 4 * low_c0),
            float(nbytes))


# conv_small.hip (12 x 20-pixel x 32-cout workgroups, halo + weights through LDS; bit-identical results) for 3x3 stride-1 H2
# launches whose standard grid is at most one workgroup per CU, i.e. one wave per SIMD (_SMALL_MAP_MAX workgroups): ResNet layer4
# at batch 16 (192 workgroups -> 256: 79 -> 50 us per launch, profiles/r05_small_map_probe.txt), layer3 (240 -> 512: equal
# alone, +0.2 % under the pipeline), small batches.  Same-device A/B (profiles/r05_ab_small_map.txt): 13.31 -> 13.19 ms per batch
# with the threshold at 224 (layer4 only), 13.09 at 256.
_SMALL_MAP_MAX = 256
_W8_HALF_ROUNDS = 3   # rounds of 512 resident workgroups from which the 128 x 128 workgroup shape is requested
_BPE = {"h2": 4, "s3": 6, None: 4}   # stored bytes per activation element


class LaunchOrder:
    """Direction in which consecutive conv launches of ONE engine (or one training tape) walk their pixel tiles:
    alternating ("snake", sfh_conv_desc.reverse_tiles), so that a launch starts on what the same XCD wrote
    last.  Per owner, not process-wide: the order a model sees does not depend on what else ran."""

    def __init__(self):
        self._flip = False

    def next(self):
        r = self._flip
        self._flip = not self._flip
        return r


_UNIT = {}


def _unit_epilogue(n, dev, scale=1.0):
    """(scale * ones, zeros) of n floats on dev, shared read-only by every backward-data conv (56 per training step;
    scale: the power of two an H2 layer's accumulator is multiplied with)"""
    key = (n, str(dev), float(scale))
    v = _UNIT.get(key)
    if v is None:
        v = _UNIT[key] = (filled((n,), torch.float32, dev, float(scale)), filled((n,), torch.float32, dev))
    return v


class _H2Layer:
    """What PackedConv and StemConv share: the folded per-channel epilogue (`scale`, `shift`) and, for H2 arithmetic, the
    source exponent folded into `scale` (escale = the power of two the accumulator is multiplied with)."""
    _shared_scale = False       # `scale` is a tensor shared with other layers (training): never rewritten in place

    def _fold_epilogue(self, bias, bn, cout_real, rep, dev):
        """scale / shift = bias and BatchNorm (either may be None) folded per channel, repeated rep times, then `escale`
        multiplied into the scale (a power of two: exact)"""
        self.scale, self.shift = (torch.empty(cout_real * rep, dtype=torch.float32, device=dev) for _ in range(2))
        b = _f32c(bias.detach(), "conv bias") if bias is not None else None
        bnt = (bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else (None,) * 4
        args = [_ptr(_f32c(t.detach(), "bn tensor")) if t is not None else None for t in bnt]
        _lib.check(_lib.load().sfh_fold_bn(_ptr(b), *args, float(bn.eps) if bn is not None else 0.0, cout_real, rep,
                                           _ptr(self.scale), _ptr(self.shift), _stream()), "fold_bn")
        self._scale_by_escale()

    def _scale_by_escale(self):
        if self.escale != 1.0:
            vec_op(self.scale, factor=self.escale, out=self.scale)

    def _fold_exp_src(self, e):
        """H2 layer: its sources now carry v * 2^e.  `scale` holds the factor 2^-(wexp + exp_src) that takes the
        accumulator back to real units: multiply the difference in (a power of two: exact)."""
        if e == self.exp_src:
            return
        if self._shared_scale:
            raise ValueError("this layer's epilogue scale is shared with other layers: its source exponent is fixed")
        f = 2.0 ** (self.exp_src - e)
        vec_op(self.scale, factor=f, out=self.scale)
        self.escale *= f
        self.exp_src = e


class PackedConv(_H2Layer):
    """One conv-shaped layer: fragment-ordered weights + folded per-channel epilogue."""

    timer = None   # set to a ConvTimer to time every launch (bench.py / profiling only)

    def _init_fields(self, tag, fmt, ksize, c0, c1, cout, cout_real, relu, stride, transposed, stem_cin):
        """every attribute the class reads, with None / 0 / False where it does not apply"""
        if fmt not in (None, "s3", "h2"):
            raise ValueError(f"fmt={fmt!r}: expected None, 's3' or 'h2'")
        self.tag, self.fmt = tag, fmt
        self.ksize, self.c0, self.c1, self.cout, self.cout_real = ksize, c0, c1, cout, cout_real
        self.relu, self.stride, self.transposed, self.stem_cin = relu, stride, transposed, stem_cin
        self.c4, self.c4h2, self.escale = False, False, 1.0
        self.exp_src = _lib.H2_ACT_EXP   # H2 layers: exponent of the source tensors currently folded into `scale`
        self.wpacked = self.scale = self.shift = None
        self.order = None                # LaunchOrder of the owning engine (set by the engine); None = always forward
        self.overflow = None             # the owner's fp16-range word (set by the engine)
        self._shared_scale = False
        # fused_up only: border shifts, BatchNorm scale alone, credited work, seeded scale / shifts + their exponents, composed weights
        self.shift_border = self.scale_bn = self.flops_per_out_pixel = None
        self._seed_scale = self._seed_border = self._seed_key = self._w2 = None

    @property
    def s3(self):
        """runs on the split-operand kernel"""
        return self.fmt is not None

    def __init__(self, weight, bias, bn, ksize, c0, c1=0, relu=True, transposed=False, stride=1,
                 stem_cin=0, tag="conv", fmt=None, wexp=None, shared_unit_scale=False, frame_h2=False, _geom=None):
        """fmt="s3": sources are split-bf16 (S3) tensors and the contraction runs as six bf16 MFMAs
        per product; fmt="h2": two-plane fp16 (H2) sources, three fp16 MFMAs per product (both sfh_conv_s3_fwd);
        otherwise fp32 sources and fp32 MFMA (sfh_conv_fwd).  frame_h2 (with fmt=None, a 3x3 conv over <= 4 channels: the
        UNet's first layer): the source is the FH2 frame tensor of sfh_frame_to_h2 - held as a float32 (B,H,W,4) tensor, 16
        bytes per pixel - and the contraction runs as three fp16 MFMAs per product (sfh_conv3x3_c4h2_fwd).
        _geom (fused_up / backward_data): (real couts, repeats, pack mode, aux) instead of what the weight's shape says;
        pack mode None: the caller packs (finish_pack)."""
        lib = _lib.load()
        dev = weight.device
        w = _f32c(weight.detach(), "conv weight")
        mode, aux = (1 if transposed else 0), 0
        if _geom is not None:
            cout, rep, mode, aux = _geom
        elif stem_cin:  # 7x7 s2 stem re-expressed as a 4x4 conv over the space-to-depth input
            cout, rep, mode, aux = w.shape[0], 1, 2, stem_cin
            assert ksize == 4 and tuple(w.shape[1:]) == (stem_cin, 7, 7) and c1 == 0
        elif transposed:
            cin, cout, rep = w.shape[0], w.shape[1], 4
            assert ksize == 1 and cin == c0 and c1 == 0 and tuple(w.shape[2:]) == (2, 2)
        else:
            cout, cin, rep = w.shape[0], w.shape[1], 1
            assert cin == c0 + c1 and tuple(w.shape[2:]) == (ksize, ksize), (w.shape, c0, c1, ksize)
        self._init_fields(tag, fmt, ksize, c0, c1, rep * cout, cout, relu, stride, transposed, stem_cin)
        if self.cout_real % 64:
            raise ValueError(f"conv with {self.cout_real} output channels: the MFMA kernel needs a multiple of 64")
        # 3x3 conv over <= 4 input channels (the UNet's first layer): tap-packed kernel
        self.c4 = (_geom is None and not self.s3 and not stem_cin and not transposed and ksize == 3 and stride == 1
                   and c1 == 0 and c0 <= 4)
        self.c4h2 = bool(frame_h2) and self.c4
        if frame_h2 and not self.c4:
            raise ValueError("frame_h2 is the first-layer kernel: a 3x3 stride-1 conv over at most 4 channels, fmt=None")
        if mode is None:        # fused_up packs the composed weights itself (finish_pack)
            pass
        elif self.c4h2:
            wx = resolve_wexp(w, wexp)    # max |w| * 2^wx in [2^13, 2^14)
            self.escale = 2.0 ** -(wx + _lib.H2_ACT_EXP)
            self.wpacked = torch.empty(lib.sfh_packed_c4h2_weight_bytes(self.cout), dtype=torch.uint8, device=dev)
            _lib.check(lib.sfh_pack_c4h2_weights(_ptr(w), _ptr(self.wpacked), c0, self.cout, wx, _stream()), "pack_c4h2_weights")
        elif self.c4:
            self.wpacked = torch.empty((self.cout // 64) * 9 * 256, dtype=torch.float32, device=dev)
            _lib.check(lib.sfh_pack_c4_weights(_ptr(w), _ptr(self.wpacked), c0, self.cout, _stream()), "pack_c4_weights")
        elif self.s3:
            self._pack_split(w, ksize, c0, c1, mode, aux, wexp)
        else:
            n = lib.sfh_packed_weight_floats(ksize, c0, c1, self.cout)
            if n <= 0:
                raise ValueError(f"unsupported {'backward-data' if mode in (3, 4) else 'conv'} geometry ksize={ksize} "
                                 f"c0={c0} c1={c1} cout={self.cout}")
            self.wpacked = torch.empty(n, dtype=torch.float32, device=dev)
            _lib.check(lib.sfh_pack_conv_weights(_ptr(w), _ptr(self.wpacked), ksize, c0, c1, self.cout,
                                                 mode, aux, _stream()), "pack_conv_weights")
        if shared_unit_scale and bn is None:
            # training convs (one PackedConv per layer and step): no BatchNorm to fold - the scale is the layer's
            # power-of-two factor times ones, shared read-only between all layers of that size, the shift the bias
            # itself: no kernel launch here (a step builds 114 of these objects)
            self.scale, zeros = _unit_epilogue(self.cout, dev, self.escale)
            b = _f32c(bias.detach(), "conv bias") if bias is not None else None
            self.shift = zeros if b is None else (b if rep == 1 else b.repeat(rep))
            self._shared_scale = True
        else:
            self._fold_epilogue(bias, bn, self.cout_real, rep, dev)

    @property
    def stats_ok(self):
        """this layer's launch can leave BatchNorm batch statistics from its epilogue (run(stats=...))"""
        return (self.fmt == "h2" and self.ksize in (1, 3) and self.stride == 1 and not self.relu and not self.transposed
                and not self.stem_cin and not self.c4)

    def _pack_split(self, w, ksize, c0, c1, mode, aux, wexp=None):
        """Pack w for the split-operand kernel in this layer's format.  H2: planes of w * 2^wexp with
        max |w| * 2^wexp in [2^13, 2^14) (wexp given by a caller that has the maximum already, else one
        device read-back here); self.escale = 2^-(wexp + H2_ACT_EXP) is what the accumulator has to be
        multiplied with (the caller folds it into `scale`)."""
        lib = _lib.load()
        if self.fmt == "h2":
            n = lib.sfh_packed_h2_weight_bytes(ksize, c0, c1, self.cout)
        else:
            n = lib.sfh_packed_s3_weight_bytes(ksize, c0, c1, self.cout)
        if n <= 0:
            raise ValueError(f"unsupported split-kernel conv geometry ksize={ksize} c0={c0} c1={c1} cout={self.cout}")
        self.wpacked = torch.empty(n, dtype=torch.uint8, device=w.device)
        if self.fmt == "h2":
            wexp = resolve_wexp(w, wexp)
            self.escale = 2.0 ** -(wexp + _lib.H2_ACT_EXP)
            _lib.check(lib.sfh_pack_h2_weights(_ptr(w), _ptr(self.wpacked), ksize, c0, c1, self.cout, mode, aux, wexp,
                                               _stream()), "pack_h2_weights")
        else:
            _lib.check(lib.sfh_pack_s3_weights(_ptr(w), _ptr(self.wpacked), ksize, c0, c1, self.cout, mode, aux,
                                               _stream()), "pack_s3_weights")

    @classmethod
    def fused_up(cls, conv, bn, up, c0, tag="fusedup2x2", fmt="s3", defer_pack=False):
        """The u-half of conv3x3(cat([skip, ConvTranspose2d(x)])) (+bias, BN, ReLU) as ONE 2x2 conv over the
        low-resolution x with quadrant scatter (sfh_compose_up_weights): takes x (S3), adds the fp32
        partial of the skip-half conv as residual and writes the activated S3 output.  Split-bf16 kernel only."""
        wc = _f32c(conv.weight.detach(), "conv weight")
        wt = _f32c(up.weight.detach(), "up weight")
        bt = _f32c(up.bias.detach(), "up bias")
        dev = wc.device
        cout, cin = wc.shape[0], wc.shape[1]
        cx, c1 = wt.shape[0], wt.shape[1]
        assert cin == c0 + c1 and tuple(wc.shape[2:]) == (3, 3) and tuple(wt.shape[2:]) == (2, 2)
        if cout % 64 or cx % 32:
            raise ValueError("fused Up conv needs cout % 64 == 0 and a multiple of 32 low-resolution channels")
        # a 2x2 up-scatter conv over the cx low-resolution channels; BatchNorm folded (escale comes with finish_pack)
        self = cls(wc, conv.bias, bn, 2, cx, relu=True, transposed=True, tag=tag, fmt=fmt, _geom=(cout, 4, None, 0))
        self.flops_per_out_pixel = 2.0 * cout * 9 * c1   # the part of the reference conv this launch stands for
        self._w2 = torch.empty((4 * cout, cx, 2, 2), dtype=torch.float32, device=dev)
        self.shift_border = torch.empty((16, 4 * cout), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().sfh_compose_up_weights(_ptr(wc), cout, c0, c1, _ptr(wt), cx, _ptr(bt), _ptr(self.scale),
                                              _ptr(self.shift), _ptr(self._w2), _ptr(self.shift_border), _stream()),
                   "compose_up_weights")
        # the skip-half conv of the block applies the same BatchNorm scale to ITS accumulator (UNetEngine)
        self.scale_bn = snapshot(self.scale)
        if not defer_pack:          # defer_pack: the engine packs all composed weights behind ONE batched |w| read-back
            self.finish_pack()
        return self

    def finish_pack(self, wexp=None):
        """second half of fused_up(): pack the composed weights (H2: with exponent wexp, else from a read-back here)"""
        self._pack_split(self._w2, 2, self.c0, 0, 0, 0, wexp)
        self._w2 = None
        self._scale_by_escale()

    @classmethod
    def backward_data(cls, weight, ksize, transposed=False, tag="bwd_data", fmt=None, wexp=None):
        """The conv that maps dz -> dx for a stride-1 nn.Conv2d (OIHW weight; taps flipped, channels
        swapped: pack mode 3) or for nn.ConvTranspose2d k2 s2 (IOHW weight; a 1x1 conv over
        space_to_depth2(dY): pack mode 4).  fp32 kernel; output channels padded to a multiple of 64."""
        w = weight.detach()
        if transposed:
            cin, cout = w.shape[0], w.shape[1]
            assert ksize == 1 and tuple(w.shape[2:]) == (2, 2)
            c0, mode, aux = 4 * cout, 4, cout
        else:
            cout, cin = w.shape[0], w.shape[1]
            assert tuple(w.shape[2:]) == (ksize, ksize) and ksize in (1, 3)
            c0, mode, aux = cout, 3, cin
        if cin % 64:
            raise ValueError(f"backward-data conv needs a multiple of 64 input channels, got {cin}")
        # no bias, no BatchNorm: the unit epilogue shared by every backward-data conv of that size
        return cls(w, None, None, ksize, c0, relu=False, tag=tag, fmt=fmt, wexp=wexp, shared_unit_scale=True,
                   _geom=(cin, 1, mode, aux))

    # ---- one launch: run() is the sequence of the steps below
    def _out_geometry(self, H, W):
        """-> output rows, columns and the shared zero rows per frame of the flattened tile grid"""
        pad2 = self.ksize // 2 + (self.ksize - 1) // 2  # pad before + pad after
        ho = (H + pad2 - self.ksize) // self.stride + 1
        wo = (W + pad2 - self.ksize) // self.stride + 1
        return ho, wo, _zero_rows(self.ksize, ho, self.fmt is not None)

    def _pick_tile(self, batch, ho, wo, zr, wg_couts, plain):
        """-> (tile id, wg_couts) where the caller names no tile; plain: no fused head, statistics or split-K"""
        if self.fmt is None:
            return choose_tile(batch, ho, wo, self.stride, zr), wg_couts
        # 128 x 128 double-buffered workgroups (conv_s3.hip): measured +3 % for 128 / 256 input channels on grids of many
        # rounds (64 -> 128: +4 %), slower for longer K or few rounds (profiles/r03_conv_rate_probe_w8half.txt)
        if (plain and self.fmt == "h2" and self.ksize == 3 and self.stride == 1 and wg_couts == 0
                and self.cout % 128 == 0 and 64 <= self.c0 + self.c1 <= 256):
            nt = _ntiles(batch, ho, wo, 1, zr, 8, 16)
            if nt * (self.cout // 128) >= _W8_HALF_ROUNDS * _WG_SLOTS:
                return _lib.TILE_8x16, 128
        return choose_tile_s3(batch, ho, wo, self.stride, zr, self.cout // 64, self.ksize), wg_couts

    def _check_tensors(self, src0, src1, dst, dst_pool, residual, out_bhw):
        """formats, destination shape and the 4 GiB range of the tensors of a launch -> format of dst"""
        fmt, dfmt = self.fmt, _fmt_of(dst)
        if _fmt_of(src0) != fmt or (src1 is not None and _fmt_of(src1) != fmt):
            raise ValueError(f"layer of format {fmt} got a source of dtype {src0.dtype}")
        if fmt is not None and dfmt not in (None, fmt):
            raise ValueError(f"layer of format {fmt} cannot write a {dst.dtype} destination")
        for t in (dst_pool, residual):
            if t is not None and _fmt_of(t) not in (None, dfmt):
                raise ValueError(f"dst_pool / residual of dtype {t.dtype} beside a {dst.dtype} destination")
        if src1 is None and self.c1:
            raise ValueError("layer was packed for two sources")
        if (dst.shape[0],) + _hw(dst) != out_bhw or _chan(dst) < self.cout_real:
            raise ValueError(f"conv dst shape {tuple(dst.shape)} does not match {out_bhw + (self.cout_real,)}")
        for t in (dst, dst_pool, residual, src0, src1):
            if t is not None and t.numel() * t.element_size() >= 0xFFFFFFF0:
                raise ValueError(f"tensor of {t.numel() * t.element_size()} bytes exceeds the 4 GiB buffer-descriptor "
                                 "range of the conv kernels; split the batch")
        return dfmt

    def _fill_desc(self, d, src0, src1, dst, dfmt, batch, H, W, pool0, pad1, residual, dst_pool, up_dst, head, exp_dst,
                   exp_res, range_word, acc_init, scale, shift_border, stats, bwd):
        """the descriptor of a plain launch (tile, wg_couts and reverse_tiles are run()'s)"""
        d.h2_exp_src = self.exp_src
        if exp_dst is not None:
            d.h2_exp_dst = int(exp_dst)
        if exp_res is not None:
            d.h2_exp_res = int(exp_res)
        d.src0 = src0.data_ptr()
        d.c0, d.cs0 = self.c0, _chan(src0)
        d.h0, d.w0 = _hw(src0)
        d.src_fmt = _SPLIT[self.fmt][2] if self.fmt else _lib.FMT_F32
        d.dst_fmt = _SPLIT[dfmt][2] if dfmt else _lib.FMT_F32
        ovf = self.overflow
        d.h2_overflow = ovf.data_ptr() if (ovf is not None and dfmt == "h2") else None
        d.h2_range = range_word if (range_word and dfmt == "h2") else None
        if dst_pool is not None:
            d.dst_pool, d.pool_cs = dst_pool.data_ptr(), _chan(dst_pool)
        d.pool0 = 1 if pool0 else 0
        if src1 is not None:
            d.src1 = src1.data_ptr()
            d.c1, d.cs1 = self.c1, _chan(src1)
            d.h1, d.w1 = _hw(src1)
            d.pad_top1, d.pad_left1 = pad1
        d.batch, d.H, d.W = batch, H, W
        d.ksize, d.stride = self.ksize, self.stride
        d.wpacked, d.shift = self.wpacked.data_ptr(), self.shift.data_ptr()
        d.scale = (scale if scale is not None else self.scale).data_ptr()
        d.cout, d.relu = self.cout, 1 if self.relu else 0
        if acc_init is not None:
            if acc_init.dtype != torch.float32 or tuple(acc_init.shape) != (batch, H, W, self.cout) or not acc_init.is_contiguous():
                raise ValueError(f"acc_init must be a contiguous float32 tensor {(batch, H, W, self.cout)}")
            d.acc_init = acc_init.data_ptr()
        if stats is not None:
            if (stats.dtype != torch.float64 or not stats.is_contiguous() or stats.dim() != 3
                    or tuple(stats.shape[1:]) != (2, self.cout)):
                raise ValueError(f"stats must be a contiguous float64 tensor (rows, 2, {self.cout})")
            d.stats_partial, d.stats_rows = stats.data_ptr(), int(stats.shape[0])
            if bwd is not None:
                z, mi, gamma, beta = bwd
                if (z.dtype != torch.float32 or not z.is_contiguous() or tuple(z.shape) != tuple(dst.shape)
                        or dst.dtype != torch.float32 or mi.numel() != 2 * self.cout):
                    raise ValueError("bwd: z must be a contiguous float32 tensor of dst's shape, mean_invstd 2 * cout floats")
                d.bwd_z, d.bwd_mi = z.data_ptr(), mi.data_ptr()
                d.bwd_gamma, d.bwd_beta = gamma.data_ptr(), beta.data_ptr()
        elif bwd is not None:
            raise ValueError("bwd needs the stats table")
        if head is not None:   # OutConv fused behind this conv (sfh_conv_desc.head_*)
            d.head_w, d.head_b, d.head_nc = head["w"].data_ptr(), head["b"].data_ptr(), head["nc"]
            d.head_logits = head["logits"].data_ptr()
            d.head_stn = head["stn"].data_ptr() if head.get("stn") is not None else None
            d.head_frame = head["frame"].data_ptr() if head.get("frame") is not None else None
            d.head_skip_dst = 1 if head.get("skip_dst") else 0
        d.residual = residual.data_ptr() if residual is not None else None
        d.residual_f32 = 1 if (residual is not None and residual.dtype == torch.float32 and dfmt is not None) else 0
        sb = shift_border if shift_border is not None else self.shift_border
        d.shift_border = sb.data_ptr() if sb is not None else None
        d.dst, d.dst_cs = dst.data_ptr(), _chan(dst)
        d.out_mode = _lib.OUT_UPSCATTER2 if self.transposed else _lib.OUT_NHWC
        if up_dst is not None:   # fused Up block with F.pad: the destination is one row / column short of 2*H x 2*W
            d.up_dst_h, d.up_dst_w = up_dst

    def _splitk(self, d, src1, dst, dfmt, dst_pool, head, residual, batch, ho, wo, ksplit, slabs, exp_dst, exp_res,
                range_word):
        """rewrite the descriptor for ksplit copies of the grid writing fp32 partial slabs -> the callable that adds them
        up with this layer's shift, residual and ReLU into dst (sfh_splitk_finish)"""
        lib = _lib.load()
        if not self.s3 or src1 is not None or dst_pool is not None or head is not None or self.transposed:
            raise ValueError("split-K needs a plain single-source conv on the split-operand kernel")
        if slabs is None or slabs.dtype != torch.float32 or tuple(slabs.shape) != (ksplit, batch, ho, wo, self.cout):
            raise ValueError(f"split-K slabs must be a float32 tensor {(ksplit, batch, ho, wo, self.cout)}")
        if _chan(dst) != self.cout:
            raise ValueError("split-K writes all channels of dst")
        zero_shift = _unit_epilogue(self.cout, dst.device)[1]
        d.dst, d.dst_cs, d.dst_fmt = slabs.data_ptr(), self.cout, _lib.FMT_F32
        d.shift, d.relu, d.residual, d.residual_f32 = zero_shift.data_ptr(), 0, None, 0
        d.h2_overflow = d.h2_range = None
        d.ksplit, d.ksplit_stride = int(ksplit), slabs.stride(0) * 4
        res_fmt = _fmt_code(residual) if residual is not None else 0
        ovf = self.overflow

        def finish():
            _lib.check(lib.sfh_splitk_finish(
                _ptr(slabs), int(ksplit), slabs.stride(0) * 4, _ptr(self.shift), _ptr(residual), res_fmt,
                int(exp_res) if exp_res is not None else _lib.H2_ACT_EXP, 1 if self.relu else 0, batch * ho, wo,
                _chan(dst), _ptr(dst), _fmt_code(dst), int(exp_dst) if exp_dst is not None else _lib.H2_ACT_EXP,
                ctypes.c_void_p(ovf.data_ptr()) if (ovf is not None and dfmt == "h2") else None,
                ctypes.c_void_p(range_word) if (range_word and dfmt == "h2") else None, _stream()),
                "splitk_finish")
        return finish

    def _pick_kernel(self, d, src0, batch, ho, wo, zr, small, auto, plain):
        """-> the sfh_*_fwd entry point of this launch.  small: True / False / None as run()'s; auto: the caller named
        neither tile nor wg_couts; plain: one source and no pooled output / head / acc_init / statistics / split-K"""
        lib = _lib.load()
        small_ok = (plain and self.fmt == "h2" and self.ksize == 3 and self.stride == 1 and not self.transposed
                    and not d.residual_f32 and not d.shift_border)
        if small and not small_ok:
            raise ValueError("the small-map kernel takes a plain 3x3 stride-1 H2 conv (one source, no pooled output / head / "
                             "acc_init / statistics / split-K)")
        if self.c4:
            if src0.shape[-1] != 4 or d.pool0 or d.dst_pool:
                raise ValueError("the <=4-channel first-layer kernel needs an fp32 NHWC source with 4 stored channels")
            if self.c4h2:
                d.src_fmt = _lib.FMT_FH2   # the (B,H,W,4) float32 tensor holds sfh_frame_to_h2's 16-byte pixels, not floats
                return lib.sfh_conv3x3_c4h2_fwd
            return lib.sfh_conv3x3_c4_fwd
        if small is None and small_ok and auto:
            small = choose_small_map(batch, ho, wo, zr, self.cout, d.tile)
        if small:
            d.wg_couts = 0          # (the small-map launcher chooses its LDS buffering itself)
            return lib.sfh_conv_small_fwd
        return lib.sfh_conv_s3_fwd if self.fmt is not None else lib.sfh_conv_fwd

    def run(self, src0, batch, H, W, dst, src1=None, pool0=False, pad1=(0, 0), residual=None, tile=None,
            dst_pool=None, up_dst=None, head=None, wg_couts=0, exp_src=None, exp_dst=None, exp_res=None,
            range_word=None, ksplit=0, slabs=None, acc_init=None, scale=None, shift_border=None, stats=None, bwd=None,
            small=None):
        """src0/src1: NHWC float32 tensors, or split tensors of the layer's format (S3 bfloat16 / H2 float16);
        dst/residual/dst_pool: float32 NHWC or the same split format (by dtype).  H, W: conv input frame.
        H2 tensors: exp_src / exp_dst / exp_res = exponents of the sources / dst and dst_pool / an H2 residual
        (None: the conventional SFH_H2_ACT_EXP), range_word: device address of dst's range word (H2Ranges).
        ksplit > 1 (split-operand kernel, one source): the K loop is split over ksplit copies of the grid that write
        fp32 partial slabs (`slabs`: float32 tensor (ksplit, B, Ho, Wo, cout)), and sfh_splitk_finish adds them up
        with this layer's shift, residual and ReLU into dst - for grids that alone leave most of the chip idle.
        acc_init (3x3 stride 1): float32 NHWC (B, H, W, cout) tensor the accumulators start from, in accumulator units
        (sfh_conv_desc.acc_init); scale / shift_border: tensors used instead of the layer's own for this launch.
        stats (training, H2 3x3 stride-1 layers with a plain fp32 dst): zero-filled float64 table (rows, 2, cout), rows a
        power of two - the epilogue adds the per-wave sums of z and z^2 for batch-statistics BatchNorm into it
        (sfh_conv_desc.stats_partial; PackedConv.stats_ok says whether a layer qualifies).  bwd (with stats, this launch
        being a backward-data conv): (z, mean_invstd, gamma, beta) of the BatchNorm + ReLU layer whose only gradient dst
        is - the table then receives sum g and sum g * xhat (sfh_conv_desc.bwd_z).
        small: True / False forces / forbids the small-map kernel (sfh_conv_small_fwd: plain 3x3 stride-1 H2 launches, same
        bits); None: the engine's rule - the standard grid is at most one workgroup per CU (one wave per SIMD)
        and the finer tiling gives at least 1.2x the workgroups."""
        if (self.fmt == "h2" or self.c4h2) and exp_src is not None:
            self._fold_exp_src(int(exp_src))
        split_k = bool(ksplit and ksplit > 1)
        ho, wo, zr = self._out_geometry(H, W)
        out_bhw = (batch,) + (tuple(up_dst) if up_dst is not None else (2 * ho, 2 * wo) if self.transposed else (ho, wo))
        dfmt = self._check_tensors(src0, src1, dst, dst_pool, residual, out_bhw)
        d = ConvDesc()
        auto = tile is None
        if auto:
            tile, wg_couts = self._pick_tile(batch, ho, wo, zr, wg_couts, head is None and stats is None and not split_k)
        d.tile, d.wg_couts = tile, wg_couts   # wg_couts 0: the launcher decides (sfh_conv_desc.wg_couts)
        self._fill_desc(d, src0, src1, dst, dfmt, batch, H, W, pool0, pad1, residual, dst_pool, up_dst, head, exp_dst, exp_res,
                        range_word, acc_init, scale, shift_border, stats, bwd)
        d.reverse_tiles = 1 if (self.fmt is not None and self.order is not None and self.order.next()) else 0
        finish = self._splitk(d, src1, dst, dfmt, dst_pool, head, residual, batch, ho, wo, ksplit, slabs, exp_dst, exp_res,
                              range_word) if split_k else None
        fwd = self._pick_kernel(d, src0, batch, ho, wo, zr, small, auto and wg_couts == 0,
                                src1 is None and dst_pool is None and head is None and acc_init is None and stats is None
                                and not split_k)
        t = _timed(self.tag) if PackedConv.timer is not None else None
        _lib.check(fwd(ctypes.byref(d), _stream()), "conv_s3_fwd" if self.fmt is not None else "conv_fwd")
        if finish is not None:
            finish()
        if t is not None:
            t.stop()
            skip_dst = head is not None and head.get("skip_dst")
            t.add(*conv_work(
                batch, ho, wo, self.ksize, self.c0, self.c1, self.cout, self.cout_real, self.transposed, self.stem_cin,
                self.flops_per_out_pixel, src_bpe=_BPE[self.fmt], dst_bpe=4 if split_k else _BPE[dfmt],
                src0_hw=(d.h0, d.w0), src1_hw=(d.h1, d.w1) if src1 is not None else None,
                weight_bytes=self.wpacked.numel() * self.wpacked.element_size(),
                dst_pixels=0 if skip_dst else out_bhw[0] * out_bhw[1] * out_bhw[2], pooled=dst_pool is not None,
                head_nc=head["nc"] if head is not None else 0,
                extra_bytes=sum(x.numel() * x.element_size() for x in (residual, acc_init) if x is not None)))
        return dst


def run_upfused(fu, sk, skip, ylow, dst, batch, H, W, exp_dst=None, range_word=None):
    """The first conv of a fused Up block as ONE launch (sfh_conv_upfused_fwd): fu / sk = the composed 2x2 conv and the skip-half
    3x3 conv of the level (PackedConv.fused_up / the skip-half PackedConv) with fu._seed_scale / fu._seed_border up to date (the
    composed conv's scale and border shifts in sk's accumulator units, as the two-launch form passes them to its first launch);
    skip / ylow / dst: H2 tensors.  Bit-identical to fu.run(...part...) followed by sk.run(..., acc_init=part)."""
    d = ConvDesc()
    d.src0, d.c0, d.cs0 = skip.data_ptr(), sk.c0, _chan(skip)
    d.h0, d.w0 = _hw(skip)
    d.src1, d.c1, d.cs1 = ylow.data_ptr(), fu.c0, _chan(ylow)
    d.h1, d.w1 = _hw(ylow)
    d.batch, d.H, d.W, d.ksize, d.stride = batch, H, W, 3, 1
    d.wpacked, d.scale, d.shift = sk.wpacked.data_ptr(), sk.scale.data_ptr(), sk.shift.data_ptr()
    d.cout, d.relu = sk.cout, 1
    d.up_wpacked, d.up_scale = fu.wpacked.data_ptr(), fu._seed_scale.data_ptr()
    d.shift_border = fu._seed_border.data_ptr()
    d.dst, d.dst_cs = dst.data_ptr(), _chan(dst)
    d.src_fmt = d.dst_fmt = _lib.FMT_H2
    d.out_mode = _lib.OUT_NHWC
    if exp_dst is not None:
        d.h2_exp_dst = int(exp_dst)
    d.h2_overflow = sk.overflow.data_ptr() if sk.overflow is not None else None
    d.h2_range = range_word if range_word else None
    if (dst.shape[0],) + _hw(dst) != (batch, H, W) or _hw(skip) != (H, W) or _fmt_of(dst) != "h2" or _fmt_of(skip) != "h2":
        raise ValueError("run_upfused: skip and dst must be H2 tensors of the output's size")
    t = _timed("upfused") if PackedConv.timer is not None else None
    _lib.check(_lib.load().sfh_conv_upfused_fwd(ctypes.byref(d), _stream()), "conv_upfused_fwd")
    if t is not None:
        t.stop()
        t.add(*upfused_work(batch, H, W, sk.c0, sk.cout, fu.c0, (d.h1, d.w1), fu.flops_per_out_pixel,
                            sk.wpacked.numel() * sk.wpacked.element_size() + fu.wpacked.numel() * fu.wpacked.element_size()))
    return dst


def inc_fused_ok(l0, l3):
    """can the pair (first conv over the FH2 frame, second conv) of a DoubleConv run as ONE launch (run_inc_fused)?"""
    return (l0.c4h2 and l3.fmt == "h2" and l0.cout == l0.cout_real == 64 and l3.cout == l3.cout_real == 64 and l3.c0 == 64
            and l3.c1 == 0 and l3.ksize == 3 and l3.stride == 1 and not l3.transposed and l0.wpacked is not None)


def run_inc_fused(l0, l3, frame, dst, batch, H, W, dst_pool=None, exp_frame=None, exp_mid=None, exp_dst=None,
                  range_mid=None, range_dst=None):
    """The UNet's first DoubleConv as ONE launch (sfh_conv_inc_fused_fwd, csrc/conv_inc_fused.hip): l0 = the first-layer
    PackedConv over the FH2 frame tensor (frame_h2=True, 64 couts), l3 = the 64 -> 64 H2 conv behind it; frame: the float32
    (B,H,W,4) tensor of sfh_frame_to_h2; dst / dst_pool: H2 tensors.  The 64-channel intermediate exists in LDS only; its
    exponent (exp_mid) and range word (range_mid) are used and written as by the two launches.  Bit-identical to
    l0.run(frame, ..., mid) followed by l3.run(mid, ..., dst, dst_pool=dst_pool)."""
    if not inc_fused_ok(l0, l3):
        raise ValueError("run_inc_fused: needs the FH2 first-layer conv (<= 4 -> 64 channels) and a plain 64 -> 64 3x3 H2 conv")
    if (tuple(frame.shape) != (batch, H, W, 4) or frame.dtype != torch.float32 or _fmt_of(dst) != "h2"
            or (dst.shape[0],) + _hw(dst) != (batch, H, W) or _chan(dst) < 64):
        raise ValueError("run_inc_fused: frame must be the float32 (B,H,W,4) FH2 tensor, dst an H2 tensor of the frame's size")
    if dst_pool is not None and (_fmt_of(dst_pool) != "h2" or (dst_pool.shape[0],) + _hw(dst_pool) != (batch, H // 2, W // 2)
                                 or _chan(dst_pool) < 64):
        raise ValueError("run_inc_fused: dst_pool must be an H2 tensor of half the frame's size")
    for t in (frame, dst, dst_pool):
        if t is not None and t.numel() * t.element_size() >= 0xFFFFFFF0:
            raise ValueError("run_inc_fused: a tensor exceeds the 4 GiB buffer-descriptor range of the conv kernels; split the batch")
    if exp_frame is not None:
        l0._fold_exp_src(int(exp_frame))
    if exp_mid is not None:
        l3._fold_exp_src(int(exp_mid))
    ovf = l3.overflow
    d0, d3 = ConvDesc(), ConvDesc()
    for d, layer in ((d0, l0), (d3, l3)):
        d.batch, d.H, d.W, d.h0, d.w0, d.ksize, d.stride = batch, H, W, H, W, 3, 1
        d.wpacked, d.scale, d.shift = layer.wpacked.data_ptr(), layer.scale.data_ptr(), layer.shift.data_ptr()
        d.cout, d.relu, d.out_mode = 64, 1 if layer.relu else 0, _lib.OUT_NHWC
        d.h2_exp_src, d.dst_fmt = layer.exp_src, _lib.FMT_H2
        d.h2_overflow = ovf.data_ptr() if ovf is not None else None
    d0.src0, d0.c0, d0.cs0, d0.src_fmt = frame.data_ptr(), l0.c0, 4, _lib.FMT_FH2
    d0.h2_exp_dst = l3.exp_src
    d0.h2_range = range_mid if range_mid else None
    d3.c0, d3.cs0, d3.src_fmt = 64, 64, _lib.FMT_H2
    d3.dst, d3.dst_cs = dst.data_ptr(), _chan(dst)
    if dst_pool is not None:
        d3.dst_pool, d3.pool_cs = dst_pool.data_ptr(), _chan(dst_pool)
    if exp_dst is not None:
        d3.h2_exp_dst = int(exp_dst)
    d3.h2_range = range_dst if range_dst else None
    d3.tile = _lib.TILE_8x32
    # one launch where the two-launch form asks the order once too (the first-layer kernel has no tile direction)
    d3.reverse_tiles = 1 if (l3.order is not None and l3.order.next()) else 0
    t = _timed("incfused") if PackedConv.timer is not None else None
    _lib.check(_lib.load().sfh_conv_inc_fused_fwd(ctypes.byref(d0), ctypes.byref(d3), _stream()), "conv_inc_fused_fwd")
    if t is not None:
        t.stop()
        t.add(*inc_fused_work(batch, H, W, l0.c0, sum(x.wpacked.numel() * x.wpacked.element_size() for x in (l0, l3)),
                              dst_pool is not None))
    return dst


def inc_fused_work(batch, H, W, c0, weight_bytes, pooled):
    """conv_work's counterpart for run_inc_fused -> (flops, executed, nbytes).  Credited with both reference convs (9 taps x
    c0 -> 64 and 9 taps x 64 -> 64; the halo pixels of the first one that neighbouring workgroups recompute are not counted);
    bytes: the 16-byte FH2 frame pixels in, the H2 output (4 B per element) and its pooled copy out, the weights."""
    flops = 2.0 * batch * H * W * 64 * 9 * (c0 + 64)
    nbytes = batch * H * W * (16 + 64 * 4) + weight_bytes
    if pooled:
        nbytes += batch * (H // 2) * (W // 2) * 64 * 4
    return flops, None, float(nbytes)


class _Workspace:
    """Named activation buffers, one per name: a call with another shape (a different batch size, the tail
    chunk of a sub-batched call) replaces the buffer instead of keeping a second full activation set in HBM."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, name, shape, dtype=torch.float32, zero=False):
        key = (tuple(shape), dtype)
        cur = self.bufs.get(name)
        if cur is None or cur[0] != key:
            self.bufs.pop(name, None)      # release the old block to the allocator before asking for the new one
            t = (filled(shape, dtype, self.device) if (zero and torch.empty((), dtype=dtype).element_size() == 4)
                 else (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device))
            self.bufs[name] = (key, t)
            return t
        return cur[1]


class _Engine:
    """What the two engines share: precision, H2 range state, workspaces and the record / replay protocol - run() records
    every launch as a step, so that the range guard can repeat the pass from the first one that writes a changed tensor."""

    def __init__(self, device, precision, overflow, ranges, options):
        if precision not in PRECISIONS:
            raise ValueError(f"precision={precision!r}: expected one of {sorted(PRECISIONS)}")
        self.device = device
        self.options = options if options is not None else Options()
        self.ws = _Workspace(device)
        self.fmt = fmt = PRECISIONS[precision]
        self.s3 = fmt is not None          # split-format activations
        self.overflow = overflow if fmt == "h2" else None
        self.ranges = (ranges if ranges is not None else H2Ranges(device)) if fmt == "h2" else _NoRanges()
        self.order = LaunchOrder()
        self.steps = []            # launches of the last run(), in order: [(names of the H2 tensors written, fn)]
        self._last_out = None

    def _adopt(self, layers):
        """self.L = layers, each launching in this engine's order and reporting to its overflow word"""
        self.L = layers
        for layer in layers.values():
            layer.order = self.order
            layer.overflow = self.overflow

    def _do(self, outs, fn):
        """record + execute one launch; outs = names of the H2 tensors it writes; everything that depends on an
        exponent is looked up inside fn, i.e. again when the step is repeated"""
        self.steps.append((tuple(outs), fn))
        fn()

    def first_step(self, keys):
        """index of the first launch of the last run() that writes an H2 tensor whose exponent key is in `keys`"""
        rg = self.ranges
        return next((i for i, (outs, _) in enumerate(self.steps) if any(rg.key(n) in keys for n in outs)), None)

    def rerun(self, first):
        """Repeat the launches of the last run() from index `first` on (same buffers, same output tensors) with the
        exponents H2Ranges holds NOW: what the range guard does after lowering the exponent of a saturated tensor."""
        with _stream_scope():
            for _, fn in self.steps[first:]:
                fn()
        return self._last_out


class UNetEngine(_Engine):
    """forward_unet (models/reconstructor.py:132-158) on the HIP kernels."""

    def __init__(self, net, device, precision="bf16x6", overflow=None, ranges=None, options=None):
        """precision: "bf16x6" - activations in split-bf16 (S3) format, contractions as six bf16
        MFMAs per product with fp32 accumulation (fp32-equivalent accuracy); "f16x3" - two-plane fp16 (H2)
        activations, three fp16 MFMAs per product (22-bit operands; `ranges`: the model's H2Ranges - per-tensor
        exponents and the device words the kernels raise to the largest magnitude they produced; `overflow`:
        optional int32 device word OR-ed with 1 on any saturation); "fp32" - fp32 activations and fp32 MFMA.
        options: the model's Options record (None: the defaults)."""
        super().__init__(device, precision, overflow, ranges, options)
        fmt, s3, options = self.fmt, self.s3, self.options
        self.bilinear = bool(net.unet_bilinear)
        # In every fused Up level the composed 2x2 conv runs first (see run()) and the skip-half 3x3 conv finishes.  Round 2
        # (the partial added as a residual at the end of the 3x3 conv): none 629, {4} 634, {3,4} 638, all four 635 frames/s;
        # round 3 (the 3x3 conv STARTS from the partial, sfh_conv_desc.acc_init), one device, ms per batch: {3,4} without
        # seeding 14.58 / 14.70, {3,4} seeded 14.58 / 14.66, {2,3,4} 14.60 / 14.57, all four 14.43 / 14.56
        self.up_seed = {}          # level -> the skip-half conv starts from the partial (sfh_conv_desc.acc_init)
        # options.up_single: levels whose fused Up block runs as ONE kernel (csrc/conv_upfused.hip, round 5; bit-identical to the
        # two-launch seeded form).  Same-device A/B at 640x360 x 16 (profiles/r05_ab_up_single.txt), ms per batch pipelined: none
        # 13.13, {4} 12.93, {3,4} 12.91-12.94, {2,3,4} 12.94, all four 13.15 (at long K a wave per parity class streams too many
        # weights); 1280x720: none 50.97, {3,4} 49.9.
        self.nc = net.mask_classes
        L = {}

        # "f16x3": the 3-channel first layer too runs on the fp16 matrix cores, from a frame tensor split once (FH2)
        self.frame_h2 = fmt == "h2"

        # the first DoubleConv (frame -> 64 -> 64) as ONE launch (csrc/conv_inc_fused.hip; bit-identical to the two launches):
        # the 0.94 GB intermediate of a 640x360 x 16 batch never leaves LDS.  Inference only - this engine; a training tape keeps
        # the intermediate for its backward pass.  options.fuse_inc = False restores the two launches.
        self.fuse_inc = self.frame_h2 and options.fuse_inc
        fuse_up = not self.bilinear and s3 and options.fuse_up
        ups = [(i, cin, getattr(net, f"up{i}")) for i, cin in enumerate((1024, 512, 256, 128), start=1)]
        # the skip halves of the Up blocks' first convs (unet/unet_parts.py:67: cat([skip, up])) as tensors of their own
        skip_w = {i: slice_in_channels(up.conv.convs()[0][0].weight, 0, cin // 2) for i, cin, up in ups} if fuse_up else {}
        # "f16x3": the exponent of every weight tensor from ONE batched |w| reduction and one read-back
        wx = weight_exps([p.detach() for n, p in net.named_parameters()
                          if p.dim() == 4 and not n.startswith("resnet_reg.") and p.is_contiguous()]
                         + list(skip_w.values())) if fmt == "h2" else {}

        def wexp(w):
            return wx.get(w.data_ptr())

        def dc(name, block, c0, c1=0, first_fmt=fmt):
            (cv1, bn1), (cv2, bn2) = block.convs()
            L[name + ".0"] = PackedConv(cv1.weight, cv1.bias, bn1, 3, c0, c1, tag="doubleconv3x3", fmt=first_fmt,
                                        frame_h2=(self.frame_h2 and first_fmt is None and c0 <= 4), wexp=wexp(cv1.weight))
            L[name + ".3"] = PackedConv(cv2.weight, cv2.bias, bn2, 3, cv1.out_channels, tag="doubleconv3x3", fmt=fmt,
                                        wexp=wexp(cv2.weight))

        dc("inc", net.inc, 3, first_fmt=None)  # 3-channel input: fp32 kernel (writes the split format itself)
        for i, cin in enumerate((64, 128, 256, 512), start=1):
            dc(f"down{i}", getattr(net, f"down{i}").block, cin)
        for i, cin, up in ups:
            if fuse_up:
                # ConvTranspose2d folded into the consumer conv (used when no F.pad is needed): the
                # skip-half 3x3 conv leaves an fp32 partial, the composed 2x2 conv over the low-resolution
                # tensor finishes it - the up-sampled tensor is never written
                (cv1, bn1), _ = up.conv.convs()
                c0s = cin // 2
                L[f"up{i}.skip"] = PackedConv(skip_w[i], None, None, 3, c0s, relu=False, tag="doubleconv3x3", fmt=fmt,
                                              wexp=wexp(skip_w[i]))
                L[f"up{i}.fused"] = PackedConv.fused_up(cv1, bn1, up.up, c0s, fmt=fmt, defer_pack=True)
            if not self.bilinear:  # bilinear variant (A3b): parameter-free 2x upsampling kernel instead
                L[f"up{i}.up"] = PackedConv(up.up.weight, up.up.bias, None, 1, cin, relu=False, transposed=True,
                                            tag="convT2x2", fmt=fmt, wexp=wexp(up.up.weight))
            dc(f"up{i}.conv", up.conv, cin // 2, cin // 2)  # cat([skip, up]): cin/2 channels each in both variants
        if fuse_up:
            # second batched read-back: the composed 2x2 weights (they exist only now) and the smallest |BatchNorm scale| of
            # each level (accumulator seeding divides by it)
            fus = [L[f"up{i}.fused"] for i, _, _ in ups]
            mm = absminmax([f._w2 for f in fus] + [f.scale_bn for f in fus])
            for k, (i, cin, up) in enumerate(ups):
                fu, sk = fus[k], L[f"up{i}.skip"]
                fu.relu, sk.relu = False, True      # the composed 2x2 conv runs first, the skip-half conv activates
                fu.finish_pack(h2_weight_exp(mm[k][0]) if fmt == "h2" else None)
                cout = up.conv.convs()[0][0].out_channels
                # the partial enters the fused conv's epilogue as a residual, i.e. after the BatchNorm scale:
                # the skip-half carries that scale itself (shift stays 0), times its own operand scaling
                vec_op(fu.scale_bn[:cout], factor=sk.escale, out=sk.scale)
                # accumulator seeding (run()) divides by this scale: only where no channel's BatchNorm scale vanishes
                smin = mm[len(fus) + k][1] * sk.escale
                self.up_seed[i] = 1e-30 < smin < float("inf")
        self._adopt(L)
        # OutConv (+ the STN input) rides in the epilogue of the last 3x3 conv (run() drops it when something else needs y)
        self.fuse_head = s3 and L["up4.conv.3"].cout_real == 64 and options.fuse_head
        # private copies: an engine holds NO live reference to a parameter (see snapshot())
        self.outc_w = snapshot(net.outc.conv.weight)
        self.outc_b = snapshot(net.outc.conv.bias)
        self.outuv = None
        if net.outuv is not None:
            self.outuv = (snapshot(net.outuv.conv.weight), snapshot(net.outuv.conv.bias))

    def run(self, x, want_stn_in=False, want_argmax=False, want_uv=False, stn_slot=0, uv_beside_head=False):
        """x: (B,3,H,W) float32 NCHW on the GPU.  Returns dict with logits (NCHW, fresh),
        and optionally stn_in (NHWC workspace of ceil4(nc + 3) stored channels), argmax (B,H,W uint8), uv, plus the NHWC
        workspace tensors x_top / y4 for callers that need them (x_top_exp: exponent of x_top if it is H2).
        uv_beside_head: with want_uv, the logits and stn_in still come from the fused head - the bits a run without want_uv
        gives - and the last conv also stores y (sfh_conv_desc.head_skip_dst = 0), from which sfh_outconv_fwd takes uv."""
        with _stream_scope():
            return self._run(x, want_stn_in, want_argmax, want_uv, stn_slot, uv_beside_head)

    def _run(self, x, want_stn_in, want_argmax, want_uv, stn_slot=0, uv_beside_head=False):
        """stn_slot: which of the STN-input buffers this pass writes (Reconstructor.predict_async alternates two, so that
        the ResNet of batch k can still read its input while the UNet of batch k + 1 writes the other)"""
        lib = _lib.load()
        x = _f32c(x, "input frames")
        B, C, H, W = x.shape
        if C != 3:
            raise ValueError(f"expected 3 input channels, got {C}")
        if H < 16 or W < 16:
            raise ValueError("frames smaller than 16x16 cannot pass four 2x2 poolings")
        ws, L, rg = self.ws, self.L, self.ranges
        self.steps = []
        do = self._do

        xin = ws.get("xin", (B, H, W, 4))
        first = (xin, None)
        if self.frame_h2:
            # one pass writes the fp32 NHWC frame (the fused head reads it) AND its two fp16 planes, 16 bytes per pixel,
            # held as a float32 (B,H,W,4) tensor; "frame" has an exponent and a range word like every H2 tensor
            fh2 = ws.get("frame_h2", (B, H, W, 4))
            rg.register("frame")
            ovf = self.overflow
            do(("frame",), lambda: _lib.check(lib.sfh_frame_to_h2(
                _ptr(x), _ptr(xin), _ptr(fh2), B, 3, H, W, rg.exp("frame"),
                ctypes.c_void_p(ovf.data_ptr()) if ovf is not None else None,
                ctypes.c_void_p(rg.word_ptr("frame")) if rg.word_ptr("frame") else None, _stream()), "frame_to_h2"))
            first = (fh2, "frame")
        else:
            do((), lambda: _lib.check(lib.sfh_nchw_to_nhwc(_ptr(x), _ptr(xin), B, 3, H, W, 4, _stream()), "nchw_to_nhwc"))

        s3, fmt = self.s3, self.fmt

        def act(name, shape_bhw, c, f32=False, key=None, word_of=None):
            """activation workspace: the engine's split format (S3 bf16 / H2 fp16), else fp32 NHWC -> (tensor, name)"""
            if s3 and not f32:
                rg.register(name, key, word_of)
                return ws.get(name, split_shape(fmt, *shape_bhw, c), _SPLIT[fmt][0]), name
            return ws.get(name, tuple(shape_bhw) + (c,)), None

        def dconv(name, src0, h, w, cout, src1=None, pool0=False, pad1=(0, 0), want_pool=False, out_f32=False, head=None):
            """src0 / src1: (tensor, name) pairs"""
            (t0, n0), (t1, _) = src0, (src1 if src1 is not None else (None, None))
            l0, l3 = L[name + ".0"], L[name + ".3"]
            fuse = (self.fuse_inc and name == "inc" and t1 is None and head is None and not pool0 and not out_f32
                    and inc_fused_ok(l0, l3))
            if fuse:    # "inc.mid" keeps its exponent and range word (the range guard reads them) but has no buffer
                rg.register(name + ".mid")
                mid, nmid = None, name + ".mid"
            else:
                mid, nmid = act(name + ".mid", (B, h, w), l0.cout_real)
            out, nout = act(name + ".out", (B, h, w), cout, f32=out_f32)
            pooled, npool = (act(name + ".pool", (B, h // 2, w // 2), cout, key=nout, word_of=nout)
                             if (want_pool and s3) else (None, None))
            if fuse:
                do((nmid, nout), lambda: run_inc_fused(
                    l0, l3, t0, out, B, h, w, dst_pool=pooled, exp_frame=rg.exp(n0), exp_mid=rg.exp(nmid), exp_dst=rg.exp(nout),
                    range_mid=rg.word_ptr(nmid), range_dst=rg.word_ptr(nout)))
                return (out, nout), (pooled, npool)
            do((nmid,) if nmid else (), lambda: l0.run(t0, B, h, w, mid, src1=t1, pool0=pool0, pad1=pad1, **rg.args(n0, nmid)))
            do((nout,) if nout else (), lambda: l3.run(mid, B, h, w, out, dst_pool=pooled, head=head, **rg.args(nmid, nout)))
            return (out, nout), (pooled, npool)

        # encoder: in bf16x6 mode every Down's MaxPool2d(2) is written by the producer's epilogue;
        # in fp32 mode it is applied while the consumer loads its halo (pool0)
        f0, p0 = dconv("inc", first, H, W, 64, want_pool=True)
        feats, pooled = [f0], [p0]
        h, w = H, W
        for i in range(1, 5):
            h, w = h // 2, w // 2
            src = pooled[-1] if s3 else feats[-1]
            cout = L[f"down{i}.3"].cout_real
            f, p = dconv(f"down{i}", src, h, w, cout, pool0=not s3, want_pool=i < 4)
            feats.append(f)
            pooled.append(p)
        y, ny = feats[4]
        logits = torch.empty((B, self.nc, H, W), dtype=torch.float32, device=x.device)
        # cat((logits, frame)) zero-padded to a multiple of 4 stored channels - ResNetEngine.cs_in's rule: 8 up to 5 classes,
        # 12 for 6..8 (the padding channels are zeroed once here and rewritten as zeros by every pass)
        stn_cs = -(-(self.nc + 3) // 4) * 4
        stn_in = (ws.get("stn_in" if not stn_slot else f"stn_in{stn_slot}", (B, H, W, stn_cs), zero=True)
                  if want_stn_in else None)
        head = None
        uv_here = want_uv and self.outuv is not None
        if self.fuse_head and not want_argmax and (not uv_here or uv_beside_head):
            head = {"w": self.outc_w, "b": self.outc_b, "nc": self.nc, "logits": logits, "stn": stn_in,
                    "frame": xin if want_stn_in else None, "skip_dst": not uv_here}
        for i in range(1, 5):
            skip, nskip = feats[4 - i]
            hs, ws_ = _hw(skip)
            hy, wy = _hw(y)
            cout = L[f"up{i}.conv.3"].cout_real
            ey, ex = hs - 2 * hy, ws_ - 2 * wy   # F.pad of Up: diff 1 pads one row / column AFTER the tensor
            if f"up{i}.fused" in L and ey in (0, 1) and ex in (0, 1):
                part = ws.get(f"up{i}.part", (B, hs, ws_, L[f"up{i}.skip"].cout_real))     # fp32 partial
                mid, nmid = act(f"up{i}.conv.mid", (B, hs, ws_), L[f"up{i}.fused"].cout_real)
                fu, sk = L[f"up{i}.fused"], L[f"up{i}.skip"]
                up_dst = (hs, ws_) if (ey or ex) else None

                def level(y=y, ny=ny, skip=skip, nskip=nskip, part=part, mid=mid, nmid=nmid, fu=fu, sk=sk,
                          up_dst=up_dst, hs=hs, ws_=ws_, hy=hy, wy=wy, ey=ey, ex=ex,
                          seed=self.up_seed.get(i, False), single=i in self.options.up_single):
                    if seed:
                        # as below, but the partial is written in the skip-half conv's ACCUMULATOR units (divided by its
                        # scale) and that conv STARTS from it (sfh_conv_desc.acc_init): sixteen loads in its prologue
                        # instead of sixteen dependent reads at its end
                        a_fu, a_sk = rg.args(ny, None), rg.args(nskip, nmid)
                        if fu.fmt == "h2":      # bring both scales up to date with the exponents before dividing them
                            fu._fold_exp_src(a_fu["exp_src"])
                            sk._fold_exp_src(a_sk["exp_src"])
                        key = (fu.exp_src, sk.exp_src)
                        if fu._seed_key != key:
                            # (sk.scale is indexed modulo its length: the four sub-positions share it)
                            fu._seed_scale, fu._seed_border, fu._seed_key = (vec_op(fu.scale, sk.scale, "div"),
                                                                             vec_op(fu.shift_border, sk.scale, "div"), key)
                        if single and fu.fmt == "h2":
                            run_upfused(fu, sk, skip, y, mid, B, hs, ws_, a_sk["exp_dst"], a_sk["range_word"])
                            return
                        fu.run(y, B, hy + ey, wy + ex, part, up_dst=up_dst, scale=fu._seed_scale,
                               shift_border=fu._seed_border, **a_fu)
                        sk.run(skip, B, hs, ws_, mid, acc_init=part, **a_sk)
                    else:
                        # composed 2x2 conv first: it writes the 4 B fp32 partial instead of reading one and writing
                        # 6 B of S3; the MFMA-bound skip-half 3x3 conv then absorbs the residual, the ReLU and the split
                        fu.run(y, B, hy + ey, wy + ex, part, up_dst=up_dst, **rg.args(ny, None))
                        sk.run(skip, B, hs, ws_, mid, residual=part, **rg.args(nskip, nmid))
                do((nmid,) if nmid else (), level)
                ymid, l3 = mid, L[f"up{i}.conv.3"]
                y, ny = act(f"up{i}.conv.out", (B, hs, ws_), cout, f32=(i == 4))
                do((ny,) if ny else (), lambda ymid=ymid, nmid=nmid, y=y, ny=ny, l3=l3, hs=hs, ws_=ws_, i=i:
                   l3.run(ymid, B, hs, ws_, y, head=head if i == 4 else None, **rg.args(nmid, ny)))
                continue
            cup = _chan(y) if self.bilinear else L[f"up{i}.up"].cout_real
            # the up-sampled tensor is the second source of the conv over cat([skip, up]): it shares the skip's exponent
            upb, nup = act(f"up{i}.up", (B, 2 * hy, 2 * wy), cup, key=nskip)
            if self.bilinear:  # nn.Upsample(2x, bilinear, align_corners=True) on an fp32 view of y
                yf = ws.get(f"up{i}.yf", (B, hy, wy, cup)) if s3 else y
                uf = ws.get(f"up{i}.uf", (B, 2 * hy, 2 * wy, cup)) if s3 else upb

                def upsample(y=y, ny=ny, yf=yf, uf=uf, upb=upb, nup=nup, hy=hy, wy=wy, cup=cup):
                    if s3:
                        _split_to_f32_into(y, yf, rg.exp(ny))
                    _lib.check(lib.sfh_upsample2x_bilinear_nhwc(_ptr(yf), _ptr(uf), B, hy, wy, cup, _stream()), "upsample2x")
                    if s3:
                        _f32_to_split_into(uf, upb, self.overflow, rg.exp(nup), rg.word_ptr(nup))
                do((nup,) if nup else (), upsample)
            else:
                lu = L[f"up{i}.up"]
                do((nup,) if nup else (), lambda y=y, ny=ny, upb=upb, nup=nup, lu=lu, hy=hy, wy=wy:
                   lu.run(y, B, hy, wy, upb, **rg.args(ny, nup)))
            dy, dx = hs - 2 * hy, ws_ - 2 * wy
            (y, ny), _ = dconv(f"up{i}.conv", (skip, nskip), hs, ws_, cout, src1=(upb, nup), pad1=(dy // 2, dx // 2),
                               out_f32=(i == 4), head=head if i == 4 else None)
        out = {"x_top": feats[4][0], "x_top_name": feats[4][1], "y4": y}
        amax = torch.empty((B, H, W), dtype=torch.uint8, device=x.device) if want_argmax else None
        if head is None:
            do((), lambda y=y: _lib.check(
                lib.sfh_outconv_fwd(_ptr(y), 64, _ptr(self.outc_w), _ptr(self.outc_b), self.nc, B, H, W,
                                    _ptr(logits), _ptr(amax), _ptr(stn_in), stn_cs if want_stn_in else 0,
                                    _ptr(xin) if want_stn_in else None, 4, _stream()), "outconv"))
        elif head["skip_dst"]:
            out.pop("y4")   # not materialised: the fused head consumed it in registers
        out["logits"] = logits
        if want_argmax:
            out["argmax"] = amax
        if want_stn_in:
            out["stn_in"] = stn_in
        if want_uv and self.outuv is not None:
            uv = torch.empty((B, 2, H, W), dtype=torch.float32, device=x.device)
            do((), lambda y=y: _lib.check(
                lib.sfh_outconv_fwd(_ptr(y), 64, _ptr(self.outuv[0]), _ptr(self.outuv[1]), 2, B, H, W,
                                    _ptr(uv), None, None, 0, None, 0, _stream()), "outconv(uv)"))
            out["uv"] = uv
        self._last_out = out
        return out

    def x_top_exp(self, out):
        """exponent of out["x_top"] when it is an H2 tensor (for nhwc_to_nchw)"""
        return self.ranges.exp(out.get("x_top_name"))


class StemConv(_H2Layer):
    """ResNetSTN stem (7x7 s2 conv + BatchNorm + ReLU) on the tap-packed split-bf16 kernel (csrc/stem.hip):
    reads the fp32 NHWC STN input (8 stored channels; 12 or 16 for 9..16 input channels) directly, no space-to-depth copy."""

    def __init__(self, conv, bn, cin, tag="resnet", fmt="s3", overflow=None, wexp=None, cs=None):
        """cs: stored channels of the input (default: 8 up to 8 input channels, else cin rounded up to 4); 8 selects the
        4-taps-by-8-channels instance, 12 / 16 the 2-taps-by-16-channels one.
        fmt: arithmetic of the kernel - "s3": the input is split into three bf16 planes, six products; "h2": two
        fp16 planes, three products (overflow: the engine's fp16-range word; wexp: the weight exponent, max |w| * 2^wexp
        in [2^13, 2^14), from a caller that has the maximum already - the training tape reads all of them back in one
        batched synchronisation - else one device read-back here)."""
        lib = _lib.load()
        w = _f32c(conv.weight.detach(), "stem weight")
        if cs is None:
            cs = 8 if cin <= 8 else -(-cin // 4) * 4
        if tuple(w.shape) != (64, cin, 7, 7) or cs not in (8, 12, 16) or not 1 <= cin <= cs:
            raise ValueError(f"stem kernel needs a (64, <=16, 7, 7) weight and 8, 12 or 16 stored channels, "
                             f"got {tuple(w.shape)} with {cs} stored")
        if fmt not in ("s3", "h2"):
            raise ValueError(f"fmt={fmt!r}: expected 's3' or 'h2'")
        dev = w.device
        self.tag, self.cin, self.cs, self.fmt, self.overflow = tag, cin, cs, fmt, overflow
        self.exp_src = _lib.H2_ACT_EXP     # h2: the input planes carry x * 2^exp_src (folded into `scale`)
        nbytes, pack = ((lib.sfh_packed_stem_weight_bytes, lib.sfh_pack_stem_weights) if cs == 8 else
                        (lib.sfh_packed_stem16_weight_bytes, lib.sfh_pack_stem16_weights))
        self.wpacked = torch.empty(nbytes(), dtype=torch.uint8, device=dev)
        self.escale = 1.0
        wexp = resolve_wexp(w, wexp) if fmt == "h2" else 0
        if fmt == "h2":
            self.escale = 2.0 ** -(wexp + _lib.H2_ACT_EXP)
        _lib.check(pack(_ptr(w), _ptr(self.wpacked), cin, _SPLIT[fmt][2], wexp, _stream()), "pack_stem_weights")
        self.relu = bn is not None
        if bn is None:   # training: the raw conv output z (batch-statistics BatchNorm follows as its own pass)
            self.scale = torch.full((64,), float(self.escale), dtype=torch.float32, device=dev)
            self.shift = torch.zeros(64, dtype=torch.float32, device=dev)
            return
        self._fold_epilogue(None, bn, 64, 1, dev)

    def run(self, x_nhwc8, B, H, W, dst, exp_src=None, range_word=None):
        """exp_src / range_word (h2 arithmetic): exponent of the split the kernel makes of its fp32 input, and the
        device word that receives the largest |x * 2^exp_src| (H2Ranges).  Built without a BatchNorm (bn=None) the
        launch writes the raw conv output (no ReLU)."""
        d = ConvDesc()
        if self.fmt == "h2" and exp_src is not None:
            self._fold_exp_src(int(exp_src))
        d.h2_exp_src = self.exp_src
        d.h2_range = range_word if (range_word and self.fmt == "h2") else None
        d.src0, d.c0, d.cs0, d.h0, d.w0 = x_nhwc8.data_ptr(), self.cin, self.cs, H, W
        d.batch, d.H, d.W, d.ksize, d.stride = B, H, W, 7, 2
        d.wpacked, d.scale, d.shift = self.wpacked.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr()
        d.cout, d.relu = 64, 1 if self.relu else 0
        d.dst, d.dst_cs, d.out_mode = dst.data_ptr(), dst.shape[3], _lib.OUT_NHWC
        d.src_fmt = d.dst_fmt = _lib.FMT_F32
        d.split_arith = _SPLIT[self.fmt][2]
        d.h2_overflow = self.overflow.data_ptr() if (self.overflow is not None and self.fmt == "h2") else None
        ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if tuple(dst.shape) != (B, ho, wo, 64) or tuple(x_nhwc8.shape) != (B, H, W, self.cs):
            raise ValueError(f"stem: shapes {tuple(x_nhwc8.shape)} -> {tuple(dst.shape)} do not match {(B, ho, wo, 64)}")
        t = _timed(self.tag) if PackedConv.timer is not None else None
        _lib.check(_lib.load().sfh_stem7x7_fwd(ctypes.byref(d), _stream()), "stem7x7_fwd")
        if t is not None:
            t.stop()
            t.add(2.0 * B * ho * wo * 64 * 49 * self.cin)
        return dst


class GroupedConv(_H2Layer):
    """One grouped 3x3 conv, nn.Conv2d(C, C, 3, stride, 1, groups=G, bias=False) - the conv2 of a ResNeXt Bottleneck
    (models/resnet.py:108-112) - on the plain fp32 kernel of csrc/conv_grouped.hip: fp32 NHWC in and out in every precision
    (one rounding per product and per add is the accuracy the split formats exist to reach).  Like PackedConv it keeps
    private copies only: the packed weights and the folded BatchNorm epilogue."""
    fmt = None
    escale = 1.0

    def __init__(self, weight, bn, groups, stride=1, relu=True, tag="resnet", backward_data=False):
        """bn None: the raw accumulator (training forward; backward_data=True: the stride-1 conv that maps dz -> dx)"""
        lib = _lib.load()
        w = _f32c(weight.detach(), "conv weight")
        C, cg = w.shape[0], w.shape[1]
        if C != groups * cg or tuple(w.shape[2:]) != (3, 3):
            raise ValueError(f"grouped conv weight {tuple(w.shape)} does not match groups={groups}")
        n = lib.sfh_packed_grouped_weight_floats(groups, cg)
        if n <= 0 or stride not in (1, 2) or (backward_data and stride != 1):
            raise ValueError(f"unsupported grouped conv geometry groups={groups} channels per group={cg} stride={stride}")
        self.tag, self.groups, self.cg, self.cout, self.stride, self.relu = tag, groups, cg, C, stride, bool(relu)
        self.order = self.overflow = None      # (set by the owning engine like every layer's; this kernel uses neither)
        self.wpacked = torch.empty(n, dtype=torch.float32, device=w.device)
        _lib.check(lib.sfh_pack_grouped_weights(_ptr(w), _ptr(self.wpacked), groups, cg, 1 if backward_data else 0, _stream()),
                   "pack_grouped_weights")
        self.scale = self.shift = None
        if bn is not None:
            self._fold_epilogue(None, bn, C, 1, w.device)

    def run(self, src, batch, H, W, dst):
        """src (B,H,W,C) -> dst (B,Ho,Wo,C), both contiguous float32 NHWC"""
        ho, wo = (H - 1) // self.stride + 1, (W - 1) // self.stride + 1
        for t, shape in ((src, (batch, H, W, self.cout)), (dst, (batch, ho, wo, self.cout))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"grouped conv: expected a contiguous float32 tensor {shape}, got {t.dtype} {tuple(t.shape)}")
        t = _timed(self.tag) if PackedConv.timer is not None else None
        _lib.check(_lib.load().sfh_conv_grouped_fwd(_ptr(src), _ptr(self.wpacked), _ptr(self.scale), _ptr(self.shift),
                                                    1 if self.relu else 0, _ptr(dst), batch, H, W, self.groups, self.cg,
                                                    self.stride, _stream()), "conv_grouped_fwd")
        if t is not None:
            t.stop()
            t.add(2.0 * batch * ho * wo * self.cout * 9 * self.cg, None,
                  float(4 * (src.numel() + dst.numel() + self.wpacked.numel())))
        return dst


class ResNetEngine(_Engine):
    """ResNetSTN forward (models/resnet.py:235-254) on the HIP kernels (BasicBlock, Bottleneck and ResNeXt depths)."""

    def __init__(self, rn, in_channels, device, precision="bf16x6", overflow=None, ranges=None, options=None):
        """precision "bf16x6" / "f16x3": the 3x3 convs (stride 1 and 2) and the 1x1 stride-2 downsample convs run
        on the split-operand kernel with S3 / H2 activations; the stem runs on the tap-packed split-operand stem kernel
        (8, 12 or 16 stored input channels and 64 output channels), else on the fp32 kernel.
        ranges / overflow / options: as UNetEngine."""
        super().__init__(device, precision, overflow, ranges, options)
        fmt, s3 = self.fmt, self.s3
        self.cin = in_channels
        self.cs_in = -(-in_channels // 4) * 4
        if (4 * self.cs_in) % 16:
            self.cs_in = -(-in_channels // 8) * 8
        L = {}
        # "f16x3": every weight exponent from ONE batched |w| reduction and one read-back
        wx = weight_exps([p.detach() for p in rn.parameters() if p.dim() == 4 and p.is_contiguous()]) if fmt == "h2" else {}

        def PC(w, *a, **k):      # (PackedConv with this engine's exponent table behind it)
            return PackedConv(w, *a, wexp=wx.get(w.data_ptr()), **k)
        # the stem stays on the fp32 kernel: the 16-tap split-bf16 instance spills registers and
        # measured 1.59 ms against 0.55 ms
        L["stem"] = PC(rn.conv0.weight, None, rn.bn1, 4, 4 * self.cs_in, stem_cin=in_channels, tag="resnet")
        # the split precisions with at most 16 input channels: the tap-packed stem kernel (its 8-channel instance for every
        # resnet_input mode up to 5 classes, the 16-channel one for 6..8 classes and for img+mask+uv)
        self.stem7 = (StemConv(rn.conv0, rn.bn1, in_channels, fmt=fmt, overflow=self.overflow,
                               wexp=wx.get(rn.conv0.weight.data_ptr()), cs=self.cs_in)
                      if (s3 and self.cs_in in (8, 12, 16) and rn.conv0.out_channels == 64) else None)
        self.blocks = []
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(rn, f"layer{li}")):
                name = f"layer{li}.{bi}"
                cin = blk.conv1.in_channels
                if hasattr(blk, "conv3"):  # Bottleneck (models/resnet.py:120-140): 1x1, 3x3 (stride), 1x1
                    width, cout = blk.conv1.out_channels, blk.conv3.out_channels
                    L[name + ".conv1"] = PC(blk.conv1.weight, None, blk.bn1, 1, cin, tag="resnet", fmt=fmt)
                    if blk.conv2.groups > 1:   # ResNeXt: the grouped fp32 kernel in every precision (see _run)
                        L[name + ".conv2"] = GroupedConv(blk.conv2.weight, blk.bn2, blk.conv2.groups, stride=blk.stride,
                                                         tag="resnet")
                    else:
                        L[name + ".conv2"] = PC(blk.conv2.weight, None, blk.bn2, 3, width, stride=blk.stride,
                                                tag="resnet", fmt=fmt)
                    L[name + ".conv3"] = PC(blk.conv3.weight, None, blk.bn3, 1, width, tag="resnet",
                                                    fmt=fmt)  # ReLU after the residual add
                else:  # BasicBlock (models/resnet.py:64-82)
                    width = cout = blk.conv1.out_channels
                    L[name + ".conv1"] = PC(blk.conv1.weight, None, blk.bn1, 3, cin, stride=blk.stride,
                                                    tag="resnet", fmt=fmt)
                    L[name + ".conv2"] = PC(blk.conv2.weight, None, blk.bn2, 3, width, tag="resnet",
                                                    fmt=fmt)  # ReLU after the residual add
                if blk.downsample is not None:
                    ds = blk.downsample
                    L[name + ".down"] = PC(ds[0].weight, None, ds[1], 1, cin, relu=False, stride=blk.stride,
                                                   tag="resnet", fmt=fmt)
                self.blocks.append((name, width, cout, blk.stride, blk.downsample is not None, hasattr(blk, "conv3")))
        self._adopt(L)
        self.reg_w = snapshot(rn.reg.weight)
        self.reg_b = snapshot(rn.reg.bias)

    def run(self, y_nhwc, B, H, W, splitk=None):
        """y_nhwc: (B,H,W,cs_in) float32 with channels >= cin zero.  Returns theta (B,1,3,3).
        splitk=False: no split-K at small batches for this pass (Reconstructor.predict_async with pipeline_splitk = False:
        beside another batch's UNet the unsplit launches - fewer, without their finish launches - overlap better)."""
        with _stream_scope():
            return self._run(y_nhwc, B, H, W, splitk)

    def _run(self, y_nhwc, B, H, W, splitk=None):
        lib = _lib.load()
        ws, L, rg = self.ws, self.L, self.ranges
        use_splitk = self.options.splitk and (splitk is None or bool(splitk))
        if y_nhwc.shape[3] != self.cs_in:
            raise ValueError(f"STN input has {y_nhwc.shape[3]} stored channels, engine expects {self.cs_in}")
        self.steps = []
        do = self._do

        s3, fmt = self.s3, self.fmt
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        c1 = ws.get("stem", (B, H2, W2, 64))
        if self.stem7 is not None:
            # the stem kernel splits its fp32 input itself: "rn.stem.in" names that (never stored) split
            rg.register("rn.stem.in")
            do(("rn.stem.in",) if fmt == "h2" else (),
               lambda: self.stem7.run(y_nhwc, B, H, W, c1, exp_src=rg.exp("rn.stem.in"), range_word=rg.word_ptr("rn.stem.in")))
        else:
            s2d = ws.get("s2d", (B, H2, W2, 4 * self.cs_in))
            do((), lambda: _lib.check(lib.sfh_space_to_depth2(_ptr(y_nhwc), _ptr(s2d), B, H, W, self.cs_in, _stream()),
                                      "space_to_depth2"))
            if L["stem"].s3:
                s2d3 = ws.get("s2d.s3", split_shape("s3", B, H2, W2, 4 * self.cs_in), torch.bfloat16)
                do((), lambda: _lib.check(lib.sfh_f32_to_s3(_ptr(s2d), _ptr(s2d3), B * H2, W2, 4 * self.cs_in, _stream()),
                                          "f32_to_s3"))
                s2d = s2d3
            do((), lambda s2d=s2d: L["stem"].run(s2d, B, H2, W2, c1))
        h, w = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1

        def act(name, hh, ww, c):
            if s3:
                rg.register("rn." + name)
                return ws.get(name, split_shape(fmt, B, hh, ww, c), _SPLIT[fmt][0]), "rn." + name
            return ws.get(name, (B, hh, ww, c)), None

        nx = None
        if s3:  # the pooled stem output enters the split domain: pooling and split in one pass (round 4; two launches before)
            x, nx = act("pool.s3", h, w, 64)
            ovf = self.overflow
            do((nx,), lambda x=x, nx=nx: _lib.check(lib.sfh_maxpool3x3s2_split_fwd(
                _ptr(c1), _ptr(x), B, H2, W2, 64, _SPLIT[fmt][2], rg.exp(nx),
                ctypes.c_void_p(ovf.data_ptr()) if (ovf is not None and fmt == "h2") else None,
                ctypes.c_void_p(rg.word_ptr(nx)) if rg.word_ptr(nx) else None, _stream()), "maxpool3x3s2_split"))
        else:
            x = ws.get("pool", (B, h, w, 64))
            do((), lambda x=x: _lib.check(lib.sfh_maxpool3x3s2_fwd(_ptr(c1), _ptr(x), B, H2, W2, 64, _stream()), "maxpool3x3s2"))
        for name, width, cout, stride, has_down, bottleneck in self.blocks:
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1

            def conv(layer, src, nsrc, hh, ww, dst, ndst, residual=None, nres=None):
                pc = L[layer]
                # layer3 / layer4 at batch 16: 60-170 workgroups for 512 slots - split the K loop to fill the chip
                ks, slabs = 1, None
                if s3 and use_splitk:
                    oh, ow = (hh - 1) // pc.stride + 1, (ww - 1) // pc.stride + 1
                    ks = choose_ksplit(B, oh, ow, pc.stride, pc.cout, (pc.c0 + pc.c1) // 32, pc.ksize)
                    if ks > 1:
                        slabs = ws.get(f"slabs{ks}x{oh}x{ow}x{pc.cout}", (ks, B, oh, ow, pc.cout))
                do((ndst,) if ndst else (), lambda: pc.run(src, B, hh, ww, dst, residual=residual, ksplit=ks, slabs=slabs,
                                                           **rg.args(nsrc, ndst, nres)))
            if has_down:
                idn, nidn = act(name + ".idn", ho, wo, cout)
                conv(name + ".down", x, nx, h, w, idn, nidn)
            else:
                idn, nidn = x, nx
            out, nout = act(name + ".out", ho, wo, cout)
            if bottleneck and isinstance(L[name + ".conv2"], GroupedConv):
                # the grouped conv2 reads and writes fp32: conv1 writes fp32 itself (the split kernels take an fp32
                # destination); in the split precisions conv2's output goes through one conversion into t2, which keeps
                # its range word and exponent.  Both steps count as writers of t2, so that a pass resumed for a saturated
                # t2 starts at conv2 and the fp32 buffer between them can be shared by all blocks of one shape.
                gc = L[name + ".conv2"]
                t1 = ws.get(name + ".t1.f32", (B, h, w, width))
                conv(name + ".conv1", x, nx, h, w, t1, None)
                if s3:
                    t2, nt2 = act(name + ".t2", ho, wo, width)
                    t2f = ws.get(f"grouped.f32.{ho}x{wo}x{width}", (B, ho, wo, width))
                    do((nt2,), lambda gc=gc, t1=t1, t2f=t2f, h=h, w=w: gc.run(t1, B, h, w, t2f))
                    do((nt2,), lambda t2f=t2f, t2=t2, nt2=nt2: _f32_to_split_into(t2f, t2, self.overflow, rg.exp(nt2),
                                                                                  rg.word_ptr(nt2)))
                else:
                    t2, nt2 = ws.get(name + ".t2", (B, ho, wo, width)), None
                    do((), lambda gc=gc, t1=t1, t2=t2, h=h, w=w: gc.run(t1, B, h, w, t2))
                conv(name + ".conv3", t2, nt2, ho, wo, out, nout, residual=idn, nres=nidn)
            elif bottleneck:
                t1, nt1 = act(name + ".t1", h, w, width)
                conv(name + ".conv1", x, nx, h, w, t1, nt1)
                t2, nt2 = act(name + ".t2", ho, wo, width)
                conv(name + ".conv2", t1, nt1, h, w, t2, nt2)
                conv(name + ".conv3", t2, nt2, ho, wo, out, nout, residual=idn, nres=nidn)
            else:
                t, nt = act(name + ".t", ho, wo, width)
                conv(name + ".conv1", x, nx, h, w, t, nt)
                conv(name + ".conv2", t, nt, ho, wo, out, nout, residual=idn, nres=nidn)
            x, nx, h, w = out, nout, ho, wo
        if s3:
            xf = ws.get("final.f32", (B, h, w, _chan(x)))
            do((), lambda x=x, nx=nx, xf=xf: _split_to_f32_into(x, xf, rg.exp(nx)))
            x = xf
        theta = torch.empty((B, 9), dtype=torch.float32, device=x.device)
        pooled = ws.get("pooled", (B, x.shape[3]))
        do((), lambda x=x, h=h, w=w: _lib.check(
            lib.sfh_avgpool_linear_fwd(_ptr(x), _ptr(self.reg_w), _ptr(self.reg_b), B, h, w, x.shape[3], 9,
                                       _ptr(pooled), _ptr(theta), _stream()), "avgpool_linear"))
        self._last_out = theta.view(B, 1, 3, 3)
        return self._last_out


def _check_template(template, B, shared_template):
    if template.dim() != 4 or template.shape[1] != 1:
        raise ValueError(f"court template must be (B,1,H,W), got {tuple(template.shape)}")
    if template.shape[0] < B and not shared_template:
        raise ValueError(f"batch {B} exceeds the court template batch {template.shape[0]}")


def homography_warp(theta, template, h, w, nearest, scale=None, want_f32=True, want_i32=False,
                    shared_template=False):
    """theta (B,1,3,3)|(B,3,3); template (>=B,1,ht,wt).  Returns (f32 or None, i32 or None)."""
    theta = _f32c(theta.reshape(-1, 3, 3).contiguous(), "theta")
    template = _f32c(template, "court template")
    B = theta.shape[0]
    _check_template(template, B, shared_template)
    ht, wt = template.shape[2], template.shape[3]
    out_f = torch.empty((B, h, w), dtype=torch.float32, device=theta.device) if want_f32 else None
    out_i = torch.empty((B, h, w), dtype=torch.int32, device=theta.device) if want_i32 else None
    bstride = 0 if shared_template else ht * wt
    t = _timed("warp") if PackedConv.timer is not None else None
    _lib.check(_lib.load().sfh_homography_warp_fwd(_ptr(theta), _ptr(template), bstride, ht, wt, B, h, w,
                                           0 if nearest else 1, float(scale if scale is not None else 1.0),
                                           _ptr(out_f), _ptr(out_i), _stream()), "homography_warp")
    if t is not None:
        t.stop()
        # algorithmic BYTES: every output once, the template once (per frame if not shared), theta
        nout = (1 if want_f32 else 0) + (1 if want_i32 else 0)
        t.add(float(B * h * w * 4 * nout + (1 if shared_template else B) * ht * wt * 4 + 36 * B))
    return out_f, out_i


def warp_consistency(theta, template, logits, scale, shared_template=False, warp_hw=None):
    """predict()'s nearest warp (* mask_classes -> int32) AND the consistency score fused (sfh_warp_consistency_fwd): 4, 7 or 8 classes;
    the warp (warp_hw = (h, w), default the logits' size) has the logits' size or exactly twice it in both directions
    (predict.py's default geometry: the score then goes through the nearest-resized mask, as the reference's).
    -> (warp_mask int32 (B,h,w), score float32 (B,)); the mask is bit-identical to homography_warp()'s."""
    lib = _lib.load()
    theta = _f32c(theta.reshape(-1, 3, 3).contiguous(), "theta")
    template = _f32c(template, "court template")
    logits = _f32c(logits, "logits")
    B, nc, hl, wl = logits.shape
    h, w = (hl, wl) if warp_hw is None else (int(warp_hw[0]), int(warp_hw[1]))
    if (h, w) not in ((hl, wl), (2 * hl, 2 * wl)):
        raise ValueError(f"warp {w}x{h} against logits {wl}x{hl}: the fused kernel takes the same size or exactly twice it")
    if theta.shape[0] != B:
        raise ValueError(f"{theta.shape[0]} homographies for {B} frames of logits")
    _check_template(template, B, shared_template)
    ht, wt = template.shape[2], template.shape[3]
    dev = theta.device
    out_i = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    partial = torch.empty(lib.sfh_warp_consistency_workspace_floats(B, h, w), dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    t = _timed("warp+ce") if PackedConv.timer is not None else None
    _lib.check(lib.sfh_warp_consistency_fwd(_ptr(theta), _ptr(template), 0 if shared_template else ht * wt, ht, wt, B, h, w,
                                            float(scale), _ptr(logits), nc, hl, wl, _ptr(out_i), _ptr(partial), _ptr(score),
                                            _stream()), "warp_consistency")
    if t is not None:
        t.stop()
        # algorithmic BYTES: the logits once, the mask once, the template once (per frame if not shared), theta
        t.add(float(B * (hl * wl * 4 * nc + h * w * 4) + (1 if shared_template else B) * ht * wt * 4 + 36 * B))
    return out_i, score
