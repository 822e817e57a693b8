"""Exponents and range words of the H2 ("f16x3") activation tensors of one model: pure host logic around one device
read-back per pass."""
import math

import torch

from . import _lib
from .ops import _ptr, _stream, filled


class FP16RangeExhausted(RuntimeError):
    """an "f16x3" activation tensor is saturated and its exponent cannot be lowered any further"""


class H2Ranges:
    """Exponents and range words of the H2 (two-plane fp16, "f16x3") activation tensors of one model.

    An H2 tensor stores u = v * 2^e and saturates beyond |v| = 65504 * 2^-e (include/sfh_amd.h); below |u| = 2^-3 its
    low plane is an fp16 subnormal and the element keeps fewer than 22 bits.  Every tensor NAME has an exponent KEY -
    tensors that enter one conv as its two sources share a key, and so do a conv output and the pooled copy its
    producer writes - and a device word that the producing kernels raise (atomic max) to the largest bit pattern of
    |v * 2^e| they produced, before saturation.  After a forward pass the host reads the words (`read`) and decides
    in BOTH directions, one decision per key:

    * a word above H2_LIMIT_BITS: the tensor was saturated; how far it overshot gives the exponent that fits (`lower`);
    * every written word of a key below RAISE_BELOW (= 4: the largest element of the key's tensors sits within 2^5 of
      the subnormal boundary, so a typical element, an order of magnitude below the peak, has lost bits - a "quiet"
      layer): the exponent is RAISED so that the peak lands in [2^12, 2^13) like after `lower` (`quiet` / `raise_`).

    The engines then repeat the pass from the first step that writes such a tensor.  Exponents start at the conventional
    2; the state is sticky, shared by the UNet and ResNet engines of a Reconstructor and kept across engine rebuilds
    (same model, new weights).  Hysteresis: the words are running maxima since the last reset (a reset happens only
    together with a decision), so a key is raised only if EVERYTHING since then was quiet, and a key that `lower` has
    touched is never raised above the exponent `lower` gave it until the weights change (`new_generation`)."""

    LIMIT = _lib.H2_LIMIT_BITS
    NONFINITE = 0x7F800000
    DEFAULT = _lib.H2_ACT_EXP
    MIN_EXP = -64
    MAX_EXP = 48          # |v| down to 2^-36 reaches [2^12, 2^13); the kernels take -64 .. 64
    RAISE_BELOW = 4.0     # stored peak |v * 2^e| below which a key counts as quiet (see above)

    def __init__(self, device, capacity=1024):
        self.device = device
        self.words = filled((capacity,), torch.int32, device) if torch.device(device).type == "cuda" else \
            torch.zeros(capacity, dtype=torch.int32, device=device)        # (CPU: the host-logic tests)
        self.exps = {}     # key -> exponent (absent = DEFAULT)
        self.slot = {}     # tensor name -> (key, word index)
        self.peak = {}     # tensor name -> largest |v| seen so far (host side, from read())
        self.ceiling = {}  # key -> exponent `lower` gave it in this weights generation: `raise_` never exceeds it
        self._nwords = 0

    def register(self, name, key=None, word_of=None):
        """name: tensor; key: name of an already registered tensor whose exponent it shares; word_of: name of a
        tensor whose word it shares (a pooled copy: its values are a subset of the other tensor's)."""
        cur = self.slot.get(name)
        k = self.slot[key][0] if key is not None else name
        if cur is not None:
            if cur[0] != k:
                raise ValueError(f"H2 tensor {name!r} is tied to exponent key {cur[0]!r}, not {k!r}")
            return
        if word_of is not None:
            idx = self.slot[word_of][1]
        else:
            idx = self._nwords
            self._nwords += 1
            if idx >= self.words.numel():
                raise RuntimeError("H2Ranges: out of range words")
        self.slot[name] = (k, idx)

    def exp(self, name):
        s = self.slot.get(name)
        return self.exps.get(s[0], self.DEFAULT) if s is not None else self.DEFAULT

    def key(self, name):
        return self.slot[name][0]

    def word_ptr(self, name):
        s = self.slot.get(name)
        return self.words.data_ptr() + 4 * s[1] if s is not None else None

    def args(self, src=None, dst=None, res=None):
        """keyword arguments of PackedConv.run / StemConv.run for a launch reading `src`, writing `dst` (+ residual)"""
        return {"exp_src": self.exp(src), "exp_dst": self.exp(dst), "exp_res": self.exp(res),
                "range_word": self.word_ptr(dst)}

    def read(self):
        """One device read-back: {tensor name: bit pattern of the largest |v * 2^e| since the words were zeroed}."""
        n = self._nwords
        if n == 0:
            return {}
        vals = self.words[:n].cpu().numpy().view("uint32")
        out = {}
        for name, (key, idx) in self.slot.items():
            b = int(vals[idx])
            out[name] = b
            if 0 < b < self.NONFINITE:
                v = _bits_to_float(b) * 2.0 ** -self.exps.get(key, self.DEFAULT)
                if v > self.peak.get(name, 0.0):
                    self.peak[name] = v
        return out

    def saturated(self, bits):
        """names whose tensor left the fp16 range, and whether any of them holds a non-finite value"""
        bad = [n for n, b in bits.items() if b > self.LIMIT]
        return bad, any(bits[n] >= self.NONFINITE for n in bad)

    def lower(self, bad, bits):
        """Lower the exponents of the saturated tensors `bad` (names; bits = read()'s dict): ONE decision per exponent
        key - a conv output and its pooled copy share word and key, a skip tensor and its up tensor share a key - from
        the largest word of the key's tensors, converted with the exponent that was in force when the words were
        written.  The new exponent puts the observed maximum into [2^12, 2^13) (8x headroom).  -> the set of keys.
        Raises FP16RangeExhausted if a key cannot go lower (the caller falls back to the three-plane operands)."""
        worst = {}
        for n in bad:
            key = self.slot[n][0]
            worst[key] = max(worst.get(key, 0), bits[n])
        before = {key: self.exps.get(key, self.DEFAULT) for key in worst}
        for key, b in worst.items():
            e = before[key]
            vmax = _bits_to_float(b) * 2.0 ** -e
            new = 13 - math.frexp(vmax)[1]                 # frexp: vmax = m * 2^x, 0.5 <= m < 1
            new = max(self.MIN_EXP, min(new, e - 1))
            if new >= e:
                raise FP16RangeExhausted(f"H2 tensor group {key!r} is saturated at the lowest exponent {e}")
            self.exps[key] = new
            self.ceiling[key] = new
        return set(worst)

    def quiet(self, bits):
        """The other direction (bits = read()'s dict of a pass WITHOUT saturated tensors): {key: larger exponent} for
        every key whose written tensors all peaked below RAISE_BELOW in stored units - the largest word of the key,
        converted with the exponent in force, goes to [2^12, 2^13).  A tensor whose word is still zero (a resumed pass
        starts behind it) is judged by the peak it showed earlier in this weights generation; one that was never seen
        says nothing, and a key with no seen tensor is left alone.  Never above the
        exponent `lower` gave the key in this weights generation, never above MAX_EXP."""
        top, skip = {}, set()
        for n, b in bits.items():
            s = self.slot.get(n)
            if s is None:
                continue
            key = s[0]
            if b > self.LIMIT:
                skip.add(key)                              # saturated / non-finite: `lower`'s business
                continue
            if b:
                stored = _bits_to_float(b)
            else:
                # not written since the words were zeroed (a resumed pass starts behind this tensor): what it showed
                # BEFORE the reset still counts - its largest |v| of this weights generation, in today's stored units -
                # so that a key shared by an early and a late tensor is never judged on the late one alone
                v = self.peak.get(n)
                if v is None:
                    continue                               # never seen (or all zeros): says nothing
                stored = v * 2.0 ** self.exps.get(key, self.DEFAULT)
            top[key] = max(top.get(key, 0.0), stored)
        plan = {}
        for key, stored in top.items():
            if key in skip or stored >= self.RAISE_BELOW or stored <= 0.0:
                continue
            e = self.exps.get(key, self.DEFAULT)
            new = 13 - math.frexp(stored * 2.0 ** -e)[1]
            new = min(new, self.MAX_EXP, self.ceiling.get(key, self.MAX_EXP))
            if new > e:
                plan[key] = new
        return plan

    def raise_(self, plan):
        """apply quiet()'s plan -> the set of keys (the caller zeroes the words and repeats the pass from the first
        launch that writes one of them)"""
        self.exps.update(plan)
        return set(plan)

    def new_generation(self):
        """The model's weights changed (or its mode): what the words and the `lower` ceilings say belongs to the old
        weights.  The exponents stay - they are the best guess for the new weights - and are re-examined in both
        directions by the first pass."""
        self._zero_words()
        self.ceiling.clear()
        self.peak.clear()

    def reset_words(self):
        self._zero_words()

    def _zero_words(self):
        if self.words.is_cuda:
            with torch.cuda.device(self.words.device):
                _lib.check(_lib.load().sfh_fill_words(_ptr(self.words), self.words.numel(), 0, _stream()), "fill_words")
        else:
            self.words.zero_()

    def headroom(self):
        """{tensor name: 65504 * 2^-e / largest |v| seen} - how far each tensor is from saturating"""
        return {n: 65504.0 * 2.0 ** -self.exp(n) / v for n, v in self.peak.items() if v > 0}


def _bits_to_float(b):
    import struct
    return struct.unpack("<f", struct.pack("<I", b & 0xFFFFFFFF))[0]


class _NoRanges:
    """stands in for H2Ranges in the other precisions: default exponents, no words"""

    def register(self, *a, **k):
        pass

    def exp(self, name):
        return _lib.H2_ACT_EXP

    def key(self, name):
        return name

    def word_ptr(self, name):
        return None

    def args(self, src=None, dst=None, res=None):
        return {}
