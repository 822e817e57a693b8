"""The TIFF files the tests of sfh_amd.tiffdec / sfh_amd.tiffenc share (tests/test_tiff_host.py, tests/test_gpu_tiff.py), built
with numpy, struct and Pillow only - nothing of the library is imported.

The compressed strips come from libtiff itself: the rows of a strip are saved through Pillow as a one-strip ``I;16`` (8 bits:
``L``) image of shape (rows, W C) with ``compression="tiff_lzw"`` and the strip is read back out of that file through tags 273 /
279.  The container - byte order, RowsPerStrip, the predictor tag, SHORT or LONG strip tables - is assembled here by hand; for
predictor 2 the samples are differenced in numpy at a stride of C before libtiff sees them, and for ``MM`` they are byte-swapped
(the differencing is on the values, the swap on what is stored).  A strip above Pillow's 64 KB strip size, and the strips without
EOI, come from the builder's own greedy encoder ``lzw_encode``, which is held byte-equal to libtiff on the strips whose dictionary
does not fill.  Every case carries its source array in the FILE's channel order; a decoder with ``bgr=True`` returns it reversed.
"""
import functools
import io
import struct

import numpy as np
from PIL import Image


def lzw_encode(raw, eoi=True, stats=None):
    """greedy TIFF 6.0 LZW as libtiff writes it; stats: a dict that receives the number of data codes and of Clear codes"""
    out = bytearray()
    acc = nb = 0
    ncodes = nclear = 0

    def put(code, width):
        nonlocal acc, nb
        acc = ((acc << width) | code) & 0xFFFFF
        nb += width
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 255)
            nb -= 8

    width, nxt, ent, table = 9, 258, -1, {}
    put(256, width)
    for c in raw:
        if ent < 0:
            ent = c
            continue
        found = table.get((ent << 8) | c)
        if found is not None:
            ent = found
            continue
        put(ent, width)
        ncodes += 1
        table[(ent << 8) | c] = nxt
        nxt += 1
        ent = c
        if nxt == 4094:
            put(256, width)
            nclear += 1
            table.clear()
            width, nxt = 9, 258
        elif nxt > (1 << width) - 1:
            width += 1
    if ent >= 0:
        put(ent, width)
        ncodes += 1
        nxt += 1
        if nxt == 4094:
            put(256, width)
            width = 9
        elif nxt > (1 << width) - 1:
            width += 1
    if eoi:
        put(257, width)
    if nb:
        out.append((acc << (8 - nb)) & 255)
    if stats is not None:
        stats.update(codes=ncodes, clears=nclear)
    return bytes(out)


def libtiff_strip(samples):
    """samples: uint8 / uint16 (rows, n) as they are to be stored (little endian) -> the LZW strip libtiff makes of them"""
    samples = np.ascontiguousarray(samples)
    assert samples.ndim == 2 and samples.nbytes <= 65536, samples.shape
    buf = io.BytesIO()
    Image.fromarray(samples).save(buf, "TIFF", compression="tiff_lzw")
    data = buf.getvalue()
    im = Image.open(io.BytesIO(data))
    offs, cnts = im.tag_v2[273], im.tag_v2[279]
    assert len(offs) == 1 and len(cnts) == 1
    return data[offs[0]:offs[0] + cnts[0]]


def libtiff_decode_strip(strip, rows, n, bits):
    """a strip re-wrapped as a one-strip (rows, n) gray file of ``bits`` bits, decoded by libtiff through Pillow -> (rows, n)"""
    entries = [(256, 4, 1, n), (257, 4, 1, rows), (258, 3, 1, bits), (259, 3, 1, 5), (262, 3, 1, 1), (273, 4, 1, 8), (277, 3, 1, 1),
               (278, 4, 1, rows), (279, 4, 1, len(strip)), (284, 3, 1, 1), (339, 3, 1, 1)]
    body = b"II*\0" + struct.pack("<I", 8 + len(strip) + (len(strip) & 1)) + strip + b"\0" * (len(strip) & 1)
    body += struct.pack("<H", len(entries)) + b"".join(struct.pack("<HHII", *e) for e in entries) + b"\0\0\0\0"
    return np.array(Image.open(io.BytesIO(body)))


def stored_rows(arr, predictor, big_endian):
    """arr (H,W,C) in the file's channel order -> (H, W C) samples as the strips hold them, read as little endian"""
    a = arr
    if predictor == 2:
        a = arr.copy()
        a[:, 1:] = arr[:, 1:] - arr[:, :-1]
    a = a.reshape(arr.shape[0], -1)
    return a.byteswap() if big_endian and a.dtype == np.uint16 else a


def container(H, W, C, bits, strips, rps, byte_order="II", compression=5, predictor=1, short_tables=False, extra=(), drop=(),
              magic=42):
    """the file around the strips.  extra: further or replacing IFD entries (tag, type, count, value); drop: tags left out"""
    e = "<" if byte_order == "II" else ">"
    out = bytearray(byte_order.encode() + struct.pack(e + "HI", magic, 0))
    offsets = []
    for s in strips:
        offsets.append(len(out))
        out += s + b"\0" * (len(s) & 1)
    n = len(strips)
    tab_t, tab_c = (3, "H") if short_tables else (4, "I")

    def array(values, code):
        at = len(out)
        out.extend(struct.pack(e + str(len(values)) + code, *values))
        out.extend(b"\0" * (len(out) & 1))
        return at

    def inline(values, code):
        return struct.unpack(e + "I", struct.pack(e + str(len(values)) + code, *values).ljust(4, b"\0"))[0]

    def ref(values, code):
        size = struct.calcsize(code) * len(values)
        return inline(values, code) if size <= 4 else array(values, code)

    entries = {256: (256, 4, 1, inline([W], "I")), 257: (257, 3, 1, inline([H], "H")),
               258: (258, 3, C, ref([bits] * C, "H")), 259: (259, 3, 1, inline([compression], "H")),
               262: (262, 3, 1, inline([1 if C == 1 else 2], "H")), 273: (273, tab_t, n, ref(offsets, tab_c)),
               277: (277, 3, 1, inline([C], "H")), 278: (278, 4, 1, inline([rps], "I")),
               279: (279, tab_t, n, ref([len(s) for s in strips], tab_c)), 284: (284, 3, 1, inline([1], "H"))}
    if predictor != 1:
        entries[317] = (317, 3, 1, inline([predictor], "H"))
    for tag, typ, count, value in extra:
        code = {1: "B", 3: "H", 4: "I"}.get(typ, "H")
        entries[tag] = (tag, typ, count, ref(list(value), code) if isinstance(value, (list, tuple)) else value)
    for tag in drop:
        entries.pop(tag, None)
    ifd = len(out)
    out += struct.pack(e + "H", len(entries))
    for tag in sorted(entries):
        out += struct.pack(e + "HHII", *entries[tag])
    out += b"\0\0\0\0"
    out[4:8] = struct.pack(e + "I", ifd)
    return bytes(out)


class Case:
    def __init__(self, name, arr, rps=None, byte_order="II", compression=5, predictor=1, short_tables=False, own_encoder=False,
                 eoi=True, junk=b""):
        """arr: uint8 / uint16 (H,W,C) in the file's channel order"""
        self.name, self.arr = name, np.ascontiguousarray(arr)
        H, W, C = arr.shape
        self.H, self.W, self.C, self.bits = H, W, C, 8 * arr.dtype.itemsize
        self.rps = H if rps is None else rps
        self.byte_order, self.compression, self.predictor = byte_order, compression, predictor
        # libtiff applies a predictor inside its LZW codec only: an uncompressed file is stored as it is, whatever tag 317 says
        rows = stored_rows(self.arr, predictor if compression == 5 else 1, byte_order == "MM")
        self.strips, self.stats = [], []
        for y in range(0, H, self.rps):
            part = np.ascontiguousarray(rows[y:y + self.rps])
            raw = part.astype("<u2" if self.bits == 16 else np.uint8).tobytes()
            st = {}
            own = lzw_encode(raw, eoi=eoi, stats=st)
            if compression == 1:
                strip = raw
            elif own_encoder or not eoi or len(raw) > 65536:
                strip = own
            else:
                strip = libtiff_strip(part)
                if st["clears"] == 0:
                    assert strip == own, f"{name}: the builder's encoder and libtiff disagree on a strip whose table did not fill"
            self.strips.append(strip + junk)
            self.stats.append(st)
        self.file = container(H, W, C, self.bits, self.strips, self.rps, byte_order, compression, predictor, short_tables)

    @property
    def fills(self):
        """whether a strip's dictionary filled (libtiff then clears by a rule of its own)"""
        return any(st["clears"] for st in self.stats)

    def expected(self, bgr):
        a = self.arr[:, :, ::-1] if bgr and self.C == 3 else self.arr
        return np.ascontiguousarray(a[:, :, 0] if self.C == 1 else a)

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------- contents
def uv_label(H, W, bits=16, C=3, seed=0):
    """a LabelMaker-like UV label in the file's order (v, u, id): few ids, u constant down columns, v constant along rows"""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    u = np.rint(np.linspace(1.0 / W, 1, W) * top).astype(np.int64)
    v = np.rint(np.linspace(1.0 / H, 1, H) * top).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    ids = ((xx * 3 // max(W, 1)) + (yy * 2 // max(H, 1)) + (rng.integers(0, 2))) % 4
    a = np.stack([np.broadcast_to(v[:, None], (H, W)), np.broadcast_to(u[None, :], (H, W)), ids], axis=2)
    a = a[:, :, :C] if C == 3 else a[:, :, 1:2]
    return a.astype(np.uint16 if bits == 16 else np.uint8)


def random_image(H, W, C, bits, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << bits, size=(H, W, C), dtype=np.uint16 if bits == 16 else np.uint8)


def ramp(H, W, C, bits=16):
    return (np.arange(H * W * C, dtype=np.int64) % (1 << bits)).astype(np.uint16 if bits == 16 else np.uint8).reshape(H, W, C)


TILE = 1024          # pixels of one tile of tiff_unpredict_kernel (csrc/tiffdec.hip: kThreads * kPixPerThread)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # every combination of depth, samples, byte order, predictor and compression on one small odd size with a short last strip
    for bits in (8, 16):
        for C in (1, 3):
            for bo in ("II", "MM"):
                for pred in (1, 2):
                    for comp in (1, 5):
                        arr = uv_label(37, 53, bits, C, seed=bits + C)
                        out.append(Case(f"combo_{bits}b_c{C}_{bo}_p{pred}_z{comp}", arr, rps=5, byte_order=bo, compression=comp,
                                        predictor=pred))
    # sizes and RowsPerStrip
    for (H, W), rps in (((1, 1), 1), ((1, 37), 1), ((9, 1), 2), ((37, 53), 1), ((12, 213), 5), ((45, 80), 2), ((45, 80), 45)):
        out.append(Case(f"size_{H}x{W}_rps{rps}", uv_label(H, W), rps=rps, predictor=2))
    out.append(Case("size_9x1_gray8", random_image(9, 1, 1, 8, 1), rps=9, predictor=2))
    # a row that crosses the unpredict kernel's tile, one pixel under and one over
    for W in (TILE - 1, TILE + 1):
        out.append(Case(f"tile_{W}", ramp(2, W, 3) * 7, rps=1, predictor=2))
        out.append(Case(f"tile_{W}_gray_MM", ramp(2, W, 1) * 5, rps=2, predictor=2, byte_order="MM"))
    # contents
    out.append(Case("zeros", np.zeros((12, 213, 3), np.uint16), rps=12, predictor=2))
    out.append(Case("zeros_8", np.zeros((45, 80, 1), np.uint8), rps=45))
    out.append(Case("ramp", ramp(45, 80, 3), rps=5, predictor=1))
    out.append(Case("ramp_p2_MM", ramp(45, 80, 3), rps=5, predictor=2, byte_order="MM"))
    rnd = Case("random_clear", random_image(4, 1400, 1, 16, 7), rps=4)
    assert rnd.fills, "4 x 1400 random uint16 must fill the dictionary"
    out.append(rnd)
    out.append(Case("random_p2_short_tables", random_image(12, 213, 3, 16, 8), rps=2, predictor=2, short_tables=True))
    # strips whose code count crosses a change of code width
    for edge in (511, 1023, 2047):
        data = random_image(1, 4096, 1, 8, edge)
        free = lambda n: 258 + Case("probe", data[:, :n], rps=1, own_encoder=True).stats[0]["codes"]   # the next free code at the end
        n = next(n for n in range(64, 4096, 8) if free(n) >= edge + 8)
        over, under = Case(f"codes_over_{edge}", data[:, :n], rps=1), Case(f"codes_under_{edge}", data[:, :n - 32], rps=1)
        assert free(n) >= edge + 8 > edge - 8 >= free(n - 32) and not over.fills, (edge, n, free(n), free(n - 32))
        out += [over, under]
    # a strip without EOI, a strip followed by junk inside its byte count
    out.append(Case("no_eoi", uv_label(12, 213), rps=5, predictor=2, eoi=False))
    out.append(Case("junk", uv_label(12, 213), rps=5, predictor=2, junk=b"\xAB\xCD\xEF\x01\x80"))
    # one strip above 64 KB decoded, from the builder's encoder
    out.append(Case("big_strip", uv_label(120, 100), rps=120, predictor=2, own_encoder=True))
    # the one full-size label: libtiff's default strips of 8 KB
    out.append(Case("full_360x640", uv_label(360, 640), rps=2, predictor=2))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def refusals():
    """one handcrafted file per refusal -> [(name, file bytes, reason code)]"""
    arr = uv_label(6, 5)
    c = Case("base", arr, rps=4, predictor=2)
    H, W, C = arr.shape
    mk = lambda **kw: container(H, W, C, 16, c.strips, 4, "II", 5, 2, **kw)
    out = [("truncated", c.file[:6], 1), ("not_tiff", b"\x89PNG\r\n\x1a\n" + c.file[8:], 2),
           ("bad_magic", c.file[:2] + b"\x2b\x01" + c.file[4:], 2),
           ("ifd_outside", c.file[:4] + struct.pack("<I", len(c.file) - 1) + c.file[8:], 3),
           ("tag_array_outside", mk(extra=[(258, 3, 3, len(c.file) + 4096)]), 4),
           ("tag_type", mk(extra=[(259, 5, 1, 5)]), 4),
           ("strip_outside", mk(extra=[(279, 4, 2, [len(c.strips[0]), 1 << 20])]), 5),
           ("strip_table", mk(extra=[(278, 4, 1, 2)]), 6),
           ("missing_tag", mk(drop=[257]), 7),
           ("zero_width", mk(extra=[(256, 4, 1, 0)]), 8),
           ("bigtiff", mk(magic=43), 100),
           ("tiles", mk(extra=[(322, 3, 1, 16), (323, 3, 1, 16)]), 101),
           ("planar", mk(extra=[(284, 3, 1, 2)]), 102),
           ("fill_order", mk(extra=[(266, 3, 1, 2)]), 103),
           ("deflate", mk(extra=[(259, 3, 1, 8)]), 104),
           ("packbits", mk(extra=[(259, 3, 1, 32773)]), 104),
           ("predictor3", mk(extra=[(317, 3, 1, 3)]), 105),
           ("bits_32", mk(extra=[(258, 3, 3, [32, 32, 32])]), 106),
           ("float", mk(extra=[(339, 3, 3, [3, 3, 3])]), 107),
           ("four_samples", mk(extra=[(277, 3, 1, 4), (258, 3, 4, [16] * 4)]), 108),
           ("palette", mk(extra=[(262, 3, 1, 3)]), 109),
           ("old_lzw", container(H, W, C, 16, [b"\x00\x01" + c.strips[0][2:], c.strips[1]], 4, "II", 5, 2), 110)]
    return out
