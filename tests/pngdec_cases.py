"""The PNG files sfh_amd.pngdec is tested on, built with nothing but zlib, struct and numpy (the project's and PIL's own files
are added by the tests that have them): a writer that takes a filter type per row, a zlib.compressobj recipe, flush points and
IDAT cut points; a bit writer for hand-made stored, fixed and dynamic blocks; and the corruptions of the host test.

``cases()`` -> {name: Case(data, segmented)}: ``segmented`` is what PngDecoder.segmented() must say for the file.  The expected
pixels are ``outputs.decode_png(data)`` (zlib's inflate), which tests/test_pngdec_host.py holds to PIL's."""
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
SHAPES = ((1, 1), (1, 7), (7, 1), (5, 3), (64, 5), (65, 5), (129, 9), (3, 700), (1, 5000), (37, 50), (333, 187))
CTYPE = {1: 0, 3: 2, 4: 6}
Case = namedtuple("Case", "data segmented")


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def ihdr(H, W, C, depth=8, ctype=None, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, CTYPE[C] if ctype is None else ctype, 0, 0, interlace))


def wrap(H, W, C, stream, cuts=(), extra=()):
    """the zlib stream of an H x W x C image -> a file; cuts: positions of the stream where a new IDAT chunk starts; extra:
    ancillary chunks (tag, body) before the first IDAT"""
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(stream))) + [len(stream)]
    idat = b"".join(chunk(b"IDAT", stream[a:b]) for a, b in zip(edges[:-1], edges[1:]))
    return SIG + ihdr(H, W, C) + b"".join(chunk(t, b) for t, b in extra) + idat + chunk(b"IEND", b"")


def filter_rows(img, filters):
    """img (H,W,C) uint8 in the file's channel order, a filter type per row -> the filtered stream (H, 1 + W*C)"""
    H, W, C = img.shape
    cur = img.reshape(H, W * C).astype(np.int32)
    up = np.vstack([np.zeros((1, W * C), np.int32), cur[:-1]])
    left = np.hstack([np.zeros((H, C), np.int32), cur[:, :-C]]) if W * C > C else np.zeros_like(cur)
    upleft = np.hstack([np.zeros((H, C), np.int32), up[:, :-C]]) if W * C > C else np.zeros_like(cur)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    pred = [np.zeros_like(cur), left, up, (left + up) >> 1, paeth]
    f = np.asarray(filters, dtype=np.int64)
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = f
    for y in range(H):
        out[y, 1:] = (cur[y] - pred[f[y]][y]) & 255
    return out


def deflate_rows(rows, recipe=None, flushes=None):
    """the filtered stream -> (zlib stream, [position of the stream behind every flush]); recipe: the arguments of
    zlib.compressobj; flushes: {row: zlib.Z_SYNC_FLUSH | zlib.Z_FULL_FLUSH} - flushed before that row"""
    co = zlib.compressobj(*(recipe or (6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY)))
    out, marks = b"", []
    for y in range(rows.shape[0]):
        if flushes and y in flushes:
            out += co.flush(flushes[y])
            marks.append(len(out))
        out += co.compress(rows[y].tobytes())
    return out + co.flush(), marks


def write_png(img, filters, recipe=None, flushes=None, cuts=(), cut_at_flushes=False, extra=()):
    img = np.asarray(img)
    img = img[:, :, None] if img.ndim == 2 else img
    H, W, C = img.shape
    stream, marks = deflate_rows(filter_rows(img, filters), recipe, flushes)
    return wrap(H, W, C, stream, list(cuts) + (marks if cut_at_flushes else []), extra)


# ------------------------------------------------------------------------------------------------------------ images and patterns

def labels(rng, H, W, C):
    """label-map-like: rectangles of few values, so that a deflater finds matches"""
    a = np.zeros((H, W, C), np.uint8)
    for _ in range(10):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        a[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = rng.integers(0, 256, C)
    return a


def noise(rng, H, W, C):
    return rng.integers(0, 256, (H, W, C), dtype=np.uint8)


def pattern(name, H):
    if name.startswith("all"):
        return [int(name[3])] * H
    if name == "cycle":
        return [y % 5 for y in range(H)]
    if name == "zero_one":
        return [(y * 7 // 3) & 1 for y in range(H)]
    if name == "one_paeth":
        return [4 if y == H // 2 else y & 1 for y in range(H)]
    raise KeyError(name)


PATTERNS = ("all0", "all1", "all2", "all3", "all4", "cycle", "zero_one", "one_paeth")
ROWS_KERNEL = ("all0", "all1", "zero_one")        # the patterns of None / Sub rows only (one_paeth with H == 1 has none either)
RECIPES = {"stored": (0, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED),
           "dynamic": (6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY), "small_blocks": (6, zlib.DEFLATED, 15, 1, zlib.Z_DEFAULT_STRATEGY),
           "window512": (9, zlib.DEFLATED, 9, 8, zlib.Z_DEFAULT_STRATEGY)}


# ------------------------------------------------------------------------------------------------------------ hand-made blocks

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Bits:
    """deflate's bit order: values least significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.put(int(format(c, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        assert self.n == 0
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)}"""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, v in enumerate(lens):
            if v == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


def len_symbol(length, k=None):
    """-> (symbol index 0..28, extra value); k: force that symbol (258 is 284 + 31 as well as 285)"""
    if k is None:
        k = max(i for i in range(29) if LEN_BASE[i] <= length)
    return k, length - LEN_BASE[k]


def put_tokens(bw, tokens, lit, dist):
    """tokens: int (a literal) or (length, distance[, length symbol index]); then the end-of-block code"""
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            bw.code(*lit[int(t)])
            continue
        k, ev = len_symbol(t[0], t[2] if len(t) > 2 else None)
        bw.code(*lit[257 + k])
        bw.put(ev, LEN_EXTRA[k])
        d = max(i for i in range(30) if DIST_BASE[i] <= t[1])
        bw.code(*dist[d])
        bw.put(t[1] - DIST_BASE[d], DIST_EXTRA[d])
    bw.code(*lit[256])


def fixed_block(bw, tokens, final):
    bw.put((1 if final else 0) | 2, 3)
    put_tokens(bw, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def stored_block(bw, data, final):
    bw.put(1 if final else 0, 3)
    bw.align()
    bw.put(len(data), 16)
    bw.put(len(data) ^ 0xFFFF, 16)
    bw.out += bytes(data)


def dynamic_block(bw, tokens, lit_lens, dist_lens, final):
    """every code length written with a 4-bit code (code-length code: 0 .. 15 at 4 bits each, no repeats)"""
    bw.put((1 if final else 0) | 4, 3)
    bw.put(len(lit_lens) - 257, 5)
    bw.put(len(dist_lens) - 1, 5)
    bw.put(19 - 4, 4)
    cl = [4] * 16 + [0] * 3
    for s in CL_ORDER:
        bw.put(cl[s], 3)
    clc = canonical(cl)
    for v in list(lit_lens) + list(dist_lens):
        bw.code(*clc[v])
    put_tokens(bw, tokens, canonical(lit_lens), canonical(dist_lens))


def detokenize(tokens, out):
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            out.append(int(t))
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return out


def zwrap(deflate, raw):
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(bytes(raw)) & 0xFFFFFFFF)


def one_row_file(deflate, raw, cuts=()):
    """a hand-made deflate stream whose output `raw` starts with a 0 (filter None) -> a 1 x (len - 1) gray image"""
    assert raw[0] == 0 and zlib.decompress(zwrap(deflate, raw)) == bytes(raw)
    return wrap(1, len(raw) - 1, 1, zwrap(deflate, raw), cuts)


# lengths of a complete literal / length code over all 286 symbols with codes of 15 bits, and of a distance code over all 30
FULL_LIT = [14] * 286
for _s, _l in zip((0, 256, 65, 257, 285, 32), (1, 2, 3, 4, 5, 6)):
    FULL_LIT[_s] = _l
for _s in range(200, 248):
    FULL_LIT[_s] = 15
FULL_DIST = [4, 4] + [5] * 28


def handmade():
    rng = np.random.default_rng(20261018)
    c = {}
    # runs of equal bytes and matches with dist < len, fixed blocks
    toks = [0]
    for k, n in enumerate((2, 3, 258, 259, 517)):
        v = 10 + k
        toks.append(v)
        left = n - 1
        while left >= 3:
            m = min(left, 258)
            m = m - 1 if left - m in (1, 2) and m > 3 else m
            toks.append((m, 1))
            left -= m
        toks += [v] * left + [99]
    for d in (1, 2, 3, 63, 64, 65):
        toks += [int(v) for v in rng.integers(100, 256, d)] + [(d + 7, d), (258, d), (3, d)]
    raw = detokenize(toks, [])
    bw = Bits()
    fixed_block(bw, toks, True)
    bw.align()
    c["hand_runs_and_overlaps"] = Case(one_row_file(bw.bytes(), raw), False)
    # a match at distance 32768, matches that wrap the ring (the output passes 49152 and 98304), an empty stored block, stored
    # blocks of 65535 + 1 bytes
    toks = [0] + [int(v) for v in rng.integers(0, 256, 32767)] + [(258, 32768), (200, 32768), 7, (3, 32768)]
    raw = detokenize(toks, [])
    bw = Bits()
    fixed_block(bw, toks, False)
    stored_block(bw, b"", False)
    tail = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    stored_block(bw, tail[:65535], False)
    stored_block(bw, tail[65535:], False)
    raw = raw + list(tail)
    toks2 = [(258, 32768), (258, 30000), 5, (100, 49152 - 16640)] + [(258, 32768)] * 70
    raw = detokenize(toks2, raw)
    fixed_block(bw, toks2, True)
    bw.align()
    c["hand_far_matches_and_stored"] = Case(one_row_file(bw.bytes(), raw), False)
    # all 286 symbols, all 30 distance codes, codes of 15 bits; 258 both as 285 and as 284 + 31
    toks = [0] + [int(v) for v in rng.integers(0, 256, 24600)] + list(range(256))
    for k in range(29):
        toks.append((LEN_BASE[k] + (1 << LEN_EXTRA[k]) - 1 if k < 28 else 258, 1 + k, k))
    toks.append((258, 5, 27))
    for d in range(30):
        toks.append((3 + d, DIST_BASE[d] + (1 << DIST_EXTRA[d]) - 1 if d < 29 else 24700))
    raw = detokenize(toks, [])
    bw = Bits()
    dynamic_block(bw, toks, FULL_LIT, FULL_DIST, True)
    bw.align()
    deflate = bw.bytes()
    c["hand_all_symbols"] = Case(one_row_file(deflate, raw), False)
    # a stored block and a dynamic header each cut by an IDAT boundary (and at every byte near them)
    bw = Bits()
    stored_block(bw, bytes(raw[:300]), False)
    mark = len(bw.out)
    dynamic_block(bw, toks[300:], FULL_LIT, FULL_DIST, True)
    bw.align()
    cuts = [2 + 3, 2 + 150] + [2 + mark + k for k in (1, 2, 3, 60, 61, 150)]
    c["hand_cut_stored_and_header"] = Case(one_row_file(bw.bytes(), raw, cuts), False)
    return c


# ------------------------------------------------------------------------------------------------------------ the list

@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261018)
    c = {}
    # every shape, the channels and patterns cycling, label-like content (matches) in dynamic blocks
    for k, (H, W) in enumerate(SHAPES):
        for j in range(3):
            C, pat = (1, 3, 4)[(k + j) % 3], PATTERNS[(3 * k + 5 * j) % len(PATTERNS)]
            c[f"shape_{H}x{W}x{C}_{pat}"] = Case(write_png(labels(rng, H, W, C), pattern(pat, H)), False)
    # every pattern with every channel count on one shape with two bands; noise, so that a wrong neighbour shows
    for C in (1, 3, 4):
        for pat in PATTERNS:
            c[f"pattern_65x5x{C}_{pat}"] = Case(write_png(noise(rng, 65, 5, C), pattern(pat, 65)), False)
            c[f"pattern_37x50x{C}_{pat}"] = Case(write_png(noise(rng, 37, 50, C), pattern(pat, 37)), False)
    # the scan carry of the rows kernel and the second band of the skew kernel on wide and tall images
    c["wide_1x5000x3_all1"] = Case(write_png(noise(rng, 1, 5000, 3), pattern("all1", 1)), False)
    c["wide_3x700x4_all1"] = Case(write_png(noise(rng, 3, 700, 4), pattern("all1", 3)), False)
    c["tall_333x187x1_cycle"] = Case(write_png(noise(rng, 333, 187, 1), pattern("cycle", 333)), False)
    # the block types
    for name, recipe in RECIPES.items():
        c[f"recipe_{name}_333x187x3"] = Case(write_png(labels(rng, 333, 187, 3), pattern("cycle", 333), recipe), False)
        c[f"recipe_{name}_37x50x1"] = Case(write_png(labels(rng, 37, 50, 1), pattern("zero_one", 37), recipe), False)
    # a block per 127 symbols: several hundred dynamic blocks
    c["recipe_small_blocks_noisy_333x187x1"] = Case(write_png(rng.integers(0, 4, (333, 187, 1), dtype=np.uint8) * 60, pattern("cycle", 333),
                                                              RECIPES["small_blocks"]), False)
    c["recipe_stored_noise_333x187x4"] = Case(write_png(noise(rng, 333, 187, 4), pattern("all4", 333), RECIPES["stored"]), False)
    # IDAT chunks of 1 byte; arbitrary cuts; ancillary chunks
    img = labels(rng, 37, 50, 3)
    stream, _ = deflate_rows(filter_rows(img, pattern("cycle", 37)))
    many, _ = deflate_rows(filter_rows(noise(rng, 37, 50, 3), pattern("one_paeth", 37)))
    c["idat_one_byte_chunks"] = Case(wrap(37, 50, 3, many, range(1, len(many))), False)   # more than the segmented leg takes
    c["idat_one_byte_chunks_few"] = Case(wrap(37, 50, 3, stream, range(1, len(stream))), False)
    c["idat_arbitrary_cuts"] = Case(wrap(37, 50, 3, stream, (1, 2, 3, len(stream) // 2, len(stream) - 5, len(stream) - 4, len(stream) - 1)), False)
    c["idat_empty_chunk_and_ancillary"] = Case(
        SIG + ihdr(37, 50, 3) + chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"tEXt", b"Comment\0pngdec") + chunk(b"IDAT", b"") +
        chunk(b"IDAT", stream[:40]) + chunk(b"IDAT", b"") + chunk(b"IDAT", stream[40:]) + chunk(b"tIME", b"\x07\xea\x0a\x12\0\0\0") +
        chunk(b"IEND", b""), False)
    # flush points: a full flush resets the window, so the chunks are independent; a sync flush does not, and repeating rows
    # make matches cross it
    rows = np.repeat(noise(rng, 1, 9, 3), 129, axis=0)
    rows[::7] = noise(rng, len(rows[::7]), 9, 3)
    for H, fl, name, seg in ((129, zlib.Z_FULL_FLUSH, "full", True), (129, zlib.Z_SYNC_FLUSH, "sync", False)):
        for pat in ("all1", "cycle"):
            c[f"flush_{name}_129x9x3_{pat}"] = Case(write_png(rows, pattern(pat, 129), flushes={40: fl, 41: fl, 100: fl}, cut_at_flushes=True), seg)
    c["flush_full_small_blocks_333x187x1"] = Case(write_png(labels(rng, 333, 187, 1), pattern("zero_one", 333), RECIPES["small_blocks"],
                                                              flushes={y: zlib.Z_FULL_FLUSH for y in range(16, 333, 16)}, cut_at_flushes=True), True)
    # a full flush whose chunks are cut one byte late: no chunk starts on a block boundary
    stream, marks = deflate_rows(filter_rows(rows, pattern("all1", 129)), flushes={40: zlib.Z_FULL_FLUSH, 100: zlib.Z_FULL_FLUSH})
    c["flush_full_cut_one_late"] = Case(wrap(129, 9, 3, stream, [m + 1 for m in marks]), False)
    # the small files the host test corrupts: one block type each
    small = rng.integers(0, 4, (20, 20, 1), dtype=np.uint8) * 60
    c["corrupt_dynamic_20x20x1"] = Case(write_png(small, pattern("cycle", 20), RECIPES["window512"]), False)
    c["corrupt_fixed_7x9x3"] = Case(write_png(labels(rng, 7, 9, 3), pattern("cycle", 7), RECIPES["fixed"]), False)
    c["corrupt_stored_7x9x3"] = Case(write_png(noise(rng, 7, 9, 3), pattern("cycle", 7), RECIPES["stored"]), False)
    assert [(joined_idat(c[n].data)[2] >> 1) & 3 for n in ("corrupt_dynamic_20x20x1", "corrupt_fixed_7x9x3", "corrupt_stored_7x9x3")] == [2, 1, 0]
    c.update(handmade())
    return c


def expected_filtered(data):
    """the filtered stream of a file, by zlib"""
    pos, idat = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            idat.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return zlib.decompress(b"".join(idat))


def rewrap(data, stream):
    """the file with its joined IDAT bodies replaced by `stream` (one chunk, CRC right)"""
    i = data.index(b"IDAT") - 4
    j = data.rindex(b"IEND") - 4
    return data[:i] + chunk(b"IDAT", stream) + data[j:]


def joined_idat(data):
    pos, idat = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            idat.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return b"".join(idat)


# ------------------------------------------------------------------------------------------------------------ other writers' files

FIXTURES = ("mask_ncaa_v4_nc4_m_onehot.png", "pitch_mask_v3_nc4_hd.png", "template_ncaa_v4_s.png")


def fixture(name):
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png", name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def writer_files():
    """files of the project's own writers and of PIL (the imports are theirs): the restatement of sfh_amd.pngenc with fixed and
    stored strips alternating, outputs.encode_png, PIL at compress_level 0, 1, 6 and optimize=True"""
    import io
    import pngenc_ref
    from PIL import Image
    from sfh_amd.outputs import encode_png
    rng = np.random.default_rng(20261019)
    c = {}
    for C in (1, 3):
        H, W = 80 + 5, 50
        img = np.zeros((H, W, C), np.uint8)
        for s in range(0, H, 2 * pngenc_ref.strip_rows(W, C)):
            img[s:s + pngenc_ref.strip_rows(W, C)] = noise(rng, min(pngenc_ref.strip_rows(W, C), H - s), W, C)
        img = img[:, :, 0] if C == 1 else img
        data, branches = pngenc_ref.ref_encode_parts(img)
        assert branches[:4] == ["stored", "fixed", "stored", "fixed"] and len(branches) == 6
        c[f"pngenc_ref_85x50x{C}"] = Case(bytes(data), True)
    c["pngenc_ref_one_strip_9x31x1"] = Case(bytes(pngenc_ref.ref_encode(labels(rng, 9, 31, 1)[:, :, 0])), False)
    c["pngenc_ref_labels_333x187x3"] = Case(bytes(pngenc_ref.ref_encode(labels(rng, 333, 187, 3))), True)
    for C in (1, 3):
        img = labels(rng, 129, 70, C)
        c[f"encode_png_129x70x{C}"] = Case(bytes(encode_png(img[:, :, 0] if C == 1 else img)), False)
    photo = (np.add.outer(np.arange(120), np.arange(200))[:, :, None] * np.array([1, 2, 3]) // 3 + rng.integers(0, 6, (120, 200, 3))).astype(np.uint8)
    for name, kw in (("level0", {"compress_level": 0}), ("level1", {"compress_level": 1}), ("level6", {"compress_level": 6}),
                     ("optimize", {"optimize": True})):
        for tag, arr in (("photo_120x200x3", photo), ("labels_90x64x1", labels(rng, 90, 64, 1)[:, :, 0]),
                         ("labels_33x20x4", labels(rng, 33, 20, 4))):
            buf = io.BytesIO()
            Image.fromarray(arr).save(buf, "PNG", **kw)
            c[f"pil_{name}_{tag}"] = Case(buf.getvalue(), False)
    return c


def all_files():
    """every well-formed file of the tests: {name: Case}"""
    c = dict(cases())
    c.update(writer_files())
    c.update({f"fixture_{n}": Case(fixture(n), False) for n in FIXTURES})
    return c
