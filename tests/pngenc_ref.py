"""The PNG format rule of sfh_amd.pngenc / csrc/pngenc.hip, restated once in numpy.  The GPU encoder must give these
bytes exactly.

A file is: signature, IHDR (8-bit, colour type 0 or 2, non-interlaced), one IDAT chunk per STRIP, IEND.

* Filtered stream: H rows of ``1 + W*C`` bytes, filter byte 1 (Sub, bpp = C) first.  3-channel images are RGB in the file;
  ``bgr=True`` (the default, cv2's convention) reverses the channels of the array first.
* Strips: ``R = max(1, min(16, 32768 // (1 + W*C)))`` rows each (the last one may be shorter); a row longer than 32768 bytes
  is refused.
* A strip is ONE deflate block.  Fixed-Huffman form (BTYPE 01): the strip's bytes are cut into maximal runs of equal bytes
  (a run may cross row ends, never a strip end).  A run of L bytes gives: its first byte as a literal; then, with n = L - 1
  bytes left, ``while n >= 3: emit match(length min(n, 258), distance 1); n -= min(n, 258)``; then the n (0, 1 or 2) bytes
  left as literals.  End-of-block follows.  A strip that is not the last then gets an empty stored block (bits 000, zero
  bits to the next byte boundary, 00 00 FF FF), so that every strip ends on a byte; the last strip has BFINAL = 1 and is
  padded with zero bits to a byte.
* Stored form: if those bytes number more than ``len(strip) + 5``, the strip is instead one stored block: the byte BFINAL,
  LEN and ~LEN little endian, the strip's bytes.
* Chunks: the first IDAT's data starts with 78 01, the last one's ends with the Adler-32 of the whole filtered stream.
"""
import struct
import zlib

import numpy as np

MAX_ROW = 32768
MAX_STRIP_ROWS = 16
SIG = b"\x89PNG\r\n\x1a\n"


def strip_rows(W, C):
    return max(1, min(MAX_STRIP_ROWS, MAX_ROW // (1 + W * C)))


def ref_capacity(H, W, C):
    """upper bound of the file size: signature, IHDR, per strip 12 (chunk) + 5 (stored header) + its bytes, zlib header and
    Adler-32, IEND"""
    row = 1 + W * C
    if C not in (1, 3) or H < 1 or W < 1 or row > MAX_ROW:
        raise ValueError(f"ref_capacity: H {H} W {W} C {C}")
    strips = -(-H // strip_rows(W, C))
    return 8 + 25 + strips * 17 + H * row + 2 + 4 + 12


def filtered_stream(img, bgr=True):
    """(H,W) or (H,W,3) uint8 -> (H, 1 + W*C) uint8: Sub-filtered scanlines, filter byte included"""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"dtype {a.dtype}: uint8 only")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"shape {a.shape}: (H,W) or (H,W,3)")
    if a.shape[2] == 3 and bgr:
        a = a[:, :, ::-1]
    H, W, C = a.shape
    if 1 + W * C > MAX_ROW:
        raise ValueError(f"row of {1 + W * C} bytes: at most {MAX_ROW}")
    px = a.astype(np.int16)
    sub = px.copy()
    sub[:, 1:] -= px[:, :-1]
    rows = (sub & 255).astype(np.uint8).reshape(H, W * C)
    return np.concatenate([np.ones((H, 1), np.uint8), rows], axis=1)


def _rev(v, n):
    return int(format(v, f"0{n}b")[::-1], 2)


def _literal(v):
    """-> (bits LSB first as an integer, number of bits): Huffman codes go into the stream most significant bit first"""
    return (_rev(0x30 + v, 8), 8) if v < 144 else (_rev(0x190 + v - 144, 9), 9)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def _match(length):
    """length 3..258 at distance 1: length symbol, its extra bits, the 5-bit distance code 0"""
    k = max(i for i in range(29) if _LEN_BASE[i] <= length)
    sym, eb = 257 + k, _LEN_EXTRA[k]
    code, n = (_rev(sym - 256, 7), 7) if sym < 280 else (_rev(0xC0 + sym - 280, 8), 8)
    code |= (length - _LEN_BASE[k]) << n
    return code, n + eb + 5


_LIT = [_literal(v) for v in range(256)]
_MATCH = {n: _match(n) for n in range(3, 259)}


def strip_tokens(data):
    """the token list of one strip: ("lit", value) and ("match", length)"""
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    ends = np.concatenate([starts[1:], [d.size]])
    toks = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v = int(d[s])
        toks.append(("lit", v))
        n = e - s - 1
        while n >= 3:
            m = min(n, 258)
            toks.append(("match", m))
            n -= m
        toks.extend([("lit", v)] * n)
    return toks


def _fixed_block(data, final):
    acc, nbits = (1 if final else 0) | (1 << 1), 3
    for kind, v in strip_tokens(data):
        code, n = _LIT[v] if kind == "lit" else _MATCH[v]
        acc |= code << nbits
        nbits += n
    nbits += 7                                      # end of block: seven zero bits
    if not final:
        nbits += 3                                  # empty stored block: BFINAL 0, BTYPE 00
    nbytes = (nbits + 7) // 8
    out = acc.to_bytes(nbytes, "little")
    return out if final else out + b"\x00\x00\xff\xff"


def strip_block(data, final):
    """-> (deflate bytes of the strip, "fixed" | "stored")"""
    raw = bytes(np.asarray(data, dtype=np.uint8))
    fixed = _fixed_block(raw, final)
    if len(fixed) > len(raw) + 5:
        n = len(raw)
        return bytes([1 if final else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + raw, "stored"
    return fixed, "fixed"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def ref_encode_parts(img, bgr=True):
    """-> (file bytes, [branch of every strip])"""
    stream = filtered_stream(img, bgr)
    H, row = stream.shape
    C = 1 if np.asarray(img).ndim == 2 else 3
    W = (row - 1) // C
    R = strip_rows(W, C)
    nstrips = -(-H // R)
    out = [SIG, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if C == 1 else 2, 0, 0, 0))]
    kinds = []
    for s in range(nstrips):
        body, kind = strip_block(stream[s * R:(s + 1) * R].reshape(-1), s == nstrips - 1)
        kinds.append(kind)
        if s == 0:
            body = b"\x78\x01" + body
        if s == nstrips - 1:
            body += struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)
        out.append(_chunk(b"IDAT", body))
    out.append(_chunk(b"IEND", b""))
    return b"".join(out), kinds


def ref_encode(img, bgr=True):
    return ref_encode_parts(img, bgr)[0]
