"""The JPEG format rule of sfh_amd.jpegenc, restated in numpy with integers only (csrc/jpegenc.hip must equal it byte for
byte; tests/test_jpegenc_host.py holds it to libjpeg's bytes through PIL).

The rule is libjpeg's baseline encoder with a restart interval of one MCU row: JFIF header, Annex K quantisation tables scaled
by libjpeg's quality rule, 16-bit fixed-point RGB -> YCbCr, 4:2:0 by h2v2 downsampling with the alternating bias, the
"islow" integer forward DCT, rounded division by 8 Q, zig-zag, the Annex K Huffman tables, byte stuffing, 1-padding before
every RSTm and before EOI.

Edges, as libjpeg does them: the input's right edge is replicated sample by sample BEFORE downsampling; the bottom row is
replicated up to an even height before downsampling and every COMPONENT's last row after it.  A block of an MCU that lies
wholly beyond the component's ceil(size / 8) blocks is a dummy: all AC zero, DC that of the block before it in the MCU, so it
codes as difference 0 and EOB.
"""
import numpy as np

MAX_WIDTH = 2048
BLOCK_MAX_BITS = 22 + 63 * 26       # DC: 11-bit code + 11 bits; every AC: 16-bit code + 10 bits (no EOB, no ZRL then)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])   # zig-zag position -> natural (row-major) index

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a4344"
    "45464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4"
    "b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def _derive(bits, vals):
    """symbol -> (code, length): the canonical codes of a DHT segment"""
    tab, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            tab[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return tab


HUFF = {("dc", 0): _derive(DC_LUMA_BITS, DC_VALS), ("ac", 0): _derive(AC_LUMA_BITS, AC_LUMA_VALS),
        ("dc", 1): _derive(DC_CHROMA_BITS, DC_VALS), ("ac", 1): _derive(AC_CHROMA_BITS, AC_CHROMA_VALS)}


def quant_table(base, quality):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): natural order"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} (1 .. 100)")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base.astype(np.int64) * s + 50) // 100, 1, 255)


def _check(img):
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"dtype {a.dtype} (uint8 only)")
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"shape {a.shape} ((H,W) or (H,W,3))")
    if a.shape[1] > MAX_WIDTH:
        raise ValueError(f"width {a.shape[1]} (at most {MAX_WIDTH})")
    return a


def geometry(H, W, C):
    """-> (MCU rows, MCUs per row, blocks per MCU)"""
    m = 16 if C == 3 else 8
    return -(-H // m), -(-W // m), 6 if C == 3 else 1


def ref_capacity(H, W, C):
    """the closed-form bound of csrc/jpegenc.hip: header + per interval twice (stuffing) the bytes of blocks * BLOCK_MAX_BITS,
    + the 2-byte marker"""
    if C not in (1, 3) or H < 1 or W < 1 or W > MAX_WIDTH or H > 65535:
        raise ValueError(f"image {W}x{H}x{C}")
    rows, mcus, per = geometry(H, W, C)
    return header_bytes(C) + rows * (2 * ((mcus * per * BLOCK_MAX_BITS + 7) // 8) + 2)


def header_bytes(C):
    return 2 + 18 + 69 + (19 if C == 3 else 13) + 33 + 183 + 6 + (14 if C == 3 else 10) + (69 + 33 + 183 if C == 3 else 0)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(H, W, C, quality):
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].astype(np.uint8)))
    if C == 3:
        out += _seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].astype(np.uint8)))
    comps = [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] if C == 3 else [(1, 0x11, 0)]
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(comps)])
                + b"".join(bytes(c) for c in comps))
    out += _seg(0xC4, bytes([0x00] + DC_LUMA_BITS + DC_VALS)) + _seg(0xC4, bytes([0x10] + AC_LUMA_BITS + AC_LUMA_VALS))
    if C == 3:
        out += _seg(0xC4, bytes([0x01] + DC_CHROMA_BITS + DC_VALS)) + _seg(0xC4, bytes([0x11] + AC_CHROMA_BITS + AC_CHROMA_VALS))
    out += _seg(0xDD, geometry(H, W, C)[1].to_bytes(2, "big"))
    out += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], c[2] * 0x11]) for c in comps) + bytes([0, 63, 0]))
    assert len(out) == header_bytes(C)
    return out


def ycc_planes(img, bgr=True):
    """-> [Y] or [Y, Cb, Cr] as int64 planes padded to whole MCUs (Y: 16 * MCUs, chroma: 8 * MCUs; gray: 8 * blocks)"""
    a = _check(img).astype(np.int64)
    H, W = a.shape[:2]
    if a.ndim == 2:
        Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
        return [np.pad(a, ((0, Hp - H), (0, Wp - W)), mode="edge")]
    r, g, b = (a[:, :, 2], a[:, :, 1], a[:, :, 0]) if bgr else (a[:, :, 0], a[:, :, 1], a[:, :, 2])
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    out = [np.pad(y, ((0, Hp - H), (0, Wp - W)), mode="edge")]
    He = H + (H & 1)
    bias = np.tile(np.array([1, 2]), Wp // 4 + 1)[:Wp // 2]
    for c in (cb, cr):
        f = np.pad(c, ((0, He - H), (0, Wp - W)), mode="edge")       # full resolution: right edge, one row to an even height
        d = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + bias) >> 2
        out.append(np.pad(d, ((0, Hp // 2 - He // 2), (0, 0)), mode="edge"))     # the COMPONENT's last row
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """jfdctint.c's pass over the last axis of d (.., 8)"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def quantised_blocks(plane, qtab):
    """plane (8 bh, 8 bw) -> (bh, bw, 64) quantised coefficients in zig-zag order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128          # (bh, bw, row, col)
    d = _dct_pass(d, True)                                               # rows
    d = _dct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    c = d.reshape(bh, bw, 64)
    div = (qtab.astype(np.int64) * 8)[None, None, :]
    mag = (np.abs(c) + (div >> 1)) // div
    return (np.sign(c) * mag)[:, :, ZIGZAG]


def _category(v):
    return int(abs(int(v))).bit_length()


def block_bits(zz, pred, table, out):
    """appends the bit strings of one block (zig-zag coefficients zz, DC prediction pred) to the list out"""
    dc, ac = HUFF[("dc", table)], HUFF[("ac", table)]
    diff = int(zz[0]) - pred
    n = _category(diff)
    code, ln = dc[n]
    out.append(format(code, f"0{ln}b"))
    if n:
        out.append(format((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), f"0{n}b"))
    last = 0
    for k in np.flatnonzero(zz[1:]) + 1:
        run = int(k) - last - 1
        while run > 15:
            code, ln = ac[0xF0]
            out.append(format(code, f"0{ln}b"))
            run -= 16
        v = int(zz[k])
        n = _category(v)
        code, ln = ac[(run << 4) | n]
        out.append(format(code, f"0{ln}b"))
        out.append(format((v if v >= 0 else v - 1) & ((1 << n) - 1), f"0{n}b"))
        last = int(k)
    if last < 63:
        code, ln = ac[0x00]
        out.append(format(code, f"0{ln}b"))


def interval_bits(img, quality=90, bgr=True):
    """-> per MCU row the list of bit strings, one entry per block's codes joined (the unit the device kernel scans)"""
    a = _check(img)
    H, W = a.shape[:2]
    C = 1 if a.ndim == 2 else 3
    rows, mcus, _ = geometry(H, W, C)
    planes = ycc_planes(a, bgr)
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    coef = [quantised_blocks(p, ql if i == 0 else qc) for i, p in enumerate(planes)]
    ybw, ybh = -(-W // 8), -(-H // 8)                                    # real Y blocks
    out = []
    for r in range(rows):
        pred = [0, 0, 0]
        blocks = []
        for m in range(mcus):
            if C == 1:
                order = [(0, r, m)]
            else:
                order = [(0, 2 * r + k // 2, 2 * m + k % 2) for k in range(4)] + [(1, r, m), (2, r, m)]
            for comp, by, bx in order:
                bits = []
                if comp == 0 and (bx >= ybw or by >= ybh):               # dummy: DC of the block before it, no AC
                    zz = np.zeros(64, np.int64)
                    zz[0] = pred[0]
                else:
                    zz = coef[comp][by, bx]
                block_bits(zz, pred[comp], 0 if comp == 0 else 1, bits)
                pred[comp] = int(zz[0])
                blocks.append("".join(bits))
        out.append(blocks)
    return out


def _stuffed(bits):
    bits += "1" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00") if bits else b""


def ref_encode(img, quality=90, bgr=True):
    """-> bytes of the JFIF file"""
    a = _check(img)
    H, W = a.shape[:2]
    C = 1 if a.ndim == 2 else 3
    if H > 65535:
        raise ValueError(f"height {H}")
    out = [header(H, W, C, quality)]
    rows = interval_bits(a, quality, bgr)
    for r, blocks in enumerate(rows):
        out.append(_stuffed("".join(blocks)))
        out.append(bytes([0xFF, 0xD9 if r == len(rows) - 1 else 0xD0 + (r & 7)]))
    return b"".join(out)
