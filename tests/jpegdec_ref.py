"""The decoder of sfh_amd.jpegdec restated in numpy / Python with integers only: marker parse, serial Huffman decode, the
subsequence iteration, pixels (csrc/jpegdec.hip and csrc/jpegdec_core.h must equal it byte for byte; tests/test_jpegdec_host.py
holds it to libjpeg's bytes through PIL).  It imports no kernel.

The pixel rule is libjpeg's: dequantise by multiplication; jidctint's "islow" IDCT (constants 13 bits, columns descaled by 11,
rows by 18, +128, clamp); gray: crop; 4:2:0 chroma through the triangle ("fancy") h2v2 upsampler over the component's
ceil(H/2) x ceil(W/2) samples; the 16-bit fixed-point YCbCr -> RGB tables.

The entropy rule is stated on RAW bit positions of a segment (the bytes between two RSTm markers), stuffed bytes included:
byte k is a stuffing byte iff it is 0x00 and byte k - 1 is 0xFF; bytes beyond the segment read as zeros.  A state is (bit
position, block index within the MCU, zig-zag index).  Status bits: 1 no such code, 2 a run past coefficient 63, 4 bits that end
early, 8 blocks left over; only the segment's own blocks count (what follows the last block is padding).
"""
import numpy as np

from jpegenc_ref import ZIGZAG

E_CODE, E_RUN, E_EOF, E_BLOCKS = 1, 2, 4, 8

# refusal reasons, include/sfh_amd.h's SFH_JPEG_R_*
R_TRUNCATED, R_NOT_JPEG, R_MARKER, R_BAD_SOF, R_BAD_TABLE, R_BAD_SOS, R_RESTART, R_SIZE, R_TOO_LONG = range(1, 10)
(R_PROGRESSIVE, R_ARITHMETIC, R_PRECISION, R_DQT16, R_COMPONENTS, R_COLORSPACE, R_SAMPLING, R_NONINTERLEAVED, R_DNL,
 R_SOF_TYPE) = range(100, 110)


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(f"reason {reason}")
        self.reason = reason


def build_huff(bits, vals):
    """one DHT table -> the lookup form of sfh_jpeg_hufftab: look (256), maxcode (18), valoff (18), vals (256)"""
    look = np.zeros(256, np.int64)
    maxcode = np.full(18, -1, np.int64)
    valoff = np.zeros(18, np.int64)
    v = np.zeros(256, np.int64)
    v[:len(vals)] = vals
    code, k = 0, 0
    for l in range(1, 17):
        valoff[l] = k - code
        n = bits[l - 1]
        if n:
            if l <= 8:
                for i in range(n):
                    lo = (code + i) << (8 - l)
                    look[lo:min(lo + (1 << (8 - l)), 256)] = (l << 8) | vals[k + i]
            k += n
            code += n
            if code > (1 << l):
                raise Refused(R_BAD_TABLE)
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0x7FFFFFFF
    return {"look": look, "maxcode": maxcode, "valoff": valoff, "vals": v}


def parse(data):
    """bytes -> dict of the header's fields and the segment table [(first byte, end byte, first MCU)]; raises Refused"""
    b = bytes(data)
    n = len(b)
    if n < 4:
        raise Refused(R_TRUNCATED)
    if b[0] != 0xFF or b[1] != 0xD8:
        raise Refused(R_NOT_JPEG)
    quant, dc, ac = {}, {}, {}
    jfif = adobe = False
    transform = -1
    sof = None
    ri = 0
    i = 2
    while True:
        if i + 2 > n:
            raise Refused(R_TRUNCATED)
        if b[i] != 0xFF:
            raise Refused(R_MARKER)
        while i < n and b[i] == 0xFF:
            i += 1
        if i >= n:
            raise Refused(R_TRUNCATED)
        m = b[i]
        i += 1
        if m in (0xD8, 0xD9, 0x01, 0x00) or 0xD0 <= m <= 0xD7:
            raise Refused(R_MARKER)
        if i + 2 > n:
            raise Refused(R_TRUNCATED)
        ln = (b[i] << 8) | b[i + 1]
        if ln < 2 or i + ln > n:
            raise Refused(R_TRUNCATED)
        body = b[i + 2:i + ln]
        if m in (0xC2, 0xC6, 0xCA, 0xCE):
            raise Refused(R_PROGRESSIVE)
        if m in (0xC9, 0xCB, 0xCD, 0xCF, 0xCC):
            raise Refused(R_ARITHMETIC)
        if m in (0xC1, 0xC3, 0xC5, 0xC7, 0xDE, 0xDF):
            raise Refused(R_SOF_TYPE)
        if m == 0xDC:
            raise Refused(R_DNL)
        if m == 0xC0:
            if sof is not None:
                raise Refused(R_MARKER)
            if len(body) < 6:
                raise Refused(R_TRUNCATED)
            if body[0] != 8:
                raise Refused(R_PRECISION if body[0] == 12 else R_BAD_SOF)
            H, W, nc = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if W == 0:
                raise Refused(R_BAD_SOF)
            if H == 0:
                raise Refused(R_DNL)
            if nc in (2, 4):
                raise Refused(R_COMPONENTS)
            if nc not in (1, 3) or len(body) != 6 + 3 * nc:
                raise Refused(R_BAD_SOF)
            comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)]
            if any(not (1 <= h <= 4 and 1 <= v <= 4 and q <= 3) for _, h, v, q in comps):
                raise Refused(R_BAD_SOF)
            sof = (H, W, comps)
        elif m == 0xDB:
            o = 0
            while o < len(body):
                pq, tq = body[o] >> 4, body[o] & 15
                if tq > 3 or pq > 1:
                    raise Refused(R_BAD_TABLE)
                if pq == 1:
                    raise Refused(R_DQT16)
                if o + 65 > len(body):
                    raise Refused(R_TRUNCATED)
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(body[o + 1:o + 65], np.uint8)
                quant[tq] = t
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(body):
                tc, th = body[o] >> 4, body[o] & 15
                if tc > 1 or th > 3:
                    raise Refused(R_BAD_TABLE)
                if o + 17 > len(body):
                    raise Refused(R_TRUNCATED)
                bits = list(body[o + 1:o + 17])
                cnt = sum(bits)
                if cnt > 256:
                    raise Refused(R_BAD_TABLE)
                if o + 17 + cnt > len(body):
                    raise Refused(R_TRUNCATED)
                vals = list(body[o + 17:o + 17 + cnt])
                if tc == 0 and any(v > 15 for v in vals):
                    raise Refused(R_BAD_TABLE)
                (ac if tc else dc)[th] = build_huff(bits, vals)
                o += 17 + cnt
        elif m == 0xDD:
            if len(body) != 2:
                raise Refused(R_MARKER)
            ri = (body[0] << 8) | body[1]
        elif m == 0xE0:
            jfif = jfif or body[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(body) >= 12 and body[:5] == b"Adobe":
                adobe, transform = True, body[11]
        elif m == 0xDA:
            if sof is None:
                raise Refused(R_MARKER)
            if len(body) < 1:
                raise Refused(R_TRUNCATED)
            ns = body[0]
            if not 1 <= ns <= 4 or len(body) != 4 + 2 * ns:
                raise Refused(R_BAD_SOS)
            H, W, comps = sof
            if ns != len(comps):
                raise Refused(R_NONINTERLEAVED)
            dcsel, acsel = [], []
            for c in range(ns):
                if body[1 + 2 * c] != comps[c][0]:
                    raise Refused(R_BAD_SOS)
                d, a = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
                if d > 3 or a > 3:
                    raise Refused(R_BAD_SOS)
                if d not in dc or a not in ac or comps[c][3] not in quant:
                    raise Refused(R_BAD_TABLE)
                dcsel.append(d)
                acsel.append(a)
            if tuple(body[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise Refused(R_BAD_SOS)
            i += ln
            break
        elif not (0xE1 <= m <= 0xEF or m == 0xFE):
            raise Refused(R_MARKER)
        i += ln
    ids = [c[0] for c in comps]
    if len(comps) == 3:
        if adobe and transform == 0:
            raise Refused(R_COLORSPACE)
        if not jfif and not adobe and ids == [ord("R"), ord("G"), ord("B")]:
            raise Refused(R_COLORSPACE)
        if any((h, v) != (1, 1) for _, h, v, _ in comps[1:]) or (comps[0][1], comps[0][2]) not in ((2, 2), (1, 1)):
            raise Refused(R_SAMPLING)
    elif (comps[0][1], comps[0][2]) != (1, 1):
        raise Refused(R_SAMPLING)
    hs = comps[0][1]
    mcu = 8 * hs
    mcus_x, mcus_y = -(-W // mcu), -(-H // mcu)
    bpm = 1 if len(comps) == 1 else hs * hs + 2
    total = mcus_x * mcus_y
    expected = -(-total // ri) if ri else 1
    scan_begin = i
    segs, start, end, after = [], i, n, -1
    while i < n:
        if b[i] != 0xFF:
            i += 1
            continue
        j = i + 1
        while j < n and b[j] == 0xFF:
            j += 1
        if j >= n:
            end = i
            break
        c = b[j]
        if c == 0:
            if j != i + 1:
                raise Refused(R_MARKER)
            i = j + 1
            continue
        if 0xD0 <= c <= 0xD7:
            if c != 0xD0 + (len(segs) & 7):
                raise Refused(R_RESTART)
            segs.append((start, i, len(segs) * ri))
            start = i = j + 1
            continue
        end, after = i, c
        break
    segs.append((start, end, len(segs) * ri))
    if after == 0xDC:
        raise Refused(R_DNL)
    if after == 0xDA:
        raise Refused(R_NONINTERLEAVED)
    if len(segs) != expected:
        raise Refused(R_RESTART)
    return {"width": W, "height": H, "ncomp": len(comps), "hsamp": hs, "vsamp": comps[0][2], "mcus_x": mcus_x, "mcus_y": mcus_y,
            "blocks_per_mcu": bpm, "restart_interval": ri, "nsegments": len(segs), "scan_begin": scan_begin, "scan_end": end,
            "qsel": [c[3] for c in comps], "dcsel": dcsel, "acsel": acsel, "quant": quant, "dc": dc, "ac": ac, "segments": segs}


# ------------------------------------------------------------------------------------------------------------ entropy decode

class Segment:
    """the bit reader's view of one segment: the data bytes (stuffing removed), their raw indices, and back"""

    def __init__(self, p, data, lo, hi):
        raw = np.concatenate([np.frombuffer(bytes(data[lo:hi]), np.uint8), np.zeros(24, np.uint8)])
        stuff = np.zeros(len(raw), bool)
        stuff[1:] = (raw[1:] == 0) & (raw[:-1] == 0xFF)
        self.nbits = (hi - lo) * 8
        self.stuff = stuff
        self.ridx = np.flatnonzero(~stuff).tolist()
        self.didx = (np.cumsum(~stuff) - 1).tolist()
        self.dbytes = bytes(raw[~stuff]) + bytes(8)
        bpm = p["blocks_per_mcu"]
        comp = [0] * bpm if p["ncomp"] == 1 else [0] * (bpm - 2) + [1, 2]
        self.bpm = bpm
        self.dc = [_fast(p["dc"][p["dcsel"][c]]) for c in comp]
        self.ac = [_fast(p["ac"][p["acsel"][c]]) for c in comp]

    def normalise(self, pos):
        k = pos >> 3
        return (k + 1) << 3 if k > 0 and k < len(self.stuff) and self.stuff[k] else pos


def _fast(t):
    return (t["look"].tolist(), t["maxcode"].tolist(), t["valoff"].tolist(), t["vals"].tolist())


def step(s, pos, blk, zz):
    """one code from the state (pos, blk, zz) -> (pos, blk, zz, k, value, done, err): csrc/jpegdec_core.h's jd_step"""
    dp = s.didx[pos >> 3] * 8 + (pos & 7)
    j = dp >> 3
    bits = (int.from_bytes(s.dbytes[j:j + 5], "big") >> (8 - (dp & 7))) & 0xFFFFFFFF
    look, maxcode, valoff, vals = s.dc[blk] if zz == 0 else s.ac[blk]
    b16 = bits >> 16
    e = look[b16 >> 8]
    if e:
        ln, sym = e >> 8, e & 255
    else:
        ln = 0
        for l in range(9, 17):
            code = b16 >> (16 - l)
            if code <= maxcode[l]:
                ln, sym = l, vals[(code + valoff[l]) & 255]
                break
    err = 0
    if ln == 0:
        nd = dp + 16
        pos = s.ridx[nd >> 3] * 8 + (nd & 7)
        return pos, blk, zz, -1, 0, 0, E_CODE | (E_EOF if pos > s.nbits else 0)
    sz = sym & 15
    run = 0 if zz == 0 else sym >> 4
    v = 0
    if sz:
        v = ((bits << ln) & 0xFFFFFFFF) >> (32 - sz)
        if v < (1 << (sz - 1)):
            v -= (1 << sz) - 1
    k, done = -1, 0
    if zz == 0:
        k, zz = 0, 1
    elif sz == 0:
        if run == 15:
            zz += 16
            if zz > 64:
                err = E_RUN
            done = int(zz >= 64)
        else:
            done = 1
    else:
        zz += run
        if zz > 63:
            err, done = E_RUN, 1
        else:
            k = zz
            zz += 1
            done = int(zz == 64)
    if k < 0:
        v = 0
    if done:
        blk = 0 if blk + 1 == s.bpm else blk + 1
        zz = 0
    nd = dp + ln + sz
    pos = s.ridx[nd >> 3] * 8 + (nd & 7)
    if pos > s.nbits:
        err |= E_EOF
    return pos, blk, zz, k, v, done, err


def _segment_blocks(p, seg):
    total = p["mcus_x"] * p["mcus_y"]
    nm = p["restart_interval"] or total
    return max(min(nm, total - seg[2]), 0) * p["blocks_per_mcu"]


def _integrate_dc(p, coef, seg, nblocks):
    """DC differences -> values, per component over the segment, wrapped to int16 as the device stores them"""
    bpm = p["blocks_per_mcu"]
    comp = np.array([0] * bpm if p["ncomp"] == 1 else [0] * (bpm - 2) + [1, 2])
    b0 = seg[2] * bpm
    view = coef[b0:b0 + nblocks, 0].astype(np.int64)
    which = np.tile(comp, nblocks // bpm)
    for c in range(p["ncomp"]):
        view[which == c] = np.cumsum(view[which == c])
    coef[b0:b0 + nblocks, 0] = view.astype(np.int16)


def decode_serial(p, data):
    """-> (coef int16 (blocks of the image in MCU order, 64) natural order, [status per segment])"""
    nblk_img = p["mcus_x"] * p["mcus_y"] * p["blocks_per_mcu"]
    coef = np.zeros((nblk_img, 64), np.int16)
    natural = ZIGZAG.tolist()
    statuses = []
    for seg in p["segments"]:
        s = Segment(p, data, seg[0], seg[1])
        nblocks = _segment_blocks(p, seg)
        b0 = seg[2] * p["blocks_per_mcu"]
        pos, blk, zz, ab, status = 0, 0, 0, 0, 0
        while pos < s.nbits and ab < nblocks:
            pos, blk, zz, k, v, done, err = step(s, pos, blk, zz)
            status |= err
            if k >= 0:
                coef[b0 + ab, natural[k]] = np.int64(v).astype(np.int16)
            ab += done
        if ab < nblocks:
            status |= E_BLOCKS
        _integrate_dc(p, coef, seg, nblocks)
        statuses.append(status)
    return coef, statuses


def decode_subsequences(p, data, subseq_bits, nthreads=256):
    """the fixed-point iteration over subsequences, lane by lane as the kernel runs it -> (coef, [status], largest round count)"""
    nblk_img = p["mcus_x"] * p["mcus_y"] * p["blocks_per_mcu"]
    coef = np.zeros((nblk_img, 64), np.int16)
    natural = ZIGZAG.tolist()
    statuses, most = [], 0
    S = subseq_bits
    for seg in p["segments"]:
        s = Segment(p, data, seg[0], seg[1])
        nblocks = _segment_blocks(p, seg)
        b0 = seg[2] * p["blocks_per_mcu"]
        nsub = max(-(-s.nbits // S), 1)
        ends = [min((i + 1) * S, s.nbits) for i in range(nsub)]
        ex = [[None] * nsub, [None] * nsub]
        lastin = [None] * nsub
        rounds = 0
        for rnd in range(nsub):
            cur, prev = ex[rnd & 1], ex[(rnd & 1) ^ 1]
            changed = False
            for i in range(nsub):
                if rnd == 0:
                    st = (0, 0, 0) if i == 0 else (s.normalise(i * S), 0, 0)
                elif i < rnd:
                    cur[i] = prev[i]
                    continue
                else:
                    st = prev[i - 1][:3]
                    if st == lastin[i]:
                        cur[i] = prev[i]
                        continue
                lastin[i] = st
                pos, blk, zz = st
                nb = 0
                while pos < ends[i]:
                    pos, blk, zz, _, _, done, _ = step(s, pos, blk, zz)
                    nb += done
                out = (pos, blk, zz, nb)
                changed = changed or rnd == 0 or out != prev[i]
                cur[i] = out
            rounds += 1
            final = cur
            if not changed:
                break
        base = np.concatenate([[0], np.cumsum([e[3] for e in final])]).tolist()
        status = 0
        for i in range(nsub):
            pos, blk, zz = (0, 0, 0) if i == 0 else final[i - 1][:3]
            ab = base[i]
            while pos < ends[i]:
                pos, blk, zz, k, v, done, err = step(s, pos, blk, zz)
                if ab < nblocks:
                    status |= err
                    if k >= 0:
                        coef[b0 + ab, natural[k]] = np.int64(v).astype(np.int16)
                ab += done
        if base[-1] < nblocks:
            status |= E_BLOCKS
        _integrate_dc(p, coef, seg, nblocks)
        statuses.append(status)
        most = max(most, rounds)
    return coef, statuses, most


def checksum(coef, statuses):
    """what tests/jpegdec_host_main.cpp prints: FNV-1a (64 bit) over the int16 coefficients as little-endian bytes"""
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(coef, dtype="<i2").tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    status = 0
    for s in statuses:
        status |= s
    return status, h


# ------------------------------------------------------------------------------------------------------------ pixels

def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, n):
    """jidctint.c's pass over the last axis of d (.., 8), descaled by n"""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    e2, e3 = z1 + z3 * -15137, z1 + z2 * 6270
    e0, e1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    o0, o1, o2, o3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return np.stack([_descale(t10 + o3, n), _descale(t11 + o2, n), _descale(t12 + o1, n), _descale(t13 + o0, n),
                     _descale(t13 - o0, n), _descale(t12 - o1, n), _descale(t11 - o2, n), _descale(t10 - o3, n)], axis=-1)


def idct_blocks(coef, qtab):
    """coef (n, 64) natural order -> (n, 8, 8) samples 0 .. 255"""
    d = (coef.astype(np.int64) * qtab.astype(np.int64)[None, :]).reshape(-1, 8, 8)
    d = _idct_pass(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # columns
    d = _idct_pass(d, 18)                                                # rows
    return np.clip(d + 128, 0, 255)


def planes(p, coef):
    """-> the component planes, whole blocks: [Y] or [Y, Cb, Cr]"""
    mx, my, bpm, hs = p["mcus_x"], p["mcus_y"], p["blocks_per_mcu"], p["hsamp"]
    c = coef.reshape(my, mx, bpm, 64)
    out = []
    for comp in range(p["ncomp"]):
        q = p["quant"][p["qsel"][comp]]
        if comp == 0 and bpm == 6:
            blk = idct_blocks(c[:, :, :4].reshape(-1, 64), q).reshape(my, mx, 2, 2, 8, 8)
            out.append(blk.transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16))
        else:
            j = comp if bpm != 6 else comp + 3
            blk = idct_blocks(c[:, :, j].reshape(-1, 64), q).reshape(my, mx, 8, 8)
            out.append(blk.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return out


def upsample_h2v2(c, H, W):
    """libjpeg's h2v2_fancy_upsample of the component's ceil(H/2) x ceil(W/2) samples -> (H, W)"""
    ch, cw = -(-H // 2), -(-W // 2)
    c = c[:ch, :cw]
    up = np.concatenate([c[:1], c[:-1]])
    dn = np.concatenate([c[1:], c[-1:]])
    v = np.empty((2 * ch, cw), np.int64)
    v[0::2] = 3 * c + up
    v[1::2] = 3 * c + dn
    last = np.concatenate([v[:, :1], v[:, :-1]], axis=1)
    nxt = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
    o = np.empty((2 * ch, 2 * cw), np.int64)
    o[:, 0::2] = (3 * v + last + 8) >> 4
    o[:, 1::2] = (3 * v + nxt + 7) >> 4
    return o[:H, :W]


def pixels(p, coef, bgr=True):
    H, W = p["height"], p["width"]
    pl = planes(p, coef)
    if p["ncomp"] == 1:
        return pl[0][:H, :W].astype(np.uint8)
    y = pl[0][:H, :W]
    if p["hsamp"] == 2:
        cb, cr = upsample_h2v2(pl[1], H, W), upsample_h2v2(pl[2], H, W)
    else:
        cb, cr = pl[1][:H, :W], pl[2][:H, :W]
    r = y + ((91881 * (cr - 128) + 32768) >> 16)
    b = y + ((116130 * (cb - 128) + 32768) >> 16)
    g = y + ((-22554 * (cb - 128) - 46802 * (cr - 128) + 32768) >> 16)
    return np.clip(np.stack([b, g, r] if bgr else [r, g, b], axis=-1), 0, 255).astype(np.uint8)


def ref_decode(data, bgr=True):
    """bytes of a JFIF file -> (H,W,3) BGR / RGB or (H,W) uint8; an image with a status comes back as zeros"""
    p = parse(data)
    coef, statuses = decode_serial(p, data)
    img = pixels(p, coef, bgr)
    return np.zeros_like(img) if any(statuses) else img
