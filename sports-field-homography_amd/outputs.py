"""Output formats on the far side of the hot path.

Mirrors what the reference's ``predict.py`` does with the dict returned by
``Reconstructor.predict``:

* ``preds_to_masks``            - utils/postprocess.py:7-18 (argmax -> uint8 class ids), on the GPU
* ``format_masks``              - predict.py:286-315: mask_type gray / bin / rgb + nearest resize to
                                  ``out_size``, one HIP pass producing the uint8 image that is written
* ``transfer_gpu_to_cpu``       - predict.py:79-121 (which keys survive, dtypes on the host)
* ``MaskPickleWriter`` / ``MaskReader`` - the PNG-in-pickle stream ``[name, png_bytes]``
                                  (predict.py:26-37, read back by viz_preds.py:52-75)
* ``CourtJsonWriter``           - ``{game}_court.json`` = ``{frame: {score, theta, poi}, ..., model}``
                                  (predict.py:343-357,399-407; consumed by utils/court.py:33-45)

The reference encodes PNGs with OpenCV, which is absent here; ``encode_png``/``decode_png`` are a
small zlib PNG codec for 8-bit gray / 3-channel images.  3-channel arrays are treated as BGR like
``cv2.imencode``/``cv2.imdecode`` do (stored RGB in the file), so streams are interchangeable.
``encode_tiff``/``decode_tiff`` are the same for the 8- and 16-bit TIFF files of the UV labels (LZW, predictor 2): the
written-down rule that ``sfh_amd.tiffenc`` / ``sfh_amd.tiffdec`` are held to.
"""
import io
import json
import os
import pickle
import struct
import zlib

import numpy as np
import torch

from . import _lib
from .engine import _ptr, _stream

# class id -> colour, utils/postprocess.py:29-51 (tuples are written into the array as given)
_PALETTES = {
    4: {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255)},
    7: {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255), 4: (255, 255, 255), 5: (255, 0, 255), 6: (0, 255, 255)},
    8: {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255), 4: (255, 255, 255), 5: (255, 0, 255), 6: (0, 255, 255),
        7: (255, 255, 0)},
}
_MODES = {"gray": 0, "bin": 1, "rgb": 2}


def _palette_bytes(n_classes):
    if n_classes not in _PALETTES:
        raise NotImplementedError(f"no colour table for mask_classes={n_classes} (reference: 4, 7, 8)")
    pal = np.zeros((8, 3), dtype=np.uint8)
    for k, c in _PALETTES[n_classes].items():
        pal[k] = c
    return pal


def format_masks(src, mask_type="gray", n_classes=4, out_size=None):
    """uint8 output masks on the GPU.

    src: logits (B,nc,H,W) float32, a warp_mask (B,H,W) int32, or an id mask (B,H,W) uint8, on the
    GPU.  out_size = (W,H) like ``args.out_size`` (default: source size).  Returns a uint8 tensor
    (B,Hout,Wout) for gray/bin, (B,Hout,Wout,3) for rgb."""
    lib = _lib.load()
    if mask_type not in _MODES:
        raise NotImplementedError(f"mask_type={mask_type!r}")
    if not src.is_cuda or not src.is_contiguous():
        raise ValueError("format_masks needs a contiguous GPU tensor")
    if src.dim() == 4 and src.dtype == torch.float32:
        kind, nc = 2, src.shape[1]
        if nc < 2:
            raise NotImplementedError("single-channel (sigmoid) logits have no class-id mask")
        B, hs, ws = src.shape[0], src.shape[2], src.shape[3]
    elif src.dim() == 3 and src.dtype in (torch.int32, torch.uint8):
        kind, nc = (0 if src.dtype == torch.int32 else 1), n_classes
        B, hs, ws = src.shape
    else:
        raise ValueError(f"format_masks: unsupported source {tuple(src.shape)} {src.dtype}")
    wd, hd = (ws, hs) if out_size is None else (int(out_size[0]), int(out_size[1]))
    mode = _MODES[mask_type]
    pal = _palette_bytes(n_classes) if mode == 2 else None
    shape = (B, hd, wd, 3) if mode == 2 else (B, hd, wd)
    out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    _lib.check(lib.sfh_mask_format_fwd(_ptr(src), kind, nc, B, hs, ws, hd, wd, mode,
                                       pal.ctypes.data if pal is not None else None, _ptr(out), _stream()),
               "mask_format")
    return out


def preds_to_masks(preds, n_classes=1, to_ndaray=True):
    """utils/postprocess.py:7-18 for n_classes > 1: argmax over the class axis (softmax is
    monotonic, so it is skipped), uint8.  The argument keeps the reference's spelling."""
    if n_classes <= 1:
        raise NotImplementedError("n_classes == 1 (sigmoid map) is not a class-id mask")
    m = format_masks(preds, "gray", n_classes)
    return m.cpu().numpy() if to_ndaray else m


def transfer_gpu_to_cpu(preds, req_outputs, mask_classes=4):
    """predict.py:92-118: post-process one predict() dict into host arrays, keeping only the
    requested outputs.  Masks are cast to uint8 on the GPU (4x less PCIe traffic than int32)."""
    out = {k: v for k, v in preds.items() if k in ("name", "orig_img")}
    if "segm_mask" in req_outputs and "logits" in preds:
        out["segm_mask"] = preds_to_masks(preds["logits"], mask_classes)
    if "warp_mask" in req_outputs and "warp_mask" in preds:
        wm = preds["warp_mask"]
        wm = wm if wm.dtype == torch.int32 else wm.to(torch.int32)
        out["warp_mask"] = format_masks(wm.contiguous(), "gray", mask_classes).cpu().numpy()
    if "theta" in req_outputs and "theta" in preds:
        out["theta"] = preds["theta"].cpu().numpy()
    if "consist_score" in preds:
        out["consist_score"] = preds["consist_score"].cpu().numpy()
    if "poi" in req_outputs and "poi" in preds:
        out["poi"] = preds["poi"].cpu().numpy()
    return out


# ------------------------------------------------------------------------------- PNG codec
_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(img, level=1):
    """8-bit gray (H,W) or BGR (H,W,3) array -> PNG file bytes as a 1-D uint8 array (what
    ``cv2.imencode('.png', img)[1]`` holds)."""
    a = np.ascontiguousarray(img)
    if a.dtype == np.bool_ or a.dtype.kind in "iu":
        if a.size and (a.min() < 0 or a.max() > 255):
            raise ValueError("encode_png: values outside 0..255")
        a = a.astype(np.uint8)
    else:
        raise ValueError(f"encode_png: dtype {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim == 2:
        ctype = 0
    elif a.ndim == 3 and a.shape[2] == 3:
        ctype, a = 2, a[:, :, ::-1]  # BGR in memory -> RGB in the file
    else:
        raise ValueError(f"encode_png: shape {a.shape}")
    h, w = a.shape[:2]
    rows = np.ascontiguousarray(a).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()  # filter 0 per scanline
    png = (_PNG_SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw, level)) + _chunk(b"IEND", b""))
    return np.frombuffer(png, dtype=np.uint8)


def decode_png(buf):
    """Inverse of encode_png for 8-bit gray / RGB / RGBA non-interlaced PNGs (all five scanline
    filters).  3/4-channel images come back BGR(A) like ``cv2.imdecode(buf, IMREAD_UNCHANGED)``."""
    data = bytes(np.asarray(buf, dtype=np.uint8).reshape(-1))
    if data[:8] != _PNG_SIG:
        raise ValueError("decode_png: not a PNG")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if zlib.crc32(tag + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError("decode_png: CRC mismatch")
        pos += 12 + n
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    w, h, depth, ctype, _, _, interlace = hdr
    nch = {0: 1, 2: 3, 6: 4}.get(ctype)
    if depth != 8 or nch is None or interlace:
        raise NotImplementedError(f"decode_png: depth {depth} colour type {ctype} interlace {interlace}")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8).reshape(h, 1 + w * nch)
    ftype, rows = raw[:, 0], raw[:, 1:]
    if not ftype.any():
        out = rows.copy()
    else:
        out = np.zeros((h, w * nch), dtype=np.uint8)
        prev = np.zeros(w * nch, dtype=np.int32)
        for y in range(h):
            cur = rows[y].astype(np.int32)
            f = int(ftype[y])
            if f == 2:
                cur = (cur + prev) & 255
            elif f != 0:
                for i in range(w * nch):
                    a = cur[i - nch] if i >= nch else 0
                    b = prev[i]
                    c = prev[i - nch] if i >= nch else 0
                    if f == 1:
                        p = a
                    elif f == 3:
                        p = (a + b) >> 1
                    else:
                        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                        p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                    cur[i] = (cur[i] + p) & 255
            out[y] = cur
            prev = cur
    out = out.reshape(h, w, nch)
    if nch == 1:
        return out[:, :, 0]
    if nch == 3:
        return np.ascontiguousarray(out[:, :, ::-1])
    return np.ascontiguousarray(out[:, :, [2, 1, 0, 3]])


def encode_jpeg(img, quality=90, restart_rows=1):
    """8-bit gray (H,W) or BGR (H,W,3) array -> baseline JPEG file bytes as a 1-D uint8 array, through PIL's libjpeg: 4:2:0, the
    standard Huffman tables - ``cv2.imencode('.jpg', img, [cv2.IMWRITE_JPEG_QUALITY, quality])`` with a restart marker every
    ``restart_rows`` MCU rows (0: none, cv2's file exactly; 1: the bytes of ``sfh_amd.jpegenc``)."""
    from PIL import Image
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"encode_jpeg: dtype {a.dtype} (uint8 only)")
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"encode_jpeg: quality {quality!r} (an integer 1 .. 100)")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    kw = {"restart_marker_rows": int(restart_rows)} if restart_rows else {}
    if a.ndim == 3 and a.shape[2] == 3:
        a, kw["subsampling"] = np.ascontiguousarray(a[:, :, ::-1]), 2           # BGR in memory -> RGB for PIL
    elif a.ndim != 2:
        raise ValueError(f"encode_jpeg: shape {a.shape}")
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=int(quality), **kw)
    return np.frombuffer(buf.getvalue(), dtype=np.uint8)


def decode_jpeg(buf):
    """JPEG file bytes -> uint8 (H,W) or BGR (H,W,3), as ``cv2.imdecode(buf, IMREAD_UNCHANGED)`` gives them (PIL's libjpeg)"""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(np.asarray(buf, dtype=np.uint8).reshape(-1))))
    a = np.array(im)
    return a if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])


# ------------------------------------------------------------------------------- TIFF codec
# The written-down rule of sfh_amd.tiffdec / sfh_amd.tiffenc (csrc/tiff_core.h), in numpy and plain Python: the files libtiff-based
# writers make of 8- and 16-bit labels.  Refusals: codes from 100 on name a feature that is not built (NotImplementedError), the
# others a malformed or unfit file (ValueError) - the SFH_TIFF_R_* of include/sfh_amd.h.
TIFF_REASONS = {1: "the bytes end inside the header", 2: "no byte-order mark or magic 42: not a TIFF file",
                3: "an IFD that reaches outside the file", 4: "a tag of an unknown type or whose array reaches outside the file",
                5: "a strip that reaches outside the file", 6: "a strip table whose length is not ceil(H / RowsPerStrip)",
                7: "a missing required tag", 8: "a zero or absurd size", 11: "size, channels or bits other than the decoder's",
                12: "a file longer than the decoder's max_file_bytes",
                100: "BigTIFF", 101: "a tiled image", 102: "PlanarConfiguration 2", 103: "FillOrder 2",
                104: "a compression other than none and LZW", 105: "a predictor other than 1 and 2",
                106: "a bit depth other than 8 or 16", 107: "a sample format other than unsigned integer",
                108: "a sample count other than 1 and 3", 109: "a palette image or a photometric interpretation other than "
                "BlackIsZero / RGB", 110: "old-style bit-reversed LZW"}
_TIFF_TAGS = {256: "width", 257: "height", 258: "bits", 259: "compression", 262: "photometric", 266: "fill_order", 273: "offsets",
              277: "channels", 278: "rows_per_strip", 279: "counts", 284: "planar", 317: "predictor", 339: "sample_format"}


def _tiff_refuse(reason, who):
    what = TIFF_REASONS[reason]
    if reason >= 100:
        raise NotImplementedError(f"{who}: {what} is not built")
    raise ValueError(f"{who}: {what}")


def tiff_parse(data, who="decode_tiff"):
    """header and first IFD of a classic TIFF (bytes) -> dict: width, height, channels, bits, compression, predictor,
    big_endian, rows_per_strip, photometric and strips = [(offset, byte count, first row, rows)]; raises as ``decode_tiff``"""
    n = len(data)
    if n < 2:
        _tiff_refuse(1, who)
    if data[:2] not in (b"II", b"MM"):
        _tiff_refuse(2, who)
    e = "<" if data[:2] == b"II" else ">"
    if n < 4:
        _tiff_refuse(1, who)
    magic = struct.unpack(e + "H", data[2:4])[0]
    if magic == 43:
        _tiff_refuse(100, who)
    if magic != 42:
        _tiff_refuse(2, who)
    if n < 8:
        _tiff_refuse(1, who)
    ifd = struct.unpack(e + "I", data[4:8])[0]
    if ifd < 8 or ifd + 2 > n:
        _tiff_refuse(3, who)
    nent = struct.unpack(e + "H", data[ifd:ifd + 2])[0]
    if ifd + 2 + 12 * nent > n:
        _tiff_refuse(3, who)
    tags, tiles = {}, False
    for i in range(nent):
        p = ifd + 2 + 12 * i
        tag, typ, count = struct.unpack(e + "HHI", data[p:p + 8])
        tiles = tiles or 322 <= tag <= 325
        if tag not in _TIFF_TAGS:
            continue
        size = {1: 1, 3: 2, 4: 4}.get(typ)
        if size is None or count < 1:
            _tiff_refuse(4, who)
        at = p + 8
        if size * count > 4:
            at = struct.unpack(e + "I", data[p + 8:p + 12])[0]
            if at + size * count > n:
                _tiff_refuse(4, who)
        tags[_TIFF_TAGS[tag]] = struct.unpack(e + str(count) + " BH I"[size], data[at:at + size * count])
    if tiles:
        _tiff_refuse(101, who)
    if any(k not in tags for k in ("width", "height", "photometric", "offsets", "counts")):
        _tiff_refuse(7, who)
    first = lambda k, d: tags[k][0] if k in tags else d
    W, H = tags["width"][0], tags["height"][0]
    if not (1 <= W < 1 << 24 and 1 <= H < 1 << 24):
        _tiff_refuse(8, who)
    C = first("channels", 1)
    if C not in (1, 3):
        _tiff_refuse(108, who)
    bits = first("bits", 1)
    if bits not in (8, 16):
        _tiff_refuse(106, who)
    if "bits" in tags and len(tags["bits"]) not in (1, C):
        _tiff_refuse(8, who)
    if any(b != bits for b in tags.get("bits", ())):
        _tiff_refuse(106, who)
    if any(f != 1 for f in tags.get("sample_format", ())):
        _tiff_refuse(107, who)
    comp = first("compression", 1)
    if comp not in (1, 5):
        _tiff_refuse(104, who)
    if tags["photometric"][0] != (1 if C == 1 else 2):
        _tiff_refuse(109, who)
    if C > 1 and first("planar", 1) != 1:
        _tiff_refuse(102, who)
    if first("fill_order", 1) != 1:
        _tiff_refuse(103, who)
    pred = first("predictor", 1)
    if pred not in (1, 2):
        _tiff_refuse(105, who)
    rps = first("rows_per_strip", 0xFFFFFFFF)
    if rps < 1:
        _tiff_refuse(8, who)
    rps = min(rps, H)
    nstrips = -(-H // rps)
    if len(tags["offsets"]) != nstrips or len(tags["counts"]) != nstrips:
        _tiff_refuse(6, who)
    strips = []
    for s, (off, cnt) in enumerate(zip(tags["offsets"], tags["counts"])):
        if off + cnt > n:
            _tiff_refuse(5, who)
        if comp == 5 and cnt >= 2 and data[off] == 0 and data[off + 1] & 1:
            _tiff_refuse(110, who)
        strips.append((off, cnt, s * rps, min(rps, H - s * rps)))
    pred = pred if comp == 5 else 1              # libtiff applies a predictor inside its LZW codec only
    return {"width": W, "height": H, "channels": C, "bits": bits, "compression": comp, "predictor": pred,
            "big_endian": e == ">", "rows_per_strip": rps, "photometric": tags["photometric"][0], "strips": strips}


def tiff_lzw_decode(data, total):
    """one TIFF 6.0 LZW strip (MSB-first codes of 9 .. 12 bits, Clear 256, EOI 257, early change) -> ``total`` bytes; the decode
    ends when they are complete, so the EOI may be missing and bytes may follow it"""
    out = bytearray()
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    acc = nbits = ip = 0
    width, prev = 9, None
    while len(out) < total:
        while nbits < width:
            if ip >= len(data):
                raise ValueError("decode_tiff: the bits of a strip end early")
            acc = (acc << 8) | data[ip]
            ip += 1
            nbits += 8
        code = (acc >> (nbits - width)) & ((1 << width) - 1)
        nbits -= width
        if code == 256:
            del table[258:]
            width, prev = 9, None
            continue
        if code == 257:
            break
        if prev is None:
            if code > 255:
                raise ValueError("decode_tiff: a first code after Clear that is not a literal")
            s = table[code]
        else:
            room = len(table) < 4096
            if code > len(table) or (code == len(table) and not room):
                raise ValueError("decode_tiff: a code above the next free code")
            s = table[code] if code < len(table) else prev + prev[:1]
            if room:
                table.append(prev + s[:1])
                if len(table) == (1 << width) - 1 and width < 12:
                    width += 1
        out += s
        prev = s
    if len(out) != total:
        raise ValueError("decode_tiff: a strip short of or beyond its rows")
    return bytes(out)


def tiff_lzw_encode(raw):
    """greedy TIFF 6.0 LZW of one strip, as libtiff writes it: Clear first, the longest match, the width grows when the next free
    code reaches 1 << width, Clear and restart when it reaches 4094, the last code then EOI at the width the decoder expects
    there, the final byte zero-padded"""
    out = bytearray()
    acc = nb = 0

    def put(code, width):
        nonlocal acc, nb
        acc = (acc << width) | code
        nb += width
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 255)
            nb -= 8
        acc &= 255

    width, nxt, ent, table = 9, 258, -1, {}
    put(256, width)
    for c in raw:
        if ent < 0:
            ent = c
            continue
        key = (ent << 8) | c
        found = table.get(key)
        if found is not None:
            ent = found
            continue
        put(ent, width)
        table[key] = nxt
        nxt += 1
        ent = c
        if nxt == 4094:
            put(256, width)
            table.clear()
            width, nxt = 9, 258
        elif nxt > (1 << width) - 1:
            width += 1
    if ent >= 0:
        put(ent, width)
        nxt += 1
        if nxt == 4094:
            put(256, width)
            width = 9
        elif nxt > (1 << width) - 1:
            width += 1
    put(257, width)
    if nb:
        out.append((acc << (8 - nb)) & 255)
    return bytes(out)


def decode_tiff(file, bgr=True):
    """TIFF file (bytes or a 1-D uint8 array) -> uint8 / uint16 (H,W) or (H,W,3).  bgr: three samples come back reversed, as
    ``cv2.imread(path, -1)`` returns them.  Classic TIFF, first IFD, II / MM, strips, 8 or 16 bits, 1 or 3 samples, compression 1
    and 5 (LZW), predictor 1 and 2 (applied to the values read in the file's byte order, per sample at a stride of the sample
    count; ignored in an uncompressed file, as libtiff does); NotImplementedError / ValueError for everything else (``TIFF_REASONS``)."""
    data = bytes(np.asarray(file, dtype=np.uint8).reshape(-1)) if not isinstance(file, (bytes, bytearray)) else bytes(file)
    t = tiff_parse(data)
    H, W, C, bits = t["height"], t["width"], t["channels"], t["bits"]
    rowbytes = W * C * bits // 8
    raw = bytearray()
    for off, cnt, _, rows in t["strips"]:
        strip = data[off:off + cnt]
        if t["compression"] == 5:
            raw += tiff_lzw_decode(strip, rows * rowbytes)
        else:
            if cnt < rows * rowbytes:
                raise ValueError("decode_tiff: a strip short of or beyond its rows")
            raw += strip[:rows * rowbytes]
    dt = np.dtype(np.uint8) if bits == 8 else np.dtype(">u2" if t["big_endian"] else "<u2")
    a = np.frombuffer(bytes(raw), dtype=dt).reshape(H, W, C).astype(np.uint8 if bits == 8 else np.uint16)
    if t["predictor"] == 2:
        a = np.cumsum(a, axis=1, dtype=np.uint64).astype(a.dtype)       # modulo 2^bits
    if C == 1:
        return np.ascontiguousarray(a[:, :, 0])
    return np.ascontiguousarray(a[:, :, ::-1] if bgr else a)


def tiff_strip_rows(H, W, C, bits, rows_per_strip=None):
    """the rows of a strip ``encode_tiff`` writes: about 8 KB by default, libtiff's choice"""
    if rows_per_strip is None:
        return min(int(H), max(1, 8192 // (int(W) * int(C) * int(bits) // 8)))
    if not 1 <= int(rows_per_strip) <= int(H):
        raise ValueError(f"encode_tiff: rows_per_strip {rows_per_strip!r} (1 .. {H})")
    return int(rows_per_strip)


def encode_tiff(img, compression="lzw", predictor=2, rows_per_strip=None, bgr=True):
    """uint8 / uint16 (H,W) or (H,W,3) array -> TIFF file bytes as a 1-D uint8 array.  bgr: a 3-channel array is BGR in memory
    (cv2's convention) and stored reversed - a UV label (id, u, v) is stored (v, u, id), which ``cv2.imread(path, -1)`` returns as
    (id, u, v).  Little endian; strips of ``rows_per_strip`` rows (default max(1, 8192 // bytes per row)) directly behind the
    header, each on an even offset; then the BitsPerSample and SampleFormat arrays (3 channels) and the two strip tables (more than
    one strip); the IFD last: tags 256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 339.  LZW: ``tiff_lzw_encode``.  The
    predictor belongs to LZW, as in libtiff: an uncompressed file is stored undifferenced with Predictor 1."""
    a = np.asarray(img)
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"encode_tiff: dtype {a.dtype} (uint8 or uint16)")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_tiff: shape {np.asarray(img).shape}")
    if compression not in ("lzw", "none"):
        raise ValueError(f'encode_tiff: compression={compression!r} ("lzw" or "none")')
    if predictor not in (1, 2):
        raise ValueError(f"encode_tiff: predictor={predictor!r} (1 or 2)")
    if compression == "none":
        predictor = 1                            # libtiff applies a predictor inside its LZW codec only
    H, W, C = a.shape
    bits = 8 * a.dtype.itemsize
    R = tiff_strip_rows(H, W, C, bits, rows_per_strip)
    if C == 3 and bgr:
        a = a[:, :, ::-1]
    if predictor == 2:
        d = a.copy()
        d[:, 1:] = a[:, 1:] - a[:, :-1]                                   # modulo 2^bits
        a = d
    rows = np.ascontiguousarray(a).astype("<u2" if bits == 16 else np.uint8).reshape(H, -1).view(np.uint8)
    out = bytearray(b"II*\0\0\0\0\0")
    offsets, counts = [], []
    for y in range(0, H, R):
        raw = rows[y:y + R].tobytes()
        strip = tiff_lzw_encode(raw) if compression == "lzw" else raw
        offsets.append(len(out))
        counts.append(len(strip))
        out += strip + b"\0" * (len(strip) & 1)
    n = len(offsets)
    arrays = len(out)
    if C == 3:
        out += struct.pack("<6H", bits, bits, bits, 1, 1, 1)
    tables = len(out)
    if n > 1:
        out += struct.pack(f"<{2 * n}I", *offsets, *counts)
    ifd = len(out)
    entries = [(256, 4, 1, W), (257, 4, 1, H), (258, 3, C, arrays if C == 3 else bits), (259, 3, 1, 5 if compression == "lzw" else 1),
               (262, 3, 1, 2 if C == 3 else 1), (273, 4, n, tables if n > 1 else offsets[0]), (277, 3, 1, C), (278, 4, 1, R),
               (279, 4, n, tables + 4 * n if n > 1 else counts[0]), (284, 3, 1, 1), (317, 3, 1, predictor),
               (339, 3, C, arrays + 6 if C == 3 else 1)]
    out += struct.pack("<H", len(entries)) + b"".join(struct.pack("<HHII", *e) for e in entries) + b"\0\0\0\0"
    out[4:8] = struct.pack("<I", ifd)
    return np.frombuffer(bytes(out), dtype=np.uint8)


# --------------------------------------------------------------------- mask streams on disk
def save_mask_as_png(mask, dst_dir, name, postfix="mask"):
    """predict.py:20-25."""
    sub = os.path.join(dst_dir, postfix)
    os.makedirs(sub, exist_ok=True)
    with open(os.path.join(sub, name + ".png"), "wb") as f:
        f.write(encode_png(mask).tobytes())


class MaskPickleWriter:
    """``{dst_dir}/{postfix}/data.pkl``: a sequence of ``pickle.dump([name, png_buffer])`` records
    (predict.py:26-37)."""

    def __init__(self, dst_dir, postfix="mask"):
        sub = os.path.join(dst_dir, postfix)
        os.makedirs(sub, exist_ok=True)
        self.path = os.path.join(sub, "data.pkl")
        self._f = open(self.path, "wb+")

    def write(self, name, mask):
        pickle.dump([name, encode_png(mask)], self._f)

    def write_encoded(self, name, png_buf):
        """a record whose PNG file exists already (sfh_amd.pngenc: encoded on the device): 1-D uint8 array or bytes"""
        buf = np.frombuffer(png_buf, dtype=np.uint8) if isinstance(png_buf, (bytes, bytearray)) else np.asarray(png_buf)
        if buf.dtype != np.uint8 or buf.ndim != 1 or bytes(buf[:8]) != _PNG_SIG:
            raise ValueError("write_encoded: expected the bytes of a PNG file as a 1-D uint8 array")
        pickle.dump([name, np.array(buf)], self._f)

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MaskReader:
    """viz_preds.py:52-75."""

    def __init__(self, path):
        self.entries = []
        with open(path, "rb") as f:
            while True:
                try:
                    self.entries.append(pickle.load(f))
                except EOFError:
                    break

    def get(self, decode=False):
        for name, buf in self.entries:
            yield name, (decode_png(buf) if decode else buf)

    decode = staticmethod(decode_png)


# ------------------------------------------------------------------------------ court json
def _json_default(obj):
    """arrays and numpy scalars -> plain lists / numbers (the court json holds theta and poi as nested lists)"""
    if hasattr(obj, "tolist"):
        return obj.tolist()
    raise TypeError(f"{type(obj).__name__} is not JSON serialisable")


def format_score(score):
    """predict.py:349: ``float('{:5f}'.format(score))`` (6 decimals)."""
    return float("{:5f}".format(float(score)))


class CourtJsonWriter:
    """Streams one JSON line per frame to ``{game}_court_processing.json`` and, on close,
    rewrites it as ``{game}_court.json`` = ``{frame: {...}, ..., "model": name}`` with indent 2
    (predict.py:343-357,399-407)."""

    def __init__(self, dst_dir, game_name, model_name):
        os.makedirs(dst_dir, exist_ok=True)
        self.tmp_path = os.path.join(dst_dir, f"{game_name}_court_processing.json")
        self.path = os.path.join(dst_dir, f"{game_name}_court.json")
        self.model_name = model_name
        self._f = open(self.tmp_path, "w+")

    def add(self, name, score=None, theta=None, poi=None):
        rec = {}
        if score is not None:
            rec["score"] = format_score(score)
        if theta is not None:
            rec["theta"] = np.asarray(theta)  # (1,3,3)
        if poi is not None:
            rec["poi"] = np.asarray(poi)
        json.dump({name: rec}, self._f, default=_json_default)
        self._f.write("\n")

    def add_batch(self, names, preds):
        """preds: host dict from transfer_gpu_to_cpu."""
        for i, n in enumerate(names):
            t = n.split("/")  # predict.py:318-323: "subdir/name" -> name
            self.add(t[1] if len(t) == 2 else t[0],
                     preds["consist_score"][i] if "consist_score" in preds else None,
                     preds["theta"][i] if "theta" in preds else None,
                     preds["poi"][i] if "poi" in preds else None)

    def close(self):
        if self._f is None:
            return self.path
        self._f.close()
        self._f = None
        with open(self.tmp_path, "r") as f:
            output = {k: v for line in f for k, v in json.loads(line).items()}
        output["model"] = self.model_name
        with open(self.path, "w") as f:
            json.dump(output, f, default=_json_default, indent=2)
        os.remove(self.tmp_path)
        return self.path

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load_court_mapping(path):
    """utils/court.py:33-45: {frame: (theta_f2c, theta_c2f, score)} from a ``*_court.json``."""
    with open(path, "r") as f:
        raw = json.load(f)
    model = raw.pop("model", None)
    frames = {}
    for fid, d in raw.items():
        t = np.array(d["theta"])[0]
        frames[fid] = (t, np.linalg.inv(t), float(d["score"]))
    return frames, model
