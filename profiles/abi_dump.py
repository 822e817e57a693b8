"""The ctypes binding as Python sees it, as one JSON document: every row of ``_lib.SIGNATURES`` (restype and argtypes by
name), the five structures field by field (name, type, offset, size) and the constants that repeat a ``#define`` of
include/sfh_amd.h.  No device and no library needed.  Run before and after a change of the binding and compare:

    python profiles/abi_dump.py > profiles/abi_dump.json

profiles/abi_dump.json is the committed output (see README, "The C ABI stated once")."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sfh_amd import _lib, evaluation, jpegdec, jpegenc, outputs, pngdec, pngenc, preparation, resample, tiffdec, visualize  # noqa: E402


def tname(t):
    """a field's type without the Python class names: uint16_t x[4][64] -> c_ushort[64][4], a structure -> struct:<bytes>"""
    if hasattr(t, "_length_"):
        return f"{tname(t._type_)}[{t._length_}]"
    return f"struct:{ctypes.sizeof(t)}" if issubclass(t, ctypes.Structure) else t.__name__


def struct(cls):
    return [(name, tname(typ), getattr(cls, name).offset, getattr(cls, name).size) for name, typ in cls._fields_]


doc = {
    "signatures": {n: (res.__name__, [a.__name__ for a in args]) for n, (res, args) in sorted(_lib.SIGNATURES.items())},
    "det_entries": list(_lib.DET_ENTRIES),
    "structs": {"ConvDesc": struct(_lib.ConvDesc), "HuffTab": struct(jpegdec.HuffTab), "JpegInfo": struct(jpegdec.JpegInfo),
                "PngInfo": struct(pngdec.PngInfo), "TiffInfo": struct(tiffdec.TiffInfo)},
    "constants": {
        **{"_lib." + k: getattr(_lib, k) for k in sorted(vars(_lib)) if k.startswith(("TILE_", "OUT_", "FMT_", "H2_"))},
        "resample.MAX_TAPS": resample.MAX_TAPS, "pngenc.MAX_ROW": pngenc.MAX_ROW, "jpegenc.MAX_WIDTH": jpegenc.MAX_WIDTH,
        "preparation.MAX_POINTS": preparation.MAX_POINTS, "evaluation.SLOTS": evaluation.SLOTS,
        "evaluation.SEG..BAD": [evaluation.SEG, evaluation.REC, evaluation.UV, evaluation.REPROJ, evaluation.REPROJ_PX,
                                evaluation.CONSIST, evaluation.NBATCH, evaluation.FRAMES, evaluation.BAD],
        "resample.FILTERS": resample.FILTERS, "resample.NEAREST_RULES": resample.NEAREST_RULES,
        "visualize.SOURCES": visualize.SOURCES, "visualize.LABEL_MAX": visualize.LABEL_MAX,
        "jpegdec.REASONS": sorted(jpegdec.REASONS), "pngdec.REASONS": sorted(pngdec.REASONS),
        "outputs.TIFF_REASONS": sorted(outputs.TIFF_REASONS)},
}
doc["structs"] = {f"{s}.{row[0]}": row[1:] for s, rows in doc["structs"].items() for row in rows}
doc["det_entries"] = {"DET_ENTRIES": doc["det_entries"]}
print("{\n" + ",\n".join(json.dumps(section) + ": {\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items())
                         + "\n }" for section, rows in doc.items()) + "\n}")      # one row per line: the file diffs row by row
