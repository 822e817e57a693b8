"""CPU-side checks of the C-ABI boundary: the library loads without a GPU and exports exactly the entry points declared in
include/sfh_amd.h; the binding that sfh_amd._abi derives from the header is the one the compiler sees; argument validation
fails loudly."""
import ctypes
import os
import shutil
import subprocess

import pytest

import host_program
from conftest import ROOT


def _exported(path):
    """the sfh_* functions the library defines, by the readelf that sits next to the compiler"""
    near = os.path.join(os.path.dirname(os.path.realpath(host_program.clangxx())), "llvm-readelf")
    readelf = next((c for c in (near, shutil.which("llvm-readelf"), shutil.which("readelf")) if c and os.path.exists(c)), None)
    assert readelf, "no llvm-readelf next to the compiler and no readelf on PATH"
    out =subprocess.run([readelf, "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]           # Num: Value Size Type Bind Vis Ndx Name
    return sorted(r[7] for r in rows if len(r) == 8 and r[3] == "FUNC" and r[6] != "UND" and r[7].startswith("sfh_"))


def test_header_symbols_are_exported_and_bound():
    from sfh_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import sfh_amd.build as b
        b.build(verbose=False)
    lib = _lib.load()
    names = sorted(_lib.SIGNATURES)
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sfh_amd.h but not exported"
    # the other direction: every definition the compiler held to its prototype is one the reader found
    assert _exported(_lib.LIB_PATH) == names, "the library exports an entry that the reader of the header did not find"
    assert lib.sfh_version() >= 100


def test_pinned_signatures():
    """One literal row for each word of the type vocabulary and each shape of declaration."""
    from sfh_amd import _lib
    p, i, i64, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    desc = ctypes.POINTER(_lib.ConvDesc)
    pinned = {
        "sfh_version": (i, []),
        "sfh_last_error": (ctypes.c_char_p, []),
        "sfh_packed_stem_weight_bytes": (i64, []),
        "sfh_multi_copy": (i, [p, p, i, f, p]),
        "sfh_prep_fit": (i, [p, p, p, i, i, d, d, i, p, p, p, p, p, p, p, p]),
        "sfh_fill_words": (i, [p, i64, ctypes.c_uint32, p]),
        "sfh_conv_inc_fused_fwd": (i, [desc, desc, p]),
        "sfh_jpeg_dec_stage": (i64, [p, p, i, i, i, i, i64, i, p, i64, p, p]),
        "sfh_jpeg_parse": (i, [p, i64, p, p, i64]),                     # a structure other than the descriptor: untyped
        "sfh_colsum_det": (i, [p, i64, i, i, p, p, ctypes.c_longlong, p]),
        "sfh_bn_stats_det_bytes": (i64, [i64, i]),
        "sfh_conv_wgrad_det_bytes": (i64, [i] * 11),
    }
    for name, row in pinned.items():
        assert _lib.SIGNATURES[name] == row, name
    assert (_lib.TILE_8x32, _lib.TILE_16x16, _lib.TILE_32x8, _lib.TILE_8x16, _lib.TILE_16x8) == (0, 1, 2, 3, 4)
    assert (_lib.FMT_F32, _lib.FMT_S3, _lib.FMT_H2, _lib.FMT_FH2, _lib.OUT_NHWC, _lib.OUT_UPSCATTER2, _lib.H2_ACT_EXP) == (0, 1, 2, 3, 0, 1, 2)
    assert _lib.ABI.defines["SFH_E_LAUNCH"] == -2
    d0 = _lib.ConvDesc()
    assert (d0.h2_exp_src, d0.h2_exp_dst, d0.h2_exp_res) == (2, 2, 2) and _lib.ConvDesc(h2_exp_src=5).h2_exp_dst == 0


def _cxx_probe(abi):
    """A C++ program that holds the reader's result against the header as the compiler reads it: a static_assert per function
    that its type is the return and parameter types as segmented; main prints every structure's size, every member's offset and
    size, and every define's value."""
    src = ['#include "sfh_amd.h"', "#include <cstddef>", "#include <cstdio>", "#include <type_traits>"]
    for name, (ret, params) in abi.functions.items():
        src.append(f'static_assert(std::is_same<decltype(&{name}), {ret} (*)({", ".join(params)})>::value, "{name}");')
    src.append("int main() {")
    for name, cls in abi.structs.items():
        src.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        for member, _ in cls._fields_:
            src.append(f'  std::printf("{name}.{member} %zu %zu\\n", offsetof({name}, {member}), sizeof({name}::{member}));')
    for name in abi.defines:
        src.append(f'  std::printf("{name} %lld\\n", (long long)({name}));')
    return "\n".join(src + ["  return 0;", "}", ""])


def test_reader_agrees_with_the_compiler(tmp_path):
    """Arity and segmentation of every prototype, the layout of every structure and the value of every define, checked by
    clang++ on a plain host program generated from what the reader found."""
    from sfh_amd import _lib, jpegdec, pngdec, tiffdec
    abi = _lib.ABI
    (tmp_path / "abi_probe.cpp").write_text(_cxx_probe(abi))
    exe = str(tmp_path / "abi_probe")
    r = subprocess.run([host_program.clangxx(), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(tmp_path / "abi_probe.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines():
        key, *numbers = line.split()
        got[key] = tuple(int(v) for v in numbers)
    want = {name: (value,) for name, value in abi.defines.items()}
    for name, cls in abi.structs.items():
        want[name] = (ctypes.sizeof(cls),)
        for member, _ in cls._fields_:
            want[f"{name}.{member}"] = (getattr(cls, member).offset, getattr(cls, member).size)
    assert got == want
    assert len(abi.functions) == len(_lib.SIGNATURES) >= 178 and len(abi.structs) == 5 and len(abi.defines) >= 100
    # the classes the package uses are those structures
    assert issubclass(_lib.ConvDesc, abi.structs["sfh_conv_desc"]) and ctypes.sizeof(_lib.ConvDesc) == got["sfh_conv_desc"][0]
    assert (jpegdec.HuffTab, jpegdec.JpegInfo, pngdec.PngInfo, tiffdec.TiffInfo) == tuple(
        abi.structs[n] for n in ("sfh_jpeg_hufftab", "sfh_jpeg_info", "sfh_png_info", "sfh_tiff_info"))
    # by hand: 28 int32 in front of quant[4][64]; a Huffman table is 512 + 72 + 72 + 256 bytes
    assert got["sfh_jpeg_info.quant"] == (112, 512) and got["sfh_jpeg_info.dc"] == (624, 4 * 912) and got["sfh_png_info.adler"] == (40, 4)


def test_constants_are_the_headers():
    from sfh_amd import _lib, evaluation, jpegdec, jpegenc, outputs, pngdec, pngenc, preparation, resample, visualize
    d = _lib.ABI.defines
    assert (resample.MAX_TAPS, pngenc.MAX_ROW, jpegenc.MAX_WIDTH, preparation.MAX_POINTS, evaluation.SLOTS) == (
        d["SFH_RESAMPLE_MAX_TAPS"], d["SFH_PNG_MAX_ROW"], d["SFH_JPEG_MAX_WIDTH"], d["SFH_PREP_MAX_POINTS"], d["SFH_EVAL_SLOTS"]) == (
        64, 32768, 2048, 256, 9)
    assert resample.FILTERS == {"box": 4, "bilinear": 2, "bicubic": 3} and resample.NEAREST_RULES == {"pil": 0, "cv2": 1}
    assert visualize.SOURCES == {"auto": 0, "warp": 1, "segm": 2} and visualize.LABEL_MAX == 32
    assert (evaluation.SEG, evaluation.REC, evaluation.UV, evaluation.REPROJ, evaluation.REPROJ_PX, evaluation.CONSIST,
            evaluation.NBATCH, evaluation.FRAMES, evaluation.BAD) == tuple(range(9))
    # the wording of a refusal is Python's; which refusals exist is the header's
    for prefix, reasons in (("SFH_JPEG_R_", jpegdec.REASONS), ("SFH_PNG_R_", pngdec.REASONS), ("SFH_TIFF_R_", outputs.TIFF_REASONS)):
        codes = {v for n, v in d.items() if n.startswith(prefix) and n != prefix + "OK"}
        assert len(codes) >= 17 and set(reasons) == codes, prefix


@pytest.mark.parametrize("line, text, what", [
    (2, "int sfh_a(int n);\nint sfh_b(const size_t* p, void* stream);\n", "size_t"),
    (4, "typedef struct sfh_a {\n  int32_t n;\n} sfh_a;\ntypedef struct sfh_b { int32_t n; sfh_c c[2]; } sfh_b;\n", "sfh_c"),
    (3, "/* two lines\n   of comment */\n#define SFH_HALF 0.5\n", "SFH_HALF"),
    (2, "#define SFH_ONE 1\nint sfh_a(int n, void* stream)\nint sfh_b(void);\n", "sfh_a"),
], ids=["unknown-type-word", "unknown-struct-member", "non-integer-define", "prototype-cut-off"])
def test_reader_refuses_what_it_does_not_understand(line, text, what):
    from sfh_amd import _abi
    with pytest.raises(_abi.SfhError, match=rf"^sfh_amd\.h:{line}: .*{what}"):
        _abi.Abi(text)


def test_reader_refuses_a_missing_header(tmp_path):
    from sfh_amd import _abi
    with pytest.raises(_abi.SfhError, match="nowhere.h"):
        _abi.read(str(tmp_path / "nowhere.h"))


def test_argument_validation_without_gpu():
    from sfh_amd import _lib
    lib = _lib.load()
    assert lib.sfh_packed_weight_floats(3, 64, 0, 64) == 4 * 9 * 1024
    assert lib.sfh_packed_weight_floats(3, 64, 64, 128) == 2 * 8 * 9 * 1024
    assert lib.sfh_packed_weight_floats(5, 64, 0, 64) == -1       # unsupported kernel size
    assert lib.sfh_packed_weight_floats(3, 64, 0, 48) == -1       # cout not a multiple of 64
    # split-operand formats: 3 bf16 planes (S3) / 2 fp16 planes (H2) of [cout/64][cin/32][tap][plane][4 KB]
    assert lib.sfh_packed_s3_weight_bytes(3, 64, 0, 64) == 2 * 9 * 3 * 4096
    assert lib.sfh_packed_h2_weight_bytes(3, 64, 0, 64) == 2 * 9 * 2 * 4096
    assert lib.sfh_packed_h2_weight_bytes(3, 48, 0, 64) == -1     # cin not a multiple of 32
    d = _lib.ConvDesc()
    rc = lib.sfh_conv_fwd(ctypes.byref(d), None)                  # all-null descriptor
    assert rc == -1 and b"null" in lib.sfh_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "conv_fwd")
    rc = lib.sfh_homography_warp_fwd(None, None, 0, 360, 640, 16, 360, 640, 0, 4.0, None, None, None)
    assert rc == -1
    # round 6 entries: argument checks fire before anything touches a device
    assert lib.sfh_vec_op(1, None, None, 16, 0, 1.0, None, None) == -1
    assert lib.sfh_multi_absminmax(None, 3, None, None) == -1
    assert lib.sfh_stn_input_assemble(None, 4, None, 3, None, 0, 2, 8, 8, 4, None, None) == -1      # 7 channels into 4
    assert b"7" in lib.sfh_last_error() or b"channels" in lib.sfh_last_error()
    assert lib.sfh_uv_loss(None, None, None, 5, 2, 2, 8, 8, 1.0, 1, None, None, None) == -1
    assert lib.sfh_adam_step(None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 1.0, 1, None) == -1
    assert lib.sfh_grad_scale(None, 1, 1, 0, None, None, None) == -1


def test_model_refuses_cpu_execution():
    import torch
    from sfh_amd import synth
    from sfh_amd.reconstructor import Reconstructor
    net = Reconstructor(synth.load_court_template(batch_size=1), synth.load_court_poi(batch_size=1)).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.predict(torch.zeros(1, 3, 360, 640))


def test_missing_library_fails_loudly(tmp_path):
    """No HIP extension -> an explicit error, never a silent CPU / PyTorch path."""
    import subprocess
    import sys
    code = ("import os, sys; sys.path.insert(0, %r); os.environ['SFH_AMD_LIB'] = %r\n"
            "from sfh_amd import _lib\n"
            "try:\n    _lib.load()\nexcept _lib.SfhError as e:\n    print('SfhError:', e); sys.exit(7)\n"
            "sys.exit(0)\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), str(tmp_path / "nope.so"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 7, r.stdout + r.stderr
    assert "not found" in r.stdout and "no CPU/PyTorch fallback" in r.stdout
