"""ctypes binding of libsfh_amd.so (C ABI: include/sfh_amd.h).

The binding is derived: ``_abi`` reads the header at import, and the signature table, the descriptor structure and the
constants below are what it found there.  There is deliberately no fallback: if the header or the library is missing or a
symbol cannot be resolved, importing the hot path fails with an explicit error.
"""
import ctypes as C
import os

from . import _abi
from ._abi import SfhError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# SFH_AMD_LIB overrides the library file (used only to load the diagnostic build for profiling)
LIB_PATH = os.environ.get("SFH_AMD_LIB") or os.path.join(_HERE, "libsfh_amd.so")

ABI = _abi.read()
_D = ABI.defines
TILE_8x32, TILE_16x16, TILE_32x8, TILE_8x16, TILE_16x8 = (_D["SFH_TILE_" + t] for t in ("8x32", "16x16", "32x8", "8x16", "16x8"))
OUT_NHWC, OUT_UPSCATTER2 = _D["SFH_OUT_NHWC"], _D["SFH_OUT_UPSCATTER2"]
FMT_F32, FMT_S3, FMT_H2, FMT_FH2 = (_D["SFH_FMT_" + f] for f in ("F32", "S3", "H2", "FH2"))
H2_ACT_EXP = _D["SFH_H2_ACT_EXP"]   # the default exponent of an H2 tensor
H2_LIMIT_BITS = 0x477FE000   # bit pattern of 65504.f: sfh_conv_desc.h2_range words above it mean saturation


class ConvDesc(ABI.structs["sfh_conv_desc"]):
    """``struct sfh_conv_desc`` (include/sfh_amd.h) with the default exponents filled in."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        # H2 tensors of a launch carry v * 2^e; callers that do not manage exponents (the training kernels) get the
        # conventional default for every tensor
        if "h2_exp_src" not in kw:
            self.h2_exp_src = self.h2_exp_dst = self.h2_exp_res = H2_ACT_EXP


# name -> (restype, argtypes); every symbol declared in include/sfh_amd.h.  NAME_det (NAME's arguments with (workspace,
# workspace_bytes) in front of the stream) and NAME_det_bytes (the size query) are declared there like every other entry.
SIGNATURES = ABI.signatures({"const sfh_conv_desc*": C.POINTER(ConvDesc)})
DET_ENTRIES = tuple(sorted(n[:-4] for n in SIGNATURES if n.endswith("_det")))

_lib = None


def load():
    """Load libsfh_amd.so and bind every symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SfhError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU/PyTorch fallback for this path."
        )
    # PyTorch first: it ships its own HIP runtime (torch/lib/libamdhip64.so) and owns device memory and streams.
    # Loading libsfh_amd.so before torch would bring /opt/rocm's copy of the runtime into the process as well,
    # and the second copy then sees no device ("no ROCm-capable device is detected" at the first launch).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().sfh_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise SfhError(f"{what}: error {rc}: {msg}")
