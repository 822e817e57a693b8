"""The stand-alone host programs (tests/*_host_main.cpp, which include the plain-C++ headers of csrc/: the decode cores
*_core.h, bn_math.h, chol8.h): found compiler and the sanitizer build that the tests/test_*_host.py files of these programs
share.  A plain module."""
import os
import shutil
import subprocess

from conftest import ROOT


def clangxx():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    near = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    for c in (shutil.which("clang++"), near, "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no clang++ on this machine (looked on PATH and next to hipcc)")


def build_host_program(tmp_path_factory, name):
    """tests/<name>_host_main.cpp -> a stand-alone executable under AddressSanitizer and UBSan, warnings as errors; no
    multiply-add is contracted, as in the library (build.py FLAGS) - bn_math.h's roundings depend on it, the integer codecs
    do not care"""
    out = str(tmp_path_factory.mktemp(f"{name}_host") / f"{name}_host_main")
    cmd = [clangxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", os.path.join(ROOT, "tests", f"{name}_host_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return out
