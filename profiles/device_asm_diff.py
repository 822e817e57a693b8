"""Is the device code of a host-only change the parent's?  Compiles sources of two trees, device side only, to assembly with
sfh_amd/build.py's flags for each file, and compares the text per file.

    python profiles/device_asm_diff.py --parent-tree DIR [--out DIR] [train.hip wgrad_s3.hip conv_grouped.hip warp.hip det.hip]

Removed before the comparison: the directives that carry a file name or the compiler's identification (.file, .ident, the
producer comment) and the compilation unit's id symbol (__hip_cuid_<hash of the source text>).  Per file it prints the kernel
count (.amdhsa_kernel directives) and one of
  identical         the two texts are the same, line for line
  same functions    the same sections (functions, kernel descriptors, metadata entries) in another order: the order in which
                    a file names its template instantiations moved, no function did.  Local labels carry the ordinal of
                    their function (.LBB64_3), so they are compared with the ordinal blanked.
  DIFFERENT         anything else; the first differing sections are shown.  Exit status 1.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DROP = re.compile(r"^\s*\.(file|ident)\b|clang version|__hip_cuid_|^\s*;.*\.hip")


def assembly(tree, source, out):
    from sfh_amd import build
    csrc = os.path.join(tree, os.path.relpath(build.CSRC, ROOT))
    path = os.path.join(out, source.replace(".hip", ".s"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + build.FLAGS + build.EXTRA_FLAGS.get(source, []) + ["--cuda-device-only", "-S", source, "-o", path],
                          cwd=csrc, stderr=subprocess.DEVNULL)
    with open(path) as f:
        return [ln for ln in f if not DROP.search(ln)]


def sections(lines):
    """functions and data by their .section / .text line, the metadata by kernel entry; labels without the function's ordinal"""
    text = re.sub(r"(BB|func_begin|func_end)\d+", r"\1#", "".join(lines))
    head, _, meta = text.partition("\t.amdgpu_metadata\n")
    return re.split(r"(?m)^(?=\t\.section\t|\t\.text)", head) + re.split(r"(?m)^  - (?=\.agpr_count)", meta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--out", help="keep the assembly here (parent/ and this/)")
    ap.add_argument("sources", nargs="*", default=["train.hip", "wgrad_s3.hip", "conv_grouped.hip", "warp.hip", "det.hip"])
    a = ap.parse_args()
    out = a.out or tempfile.mkdtemp(prefix="device_asm_")
    bad = 0
    for src in a.sources:
        texts = []
        for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
            os.makedirs(os.path.join(out, name), exist_ok=True)
            texts.append(assembly(tree, src, os.path.join(out, name)))
        kernels = [sum(ln.lstrip().startswith(".amdhsa_kernel ") for ln in t) for t in texts]
        if texts[0] == texts[1]:
            verdict = "identical"
        else:
            p, t = (collections.Counter(sections(x)) for x in texts)
            verdict = "same functions, another order" if p == t else "DIFFERENT"
            if p != t:
                bad = 1
                for k in list((p - t).keys())[:2] + list((t - p).keys())[:2]:
                    print("   ", k[:300].replace("\n", "\n    "))
        print(f"{src}: {kernels[0]} | {kernels[1]} kernels, {len(texts[0])} | {len(texts[1])} lines: {verdict}", flush=True)
    return bad


if __name__ == "__main__":
    sys.exit(main())
