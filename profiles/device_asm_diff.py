"""Is the device code of a host-only change the parent's?  Compiles sources of two trees, device side only, to assembly with
sfh_amd/build.py's flags for each file, and compares the text per file - or, for a file that was split or merged, the
pooled text of a set of files of this tree with that of a set of files of the parent tree.

    python profiles/device_asm_diff.py --parent-tree DIR [--out DIR] [FILE.hip ...]
                                       [--parent-sources train.hip --sources train_bn.hip train_heads.hip train_wgrad.hip train_step.hip]

FILE.hip ...: compared one to one (default: the training files that are not named by --sources).  --parent-sources /
--sources: one more comparison, many against one or many against many.

Removed before the comparison: the directives that carry a file name or the compiler's identification (.file, .ident, the
producer comment) and the compilation unit's id symbol (__hip_cuid_<hash of the source text>).  Per comparison it prints the
kernel count (.amdhsa_kernel directives) and one of
  identical         the two texts are the same, line for line
  same functions    the same sections (functions, kernel descriptors, metadata entries) in another order: the order in which
                    a file names its template instantiations moved, or a function moved to another file; no function
                    changed.  Local labels carry the ordinal of their function (.LBB64_3), so they are compared with the
                    ordinal blanked, and with one space before the comment that the assembler pads to a column behind them
                    (the padding depends on the ordinal's width).  Sections that belong to a file and not to a function (the
                    target header, .AMDGPU.gpr_maximums, the padding behind the last function, the one-byte .bss,
                    .note.GNU-stack / .addrsig, the head and the tail of the metadata) occur once per file, so they are
                    compared as SETS: both sides must have the same ones, however many files each side has.  A switch to
                    a section into which nothing follows (the assembler returns to the section it came from before the
                    file's own sections: .text where the file has a function outside a COMDAT group, .AMDGPU.csdata
                    where it has none) defines nothing and is left out.
  same up to commuted operands
                    the two texts have the same number of lines, and every pair of lines that differs is the same v_mul_f64,
                    v_add_f64, v_mul_f32, v_add_f32, v_mul_lo_u32 or v_mul_hi_u32 with the same destination and its two
                    sources - plain registers, no modifier - exchanged, or the same v_mad_u64_u32 (vdst, sdst, src0, src1,
                    src2) with its two factors src0 and src1 exchanged and everything else the same: the compiler met
                    the two factors of a product in the other order.  IEEE multiplication and addition are commutative bit for bit (for two NaN operands
                    the payload may be the other one's) and integer multiplication commutes exactly, so every function
                    computes what it computed, with the same instructions in the same places.  Exit status 0.
  every function of the parent unchanged; added: ...
                    this tree's file holds every section of the parent's, the same text, and more of them: kernels were
                    added to the file (they are named) and no existing one moved.  Exit status 0.
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
# a section of a function: its code, its kernel descriptor, its size and register symbols, its resource comment, its metadata
OF_FUNCTION = re.compile(r"@function|\.amdhsa_kernel |func_end#|codeLenInByte|^\.agpr_count")
EMPTY = re.compile(r"\t\.(section\t.*|text)\n\s*")   # a switch to a section that nothing is put into
REG = r"(?:[vs]\d+|[vs]\[\d+:\d+\])"
COMMUTES = re.compile(rf"\s*(v_(?:(?:mul|add)_f(?:32|64)|mul_(?:lo|hi)_u32)(?:_e32|_e64)?)\s+({REG}),\s*({REG}),\s*({REG})\s*")
# the 64-bit multiply-add: vdst, sdst (carry out), src0 * src1 + src2
COMMUTES_MAD = re.compile(rf"\s*(v_mad_u64_u32(?:_e64)?)\s+({REG}),\s*({REG}|vcc),\s*({REG}),\s*({REG}),\s*({REG}|-?\d+)\s*")
DEFAULT = ["train_bn.hip", "train_heads.hip", "train_wgrad.hip", "train_step.hip", "wgrad_s3.hip", "conv_grouped.hip", "warp.hip",
           "det.hip"]


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
    text = re.sub(r"(?m)^(\.LBB#_\d+:)[ \t]+;", r"\1 ;", text)
    head, _, meta = text.partition("\t.amdgpu_metadata\n")
    return re.split(r"(?m)^(?=\t\.section\t|\t\.text)", head) + re.split(r"(?m)^  - (?=\.agpr_count)|^(?=amdhsa\.target:)", meta)


def pooled(files):
    """(the functions' sections of all files as a multiset, the files' own sections as a set)"""
    secs = [s for lines in files for s in sections(lines) if not EMPTY.fullmatch(s)]
    return collections.Counter(s for s in secs if OF_FUNCTION.search(s)), {s for s in secs if not OF_FUNCTION.search(s)}


def commuted(parent, this):
    """every differing line pair is one commutative instruction with its two register sources exchanged"""
    if len(parent) != len(this):
        return False
    for a, b in zip(parent, this):
        if a != b:
            ma, mb = COMMUTES.fullmatch(a), COMMUTES.fullmatch(b)
            mad_a, mad_b = COMMUTES_MAD.fullmatch(a), COMMUTES_MAD.fullmatch(b)
            if not (ma and mb and ma.group(1, 2, 3, 4) == mb.group(1, 2, 4, 3)) and not (
                    mad_a and mad_b and mad_a.group(1, 2, 3, 4, 5, 6) == mad_b.group(1, 2, 3, 5, 4, 6)):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--out", help="keep the assembly here (parent/ and this/)")
    ap.add_argument("--parent-sources", nargs="+", default=[], help="files of the parent tree whose pooled device code ...")
    ap.add_argument("--sources", nargs="+", default=[], help="... is that of these files of this tree")
    ap.add_argument("files", nargs="*", help="compared one to one")
    a = ap.parse_args()
    if bool(a.parent_sources) != bool(a.sources):
        ap.error("--parent-sources and --sources come together")
    out = a.out or tempfile.mkdtemp(prefix="device_asm_")
    groups = [(a.parent_sources, a.sources)] if a.sources else []
    groups += [([f], [f]) for f in (a.files or [f for f in DEFAULT if f not in a.sources])]
    bad = 0
    for group in groups:
        texts = []
        for name, tree, srcs in (("parent", os.path.abspath(a.parent_tree), group[0]), ("this", ROOT, group[1])):
            os.makedirs(os.path.join(out, name), exist_ok=True)
            texts.append([assembly(tree, src, os.path.join(out, name)) for src in srcs])
        kernels = [sum(ln.lstrip().startswith(".amdhsa_kernel ") for t in side for ln in t) for side in texts]
        lines = [sum(len(t) for t in side) for side in texts]
        if texts[0] == texts[1]:
            verdict = "identical"
        else:
            (p, p_own), (t, t_own) = pooled(texts[0]), pooled(texts[1])
            if p == t and p_own == t_own:
                verdict = "same functions, another order"
            elif commuted(*([ln for f in side for ln in f] for side in texts)):
                verdict = "same up to commuted operands"
            elif not (p - t) and p_own == t_own:
                added = sorted({m for s in (t - p) for m in re.findall(r"\.amdhsa_kernel (\S+)", s)})
                verdict = f"every function of the parent unchanged; added: {', '.join(added) or 'no kernel'}"
            else:
                verdict = "DIFFERENT"
            if verdict == "DIFFERENT":
                bad = 1
                for k in list((p - t).keys())[:2] + list((t - p).keys())[:2] + list(p_own ^ t_own)[:2]:
                    print("   ", k[:300].replace("\n", "\n    "))
        title = " + ".join(group[1]) if group[0] == group[1] else " + ".join(group[0]) + " -> " + " + ".join(group[1])
        print(f"{title}: {kernels[0]} | {kernels[1]} kernels, {lines[0]} | {lines[1]} lines: {verdict}", flush=True)
    return bad


if __name__ == "__main__":
    sys.exit(main())
