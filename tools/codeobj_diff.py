"""
Compare the gfx950 kernels of two builds of libumpa_hip.so, symbol by symbol (no GPU needed).

    python tools/codeobj_diff.py PARENT_LIB BRANCH_LIB       # a library, or an already unbundled code object

Per kernel: the bytes of its function in .text, and from the code object's metadata notes the resource tuple
(.vgpr_count, .sgpr_count, .private_segment_fixed_size = scratch bytes, .group_segment_fixed_size = LDS bytes,
.vgpr_spill_count).  Class A: bytes identical.  Class B: bytes differ; its before / after tuples are printed.
Per family (the kernel's name without template arguments): kernels, class A, class B.  Names only in one of the two
builds are listed and make the exit status 1.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_coverage import TARGET, _run, llvm_tool   # noqa: E402

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".vgpr_spill_count")


def code_object(path, td, tag):
    """`path` itself if it is an ELF code object, else the gfx950 code object unbundled from its .hip_fatbin section."""
    sections = _run([llvm_tool("llvm-readelf"), "--sections", "--wide", path])
    if ".hip_fatbin" not in sections:
        return path
    fatbin, co = os.path.join(td, tag + ".fatbin"), os.path.join(td, tag + ".co")
    _run([llvm_tool("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fatbin, path, os.path.join(td, tag + ".stripped")])
    _run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin, "--output=" + co])
    return co


def kernels(co):
    """mangled name -> (demangled name, bytes, resource tuple)"""
    readelf = llvm_tool("llvm-readelf")
    text = None
    for line in _run([readelf, "--sections", "--wide", co]).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16))
    if text is None:
        raise RuntimeError("no .text section in %s" % co)
    ndx, addr, off = text
    blob = open(co, "rb").read()
    funcs, kds, pretty = {}, set(), {}
    plain = _run([readelf, "--symbols", "--wide", co]).splitlines()
    demangled = _run([readelf, "--symbols", "--wide", "--demangle", co]).splitlines()      # the same rows, names demangled
    for line, dline in zip(plain, demangled):
        f, d = line.split(None, 7), dline.split(None, 7)
        if len(f) == 8 and f[6] != "UND":
            if f[3] == "FUNC" and f[6] == str(ndx):
                value, size = int(f[1], 16), int(f[2])
                funcs[f[7].strip()] = blob[off + value - addr: off + value - addr + size]
                pretty[f[7].strip()] = d[7].strip()
            elif f[3] == "OBJECT" and f[7].strip().endswith(".kd"):
                kds.add(f[7].strip()[:-3])
    notes = _run([readelf, "--notes", co])
    res = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\n\s*\.name:\s+(\S+)", block)
        if name:
            found = [re.search(r"\n\s*%s:\s+(\d+)" % re.escape(k), block) for k in FIELDS]
            if None in found:
                raise RuntimeError("kernel %s: no %s in its metadata note (%s)" % (name.group(1), FIELDS[found.index(None)], co))
            res[name.group(1).strip("'\"")] = tuple(int(m.group(1)) for m in found)
    out = {}
    for n in sorted(n for n in funcs if n in kds):
        if n not in res:
            raise RuntimeError("kernel %s has no metadata note in %s" % (n, co))
        out[n] = (pretty[n].split("(")[0].replace("void ", "", 1), funcs[n], res[n])
    return out


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as td:
        a = kernels(code_object(argv[0], td, "parent"))
        b = kernels(code_object(argv[1], td, "branch"))
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print("# kernel symbols: parent %d, branch %d, only in parent %d, only in branch %d" % (len(a), len(b), len(only_a), len(only_b)))
    for n in only_a:
        print("only in parent: %s" % a[n][0])
    for n in only_b:
        print("only in branch: %s" % b[n][0])
    fam = {}
    for n in sorted(set(a) & set(b)):
        f = fam.setdefault(a[n][0].split("<")[0], [0, []])
        f[0] += 1
        if a[n][1] != b[n][1]:
            f[1].append(n)
    print("# per family: kernels, class A (bytes identical), class B (bytes differ)")
    for name in sorted(fam):
        print("%-44s %4d %4d %4d" % (name, fam[name][0], fam[name][0] - len(fam[name][1]), len(fam[name][1])))
    print("# total: %d kernels, class A %d, class B %d" % (
        sum(f[0] for f in fam.values()), sum(f[0] - len(f[1]) for f in fam.values()), sum(len(f[1]) for f in fam.values())))
    print("# class B: (%s) and code bytes, parent -> branch" % ", ".join(k.lstrip(".") for k in FIELDS))
    for name in sorted(fam):
        for n in fam[name][1]:
            flag = ""
            if b[n][2][2] > a[n][2][2] or b[n][2][4] > a[n][2][4]:
                flag = "   <-- more scratch / spills"
            print("%s: %s %d B -> %s %d B%s" % (a[n][0], a[n][2], len(a[n][1]), b[n][2], len(b[n][1]), flag))
    return 1 if only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
