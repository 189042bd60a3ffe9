"""
Which of libumpa_hip.so's gfx950 kernels a run launched.

    python tools/kernel_coverage.py                      # the kernel symbols of the code object, one per line
    python tools/kernel_coverage.py TRACE_DIR_OR_CSV ... # + which of them the traced run launched, and which it did not

Symbols: the .hip_fatbin section of the library, unbundled to its gfx950 code object, read as demangled ELF FUNC symbols
that have a kernel descriptor (a `<name>.kd` OBJECT): device functions the compiler did not inline are not kernels.
Launches: every `*kernel_stats.csv` / `*kernel_trace.csv` that `rocprofv3 --kernel-trace --stats --output-format csv` wrote
under the given directories (the suite starts child processes: each writes its own files), read by the `Name` /
`Kernel_Name` column, which uses the same demangled form.

The LLVM tools come from $ROCM_PATH/llvm/bin (default /opt/rocm); a missing tool is an error, never an empty list.
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "umpa_amd", "libumpa_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


class ToolMissing(RuntimeError):
    pass


def llvm_tool(name):
    d = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    p = os.path.join(d, name)
    if not os.access(p, os.X_OK):
        raise ToolMissing("%s not found in %s: kernel_coverage needs llvm-objcopy, clang-offload-bundler and "
                          "llvm-readelf of the ROCm LLVM toolchain (set ROCM_PATH)" % (name, d))
    return p


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (os.path.basename(cmd[0]), r.returncode, r.stderr.strip()))
    return r.stdout


def kernel_symbols(lib=LIB):
    """The demangled kernel names of `lib`'s gfx950 code object, sorted."""
    if not os.path.exists(lib):
        raise FileNotFoundError("%s not built (python -c 'import __graft_entry__ as g; g.build()')" % lib)
    objcopy, bundler, readelf = llvm_tool("llvm-objcopy"), llvm_tool("clang-offload-bundler"), llvm_tool("llvm-readelf")
    with tempfile.TemporaryDirectory() as td:
        fatbin, co = os.path.join(td, "fatbin"), os.path.join(td, "gfx950.co")
        _run([objcopy, "--dump-section=.hip_fatbin=" + fatbin, lib, os.path.join(td, "stripped")])
        _run([bundler, "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin, "--output=" + co])
        out = _run([readelf, "--symbols", "--wide", "--demangle", co])
    funcs, kds = set(), set()
    for line in out.splitlines():
        f = line.split(None, 7)
        # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[6] != "UND":
            name = f[7].strip()
            if f[3] == "FUNC":
                funcs.add(name)
            elif f[3] == "OBJECT" and name.endswith(" (.kd)"):   # the descriptor, demangled: "name(args) (.kd)"
                kds.add(name[:-6])
            elif f[3] == "OBJECT" and name.endswith(".kd"):      # ... or a name that does not demangle: "name.kd"
                kds.add(name[:-3])
    names = funcs & kds                                               # a kernel has a descriptor; a device function does not
    if not names:
        raise RuntimeError("no kernel symbols in the gfx950 code object of %s" % lib)
    return sorted(names)


def _trace_files(paths):
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += glob.glob(os.path.join(p, "**", "*kernel_stats.csv"), recursive=True)
            files += glob.glob(os.path.join(p, "**", "*kernel_trace.csv"), recursive=True)
        else:
            files.append(p)
    return sorted(set(files))


def launched(paths):
    """Kernel name -> launches, summed over every kernel-stats / kernel-trace CSV under `paths`.  A trace row counts one
    launch; a stats row counts its `Calls`.  (A directory with both kinds of file for one process counts it twice: the
    number is a presence test, not a launch count.)"""
    files = _trace_files(paths)
    if not files:
        raise FileNotFoundError("no *kernel_stats.csv / *kernel_trace.csv under %s" % ", ".join(paths))
    seen = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("Kernel_Name")
                if not name:
                    continue
                n = int(row["Calls"]) if row.get("Calls") else 1
                seen[name.strip()] = seen.get(name.strip(), 0) + n
    return seen


def main(argv):
    syms = kernel_symbols()
    if not argv:
        print("\n".join(syms))
        print("# %d kernel symbols" % len(syms), file=sys.stderr)
        return 0
    seen = launched(argv)
    hit = [s for s in syms if seen.get(s)]
    miss = [s for s in syms if not seen.get(s)]
    print("# %d kernel symbols, %d launched, %d not launched" % (len(syms), len(hit), len(miss)))
    print("## launched (calls)")
    for s in hit:
        print("%8d  %s" % (seen[s], s))
    print("## not launched")
    for s in miss:
        print("          %s" % s)
    other = sorted(n for n in seen if n not in set(syms))
    if other:
        print("## launched, not in the library (other code objects)")
        for s in other:
            print("%8d  %s" % (seen[s], s))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
