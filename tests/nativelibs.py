"""
What the tests of the native libraries share: building them, their exported symbols, their kernels, the symbols a public
header declares.  One row of LIBRARIES per library: (attribute of __graft_entry__, symbol prefix, list of umpa_amd._lib,
kernel families).
"""
import os
import re
import sys

from conftest import REPO

LIBRARIES = [
    ("HIP_LIB", "umpa_hip_", "HIP_SYMBOLS", None),                    # the main library's kernel set: tests/test_kernel_coverage.py
    ("GRID_LIB", "umpa_grid_", "GRID_SYMBOLS", ("grid_min_kernel", "cost_volume_kernel")),
    ("UNWARP_LIB", "umpa_unwarp_", "UNWARP_SYMBOLS", ("unwarp_kernel",)),
    ("REGISTER_LIB", "umpa_register_", "REGISTER_SYMBOLS", ("register_tile_kernel", "register_norm_kernel", "register_reduce_kernel")),
    ("INTEGRATE_LIB", "umpa_integrate_", "INTEGRATE_SYMBOLS", tuple("integrate_%s_kernel" % k for k in (
        "weights", "diag", "rhs", "coarsen", "sweep0", "sweep", "restrict", "prolong", "jacobi", "tail",
        "apply_dot", "update", "residual", "dot", "direction", "gauge", "output", "scalar"))),
    ("DDF_LIB", "umpa_ddf_", "DDF_SYMBOLS", ("ddf_blur_kernel", "ddf_fold_kernel")),
]


def tool(name):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def build_all():
    """__graft_entry__, after building where any of the six libraries is missing"""
    import __graft_entry__ as g
    if not all(os.path.exists(getattr(g, row[0])) for row in LIBRARIES):
        g.build()
    return g


def declared(header, prefix):
    """the functions with `prefix` that include/<header> declares"""
    hdr = open(os.path.join(REPO, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, hdr)))


def exported(lib):
    """the defined dynamic symbols of a shared library"""
    kc = tool("kernel_coverage")
    out = kc._run([kc.llvm_tool("llvm-readelf"), "--dyn-syms", "--wide", lib])
    names = set()
    for line in out.splitlines():
        f = line.split(None, 7)
        if len(f) == 8 and f[6] != "UND" and f[3] in ("FUNC", "OBJECT"):
            names.add(f[7].split("@")[0].strip())
    return names


def kernel_keys(lib):
    kc = tool("kernel_coverage")
    return [re.sub(r"^void ", "", s).split("(", 1)[0].split("::", 1)[-1] for s in kc.kernel_symbols(lib)]


def gpu_test_module(name):
    """tests/test_hip_<name>.py as a module (for its REACHES table)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_%s_gpu" % name, os.path.join(REPO, "tests", "test_hip_%s.py" % name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_claimed(syms, name):
    """every kernel of `syms` is claimed by a test of tests/test_hip_<name>.py, and its REACHES table names no other"""
    mod = gpu_test_module(name)
    claimed = set()
    for names in mod.REACHES.values():
        claimed |= set(names)
    orphans = [s for s in syms if s not in claimed]
    assert not orphans, "kernels of libumpa_%s.so no test of tests/test_hip_%s.py claims: %s" % (name, name, orphans)
    stale = sorted(claimed - set(syms))
    assert not stale, "REACHES names kernels the library does not have: %s" % stale
    return mod
