"""
The six native libraries against each other, without a GPU: what each exports and which kernels it holds (one test in
place of the copies that tests/test_register_cpu.py, tests/test_integrate_cpu.py and tests/test_ddf_cpu.py had, each for
the libraries that existed when it was written).
"""
from nativelibs import LIBRARIES, build_all, declared, exported, kernel_keys


def test_every_library_exports_its_own_symbols_and_holds_its_own_kernels():
    """All six libraries: each exports exactly the symbols its own header declares under its own prefix (the lists of
    umpa_amd._lib), no symbol under another library's prefix, and holds none of another library's kernel families; the three
    libraries that include none of the kernel headers hold their own families and nothing else."""
    g = build_all()
    from umpa_amd import _lib
    for attr, prefix, symbols, families in LIBRARIES:
        lib = getattr(g, attr)
        names, keys = exported(lib), kernel_keys(lib)
        own = sorted(n for n in names if n.startswith(prefix))
        assert own == sorted(prefix + s for s in getattr(_lib, symbols)), lib
        assert own == declared(prefix[:-1] + ".h", prefix), lib
        for _, other, _, theirs in LIBRARIES:
            if other != prefix:
                assert not [n for n in names if n.startswith(other[:-1])], (lib, other)
                assert not [k for k in keys if theirs and k.split("<", 1)[0] in theirs], (lib, other)
        if attr in ("REGISTER_LIB", "INTEGRATE_LIB", "DDF_LIB"):
            assert keys and {k.split("<", 1)[0] for k in keys} <= set(families), lib
        elif families:
            assert set(families) <= {k.split("<", 1)[0] for k in keys}, lib
    assert sorted(kernel_keys(g.INTEGRATE_LIB)) == sorted(LIBRARIES[4][3])     # no templates there: one kernel per family
