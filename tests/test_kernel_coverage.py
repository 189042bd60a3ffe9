"""
Every kernel symbol of the built library has a test that launches it.

The symbols come from the gfx950 code object of umpa_amd/libumpa_hip.so (tools/kernel_coverage.py).  Each must be claimed,
by its full `name<args>`, by a `reaches` entry of tests/test_hip_instantiations.py, by a named test elsewhere in the suite,
or by an exclusion below with its reason; a new instantiation without a test fails here.  Every claim must name a symbol,
so that a table that outlives the kernels it was written for fails too.  Where the cases choose an instantiation through
tables that mirror the dispatch (corr_volume's workgroup shapes, pick_ub's batch widths, masked_ub), those tables are
checked against the source.  Whether the claims hold is what a kernel trace of the GPU suite shows
(`rocprofv3 --kernel-trace --stats`, read by the same tool).
"""
import importlib.util
import os
import re

import pytest

from conftest import REPO

TILED_H = os.path.join(REPO, "umpa_amd", "csrc", "umpa_tiled.h")

# kernel -> the existing test that launches it
NAMED = {
    "badpix_mark_kernel": "tests/test_align.py::test_hip_bad_pixels_match_reference_golden",
    "badpix_pass_kernel": "tests/test_align.py::test_hip_bad_pixels_match_reference_golden",
    "coverage_kernel": "tests/test_hip_parity.py::test_sample_stepping_on_the_tiled_path (coverage())",
    "spfit_kernel": "tests/test_hip_parity.py::test_subpixel_kats_on_device",
    "od_list_kernel": "tests/test_hip_parity.py::test_on_demand_table_passes_change_nothing",
    "mask_binary_kernel": "tests/test_hip_parity.py::test_masks_and_sample_stepping_together",
    "cost_one_kernel<0, false>": "tests/test_hip_parity.py::test_single_pixel_entry_points",
    "cost_one_kernel<1, false>": "tests/test_hip_parity.py::test_single_pixel_entry_points",
    "cost_one_kernel<2, false>": "tests/test_hip_parity.py::test_dfkernel_single_pixel_and_mask",
    "cost_one_kernel<2, true>": "tests/test_hip_parity.py::test_dfkernel_single_pixel_and_mask",
    "corr_march_kernel<7, 4, 4, 2, 768, 3, 1>": "tests/test_hip_parity.py::test_wide_windows_take_the_marching_table_kernel",
}

# kernel -> why no test launches it
EXCLUDED = {
}


def _key(symbol):
    """'void umpa::foo_kernel<1, 2>(args)' -> 'foo_kernel<1, 2>'; 'umpa::bar_kernel(args)' -> 'bar_kernel'."""
    s = re.sub(r"^void ", "", symbol)
    s = s.split("(", 1)[0]
    return s.split("::", 1)[1] if "::" in s else s


@pytest.fixture(scope="module")
def inst():
    spec = importlib.util.spec_from_file_location("_inst", os.path.join(REPO, "tests", "test_hip_instantiations.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def symbols():
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_coverage
    finally:
        sys.path.pop(0)
    lib = os.path.join(REPO, "umpa_amd", "libumpa_hip.so")
    if not os.path.exists(lib):
        pytest.fail("umpa_amd/libumpa_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    try:
        return [_key(s) for s in kernel_coverage.kernel_symbols(lib)]
    except kernel_coverage.ToolMissing as e:
        pytest.fail(str(e))


def _claims(inst):
    """(claims that must each name a symbol, claims that name one only where the instantiation is compiled)"""
    strict = set(NAMED) | set(EXCLUDED)
    for names in inst.REACHES.values():
        strict |= set(names)
    optional = set()
    for names in inst.REACHES_WHERE_COMPILED.values():
        optional |= set(names)
    return strict, optional


def test_every_kernel_symbol_is_claimed(symbols, inst):
    strict, optional = _claims(inst)
    orphans = [s for s in symbols if s not in strict and s not in optional]
    assert not orphans, "%d kernel symbols no test claims (add a case to tests/test_hip_instantiations.py):\n  %s" % (
        len(orphans), "\n  ".join(orphans))


def test_every_claim_names_a_symbol(symbols, inst):
    have = set(symbols)
    strict, _ = _claims(inst)
    stale = sorted(strict - have)
    assert not stale, "claims that name no kernel of the library: %s" % stale
    # a forced corr_volume shape that is not compiled runs the fallback shape, which is compiled for every (Nw, UB) the
    # dispatch picks: each case's fallback names must exist
    for test, names in inst.REACHES_WHERE_COMPILED.items():
        Nw, ms = [int(x) for x in re.match(r".*\[Nw(\d+)-ms(\d+)\]", test).groups()]
        tail = inst.corr_tail(Nw, inst._ub(Nw, ms), inst.CORR_FALLBACK)
        for q in ("", "_queue"):
            assert "corr_volume%s_kernel%s" % (q, tail) in have and "corr_volume%s_kernel%s" % (q, tail) in names, (test, tail)


def test_dispatch_tables_mirror_the_source(inst):
    """The cases' copies of UMPA_CORR_SHAPES, launch_corr_shape's fallback, pick_ub's candidates and masked_ub."""
    src = open(TILED_H).read()
    m = re.search(r"#define UMPA_CORR_SHAPES\(X\)(.*)", src)
    assert m, "UMPA_CORR_SHAPES not found in umpa_tiled.h"
    shapes = {int(t[0]): tuple(int(x) for x in t[1:]) for t in re.findall(
        r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", m.group(1))}
    assert shapes == inst.CORR_SHAPES, "UMPA_CORR_SHAPES changed: give every shape id a case in test_corr_volume_every_shape " \
                                       "(CORR_SHAPES) -- source %s, cases %s" % (shapes, inst.CORR_SHAPES)
    body = src[src.index("inline hipError_t launch_corr_shape("):]
    body = body[:body.index("\n}\n")]
    fb = re.findall(r"return launch_corr<NW, UB, (\d+), (\d+), (\d+), (\d+), (\d+)>\(", body)
    assert len(fb) == 1, fb
    assert tuple(int(x) for x in fb[0]) + (1,) == inst.CORR_SHAPES[inst.CORR_FALLBACK], fb
    cand = re.search(r"inline int pick_ub\(int UJ\).*?const int cand\[\d+\] = \{([^}]*)\};", src, re.S)
    assert cand and tuple(int(x) for x in cand.group(1).split(",")) == inst.CORR_UB_CANDIDATES, cand and cand.group(1)
    mub = re.search(r"constexpr int masked_ub\(\) \{ return KIND == 1 \? \(NW <= (\d+) \? (\d+) : (\d+)\) : "
                    r"\(NW <= (\d+) \? (\d+) : (\d+)\); \}", src)
    assert mub, "masked_ub changed: update masked_ub in tests/test_hip_instantiations.py"
    n1, a1, b1, n0, a0, b0 = (int(x) for x in mub.groups())
    for Nw in range(1, 9):
        assert inst.masked_ub(1, Nw) == (a1 if Nw <= n1 else b1) and inst.masked_ub(0, Nw) == (a0 if Nw <= n0 else b0), Nw


def test_the_listing_sees_every_family(symbols):
    fams = {s.split("<", 1)[0] for s in symbols}
    assert {"corr_volume_kernel", "corr_volume_queue_kernel", "replay_walk_kernel", "match_direct_kernel",
            "corr_march_kernel", "corr_masked_kernel", "blur_tiles_kernel", "flat_correct_kernel"} <= fams, fams
    assert len(symbols) == len(set(symbols))
