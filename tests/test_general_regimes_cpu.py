"""
The general shift table over input regimes, bad pixels and the LDS limit, what can be checked without a GPU: the host sweep of
the kernel's footprint arithmetic (tests/general_addr_check.cpp over umpa_amd/csrc/umpa_general_geom.h) under AddressSanitizer
and UBSan, the staged / fallback list it prints against the restatement of tests/general_expect.py, the near-tie caps of the
regime inputs from extended precision alone, and the hit sets of the bad-pixel cases.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import general_expect as G
import grid_expect as GE


# ----------------------------------------------------------------------------- 1. the footprint arithmetic on the host

def test_footprint_arithmetic_sweep_under_the_sanitizers(tmp_path):
    """tests/general_addr_check.cpp: a host program of its own, built with AddressSanitizer and UBSan and run as it is.  Its
    case list is the authority on staged / fallback and the LDS bytes: general_expect.LDS_CASES is a copy of it, and
    general_expect.lds_geometry restates the formula."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "general_addr_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(REPO, "tests", "general_addr_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all in range" in out, out
    printed = [(tuple(int(x) for x in m.groups()[:6]), (m.group(7), int(m.group(8)))) for m in
               re.finditer(r"case Nw (\d+) ms (\d+) step (\d+) (\d+) mask (\d) ref (\d): (staged|fallback) (\d+)", out)]
    assert printed == G.LDS_CASES, printed
    for case, want in printed:
        assert G.lds_geometry(*case) == want, case
    total = re.search(r"(\d+) cases \((\d+) staged, (\d+) fallback\), (\d+) reads", out)
    assert total and int(total.group(1)) == 9 * 9 * 22 * 4 and int(total.group(2)) > 3000 and int(total.group(4)) > 10 ** 8, out


def test_the_issues_worked_cases_and_the_gpu_cases_at_the_limit():
    """Nw 1, ms 2, step (4, 4): footprints of 63^2 and 65^2 doubles, 65 656 bytes, 120 past the limit; (4, 3) staged; Nw 1,
    ms 1, (4, 4): 63 608 bytes, staged.  Every LIMIT_CASES row has a staged and a fallback step in the program's list."""
    table = dict(G.LDS_CASES)
    assert table[(1, 2, 4, 4, 0, 0)] == ("fallback", 65656) and 65656 - G.LDS_LIMIT == 120
    assert 8 * (63 * 63 + 1 + 65 * 65 + 1 + 9 + 2) == 65656
    assert table[(1, 2, 4, 3, 0, 0)][0] == "staged" and table[(1, 1, 4, 4, 0, 0)] == ("staged", 63608)
    for case in G.LIMIT_CASES:
        (a, na), (b, nb) = G.limit_listed(case)
        assert (a, b) == ("staged", "fallback") and na <= G.LDS_LIMIT < nb, case
    # the existing edge cases: (5, 5) is a fallback at every (Nw, ms) of EDGE_CASES, far past the limit
    for Nw, ms, _, _, _, assign, masked in G.EDGE_CASES:
        assert G.lds_geometry(Nw, ms, 5, 5, masked, assign == "ref") > ("fallback", 90000)


# ----------------------------------------------------------------------------- 2. the regime inputs

def test_regime_cases_meet_every_instantiation_and_both_modes():
    for r in G.REGIME_NAMES:
        mine = [c for c in G.REGIME_CASES if c[0] == r]
        assert {(k, mk) for _, s, k, _, mk in mine if s == "D"} == set(G.INSTANCES)
        assert sum(s == "edge" for _, s, _, _, _ in mine) == 1
    assert {a for _, _, _, a, _ in G.REGIME_CASES} == {"sam", "ref"}
    for inst in G.INSTANCES:                                         # ... and every instantiation both modes
        assert {a for _, s, k, a, mk in G.REGIME_CASES if (k, mk) == inst} == {"sam", "ref"}
    assert {(k, mk) for _, s, k, _, mk in G.REGIME_CASES if s == "edge"} == {(0, True), (1, False)}


@pytest.mark.parametrize("regime,stack,kind,assign,masked", G.REGIME_CASES, ids=G.REGIME_IDS)
def test_regime_near_tie_share_from_extended_precision(regime, stack, kind, assign, masked):
    """The cap is a condition on the inputs, not on the device.  Every pixel a frame contributes to has a finite cost at every
    shift (D's masks leave no window without a pair weight), well above its fp64 bound or not -- the bound is what the GPU
    test holds the kernel to."""
    v = G.regime_hp(regime, stack, kind, assign, masked)
    fin = np.isfinite(v["cost"].astype(np.float64))
    dead = v["sets"] == 0
    assert not fin[:, :, dead].any() and fin[:, :, ~dead].all()
    share, near = G.near_tie_share(v)
    with np.errstate(invalid="ignore"):
        rel = float((v["bound"][fin] / np.abs(v["cost"][fin])).max())
    print("%s %s kind %d %s masked %d: near-tie %d of %d, max bound / |cost| %.2e" % (regime, stack, kind, assign, masked, near.sum(), (~dead).sum(), rel))
    assert share <= GE.NEAR_TIE_CAP
    # the cells on which df does not admit the parity bar, from the reference's own a-priori bound
    case = G.REGIME_IDS[G.REGIME_CASES.index((regime, stack, kind, assign, masked))]
    if kind:
        loose = int((v["df_bound"][fin] > 1e-5).sum())
        assert loose == G.DF_LOOSE.get(case, 0) and loose <= 0.07 * fin.sum(), (case, loose)
    else:
        assert case not in G.DF_LOOSE


@pytest.mark.parametrize("kind,assign", G.MODES, ids=["%s-%s" % ("DF" if k else "NoDF", a) for k, a in G.MODES])
def test_weighted_masks_near_tie_share_and_distinct_weights(kind, assign):
    v = G.D_hp_weighted(kind, assign)
    fin = np.isfinite(v["cost"].astype(np.float64))
    dead = v["sets"] == 0
    assert not fin[:, :, dead].any() and fin[:, :, ~dead].all()
    share, near = G.near_tie_share(v)
    assert share <= GE.NEAR_TIE_CAP
    if kind:
        assert (v["df_bound"][fin] <= 1e-5).all()                     # df admits the parity bar at every cell
    w = np.concatenate([m.ravel() for m in G.D_weights()])
    assert 0.03 < (w == 0).mean() < 0.07 and len(np.unique(w)) > 0.9 * w.size       # no two weights alike (D_masks(): two values)


@pytest.mark.parametrize("which", sorted(G.REFUSED))
@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_refused_models_have_a_finite_expectation_everywhere(which, kind):
    """the two models the masked path refuses (test_hip_longlived_general.py): no cell without a pair weight and none that is
    rank-deficient in extended precision, so the a-priori bound judges every entry"""
    v = G.refused_hp(which, kind)
    assert np.isfinite(v["cost"].astype(np.float64)).all() and np.isfinite(v["bound"].astype(np.float64)).all()
    sam, _, _, Nw, ms = G.refused_inputs(which)
    assert (len(sam) * (2 * Nw + 1) ** 2 <= 9) == (which == "exact fit") and (Nw > 8) == (which == "no configuration")


# ----------------------------------------------------------------------------- 3. the bad-pixel hit sets

def test_bad_pixel_hit_sets():
    """By the frame-contribution rule (li >= pad, reach Nw + ms - 1 < pad) no contributing pixel's window reaches a frame's
    row 0 or column 0: the hit set is empty.  The last row and column are reached by the moving window alone, and only at the
    extreme shift; interior and seam are reached at every shift."""
    sam, _, pos, Nw, ms = G.D()
    U = 2 * ms - 1
    for assign in ("sam", "ref"):
        for where in ("sam", "ref"):
            moves = (where == "ref") == (assign == "sam")
            for name in ("row0", "col0"):
                assert not G.bad_hit(where, assign, *G.BAD_POSITIONS[name]).any()
            for name in ("interior", "seam"):
                assert G.bad_hit(where, assign, *G.BAD_POSITIONS[name]).any(axis=(2, 3)).all()
            for name, axis in (("last_row", 0), ("last_col", 1)):
                shifts = np.argwhere(G.bad_hit(where, assign, *G.BAD_POSITIONS[name]).any(axis=(2, 3)))
                if not moves:
                    assert shifts.size == 0
                    continue
                extreme = U - 1 if assign == "sam" else 0             # the window moves by +s in 'sam' mode, by -s in 'ref' mode
                assert shifts.shape[0] == U and (shifts[:, axis] == extreme).all(), (name, assign, where)
    k, r, c = G.BAD_POSITIONS["seam"]
    assert (r + pos[k][0] - (Nw + ms)) % 16 == 0                      # a workgroup seam of the output grid
    for k, r, c in G.BAD_POSITIONS.values():
        assert 0 <= r < sam[k].shape[0] and 0 <= c < sam[k].shape[1]
    kr, rr, _ = G.BAD_POSITIONS["last_row"]
    kc, _, cc = G.BAD_POSITIONS["last_col"]
    assert rr == sam[kr].shape[0] - 1 and cc == sam[kc].shape[1] - 1


# ----------------------------------------------------------------------------- 4. the claims of the GPU module

def test_the_gpu_modules_claims_name_kernels_and_tests_that_exist():
    """tests/test_hip_general_regimes.py's REACHES: every general_table_kernel instantiation is claimed by every test of the
    table, no claim names a kernel the library does not have, and every key is a test of the module"""
    from nativelibs import build_all, gpu_test_module, kernel_keys
    g = build_all()
    keys = set(kernel_keys(g.GRID_LIB))
    mod = gpu_test_module("general_regimes")
    want = {k for k in keys if k.split("<", 1)[0] == "general_table_kernel"}
    assert len(want) == 4
    for test, names in mod.REACHES.items():
        path, name = test.split("::")
        assert path == "tests/test_hip_general_regimes.py" and callable(getattr(mod, name)), test
        assert set(names) <= keys and (want <= set(names) or "weighted" in name), (test, sorted(set(names) - keys))
