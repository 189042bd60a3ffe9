"""
The exhaustive grid search and the cost volume, what can be checked without a GPU: the expectation the GPU tests use
(tests/grid_expect.py), the admissibility of their inputs, and the second library's build.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO, Case

import grid_expect as GE
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
FAMILIES = ("grid_min_kernel", "cost_volume_kernel")


# ----------------------------------------------------------------------------- 1. the helper is right

PERTURB = 1e-13                 # relative noise put on a 4x4 entry.  The reference for it is the agreement this test itself asserts
                                # between the oracle's fp64 4x4 and the helper's extended-precision one: 1e-12 of the largest entry.
                                # A tenth of that, so the exemption is narrower than the asserted agreement alone would allow.


def _oracle_fit_is_sensitive(a16, memo25, tol=1e-10):
    """Does the ORACLE's own sub-pixel fit, on its own 4x4, move by more than `tol` when the entries are scaled by
    (1 +- PERTURB)?  (Eight fixed sign patterns, as oracle.parity.newton_unstable; nothing of the helper enters.)"""
    from oracle.parity import _spmin_from_start
    a = np.ascontiguousarray(a16, dtype=np.float64)
    p0 = _spmin_from_start(a, memo25)
    rng = np.random.default_rng(12345)
    for _ in range(8):
        p = _spmin_from_start(a * (1.0 + PERTURB * rng.choice([-1.0, 1.0], size=a.shape)), memo25)
        if np.any(~(np.abs(p - p0) <= tol * np.maximum(1.0, np.abs(p0)))):
            return True
    return False


@pytest.mark.parametrize("name,modes", [("A_small", (-1, 0, 1)), ("F8_C2_crop", (-1,))], ids=["A_small", "F8_C2_crop"])
def test_helper_agrees_with_the_walk_where_the_walk_found_the_global_minimum(name, modes, port_ns):
    """The pixels: err == 1 in the oracle's walk and the walk's integer minimum (dy, dx of a sub_pixel_mode-0 run: the centre
    of its memo) IS the helper's argmin -- nothing else selects them.  There the helper must report err == 1 too, its 4x4
    must be the walk's (to 1e-12 of the largest entry: extended precision rounded to fp64 against fp64), and dx, dy, f agree to
    1e-10.  The quadratic fit (mode 1) and mode 0 are closed forms: no miss is admitted.  The reference's Newton iteration
    (mode -1: at most 21 undamped steps, stops at a step of 1e-4 px, Optim.cpp:91-124) does not define its answer to 1e-10 on
    every 4x4: a miss is admitted only where the ORACLE's own fit on its own 4x4 moves by more than 1e-10 under rounding
    noise of the inputs (_oracle_fit_is_sensitive; the helper has no say in that), and the misses beyond the project's
    parity bar of 1e-5 must also be classified by oracle.parity and stay within its allowance of 0.2 % (at least 2).
    Seen: A_small mode -1: 9 of 1816 pixels, exactly the 9 the oracle itself cannot reproduce (eight between 1.7e-7 and
    8e-6 px, one at 0.59 px); modes 0, 1 and F8_C2_crop: none.
    And the helper's minimum is a minimum: no cell any walk has seen lies below it by more than the fp64 bound of the
    helper's own cell (the memo holds fp64 evaluations, the helper's cost is the extended-precision one: they differ by up
    to that bound on the very same cell)."""
    from oracle.parity import newton_unconverged, newton_unstable, unconverged_cap
    c = Case(name)
    v = next(v for v in c.variants if v["model"] in ("UMPAModelDF", "UMPAModelNoDF") and "dxdy" not in v
             and "step" not in v and "ROI" not in v and "Nw_set" not in v)
    kind = 1 if v["model"] == "UMPAModelDF" else 0
    assign = v.get("assign", "sam")
    m = getattr(port_ns, v["model"])(c.sam, c.ref, window_size=c.Nw, max_shift=c.max_shift)
    m.assign_coordinates = assign
    m.sub_pixel_mode = 0
    walk0 = m.match(quiet=True)                                       # dy, dx: the walk's integer minimum
    for subpx in modes:
        m.sub_pixel_mode = subpx
        walk = m.match(quiet=True)
        exp, near = GE.expected(kind, c.sam, c.ref, m.window, c.max_shift, m.padding, assign, subpx)
        same = (walk["err"] == 1) & (walk0["dy"] == exp["ci"]) & (walk0["dx"] == exp["cj"])
        assert same.sum() > 0.5 * same.size, "%d of %d pixels comparable" % (same.sum(), same.size)
        assert np.all(exp["err"][same] == 1) and np.all(exp["debug_Ncalls"] == (2 * c.max_shift - 1) ** 2)
        scale = np.abs(walk["debug_a"]).max(axis=-1, keepdims=True)
        assert np.all((np.abs(walk["debug_a"] - exp["debug_a"]) <= 1e-12 * scale)[same]), "the helper's 4x4 is not the walk's"
        d = np.zeros(same.shape)
        for k in ("dx", "dy", "f"):
            d = np.maximum(d, np.abs(walk[k] - exp[k]) / np.maximum(1.0, np.abs(walk[k])))
        miss = same & ~(d <= 1e-10)
        if subpx != -1:
            assert not miss.any(), "%s subpx %d: %d pixels differ, worst %.2e" % (name, subpx, miss.sum(), d[same].max())
        for xi, xj in np.argwhere(miss):
            a16, memo = walk["debug_a"][xi, xj], walk["debug_d"][xi, xj]
            assert _oracle_fit_is_sensitive(a16, memo), \
                "%s (%d,%d): differs by %.2e although the oracle's own fit is reproducible there" % (name, xi, xj, d[xi, xj])
            if d[xi, xj] > 1e-5:
                assert newton_unconverged(a16, memo) or newton_unstable(a16, memo), (name, xi, xj, d[xi, xj])
        far = int((miss & (d > 1e-5)).sum())
        assert far <= unconverged_cap("", int(same.sum())), "%d pixels beyond 1e-5" % far
        known = walk0["debug_d"] >= 0
        below = known & (walk0["debug_d"] < (exp["cmin"] - exp["cmin_bound"]).astype(np.float64)[..., None])
        assert not below.any(), "%d memo cells below the helper's minimum" % below.sum()
        print("%s subpx %d: %d of %d pixels compared, %d not reproducible by the oracle itself (%d beyond 1e-5), walk elsewhere than "
              "the global minimum on %.2f %% of its ok pixels" % (name, subpx, same.sum(), same.size, miss.sum(), far,
                                                                 100.0 * np.mean(~same[walk["err"] == 1])))


# ----------------------------------------------------------------------------- 2. the GPU tests' inputs are admissible

@pytest.mark.parametrize("name", sorted(GE.STACKS))
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("assign", ["sam", "ref"])
def test_gpu_inputs_have_few_near_ties(name, kind, assign):
    exp, near = GE.expected_for(name, kind, assign, 0)
    share = near.mean()
    print("%s kind %d %s: near-tie share %.4f %%, ok pixels %d of %d" % (name, kind, assign, 100 * share, exp["err"].sum(), near.size))
    assert share <= GE.NEAR_TIE_CAP
    assert exp["err"].sum() > 0.5 * near.size and (exp["err"] == 0).any()       # both outcomes are exercised


# ----------------------------------------------------------------------------- 3. the library builds

def test_grid_library_builds_and_its_kernels_are_claimed():
    _build()
    assert os.path.exists(GRID_LIB)
    from umpa_amd import _lib
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS) and len(declared("umpa_grid.h", "umpa_grid_")) >= 2
    _lib.hip()
    lib = ctypes.CDLL(GRID_LIB)
    for name in declared("umpa_grid.h", "umpa_grid_"):
        assert hasattr(lib, name), name
    assert _lib.grid().path == GRID_LIB
    syms = [k for k in kernel_keys(GRID_LIB) if k.split("<", 1)[0] in FAMILIES]
    assert {s.split("<", 1)[0] for s in syms} == set(FAMILIES), syms
    assert_claimed(syms, "grid")


# ----------------------------------------------------------------------------- 4. the main library: the hook, nothing else

def test_main_library_exports_the_consumer_setter_and_no_new_public_symbol():
    _build()
    import __graft_entry__ as g
    from umpa_amd import _lib
    names = exported(g.HIP_LIB)
    assert "umpa_hipx_set_table_consumer" in names
    public = sorted(n for n in names if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS), set(public) ^ set("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    hdr = open(os.path.join(REPO, "include", "umpa_hip.h")).read()
    assert "umpa_hipx" not in hdr and "consumer" not in hdr
    # the grid library exports its C ABI and nothing else of its own
    own = sorted(n for n in exported(GRID_LIB) if n.startswith("umpa"))
    assert own == declared("umpa_grid.h", "umpa_grid_"), own
