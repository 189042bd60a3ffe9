"""
Phase integration, what can be checked without a GPU: the fifth library's build and symbol sets, the restatement the GPU
tests use (tests/integrate_expect.py) against a dense least-squares solve, the properties of the operation on the
restatement (a ramp, garbage at weight 0), the argument errors and the library's error without a GPU.

tests/golden/integrate_observed.json records, per case, the worst component-demeaned deviation of the restated solve from
the dense solve and its iteration count: the yardstick of tests/test_hip_integrate.py.  tests/golden/integrate_dense.npz
keeps the dense solutions, so that the GPU tests need not solve them again; both are written by
tests/golden/make_golden_integrate.py and checked here against a live dense solve.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from conftest import REPO

import integrate_expect as E
from nativelibs import assert_claimed, build_all as _build, declared as _declared, exported, kernel_keys

INTEGRATE_LIB = os.path.join(REPO, "umpa_amd", "libumpa_integrate.so")

def _module():
    return importlib.import_module("umpa_amd.integrate")


# ----------------------------------------------------------------------------- 1. the library builds

def test_build_produces_the_integrate_library_with_the_declared_symbols():
    g = _build()
    assert g.INTEGRATE_LIB == INTEGRATE_LIB and os.path.exists(INTEGRATE_LIB)
    from umpa_amd import _lib
    declared = _declared("umpa_integrate.h", "umpa_integrate_")
    assert declared == sorted("umpa_integrate_" + s for s in _lib.INTEGRATE_SYMBOLS) and len(declared) == 3
    own = sorted(n for n in exported(INTEGRATE_LIB) if n.startswith("umpa"))
    assert own == declared, own                                       # its C ABI and nothing else of its own
    _lib.hip()
    lib = ctypes.CDLL(INTEGRATE_LIB)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.integrate().path == INTEGRATE_LIB
    hdr = open(os.path.join(REPO, "include", "umpa_integrate.h")).read()
    for name in ("F_NO_TAIL", "F_JACOBI", "F_DEBUG", "CONVERGED", "MAXITER", "BREAKDOWN", "CHECK_EVERY"):
        assert int(re.search(r"#define UMPA_INTEGRATE_%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, "INTEGRATE_" + name), name
    I = _module()
    assert (I.CONVERGED, I.MAXITER, I.BREAKDOWN) == (E.CONVERGED, E.MAXITER, E.BREAKDOWN)
    src = open(os.path.join(REPO, "umpa_amd", "csrc", "umpa_integrate.hip")).read()
    assert "umpa_tiled.h" not in src
    for name, val in (("OMEGA", E.OMEGA), ("NU", E.NU), ("COARSE_SWEEPS", E.COARSE_SWEEPS), ("COARSEST", E.COARSEST)):
        assert float(re.search(r"constexpr \w+ %s = ([0-9.]+);" % name, src).group(1)) == val, name


def test_every_integrate_kernel_is_claimed_by_a_gpu_test():
    _build()
    syms = kernel_keys(INTEGRATE_LIB)
    mod = assert_claimed(syms, "integrate")
    for test in mod.REACHES:
        assert hasattr(mod, test.split("::")[1]), test


# ----------------------------------------------------------------------------- 2. the restatement

def test_restriction_is_the_transpose_of_prolongation():
    rng = np.random.default_rng(0)
    for sh in E.SHAPES + E.SMALL + [(6, 7), (8, 8)]:
        r, e = rng.standard_normal(sh), rng.standard_normal(E.coarse_shape(sh))
        lhs, rhs = (E.restrict(r) * e).sum(), (r * E.prolong(e, sh)).sum()
        assert abs(lhs - rhs) <= 1e-13 * (np.abs(r).sum() + np.abs(e).sum()), sh
        np.testing.assert_array_equal(E.prolong(np.ones(E.coarse_shape(sh)), sh), np.ones(sh))   # P keeps constants


def test_the_vcycle_is_a_symmetric_operator():
    rng = np.random.default_rng(1)
    for name in ("33x47_holes", "17x300_ones"):
        gx, gy, w, _ = E.case(name)
        lv = E.levels(E.weights0(gx, gy, w))
        u, v = rng.standard_normal(w.shape), rng.standard_normal(w.shape)
        a, b = (u * E.vcycle(lv, v)).sum(), (v * E.vcycle(lv, u)).sum()
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0), name


@pytest.mark.parametrize("kind", ["ones", "holes"])
@pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restated_pcg_against_the_dense_solve(shape, kind):
    """The restated solve at tol = 1e-10 against np.linalg.lstsq on the assembled L, component by component.  The recorded
    deviation is what this deterministic restatement gives; a live dense solve may differ from the recorded one by its own
    error, 4 cond(L) 2^-53 max |Phi| (integrate_expect.dense_error: 2e-12 .. 8e-11 here), and that is all the slack there is."""
    name = E.case_name(shape, kind)
    gx, gy, w, _ = E.case(name)
    phi, it, resid, status = E.pcg(gx, gy, w if kind == "holes" else None)
    rec = E.observed()[name]
    live = E.dense_live(name)
    on = np.isfinite(live)
    drift = np.abs(live[on] - E.dense(name)[on]).max()
    dev = E.deviation(phi, name, ref=live)
    dense_err = E.dense_error(name)
    print("%s: %d iterations (recorded %d), residual %.2e, deviation from the dense solve %.3e (recorded %.3e), live against recorded dense %.1e, dense error %.1e"
          % (name, it, rec["iterations"], resid, dev, rec["deviation"], drift, dense_err))
    assert status == E.CONVERGED and resid <= 1e-10 and it < 500
    assert it == rec["iterations"]
    assert (np.isfinite(E.dense(name)) == on).all() and drift <= dense_err
    assert dev <= rec["deviation"] + dense_err
    assert dense_err < 2e-10 and rec["deviation"] < 1e-8              # the reference is sharp enough; tol * range * a factor of 20 at most


def test_a_linear_ramp_is_recovered_up_to_its_mean():
    H, W, c1, c2 = 33, 47, 0.37, -1.25
    gx, gy = np.full((H, W), c1), np.full((H, W), c2)
    phi, it, resid, status = E.pcg(gx, gy)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ramp = c1 * j + c2 * i
    ramp = ramp - ramp.mean()
    # L (phi - ramp) = -(b - L phi): |error|_2 <= |residual|_2 / lambda_2, lambda_2 = 2 - 2 cos(pi / max(H, W)) of the grid
    b = E.rhs(np.ones((H, W)), gx, gy)
    bound = resid * E.lnorm(b) / (2.0 - 2.0 * np.cos(np.pi / max(H, W)))
    err = np.sqrt(((phi - ramp) ** 2).sum())
    print("ramp: %d iterations, residual %.2e, |phi - ramp|_2 = %.2e, bound %.2e" % (it, resid, err, bound))
    assert status == E.CONVERGED and resid <= 1e-10 and bound < 1e-6
    assert err <= bound + 1e-12 * np.abs(ramp).max()


def test_garbage_at_weight_zero_changes_nothing_and_nan_reaches_no_output():
    gx, gy, w, _ = E.case("33x47_holes")
    off = w == 0
    assert off.any() and np.isnan(gx[off]).all()
    a = E.pcg(gx, gy, w)
    gx2, gy2 = gx.copy(), gy.copy()
    gx2[off], gy2[off] = 1e30, -np.inf
    b = E.pcg(gx2, gy2, w)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1:] == b[1:]
    d = E.diag(E.weights0(gx, gy, w))
    assert np.isfinite(a[0][d > 0]).all() and np.isnan(a[0][d == 0]).all() and (d == 0).any()
    c = E.pcg(gx, gy, None)                                           # without w the non-finite pixels are the weight-0 ones
    assert np.isfinite(c[0][E.diag(E.weights0(gx, gy, None)) > 0]).all() and c[3] == E.CONVERGED


def test_hole_cases_stay_below_maxiter_and_beat_jacobi():
    obs = E.observed()
    for name, rec in obs.items():
        assert rec["iterations"] < 500, name
    gx, gy, w, _ = E.case("33x47_holes")
    jac = E.pcg(gx, gy, w, maxiter=3000, jacobi=True)
    assert jac[3] == E.CONVERGED and jac[1] > 4 * obs["33x47_holes"]["iterations"]


# ----------------------------------------------------------------------------- 3. argument errors, no CPU fallback

def test_python_argument_errors():
    _build()
    I = _module()
    g = np.zeros((20, 30))
    with pytest.raises(ValueError, match="does not match"):
        I.integrate(g, np.zeros((20, 31)))
    with pytest.raises(ValueError, match="does not match"):
        I.integrate(g, g, weight=np.ones((30, 20)))
    with pytest.raises(ValueError, match=r"\[H, W\] or \[K, H, W\]"):
        I.integrate(np.zeros(30), np.zeros(30))
    with pytest.raises(ValueError, match="at least 2 x 2"):
        I.integrate(np.zeros((1, 30)), np.zeros((1, 30)))
    with pytest.raises(ValueError, match="finite and >= 0"):
        w = np.ones((20, 30)); w[3, 4] = -1e-300
        I.integrate(g, g, weight=w)
    with pytest.raises(ValueError, match="finite and >= 0"):
        w = np.ones((20, 30)); w[0, 0] = np.nan
        I.integrate(g, g, weight=w)
    with pytest.raises(ValueError, match="tol"):
        I.integrate(g, g, tol=-1.0)
    with pytest.raises(ValueError, match="maxiter"):
        I.integrate(g, g, maxiter=-1)
    with pytest.raises(ValueError, match="finite and >= 0"):
        I.vcycle(g, weight=np.full((20, 30), np.inf))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        I.vcycle(np.zeros((2, 20, 30)))
    res = {"dx": g, "dy": g, "err": np.ones((20, 30)), "f": g}
    with pytest.raises(ValueError, match="'err', 'f' or an array"):
        I.phase_from_match(res, weight="df")
    with pytest.raises(ValueError, match="does not match the maps"):
        I.phase_from_match(res, weight=np.ones((3, 3)))


def test_match_weights():
    I = _module()
    rng = np.random.default_rng(2)
    dx, dy, f = rng.standard_normal((3, 6, 7))
    f = np.abs(f)
    err = np.ones((6, 7)); err[1, 2] = 0; err[4, 4] = 2
    dx[0, 0] = np.nan
    res = {"dx": dx, "dy": dy, "err": err, "f": f}
    ok = (err == 1) & np.isfinite(dx)
    np.testing.assert_array_equal(I.match_weight(res, "err"), ok.astype(float))
    wf = I.match_weight(res, "f")
    np.testing.assert_array_equal(wf, np.where(ok, 1.0 / (f + np.median(f[ok])), 0.0))
    assert (wf[ok] > 0).all() and ok.sum() == 39


def test_c_abi_argument_errors_come_before_any_device_work():
    _build()
    from umpa_amd import _lib
    lib = _lib.integrate()
    vp = ctypes.c_void_p
    g = np.zeros((20, 30)); phi = np.zeros((20, 30))
    it, st, res = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1)
    w = np.ones((20, 30)); w[5, 6] = -1.0

    def solve(H=20, W=30, wv=None, K=1, tol=1e-10, maxiter=5, flags=0, gxp=g):
        return lib.solve(gxp.ctypes.data_as(vp) if gxp is not None else None, g.ctypes.data_as(vp), wv.ctypes.data_as(vp) if wv is not None else None,
                         K, H, W, tol, maxiter, 0.0, phi.ctypes.data_as(vp), it.ctypes.data_as(vp), res.ctypes.data_as(vp),
                         st.ctypes.data_as(vp), 0, flags, None)

    def vc(H=20, W=30, wv=None, flags=0):
        return lib.vcycle(wv.ctypes.data_as(vp) if wv is not None else None, g.ctypes.data_as(vp), phi.ctypes.data_as(vp), H, W, 0, flags, None)

    E_ARG = -1
    assert solve(H=1) == E_ARG and "H, W >= 2" in lib.error()
    assert solve(W=0) == E_ARG and solve(K=-1) == E_ARG and solve(gxp=None) == E_ARG
    assert solve(wv=w) == E_ARG and "pixel (5, 6)" in lib.error()
    assert solve(tol=-1.0) == E_ARG and solve(tol=float("nan")) == E_ARG and solve(maxiter=-1) == E_ARG
    assert solve(flags=2) == E_ARG and solve(flags=2048) == E_ARG
    assert solve(H=65536, W=32768) == E_ARG and "2^31" in lib.error()
    assert vc(H=1) == E_ARG and vc(wv=w) == E_ARG and "pixel (5, 6)" in lib.error() and vc(flags=4) == E_ARG


def test_without_a_gpu_the_librarys_error_is_raised():
    _build()
    from umpa_amd import _lib
    I = _module()
    g = np.ones((20, 30))
    if _lib.hip().device_count() > 0:                                 # a GPU is present: the same call must then succeed
        res = I.integrate(g, g)
        assert res.status == I.CONVERGED and res.phi.shape == (20, 30)
        return
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        I.integrate(g, g)
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        I.vcycle(g)
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        I.phase_from_match({"dx": g, "dy": g, "err": g, "f": g})


def test_the_package_reexports_the_names():
    import umpa_amd
    I = _module()
    for name in ("integrate", "vcycle", "phase_from_match", "Integration"):
        assert getattr(umpa_amd, name) is getattr(I, name) and name in umpa_amd.__all__
    assert (I.Integration.CONVERGED, I.Integration.MAXITER, I.Integration.BREAKDOWN) == (0, 1, 2)
    assert "2 pi p^2 / (lambda z)" in I.phase_from_match.__doc__ and "sam[i, j] = ref[i + dy, j + dx]" in I.phase_from_match.__doc__
