"""
The directional dark-field search, what can be checked without a GPU: the sixth library's build and symbol sets, the host
functions of umpa_amd.ddf against the restatement (tests/ddf_expect.py), the restatement's fold against a brute-force loop,
the IDENTITY the whole feature rests on (the kernel model with one (a, b, c) everywhere is the plain model on the blurred
reference, 8 pixels further in) on both CPU checkers, the recorded reference maps (tests/golden/K_ddf.npz), the recovery
case's own quality, and the refusals that need no GPU.

The cap on unconverged-Newton pixels.  The two sides of the identity see blurred references that differ in the last bits
(one blur is rounded once from extended precision, the other is the model's own fp64 chain), so pixels whose Newton
iteration is not converged may differ; assert_parity classifies each one.  Their share is capped at what the suite allows
the plain model at this configuration (3 frames, Nw = 2: tests/test_hip_fuzz.py::_illposed_share, 1.2 %).  Where the
reference's own build is one of the sides, `f` of failed pixels is not compared, as in tests/test_oracle_golden.py (the
reference returns an uninitialised value there).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, assert_parity

import ddf_expect as DE
from nativelibs import assert_claimed, build_all as _build, declared as _declared, exported, kernel_keys

DDF_LIB = os.path.join(REPO, "umpa_amd", "libumpa_ddf.so")
ILLPOSED = 0.012


# ----------------------------------------------------------------------------- 1. the library builds

def test_build_produces_the_ddf_library_with_the_declared_symbols():
    g = _build()
    assert g.DDF_LIB == DDF_LIB and os.path.exists(DDF_LIB)
    from umpa_amd import _lib
    declared = _declared("umpa_ddf.h", "umpa_ddf_")
    assert declared == sorted("umpa_ddf_" + s for s in _lib.DDF_SYMBOLS) and len(declared) == 4
    own = sorted(n for n in exported(DDF_LIB) if n.startswith("umpa"))
    assert own == declared, own                                       # its C ABI and nothing else of its own
    _lib.hip()
    lib = ctypes.CDLL(DDF_LIB)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.ddf().path == DDF_LIB
    hdr = open(os.path.join(REPO, "include", "umpa_ddf.h")).read()
    for name, value in (("TAPS", _lib.DDF_TAPS), ("HALF", _lib.DDF_HALF), ("MAX_FRAMES", _lib.DDF_MAX_FRAMES)):
        assert int(re.search(r"#define UMPA_DDF_%s (\d+)" % name, hdr).group(1)) == value
    assert (DE.TAPS, DE.HALF) == (_lib.DDF_TAPS, _lib.DDF_HALF)


def test_every_ddf_kernel_is_claimed_by_a_gpu_test():
    _build()
    syms = kernel_keys(DDF_LIB)
    assert sorted(syms) == ["ddf_blur_kernel<false>", "ddf_blur_kernel<true>", "ddf_fold_kernel"], syms
    mod = assert_claimed(syms, "ddf")
    for test in mod.REACHES:
        assert hasattr(mod, test.split("::")[1]), test


# ----------------------------------------------------------------------------- 2. host functions against the restatement

@pytest.mark.parametrize("abc", DE.BLUR_KERNELS + DE.KERNELS[3:], ids=str)
def test_gaussian_kernel_equals_the_restatement_and_sums_to_one(abc):
    _build()
    from umpa_amd import ddf
    g, e = ddf.gaussian_kernel(*abc), DE.kernel(*abc)
    assert g.shape == (17, 17) and g.dtype == np.float64
    # the same expression in the same order; libm's exp and numpy's may differ in the last bit, the sum of 289 terms with them
    np.testing.assert_allclose(g, e, rtol=1e-13, atol=0)
    assert abs(g.sum() - 1.0) < 289 * 2.0 ** -52
    assert g[8, 8] == g.max() and (g >= 0).all()
    np.testing.assert_array_equal(g, g[::-1, ::-1])                   # the exponent is even in (i, j)
    if abc[1] != 0:
        assert g[9, 9] != g[9, 7]                                     # b couples rows and columns: k is the row
        assert (g[9, 9] < g[9, 7]) == (abc[1] > 0)


def test_widths_and_angle_round_trip():
    _build()
    from umpa_amd import ddf
    rng = np.random.default_rng(3)
    for _ in range(50):
        sM = rng.uniform(0.5, 4.0)
        sm = sM * rng.uniform(0.2, 0.95)
        th = rng.uniform(0, np.pi)
        abc = ddf.kernel_from_sigma(sM, sm, th)
        np.testing.assert_allclose(abc, DE.kernel_from_sigma(sM, sm, th), rtol=1e-12, atol=1e-15)
        assert DE.admissible(*abc)
        np.testing.assert_allclose(ddf.sigma_from_kernel(*abc), (sM, sm, th), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(DE.sigma_from_kernel(*abc), (sM, sm, th), rtol=1e-10, atol=1e-10)
    # the axes: theta = 0 blurs along the rows (a small), pi / 2 along the columns (c small); isotropic: theta = 0
    a, b, c = ddf.kernel_from_sigma(2.0, 0.6, 0.0)
    assert a < c and b == 0
    a, b, c = ddf.kernel_from_sigma(2.0, 0.6, np.pi / 2)
    assert a > c and abs(b) < 1e-15
    s1, s2, t = ddf.sigma_from_kernel(0.2, 0.0, 0.2)
    assert s1 == s2 == pytest.approx(np.sqrt(2.5), rel=1e-14) and t == 0.0
    g = ddf.gaussian_kernel(*ddf.kernel_from_sigma(2.0, 0.6, np.pi / 4))
    assert g[10, 10] > g[10, 6]                                       # the major axis runs along (+i, +j)
    # the angle stays in [0, pi)
    for th in (0.0, 1e-9, np.pi - 1e-9, np.pi / 2):
        t = ddf.sigma_from_kernel(*ddf.kernel_from_sigma(2.0, 1.0, th))[2]
        assert 0.0 <= t < np.pi


def test_sigma_from_kernel_works_on_maps_with_nan():
    _build()
    from umpa_amd import ddf
    sM = np.array([[2.0, 1.5, 3.0], [1.0, 2.5, 0.7]])
    sm = np.array([[0.6, 1.5, 1.0], [0.5, 2.0, 0.7]])
    th = np.array([[0.3, 0.0, 2.0], [1.0, 3.0, 0.0]])
    a, b, c = ddf.kernel_from_sigma(sM, sm, th)
    assert a.shape == sM.shape
    a[0, 2] = b[0, 2] = c[0, 2] = np.nan                              # a pixel where every candidate failed
    a2, b2, c2 = a.copy(), b.copy(), c.copy()
    b2[1, 0] = 10.0                                                   # and one that is no Gaussian
    s1, s2, t = ddf.sigma_from_kernel(a2, b2, c2)
    bad = np.zeros(sM.shape, dtype=bool)
    bad[0, 2] = bad[1, 0] = True
    for got, want in ((s1, sM), (s2, sm), (t, th)):
        assert np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any()
        np.testing.assert_allclose(got[~bad], want[~bad], rtol=1e-10, atol=1e-10)
    with pytest.raises(ValueError, match="s_major >= s_minor > 0"):
        ddf.kernel_from_sigma(1.0, 2.0, 0.0)


def test_every_row_of_candidate_grid_is_admissible():
    _build()
    from umpa_amd import ddf
    cand = ddf.candidate_grid([0.6, 1.0, 2.0, 3.5], [1.0, 0.6, 0.25], 6)
    assert cand.shape == (4 * (1 + 2 * 6), 3) and cand.dtype == np.float64
    assert all(DE.admissible(*row) for row in cand)
    assert len({tuple(np.round(row, 12)) for row in cand}) == len(cand)    # no candidate twice
    s1, s2, th = ddf.sigma_from_kernel(cand[:, 0], cand[:, 1], cand[:, 2])
    assert set(np.round(s1, 9)) == {0.6, 1.0, 2.0, 3.5} and (th >= 0).all() and (th < np.pi).all()
    for row in cand:
        ddf.gaussian_kernel(*row)
    with pytest.raises(ValueError, match="ratios in"):
        ddf.candidate_grid([1.0], [1.5], 4)
    with pytest.raises(ValueError, match="n_angles"):
        ddf.candidate_grid([1.0], [0.5], 0)


# ----------------------------------------------------------------------------- 3. the restatement itself

def test_fold_restatement_matches_a_brute_force_argmin():
    planes = DE.hand_made_planes()
    got, want = DE.fold(planes), DE.fold_brute(planes)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["index"].dtype == np.int32 and got["err"].dtype == np.int32
    assert (got["index"][1, :3] == -1).all() and (got["err"][1, :3] == 0).all()
    assert (got["index"][0, :][np.stack([p["err"][0] for p in planes]).any(axis=0)] > 0).all()
    assert got["index"][2, 0] == 0
    # against an independent argmin where it is unambiguous: no NaN among the valid costs
    F = np.stack([np.where(p["err"] == 1, p["f"], np.inf) for p in planes])
    valid = np.stack([p["err"] == 1 for p in planes])
    clean = ~np.isnan(F).any(axis=0) & valid.any(axis=0)
    np.testing.assert_array_equal(got["index"][clean], np.argmin(F, axis=0)[clean])   # argmin takes the FIRST minimum
    # one candidate: untouched
    one = DE.fold(planes[:1])
    for k in ("f", "T", "dx", "dy", "err"):
        np.testing.assert_array_equal(one[k], planes[0][k])


def test_blur_restatement_on_hand_made_frames():
    g = DE.kernel(0.5, 0.2, 0.3)
    flat = np.full((20, 23), 3.25)
    out, bound = DE.blur_exact(flat, g)
    assert np.abs(out - 3.25).max() <= bound.max() and bound[8:-8, 8:-8].min() > 0 and bound[0, 0] == 0
    one = np.zeros((17, 19))
    one[8, 9] = 1.0                                                   # a delta: the flipped kernel appears around it
    out, _ = DE.blur_exact(one, g)
    assert out[8, 8] == g[8, 9] and out[8, 10] == g[8, 7] and out[8, 9] == g[8, 8]
    assert out[0, 0] == 0 and out[8, 9 + 1] != 0


# ----------------------------------------------------------------------------- 4. the identity, the recorded reference

@pytest.fixture(scope="module")
def namespaces(port_ns):
    from oracle import cpu_model
    return {"port": port_ns, "ref": cpu_model.ref if cpu_model.have_ref() else None}


@pytest.mark.parametrize("which", ["port", "ref"])
@pytest.mark.parametrize("n", range(len(DE.KERNELS)))
def test_identity_uniform_kernel_model_is_the_plain_model_on_the_blurred_reference(namespaces, which, n):
    ns = namespaces[which]
    if ns is None:
        pytest.skip("oracle/_ref/libumpa_ref.so not built")
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    left = DE.dfkernel_uniform(ns, sam, ref, DE.KERNELS[n], p["Nw"], p["max_shift"])
    right = DE.nodf_on_blurred(ns, sam, ref, DE.KERNELS[n], p["Nw"], p["max_shift"])
    np.testing.assert_array_equal(left["err"], right["err"])
    np.testing.assert_array_equal(left["debug_Ncalls"], right["debug_Ncalls"])
    ok = left["err"] == 1
    assert ok.sum() > 400
    assert np.abs(left["T"] - right["T"])[ok].max() < 1e-14
    st = assert_parity(right, left, p["max_shift"], "ddf identity %s %d" % (which, n), allow_illposed=ILLPOSED, f_on_failed=which == "port")
    print("identity %s %r: %d ok, %d unconverged" % (which, DE.KERNELS[n], st["ok"], st["unconverged"]))


@pytest.mark.parametrize("which", ["port", "ref"])
def test_identity_with_reference_coordinates_and_a_stepped_roi(namespaces, which):
    ns = namespaces[which]
    if ns is None:
        pytest.skip("oracle/_ref/libumpa_ref.so not built")
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    assert DE.shifted(DE.STEPPED) == ((11, 41, 3), (10, 48, 2))
    left = DE.dfkernel_uniform(ns, sam, ref, DE.KERNELS[1], p["Nw"], p["max_shift"], DE.STEPPED, "ref")
    right = DE.nodf_on_blurred(ns, sam, ref, DE.KERNELS[1], p["Nw"], p["max_shift"], DE.STEPPED, "ref")
    assert left["err"].shape == (10, 19)
    np.testing.assert_array_equal(left["err"], right["err"])
    np.testing.assert_array_equal(left["debug_Ncalls"], right["debug_Ncalls"])
    assert_parity(right, left, p["max_shift"], "ddf identity stepped " + which, allow_illposed=ILLPOSED, f_on_failed=which == "port")


def test_golden_file_holds_the_identity_stack_and_is_small():
    g = DE.golden()
    sam, ref = DE.identity_stack()
    np.testing.assert_array_equal(g["sam"], sam)
    np.testing.assert_array_equal(g["ref"], ref)
    assert os.path.getsize(DE.GOLDEN) <= os.path.getsize(os.path.join(REPO, "tests", "golden", "J_register.npz"))
    import json
    meta = json.loads(str(g["meta"]))
    assert [tuple(v["abc"]) for v in meta["variants"]] == [v[0] for v in DE.GOLDEN_VARIANTS]


@pytest.mark.parametrize("n", range(len(DE.GOLDEN_VARIANTS)))
def test_search_restatement_reproduces_the_recorded_reference(n):
    """One candidate through the restatement's loop against the REFERENCE's kernel model (K_ddf.npz)."""
    abc, assign, subpx, roi = DE.GOLDEN_VARIANTS[n]
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    best, per = DE.search(sam, ref, [abc], p["Nw"], p["max_shift"], roi, assign, subpx)
    want = DE.golden_maps(n)
    for k in ("f", "T", "dx", "dy", "err"):
        np.testing.assert_array_equal(best[k], per[0][k])             # a single candidate comes back untouched
    got = dict(per[0])
    assert_parity(got, want, p["max_shift"], "ddf golden %d" % n, allow_illposed=ILLPOSED, subpx=subpx, f_on_failed=False)


def test_golden_generator_reproduces_the_file(namespaces):
    """What make_golden_ddf.py records, made again from oracle/_ref: the file is what the generator writes."""
    if namespaces["ref"] is None:
        pytest.skip("oracle/_ref/libumpa_ref.so not built")
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    abc, assign, subpx, roi = DE.GOLDEN_VARIANTS[1]
    res = DE.dfkernel_uniform(namespaces["ref"], sam, ref, abc, p["Nw"], p["max_shift"], roi, assign, subpx)
    want = DE.golden_maps(1)
    np.testing.assert_array_equal(res["err"], want["err"])
    np.testing.assert_array_equal(res["debug_Ncalls"], want["debug_Ncalls"])
    np.testing.assert_allclose(res["T"], want["T"], rtol=1e-12)


# ----------------------------------------------------------------------------- 5. the recovery case

def test_recovery_case_restatement_names_the_true_candidate():
    best, per = DE.recovery_search()
    truth, far = DE.recovery_truth()
    assert best["index"].shape == truth.shape == (52, 68)
    share = (best["index"] == truth)[far].mean()
    ok = best["err"] == 1
    print("recovery: %.1f %% of the pixels more than Nw + 2 columns from the seam, median dx %.3f dy %.3f" % (
        100 * share, np.median(best["dx"][ok]), np.median(best["dy"][ok])))
    assert share >= 0.85
    assert abs(np.median(best["dx"][ok]) + 1.0) < 0.02 and abs(np.median(best["dy"][ok]) - 1.0) < 0.02
    assert set(np.unique(truth)) == set(DE.RECOVERY_TRUE) and far.mean() > 0.8


# ----------------------------------------------------------------------------- 6. refusals, no CPU fallback

def test_python_refusals():
    _build()
    from umpa_amd import ddf
    import umpa_amd
    assert umpa_amd.KernelSearch is ddf.KernelSearch and umpa_amd.blur_frames is ddf.blur_frames
    frames = [np.ones((40, 44))] * 2
    with pytest.raises(ValueError, match="no masks"):
        ddf.KernelSearch(frames, frames, mask_list=frames)
    with pytest.raises(ValueError, match="no pos_list"):
        ddf.KernelSearch(frames, frames, pos_list=[(0, 0), (1, 0)])
    with pytest.raises(ValueError, match="unequal shapes"):
        ddf.KernelSearch(frames, [np.ones((40, 44)), np.ones((40, 45))])
    with pytest.raises(ValueError, match="smaller than the 17 x 17 kernel"):
        ddf.KernelSearch([np.ones((16, 44))], [np.ones((16, 44))])
    with pytest.raises(ValueError, match="no pixel inside the padding"):
        ddf.KernelSearch([np.ones((28, 44))], [np.ones((28, 44))])
    with pytest.raises(ValueError, match="inadmissible"):
        ddf.check_candidates([(0.1, 0.0, 0.1), (1.0, 3.0, 1.0)])       # indefinite
    with pytest.raises(ValueError, match="candidate 0.*inadmissible"):
        ddf.check_candidates([(0.1, np.nan, 0.1)])
    with pytest.raises(ValueError, match="inadmissible"):
        ddf.check_candidates([(-0.1, 0.0, 0.1)])
    with pytest.raises(ValueError, match="empty"):
        ddf.check_candidates([])
    with pytest.raises(ValueError, match=r"\[M, 3\]"):
        ddf.check_candidates(np.ones((2, 4)))
    with pytest.raises(ValueError, match="inadmissible"):
        ddf.gaussian_kernel(1.0, 2.0, 1.0)                            # 4 a c - b^2 = 0: degenerate
    with pytest.raises(ValueError, match="smaller than the 17 x 17 kernel"):
        ddf.blur_frames(np.ones((2, 16, 40)), (0.1, 0.0, 0.1))
    with pytest.raises(ValueError, match="unequal shapes"):
        ddf.blur_frames([np.ones((20, 40)), np.ones((20, 41))], (0.1, 0.0, 0.1))


def test_c_abi_argument_errors_come_before_any_device_work():
    _build()
    from umpa_amd import _lib
    lib = _lib.ddf()
    vp = ctypes.c_void_p
    E_ARG = -1
    g = np.zeros(289)
    assert lib.kernel(1.0, 3.0, 1.0, g.ctypes.data_as(vp)) == E_ARG and "no Gaussian" in lib.error()
    assert lib.kernel(np.inf, 0.0, 1.0, g.ctypes.data_as(vp)) == E_ARG and "not finite" in lib.error()
    assert lib.kernel(0.1, 0.0, 0.1, None) == E_ARG
    assert lib.kernel(0.1, 0.0, 0.1, g.ctypes.data_as(vp)) == 0 and abs(g.sum() - 1) < 1e-13
    a, o = np.ones((16, 40)), np.zeros((16, 40))
    tin, tout = (vp * 1)(a.ctypes.data), (vp * 1)(o.ctypes.data)
    assert lib.blur(tin, tout, 1, 16, 40, g.ctypes.data_as(vp), 0, 0, None) == E_ARG and "smaller than the 17 x 17 kernel" in lib.error()
    assert lib.blur(tin, tout, 1, 40, 16, g.ctypes.data_as(vp), 0, 0, None) == E_ARG
    b = np.ones((20, 40))
    tb = (vp * 1)(b.ctypes.data)
    assert lib.blur(tb, tb, 1, 20, 40, g.ctypes.data_as(vp), 0, 0, None) == E_ARG and "may not alias" in lib.error()
    assert lib.blur(tb, tout, 1, 20, 40, g.ctypes.data_as(vp), 0, 2, None) == E_ARG and "no other flag" in lib.error()
    assert lib.blur(tb, tout, -1, 20, 40, g.ctypes.data_as(vp), 0, 0, None) == E_ARG
    bad = g.copy(); bad[5] = np.nan
    assert lib.blur(tb, tout, 1, 20, 40, bad.ctypes.data_as(vp), 0, 0, None) == E_ARG and "not finite" in lib.error()
    d, e = np.zeros(4), np.zeros(4, dtype=np.int32)
    p = lambda x: x.ctypes.data_as(vp)
    assert lib.fold(-1, 4, p(d), p(d), p(d), p(d), p(e), p(d), p(d), p(d), p(d), p(e), p(e), 0, 0, None) == E_ARG
    assert lib.fold(0, -4, p(d), p(d), p(d), p(d), p(e), p(d), p(d), p(d), p(d), p(e), p(e), 0, 0, None) == E_ARG
    assert lib.fold(0, 4, p(d), p(d), p(d), p(d), None, p(d), p(d), p(d), p(d), p(e), p(e), 0, 0, None) == E_ARG


def test_without_a_gpu_the_librarys_error_is_raised():
    _build()
    from umpa_amd import _lib, ddf
    frames = np.ones((2, 40, 44))
    if _lib.hip().device_count() > 0:                                 # a GPU is present: the same call must then succeed
        out = ddf.blur_frames(frames, (0.1, 0.0, 0.1))
        assert out.shape == frames.shape and np.abs(out - 1.0).max() < 1e-13
        return
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        ddf.blur_frames(frames, (0.1, 0.0, 0.1))
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        ddf.KernelSearch(list(frames), list(frames))
