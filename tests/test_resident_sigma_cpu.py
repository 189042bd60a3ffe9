"""
Model-resident uncertainty maps (umpa_grid_uncertainty, include/umpa_grid.h), what can be checked without a GPU: the symbol,
the main library's hook and the kernel family; the argument refusals of the C call and of the Python front under
resident=True (the default call's are pinned by tests/test_sigma_cpu.py); the numpy restatement of the masked definition
(tests/resident_sigma_expect.py) against an extended-precision evaluation of the sums, an independent brute-force
evaluation, the unmasked restatement under a constant mask, dead windows and NaNs; and the behavioural case the masked
definition is validated on: the scatter of the CPU checker's own masked matches over noise realisations.
"""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, REPO

import resident_sigma_expect as RE
import sigma_expect as SE
from nativelibs import assert_claimed, build_all, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
FAMILY = "resident_moments_kernel"
E_ARG = -1


def _build():
    return build_all()


# ----------------------------------------------------------------------------- 1. build and symbols

def test_the_call_is_declared_exported_and_bound():
    g = _build()
    from umpa_amd import _lib
    assert "umpa_grid_uncertainty" in declared("umpa_grid.h", "umpa_grid_")
    assert "uncertainty" in _lib.GRID_SYMBOLS and "uncertainty" in _lib._GRID_ABI
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._GRID_ABI["uncertainty"] == (i, [vp] + [i] * 6 + [vp] * 6 + [i, vp])
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    hdr = open(os.path.join(REPO, "include", "umpa_grid.h")).read()
    for name, value in (("PLAIN", RE.PLANES[0]), ("DF", RE.PLANES[1])):
        assert int(re.search(r"#define UMPA_GRID_SIGMA_PLANES_%s (\w+)" % name, hdr).group(1), 0) == value
    assert _lib.GRID_SIGMA_PLANES == RE.PLANES == (17, 50)
    # the main library: the hook is exported, is no public symbol and is not in the public header
    names = exported(g.HIP_LIB)
    assert "umpa_hipx_model_view" in names
    assert sorted(n for n in names if n.startswith("umpa_hip_")) == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    pub = open(os.path.join(REPO, "include", "umpa_hip.h")).read()
    assert "model_view" not in pub and "umpa_hipx" not in pub
    assert "umpa_hipx_model_view" in open(os.path.join(REPO, "umpa_amd", "csrc", "umpa_hipx.h")).read()
    # the eighth library is what it was: nothing of this lives there
    assert len(g.LIBRARIES) == 8
    assert not [n for n in exported(g.SIGMA_LIB) if "resident" in n or "uncertainty" in n]


def test_the_four_kernels_exist_and_are_claimed():
    g = _build()
    keys = kernel_keys(GRID_LIB)
    syms = [k for k in keys if k.split("<", 1)[0] == FAMILY]
    want = ["%s<%d, %s>" % (FAMILY, kind, masked) for kind in (0, 1) for masked in ("false", "true")]
    assert sorted(syms) == sorted(want), syms
    assert not [k for k in keys if "resident" in k and k not in syms]
    mod = assert_claimed(syms, "resident_sigma")
    for test in mod.REACHES:
        assert hasattr(mod, test.split("::")[1]), test
    for lib in (g.HIP_LIB, g.SIGMA_LIB):
        assert not [k for k in kernel_keys(lib) if "resident" in k], lib


# ----------------------------------------------------------------------------- 2. refusals

def test_c_abi_argument_errors_come_before_any_device_work():
    """A NULL model or array and a foreign flag are refused before the model is looked at (the model pointer given here is
    not one): UMPA_HIP_E_ARG.  The region and the model's own refusals need a model: tests/test_hip_resident_sigma.py."""
    _build()
    from umpa_amd import _lib
    lib = _lib.grid()
    vp = ctypes.c_void_p
    a = {"shift": np.zeros((2, 3, 4), dtype=np.int32), "unit": np.zeros((3, 3, 4)), "s2": np.zeros((3, 4)), "dof": np.zeros((3, 4)),
         "valid": np.zeros((3, 4), dtype=np.int32)}
    reg = (0, 1, 3, 0, 1, 4)

    def call(model, null=None, flags=0, reg=reg):
        p = {k: (None if k == null else v.ctypes.data_as(vp)) for k, v in a.items()}
        return lib.uncertainty(model, *reg, p["shift"], None, p["unit"], p["s2"], p["dof"], p["valid"], flags, None)

    assert call(None) == E_ARG and "null argument" in lib.error()
    fake = ctypes.cast(ctypes.create_string_buffer(64), vp)           # never dereferenced: every call below fails before that
    for null in ("shift", "unit", "s2", "dof", "valid"):
        assert call(fake, null=null) == E_ARG and "null argument" in lib.error(), null
    for flags in (2, 32, 64, 1 | 32):
        assert call(fake, flags=flags) == E_ARG and "no other flag" in lib.error(), flags
    for bad in ((0, 1, 0, 0, 1, 4), (0, 1, 3, 0, 1, 0), (0, 0, 3, 0, 1, 4), (0, 1, 3, 0, 0, 4), (-1, 1, 3, 0, 1, 4), (0, 1, 3, -1, 1, 4),
                (9, 2 ** 30, 3, 0, 1, 4)):
        assert call(fake, reg=bad) == E_ARG and "region axis" in lib.error(), bad


def _fake_model(**kw):
    from umpa_amd import model as M
    base = dict(_lib=types.SimpleNamespace(is_hip=True), _kind=M.KIND_DF, _mask=None, _refshift=0, _Nw=2, _max_shift=3, _padding=5,
                _trivial_coverage=lambda: True, _one_frame_box=lambda: True)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_python_refusals_under_resident():
    _build()
    from umpa_amd import model as M, sigma
    import inspect
    res = {"dx": np.zeros((3, 4)), "dy": np.zeros((3, 4)), "err": np.ones((3, 4), dtype=np.int32)}
    for kw, text in ((dict(_kind=M.KIND_DFKERNEL), "kernel dark-field model"), (dict(_one_frame_box=lambda: False), "pos_list"),
                     (dict(_mask=[1], _one_frame_box=lambda: False), "different shapes"), (dict(_refshift=1), "assign_coordinates='ref'"),
                     (dict(_Nw=9, _padding=12), "Nw = 9"), (dict(_Nw=1), "narrower"), (dict(_mask=[1], _Nw=1), "narrower"),
                     (dict(_lib=types.SimpleNamespace(is_hip=False)), "HIP library only")):
        with pytest.raises(RuntimeError, match="uncertainty: .*%s" % re.escape(text)):
            sigma.uncertainty(_fake_model(**kw), res, resident=True)
    with pytest.raises(RuntimeError, match="kernel dark-field model is not supported"):
        M.UMPAModelDFKernel.uncertainty(None, res, resident=True)
    # masks are refused by the default call as ever, and pass this check under resident=True (the next refusal is sam=)
    with pytest.raises(RuntimeError, match="uncertainty: masked models are not supported"):
        sigma.uncertainty(_fake_model(_mask=[1]), res)
    with pytest.raises(ValueError, match="sam= cannot be given"):
        sigma.uncertainty(_fake_model(_mask=[1]), res, resident=True, sam=np.ones((2, 20, 22)))
    with pytest.raises(ValueError, match="shift= needs resident=True"):
        sigma.uncertainty(_fake_model(), res, shift=np.zeros((2, 3, 4), dtype=np.int32))
    for nv in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="noise_var"):
            sigma.uncertainty(_fake_model(), res, noise_var=nv, resident=True)
    for fn in (sigma.uncertainty, M._UMPAModelPlain.uncertainty, M.UMPAModelDFKernel.uncertainty):
        par = inspect.signature(fn).parameters
        assert list(par)[-2:] == ["resident", "shift"] and par["resident"].default is False and par["shift"].default is None


# ----------------------------------------------------------------------------- 3. the restatement

CASES = [(0, 1, 2, 1), (1, 2, 3, 3), (0, 3, 4, 4), (1, 1, 2, 2)]             # kind, Nw, ms, K  (tests/test_sigma_cpu.py's)
H, W = 34, 40


def _inputs(kind, Nw, ms, K, which, seed=0):
    sam, ref = SE.stack(H, W, K, ms, kind)
    return sam, ref, RE.masks(sam.shape, Nw, ms, seed)[which], SE.window(Nw)


@pytest.mark.parametrize("which", ["binary", "real"])
@pytest.mark.parametrize("kind,Nw,ms,K", CASES, ids=str)
def test_restated_moments_lie_within_the_bound_of_the_extended_precision_ones(kind, Nw, ms, K, which):
    sam, ref, mask, win = _inputs(kind, Nw, ms, K, which)
    reg = (1, 2, 6, 0, 1, W - 2 * (Nw + ms))
    shift = SE.random_shift(reg[2], reg[5], ms, 10 * Nw + kind)
    shift[:, 2, 3] = SE.SKIP
    shift[1, 3, 1] = ms
    got, _ = RE.moments(sam, ref, mask, win, Nw, ms, kind, reg, shift)
    want, bound = RE.moments(sam, ref, mask, win, Nw, ms, kind, reg, shift, np.longdouble)
    assert got.shape == (RE.PLANES[kind], reg[2], reg[5]) and got.dtype == np.float64
    skipped = ~SE.guard(shift, ms)
    assert skipped.sum() == 2 and np.isnan(got[:, skipped]).all() and not np.isnan(got[:, ~skipped]).any()
    err = np.abs(got - want).astype(np.float64)[:, ~skipped]
    assert (err <= bound[:, ~skipped]).all(), np.nanmax(err / bound[:, ~skipped])
    assert (bound[:, ~skipped] <= 1e-12 * np.abs(want[:, ~skipped]).max()).all()  # a rounding bound, not a tolerance


def _sampled_pixels(N0, N1, seed, n=40):
    rng = np.random.default_rng(seed)
    return [(0, 0), (N0 - 1, N1 - 1), (0, N1 - 1)] + [(int(rng.integers(N0)), int(rng.integers(N1))) for _ in range(n)]


@pytest.mark.parametrize("which", ["binary", "real"])
@pytest.mark.parametrize("kind,Nw,ms,K", CASES[1:], ids=str)
def test_restated_solve_equals_the_brute_force_evaluation(kind, Nw, ms, K, which):
    """1e-9 relative on the pixels with cond(A) <= 1e8; those are at least 90 % of the sampled live pixels (the share is
    judged on the brute-force evaluation of the inputs alone, before the restatement is looked at).  Live: more taps carry
    weight than the model has unknowns, n = 3 or 4 -- with n taps or fewer (the rim of the dead block) the fit is exact, the
    definition's dof = sum w - tr is 0 and rounding alone decides its sign."""
    sam, ref, mask, win = _inputs(kind, Nw, ms, K, which)
    reg = SE.full_region(sam.shape, Nw, ms)
    shift = SE.random_shift(reg[2], reg[5], ms, 7 + Nw)
    pixels = _sampled_pixels(reg[2], reg[5], Nw)
    ref_out = RE.brute(sam, ref, mask, win, Nw, ms, kind, reg, shift, pixels)
    live = [(px, b) for px, b in zip(pixels, ref_out) if b is not None and b["taps"] > (4 if kind else 3)]
    well = [(px, b) for px, b in live if b["cond"] <= 1e8]
    assert len(live) >= 35 and len(well) >= 0.9 * len(live), (len(live), len(well))
    out = RE.restated(sam, ref, mask, win, Nw, ms, kind, reg, shift)
    for (i, j), b in well:
        assert out["valid"][i, j] == 1, (i, j, b)
        np.testing.assert_allclose(out["unit"][:, i, j], b["unit"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(out["dof"][i, j], b["dof"], rtol=1e-9)
        np.testing.assert_allclose(out["s2"][i, j], b["s2"], rtol=1e-9)
        assert 0 < out["dof"][i, j] < b["weight"] <= K and out["unit"][0, i, j] > 0 and out["unit"][1, i, j] > 0
        assert out["unit"][2, i, j] ** 2 <= out["unit"][0, i, j] * out["unit"][1, i, j]


@pytest.mark.parametrize("kind,Nw,ms,K", CASES[1:], ids=str)
def test_a_constant_mask_gives_the_unmasked_covariance(kind, Nw, ms, K):
    """All-ones masks scaled by 2: c = 4 / (4 + 1e-8), one weight for every tap.  The covariance does not depend on the scale
    of the weights, so `unit` agrees with the unmasked restatement to 1e-7 relative (c differs from 1 by 2.5e-9)."""
    sam, ref = SE.stack(H, W, K, ms, kind)
    win, reg = SE.window(Nw), SE.full_region(sam.shape, Nw, ms)
    shift = SE.random_shift(reg[2], reg[5], ms, 5)
    got = RE.restated(sam, ref, np.full(sam.shape, 2.0), win, Nw, ms, kind, reg, shift)
    want = SE.restated(sam, ref, win, Nw, ms, kind, reg, shift)
    np.testing.assert_array_equal(got["valid"], want["valid"])
    # the two restatements round differently, and cond(A) multiplies the difference: the pixels with cond(A) <= 1e8, as in the
    # brute-force test, judged by the unmasked brute-force evaluation of the inputs
    every = [(i, j) for i in range(reg[2]) for j in range(reg[5])]
    cond = np.array([b["cond"] for b in SE.brute(sam, ref, win, Nw, ms, kind, reg, shift, every)]).reshape(reg[2], reg[5])
    ok = (want["valid"] == 1) & (cond <= 1e8)
    assert ok.mean() > 0.9
    np.testing.assert_allclose(got["unit"][:, ok], want["unit"][:, ok], rtol=1e-7, atol=0)
    np.testing.assert_allclose(got["dof"][ok], want["dof"][ok], rtol=1e-7)
    np.testing.assert_allclose(got["moments"][RE.WW][ok], K, rtol=1e-8)


@pytest.mark.parametrize("kind", [0, 1])
def test_a_dead_window_is_invalid_and_a_nan_under_zero_weight_poisons_its_footprint(kind):
    Nw, ms, K = 2, 3, 3
    sam, ref, mask, win = _inputs(kind, Nw, ms, K, "binary")
    reg = SE.full_region(sam.shape, Nw, ms)
    shift = SE.random_shift(reg[2], reg[5], ms, 3)
    out = RE.restated(sam, ref, mask, win, Nw, ms, kind, reg, shift)
    dead = RE.dead_pixels(sam.shape, Nw, ms, reg)
    assert dead.sum() == (RE.BLOCK_ROWS - 2 * Nw) * (RE.BLOCK_COLS - 2 * Nw)
    assert (out["moments"][:, dead] == 0).all()                       # no pair weight: every sum is 0, T is 0 / 0
    assert (out["valid"][dead] == 0).all() and np.isnan(out["unit"][:, dead]).all() and np.isnan(out["s2"][dead]).all()
    assert (out["valid"][~dead] == 1).mean() > 0.95
    # a NaN in the sample stack under a zero of the mask: 0 * NaN, exactly the windows that hold the pixel
    pad = Nw + ms
    zeros = np.argwhere(mask[1, pad + 2 * Nw:H - pad - 2 * Nw, pad + 2 * Nw:W - pad - 2 * Nw] == 0)
    r0, c0 = RE.block_origin(sam.shape, Nw, ms)
    far = [z for z in zeros if abs(z[0] + pad + 2 * Nw - r0) > 12 or abs(z[1] + pad + 2 * Nw - c0) > 14]
    bi, bj = far[0] + pad + 2 * Nw
    assert mask[1, bi, bj] == 0
    bad = sam.copy()
    bad[1, bi, bj] = np.nan
    poisoned = RE.restated(bad, ref, mask, win, Nw, ms, kind, reg, shift)
    i, j = np.indices((reg[2], reg[5]))
    holds = (np.abs(i + pad - bi) <= Nw) & (np.abs(j + pad - bj) <= Nw)
    assert holds.sum() == 25
    np.testing.assert_array_equal((poisoned["valid"] == 0) & (out["valid"] == 1), holds & (out["valid"] == 1))
    np.testing.assert_array_equal(poisoned["unit"][:, ~holds], out["unit"][:, ~holds])


# ----------------------------------------------------------------------------- 4. the behavioural case

@pytest.mark.parametrize("which", RE.SCATTER_MASKS)
@pytest.mark.parametrize("name", RE.SCATTER_NAMES)
def test_predicted_sigma_against_the_scatter_of_the_checkers_masked_matches(name, which):
    """With noise_var given, the median over pixels of predicted sigma / empirical standard deviation of 100 masked matches
    lies in [2/3, 3/2] per axis (the cap of tests/test_sigma_cpu.py), and the plain model's median s2 / noise_var in
    [0.8, 1.25].  The values of this test are recorded in tests/golden/resident_sigma_observed.json."""
    got = RE.scatter_case(name, which)
    print(name, which, got)
    assert got["pixels"] > 500
    for axis in ("ratio_dx", "ratio_dy"):
        assert 2 / 3 <= got[axis] <= 3 / 2, (axis, got[axis])
    if name.startswith("plain"):
        assert 0.8 <= got["s2_ratio"] <= 1.25, got["s2_ratio"]
    rec = json.load(open(os.path.join(GOLDEN, "resident_sigma_observed.json")))["%s-%s" % (name, which)]
    for axis in ("ratio_dx", "ratio_dy"):
        assert abs(got[axis] - rec[axis]) < 0.02, (axis, got[axis], rec[axis])
