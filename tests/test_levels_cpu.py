"""
Scale-space search (umpa_grid_levels_track, umpa_amd.levels), what can be checked without a GPU: the library's build and its
kernels, the refusals that come before any device work and their order, the Python layer's refusals, the selection rule
against a loop over pixels, the CPU-decided pixel set of the use case, and the uniform-lag row arithmetic under the sanitizers.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import levels_expect as LE
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
NAN, INF = float("nan"), float("inf")
E_ARG = -1


# ----------------------------------------------------------------------------- 1. the library

def test_grid_library_exports_the_entry_point_and_its_levels_kernels_are_claimed():
    g = _build()
    from umpa_amd import _lib
    assert len(g.LIBRARIES) == 8                                      # one more entry point in libumpa_grid.so, not a ninth library
    names = declared("umpa_grid.h", "umpa_grid_")
    assert "umpa_grid_levels_track" in names and "levels_track" in _lib.GRID_SYMBOLS
    assert names == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == names
    assert hasattr(_lib.grid(), "levels_track")
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib._GRID_ABI["levels_track"] == (i, [vp] + [i] * 6 + [i, vp, i, d, d, vp] + [vp] * 26 + [i, vp])
    hdr = open(os.path.join(REPO, "include", "umpa_grid.h")).read()
    assert "#define UMPA_GRID_MAX_LEVELS 4" in hdr and _lib.GRID_MAX_LEVELS == 4 and _lib.GRID_LEVEL_WIDTHS == LE.WIDTHS
    keys = kernel_keys(GRID_LIB)
    syms = [k for k in keys if k.startswith("levels_")]
    assert len(LE.TABLE_KERNELS) == 20 and len(set(LE.SUBSETS)) == 10
    assert sorted(syms) == sorted(LE.KERNELS), sorted(set(syms) ^ set(LE.KERNELS))
    assert_claimed(syms, "levels")
    # the other families of the library keep their counts
    count = lambda prefix: sum(1 for k in keys if k.startswith(prefix))
    assert count("widen_") == 33 and count("grid_track_kernel") == 26 and count("grid_basins_kernel") == 26
    assert len(keys) == len(set(keys))
    # the main library: no new public symbol
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)


LIST_TEXT = ("grid: levels: the half-widths must decrease, the widened ones from {1, 2, 4, 8} and at most three, "
             "a 0 only at the end, not %s")


def test_c_abi_refusals_come_before_any_device_work():
    """No device, no model: a pointer that is never followed stands for one.  The order is the header's: NULL arguments, L,
    the list, tol, the selected group, then umpa_grid_wide_track's checks with its texts."""
    _build()
    from umpa_amd import _lib
    g = _lib.grid()
    fake = ctypes.addressof(ctypes.create_string_buffer(64))
    dbl = [np.zeros(32) for _ in range(14)]
    ints = [np.zeros(32, np.int32) for _ in range(12)]
    p = lambda a: None if a is None else a.ctypes.data
    region = (0, 1, 1, 0, 1, 1)

    def call(model=fake, b=(4, 2, 1, 0), L=None, mode=0, lam=0.0, radius=-1.0, tol=None, lev=None, sel="all", flags=0, no_list=False):
        bb = np.asarray(b, np.int32)
        tt = None if tol is None else np.asarray(tol, np.float64)
        per = [p(a) for a in dbl[:5]] + [None] + [p(a) for a in ints[:3]] + [p(dbl[5])] + [p(a) for a in ints[3:5]]
        if lev is not None:
            per[lev] = None
        chosen = [p(a) for a in dbl[6:11]] + [None] + [p(a) for a in ints[5:8]] + [p(dbl[11])] + [p(a) for a in ints[8:12]]
        if sel == "none":
            chosen = [None] * 14
        elif sel != "all":
            chosen[sel] = None
        rc = g.levels_track(model, *region, len(b) if L is None else L, None if no_list else p(bb), mode, lam, radius, p(tt),
                            *per, *chosen, flags, None)
        return rc, g.error()

    null = (E_ARG, "grid: levels: null argument")
    assert call(model=None, L=0) == null and call(no_list=True, L=9) == null
    for q in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11):                     # every per-level array but df
        assert call(lev=q, L=0) == null, q
    # L, then the list
    for bad in (0, 5, -1, 1 << 20):
        assert call(L=bad, b=(3, 3, 3, 3), tol=[NAN] * 4) == (E_ARG, "grid: levels: 1 to 4 levels, not %d" % bad)
    for bad in ((2, 2), (1, 2), (2, 4, 1), (3,), (4, 3), (0, 1), (4, 0, 0), (8, 4, 2, 1), (9, 1), (-1,), (4, 2, -1)):
        assert call(b=bad, tol=[-1.0] * len(bad)) == (E_ARG, LIST_TEXT % ("(" + ", ".join(str(v) for v in bad) + ")")), bad
    # tol: negative and NaN, naming the entry; +Inf and 0 pass on to the next check
    assert call(tol=[0.0, -1e-300, 0.0, 0.0], sel=0) == (E_ARG, "grid: levels: tol[1] must be >= 0 or +Inf")
    assert call(tol=[0.0, INF, 0.5, NAN], mode=7) == (E_ARG, "grid: levels: tol[3] must be >= 0 or +Inf")
    assert call(b=(2,), tol=[-0.5], mode=7) == (E_ARG, "grid: levels: tol[0] must be >= 0 or +Inf")
    # the selected group: all or none
    group = (E_ARG, "grid: levels: the selected arrays must be all given or all NULL")
    for q in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13):
        assert call(sel=q, tol=[0.0, INF, 0.0, 0.0], mode=7) == group, q
    # then the sibling's checks, with its texts
    for sel in ("all", "none"):
        assert call(sel=sel, mode=7) == (E_ARG, "grid: track: mode must be UMPA_GRID_TRACK_NEAREST (0) or UMPA_GRID_TRACK_PENALTY (1), not 7")
        assert call(sel=sel, mode=1, lam=-1.0, radius=NAN) == (E_ARG, "grid: track: lam must be finite and not negative")
        assert call(sel=sel, mode=1, lam=INF) == (E_ARG, "grid: track: lam must be finite and not negative")
        assert call(sel=sel, mode=0, lam=-1.0, radius=NAN, flags=_lib.F_PLANAR) == (E_ARG, "grid: track: radius must not be NaN")
        assert call(sel=sel, b=(8, 4, 2, 0), flags=_lib.F_PLANAR) == (E_ARG, "grid: track takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag")
    assert all((a == 0).all() for a in dbl + ints)


# ----------------------------------------------------------------------------- 2. the Python layer

class _HipLib:
    is_hip = True


def _stub(cls, **kw):
    """a model object that has what the checks in front of the native call read, and no device: 28 x 36 pixels"""
    from umpa_amd import model
    m = object.__new__(getattr(model, cls))
    m._lib, m._mask, m._force, m._device = _HipLib(), None, 0, 0
    m._pos_list, m._shape_list, m._padding = [(0, 0)] * 3, [(40, 48)] * 3, 6
    m._ROI = ((0, 28, 1), (0, 36, 1))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_python_refusals():
    import umpa_amd
    from umpa_amd import levels as LV, _lib
    assert umpa_amd.levels is LV and LV.__all__ == ["scale_space", "select_levels"]
    assert all(n in umpa_amd.__all__ for n in ("levels", "scale_space", "select_levels"))
    assert umpa_amd.scale_space is LV.scale_space and umpa_amd.select_levels is LV.select_levels
    for cls in ("UMPAModelDF", "UMPAModelNoDF"):
        for bad in ((), (3,), (1, 2), (4, 4), (0, 1), (8, 4, 2, 1), (4, 2, 1, 0, 0), (4.0, 2), (True,), ("2",), 4, None, (9, 1)):
            with pytest.raises(ValueError) as e:
                LV.scale_space(_stub(cls), levels=bad)
            assert str(e.value).startswith("levels must be 1 to 4 decreasing half-widths") and str(e.value).endswith("not %r" % (bad,))
        for bad in (-1.0, NAN, (0.0, 1.0), (0.0, -1.0, 0.0), "x"):
            with pytest.raises((ValueError, TypeError)):
                LV.scale_space(_stub(cls), levels=(4, 2, 0), tol=bad)
        for kw, text in ((dict(lam=-1.0), "scale_space: lam must be None"), (dict(lam=INF), "scale_space: lam must be None"),
                         (dict(radius=-2.0), "scale_space: radius must be None"), (dict(radius=True), "scale_space: radius must be None")):
            with pytest.raises(ValueError, match=text):
                LV.scale_space(_stub(cls), **kw)
        with pytest.raises(RuntimeError, match="Step and ROI|exceeds the reconstructible extent"):
            LV.scale_space(_stub(cls), ROI=((0, 99, 1), (0, 36, 1)))
    # what the grid consumers refuse, with their texts
    tail = "scale_space (grid search / cost volume): "
    for kw, why in ((dict(_mask=[1]), "masked models are not supported (their table holds finished costs)"),
                    (dict(_pos_list=[(0, 0), (0, 1), (0, 0)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                    (dict(_force=_lib.F_FORCE_DIRECT), "the model is forced onto the direct kernel")):
        with pytest.raises(RuntimeError) as e:
            LV.scale_space(_stub("UMPAModelNoDF", **kw))
        assert str(e.value) == tail + why
    with pytest.raises(RuntimeError) as e:
        LV.scale_space(_stub("UMPAModelDFKernel"))
    assert str(e.value) == tail + "the kernel dark-field model has no shift table"
    with pytest.raises(RuntimeError, match="scale_space needs a model with track"):
        LV.scale_space(object())


def test_without_a_device_the_model_is_refused_not_replaced():
    """there is no CPU route: where no HIP device is present, a model cannot be built and scale_space has nothing to run on"""
    _build()
    from umpa_amd import _lib, model, levels as LV
    if _lib.hip().device_count() >= 1:
        return                                                        # (tests/test_hip_levels.py runs the call here)
    frames = [np.ones((40, 48)) for _ in range(3)]
    with pytest.raises(RuntimeError, match="no HIP device|could not create the native model"):
        LV.scale_space(model.UMPAModelNoDF(frames, frames, window_size=2, max_shift=4))


# ----------------------------------------------------------------------------- 3. the selection rule

def _stack(dx, dy, err):
    """level results of hand-made [L, N0, N1] stacks, with the other maps coded by level"""
    L = dx.shape[0]
    return [dict(dx=dx[l], dy=dy[l], err=err[l], f=np.full(dx[l].shape, 10.0 + l), found=np.full(dx[l].shape, l + 1, np.int32),
                 shift=np.full((2,) + dx[l].shape, l, np.int32), region=((0, dx.shape[1], 1), (0, dx.shape[2], 1))) for l in range(L)]


def test_select_levels_against_a_loop():
    from umpa_amd import levels as LV
    rng = np.random.default_rng(7)
    L, N0, N1 = 4, 9, 11
    # quarter steps: differences are exact and ties at tol happen
    dx, dy = rng.integers(-8, 9, (L, N0, N1)) * 0.25, rng.integers(-8, 9, (L, N0, N1)) * 0.25
    err = (rng.random((L, N0, N1)) < 0.8).astype(np.int32)
    dx[rng.random(dx.shape) < 0.05] = NAN
    dy[rng.random(dy.shape) < 0.05] = INF
    err[:, 0, 0] = 0                                                  # no level is ok
    err[:, 0, 1] = 1; dx[:, 0, 1] = [0.0, 0.25, 0.5, 0.75]; dy[:, 0, 1] = 0.0      # a chain of ties exactly at tol
    err[:, 0, 2] = [1, 0, 0, 1]; dx[:, 0, 2] = [0.0, 50.0, -50.0, 0.25]; dy[:, 0, 2] = 0.0   # wider levels that are not ok are skipped
    err[:, 0, 3] = [0, 0, 0, 1]; dx[:, 0, 3] = 3.0; dy[:, 0, 3] = -3.0                       # only the narrowest is ok
    err[:, 0, 4] = 1; dx[:, 0, 4] = [0.0, 0.0, 2.0, 0.0]; dy[:, 0, 4] = 0.0                  # a level in between disagrees
    levels = (8, 4, 1, 0)
    res = _stack(dx, dy, err)
    for tol in (0.0, 0.25, 0.5, INF, None, (0.25, 0.0, INF, 0.0), (0.75, 0.5, 0.25, 0.0)):
        t = LV.check_tol(tol, L)
        got = LV.select_levels(res, tol, levels=levels)
        want = LE.brute_select(dx, dy, err, t)
        np.testing.assert_array_equal(got["level"], want, err_msg=str(tol))
        assert got["level"].dtype == np.int32 and got["halfwidth"].dtype == np.int32
        np.testing.assert_array_equal(got["halfwidth"], np.asarray(levels + (-1,))[want])
        pick = np.where(want < 0, L - 1, want)
        np.testing.assert_array_equal(got["f"], 10.0 + pick)
        np.testing.assert_array_equal(got["found"], pick + 1)
        np.testing.assert_array_equal(got["shift"], np.broadcast_to(pick, (2, N0, N1)))
        np.testing.assert_array_equal(got["dx"], np.take_along_axis(dx, pick[None], 0)[0])
        assert got["region"] == res[0]["region"] and "halfwidth" not in LV.select_levels(res, tol)
        assert want[0, 0] == -1
        assert want[0, 3] == 3
    lv = lambda tol: LV.select_levels(res, tol)["level"]
    assert [lv(t)[0, 1] for t in (0.0, 0.25, 0.5, 0.75)] == [0, 1, 2, 3]       # |dx_l - dx_m| <= tol, the tie included
    assert lv(0.25)[0, 2] == 3 and lv(0.0)[0, 2] == 0
    assert lv(1.0)[0, 4] == 1 and lv(INF)[0, 4] == 3 and lv(0.0)[0, 4] == 1 and lv((0.0, 0.0, 5.0, 0.0))[0, 4] == 3
    # tol = inf: the narrowest ok level; tol = 0: exact agreement with every wider ok level
    ok = (err == 1) & np.isfinite(dx) & np.isfinite(dy)
    narrowest = np.full((N0, N1), -1)
    for l in range(L):
        narrowest[ok[l]] = l
    np.testing.assert_array_equal(lv(INF), narrowest)
    np.testing.assert_array_equal(lv(None), narrowest)
    with pytest.raises(ValueError):
        LV.select_levels([], 0.0)
    with pytest.raises(ValueError):
        LV.select_levels(res, (0.0, 1.0))


# ----------------------------------------------------------------------------- 4. the use case, decided on the CPU

def test_use_case_is_decided_on_the_cpu():
    u, sam, ref, known, sure = LE.use_case()
    assert sure.shape == known.shape and sure.dtype == bool
    b = LE.USE_LEVELS[0]
    assert not sure[:b].any() and not sure[-b:].any() and not sure[:, :b].any() and not sure[:, -b:].any()
    print("use case, levels %s: the true shift is sure at every level at %d of %d pixels, at %d of the %d known pixels"
          % (LE.USE_LEVELS, sure.sum(), sure.size, (sure & known).sum(), known.sum()))
    assert sure.any()


# ----------------------------------------------------------------------------- 5. the row arithmetic, under the sanitizers

def test_level_lists_of_the_geometry_header_are_the_python_layer_s():
    """levels_check (umpa_levels_geom.h) and umpa_amd.levels.check_levels accept the same lists: the ten subsets and the
    single widths, each with and without a final 0, and the 0 alone"""
    from umpa_amd import levels as LV
    good = [s + t for s in LE.SUBSETS + [(b,) for b in LE.WIDTHS] for t in ((), (0,))] + [(0,)]
    assert len(good) == 29
    for lv in good:
        assert LV.check_levels(lv) == list(lv)


def test_row_arithmetic_sweep_under_the_sanitizers(tmp_path):
    """tests/levels_addr_check.cpp: a host program of its own, built with AddressSanitizer and UBSan and run as it is"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "levels_addr_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(REPO, "tests", "levels_addr_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all in range" in out, out
