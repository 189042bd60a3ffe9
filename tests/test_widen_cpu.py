"""
Window widening (umpa_grid_wide_*, ``widen=`` on the grid consumers, umpa_amd.widen), what can be checked without a GPU: the
library's build and its kernels, the refusals that come before any device work, the definition (the window W', the pooled
route against oracle/hp_cost.py given W'), the bound and the admissibility of the GPU tests' inputs, the CPU-decided pixel
sets of the use case, the host logic of umpa_amd.widen, and the address sweep of the chunked box filter under the sanitizers.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import grid_expect as GE
import widen_expect as WE
from nativelibs import assert_claimed, build_all as _build, declared, exported, gpu_test_module, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
WIDE = ("wide_match_region", "wide_cost_volume", "wide_basins", "wide_track")
MAXB = 8
NAN = float("nan")


# ----------------------------------------------------------------------------- 1. the library

def test_grid_library_exports_the_wide_entry_points_and_its_widen_kernels_are_claimed():
    g = _build()
    from umpa_amd import _lib
    assert len(g.LIBRARIES) == 8                                      # four more entry points in libumpa_grid.so, not a ninth library
    names = declared("umpa_grid.h", "umpa_grid_")
    assert all("umpa_grid_" + s in names and s in _lib.GRID_SYMBOLS for s in WIDE)
    assert names == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == names
    assert all(hasattr(_lib.grid(), s) for s in WIDE)
    for s in WIDE:                                                    # the sibling's arguments with `int b` after N1
        sib = _lib._GRID_ABI[s[len("wide_"):]]
        assert _lib._GRID_ABI[s] == (sib[0], sib[1][:7] + [ctypes.c_int] + sib[1][7:])
    hdr = open(os.path.join(REPO, "include", "umpa_grid.h")).read()
    assert "#define UMPA_GRID_MAX_WIDEN 8" in hdr and _lib.GRID_MAX_WIDEN == MAXB
    syms = [k for k in kernel_keys(GRID_LIB) if k.startswith("widen_")]
    # what the dispatch can reach: every half-width on either table layout and either map element, and the carry copy
    want = ["widen_table_kernel<%d, %s>" % (b, s) for b in range(1, MAXB + 1) for s in ("false", "true")] \
        + ["widen_map_kernel<%d, %s>" % (b, s) for b in range(1, MAXB + 1) for s in ("false", "true")] + ["widen_carry_kernel"]
    assert sorted(syms) == sorted(want) and len(syms) == 33, sorted(set(syms) ^ set(want))
    assert_claimed(syms, "widen")
    # the main library: no new public symbol
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)


E_ARG = -1
B_TEXT = "grid: widen: the half-width b must be 0 to 8, not %d"


def test_c_abi_refusals_come_before_any_device_work():
    """No device, no model: a pointer that is never followed stands for one.  The order is the header's: NULL arguments (the
    sibling's text), the range of b, then the sibling's own checks."""
    _build()
    from umpa_amd import _lib
    g = _lib.grid()
    fake = ctypes.addressof(ctypes.create_string_buffer(64))
    dbl = [np.zeros(8) for _ in range(9)]
    ints = [np.zeros(8, np.int32) for _ in range(5)]
    p = lambda a: a.ctypes.data
    region = (0, 1, 1, 0, 1, 1)

    def volume(model=fake, b=1, cost=p(dbl[0]), flags=0):
        return g.wide_cost_volume(model, *region, b, cost, p(dbl[1]), None, flags, None), g.error()

    def match(model=fake, b=1, uv=None):
        return g.wide_match_region(model, *region, b, p(dbl[0]), 4, uv, p(ints[0]), None, 0.0, None, None, None, 0, None), g.error()

    def basins(model=fake, b=1, K=2, f=p(dbl[0]), flags=0):
        return g.wide_basins(model, *region, b, K, f, *[p(a) for a in dbl[1:5]], None, *[p(a) for a in ints[:4]], flags, None), g.error()

    def track(model=fake, b=1, mode=0, found=p(ints[4]), flags=0):
        return g.wide_track(model, *region, b, p(dbl[0]), p(dbl[1]), mode, 0.0, -1.0, *[p(a) for a in dbl[2:7]], None,
                            p(ints[0]), p(ints[1]), p(ints[2]), p(dbl[7]), p(ints[3]), found, flags, None), g.error()

    for bad in (-1, 9, 1 << 20, -(1 << 31)):
        for call in (volume, match, basins, track):
            assert call(b=bad) == (E_ARG, B_TEXT % bad), (call.__name__, bad)
    # NULL arguments come first, with the sibling's text
    assert volume(model=None, b=9) == (E_ARG, "grid: null argument") and volume(cost=None, b=-1) == (E_ARG, "grid: null argument")
    assert match(model=None, b=9) == (E_ARG, "grid: null model")
    assert basins(model=None, b=9) == (E_ARG, "grid: basins: null argument") and basins(f=None, b=9) == (E_ARG, "grid: basins: null argument")
    assert track(model=None, b=9) == (E_ARG, "grid: track: null argument") and track(found=None, b=9) == (E_ARG, "grid: track: null argument")
    # b comes before the sibling's other checks; those follow with their own texts for every b in range
    assert match(b=9, uv=p(dbl[8])) == (E_ARG, B_TEXT % 9)
    assert basins(b=9, K=0) == (E_ARG, B_TEXT % 9) and track(b=-1, mode=7) == (E_ARG, B_TEXT % -1)
    assert volume(b=9, flags=_lib.F_PLANAR) == (E_ARG, B_TEXT % 9)
    for b in (0, 1, MAXB):
        assert match(b=b, uv=p(dbl[8])) == (E_ARG, "grid search takes no start shifts (uv must be NULL)")
        assert basins(b=b, K=0) == (E_ARG, "grid: basins keeps 1 to 8 basins per pixel, not 0")
        assert track(b=b, mode=7) == (E_ARG, "grid: track: mode must be UMPA_GRID_TRACK_NEAREST (0) or UMPA_GRID_TRACK_PENALTY (1), not 7")
        assert volume(b=b, flags=_lib.F_PLANAR) == (E_ARG, "grid: cost_volume takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag")
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
    text = "widen must be an integer from 0 to 8, not %r"
    for cls in ("UMPAModelDF", "UMPAModelNoDF"):
        for bad in (-1, 9, 1.0, "2", True, None, (1,)):
            for call in (lambda m: m.match(search='grid', widen=bad, quiet=True), lambda m: m.cost_volume(widen=bad),
                         lambda m: m.basins(widen=bad), lambda m: m.track(0.0, 0.0, widen=bad)):
                with pytest.raises(ValueError) as e:
                    call(_stub(cls))
                assert str(e.value) == text % (bad,)
        for b in (1, MAXB):
            for kw in (dict(), dict(search='walk')):
                with pytest.raises(ValueError) as e:
                    _stub(cls).match(widen=b, quiet=True, **kw)
                assert str(e.value) == "widen > 0 needs search='grid': the walk reads the cost under the model's own window"


def test_module_and_its_host_logic():
    import torch
    import umpa_amd
    from umpa_amd import widen as W, model
    assert umpa_amd.widen is W and "widen" in umpa_amd.__all__ and W.__all__ == ["window", "valid_region", "embed", "coarse_to_fine"]
    # the window: an independent construction from numpy.hamming; separable, the sum of the model's, half-width Nw + b
    for Nw in (1, 2, 3, 6, 8):
        for b in range(0, MAXB + 1):
            w = W.window(Nw, b)
            assert w.shape == (2 * (Nw + b) + 1,) * 2 and w.flags.c_contiguous
            # (two fp64 routes to sums of B terms per axis: B + 2 roundings each at the most)
            np.testing.assert_allclose(w, WE.window(Nw, b), rtol=2 * (2 * b + 3) * 2.0 ** -53, atol=0)
            assert abs(w.sum() - 1.0) < 1e-14 and np.linalg.matrix_rank(w) == 1
        np.testing.assert_array_equal(W.window(Nw, 0), GE.window(Nw))
    # regions: unit steps keep what fits the extent; steps grow on the requested grid where the extent allows
    m = _stub("UMPAModelNoDF")
    assert W.valid_region(m, 0) == ((0, 28, 1), (0, 36, 1)) and W.valid_region(m, 3) == ((3, 25, 1), (3, 33, 1))
    assert W.valid_region(m, 2, ROI=((5, 20, 1), (8, 30, 1))) == ((5, 20, 1), (8, 30, 1))         # interior: all of it
    assert W.valid_region(m, 2, ROI=((0, 20, 1), (30, 36, 1))) == ((2, 20, 1), (30, 34, 1))
    assert W.valid_region(m, 1, step=2) == ((2, 25, 2), (2, 33, 2)) and W.valid_region(m, 2, step=3) == ((3, 25, 3), (3, 31, 3))
    native, crop, region = model.widen_region((28, 36), (5, 20, 2), (8, 30, 3), 8, 8, 2)
    assert native == ((3, 22, 2), (5, 33, 3), 10, 10) and crop == (slice(1, 9), slice(1, 9)) and region == ((5, 20, 2), (8, 30, 3))
    with pytest.raises(RuntimeError, match="widen=8: no pixel of the region"):
        model.widen_region((12, 36), (0, 12, 1), (0, 36, 1), 12, 36, 8)
    # embed: onto a larger, a smaller and a shifted region of the same grid, numpy and torch alike
    a = np.arange(12.0).reshape(3, 4)
    big = W.embed(a, ((2, 5, 1), (1, 5, 1)), ((0, 6, 1), (0, 6, 1)))
    assert big.shape == (6, 6) and np.isnan(big).sum() == 24
    np.testing.assert_array_equal(big[2:5, 1:5], a)
    np.testing.assert_array_equal(W.embed(a, ((2, 5, 1), (1, 5, 1)), ((3, 5, 1), (2, 4, 1))), a[1:3, 1:3])
    np.testing.assert_array_equal(W.embed(a, ((0, 6, 2), (0, 8, 2)), ((2, 8, 2), (0, 4, 2)), fill=-1.0), [[4.0, 5.0], [8.0, 9.0], [-1.0, -1.0]])
    t = W.embed(torch.as_tensor(a), ((2, 5, 1), (1, 5, 1)), ((0, 6, 1), (0, 6, 1)))
    np.testing.assert_array_equal(t.numpy(), big)
    stack = W.embed(np.stack([a, -a]), ((2, 5, 1), (1, 5, 1)), ((0, 6, 1), (0, 6, 1)), fill=0.0)
    assert stack.shape == (2, 6, 6) and (stack[1, 2:5, 1:5] == -a).all()


# ----------------------------------------------------------------------------- 3. the definition and the bound

@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
@pytest.mark.parametrize("assign", ["sam", "ref"])
def test_the_pooled_route_is_the_model_of_the_wide_window(kind, assign):
    """the box mean of per-pixel extended-precision sums, solved once, against hp_cells given W': 1e-14 relative"""
    from oracle import hp_cost
    sam, ref, c = GE.stack("64x72x3")
    Nw, ms = c["Nw"], c["ms"]
    rng = np.random.default_rng(3)
    for b in (1, 2):
        pad = ms + Nw + b
        n = 300
        pi, pj = rng.integers(pad, c["H"] - pad, n), rng.integers(pad, c["W"] - pad, n)
        si, sj = rng.integers(1 - ms, ms, n), rng.integers(1 - ms, ms, n)
        want = hp_cost.hp_cells(kind, sam, ref, WE.window(Nw, b), pi, pj, si, sj, assign)
        got = WE.pooled_cells(kind, sam, ref, Nw, b, pi, pj, si, sj, assign)
        for k in ("cost", "T"):
            rel = np.abs(got[k] - want[k]) / np.abs(want[k])
            assert rel.max() <= 1e-14, (b, k, float(rel.max()))
        if kind:
            # df = K / T, and K's numerator cancels where the dark-field is weak: the two routes differ in the fp64 rounding of
            # W' (2^-53 per entry), which that cancellation amplifies by its condition number (widen_expect.pooled_cells)
            rel = np.abs(got["df"] - want["df"]) / np.abs(want["df"])
            assert (rel <= 1e-14 * got["df_cond"]).all(), (b, float((rel / got["df_cond"]).max()))


def test_the_bound_is_scaled_by_the_count_of_roundings():
    for Na, Nw, b in ((3, 2, 1), (3, 2, 4), (4, 3, 2), (3, 6, 8)):
        B = 2 * b + 1
        s = WE.scale(Na, Nw, b)
        assert s == np.longdouble(Na * B * B * (2 * Nw + 1) ** 2 + B * B + 3) / np.longdouble(Na * (2 * (Nw + b) + 1) ** 2 + 8)
        assert 1.0 < s < B * B + 1
    sam, ref, c = GE.stack("64x72x3")
    xi, xj = np.meshgrid(np.arange(0, 40, 13), np.arange(0, 48, 11), indexing="ij")
    v = WE.volumes(1, sam, ref, c["Nw"], 2, c["ms"], "sam", pixels=(xi, xj))
    plain = GE.hp_volumes(1, sam, ref, WE.window(c["Nw"], 2), c["ms"], c["ms"] + c["Nw"] + 2, "sam", pixels=(xi, xj))
    np.testing.assert_array_equal(v["bound"], plain["bound"] * WE.scale(3, c["Nw"], 2))
    np.testing.assert_array_equal(v["cost"], plain["cost"])


@pytest.mark.parametrize("name,b", WE.CASES, ids=["%s-b%d" % c for c in WE.CASES])
def test_gpu_inputs_are_admissible(name, b):
    """the near-tie share under the scaled bound, from the reference side alone, for every input of the GPU tests"""
    for kind in (0, 1):
        for assign in ("sam", "ref"):
            share = WE.near_tie_share(WE.volumes_for(name, b, kind, assign))
            print("%s b %d kind %d %s: near-tie share %.5f" % (name, b, kind, assign, share))
            assert share <= GE.NEAR_TIE_CAP


# ----------------------------------------------------------------------------- 4. the use case, decided on the CPU

def test_use_case_is_decided_on_the_cpu():
    mod = gpu_test_module("basins")
    sam, ref, known = mod._use_case()
    u = mod.USE
    Nw, ms, true = u["Nw"], u["ms"], u["true"]
    sure0 = WE.use_case_sure(sam, ref, Nw, ms, 0, true)
    assert sure0.shape == known.shape and not (sure0 & known).any()  # b = 0: the alias wins at every known pixel
    b = 4
    sure = WE.use_case_sure(sam, ref, Nw, ms, b, true)
    inside = known[b:-b, b:-b]
    assert sure.shape == inside.shape
    print("use case, b = 4: the true shift is sure at %.1f %% of %d valid pixels, at %d of the %d known pixels inside"
          % (100 * sure.mean(), sure.size, (sure & inside).sum(), inside.sum()))
    assert sure.mean() >= 0.95
    assert (sure & inside).sum() >= 340


# ----------------------------------------------------------------------------- 5. the addressing, under the sanitizers

def test_address_sweep_under_the_sanitizers(tmp_path):
    """tests/widen_addr_check.cpp: a host program of its own, built with AddressSanitizer and UBSan and run as it is"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "widen_addr_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(REPO, "tests", "widen_addr_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all in range" in out, out
