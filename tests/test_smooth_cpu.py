"""
The regularised shift search, what can be checked without a GPU: the seventh library's build, symbols and kernel families
(and that the six other libraries hold nothing of it), the argument refusals of its C ABI, the numpy restatement
(tests/smooth_expect.py) against a brute-force evaluation of the recursion, the behavioural case the feature exists for,
and cost_scale.

This file carries the library's row of tests/nativelibs.py itself (SMOOTH_ROW) and calls that module's helpers.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import smooth_expect as SE
from nativelibs import LIBRARIES, assert_claimed, build_all, declared, exported, kernel_keys

SMOOTH_LIB = os.path.join(REPO, "umpa_amd", "libumpa_smooth.so")
SMOOTH_ROW = ("SMOOTH_LIB", "umpa_smooth_", "SMOOTH_SYMBOLS", ("smooth_path_kernel", "smooth_transpose_kernel", "smooth_select_kernel"))
US = (3, 5, 7, 9, 11, 13, 15)


def _build():
    import __graft_entry__ as g
    if not os.path.exists(g.SMOOTH_LIB):
        g.build()
    return build_all()


# ----------------------------------------------------------------------------- 1. the library builds

def test_build_produces_the_smooth_library_with_the_declared_symbols():
    g = _build()
    assert g.SMOOTH_LIB == SMOOTH_LIB and os.path.exists(SMOOTH_LIB)
    row = [r for r in g.LIBRARIES if r[0] == SMOOTH_LIB]
    assert len(row) == 1 and row[0][1:3] == ("umpa_smooth.hip", False)           # built alone, over no kernel header
    from umpa_amd import _lib
    attr, prefix, symbols, _ = SMOOTH_ROW
    want = declared("umpa_smooth.h", prefix)
    assert want == sorted(prefix + s for s in getattr(_lib, symbols)) and len(want) == 3
    own = sorted(n for n in exported(SMOOTH_LIB) if n.startswith("umpa"))
    assert own == want, own                                           # its C ABI and nothing else of its own
    assert _lib.smooth().path == SMOOTH_LIB == _lib.SMOOTH_LIB_PATH
    hdr = open(os.path.join(REPO, "include", "umpa_smooth.h")).read()
    for name, value in (("MIN_U", _lib.SMOOTH_MIN_U), ("MAX_U", _lib.SMOOTH_MAX_U), ("ALL_DIRS", _lib.SMOOTH_ALL_DIRS)):
        assert int(re.search(r"#define UMPA_SMOOTH_%s (\w+)" % name, hdr).group(1), 0) == value
    src = open(os.path.join(REPO, "umpa_amd", "csrc", "umpa_smooth.hip")).read()
    included = re.findall(r'#include "([^"]+)"', src)
    assert included == ["../../include/umpa_smooth.h", "umpa_host.h"], included    # stand-alone: no kernel header


def test_the_library_holds_only_smooth_kernels_and_every_family_is_claimed():
    _build()
    keys = kernel_keys(SMOOTH_LIB)
    want = ["smooth_path_kernel<%d, %d, %s>" % (U, TW, f) for U in US for TW in (8, 16) for f in ("false", "true")]
    want += ["smooth_select_kernel<%d>" % U for U in US] + ["smooth_transpose_kernel<false>", "smooth_transpose_kernel<true>"]
    assert sorted(keys) == sorted(want), keys
    assert {k.split("<", 1)[0] for k in keys} == set(SMOOTH_ROW[3])
    mod = assert_claimed(keys, "smooth")
    for test in mod.REACHES:
        assert hasattr(mod, test.split("::")[1]), test


def test_the_other_six_libraries_hold_nothing_of_it():
    g = _build()
    assert len(LIBRARIES) >= 6 and "SMOOTH_LIB" not in [row[0] for row in LIBRARIES]
    for attr, prefix, _, _ in LIBRARIES:
        lib = getattr(g, attr)
        assert not [n for n in exported(lib) if n.startswith("umpa_smooth")], lib
        assert not [k for k in kernel_keys(lib) if k.startswith("smooth_")], lib
    names = exported(SMOOTH_LIB)
    for _, prefix, _, families in LIBRARIES:
        assert not [n for n in names if n.startswith(prefix)], prefix
        assert not [k for k in kernel_keys(SMOOTH_LIB) if families and k.split("<", 1)[0] in families], prefix


# ----------------------------------------------------------------------------- 2. refusals before any device

def _call(lib, cost, U, N0, N1, lam, trunc, dirs, shift="own", flags=0):
    vp = ctypes.c_void_p
    c = None if cost is None else cost.ctypes.data_as(vp)
    out = np.zeros((2, max(N0, 1), max(N1, 1)), dtype=np.int32)
    s = out.ctypes.data_as(vp) if shift == "own" else None
    return lib.aggregate(c, U, N0, N1, lam, trunc, dirs, s, None, None, None, None, 0, flags, None)


def test_c_abi_argument_errors_come_before_any_device_work():
    _build()
    from umpa_amd import _lib
    lib = _lib.smooth()
    E_ARG = -1
    cost = np.zeros((9, 4, 5))
    for U in (1, 2, 4, 8, 17, -3, 0):
        assert _call(lib, cost, U, 4, 5, 1.0, 2.0, 0xFF) == E_ARG and ("U = %d" % U) in lib.error(), U
        assert lib.workspace_bytes(U, 4, 5, 0xFF) == -1 and ("U = %d" % U) in lib.error()
    for N0, N1 in ((0, 5), (4, 0), (-1, 5), (4, -2)):
        assert _call(lib, cost, 3, N0, N1, 1.0, 2.0, 0xFF) == E_ARG and "region of %d x %d" % (N0, N1) in lib.error()
        assert lib.workspace_bytes(3, N0, N1, 0xFF) == -1
    for lam in (-1.0, -1e-300, np.nan, -np.inf):
        assert _call(lib, cost, 3, 4, 5, lam, 2.0, 0xFF) == E_ARG and "lam = " in lib.error(), lam
    for trunc in (-1.0, np.nan, -np.inf):
        assert _call(lib, cost, 3, 4, 5, 1.0, trunc, 0xFF) == E_ARG and "trunc = " in lib.error(), trunc
    for dirs in (0, 0x100, -1, 0x1FF):
        assert _call(lib, cost, 3, 4, 5, 1.0, 2.0, dirs) == E_ARG and "dirs = " in lib.error(), dirs
        assert lib.workspace_bytes(3, 4, 5, dirs) == -1
    assert _call(lib, None, 3, 4, 5, 1.0, 2.0, 0xFF) == E_ARG and "null argument" in lib.error()
    assert _call(lib, cost, 3, 4, 5, 1.0, 2.0, 0xFF, shift=None) == E_ARG and "null argument" in lib.error()
    assert _call(lib, cost, 3, 4, 5, 1.0, 2.0, 0xFF, flags=2) == E_ARG and "no other flag" in lib.error()
    # the workspace: the sum; the transposed input and the transposed H where a horizontal direction is selected
    vol = 9 * 9 * 40 * 52 * 8
    assert lib.workspace_bytes(9, 40, 52, 0xFF) == 3 * vol and lib.workspace_bytes(9, 40, 52, 0x0F) == 3 * vol
    assert lib.workspace_bytes(9, 40, 52, 0x01) == 3 * vol and lib.workspace_bytes(9, 40, 52, 0xFC) == vol
    assert lib.workspace_bytes(15, 4066, 4066, 0xFF) == 3 * 225 * 4066 * 4066 * 8     # beyond 2^32


def test_python_refusals():
    _build()
    import umpa_amd
    from umpa_amd import smooth
    assert umpa_amd.aggregate is smooth.aggregate and umpa_amd.match_smooth is smooth.match_smooth
    assert umpa_amd.cost_scale is smooth.cost_scale and "match_smooth" in umpa_amd.__all__
    c = np.zeros((3, 3, 4, 5))
    with pytest.raises(ValueError, match="paths must be 4 or 8"):
        smooth.aggregate(c, 1.0, 2.0, paths=6)
    with pytest.raises(ValueError, match="lam must be >= 0"):
        smooth.aggregate(c, -1.0, 2.0)
    with pytest.raises(ValueError, match="trunc must be >= 0"):
        smooth.aggregate(c, 1.0, np.nan)
    with pytest.raises(ValueError, match=r"\[U, U, N0, N1\]"):
        smooth.aggregate(np.zeros((3, 4, 4, 5)), 1.0, 2.0)
    with pytest.raises(ValueError, match="odd and within 3 to 15"):
        smooth.aggregate(np.zeros((4, 4, 4, 5)), 1.0, 2.0)
    with pytest.raises(ValueError, match="odd and within 3 to 15"):
        smooth.aggregate(np.zeros((17, 17, 2, 2)), 1.0, 2.0)
    with pytest.raises(ValueError, match="dirs must be a mask"):
        smooth.aggregate(c, 1.0, 2.0, dirs=0)


def test_without_a_gpu_the_librarys_error_is_raised():
    _build()
    from umpa_amd import _lib, smooth
    cost = SE.random_volume(3, 4, 5, 0)
    if _lib.hip().device_count() > 0:                                 # a GPU is present: the same call must then succeed
        got, want = smooth.aggregate(cost, 0.5, 1.0), SE.aggregate(cost, 0.5, 1.0)
        np.testing.assert_array_equal(got["shift"], want["shift"])
        return
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        smooth.aggregate(cost, 0.5, 1.0)


# ----------------------------------------------------------------------------- 3. the restatement against brute force

# dyadic penalties on costs that are multiples of 1/8: every sum is exact, the sweeps equal the closed form
PENALTIES = [(0.5, 1.25), (1.0, 8.0), (0.25, np.inf), (0.0, 3.0), (2.0, 0.5)]


@pytest.mark.parametrize("shape", [(5, 7), (7, 5)], ids=["5x7", "7x5"])
@pytest.mark.parametrize("U", [3, 5])
def test_restatement_equals_brute_force_in_every_direction(U, shape):
    """Each direction alone, N0 < N1 and N0 > N1 (where the diagonals start on either border)."""
    cost = SE.random_volume(U, shape[0], shape[1], 10 * U + shape[0])
    lam, trunc = PENALTIES[U // 2 - 1]
    for d in range(8):
        got = SE.path_cost(cost, lam, trunc, d)
        want = SE.path_cost_brute(cost, lam, trunc, d)
        np.testing.assert_array_equal(got, want, err_msg="direction %d" % d)
        dr, dc = SE.DIRECTIONS[d]
        first = np.zeros(shape, dtype=bool)                           # the path starts: L = C' there
        if dr:
            first[0 if dr > 0 else -1, :] = True
        if dc:
            first[:, 0 if dc > 0 else -1] = True
        np.testing.assert_array_equal(got[:, :, first], cost[:, :, first])
        assert (got[:, :, ~first] != cost[:, :, ~first]).any()


@pytest.mark.parametrize("lam,trunc", PENALTIES, ids=str)
def test_restatement_equals_brute_force_for_every_penalty_pair(lam, trunc):
    cost = SE.random_volume(3, 5, 7, 77)
    for d in (0, 3, 4, 7):
        np.testing.assert_array_equal(SE.path_cost(cost, lam, trunc, d), SE.path_cost_brute(cost, lam, trunc, d))


def test_void_pixels_reset_a_path():
    cost = SE.with_specials(SE.random_volume(3, 5, 7, 5), 6, void_row=2, void_col=4)
    void = ~np.isfinite(cost).any(axis=(0, 1))
    assert void[2].all() and void[:, 4].all() and void.sum() > 5 + 7 - 1      # and scattered ones
    C = SE.conditioned(cost)
    for d in range(8):
        got = SE.path_cost(cost, 0.5, 1.25, d)
        np.testing.assert_array_equal(got, SE.path_cost_brute(cost, 0.5, 1.25, d), err_msg="direction %d" % d)
        assert not np.isnan(got).any()
        assert (got[:, :, void] == 0).all()
        dr, dc = SE.DIRECTIONS[d]
        for i in range(5):
            for j in range(7):
                qi, qj = i - dr, j - dc
                if not void[i, j] and 0 <= qi < 5 and 0 <= qj < 7 and void[qi, qj]:
                    np.testing.assert_array_equal(got[:, :, i, j], C[:, :, i, j])   # restarted behind a void pixel


def test_sum_grouping_and_selection():
    cost = SE.with_specials(SE.random_volume(5, 6, 7, 8), 9)
    L = [SE.path_cost(cost, 0.5, 2.0, d) for d in range(8)]
    H, V = L[0] + L[1], ((((L[2] + L[3]) + L[4]) + L[5]) + L[6]) + L[7]
    np.testing.assert_array_equal(SE.summed(cost, 0.5, 2.0, 0xFF), H + V)
    np.testing.assert_array_equal(SE.summed(cost, 0.5, 2.0, 0x0F), H + (L[2] + L[3]))
    np.testing.assert_array_equal(SE.summed(cost, 0.5, 2.0, 0x03), H)
    np.testing.assert_array_equal(SE.summed(cost, 0.5, 2.0, 0x90), L[4] + L[7])
    out = SE.aggregate(cost, 0.5, 2.0)
    void = ~np.isfinite(cost).any(axis=(0, 1))
    assert void.any() and (out["valid"] == ~void).all() and out["valid"].dtype == np.int32 and out["shift"].dtype == np.int32
    for k in ("smin", "margin"):
        assert (out[k][void] == 0).all()
    assert (out["shift"][:, void] == 0).all()
    total = out["total"].reshape(25, 6, 7)
    for i, j in zip(*np.nonzero(~void)):
        l = int(np.argmin(total[:, i, j]))                            # argmin takes the first minimum; no NaN in a total
        assert tuple(out["shift"][:, i, j]) == (l // 5 - 2, l % 5 - 2) and out["smin"][i, j] == total[l, i, j]
        away = [total[a * 5 + b, i, j] for a in range(5) for b in range(5) if max(abs(a - l // 5), abs(b - l % 5)) >= 2]
        assert out["margin"][i, j] == min(away) - total[l, i, j] >= 0
    # U = 3 and the centre label wins: no label is 2 steps away
    c3 = np.ones((3, 3, 1, 2))
    c3[1, 1, 0, 0], c3[0, 0, 0, 1] = 0.0, 0.0
    o3 = SE.aggregate(c3, 0.5, 1.0)
    assert o3["margin"][0, 0] == np.inf and np.isfinite(o3["margin"][0, 1]) and tuple(o3["shift"][:, 0, 1]) == (-1, -1)


# ----------------------------------------------------------------------------- 4. the behavioural case

def test_behavioural_case_regularisation_removes_the_spurious_basins():
    p = SE.BEHAVIOUR
    cost, truth, spoiled = SE.behavioural_case()
    assert cost.shape == (9, 9, 40, 52) and 0.07 < spoiled.mean() < 0.13
    # the premise: the per-pixel argmin is right where nothing was spoiled and wrong, by 3 labels or more, where it was
    plain = SE.argmin_field(cost)
    wrong = (plain != truth).any(axis=0)
    np.testing.assert_array_equal(wrong, spoiled)
    assert (np.abs(plain - truth).max(axis=0)[spoiled] >= 3).all()
    out = SE.aggregate(cost, p["lam"], p["trunc"])
    inner = np.zeros(spoiled.shape, dtype=bool)
    inner[2:-2, 2:-2] = True
    assert (spoiled & inner).sum() > 100
    miss = (out["shift"] != truth).any(axis=0) & inner
    assert not miss.any(), "%d pixels at least 2 from the border differ from the truth" % miss.sum()
    assert (out["valid"] == 1).all() and (out["margin"][inner] > 0).all()
    four = SE.aggregate(cost, p["lam"], p["trunc"], 0x0F)             # 4 paths do it too on this case
    assert not ((four["shift"] != truth).any(axis=0) & inner).any()
    # without a penalty the result is the per-pixel argmin
    np.testing.assert_array_equal(SE.aggregate(cost, 0.0, 0.0)["shift"], plain)


# ----------------------------------------------------------------------------- 5. cost_scale

def test_cost_scale_on_a_hand_made_volume():
    _build()
    from umpa_amd import smooth
    cost = np.empty((3, 3, 2, 3))
    base = np.arange(9, dtype=np.float64).reshape(3, 3)               # mean 4, least 0
    for n, (i, j) in enumerate(np.ndindex(2, 3)):
        cost[:, :, i, j] = (n + 1) * base                             # mean - min = 4 (n + 1): 4 .. 24
    assert smooth.cost_scale(cost) == 14.0                            # the median of 4, 8, 12, 16, 20, 24
    cost[:, :, 0, 0] = np.nan                                         # a void pixel takes no part: 8 .. 24
    assert smooth.cost_scale(cost) == 16.0
    cost[2, 2, 1, 2] = np.inf                                         # a non-finite label is left out of its pixel's mean:
    assert smooth.cost_scale(cost) == 16.0                            # 6 * 28 / 8 - 0 = 21 instead of 24, the median stays
    cost[0, 0, 0, 1] = -np.inf                                        # ... and out of the least: pixel (0, 1) has 2 * (1 .. 8)
    assert smooth.cost_scale(cost) == np.median([2 * 36 / 8 - 2, 12, 16, 20, 21])
    assert smooth.cost_scale(cost.reshape(9, 2, 3)) == smooth.cost_scale(cost)
    assert np.isnan(smooth.cost_scale(np.full((3, 3, 2, 2), np.nan)))
    assert smooth.LAM_REL > 0 and smooth.TRUNC_REL > 0
