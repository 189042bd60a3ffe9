"""
Frame registration, what can be checked without a GPU: the fourth library's build and symbol sets, the expectation the GPU
tests use (tests/register_expect.py) against the reference's recorded results (tests/golden/J_register.npz), the host
logic of umpa_amd.register (fit, overlap, position solver), the argument errors and the library's error without a GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import register_expect as RE
from nativelibs import assert_claimed, build_all as _build, declared as _declared, exported, kernel_keys

REGISTER_LIB = os.path.join(REPO, "umpa_amd", "libumpa_register.so")
S8 = (8, 8)


# ----------------------------------------------------------------------------- 1. the library builds

def test_build_produces_the_register_library_with_the_declared_symbols():
    g = _build()
    assert g.REGISTER_LIB == REGISTER_LIB and os.path.exists(REGISTER_LIB)
    from umpa_amd import _lib
    declared = _declared("umpa_register.h", "umpa_register_")
    assert declared == sorted("umpa_register_" + s for s in _lib.REGISTER_SYMBOLS) and len(declared) == 2
    own = sorted(n for n in exported(REGISTER_LIB) if n.startswith("umpa"))
    assert own == declared, own                                       # its C ABI and nothing else of its own
    _lib.hip()
    lib = ctypes.CDLL(REGISTER_LIB)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.register().path == REGISTER_LIB
    hdr = open(os.path.join(REPO, "include", "umpa_register.h")).read()
    assert int(re.search(r"#define UMPA_REGISTER_MAX_SHIFT (\d+)", hdr).group(1)) == _lib.REGISTER_MAX_SHIFT
    assert int(re.search(r"#define UMPA_REGISTER_F_SHARED_A (\d+)", hdr).group(1)) == _lib.REGISTER_F_SHARED_A
    assert int(re.search(r"#define UMPA_REGISTER_F_SHARED_W (\d+)", hdr).group(1)) == _lib.REGISTER_F_SHARED_W


def test_every_register_kernel_is_claimed_by_a_gpu_test():
    _build()
    syms = kernel_keys(REGISTER_LIB)
    assert len(syms) == 3 * 2 * 2 + 3 + 1, syms                       # dtype x weighted x boundary, the norms, the reduction
    mod = assert_claimed(syms, "register")
    for test in mod.REACHES:
        assert hasattr(mod, test.split("::")[1]), test


# ----------------------------------------------------------------------------- 2. the helper against the reference

def test_extended_precision_is_extended():
    cast, _ = RE._extended()
    one = cast(np.array([1.0]))
    assert (one + cast(np.array([2.0 ** -60])))[0] != one[0]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n", [0, 1, 2])
def test_helper_reproduces_the_references_distance(n, weighted):
    g = RE.golden()
    a, b, w = RE.pair(n)
    w = w if weighted else None
    e = RE.expect(a, b, w, S8, "wrap", key=("pair", n, weighted))
    cc, coeff = (g["p%d_ccw" % n], g["p%d_coeffw" % n]) if weighted else (g["p%d_cc" % n], g["p%d_coeff" % n])
    ccmax = float(g["p%d_ccwmax" % n] if weighted else g["p%d_ccmax" % n])
    fP, fQ, fA = RE.fft_bound(a, b, w)
    eps = RE.EPSILON if weighted else 0.0
    # the FFT route's error plus the helper's own (its bound for float64, scaled to the extended arithmetic it uses)
    bound = RE.distance(e["P"], e["Q"], e["A"], eps, fP, fQ, fA)[2] + e["dD"] * RE.extended_over_double()
    err = np.abs(e["D"] - cc)
    print("pair %d %s: max |D - cc| = %.2e max|cc|, bound %.2e max|cc|" % (n, "weighted" if weighted else "plain", err.max() / ccmax, bound.max() / ccmax))
    # observed 0.5 - 1.2e-14 of max |cc|; a bound above 1e-11 of max |cc| would be a mistake in fft_bound
    assert bound.max() < 1e-11 * ccmax
    assert (err <= bound).all()
    x = RE.extended_over_double()
    dalpha = (fP + e["dP"] * x) / (e["Q"] + eps) + np.abs(e["P"]) / (e["Q"] + eps) ** 2 * (fQ + e["dQ"] * x)
    assert (np.abs(e["alpha"] - coeff) <= dalpha).all()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_helper_reproduces_shift_best(n):
    g = RE.golden()
    a, b, _ = RE.pair(n)
    e = RE.expect(a, b, None, S8, "wrap", key=("pair", n, False))
    assert e["status"] == RE.INTERIOR
    fP, fQ, fA = RE.fft_bound(a, b)
    i, j = e["imin"]
    dD = (RE.distance(e["P"], e["Q"], e["A"], 0.0, fP, fQ, fA)[2] + e["dD"] * RE.extended_over_double())[i - 1:i + 2, j - 1:j + 2].max()
    lam = RE.fit(e["D"][i - 1:i + 2, j - 1:j + 2])[3]
    tol = 4.0 * dD / lam
    want = -RE.wrap_centred(g["p%d_best_r" % n], a.shape)               # r*, the reference returns -r* unwrapped
    print("pair %d: r* = %r, reference %r, tol %.2e" % (n, e["shift"], want, tol))
    assert e["tol"] < 1e-6 and tol < 1e-6
    assert np.abs(e["shift"] - want).max() <= tol
    assert abs(e["mindist"] - float(g["p%d_best_mindist" % n])) <= 4.0 * dD + 1e-12 * abs(e["mindist"])


def test_helper_reproduces_get_diff_pos_exactly():
    g = RE.golden()
    got = RE.get_diff_pos(g["dp_refs"])
    np.testing.assert_array_equal(got, g["dp_pos"])
    assert np.abs(g["dp_pos"][1:]).min() > 0.5                        # the fixture moves


def test_helper_reproduces_the_references_chain_on_the_references_crops():
    """find_sam_shift of the reference over the four maps.  Its loop overwrites the frame shape with the last crop's shape
    and shadows its percentile argument with the loop index, so link i is computed at the i-th percentile and links 2 and
    3 on crops narrower than the common region: 50 x 48 of 50 x 60, then 50 x 36 of 60 x 60.  On exactly those crops the
    helper reproduces the recorded chain; on the common region (what umpa_amd registers) links 2 and 3 differ from it."""
    from oracle import align_oracle
    g = RE.golden()
    T, chain = g["T"], g["T_chain"]
    crops = [(T[0][:, 12:72], T[1][:, 0:60]),                         # positions (0, 0) -> (0, 12): the common region
             (T[1][10:60, 0:48], T[2][0:50, 12:60]),                  # (0, 12) -> (10, 0) with the shape (60, 60) of link 1's crop
             (T[2][0:50, 12:48], T[3][0:50, 0:36])]                   # (10, 0) -> (10, 12) with the shape (50, 48) of link 2's
    for i, (a, b) in enumerate(crops):
        a, b = [align_oracle.correct_bad_pixels(im, np.percentile(im, float(i))) for im in (a, b)]
        e = RE.expect(a, b, None, S8, "wrap")
        fP, fQ, fA = RE.fft_bound(a, b)
        ii, jj = e["imin"]
        dD = (RE.distance(e["P"], e["Q"], e["A"], 0.0, fP, fQ, fA)[2] + e["dD"] * RE.extended_over_double())[ii - 1:ii + 2, jj - 1:jj + 2].max()
        tol = 4.0 * dD / RE.fit(e["D"][ii - 1:ii + 2, jj - 1:jj + 2])[3]
        print("link %d: %r, reference %r, tol %.2e" % (i + 1, e["shift"], chain[i + 1], tol))
        assert tol < 1e-6 and np.abs(e["shift"] - chain[i + 1]).max() <= tol
    # the fixture: the recorded two-map shifts are the differences of the sub-pixel errors the maps were cut with
    # (to the accuracy a median-filtered, non-periodic crop allows)
    want = np.array([g["T_err"][j] - g["T_err"][i] for i, j in g["T_pairs"]])
    assert np.abs(g["T_found"] - want).max() < 0.25 and np.abs(want).min() > 0.25


# ----------------------------------------------------------------------------- 3. host logic

def _paraboloid(x0, h, c=3.0):
    u, v = np.meshgrid([-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], indexing="ij")
    du, dv = u - x0[0], v - x0[1]
    return c + h[0][0] * du * du + 2 * h[0][1] * du * dv + h[1][1] * dv * dv


@pytest.mark.parametrize("x0,h", [((0.0, 0.0), ((1.0, 0.0), (0.0, 1.0))), ((0.3, -0.2), ((2.0, 0.5), (0.5, 1.0))),
                                  ((-0.45, 0.4), ((0.7, -0.3), (-0.3, 3.0)))])
def test_fit_recovers_hand_made_paraboloids(x0, h):
    from umpa_amd.register import fit3x3
    z = _paraboloid(x0, h)
    off, val = fit3x3(z)
    np.testing.assert_allclose(off, x0, atol=1e-13)
    assert abs(val - 3.0) < 1e-13
    off2, val2, kind, lam = RE.fit(z)                                 # the helper's lstsq route agrees
    assert kind == "2d" and lam > 0
    np.testing.assert_allclose(off2, off, atol=1e-12)


def test_fit_of_a_saddle_uses_the_two_parabolas():
    from umpa_amd.register import fit3x3
    # positive curvature along both axes, a cross term that makes the paraboloid a saddle
    z = _paraboloid((0.1, -0.1), ((1.0, 2.0), (2.0, 1.0)))
    off, val = fit3x3(z)
    col, row = z[:, 1], z[1, :]
    want = [-(col[2] - col[0]) / (2 * (col[2] + col[0] - 2 * col[1])), -(row[2] - row[0]) / (2 * (row[2] + row[0] - 2 * row[1]))]
    np.testing.assert_allclose(off, want, atol=1e-14)
    mins = [col[1] - (col[2] - col[0]) ** 2 / (8 * (col[2] + col[0] - 2 * col[1])), row[1] - (row[2] - row[0]) ** 2 / (8 * (row[2] + row[0] - 2 * row[1]))]
    assert abs(val - max(mins)) < 1e-14
    off2, val2, kind, _ = RE.fit(z)
    assert kind == "1d"
    np.testing.assert_allclose(off2, off, atol=1e-12)


def test_locate_interior_border_and_no_finite_value():
    from umpa_amd import register as R
    ii, jj = np.meshgrid(np.arange(-3, 4.0), np.arange(-4, 5.0), indexing="ij")
    cc = (ii - 1.25) ** 2 + 2 * (jj + 2.5) ** 2
    shift, alpha, mind, status = R.locate(cc, np.ones_like(cc))
    assert status == R.INTERIOR
    np.testing.assert_allclose(shift, [1.25, -2.5], atol=1e-12)      # jj = -2 and -3 tie: the first minimum, then the fit
    assert abs(mind) < 1e-12
    cc = (ii - 3.4) ** 2 + (jj + 1.0) ** 2                            # the minimum on the last row of the box
    shift, alpha, mind, status = R.locate(cc, np.full_like(cc, 0.5))
    assert status == R.BORDER and tuple(shift) == (3.0, -1.0) and mind == cc[6, 3] and alpha == 0.5
    shift, alpha, mind, status = R.locate(np.full((7, 9), np.nan), np.full((7, 9), np.nan))
    assert status == R.NO_FINITE and np.isnan(shift).all()
    assert (R.INTERIOR, R.BORDER, R.NO_FINITE) == (RE.INTERIOR, RE.BORDER, RE.NO_FINITE)


def test_overlap_of_hand_placed_frames():
    from umpa_amd.register import overlap
    d0, d1, ov = overlap(np.array([[5.0, 5.0], [5.0, 15.4], [25.0, 5.0], [105.0, 5.0]]), (100, 40))
    assert d0[2, 0] == 20.0 and d1[1, 0] == pytest.approx(10.4) and d0[0, 2] == -20.0
    assert ov[0, 0] == 1.0 and ov[0, 1] == pytest.approx(30 / 40) and ov[0, 2] == pytest.approx(0.8)
    assert ov[0, 3] == 0.0 and ov[1, 2] == pytest.approx(0.8 * 0.75)
    np.testing.assert_array_equal(ov, ov.T)


def test_solver_on_a_hand_built_graph_keeps_the_mean_of_the_start():
    from umpa_amd.register import solve_positions
    true = np.array([[0.0, 0.0], [1.5, -2.0], [-0.5, 4.0], [3.0, 1.0], [2.0, 2.0]])
    pairs = [(0, 1), (1, 2), (2, 3), (0, 3), (1, 3), (3, 4)]
    found = np.array([true[j] - true[i] for i, j in pairs])
    x0 = np.array([[10.0, 20.0], [11.0, 19.0], [9.0, 22.0], [12.0, 21.0], [13.0, 23.0]])
    x = solve_positions(pairs, found, x0)
    np.testing.assert_allclose(x.mean(axis=0), x0.mean(axis=0), atol=1e-12)
    np.testing.assert_allclose(x - x.mean(axis=0), true - true.mean(axis=0), atol=1e-12)
    # inconsistent measurements: the least-squares solution, from the normal equations of the graph Laplacian
    rng = np.random.default_rng(0)
    found2 = found + 0.1 * rng.standard_normal(found.shape)
    x = solve_positions(pairs, found2, x0)
    A = np.zeros((len(pairs), 5))
    for k, (i, j) in enumerate(pairs):
        A[k, i], A[k, j] = -1.0, 1.0
    np.testing.assert_allclose(A.T @ (A @ x - found2), 0.0, atol=1e-12)
    np.testing.assert_allclose(x.mean(axis=0), x0.mean(axis=0), atol=1e-12)
    # two components: each keeps its own start where nothing ties it down
    x = solve_positions([(0, 1)], [[1.0, 1.0]], np.zeros((3, 2)))
    np.testing.assert_allclose(x, [[-0.5, -0.5], [0.5, 0.5], [0.0, 0.0]], atol=1e-15)


def test_solver_reproduces_the_references_bfgs_positions():
    """The closed-form positions against the reference's BFGS result, within the bound of BFGS's stopping rule.

    scipy's BFGS stops at |gradient|_inf <= gtol = 1e-5; the gradient is 2 L (x - x*) per coordinate (L: the Laplacian of
    the pair graph), so |x - x*|_2 <= |gradient|_2 / (2 lambda_2) <= gtol sqrt(2 N) / (2 lambda_2) = 3.5e-6 px here.  That
    holds orthogonal to the common offset (the null space of L), and there the two agree to 9.2e-7 px.  Along the common
    offset the cost is flat and an exact gradient never moves; the reference differentiates numerically (forward
    differences, bias h f''/2 = 4.5e-8 on EVERY coordinate), follows that bias and ends with a mean 4.3e-6 / 3.8e-6 px
    (row / column) away from the mean of its start.  The whole vectors therefore differ by 1.15e-5 px, which is the
    reference's drift, not a solver error: the offset is compared with what it should be, the start's mean, exactly."""
    from umpa_amd.register import solve_positions, matching_pairs
    g = RE.golden()
    pos, pairs = g["T_pos"], [tuple(p) for p in g["T_pairs"]]
    assert matching_pairs(pos, g["T"][-1].shape, 0.5) == pairs and len(pairs) == 6
    x = solve_positions(pairs, g["T_found"], pos)
    N = len(pos)
    L = np.zeros((N, N))
    for i, j in pairs:
        L[i, i] += 1; L[j, j] += 1; L[i, j] -= 1; L[j, i] -= 1
    lam = np.linalg.eigvalsh(L)
    assert abs(lam[0]) < 1e-12 and lam[1] > 1e-6
    bound = 1e-5 * np.sqrt(2 * N) / (2 * lam[1])
    ref = g["T_newpos"]
    whole = np.sqrt(((x - ref) ** 2).sum())
    free = np.sqrt((((x - x.mean(axis=0)) - (ref - ref.mean(axis=0))) ** 2).sum())
    print("solver: |x - reference|_2 = %.2e whole, %.2e without the common offset, bound %.2e; the reference's mean moved by %r"
          % (whole, free, bound, ref.mean(axis=0) - pos.mean(axis=0)))
    assert free <= bound
    np.testing.assert_allclose(x.mean(axis=0), pos.mean(axis=0), atol=1e-12)
    assert np.abs(ref.mean(axis=0) - pos.mean(axis=0)).max() < 1e-5   # the reference's drift stays what it was recorded as


# ----------------------------------------------------------------------------- 4. argument errors, no CPU fallback

def test_python_argument_errors():
    _build()
    from umpa_amd import register as R
    a = np.ones((20, 30))
    with pytest.raises(ValueError, match="wider than the frame"):
        R.shift_sums(a, a, max_shift=10)
    with pytest.raises(ValueError, match="wider than the frame"):
        R.shift_sums(a, a, max_shift=(4, 15))
    with pytest.raises(ValueError, match="limited to"):
        R.shift_sums(np.ones((200, 200)), np.ones((200, 200)), max_shift=R.MAX_SHIFT + 1)
    with pytest.raises(ValueError, match="finite and >= 0"):
        w = np.ones((20, 30)); w[3, 4] = -1e-300
        R.shift_sums(a, a, w=w, max_shift=2)
    with pytest.raises(ValueError, match="finite and >= 0"):
        w = np.ones((20, 30)); w[0, 0] = np.inf
        R.shift_sums(a, a, w=w, max_shift=2)
    with pytest.raises(ValueError, match="does not match"):
        R.shift_sums(np.ones((20, 31)), a, max_shift=2)
    with pytest.raises(ValueError, match="does not match"):
        R.shift_sums(np.ones((2, 20, 30)), np.ones((3, 20, 30)), max_shift=2)
    with pytest.raises(ValueError, match="does not match"):
        R.shift_sums(a, a, w=np.ones((30, 20)), max_shift=2)
    with pytest.raises(ValueError, match="boundary"):
        R.shift_sums(a, a, boundary="reflect")
    with pytest.raises(ValueError, match="float64, float32 or uint16"):
        R.shift_sums(a.astype(np.int32), a.astype(np.int32), max_shift=2)


def test_c_abi_argument_errors_come_before_any_device_work():
    _build()
    from umpa_amd import _lib
    lib = _lib.register()
    vp = ctypes.c_void_p
    a = np.ones((20, 30)); out = np.zeros((3, 41, 41))
    w = np.ones((20, 30)); w[5, 6] = -1.0

    def call(S0, S1, wv=None, dtype=0, boundary=0, flags=0, H=20, W=30):
        o = [out[i].ctypes.data_as(vp) for i in range(3)]
        return lib.sums(a.ctypes.data_as(vp), a.ctypes.data_as(vp), wv.ctypes.data_as(vp) if wv is not None else None,
                        dtype, 1, H, W, S0, S1, boundary, o[0], o[1], o[2], 0, flags, None)

    E_ARG, E_UNSUPPORTED = -1, -4
    assert call(10, 2) == E_ARG and "wider than the frame" in lib.error()
    assert call(2, 15) == E_ARG and "wider than the frame" in lib.error()
    assert call(_lib.REGISTER_MAX_SHIFT + 1, 2) == E_UNSUPPORTED and "at most 32" in lib.error()
    assert call(2, 2, wv=w) == E_ARG and "pixel (5, 6)" in lib.error()
    assert call(2, 2, dtype=3) == E_ARG and call(2, 2, boundary=2) == E_ARG and call(2, 2, flags=2) == E_ARG
    assert call(-1, 2) == E_ARG and call(2, 2, H=0) == E_ARG


def test_without_a_gpu_the_librarys_error_is_raised():
    _build()
    from umpa_amd import _lib, align
    a = np.ones((20, 30))
    if _lib.hip().device_count() > 0:                                 # a GPU is present: the same call must then succeed
        P, Q, A = align.shift_sums(a, a, max_shift=2)
        assert P.shape == (5, 5) and (P == 600.0).all() and (Q == 600.0).all() and (A == 600.0).all()
        return
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        align.shift_sums(a, a, max_shift=2)
    with pytest.raises(_lib.NativeError, match="no HIP device"):
        align.get_diff_pos(np.ones((2, 20, 30)), max_shift=2)


def test_align_reexports_the_registration_names():
    from umpa_amd import align, register
    for name in ("shift_sums", "shift_dist", "register", "shift_best", "get_diff_pos", "overlap", "find_sam_shift",
                 "get_new_sam_pos", "shift_data"):
        assert getattr(align, name) is getattr(register, name) and name in align.__all__
    assert "not part of this package" not in align.__doc__
