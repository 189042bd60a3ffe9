"""
Frame registration on the GPU (libumpa_register.so): every sum against the extended-precision restatement of
include/umpa_register.h (tests/register_expect.py) within the bound that holds for any summation order, the minima and
sub-pixel shifts, determinism, device arrays, and the reference's recorded results (tests/golden/J_register.npz).

REACHES names, per test, the kernels of libumpa_register.so it is there for (tests/test_register_cpu.py checks on the CPU
that every kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import numpy as np
import pytest

import register_expect as RE

pytestmark = pytest.mark.gpu

RAW_C = {np.uint16: "unsigned short", np.float32: "float", np.float64: "double"}
REACHES = {
    "tests/test_hip_register.py::test_sums_minimum_and_shift_against_the_helper":
        ["register_tile_kernel<%s, %s, %d>" % (c, wt, bd) for c in RAW_C.values() for wt in ("false", "true") for bd in (0, 1)]
        + ["register_norm_kernel<%s>" % c for c in RAW_C.values()] + ["register_reduce_kernel"],
}

# name -> (shape, max_shift, where the frames come from)
#   70 x 83: no multiple of any tile.  64 x 64 at (3, 5): teams of one wave.  37 x 130 at 16: two passes per thread, three
#   tile columns.  17 x 300 at (8, 8): U0 = H, every row wraps; five tile columns.  70 x 83 at 32, the limit: five passes
#   per thread, tiles of 8 x 32 (weighted overlap: the largest LDS image).  70 x 83 at 20: tiles of 16 x 32.  (The boxes
#   up to 8 take tiles of 32 x 64 unweighted and 16 x 64 weighted, 16 takes 16 x 64: all four tile shapes are launched.)
CASES = {
    "70x83_s20": ((70, 83), (20, 20), ("pair", 0)),
    "70x83_s32": ((70, 83), (32, 32), ("pair", 0)),
    "70x83_s8": ((70, 83), (8, 8), ("pair", 0)),
    "64x64_s3x5": ((64, 64), (3, 5), ("synthetic", [(1.3, -2.6)], 31)),
    "37x130_s16": ((37, 130), (16, 16), ("pair", 2)),
    "17x300_s8": ((17, 300), (8, 8), ("synthetic", [(-2.4, 3.7)], 32)),
}
DTYPES = [np.uint16, np.float32, np.float64]
IDS = ["u16", "f32", "f64"]


@pytest.fixture(scope="module")
def R():
    from umpa_amd import _lib, register
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return register


_frames = {}


def frames(case, dtype):
    """(a, b, w) of a case in a dtype, made once"""
    key = (case, dtype)
    if key not in _frames:
        shape, S, src = CASES[case]
        if src[0] == "pair":
            a, b, w = RE.pair(src[1])
        else:
            a, bs = RE.synthetic(shape, src[1], src[2])
            b, w = bs[0], RE.weights(shape, src[2])
        assert a.shape == shape
        _frames[key] = (RE.as_dtype(a, dtype), RE.as_dtype(b, dtype), w)
    return _frames[key]


def expected(case, dtype, weighted, boundary):
    a, b, w = frames(case, dtype)
    return RE.expect(a.astype(np.float64), b.astype(np.float64), w if weighted else None, CASES[case][1], boundary,
                     key=("gpu", case, dtype, weighted, boundary))


def _check(R, case, dtype, weighted, boundary):
    a, b, w = frames(case, dtype)
    S = CASES[case][1]
    e = expected(case, dtype, weighted, boundary)
    P, Q, A = R.shift_sums(a, b, w if weighted else None, max_shift=S, boundary=boundary)
    for name, got in (("P", P), ("Q", Q), ("A", A)):
        err, bound = np.abs(got - e[name]), e["d" + name]
        print("%s %s %s %s %s: max |err| / bound = %.3f" % (case, dtype.__name__, weighted, boundary, name, (err / bound).max()))
        assert got.shape == (2 * S[0] + 1, 2 * S[1] + 1) and (err <= bound).all(), name
    reg = R.register(a, b, w if weighted else None, max_shift=S, boundary=boundary)
    i, j = np.unravel_index(np.argmin(reg.cc), reg.cc.shape)
    print("   minimum %r, shift %r (helper %r), tol %.2e" % ((i, j), reg.shift, e["shift"], e["tol"]))
    assert (i, j) == e["imin"] and reg.status == e["status"] == R.INTERIOR
    assert e["tol"] < 1e-6                                            # the fixture is no degenerate one
    assert np.abs(reg.shift - e["shift"]).max() <= e["tol"]
    assert (np.abs(reg.cc - e["D"]) <= e["dD"]).all()


# ----------------------------------------------------------------------------- 1. the sums

@pytest.mark.parametrize("boundary", ["wrap", "overlap"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sums_minimum_and_shift_against_the_helper(R, dtype, weighted, boundary):
    _check(R, "70x83_s8", dtype, weighted, boundary)


@pytest.mark.parametrize("boundary", ["wrap", "overlap"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("case", ["64x64_s3x5", "37x130_s16", "17x300_s8"])
def test_other_shapes_against_the_helper(R, case, weighted, boundary):
    _check(R, case, np.float64, weighted, boundary)


@pytest.mark.parametrize("boundary", ["wrap", "overlap"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_a", "distinct_a"])
def test_a_batch_of_three_equals_three_calls_bit_for_bit(R, shared, boundary):
    shape, S = (70, 83), (8, 8)
    a0, bs = RE.synthetic(shape, [(1.3, -2.6), (-3.2, 0.4), (5.5, 6.1)], 33)
    a = a0 if shared else np.stack([a0, 0.9 * np.roll(a0, 1, axis=0), 1.1 * np.roll(a0, -2, axis=1)])
    w1 = RE.weights(shape, 33)
    w = w1 if shared else np.stack([w1, RE.weights(shape, 34), RE.weights(shape, 35)])
    for ww in (None, w):
        got = R.shift_sums(a, bs, ww, max_shift=S, boundary=boundary)
        assert got[0].shape == (3, 17, 17)
        for k in range(3):
            one = R.shift_sums(a if shared else a[k], bs[k], None if ww is None else (ww if shared else ww[k]), max_shift=S, boundary=boundary)
            for g3, g1 in zip(got, one):
                np.testing.assert_array_equal(g3[k], g1)
    e = RE.expect(a0, bs[2], None, S, boundary)
    reg = R.register(a, bs, None, max_shift=S, boundary=boundary)
    assert reg.shift.shape == (3, 2) and reg.status.shape == (3,) and reg.cc.shape == (3, 17, 17)
    if shared:
        assert np.abs(reg.shift[2] - e["shift"]).max() <= e["tol"] < 1e-6


def test_all_zero_weights_give_zero_sums(R):
    a, b, _ = frames("70x83_s8", np.float64)
    for boundary in ("wrap", "overlap"):
        P, Q, A = R.shift_sums(a, b, np.zeros(a.shape), max_shift=8, boundary=boundary)
        assert (P == 0).all() and (Q == 0).all() and (A == 0).all()
        reg = R.register(a, b, np.zeros(a.shape), max_shift=8, boundary=boundary)
        assert (reg.cc == 0).all() and reg.status == R.BORDER and tuple(reg.shift) == (-8.0, -8.0)


@pytest.mark.parametrize("case,weighted,boundary", [("70x83_s32", False, "wrap"), ("70x83_s32", True, "overlap"), ("70x83_s20", True, "overlap")],
                         ids=["s32_plain_wrap", "s32_weighted_overlap", "s20_weighted_overlap"])
def test_large_boxes_against_the_helper(R, case, weighted, boundary):
    _check(R, case, np.float64, weighted, boundary)


# ----------------------------------------------------------------------------- 2. determinism, device arrays, NaN

@pytest.mark.parametrize("boundary", ["wrap", "overlap"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_two_calls_and_device_arrays_agree_bit_for_bit(R, weighted, boundary):
    import torch
    a0, bs = RE.synthetic((70, 83), [(1.3, -2.6), (-3.2, 0.4)], 36)
    w = RE.weights((70, 83), 36) if weighted else None
    for dtype in (np.float64, np.float32):
        a, b = RE.as_dtype(a0, dtype), RE.as_dtype(bs, dtype)
        first = R.shift_sums(a, b, w, max_shift=(8, 5), boundary=boundary)
        again = R.shift_sums(a, b, w, max_shift=(8, 5), boundary=boundary)
        dev = R.shift_sums(torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0"),
                           None if w is None else torch.from_numpy(w).to("cuda:0"), max_shift=(8, 5), boundary=boundary)
        for f, g, d in zip(first, again, dev):
            assert d.is_cuda and d.dtype == torch.float64
            np.testing.assert_array_equal(f, g)
            np.testing.assert_array_equal(f, d.cpu().numpy())


def test_one_nan_pixel_gives_the_no_finite_value_status(R):
    a, b, w = frames("70x83_s8", np.float64)
    b = b.copy()
    b[40, 17] = np.nan
    for ww in (None, w):
        reg = R.register(a, b, ww, max_shift=8, boundary="wrap")
        assert reg.status == R.NO_FINITE and np.isnan(reg.shift).all() and np.isnan(reg.cc).all()
    regs = R.register(a, np.stack([b, frames("70x83_s8", np.float64)[1]]), None, max_shift=8)
    assert list(regs.status) == [R.NO_FINITE, R.INTERIOR]            # the next pair of the batch is not touched


# ----------------------------------------------------------------------------- 3. the reference's recorded results

def _against_reference(a, b, S, key):
    """(helper's expectation, tolerance of the sub-pixel shift, bound of D on the 3 x 3) for a GPU result compared with
    the reference's: the GPU sums' bound plus the FFT route's, through the fit"""
    e = RE.expect(a, b, None, S, "wrap", key=key)
    fP, fQ, fA = RE.fft_bound(a, b)
    ii, jj = e["imin"]
    dD = (RE.distance(e["P"], e["Q"], e["A"], 0.0, fP, fQ, fA)[2] + e["dD"])[ii - 1:ii + 2, jj - 1:jj + 2].max()
    tol = 4.0 * dD / RE.fit(e["D"][ii - 1:ii + 2, jj - 1:jj + 2])[3]
    assert tol < 1e-6
    return e, tol, dD


def test_get_diff_pos_reproduces_the_reference(R):
    g = RE.golden()
    refs = g["dp_refs"]
    # the unrounded positions lie >= 5e-4 px from a rounding tie (checked when the fixture was made) and agree within
    # the tolerance, so the rounded positions are equal
    reg = R.register(refs[0], refs, None, max_shift=8)
    for k in range(len(refs)):
        tol = _against_reference(refs[0], refs[k], (8, 8), ("dp", k))[1]
        assert np.abs(RE.wrap_centred(-reg.shift[k], refs.shape[1:]) - g["dp_unrounded"][k]).max() <= tol
    np.testing.assert_array_equal(R.get_diff_pos(refs), g["dp_pos"])


@pytest.mark.parametrize("n", [0, 1, 2])
def test_shift_best_reproduces_the_references_triple(R, n):
    """(b', -r*, alpha) of the reference.  With the shift within tol of the reference's, the bilinearly resampled frame
    moves by at most G tol per pixel (G: the largest difference of neighbouring pixels of b, summed over the two axes)
    plus a few roundings; alpha = sum a b_s / sum b_s^2 then by (|a|_2 / |b_s|_2 + 2 |alpha|) |db_s|_2 / |b_s|_2."""
    from umpa_amd import align
    g = RE.golden()
    a, b, _ = RE.pair(n)
    e, tol, dD = _against_reference(a, b, (8, 8), ("best", n))
    bb, r, alpha = align.shift_best(a, b)
    want_r = g["p%d_best_r" % n]
    assert np.abs(RE.wrap_centred(r - want_r, a.shape)).max() <= tol and np.abs(r).max() < 8      # -r*, the reference's unwrapped
    G = np.abs(np.diff(b, axis=0, append=b[:1])).max() + np.abs(np.diff(b, axis=1, append=b[:, :1])).max()
    db = G * tol + 16 * RE.U * np.abs(b).max()
    nb = np.sqrt((bb * bb).sum()) / abs(alpha)
    dalpha = (np.sqrt((a * a).sum()) / nb + 2 * abs(alpha)) * np.sqrt(a.size) * db / nb + 4 * a.size * RE.U * abs(alpha)
    print("pair %d: -r* %r (reference %r), alpha %.15g (reference %.15g, bound %.1e)" % (n, r, want_r, alpha, float(g["p%d_best_alpha" % n]), dalpha))
    assert abs(alpha - float(g["p%d_best_alpha" % n])) <= dalpha
    assert 0.8 < alpha / (1 / 0.85) < 1.2                             # b is 0.85 a, shifted: the scale is the inverse
    if n == 0:
        err = np.abs(bb - g["p0_best_b"]).max()
        print("        max |b' - reference| = %.2e, bound %.2e" % (err, abs(alpha) * db + dalpha * np.abs(b).max()))
        assert err <= abs(alpha) * db + dalpha * np.abs(b).max()
        rms = lambda x: np.sqrt((x * x).mean())
        assert rms(bb - a) < 0.05 and rms(b - a) > 0.3                 # b' lies on a, b did not
    assert abs(align.shift_best.mindist - float(g["p%d_best_mindist" % n])) <= 4.0 * dD + 1e-12 * abs(float(g["p%d_best_mindist" % n]))
    np.testing.assert_array_equal(align.shift_best(a, b, return_params=False), bb)


def _crops(T, pos, i, j, p):
    """the two repaired crops find_sam_shift registers: the pixels both maps show, by the CPU restatement of
    correct_bad_pixels.  Map j starts step = round(pos[j] - pos[i]) sample pixels after map i."""
    from oracle import align_oracle
    step = np.rint(pos[j] - pos[i]).astype(int)
    rows, cols = [np.arange(n) for n in T[i].shape]
    ri = rows[(rows - step[0] >= 0) & (rows - step[0] < len(rows))]  # rows of map i that map j has too
    ci = cols[(cols - step[1] >= 0) & (cols - step[1] < len(cols))]
    ims = (T[i][np.ix_(ri, ci)], T[j][np.ix_(ri - step[0], ci - step[1])])
    return [align_oracle.correct_bad_pixels(im, np.percentile(im, p)) for im in ims]


def _pair_tol(T, pos, i, j, p):
    """tolerance of one registered pair against the reference"""
    a, b = _crops(T, pos, i, j, p)
    return _against_reference(a, b, (8, 8), ("T", i, j, p))[1]


def test_find_sam_shift_reproduces_the_reference(R):
    """The reference's find_sam_shift of every overlapping pair of the 2 x 2 grid (what its get_new_sam_pos calls), and the
    first link of its chain over the four maps.

    Two properties of the reference decide what is comparable.  Its loop variable shadows the percentile argument p, so
    pair i of a call is repaired at the i-th percentile: p=0 reproduces a two-map call.  And inside the loop it replaces the
    frame shape by the shape of the last CROP, so from the second link of a chain on it crops narrower than the common
    region (tests/test_register_cpu.py reproduces links 2 and 3 of the recorded chain on those narrower crops).  Links 2 and
    3 are therefore compared with the two-map calls of the same pairs, which the reference computes on the common region."""
    g = RE.golden()
    T, pos, pairs = g["T"], g["T_pos"], [tuple(p) for p in g["T_pairs"]]
    for (i, j), want in zip(pairs, g["T_found"]):
        got = R.find_sam_shift([T[i], T[j]], pos[[i, j]], max_shift=8, p=0)
        tol = _pair_tol(T, pos, i, j, 0.0)
        print("maps %d, %d: %r, reference %r, tol %.2e" % (i, j, got[1], want, tol))
        assert (got[0] == 0).all() and np.abs(got[1] - want).max() <= tol
    chain = np.array(R.find_sam_shift(T, pos, max_shift=8, p=0))
    assert chain.shape == (4, 2) and (chain[0] == 0).all()
    assert np.abs(chain[1] - g["T_chain"][1]).max() <= _pair_tol(T, pos, 0, 1, 0.0)
    for i in (1, 2):                                                  # (1, 2) and (2, 3) are pairs of the grid
        assert np.abs(chain[i + 1] - g["T_found"][pairs.index((i, i + 1))]).max() <= _pair_tol(T, pos, i, i + 1, 0.0)
    # a percentile per link, and the default p = 99.9: each link against the helper on crops repaired at that percentile
    ps = [0.0, 50.0, 99.9]
    for got, pp in ((np.array(R.find_sam_shift(T, pos, max_shift=8, p=ps)), ps), (np.array(R.find_sam_shift(T, pos)), [99.9] * 3)):
        for i in range(3):
            a, b = _crops(T, pos, i, i + 1, pp[i])
            e = RE.expect(a, b, None, (8, 8), "wrap", key=("Tp", i, pp[i]))
            assert e["tol"] < 1e-6 and np.abs(got[i + 1] - e["shift"]).max() <= e["tol"]


def test_get_new_sam_pos_reproduces_the_reference(R):
    g = RE.golden()
    T, pos, pairs = g["T"], g["T_pos"], [tuple(p) for p in g["T_pairs"]]
    got = R.get_new_sam_pos(T, pos, ov_thr=0.5, max_shift=8, p=0)
    N = len(pos)
    L = np.zeros((N, N))
    for i, j in pairs:
        L[i, i] += 1; L[j, j] += 1; L[i, j] -= 1; L[j, i] -= 1
    lam2 = np.linalg.eigvalsh(L)[1]
    tol = max(_pair_tol(T, pos, i, j, 0.0) for i, j in pairs)
    # BFGS's stopping rule (tests/test_register_cpu.py) plus the pairs' tolerance through the pseudo-inverse
    bound = 1e-5 * np.sqrt(2 * N) / (2 * lam2) + np.sqrt(2 * len(pairs)) * tol / np.sqrt(lam2)
    # without the common offset: the reference's own mean drifts with its numerical gradient (test_register_cpu.py,
    # test_solver_reproduces_the_references_bfgs_positions); the offset is compared with the start's mean instead
    ref = g["T_newpos"]
    err = np.sqrt((((got - got.mean(axis=0)) - (ref - ref.mean(axis=0))) ** 2).sum())
    print("get_new_sam_pos: |x - reference|_2 without the common offset = %.2e, bound %.2e" % (err, bound))
    assert err <= bound
    np.testing.assert_allclose(got.mean(axis=0), pos.mean(axis=0), atol=1e-12)


# ----------------------------------------------------------------------------- 4. shift_data

def test_shift_data_integer_shifts_copy_pixels(R):
    rng = np.random.default_rng(8)
    frames_ = rng.integers(0, 65535, size=(3, 37, 71)).astype(np.uint16)
    shifts = [(2, -3), (0, 0), (-5, 40)]
    for interp in ("cubic", "linear"):
        got = R.shift_data(frames_, shifts, interp=interp)
        for k, (s0, s1) in enumerate(shifts):
            ii = np.clip(np.arange(37) - s0, 0, 36)
            jj = np.clip(np.arange(71) - s1, 0, 70)
            np.testing.assert_array_equal(got[k], frames_[k].astype(np.float64)[ii[:, None], jj[None, :]])


def test_shift_data_fractional_shifts_are_the_unwarp_librarys(R):
    from umpa_amd import UnwarpMap
    rng = np.random.default_rng(9)
    f = rng.random((2, 37, 71))
    shifts = [(1.25, -0.6), (-2.5, 3.75)]
    for interp in ("cubic", "linear"):
        got = R.shift_data(f, shifts, interp=interp)
        for k, s in enumerate(shifts):
            m = UnwarpMap(np.full((37, 71), -s[0], np.float32), np.full((37, 71), -s[1], np.float32), interp=interp)
            np.testing.assert_array_equal(got[k], m.apply(f[k])[0])
