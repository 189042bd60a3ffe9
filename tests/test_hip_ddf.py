"""
The directional dark-field search on the GPU (libumpa_ddf.so, umpa_amd/ddf.py): the blur within its rounding bound of the
longdouble restatement, its bit-reproducibility and NaN footprint; one candidate against the plain model, the CPU checker's
kernel model and the reference's recorded maps; sequences of candidates on one searcher; the fold; the recovery of two known
kernels; the refusals.  tests/ddf_expect.py is the restatement.

REACHES names, per test, the kernels of libumpa_ddf.so it is there for (tests/test_ddf_cpu.py checks on the CPU that every
kernel of the library is claimed).

The cap on unconverged-Newton pixels is the one of tests/test_ddf_cpu.py (1.2 %, the suite's share for the plain model
with 3 frames and Nw = 2), `f` of failed pixels is not compared with the reference's recorded maps (see there).
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity

import ddf_expect as DE

pytestmark = pytest.mark.gpu

ILLPOSED = 0.012
BLUR_V, BLUR_S, FOLD = "ddf_blur_kernel<true>", "ddf_blur_kernel<false>", "ddf_fold_kernel"
REACHES = {
    "test_hip_ddf.py::test_blur_within_bound": [BLUR_V, BLUR_S],
    "test_hip_ddf.py::test_blur_is_bit_identical_on_repetition_and_between_host_and_device": [BLUR_V, BLUR_S],
    "test_hip_ddf.py::test_nan_reaches_exactly_its_footprint": [BLUR_V, BLUR_S],
    "test_hip_ddf.py::test_blur_of_more_frames_than_one_launch_takes": [BLUR_V],
    "test_hip_ddf.py::test_one_candidate": [BLUR_V, FOLD],
    "test_hip_ddf.py::test_sequence_of_candidates_on_one_searcher": [BLUR_V, FOLD],
    "test_hip_ddf.py::test_fold_of_a_search_equals_the_numpy_fold": [FOLD],
    "test_hip_ddf.py::test_fold_hand_made_planes_through_the_c_abi": [FOLD],
    "test_hip_ddf.py::test_recovery": [BLUR_V, FOLD],
}

# 17 x 17: one interior pixel (odd W: the scalar kernel); 24 x 40; 49 x 131: odd, no tile multiple; 70 x 150: more than one
# tile both ways (32 x 64 tiles); 64 x 72 x 3
SHAPES = [(1, 17, 17), (1, 24, 40), (1, 49, 131), (1, 70, 150), (3, 64, 72)]


def _frames(shape, seed=0):
    rng = np.random.default_rng(100 + seed)
    x = 1.0 + 0.3 * rng.standard_normal(shape)
    x[..., ::7, ::5] *= -40.0                                         # mixed signs and scales: the bound is on sum g |in|
    return x


@pytest.fixture(scope="module")
def ddf():
    import torch
    assert torch.cuda.is_available()
    from umpa_amd import ddf
    return ddf


WORST = {}


@pytest.mark.parametrize("abc", DE.BLUR_KERNELS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blur_within_bound(ddf, shape, abc):
    x = _frames(shape)
    got = ddf.blur_frames(x, abc)
    assert got.shape == shape and got.dtype == np.float64
    g = ddf.gaussian_kernel(*abc)
    worst = 0.0
    for k in range(shape[0]):
        want, bound = DE.blur_exact(x[k], g)
        inner = np.zeros(shape[1:], dtype=bool)
        inner[8:shape[1] - 8, 8:shape[2] - 8] = True
        assert inner.sum() == (shape[1] - 16) * (shape[2] - 16) >= 1
        np.testing.assert_array_equal(got[k][~inner], x[k][~inner])   # the border: the input, bit for bit
        err = np.abs(got[k].astype(np.longdouble) - want)
        assert (bound[inner] > 0).all()
        ratio = float((err[inner] / bound[inner]).max())
        worst = max(worst, ratio)
        assert (err[inner] <= bound[inner]).all(), "frame %d: %.3f of the bound" % (k, ratio)
    WORST[(shape, abc)] = worst
    print("blur %r %r: worst |out - exact| / bound = %.4f (overall so far %.4f)" % (shape, abc, worst, max(WORST.values())))


def test_blur_is_bit_identical_on_repetition_and_between_host_and_device(ddf):
    import torch
    abc = DE.BLUR_KERNELS[1]
    for shape in [(3, 70, 150), (2, 49, 131)]:                        # the 16-byte kernel, the scalar kernel
        x = _frames(shape, 1)
        first = ddf.blur_frames(x, abc)
        np.testing.assert_array_equal(ddf.blur_frames(x, abc), first)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            t = torch.from_numpy(x).cuda()
            out = ddf.blur_frames(t, abc)
            again = ddf.blur_frames([t[k] for k in range(shape[0])], abc)
        side.synchronize()
        assert out.is_cuda and out.shape == t.shape
        np.testing.assert_array_equal(out.cpu().numpy(), first)
        np.testing.assert_array_equal(again.cpu().numpy(), first)
    # more frames than one launch takes
    x = _frames((35, 20, 24), 2)
    got = ddf.blur_frames(x, abc)
    np.testing.assert_array_equal(got[34], ddf.blur_frames(x[34], abc))
    np.testing.assert_array_equal(got[3], ddf.blur_frames(x[3:4], abc)[0])


def test_blur_of_more_frames_than_one_launch_takes(ddf):
    """33 frames, one more than UMPA_DDF_MAX_FRAMES: the host-array call uploads, blurs and downloads them in two rounds, the
    device call launches twice.  The smallest frame the 16-byte kernel admits (17 x 18: two interior pixels), an
    anisotropic kernel, every frame of both calls within the bound of test_blur_within_bound."""
    import torch
    from umpa_amd import _lib
    K, abc = _lib.DDF_MAX_FRAMES + 1, DE.BLUR_KERNELS[2]
    assert K == 33 and abc[0] != abc[2] and abc[1] != 0
    x = _frames((K, 17, 18), 4)
    g = ddf.gaussian_kernel(*abc)
    host = ddf.blur_frames(x, abc)
    dev = ddf.blur_frames(torch.from_numpy(x).cuda(), abc)
    assert host.shape == x.shape and dev.is_cuda and tuple(dev.shape) == x.shape
    dev = dev.cpu().numpy()
    inner = np.zeros((17, 18), dtype=bool)
    inner[8, 8:10] = True
    for k in range(K):
        want, bound = DE.blur_exact(x[k], g)
        assert (bound[inner] > 0).all()
        for name, got in (("host", host[k]), ("device", dev[k])):
            np.testing.assert_array_equal(got[~inner], x[k][~inner], err_msg="%s frame %d" % (name, k))
            err = np.abs(got.astype(np.longdouble) - want)
            assert (err[inner] <= bound[inner]).all(), "%s frame %d: %.3f of the bound" % (name, k, float((err[inner] / bound[inner]).max()))
            assert (got[inner] != x[k][inner]).all()                  # blurred, not copied


@pytest.mark.parametrize("shape,at", [((40, 70), (20, 33)), ((40, 70), (3, 66)), ((41, 71), (20, 33)), ((41, 71), (37, 2))],
                         ids=["even-inside", "even-border", "odd-inside", "odd-border"])
def test_nan_reaches_exactly_its_footprint(ddf, shape, at):
    x = _frames(shape, 3)
    clean = ddf.blur_frames(x, (50.0, 0.0, 50.0))                     # near-delta: most taps underflow to 0, 0 * NaN is NaN
    x[at] = np.nan
    got = ddf.blur_frames(x, (50.0, 0.0, 50.0))
    ii, jj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    inner = (ii >= 8) & (ii < shape[0] - 8) & (jj >= 8) & (jj < shape[1] - 8)
    want = inner & (np.abs(ii - at[0]) <= 8) & (np.abs(jj - at[1]) <= 8)
    want[at] = True                                                   # copied where it is on the border, summed otherwise
    np.testing.assert_array_equal(np.isnan(got), want)
    np.testing.assert_array_equal(got[~want], clean[~want])


# ----------------------------------------------------------------------------- one candidate

def _search(ddf, sam, ref, Nw, ms, assign="sam", subpx=-1, debug=True):
    s = ddf.KernelSearch(list(sam), list(ref), window_size=Nw, max_shift=ms)
    s.assign_coordinates = assign
    s.sub_pixel_mode = subpx
    s.debug = debug
    return s


@pytest.mark.parametrize("n", range(len(DE.GOLDEN_VARIANTS)))
def test_one_candidate(ddf, port_ns, n):
    """Both coordinate conventions, one stepped ROI, sub-pixel modes -1 and 1 (ddf_expect.GOLDEN_VARIANTS)."""
    import umpa_amd
    abc, assign, subpx, roi = DE.GOLDEN_VARIANTS[n]
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    s = _search(ddf, sam, ref, p["Nw"], p["max_shift"], assign, subpx)
    assert s.extent == (p["H"] - 28, p["W"] - 28) and s.padding == 14
    got = s.match([abc], ROI=roi)
    # (a) bit for bit the plain model on the blurred stack, a fresh model, the region shifted by 8
    m = umpa_amd.UMPAModelNoDF(list(sam), list(ddf.blur_frames(np.array(ref), abc)), window_size=p["Nw"], max_shift=p["max_shift"])
    m.assign_coordinates, m.sub_pixel_mode = assign, subpx
    plain = m.match(ROI=DE.shifted(roi if roi is not None else DE.full_roi(sam[0].shape, p["Nw"], p["max_shift"])), quiet=True)
    for k in ("f", "T", "dx", "dy", "err", "debug_Ncalls", "debug_a", "debug_d"):
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    assert got["err"].dtype == np.int32 and got["index"].dtype == np.int32
    np.testing.assert_array_equal(got["index"], np.where(plain["err"] == 1, 0, -1))
    won = got["index"] == 0
    for k, v in zip("abc", abc):
        assert (got[k][won] == v).all() and np.isnan(got[k][~won]).all()
    # (b) the CPU checker's kernel model with the same (a, b, c) everywhere
    want = DE.dfkernel_uniform(port_ns, sam, ref, abc, p["Nw"], p["max_shift"], roi, assign, subpx)
    st = assert_parity(got, want, p["max_shift"], "ddf one candidate %d port" % n, allow_illposed=ILLPOSED, subpx=subpx)
    # (c) the reference's recorded maps
    st2 = assert_parity(got, DE.golden_maps(n), p["max_shift"], "ddf one candidate %d reference" % n, allow_illposed=ILLPOSED,
                        subpx=subpx, f_on_failed=False)
    print("one candidate %d: %d ok, unconverged %d (port) %d (reference)" % (n, st["ok"], st["unconverged"], st2["unconverged"]))
    # the maps go straight into the kernel model: same shape, same coordinates
    km = umpa_amd.UMPAModelDFKernel(list(sam), list(ref), window_size=p["Nw"], max_shift=p["max_shift"])
    c0, c1 = km.coords(ROI=roi) if roi is not None else km.coords()
    s0, s1 = s.coords(ROI=roi)
    np.testing.assert_array_equal(c0, s0)
    np.testing.assert_array_equal(c1, s1)
    assert got["a"].shape == (len(c0), len(c1))


def test_sequence_of_candidates_on_one_searcher(ddf):
    """A, B, A on one searcher: nothing of an earlier candidate (the reference-side maps above all) survives into a later one."""
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    A, B = DE.KERNELS[1], DE.KERNELS[2]
    s = _search(ddf, sam, ref, p["Nw"], p["max_shift"], debug=False)
    seq = s.match([A, B, A], keep=True)
    assert seq["f_all"].shape == (3,) + seq["f"].shape and seq["err_all"].dtype == np.int32
    for m, abc in enumerate((A, B)):
        fresh = _search(ddf, sam, ref, p["Nw"], p["max_shift"], debug=False).match([abc], keep=True)
        np.testing.assert_array_equal(seq["f_all"][m], fresh["f_all"][0])
        np.testing.assert_array_equal(seq["err_all"][m], fresh["err_all"][0])
        np.testing.assert_array_equal(fresh["f"], fresh["f_all"][0])
    np.testing.assert_array_equal(seq["f_all"][2], seq["f_all"][0])
    np.testing.assert_array_equal(seq["err_all"][2], seq["err_all"][0])
    assert not (seq["index"] == 2).any()                              # equal costs: the first stays
    assert (seq["f_all"][1] != seq["f_all"][0]).any()
    # and a second call on the same searcher repeats the first
    again = s.match([A, B, A], keep=True)
    for k in ("index", "f", "T", "dx", "dy", "err", "f_all"):
        np.testing.assert_array_equal(again[k], seq[k], err_msg=k)


# ----------------------------------------------------------------------------- fold

def test_fold_of_a_search_equals_the_numpy_fold(ddf):
    import umpa_amd
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    cand = np.array([DE.KERNELS[3], DE.KERNELS[0], DE.KERNELS[1], DE.KERNELS[2], (50.0, 0.0, 50.0), (0.3, 0.0, 0.3)])
    got = _search(ddf, sam, ref, p["Nw"], p["max_shift"], debug=False).match(cand, keep=True)
    per = []
    for m, abc in enumerate(cand):
        one = _search(ddf, sam, ref, p["Nw"], p["max_shift"], debug=False).match([abc])
        np.testing.assert_array_equal(one["f"], got["f_all"][m])
        np.testing.assert_array_equal(one["err"], got["err_all"][m])
        per.append({k: one[k] for k in ("f", "T", "dx", "dy", "err")})
    want = DE.fold(per)
    for k in ("index", "f", "T", "dx", "dy", "err"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    won = want["index"] >= 0
    for n_, k in enumerate("abc"):
        np.testing.assert_array_equal(got[k][won], cand[want["index"][won], n_])
        assert np.isnan(got[k][~won]).all()
    assert len(np.unique(want["index"])) >= 4                         # the candidates really compete
    s1, s2, th = ddf.sigma_from_kernel(got["a"], got["b"], got["c"])
    for k, v in (("sigma_major", s1), ("sigma_minor", s2), ("theta", th)):
        np.testing.assert_array_equal(got[k], v)
    # the abc maps go straight into the kernel model
    abc_map = np.stack([np.where(won, got[k], 0.1) for k in "abc"], axis=-1)
    abc_map[~won, 1] = 0.0
    km = umpa_amd.UMPAModelDFKernel(list(sam), list(ref), window_size=p["Nw"], max_shift=p["max_shift"])
    assert km.match(abc=abc_map, quiet=True)["f"].shape == got["f"].shape


def test_fold_where_the_first_candidate_fails_on_a_patch(ddf):
    """A sample patch moved by more than the search box fails for the candidate that keeps the speckle sharp; -1 only where
    every candidate fails."""
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    got = _search(ddf, sam, ref, p["Nw"], p["max_shift"], debug=False).match([DE.KERNELS[3], DE.KERNELS[1], DE.KERNELS[0]], keep=True)
    all_fail = (got["err_all"] != 1).all(axis=0)
    first_fails = got["err_all"][0] != 1
    assert first_fails.sum() > 100 and (first_fails & ~all_fail).sum() > 100 and all_fail.sum() > 0
    np.testing.assert_array_equal(got["index"] == -1, all_fail)
    np.testing.assert_array_equal(got["err"] == 0, all_fail)
    assert (got["index"][first_fails & ~all_fail] > 0).all()
    np.testing.assert_array_equal(got["f"][all_fail], got["f_all"][0][all_fail])   # the first candidate's maps stay there


def test_fold_hand_made_planes_through_the_c_abi(ddf):
    planes = DE.hand_made_planes()
    want = DE.fold(planes)
    shape = planes[0]["err"].shape
    best = [np.full(shape, 7.0) for _ in range(4)] + [np.full(shape, 5, dtype=np.int32) for _ in range(2)]
    for m, p in enumerate(planes):
        ddf.fold(m, [np.ascontiguousarray(p[k]) for k in ("f", "T", "dx", "dy", "err")], best)
    for k, got in zip(("f", "T", "dx", "dy", "index", "err"), best):
        np.testing.assert_array_equal(got, want[k], err_msg=k)
    # the same on device planes, on a side stream
    import torch
    from umpa_amd import _lib
    lib = _lib.ddf()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dbest = [torch.full((want["f"].size,), 7.0, dtype=torch.float64, device="cuda") for _ in range(4)] + \
                [torch.full((want["f"].size,), 5, dtype=torch.int32, device="cuda") for _ in range(2)]
        for m, p in enumerate(planes):
            dc = [torch.from_numpy(np.ascontiguousarray(p[k]).reshape(-1)).cuda() for k in ("f", "T", "dx", "dy", "err")]
            rc = lib.fold(m, want["f"].size, *[t.data_ptr() for t in dc], *[t.data_ptr() for t in dbest],
                          torch.cuda.current_device(), _lib.F_DEVICE_IO, side.cuda_stream)
            assert rc == 0, lib.error()
    side.synchronize()
    for k, got in zip(("f", "T", "dx", "dy", "index", "err"), dbest):
        np.testing.assert_array_equal(got.cpu().numpy().reshape(shape), want[k], err_msg=k)


# ----------------------------------------------------------------------------- recovery

def test_recovery(ddf):
    """Two known kernels, left and right: the GPU's index equals the restatement's loop everywhere except on pixels the
    parity classification marks unconverged for some candidate (cap: 1 % of the pixels)."""
    from oracle import parity
    sam, ref, cand = DE.recovery_case()
    p = DE.RECOVERY
    want, per = DE.recovery_search()
    s = _search(ddf, sam, ref, p["Nw"], p["max_shift"], debug=True)
    got = s.match(cand, keep=True)
    assert got["index"].shape == want["index"].shape
    differ = np.argwhere(got["index"] != want["index"])
    unconverged = 0
    for xi, xj in differ:
        ill = any(parity.newton_unconverged(q["debug_a"][xi, xj], q["debug_d"][xi, xj]) or
                  parity.newton_unstable(q["debug_a"][xi, xj], q["debug_d"][xi, xj]) for q in per if q["err"][xi, xj] == 1)
        assert ill, "pixel (%d, %d): index %d, restatement %d, every candidate's Newton iteration converged; costs %r against %r" % (
            xi, xj, got["index"][xi, xj], want["index"][xi, xj], got["f_all"][:, xi, xj], [q["f"][xi, xj] for q in per])
        unconverged += 1
    print("recovery: %d of %d pixels differ from the restatement (all unconverged for some candidate)" % (unconverged, want["index"].size))
    assert unconverged <= 0.01 * want["index"].size
    truth, far = DE.recovery_truth()
    share = (got["index"] == truth)[far].mean()
    ok = got["err"] == 1
    print("recovery: the GPU names the true candidate on %.1f %% of the pixels away from the seam; median dx %.3f dy %.3f" % (
        100 * share, np.median(got["dx"][ok]), np.median(got["dy"][ok])))
    same = got["index"] == want["index"]
    sel = same & ok
    assert np.abs(got["T"] - want["T"])[sel].max() <= 1e-5 * np.abs(want["T"][sel]).max()   # the winner's maps are its own


# ----------------------------------------------------------------------------- refusals

def test_refusals_on_the_gpu(ddf):
    from umpa_amd import _lib
    sam, ref = DE.identity_stack()
    with pytest.raises(ValueError, match="no masks"):
        ddf.KernelSearch(list(sam), list(ref), mask_list=[np.ones_like(x) for x in sam])
    with pytest.raises(ValueError, match="no pos_list"):
        ddf.KernelSearch(list(sam), list(ref), pos_list=[(0, 0)] * len(sam))
    with pytest.raises(ValueError, match="smaller than the 17 x 17 kernel"):
        ddf.KernelSearch([np.ones((16, 64))], [np.ones((16, 64))])
    with pytest.raises(ValueError, match="smaller than the 17 x 17 kernel"):
        ddf.blur_frames(np.ones((16, 64)), (0.1, 0.0, 0.1))
    s = ddf.KernelSearch(list(sam), list(ref), window_size=2, max_shift=4)
    with pytest.raises(ValueError, match="candidate 1.*inadmissible"):
        s.match([(0.1, 0.0, 0.1), (1.0, 3.0, 1.0)])                   # indefinite
    with pytest.raises(ValueError, match="empty"):
        s.match([])
    with pytest.raises(RuntimeError, match="exceeds the reconstructible extent"):
        s.match([(0.1, 0.0, 0.1)], ROI=((0, 40, 1), (0, 44, 1)))      # the plain model's extent is not this search's
    # the library itself
    lib = _lib.ddf()
    vp = ctypes.c_void_p
    a, o, g = np.ones((16, 40)), np.zeros((16, 40)), np.full(289, 1.0 / 289)
    rc = lib.blur((vp * 1)(a.ctypes.data), (vp * 1)(o.ctypes.data), 1, 16, 40, g.ctypes.data_as(vp), 0, 0, None)
    assert rc == -1 and "smaller than the 17 x 17 kernel" in lib.error()
    # and the searcher still works after the refusals
    assert s.match([(0.1, 0.0, 0.1)])["f"].shape == (36, 44)
