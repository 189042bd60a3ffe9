"""
The per-pixel uncertainty maps on the GPU (libumpa_sigma.so, umpa_amd/sigma.py).  tests/sigma_expect.py, the numpy
restatement of include/umpa_sigma.h, is the expectation: the moments lie within the header's rounding bound of an
np.longdouble evaluation, and unit, s2, dof and valid are EQUAL, bit for bit, to the restated solve fed the GPU's own
moments (+ - * / in a fixed order, compiled without contraction).

REACHES names, per test, the kernels of libumpa_sigma.so it is there for (tests/test_sigma_cpu.py checks on the CPU that
every kernel of the library is claimed).  The moments kernel takes 32 x 8 pixels per workgroup, the solve kernel 256.
"""
import functools

import numpy as np
import pytest

import sigma_expect as SE

pytestmark = pytest.mark.gpu

MOMENTS = ["sigma_moments_kernel<0>", "sigma_moments_kernel<1>"]
SOLVE = ["sigma_solve_kernel<0>", "sigma_solve_kernel<1>"]
REACHES = {
    "test_hip_sigma.py::test_sums_and_solve_on_every_stack_shape": MOMENTS,
    "test_hip_sigma.py::test_the_widest_window": MOMENTS,
    "test_hip_sigma.py::test_regions_off_the_tile_size_with_offsets_and_steps": MOMENTS,
    "test_hip_sigma.py::test_skipped_and_out_of_range_shifts": MOMENTS,
    "test_hip_sigma.py::test_a_nan_and_a_constant_reference": MOMENTS,
    "test_hip_sigma.py::test_repeats_and_io_modes_are_bit_identical": MOMENTS + SOLVE,
    "test_hip_sigma.py::test_solve_on_hand_made_moments": SOLVE,
    "test_hip_sigma.py::test_model_front": MOMENTS,
}
KEYS = ("unit", "s2", "dof", "valid")


@pytest.fixture(scope="module")
def sigma():
    import torch
    assert torch.cuda.is_available()
    from umpa_amd import sigma
    return sigma


@functools.lru_cache(maxsize=None)
def _exact(H, W, K, Nw, ms, kind, reg, seed):
    """the stack, the shift field and the extended-precision moments with their bound, computed once per case"""
    sam, ref = SE.stack(H, W, K, ms, kind)
    shift = SE.random_shift(reg[2], reg[5], ms, seed)
    want, bound = SE.moments(sam, ref, SE.window(Nw), Nw, ms, kind, reg, shift, np.longdouble)
    return sam, ref, shift, want, bound


def _equal_solve(got, kind, K, win, what):
    """unit, s2, dof, valid of `got` EQUAL the restated solve on got's own moments"""
    want = SE.solve(got["moments"], kind, K, SE.window_sv(win))
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def _within_bound(mom, want, bound, what):
    live = ~np.isnan(bound)
    np.testing.assert_array_equal(np.isnan(mom), ~live, err_msg=what)
    err = np.abs(mom - want).astype(np.float64)
    worst = (err[live] / bound[live]).max()
    print("%s: worst moment error / bound = %.3f" % (what, worst))
    assert worst <= 1.0, (what, worst)


def _check(sigma, H, W, K, Nw, ms, kind, reg, seed=0):
    sam, ref, shift, want, bound = _exact(H, W, K, Nw, ms, kind, reg, seed)
    win = SE.window(Nw)
    what = "%dx%d K=%d Nw=%d ms=%d kind=%d region %r" % (H, W, K, Nw, ms, kind, reg)
    got = sigma.region(sam, ref, win, ms, kind, reg, shift, moments=True)
    _within_bound(got["moments"], want, bound, what)
    _equal_solve(got, kind, K, win, what)
    return got


@pytest.mark.parametrize("Nw,ms", [(1, 2), (2, 3), (3, 4)], ids=str)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 11])
def test_sums_and_solve_on_every_stack_shape(sigma, K, kind, Nw, ms):
    reg = SE.full_region((40, 44), Nw, ms)
    got = _check(sigma, 40, 44, K, Nw, ms, kind, reg, seed=K + Nw)
    ok = got["valid"] == 1
    assert (got["unit"][:2, ok] > 0).all() and (got["dof"][ok] > 0).all() and (got["dof"][ok] < K).all() and (got["s2"][ok] >= 0).all()
    if K > 1:                                                         # (one frame leaves few or no degrees of freedom)
        assert ok.mean() > 0.9


@pytest.mark.parametrize("kind", [0, 1])
def test_the_widest_window(sigma, kind):
    got = _check(sigma, 52, 52, 2, 8, 2, kind, SE.full_region((52, 52), 8, 2), seed=8)
    assert got["valid"].all()


# frames of 40 x 44 with Nw = 1, ms = 2 leave an extent of 34 x 38 pixels
REGIONS = [(0, 2, 17, 0, 2, 19), (1, 1, 33, 3, 2, 5), (33, 1, 1, 37, 1, 1), (2, 3, 9, 1, 1, 37), (0, 1, 8, 0, 1, 32), (0, 1, 9, 0, 1, 33), (5, 33, 1, 7, 3, 11)]


@pytest.mark.parametrize("reg", REGIONS, ids=str)
def test_regions_off_the_tile_size_with_offsets_and_steps(sigma, reg):
    got = _check(sigma, 40, 44, 3, 1, 2, 1, reg, seed=sum(reg))
    if reg[2] * reg[5] > 1:                                           # the same pixels as the whole extent's
        sam, ref, shift, _, _ = _exact(40, 44, 3, 1, 2, 1, reg, sum(reg))
        full = SE.full_region((40, 44), 1, 2)
        big = np.zeros((2, full[2], full[5]), dtype=np.int32)
        rows, cols = reg[0] + reg[1] * np.arange(reg[2]), reg[3] + reg[4] * np.arange(reg[5])
        big[:, rows[:, None], cols[None, :]] = shift
        whole = sigma.region(sam, ref, SE.window(1), 2, 1, full, big, moments=True)
        np.testing.assert_array_equal(whole["moments"][:, rows[:, None], cols[None, :]], got["moments"])
        np.testing.assert_array_equal(whole["unit"][:, rows[:, None], cols[None, :]], got["unit"])


@pytest.mark.parametrize("kind", [0, 1])
def test_skipped_and_out_of_range_shifts(sigma, kind):
    """The sentinel and shifts beyond +-(ms - 1), huge ones at the frame's corners included, are skipped before any address
    is formed: NaN, valid = 0, and every other pixel is what it is without them."""
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    reg = SE.full_region((H, W), Nw, ms)
    sam, ref, shift, want, bound = _exact(H, W, K, Nw, ms, kind, reg, 21)
    win = SE.window(Nw)
    clean = sigma.region(sam, ref, win, ms, kind, reg, shift, moments=True)
    bad = shift.copy()
    spots = {(0, 0): (2 ** 31 - 1, 0), (0, reg[5] - 1): (0, -2 ** 31), (reg[2] - 1, 0): (-10 ** 6, 10 ** 6), (reg[2] - 1, reg[5] - 1): (ms, 0),
             (5, 7): (sigma.SKIP, sigma.SKIP), (6, 7): (0, -ms), (17, 40 - 2 * (Nw + ms)): (ms - 1, ms), (9, 9): (-ms, ms - 1)}
    for (i, j), s in spots.items():
        bad[:, i, j] = s
    got = sigma.region(sam, ref, win, ms, kind, reg, bad, moments=True)
    skipped = np.zeros(shift.shape[1:], dtype=bool)
    for i, j in spots:
        skipped[i, j] = True
    np.testing.assert_array_equal(~SE.guard(bad, ms), skipped)
    assert (got["valid"][skipped] == 0).all()
    for k in ("moments", "unit", "s2", "dof"):
        assert np.isnan(got[k][..., skipped]).all(), k
        np.testing.assert_array_equal(got[k][..., ~skipped], clean[k][..., ~skipped], err_msg=k)
    np.testing.assert_array_equal(got["valid"][~skipped], clean["valid"][~skipped])
    _equal_solve(got, kind, K, win, "with skipped pixels")


@pytest.mark.parametrize("kind", [0, 1])
def test_a_nan_and_a_constant_reference(sigma, kind):
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    reg = SE.full_region((H, W), Nw, ms)
    sam, ref, shift, _, _ = _exact(H, W, K, Nw, ms, kind, reg, 21)
    win = SE.window(Nw)
    assert sigma.region(sam, ref, win, ms, kind, reg, shift)["valid"].all()
    bad = sam.copy()
    bad[1, 14, 17] = np.nan
    got = sigma.region(bad, ref, win, ms, kind, reg, shift, moments=True)
    i, j = np.indices((reg[2], reg[5]))
    holds = (np.abs(i + Nw + ms - 14) <= Nw) & (np.abs(j + Nw + ms - 17) <= Nw)
    assert holds.sum() == 25
    np.testing.assert_array_equal(got["valid"] == 0, holds)           # exactly the pixels whose window holds the NaN
    assert np.isnan(got["unit"][:, holds]).all() and np.isnan(got["s2"][holds]).all() and np.isnan(got["dof"][holds]).all()
    _equal_solve(got, kind, K, win, "a NaN in sam")
    flat = sigma.region(sam, np.full_like(ref, 1.25), win, ms, kind, reg, shift, moments=True)
    assert (flat["valid"] == 0).all() and np.isnan(flat["unit"]).all() and np.isnan(flat["s2"]).all() and np.isnan(flat["dof"]).all()
    assert (flat["moments"][SE.S00] == 0).all() and (flat["moments"][SE.S22] > 0).all()
    _equal_solve(flat, kind, K, win, "a constant reference")


@pytest.mark.parametrize("kind", [0, 1])
def test_repeats_and_io_modes_are_bit_identical(sigma, kind):
    import torch
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    reg = (1, 1, 27, 0, 2, 17)
    sam, ref, shift, _, _ = _exact(H, W, K, Nw, ms, kind, reg, 33)
    win = SE.window(Nw)
    first = sigma.region(sam, ref, win, ms, kind, reg, shift, moments=True)
    again = sigma.region(sam, ref, win, ms, kind, reg, shift, moments=True)
    plain = sigma.region(sam, ref, win, ms, kind, reg, shift)         # without the moments: the same results
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        t = [torch.from_numpy(np.array(a)).to(dev) for a in (sam, ref, shift)]
        on_dev = sigma.region(t[0], t[1], win, ms, kind, reg, t[2], moments=True)
        solved = sigma.solve(on_dev["moments"], kind, K, SE.window_sv(win))
        assert all(v.is_cuda for v in on_dev.values()) and all(v.is_cuda for v in solved.values())
    side.synchronize()
    hosted = sigma.solve(first["moments"], kind, K, SE.window_sv(win))
    for k in KEYS + ("moments",):
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
        np.testing.assert_array_equal(on_dev[k].cpu().numpy(), first[k], err_msg=k)
        if k != "moments":
            np.testing.assert_array_equal(plain[k], first[k], err_msg=k)
            np.testing.assert_array_equal(solved[k].cpu().numpy(), first[k], err_msg=k)
            np.testing.assert_array_equal(hosted[k], first[k], err_msg=k)


@pytest.mark.parametrize("kind", [0, 1])
def test_solve_on_hand_made_moments(sigma, kind):
    """umpa_sigma_solve on moments the caller supplies: restated ones of 300 pixels (off the 256 of a workgroup), some of
    them spoiled by hand: zeros (0 / 0), a negative and an infinite first pivot, a NaN, a huge residual."""
    Nw, ms, K = 2, 3, 4
    sam, ref = SE.stack(40, 44, K, ms, kind)
    reg = (0, 1, 10, 0, 1, 30)
    win = SE.window(Nw)
    m = SE.restated(sam, ref, win, Nw, ms, kind, reg, SE.random_shift(10, 30, ms, 2))["moments"].reshape(SE.PLANES[kind], 300).copy()
    m[:, 0] = 0.0
    m[SE.S00, 1] = -1e3
    m[SE.S00, 2] = np.inf
    m[SE.V12, 3] = np.nan
    m[SE.QQ, 4] *= 4.0
    m[:, 299] *= 3.0                                                  # a scaled stack: the same unit, 3 x s2 ... up to rounding
    sv = SE.window_sv(win)
    want = SE.solve(m, kind, K, sv)
    np.testing.assert_array_equal(want["valid"][:6], [0, 0, 0, 0, 1, 1])
    got = sigma.solve(m, kind, K, sv)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    shaped = sigma.solve(m.reshape(-1, 10, 30), kind, K, sv)
    np.testing.assert_array_equal(shaped["unit"].reshape(3, 300), got["unit"])
    one = sigma.solve(m[:, 7:8], kind, K, sv)
    np.testing.assert_array_equal(one["unit"][:, 0], got["unit"][:, 7])


@pytest.mark.parametrize("cls", ["UMPAModelNoDF", "UMPAModelDF"])
def test_model_front(sigma, cls):
    """model.uncertainty(model.match()) against the restatement, through host frames and through borrowed device frames."""
    import torch
    import umpa_amd
    Nw, ms, K = 2, 4, 4
    kind = int(cls == "UMPAModelDF")
    sam, ref = SE.stack(48, 56, K, ms, kind, noise=0.02, amplitude=1.7)
    model = getattr(umpa_amd, cls)(list(sam), list(ref), window_size=Nw, max_shift=ms, device=0)
    res = model.match(quiet=True)
    unc = model.uncertainty(res)
    assert isinstance(unc, umpa_amd.Uncertainty)
    reg = SE.full_region(sam.shape, Nw, ms)
    shift = SE.shift_field(res, ms)
    np.testing.assert_array_equal(sigma.shift_field(res, ms), shift)
    assert len(np.unique(shift[shift != SE.SKIP])) >= 3
    np.testing.assert_array_equal(model.window, SE.window(Nw))
    direct = sigma.region(sam, ref, model.window, ms, kind, reg, shift, moments=True)
    for k, v in (("unit", unc.unit), ("s2", unc.s2), ("dof", unc.dof)):
        np.testing.assert_array_equal(v, direct[k], err_msg=k)
    want = SE.restated(sam, ref, SE.window(Nw), Nw, ms, kind, reg, shift)
    both = (want["valid"] == 1) & (direct["valid"] == 1)
    assert both.mean() > 0.9
    sdy, sdx = SE.sigmas(want)
    np.testing.assert_allclose(unc.sigma_dy[both], sdy[both], rtol=1e-6)
    np.testing.assert_allclose(unc.sigma_dx[both], sdx[both], rtol=1e-6)
    known = model.uncertainty(res, noise_var=4e-4)
    np.testing.assert_array_equal(known.sigma_dx, np.sqrt(4e-4 * direct["unit"][1]))
    w = unc.weight()
    assert w.shape == res["dx"].shape and np.isfinite(w).all() and (w[unc.valid] > 0).all() and (w[~unc.valid] == 0).all()
    phi = umpa_amd.phase_from_match(res, weight=w).phi              # the weight passes straight into the integration
    pos = w > 0                                                       # (integrate() fills pixels without a positive-weight edge)
    edge = np.zeros_like(pos)
    edge[1:] |= pos[:-1]
    edge[:-1] |= pos[1:]
    edge[:, 1:] |= pos[:, :-1]
    edge[:, :-1] |= pos[:, 1:]
    assert phi.shape == w.shape and np.isfinite(phi[pos & edge]).all() and (pos & edge).mean() > 0.9
    # a region of the model: ROI and step
    part = model.match(ROI=((2, 30, 3), (1, 40, 2)), quiet=True)
    pu = model.uncertainty(part)
    rows, cols = np.arange(2, 30, 3), np.arange(1, 40, 2)
    d2 = sigma.region(sam, ref, model.window, ms, kind, (2, 3, len(rows), 1, 2, len(cols)), SE.shift_field(part, ms))
    np.testing.assert_array_equal(pu.unit, d2["unit"])
    # device frames: the planes of one stack are read where they lie
    ts, tr = torch.from_numpy(sam.copy()).to("cuda:0"), torch.from_numpy(ref.copy()).to("cuda:0")
    dmodel = getattr(umpa_amd, cls)([ts[k] for k in range(K)], [tr[k] for k in range(K)], window_size=Nw, max_shift=ms, device=0)
    assert sigma._stack(dmodel._sam).data_ptr() == ts.data_ptr()
    dunc = dmodel.uncertainty(res)
    np.testing.assert_array_equal(dunc.unit, unc.unit)
    np.testing.assert_array_equal(dunc.s2, unc.s2)
    lone = [ts[k].clone() for k in range(K)]                          # separate tensors: stacked on the device
    lmodel = getattr(umpa_amd, cls)(lone, [tr[k] for k in range(K)], window_size=Nw, max_shift=ms, device=0)
    np.testing.assert_array_equal(lmodel.uncertainty(res).unit, unc.unit)
