"""
Model-resident uncertainty maps on the GPU (umpa_grid_uncertainty of libumpa_grid.so, umpa_amd.sigma.resident and
uncertainty(resident=True)): the moments kernel runs on the model's own device frames.

Unmasked models: tests/sigma_expect.py, the numpy restatement of include/umpa_sigma.h, is the expectation.  Masked models:
tests/resident_sigma_expect.py, the restatement of the masked definition of include/umpa_grid.h.  Either way the moments lie
within the header's rounding bound of an np.longdouble evaluation, and unit, s2, dof and valid are EQUAL, bit for bit, to
the restated solve fed the GPU's own moments (+ - * / in a fixed order, compiled without contraction), NaN pixels included.

REACHES names, per test, the kernels of the family it is there for (tests/test_resident_sigma_cpu.py checks on the CPU that
every kernel of the family is claimed).  The kernel takes 32 x 8 pixels per workgroup.
"""
import ctypes
import functools

import numpy as np
import pytest

import resident_sigma_expect as RE
import sigma_expect as SE

pytestmark = pytest.mark.gpu

UNMASKED = ["resident_moments_kernel<0, false>", "resident_moments_kernel<1, false>"]
MASKED = ["resident_moments_kernel<0, true>", "resident_moments_kernel<1, true>"]
REACHES = {
    "test_hip_resident_sigma.py::test_unmasked_sums_and_solve_on_every_stack_shape": UNMASKED,
    "test_hip_resident_sigma.py::test_masked_sums_and_solve_on_every_stack_shape": MASKED,
    "test_hip_resident_sigma.py::test_the_widest_window": UNMASKED + MASKED,
    "test_hip_resident_sigma.py::test_regions_off_the_tile_size_with_offsets_and_steps": UNMASKED + MASKED,
    "test_hip_resident_sigma.py::test_skipped_and_out_of_range_shifts": UNMASKED + MASKED,
    "test_hip_resident_sigma.py::test_a_nan_with_a_live_weight_and_under_a_zero_weight": MASKED,
    "test_hip_resident_sigma.py::test_repeats_and_io_modes_are_bit_identical": UNMASKED + MASKED,
    "test_hip_resident_sigma.py::test_refusals_that_need_a_model": UNMASKED,
    "test_hip_resident_sigma.py::test_model_front": UNMASKED,
    "test_hip_resident_sigma.py::test_after_stage_sample": UNMASKED,
    "test_hip_resident_sigma.py::test_a_masked_models_track_shift_and_the_weight_into_the_integration": MASKED,
}
KEYS = ("unit", "s2", "dof", "valid")
CLS = ("UMPAModelNoDF", "UMPAModelDF")


@pytest.fixture(scope="module")
def sigma():
    import torch
    assert torch.cuda.is_available()
    from umpa_amd import sigma
    return sigma


def _model(kind, sam, ref, Nw, ms, mask=None):
    import umpa_amd
    return getattr(umpa_amd, CLS[kind])(list(sam), list(ref), mask_list=None if mask is None else list(mask), window_size=Nw,
                                        max_shift=ms, device=0)


@functools.lru_cache(maxsize=None)
def _exact(H, W, K, Nw, ms, kind, reg, seed, which=None):
    """the stack, the mask, the shift field and the extended-precision moments with their bound, computed once per case"""
    sam, ref = SE.stack(H, W, K, ms, kind)
    shift = SE.random_shift(reg[2], reg[5], ms, seed)
    win = SE.window(Nw)
    if which is None:
        want, bound = SE.moments(sam, ref, win, Nw, ms, kind, reg, shift, np.longdouble)
        return sam, ref, None, shift, want, bound
    mask = RE.masks(sam.shape, Nw, ms, seed)[which]
    want, bound = RE.moments(sam, ref, mask, win, Nw, ms, kind, reg, shift, np.longdouble)
    return sam, ref, mask, shift, want, bound


def _restated_solve(mom, kind, K, win, masked):
    return RE.solve(mom, kind) if masked else SE.solve(mom, kind, K, SE.window_sv(win))


def _equal_solve(got, kind, K, win, masked, what):
    """unit, s2, dof, valid of `got` EQUAL the restated solve on got's own moments"""
    want = _restated_solve(got["moments"], kind, K, win, masked)
    assert got["moments"].shape[0] == (RE.PLANES if masked else SE.PLANES)[kind]
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def _within_bound(mom, want, bound, what):
    live = ~np.isnan(bound)
    assert live.any()
    np.testing.assert_array_equal(np.isnan(mom), ~live, err_msg=what)
    err = np.abs(mom - want).astype(np.float64)
    pos = live & (bound > 0)
    assert (err[live & ~pos] == 0).all(), what                       # a sum without any term (a dead window) is exactly 0
    worst = (err[pos] / bound[pos]).max()
    print("%s: worst moment error / bound = %.3f" % (what, worst))
    assert worst <= 1.0, (what, worst)


def _check(sigma, H, W, K, Nw, ms, kind, reg, seed=0, which=None, model=None):
    sam, ref, mask, shift, want, bound = _exact(H, W, K, Nw, ms, kind, reg, seed, which)
    win = SE.window(Nw)
    what = "%dx%d K=%d Nw=%d ms=%d kind=%d mask=%s region %r" % (H, W, K, Nw, ms, kind, which, reg)
    model = model or _model(kind, sam, ref, Nw, ms, mask)
    got = sigma.resident(model, reg, shift, moments=True)
    _within_bound(got["moments"], want, bound, what)
    _equal_solve(got, kind, K, win, which is not None, what)
    return got


SHAPES = [(1, 2), (2, 3), (3, 4)]


@pytest.mark.parametrize("Nw,ms", SHAPES, ids=str)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 11])
def test_unmasked_sums_and_solve_on_every_stack_shape(sigma, K, kind, Nw, ms):
    reg = SE.full_region((40, 44), Nw, ms)
    got = _check(sigma, 40, 44, K, Nw, ms, kind, reg, seed=K + Nw)
    ok = got["valid"] == 1
    assert (got["unit"][:2, ok] > 0).all() and (got["dof"][ok] > 0).all() and (got["dof"][ok] < K).all() and (got["s2"][ok] >= 0).all()
    if K > 1:                                                         # (one frame leaves few or no degrees of freedom)
        assert ok.mean() > 0.9


@pytest.mark.parametrize("which", ["binary", "real"])
@pytest.mark.parametrize("Nw,ms", SHAPES, ids=str)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 11])
def test_masked_sums_and_solve_on_every_stack_shape(sigma, K, kind, Nw, ms, which):
    reg = SE.full_region((40, 44), Nw, ms)
    got = _check(sigma, 40, 44, K, Nw, ms, kind, reg, seed=K + Nw, which=which)
    dead = RE.dead_pixels((K, 40, 44), Nw, ms, reg)
    assert dead.sum() == (RE.BLOCK_ROWS - 2 * Nw) * (RE.BLOCK_COLS - 2 * Nw)
    assert (got["valid"][dead] == 0).all() and np.isnan(got["unit"][:, dead]).all() and (got["moments"][:, dead] == 0).all()
    ok = got["valid"] == 1
    # what the definition gives whatever the conditioning: dof > 0 and s2 = rss / dof >= 0 where valid, W <= K (c <= 1 / 2 for
    # weights up to 1).  (Signs of `unit` are not asserted: around the dead block windows keep as few taps as the model has
    # unknowns, A is then singular up to rounding, and the EQUAL check above already pins every bit.)
    assert (got["dof"][ok] > 0).all() and (got["s2"][ok] >= 0).all() and (got["moments"][RE.WW][~np.isnan(got["moments"][RE.WW])] <= K).all()
    if K > 1:
        assert ok[~dead].mean() > 0.85 and (got["unit"][:2, ok] > 0).mean() > 0.99


@pytest.mark.parametrize("which", [None, "real"])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_widest_window(sigma, kind, which):
    """Nw = 8: 17 x 17 taps, wider than the dead block, so every window keeps weight"""
    got = _check(sigma, 52, 52, 2, 8, 2, kind, SE.full_region((52, 52), 8, 2), seed=8, which=which)
    assert got["valid"].all()


# frames of 40 x 44 with Nw = 1, ms = 2 leave an extent of 34 x 38 pixels
REGIONS = [(0, 2, 17, 0, 2, 19), (1, 1, 33, 3, 2, 5), (33, 1, 1, 37, 1, 1), (2, 3, 9, 1, 1, 37), (0, 1, 8, 0, 1, 32), (0, 1, 9, 0, 1, 33), (5, 33, 1, 7, 3, 11)]


@functools.lru_cache(maxsize=None)
def _region_models():
    """one unmasked plain and one masked dark-field model for all the regions, and the whole extent's results per shift seed"""
    sam, ref = SE.stack(40, 44, 3, 2, 1)
    mask = RE.masks(sam.shape, 1, 2, 0)["real"]
    return {None: (0, _model(0, *SE.stack(40, 44, 3, 2, 0), 1, 2)), "real": (1, _model(1, sam, ref, 1, 2, mask))}


@pytest.mark.parametrize("which", [None, "real"])
@pytest.mark.parametrize("reg", REGIONS, ids=str)
def test_regions_off_the_tile_size_with_offsets_and_steps(sigma, reg, which):
    kind, model = _region_models()[which]
    sam, ref = SE.stack(40, 44, 3, 2, kind)
    win = SE.window(1)
    shift = SE.random_shift(reg[2], reg[5], 2, sum(reg))
    got = sigma.resident(model, reg, shift, moments=True)
    if which is None:
        want, bound = SE.moments(sam, ref, win, 1, 2, kind, reg, shift, np.longdouble)
    else:
        want, bound = RE.moments(sam, ref, RE.masks(sam.shape, 1, 2, 0)["real"], win, 1, 2, kind, reg, shift, np.longdouble)
    _within_bound(got["moments"], want, bound, str(reg))
    _equal_solve(got, kind, 3, win, which is not None, str(reg))
    if reg[2] * reg[5] > 1:                                           # the same pixels as the whole extent's
        full = SE.full_region((40, 44), 1, 2)
        big = np.zeros((2, full[2], full[5]), dtype=np.int32)
        rows, cols = reg[0] + reg[1] * np.arange(reg[2]), reg[3] + reg[4] * np.arange(reg[5])
        big[:, rows[:, None], cols[None, :]] = shift
        whole = sigma.resident(model, full, big, moments=True)
        for k in KEYS + ("moments",):
            np.testing.assert_array_equal(whole[k][..., rows[:, None], cols[None, :]], got[k], err_msg=k)


@pytest.mark.parametrize("which", [None, "binary"])
@pytest.mark.parametrize("kind", [0, 1])
def test_skipped_and_out_of_range_shifts(sigma, kind, which):
    """The sentinel and shifts beyond +-(ms - 1), huge ones at the frame's corners included, are skipped before any address
    is formed: NaN, valid = 0, and every other pixel is what it is without them."""
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    reg = SE.full_region((H, W), Nw, ms)
    sam, ref, mask, shift, want, bound = _exact(H, W, K, Nw, ms, kind, reg, 21, which)
    win = SE.window(Nw)
    model = _model(kind, sam, ref, Nw, ms, mask)
    assert (shift[:, 0, 0] == -(ms - 1)).all() and (shift[:, -1, -1] == ms - 1).all()      # both extremes at the corners
    clean = sigma.resident(model, reg, shift, moments=True)
    _within_bound(clean["moments"], want, bound, "clean")
    bad = shift.copy()
    spots = {(0, 0): (2 ** 31 - 1, 0), (0, reg[5] - 1): (0, -2 ** 31), (reg[2] - 1, 0): (-10 ** 6, 10 ** 6), (reg[2] - 1, reg[5] - 1): (ms, 0),
             (5, 7): (sigma.SKIP, sigma.SKIP), (6, 7): (0, -ms), (17, 40 - 2 * (Nw + ms)): (ms - 1, ms), (9, 9): (-ms, ms - 1)}
    for (i, j), s in spots.items():
        bad[:, i, j] = s
    got = sigma.resident(model, reg, bad, moments=True)
    skipped = np.zeros(shift.shape[1:], dtype=bool)
    for i, j in spots:
        skipped[i, j] = True
    np.testing.assert_array_equal(~SE.guard(bad, ms), skipped)
    assert (got["valid"][skipped] == 0).all()
    for k in ("moments", "unit", "s2", "dof"):
        assert np.isnan(got[k][..., skipped]).all(), k
        np.testing.assert_array_equal(got[k][..., ~skipped], clean[k][..., ~skipped], err_msg=k)
    np.testing.assert_array_equal(got["valid"][~skipped], clean["valid"][~skipped])
    _equal_solve(got, kind, K, win, which is not None, "with skipped pixels")


@pytest.mark.parametrize("kind", [0, 1])
def test_a_nan_with_a_live_weight_and_under_a_zero_weight(sigma, kind):
    """A NaN in the sample stack poisons exactly the windows that hold it, whether the mask gives the pixel weight or not
    (0 * NaN), as it poisons the reference's masked cost."""
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    pad = Nw + ms
    reg = SE.full_region((H, W), Nw, ms)
    sam, ref, mask, shift, _, _ = _exact(H, W, K, Nw, ms, kind, reg, 21, "binary")
    win = SE.window(Nw)
    clean = sigma.resident(_model(kind, sam, ref, Nw, ms, mask), reg, shift, moments=True)
    r0, c0 = RE.block_origin(sam.shape, Nw, ms)
    i, j = np.indices((reg[2], reg[5]))
    for weight in (1.0, 0.0):
        spots = [(a, b) for a, b in np.argwhere(mask[1] == weight) if a > r0 + RE.BLOCK_ROWS + 2 * Nw + 1 and 2 * pad <= b < W - 2 * pad and a < H - 2 * pad]
        bi, bj = spots[0]
        bad = sam.copy()
        bad[1, bi, bj] = np.nan
        got = sigma.resident(_model(kind, bad, ref, Nw, ms, mask), reg, shift, moments=True)
        holds = (np.abs(i + pad - bi) <= Nw) & (np.abs(j + pad - bj) <= Nw)
        assert holds.sum() == 25 and (clean["valid"][holds] == 1).any()
        assert (got["valid"][holds] == 0).all() and np.isnan(got["unit"][:, holds]).all() and np.isnan(got["s2"][holds]).all()
        for k in KEYS + ("moments",):                                 # exactly its footprint
            np.testing.assert_array_equal(got[k][..., ~holds], clean[k][..., ~holds], err_msg="%s, weight %g" % (k, weight))
        _equal_solve(got, kind, K, win, True, "a NaN in sam, weight %g" % weight)


@pytest.mark.parametrize("which", [None, "real"])
@pytest.mark.parametrize("kind", [0, 1])
def test_repeats_and_io_modes_are_bit_identical(sigma, kind, which):
    import torch
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    reg = (1, 1, 27, 0, 2, 17)
    sam, ref, mask, shift, _, _ = _exact(H, W, K, Nw, ms, kind, reg, 33, which)
    model = _model(kind, sam, ref, Nw, ms, mask)
    first = sigma.resident(model, reg, shift, moments=True)
    again = sigma.resident(model, reg, shift, moments=True)
    plain = sigma.resident(model, reg, shift)                         # without the moments: the same results
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        on_dev = sigma.resident(model, reg, torch.from_numpy(shift).to(dev), moments=True)
        assert all(v.is_cuda for v in on_dev.values())
    side.synchronize()
    for k in KEYS + ("moments",):
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
        np.testing.assert_array_equal(on_dev[k].cpu().numpy(), first[k], err_msg=k)
        if k != "moments":
            np.testing.assert_array_equal(plain[k], first[k], err_msg=k)


def test_refusals_that_need_a_model(sigma):
    """The region rule against the model's extent (UMPA_HIP_E_ARG) and the models the call does not take
    (UMPA_HIP_E_UNSUPPORTED, the text names the reason and the values); a good call after each still works."""
    import umpa_amd
    from umpa_amd import _lib
    lib = _lib.grid()
    Nw, ms, K = 2, 3, 2
    sam, ref = SE.stack(40, 44, K, ms, 0)
    reg = SE.full_region(sam.shape, Nw, ms)                           # 30 x 34 pixels
    vp = ctypes.c_void_p

    def call(model, reg):
        a = {"shift": np.zeros((2, max(reg[2], 1), max(reg[5], 1)), dtype=np.int32), "unit": np.zeros((3, max(reg[2], 1), max(reg[5], 1))),
             "s2": np.zeros((max(reg[2], 1), max(reg[5], 1))), "dof": np.zeros((max(reg[2], 1), max(reg[5], 1))),
             "valid": np.zeros((max(reg[2], 1), max(reg[5], 1)), dtype=np.int32)}
        return lib.uncertainty(model._handle, *reg, *[a[k].ctypes.data_as(vp) if k else None for k in ("shift", None, "unit", "s2", "dof", "valid")], 0, None)

    model = _model(0, sam, ref, Nw, ms)
    for bad in ((0, 1, 31, 0, 1, 4), (0, 1, 3, 0, 1, 35), (2, 3, 11, 0, 1, 4), (0, 1, 3, 3, 2, 17), (30, 1, 1, 0, 1, 1)):
        assert call(model, bad) == -1 and "region axis" in lib.error(), bad
    assert call(model, reg) == 0
    ref_mode = _model(0, sam, ref, Nw, ms)
    ref_mode.assign_coordinates = "ref"
    rc = call(ref_mode, reg)
    assert rc == -4 and "ref_mode = 1" in lib.error(), lib.error()   # UMPA_HIP_E_UNSUPPORTED
    narrow = _model(0, sam, ref, Nw, ms)
    narrow.Nw = 1
    assert call(narrow, reg) == rc and "padding = 5, Nw + max_shift = 1 + 3" in lib.error(), lib.error()
    shapes = [sam[0], np.ascontiguousarray(sam[1][:-2])]
    uneven = umpa_amd.UMPAModelNoDF(shapes, [ref[0], np.ascontiguousarray(ref[1][:-2])], window_size=Nw, max_shift=ms, device=0)
    assert call(uneven, (0, 1, 3, 0, 1, 4)) == rc and "frame 1 has 38 x 44 pixels" in lib.error(), lib.error()
    moved = umpa_amd.UMPAModelNoDF(list(sam), list(ref), pos_list=[(0, 0), (2, 1)], window_size=Nw, max_shift=ms, device=0)
    assert call(moved, (0, 1, 3, 0, 1, 4)) == rc and "at (2, 1)" in lib.error(), lib.error()
    wide = _model(0, *SE.stack(64, 64, 1, 2, 0), 9, 2)
    assert call(wide, (0, 1, 3, 0, 1, 4)) == rc and "Nw = 9" in lib.error(), lib.error()
    kern = umpa_amd.UMPAModelDFKernel(list(sam), list(ref), window_size=Nw, max_shift=ms, device=0)
    assert call(kern, (0, 1, 3, 0, 1, 4)) == rc and "kernel dark-field model" in lib.error(), lib.error()
    assert call(model, reg) == 0


@pytest.mark.parametrize("cls", CLS)
def test_model_front(sigma, cls):
    """model.uncertainty(model.match(), resident=True), through host frames and through borrowed device frames: bit-identical
    to the umpa_grid_uncertainty call, whose moments lie within the bound and whose solve equals the restated one; the default
    call (two uploaded stacks, the sibling library) agrees within both bounds."""
    import torch
    import umpa_amd
    Nw, ms, K = 2, 4, 4
    kind = int(cls == "UMPAModelDF")
    sam, ref = SE.stack(48, 56, K, ms, kind, noise=0.02, amplitude=1.7)
    win = SE.window(Nw)
    model = getattr(umpa_amd, cls)(list(sam), list(ref), window_size=Nw, max_shift=ms, device=0)
    res = model.match(quiet=True)
    unc = model.uncertainty(res, resident=True)
    assert isinstance(unc, umpa_amd.Uncertainty)
    reg = SE.full_region(sam.shape, Nw, ms)
    shift = SE.shift_field(res, ms)
    assert len(np.unique(shift[shift != SE.SKIP])) >= 3
    direct = sigma.resident(model, reg, shift, moments=True)
    for k, v in (("unit", unc.unit), ("s2", unc.s2), ("dof", unc.dof)):
        assert isinstance(v, np.ndarray)
        np.testing.assert_array_equal(v, direct[k], err_msg=k)
    np.testing.assert_array_equal(unc.valid, (direct["valid"] == 1) & np.isfinite(unc.sigma_dx) & np.isfinite(unc.sigma_dy))
    want, bound = SE.moments(sam, ref, win, Nw, ms, kind, reg, shift, np.longdouble)
    _within_bound(direct["moments"], want, bound, cls)
    _equal_solve(direct, kind, K, win, False, cls)
    sibling = sigma.region(sam, ref, model.window, ms, kind, reg, shift, moments=True)
    _within_bound(sibling["moments"], want, bound, cls + " sibling")
    old = model.uncertainty(res)
    both = unc.valid & old.valid
    assert both.mean() > 0.9
    np.testing.assert_allclose(unc.sigma_dx[both], old.sigma_dx[both], rtol=1e-6)
    np.testing.assert_allclose(unc.sigma_dy[both], old.sigma_dy[both], rtol=1e-6)
    known = model.uncertainty(res, noise_var=4e-4, resident=True)
    np.testing.assert_array_equal(known.sigma_dx, np.sqrt(4e-4 * direct["unit"][1]))
    # a region of the model: ROI and step
    part = model.match(ROI=((2, 30, 3), (1, 40, 2)), quiet=True)
    pu = model.uncertainty(part, resident=True)
    rows, cols = np.arange(2, 30, 3), np.arange(1, 40, 2)
    d2 = sigma.resident(model, (2, 3, len(rows), 1, 2, len(cols)), SE.shift_field(part, ms))
    np.testing.assert_array_equal(pu.unit, d2["unit"])
    # shift= as a host array and as a HIP tensor on the model's device
    su = model.uncertainty(part, resident=True, shift=SE.shift_field(part, ms))
    tu = model.uncertainty(part, resident=True, shift=torch.from_numpy(SE.shift_field(part, ms)).to("cuda:0"))
    for u in (su, tu):
        assert isinstance(u.unit, np.ndarray)
        np.testing.assert_array_equal(u.unit, pu.unit)
        np.testing.assert_array_equal(u.s2, pu.s2)
    # borrowed device frames, separate tensors: read where they lie, nothing is stacked
    ts, tr = torch.from_numpy(sam.copy()).to("cuda:0"), torch.from_numpy(ref.copy()).to("cuda:0")
    lone = [ts[k].clone() for k in range(K)]
    dmodel = getattr(umpa_amd, cls)(lone, [tr[k] for k in range(K)], window_size=Nw, max_shift=ms, device=0)
    dunc = dmodel.uncertainty(res, resident=True)
    np.testing.assert_array_equal(dunc.unit, unc.unit)
    np.testing.assert_array_equal(dunc.s2, unc.s2)
    np.testing.assert_array_equal(dunc.dof, unc.dof)
    with pytest.raises(ValueError, match="sam= cannot be given"):
        model.uncertainty(res, resident=True, sam=sam)


@pytest.mark.parametrize("cls", CLS)
def test_after_stage_sample(sigma, cls):
    """After stage_sample + match() the device holds a stack the model has no host copy of: resident=True reads it; the
    default call still raises without sam=, and given the stack it agrees within the bound.  (A float64 stack without dark
    and flat is staged as it is, so the expectation knows its every bit.)"""
    import umpa_amd
    Nw, ms, K = 2, 4, 4
    kind = int(cls == "UMPAModelDF")
    sam, ref = SE.stack(48, 56, K, ms, kind, noise=0.02, amplitude=1.7)       # (test_model_front's: most minima inside the box)
    sam2 = np.ascontiguousarray(1.25 * sam + 0.01 * np.random.default_rng(5).standard_normal(sam.shape))   # still matches ref
    win = SE.window(Nw)
    model = getattr(umpa_amd, cls)(list(sam), list(ref), window_size=Nw, max_shift=ms, device=0)
    reg = SE.full_region(sam.shape, Nw, ms)
    first = model.match(quiet=True)
    before = sigma.resident(model, reg, SE.shift_field(first, ms), moments=True)
    model.stage_sample(list(sam2))
    # staged, not adopted: the stack the last match adopted is still the one that is read
    pending = sigma.resident(model, reg, SE.shift_field(first, ms), moments=True)
    for k in KEYS + ("moments",):
        np.testing.assert_array_equal(pending[k], before[k], err_msg=k)
    res = model.match(quiet=True)
    shift = SE.shift_field(res, ms)
    with pytest.raises(RuntimeError, match="the sample stack was staged"):
        model.uncertainty(res)
    unc = model.uncertainty(res, resident=True)
    got = sigma.resident(model, reg, shift, moments=True)
    np.testing.assert_array_equal(unc.unit, got["unit"])
    np.testing.assert_array_equal(unc.s2, got["s2"])
    want, bound = SE.moments(sam2, ref, win, Nw, ms, kind, reg, shift, np.longdouble)
    _within_bound(got["moments"], want, bound, cls + " staged")
    _equal_solve(got, kind, K, win, False, cls + " staged")
    assert not np.array_equal(got["moments"][SE.QQ], before["moments"][SE.QQ])
    given = model.uncertainty(res, sam=sam2)
    sib = sigma.region(sam2, ref, model.window, ms, kind, reg, shift, moments=True)
    _within_bound(sib["moments"], want, bound, cls + " staged, sibling")
    np.testing.assert_array_equal(given.unit, sib["unit"])
    both = unc.valid & given.valid
    assert both.mean() > 0.8 and (unc.valid == given.valid).mean() > 0.99
    np.testing.assert_allclose(unc.sigma_dx[both], given.sigma_dx[both], rtol=1e-6)
    np.testing.assert_allclose(unc.sigma_dy[both], given.sigma_dy[both], rtol=1e-6)


@pytest.mark.parametrize("cls", CLS)
def test_a_masked_models_track_shift_and_the_weight_into_the_integration(sigma, cls):
    """A masked model: match() -> uncertainty(resident=True) -> weight() -> phase_from_match; and the integer shift of its
    track() passed as shift=, as host arrays and as HIP tensors."""
    import torch
    import umpa_amd
    Nw, ms, K = 2, 4, 4
    kind = int(cls == "UMPAModelDF")
    sam, ref = SE.stack(48, 56, K, ms, kind, noise=0.02, amplitude=1.7)
    mask = RE.masks(sam.shape, Nw, ms, 3)["binary"]
    win = SE.window(Nw)
    model = getattr(umpa_amd, cls)(list(sam), list(ref), mask_list=list(mask), window_size=Nw, max_shift=ms, device=0)
    res = model.match(quiet=True)
    with pytest.raises(RuntimeError, match="masked models are not supported"):
        model.uncertainty(res)
    unc = model.uncertainty(res, resident=True)
    reg = SE.full_region(sam.shape, Nw, ms)
    shift = SE.shift_field(res, ms)
    direct = sigma.resident(model, reg, shift, moments=True)
    np.testing.assert_array_equal(unc.unit, direct["unit"])
    want, bound = RE.moments(sam, ref, mask, win, Nw, ms, kind, reg, shift, np.longdouble)
    _within_bound(direct["moments"], want, bound, cls)
    _equal_solve(direct, kind, K, win, True, cls)
    dead = RE.dead_pixels(sam.shape, Nw, ms, reg)
    assert dead.sum() == 24 and not unc.valid[dead].any()
    w = unc.weight()
    assert w.shape == res["dx"].shape and np.isfinite(w).all() and (w[unc.valid] > 0).all() and (w[~unc.valid] == 0).all()
    assert unc.valid.mean() > 0.7
    phi = umpa_amd.phase_from_match(res, weight=w).phi
    pos = w > 0
    edge = np.zeros_like(pos)
    edge[1:] |= pos[:-1]
    edge[:-1] |= pos[1:]
    edge[:, 1:] |= pos[:, :-1]
    edge[:, :-1] |= pos[:, 1:]
    assert phi.shape == w.shape and np.isfinite(phi[pos & edge]).all()
    # track() on the masked model: its integer shift as shift=
    model.masked_grid = True
    tr = model.track(res["dx"], res["dy"])
    ts = np.ascontiguousarray(tr["shift"])
    assert ts.dtype == np.int32 and ts.shape == (2,) + res["dx"].shape and SE.guard(ts, ms).all()
    tu = model.uncertainty(tr, resident=True, shift=ts)
    td = sigma.resident(model, reg, ts, moments=True)
    np.testing.assert_array_equal(tu.unit, td["unit"])
    want, bound = RE.moments(sam, ref, mask, win, Nw, ms, kind, reg, ts, np.longdouble)
    _within_bound(td["moments"], want, bound, cls + " track")
    _equal_solve(td, kind, K, win, True, cls + " track")
    assert (td["valid"][dead] == 0).all() and (td["valid"] == 1).mean() > 0.5
    on_dev = model.uncertainty(tr, resident=True, shift=torch.from_numpy(ts).to("cuda:0"))
    np.testing.assert_array_equal(on_dev.unit, tu.unit)
    np.testing.assert_array_equal(on_dev.dof, tu.dof)
