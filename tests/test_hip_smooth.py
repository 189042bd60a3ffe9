"""
The regularised shift search on the GPU (libumpa_smooth.so, umpa_amd/smooth.py).  tests/smooth_expect.py, the numpy
restatement of include/umpa_smooth.h, is the expectation, and EQUALITY is the bar for total, shift, smin, margin and valid:
the operation is made of fp64 additions, subtractions and comparisons in a fixed order.

REACHES names, per test, the kernels of libumpa_smooth.so it is there for (tests/test_smooth_cpu.py checks on the CPU that
every kernel of the library is claimed).  The marching kernel takes 8 columns per workgroup (16 from 3072 columns on), the transpose 32 x 32 tiles
(the horizontal passes march over the transposed volume: there N0 is the column count), the selection 256 pixels.
"""
import numpy as np
import pytest

import smooth_expect as SE

pytestmark = pytest.mark.gpu

US = (3, 5, 7, 9, 11, 13, 15)
PATH = lambda U, TW=8: ["smooth_path_kernel<%d, %d, false>" % (U, TW), "smooth_path_kernel<%d, %d, true>" % (U, TW)]
SELECT = lambda U: ["smooth_select_kernel<%d>" % U]
TRANSPOSE = ["smooth_transpose_kernel<false>", "smooth_transpose_kernel<true>"]
REACHES = {
    "test_hip_smooth.py::test_every_u_with_all_eight_directions": sum((PATH(U) + SELECT(U) for U in US), []) + TRANSPOSE,
    "test_hip_smooth.py::test_each_direction_alone_and_the_path_sets": PATH(5) + PATH(9) + SELECT(5) + SELECT(9) + TRANSPOSE,
    "test_hip_smooth.py::test_wide_regions_take_the_16_column_kernel": sum((PATH(U, 16) + SELECT(U) for U in US), []) + TRANSPOSE,
    "test_hip_smooth.py::test_shapes": PATH(5) + SELECT(5) + TRANSPOSE,
    "test_hip_smooth.py::test_special_cost_entries": PATH(5) + SELECT(5) + TRANSPOSE,
    "test_hip_smooth.py::test_parameter_edge_cases": PATH(5) + SELECT(5) + TRANSPOSE,
    "test_hip_smooth.py::test_repeats_and_io_modes_are_bit_identical": PATH(9) + SELECT(9) + TRANSPOSE,
    "test_hip_smooth.py::test_match_smooth": PATH(9) + SELECT(9) + TRANSPOSE,
}
KEYS = ("total", "shift", "smin", "margin", "valid")


@pytest.fixture(scope="module")
def smooth():
    import torch
    assert torch.cuda.is_available()
    from umpa_amd import smooth
    return smooth


def _equal(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def _check(smooth, cost, lam, trunc, what, **kw):
    got = smooth.aggregate(cost, lam, trunc, return_total=True, **kw)
    dirs = kw.get("dirs", 0x0F if kw.get("paths", 8) == 4 else 0xFF)
    want = SE.aggregate(cost, lam, trunc, dirs)
    _equal(got, want, what)
    return got


@pytest.mark.parametrize("U", US)
def test_every_u_with_all_eight_directions(smooth, U):
    cost = SE.with_specials(SE.random_volume(U, 19, 23, U), 100 + U)
    got = _check(smooth, cost, 0.5, 2.25, "U = %d" % U)
    assert got["valid"].min() == 0 and got["valid"].max() == 1
    assert len(np.unique(got["shift"])) >= 3
    flat = _check(smooth, cost.reshape(U * U, 19, 23), 0.5, 2.25, "U = %d, [U * U, N0, N1]" % U)
    np.testing.assert_array_equal(flat["total"].reshape(cost.shape), got["total"])


@pytest.mark.parametrize("U", [5, 9])
def test_each_direction_alone_and_the_path_sets(smooth, U):
    cost = SE.with_specials(SE.random_volume(U, 22, 37, 3 * U), 7 * U)
    seen = []
    for d in range(8):
        got = _check(smooth, cost, 1.0, 3.5, "U = %d, direction %d" % (U, d), dirs=1 << d)
        np.testing.assert_array_equal(got["total"], SE.path_cost(cost, 1.0, 3.5, d))
        seen.append(got["total"])
    for a in range(8):
        for b in range(a):
            assert not np.array_equal(seen[a], seen[b]), (a, b)       # eight different passes
    four = _check(smooth, cost, 1.0, 3.5, "U = %d, 4 paths" % U, paths=4)
    eight = _check(smooth, cost, 1.0, 3.5, "U = %d, 8 paths" % U, paths=8)
    assert not np.array_equal(four["total"], eight["total"])
    _check(smooth, cost, 1.0, 3.5, "U = %d, the diagonals" % U, dirs=0xF0)
    _check(smooth, cost, 1.0, 3.5, "U = %d, the rows and one diagonal" % U, dirs=0x23)


# paths of length 1; diagonals that wrap several times over two-plus lane tiles, both ways round; a column count below one
# tile of the march (8), one past a tile, one past two tiles, a multiple; the same for the transpose's tiles (32) in both
# directions (for the horizontal passes N0 is the march's column count)
SHAPES = [(1, 1), (1, 40), (40, 1), (37, 130), (130, 37), (21, 5), (21, 9), (17, 16), (21, 17), (21, 33), (33, 65), (65, 31)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes(smooth, shape):
    cost = SE.random_volume(5, shape[0], shape[1], shape[0] + 3 * shape[1], dyadic=False)
    got = _check(smooth, cost, 0.31, 1.7, "%d x %d" % shape)
    assert (got["valid"] == 1).all()
    if shape[0] == 1 or shape[1] == 1:                                # the diagonals' paths have length 1
        for d in (4, 5, 6, 7):
            np.testing.assert_array_equal(smooth.aggregate(cost, 0.31, 1.7, dirs=1 << d, return_total=True)["total"], cost)
    _check(smooth, SE.with_specials(cost, shape[1]), 0.31, 1.7, "%d x %d with special entries" % shape)


WIDE_FROM = 3072                                                     # columns from which the march takes 16 per workgroup


@pytest.mark.parametrize("U", US)
def test_wide_regions_take_the_16_column_kernel(smooth, U):
    """Two rows of 3073 columns: the first pass and the accumulating passes of the wide kernel, for every U.  At U = 3 also
    both sides of the switch with all eight directions, and a region of 3073 ROWS: the horizontal passes march over the
    transposed volume, whose column count that is."""
    cost = SE.with_specials(SE.random_volume(U, 2, WIDE_FROM + 1, 200 + U, dyadic=False), 300 + U)
    _check(smooth, cost, 0.31, 1.7, "U = %d, 2 x %d" % (U, WIDE_FROM + 1), dirs=0xFC)
    if U == 3:
        _check(smooth, cost, 0.31, 1.7, "2 x %d" % (WIDE_FROM + 1))
        _check(smooth, np.ascontiguousarray(cost[..., :WIDE_FROM - 1]), 0.31, 1.7, "2 x %d" % (WIDE_FROM - 1))
        _check(smooth, np.ascontiguousarray(cost[..., :WIDE_FROM]), 0.31, 1.7, "2 x %d" % WIDE_FROM)
        tall = np.ascontiguousarray(cost.transpose(0, 1, 3, 2))
        _check(smooth, tall, 0.31, 1.7, "%d x 2, the rows and one column direction" % (WIDE_FROM + 1), dirs=0x07)


@pytest.mark.parametrize("case", ["scattered", "void row", "void column", "row, column and scattered", "all void"])
def test_special_cost_entries(smooth, case):
    base = SE.random_volume(5, 26, 35, 50)
    cost = {"scattered": lambda: SE.with_specials(base, 51),
            "void row": lambda: SE.with_specials(base, 52, void_row=11, scattered=False),
            "void column": lambda: SE.with_specials(base, 53, void_col=17, scattered=False),
            "row, column and scattered": lambda: SE.with_specials(base, 54, void_row=25, void_col=0),
            "all void": lambda: np.where(np.arange(35) % 3 == 0, np.nan, np.where(np.arange(35) % 3 == 1, np.inf, -np.inf)) + 0 * base}[case]()
    got = _check(smooth, cost, 0.5, 1.5, case)
    assert not np.isnan(got["total"]).any() and not np.isnan(got["smin"]).any() and not np.isnan(got["margin"]).any()
    void = ~np.isfinite(cost).any(axis=(0, 1))
    np.testing.assert_array_equal(got["valid"], (~void).astype(np.int32))
    assert (got["total"][:, :, void] == 0).all() and (got["shift"][:, void] == 0).all()
    if case == "all void":
        assert void.all()
    else:
        assert void.any() and not void.all()
        if case == "scattered":
            assert np.isnan(cost).any() and (cost == np.inf).any() and (cost == -np.inf).any()
            assert np.isinf(got["total"][:, :, ~void]).any()          # a non-finite label of a live pixel stays +INF


EDGES = [("lam = 0", 0.0, 2.0, 1.0), ("trunc below lam", 2.0, 0.75, 1.0), ("no truncation", 0.5, np.inf, 1.0),
         ("both zero", 0.0, 0.0, 1.0), ("costs of 1e-6", 0.3e-6, 1.7e-6, 1e-6), ("costs of 1e6", 0.3e6, 1.7e6, 1e6)]


@pytest.mark.parametrize("case,lam,trunc,scale", EDGES, ids=[e[0] for e in EDGES])
def test_parameter_edge_cases(smooth, case, lam, trunc, scale):
    dyadic = scale == 1.0
    cost = SE.random_volume(5, 24, 29, 60, dyadic=dyadic, scale=scale)
    cost = SE.with_specials(cost, 61)
    got = _check(smooth, cost, lam, trunc, case)
    live = got["valid"] == 1
    if case == "both zero":                                           # no penalty at all: eight times the conditioned cost
        np.testing.assert_array_equal(got["shift"][:, live], SE.argmin_field(cost)[:, live])
    if not dyadic:
        assert abs(np.log10(np.median(got["smin"][live]) / scale)) < 1.5


def test_repeats_and_io_modes_are_bit_identical(smooth):
    import torch
    cost = SE.with_specials(SE.random_volume(9, 37, 70, 70, dyadic=False), 71)
    want = SE.aggregate(cost, 0.27, 1.9)
    first = smooth.aggregate(cost, 0.27, 1.9, return_total=True)
    _equal(first, want, "host arrays")
    again = smooth.aggregate(cost, 0.27, 1.9, return_total=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = torch.from_numpy(cost).cuda()
        dev = smooth.aggregate(t, 0.27, 1.9, return_total=True)
        lean = smooth.aggregate(t, 0.27, 1.9)                         # without `total`: the library's own volume
    side.synchronize()
    assert all(v.is_cuda for v in dev.values()) and "total" not in lean
    for k in KEYS:
        assert np.array_equal(again[k], first[k], equal_nan=True), k
        assert np.array_equal(dev[k].cpu().numpy(), first[k], equal_nan=True), k
        if k != "total":
            assert np.array_equal(lean[k].cpu().numpy(), first[k], equal_nan=True), k
    np.testing.assert_array_equal(t.cpu().numpy(), cost)              # the input is left alone
    # results the caller does not ask for: smin, margin, valid and total may each be null
    import ctypes
    from umpa_amd import _lib
    shift = np.zeros((2, 37, 70), dtype=np.int32)
    rc = _lib.smooth().aggregate(cost.ctypes.data_as(ctypes.c_void_p), 9, 37, 70, 0.27, 1.9, 0xFF, shift.ctypes.data_as(ctypes.c_void_p),
                                 None, None, None, None, 0, 0, None)
    assert rc == 0, _lib.smooth().error()
    np.testing.assert_array_equal(shift, first["shift"])


MATCH = dict(H=96, W=112, K=4, Nw=3, max_shift=5, noise=0.08)


@pytest.fixture(scope="module")
def noisy_stack():
    from umpa_amd.synth import make_stack
    p = MATCH
    sam, ref, _ = make_stack(p["H"], p["W"], p["K"], p["max_shift"], df=True, seed=5, noise=p["noise"], amplitude=2.5)
    return sam, ref


@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_match_smooth(smooth, noisy_stack, cls):
    import umpa_amd
    p = MATCH
    sam, ref = noisy_stack
    m = getattr(umpa_amd, cls)(list(sam), list(ref), window_size=p["Nw"], max_shift=p["max_shift"])
    vol = m.cost_volume()["cost"]
    assert vol.shape == (9, 9, 80, 96)
    unit = smooth.cost_scale(vol)
    assert unit > 0
    lam, trunc = 0.3 * unit, 2.5 * unit                               # stated here: no test depends on the defaults
    got = smooth.match_smooth(m, lam=lam, trunc=trunc)
    want = SE.aggregate(vol, lam, trunc)
    np.testing.assert_array_equal(got["start"], want["shift"])
    np.testing.assert_array_equal(got["margin"], want["margin"])
    np.testing.assert_array_equal(got["valid"], want["valid"])
    assert got["lam"] == lam and got["trunc"] == trunc
    plain = SE.argmin_field(vol)
    changed = (got["start"] != plain).any(axis=0).mean()
    print("%s: the regularised start differs from the per-pixel argmin on %.2f %% of the pixels" % (cls, 100 * changed))
    assert changed > 0                                                # strong noise: the regularisation does something
    ref_maps = m.match(dxdy=(got["start"][0], got["start"][1]), quiet=True)
    maps = ("f", "T", "dx", "dy", "err") + (("df",) if cls == "UMPAModelDF" else ())
    for k in maps:
        assert np.array_equal(got[k], ref_maps[k], equal_nan=True), k
    # 4 paths; a stepped ROI; a step
    four = smooth.match_smooth(m, lam=lam, trunc=trunc, paths=4)
    np.testing.assert_array_equal(four["start"], SE.aggregate(vol, lam, trunc, 0x0F)["shift"])
    roi = ((4, 60, 2), (3, 90, 3))
    sub = smooth.match_smooth(m, lam=lam, trunc=trunc, ROI=roi)
    rvol = m.cost_volume(ROI=roi)["cost"]
    assert rvol.shape == (9, 9, 28, 29) and sub["start"].shape == (2, 28, 29)
    np.testing.assert_array_equal(sub["start"], SE.aggregate(rvol, lam, trunc)["shift"])
    sub_maps = m.match(dxdy=(sub["start"][0], sub["start"][1]), ROI=roi, quiet=True)
    for k in maps:
        assert np.array_equal(sub[k], sub_maps[k], equal_nan=True), k
    m.ROI = None
    stepped = smooth.match_smooth(m, lam=lam, trunc=trunc, step=3)
    m.ROI = None
    svol = m.cost_volume(step=3)["cost"]
    np.testing.assert_array_equal(stepped["start"], SE.aggregate(svol, lam, trunc)["shift"])
    m.ROI = None
    step_maps = m.match(dxdy=(stepped["start"][0], stepped["start"][1]), step=3, quiet=True)
    for k in maps:
        assert np.array_equal(stepped[k], step_maps[k], equal_nan=True), k
    # the defaults run (their values are not tested)
    m.ROI = None
    auto = smooth.match_smooth(m)
    assert auto["lam"] > 0 and auto["trunc"] > 0 and auto["start"].shape == (2, 80, 96)


def test_match_smooth_refuses_what_cost_volume_refuses(smooth, noisy_stack):
    import umpa_amd
    p = MATCH
    sam, ref = noisy_stack
    kw = dict(window_size=p["Nw"], max_shift=p["max_shift"])
    models = {
        "masked models are not supported": umpa_amd.UMPAModelNoDF(list(sam), list(ref), mask_list=[np.ones_like(x) for x in sam], **kw),
        "pos_list": umpa_amd.UMPAModelNoDF(list(sam), list(ref), pos_list=[(0, 0), (2, 1), (1, 3), (0, 2)], **kw),
        "kernel dark-field model has no shift table": umpa_amd.UMPAModelDFKernel(list(sam), list(ref), **kw),
    }
    for text, model in models.items():
        with pytest.raises(RuntimeError) as a:
            getattr(model, "cost_volume", model._cost_volume)()      # (the kernel model has no public cost_volume)
        with pytest.raises(RuntimeError, match=text) as b:
            smooth.match_smooth(model, lam=1.0, trunc=2.0)
        assert str(a.value) == str(b.value)                           # the same message
    ok = umpa_amd.UMPAModelNoDF(list(sam), list(ref), **kw)
    with pytest.raises(RuntimeError, match="exceeds the reconstructible extent"):
        smooth.match_smooth(ok, lam=1.0, trunc=2.0, ROI=((0, 90, 1), (0, 96, 1)))
    with pytest.raises(ValueError, match="paths must be 4 or 8"):
        smooth.match_smooth(ok, lam=1.0, trunc=2.0, paths=5)
    with pytest.raises(ValueError, match="lam must be >= 0"):
        smooth.match_smooth(ok, lam=-1.0, trunc=2.0)
    assert smooth.match_smooth(ok, lam=1e-3, trunc=1e-2)["start"].shape == (2, 80, 96)   # and it still works afterwards


def test_a_workspace_beyond_the_free_device_memory_is_refused(smooth):
    """U = 15 on 2^20 x 2^20 pixels, 1.9 PB per volume, claimed for two tensors of 64 elements.  The size check sits before
    every allocation and launch: the call returns UMPA_HIP_E_UNSUPPORTED and names the bytes needed and the bytes free.  Were
    the check broken, the first hipMalloc of a volume would fail instead (UMPA_HIP_E_NOMEM): either way no kernel can run on
    the short tensors, so this test cannot write out of bounds."""
    import re
    import torch
    from umpa_amd import _lib
    lib = _lib.smooth()
    U, N = 15, 1 << 20
    vol = U * U * N * N * 8
    assert lib.workspace_bytes(U, N, N, 0xFF) == 3 * vol
    cost = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    shift = torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
    rc = lib.aggregate(cost.data_ptr(), U, N, N, 1.0, 2.0, 0xFF, shift.data_ptr(), None, None, None, None, 0, _lib.F_DEVICE_IO, None)
    assert rc == -4, (rc, lib.error())                               # UMPA_HIP_E_UNSUPPORTED
    said = re.search(r"smooth: (\d+) bytes of device memory needed for a 15 x 15 x 1048576 x 1048576 volume, (\d+) free", lib.error())
    assert said, lib.error()
    need, free = int(said.group(1)), int(said.group(2))
    assert need == 3 * vol and 0 < free < need
    torch.cuda.synchronize()
    assert (shift == 7).all() and (cost == 0).all()
    # and the library still works: a small volume against the restatement
    small = SE.with_specials(SE.random_volume(5, 19, 23, 5), 105)
    host = _check(smooth, small, 0.5, 2.25, "after the refusal")
    on_dev = smooth.aggregate(torch.from_numpy(small).cuda(), 0.5, 2.25, return_total=True)
    _equal({k: v.cpu().numpy() for k, v in on_dev.items()}, host, "after the refusal, device arrays")
