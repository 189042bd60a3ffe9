"""
model.track() / umpa_grid_track on the GPU (libumpa_grid.so).  In every case each output EQUALS the restatement of
tests/track_expect.py applied to the device's own cost_volume(with_fit=True) of the same model and region -- shift, cost,
cost0, count, found, err, T, df, and dx, dy, f bit for bit (the 4x4 fit of the sub-pixel modes -1 and 1 is the device's own
entry point for one array), pixels without an admissible basin included.

REACHES names, per test, the kernels of libumpa_grid.so it is there for (tests/test_track_cpu.py checks on the CPU that
every grid_track_kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import ctypes
import functools

import numpy as np
import pytest

import basins_expect as BE
import grid_expect as GE
import track_expect as TE

pytestmark = pytest.mark.gpu

KTEMPL = 24                      # UMPA_KTEMPL: frame counts with their own instantiation (dark-field model)
REACHES = {
    "tests/test_hip_track.py::test_every_frame_count": ["grid_track_kernel<1, %d>" % (n if n <= KTEMPL else 0) for n in range(1, KTEMPL + 2)],
    "tests/test_hip_track.py::test_cross_checks": ["grid_track_kernel<0, 0>"],
}
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _model(hip_ns, kind, sam, ref, Nw, ms, assign="sam", subpx=0, **kw):
    m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, window_size=Nw, max_shift=ms, **kw)
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    return m


def _launches(m, fn):
    """fn() with the library's timers on: (result, {kernel family: launches})"""
    lib, h = m._lib, m._handle
    lib.timing_enable(h, 1)
    try:
        out = fn()
    finally:
        lib.timing_enable(h, 0)
    seen = {}
    for q in range(lib.timing_collect(h)):
        nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
        seen[nm.value.decode()] = cnt.value
    return out, seen


def _prior(ms, shape, seed, nan_share=0.03):
    """(prior_dx, prior_dy): a seeded random field within +-(ms + 1), a few pixels blind"""
    rng = np.random.default_rng(seed)
    dx, dy = rng.uniform(-(ms + 1), ms + 1, shape), rng.uniform(-(ms + 1), ms + 1, shape)
    dx[rng.random(shape) < nan_share] = NAN
    return dx, dy


def _check(m, cases, what="", **region):
    """track() of the region for every (prior_dx, prior_dy, lam, radius) of `cases` against the restatement on the device's
    own volume: ([results], volume)"""
    vol = m.cost_volume(with_fit=True, **region)
    sub = m.sub_pixel_mode
    fit = BE.device_fit(sub, m._device) if sub else None
    res = []
    for q, (pdx, pdy, lam, radius) in enumerate(cases):
        t = m.track(pdx, pdy, lam=lam, radius=radius, **region)
        want = TE.restate(vol["cost"], vol["T"], vol.get("df"), pdy, pdx, TE.NEAREST if lam is None else TE.PENALTY,
                          0.0 if lam is None else lam, radius, sub, fit=fit)
        TE.assert_equal(t, want, "%s case %d (lam %r radius %r)" % (what, q, lam, radius))
        res.append(t)
    return res, vol


def _mid_lam(vol):
    """a penalty weight on the scale of the volume (from the volume alone): a quarter of the median gap between the two
    lowest costs of a pixel"""
    U = vol["cost"].shape[0]
    c = np.sort(np.where(np.isnan(vol["cost"]), np.inf, vol["cost"]).reshape(U * U, -1), axis=0)
    gap = (c[1] - c[0])[np.isfinite(c[1])] if U > 1 else np.ones(1)
    return float(np.median(gap) / 4.0) if gap.size else 1.0


# ----------------------------------------------------------------------------- 1. every instantiation

@pytest.mark.parametrize("K", list(range(1, KTEMPL + 2)))
def test_every_frame_count(hip_ns, K):
    from umpa_amd.synth import make_stack
    Nw, ms = 2, 3
    sam, ref, _ = make_stack(44, 80, K, ms, df=True, seed=100 + K)
    for assign in ("sam", "ref"):
        for kind in (1, 0):
            m = _model(hip_ns, kind, sam, ref, Nw, ms, assign)
            pdx, pdy = _prior(ms, m.sh, 1000 + K)
            (res, _), seen = _launches(m, lambda: _check(m, [(pdx, pdy, None, None), (pdx, pdy, 0.05, 3.0)], "K %d %s kind %d" % (K, assign, kind)))
            assert seen.get("table_consumer") == 3 and "replay_walk" not in seen, seen   # the volume and the two tracks
            assert (res[0]["count"] >= 1).all() and (res[0]["found"] == res[0]["count"]).all()
            assert (res[1]["found"] < res[1]["count"]).any() and (res[1]["found"] > 0).any()


# ----------------------------------------------------------------------------- 2. against the grid search and the basins

@functools.lru_cache(maxsize=None)
def _hp_stack():
    return GE.stack("64x72x3")


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
@pytest.mark.parametrize("subpx", [-1, 0, 1])
def test_cross_checks(hip_ns, kind, subpx):
    from umpa_amd import basins as B
    sam, ref, c = _hp_stack()
    ms = c["ms"]
    m = _model(hip_ns, kind, sam, ref, c["Nw"], ms, "sam", subpx)
    pdx, pdy = _prior(ms, m.sh, 7 + subpx, nan_share=0.0)
    vol = m.cost_volume(with_fit=True)
    (near, lam0, blind, blind_pen, mid), _ = _check(m, [(pdx, pdy, None, None), (pdx, pdy, 0.0, None), (NAN, NAN, None, None),
                                                        (pdx, NAN, 2.5, 0.0), (pdx, pdy, _mid_lam(vol), 2.5)], "subpx %d" % subpx)
    grid = m.match(quiet=True, search="grid")
    m.ROI = None
    b1, b8 = m.basins(k=1), m.basins(k=8)
    rank0 = B.select(b1, 0)
    maps = ("dx", "dy", "f", "T", "err") + (("df",) if kind else ())
    for what, t in (("lam 0", lam0), ("NaN prior", blind), ("NaN prior, penalty, radius 0", blind_pen)):
        for n in maps:
            np.testing.assert_array_equal(t[n], grid[n], err_msg="%s against search='grid': %s" % (what, n))
        for n in maps + ("cost", "shift"):
            np.testing.assert_array_equal(t[n], rank0[n], err_msg="%s against basins(k=1): %s" % (what, n))
        np.testing.assert_array_equal(t["cost"], t["cost0"])
        np.testing.assert_array_equal(t["count"], b1["count"])
    sel = B.select(b8, B.nearest(b8, pdx, pdy))
    all_kept = b8["count"] <= 8
    assert all_kept.mean() >= 0.90
    for n in maps + ("cost", "shift"):
        np.testing.assert_array_equal(near[n][..., all_kept], sel[n][..., all_kept], err_msg="nearest against select(basins(8), nearest): %s" % n)
    assert (near["cost"] > near["cost0"]).any() and (mid["found"] < mid["count"]).any()
    assert (near["err"] == 1).any() and (near["err"] == 0).any()


# ----------------------------------------------------------------------------- 3. search ranges

@pytest.mark.parametrize("ms,Nw,H,W", [(1, 2, 40, 80), (2, 2, 44, 84), (5, 3, 56, 96), (17, 2, 58, 108)], ids=["ms1", "ms2", "ms5", "ms17"])
def test_search_ranges(hip_ns, ms, Nw, H, W):
    """ms 1: a box of one shift; ms 2: no 4 x 4 neighbourhood fits; ms 17: the largest box the tiled path admits, 33 x 33
    shifts -- the LDS ring of the kernel at its limit (50,688 bytes per wave) -- where pixels have more basins than
    basins() keeps and the prior picks one of those."""
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(H, W, 3, 4, df=True, seed=300 + ms)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, "sam" if kind else "ref")
        pdx, pdy = _prior(ms, m.sh, 40 + ms)
        (near, pen), vol = _check(m, [(pdx, pdy, None, None), (pdx, pdy, 0.01, float(ms))], "ms %d kind %d" % (ms, kind))
        if ms == 1:
            assert (near["count"] == 1).all() and (near["err"] == 0).all() and (near["shift"] == 0).all()
        if ms == 2:
            assert (near["err"] == 0).all()                           # a box of 3 x 3 shifts holds no 4 x 4 neighbourhood
        if ms == 17:
            b8 = m.basins(k=8)
            kept = ((b8["shift"][:, 0] == near["shift"][0][None]) & (b8["shift"][:, 1] == near["shift"][1][None]) & (b8["err"] >= 0)).any(axis=0)
            beyond = (near["count"] > 8) & ~kept
            print("ms 17 kind %d: %.1f %% of the pixels have more than 8 basins; at %.1f %% the nearest basin is none of the 8 kept" % (
                kind, 100 * (near["count"] > 8).mean(), 100 * beyond.mean()))
            assert beyond.any() and (near["found"][beyond] > 8).all() and (near["err"] == 1).any()


def test_wide_windows_through_the_marching_table(hip_ns):
    from umpa_amd.synth import make_stack
    K, Nw, ms = 20, 7, 8
    sam, ref, _ = make_stack(2 * (Nw + ms) + 24, 2 * (Nw + ms) + 60, K, ms, df=True, seed=5, order=1)   # 24 x 60 pixels: two strips of corr_march
    for kind, assign in ((1, "sam"), (0, "ref")):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, assign)
        pdx, pdy = _prior(ms, m.sh, 50 + kind)
        _, seen = _launches(m, lambda: _check(m, [(pdx, pdy, None, 4.0), (pdx, pdy, 0.02, None)], "march kind %d" % kind))
        assert seen.get("corr_march", 0) >= 1 and seen.get("table_consumer") == 3 and "corr_volume" not in seen and "replay_walk" not in seen, seen


# ----------------------------------------------------------------------------- 4. chunks, regions

def _chunk_stack():
    from umpa_amd.synth import make_stack
    # 128 x 512 output pixels, 81 planes of 512 doubles per row: a 16 MB table holds 32 rows -> four row chunks
    return make_stack(144, 528, 4, 5, df=True, seed=9, order=1)[:2]


def test_four_row_chunks_change_nothing(hip_ns, monkeypatch):
    sam, ref = _chunk_stack()
    res = {}
    pdx, pdy = _prior(5, (128, 512), 11)
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = _model(hip_ns, 1, sam, ref, 3, 5, subpx=-1)
        res[mb], seen = _launches(m, lambda: [m.track(pdx, pdy), m.track(pdx, pdy, lam=0.02, radius=3.0)])
        assert seen.get("table_consumer") == (8 if mb else 2), (mb, seen)
    for a, b in zip(res["16"], res[None]):
        TE.assert_equal(a, {n: np.asarray(v) for n, v in b.items()}, "four chunks")


def test_roi_and_steps_are_slices_of_the_full_result(hip_ns):
    sam, ref = _chunk_stack()
    pdx, pdy = _prior(5, (128, 512), 12)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, 3, 5, subpx=-1)
        roi_before = m.ROI
        for lam, radius in ((None, 3.5), (0.02, None)):
            full = m.track(pdx, pdy, lam=lam, radius=radius)
            cut = lambda s0, s1: {n: np.ascontiguousarray(v[..., s0, s1]) for n, v in full.items()}
            for step in (2, 3):
                s = slice(None, None, step)
                TE.assert_equal(m.track(pdx[s, s], pdy[s, s], lam=lam, radius=radius, step=step), cut(s, s), "step %d" % step)
            s0, s1 = slice(17, 90, 2), slice(5, 400, 3)
            TE.assert_equal(m.track(pdx[s0, s1], pdy[s0, s1], lam=lam, radius=radius, ROI=((17, 90, 2), (5, 400, 3))), cut(s0, s1), "ROI")
        assert m.ROI == roi_before                                    # the model's own ROI is left alone


# ----------------------------------------------------------------------------- 5. special pixels, ties

@pytest.mark.parametrize("march", [False, True], ids=["corr_volume", "corr_march"])
@pytest.mark.parametrize("bad", ["nan", "+inf", "zero"])
def test_special_pixels_on_the_seams(hip_ns, bad, march):
    """NaN, Inf and 0 pixels placed as tests/regimes.py places them (tile seam, strip seam, padding border, last frame), on
    both table kernels: pixels without any basin (count = found = 0, cost0 = 0, zeros) and basins beside NaN cells must
    be the restatement's on the dirty volume."""
    import regimes
    from umpa_amd.synth import make_stack
    cfg = dict(Nw=6, K=3, ms=3, H=66, W=92) if march else dict(Nw=2, K=3, ms=3, H=60, W=70)
    sam, ref, _ = make_stack(cfg["H"], cfg["W"], cfg["K"], cfg["ms"], df=True, seed=77)
    pos = regimes.bad_positions(cfg)
    for kind, where, assign in ((1, "ref", "sam"), (0, "sam", "ref")):
        s, r = regimes.bad_pixels(sam, ref, bad, where, pos)
        m = _model(hip_ns, kind, s, r, cfg["Nw"], cfg["ms"], assign)
        pdx, pdy = _prior(cfg["ms"], m.sh, 60 + kind)
        ((near, pen), vol), seen = _launches(m, lambda: _check(m, [(pdx, pdy, None, None), (pdx, pdy, 0.05, 2.0)], "%s in %s" % (bad, where)))
        assert seen.get("corr_march" if march else "corr_volume", 0) >= 1, seen
        far = regimes.far_from(cfg, pos, near["count"].shape)
        assert (~far).any() and far.any()
        if bad != "zero":
            none = near["count"] == 0
            assert none.any() and not none[far].any()
            assert (near["found"][none] == 0).all() and (near["cost0"][none] == 0).all() and (near["err"][none] == 0).all()
            U = 2 * cfg["ms"] - 1
            with np.errstate(invalid="ignore"):
                holes = ~(vol["cost"] < np.inf).reshape(U * U, -1)
            assert ((near["count"].ravel() > 0) & holes.any(axis=0)).any()   # pixels that have basins and NaN cells in one box


def test_plateaus_equal_basins_and_empty_radii(hip_ns):
    """The two integer-valued stacks of the basins tests (the sums are exact in any order): a stack that is constant along
    the columns -- every cost row is a plateau, only its earliest member can be a basin -- and a reference of column period
    4 under ms = 4, where shifts 4 columns apart have EQUAL costs.  Priors on integers and half-integers make d2 tie as
    well, so that the cost and then the scan order decide; a radius below the distance to any shift leaves found = 0."""
    rng = np.random.default_rng(41)
    K, H, W, Nw, ms = 3, 48, 76, 2, 4
    col = rng.integers(1, 64, (K, H, 1)).astype(np.float64)
    flat_sam, flat_ref = np.repeat(col, W, axis=2), np.repeat(np.roll(col, 1, axis=1) + 3.0, W, axis=2)
    cases = [(0.5, 0.0, None, None), (-1.0, 1.0, None, None), (-1.0, 1.0, 0.0, None), (-1.0, 1.0, 1.0, 2.0), (0.5, 0.5, None, 0.75),
             (0.5, 0.5, None, 0.5), (1.0, 1.0, None, 0.0), (1.0, 1.0, 0.5, 0.0)]
    for kind in (0, 1):
        m = _model(hip_ns, kind, np.ascontiguousarray(flat_sam), np.ascontiguousarray(flat_ref), Nw, ms)
        res, vol = _check(m, cases, "column-constant kind %d" % kind)
        np.testing.assert_array_equal(vol["cost"], np.repeat(vol["cost"][:, :1], 2 * ms - 1, axis=1))   # the plateaus are exact
        got = res[0]["found"] > 0
        assert got.any() and (res[0]["shift"][1][got] == 1 - ms).all()
        assert (res[5]["found"] == 0).all() and (res[5]["err"] == 0).all() and (res[5]["count"] == res[0]["count"]).all()
    tile = rng.integers(1, 64, (K, H, 4)).astype(np.float64)
    per_ref = np.ascontiguousarray(np.tile(tile, (1, 1, W // 4)))
    sam = np.ascontiguousarray(np.roll(per_ref, (-1, -1), axis=(1, 2)) + rng.integers(0, 3, per_ref.shape))
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, per_ref, Nw, ms, "sam")
        res, vol = _check(m, cases, "period 4 kind %d" % kind)
        b = m.basins(k=8)
        pair = (b["err"][0] >= 0) & (b["err"][1] >= 0) & (b["cost"][0] == b["cost"][1])
        d = b["shift"][1] - b["shift"][0]
        assert pair.mean() > 0.5 and ((d[0][pair] == 0) & (d[1][pair] == 4)).all()
        # a prior half way between the two best basins: they are equally far and equally cheap, and where no third basin is
        # nearer, scan order decides for the first of them
        first, second = b["shift"][0], b["shift"][1]
        (half, _), _ = _check(m, [(first[1] + 2.0, first[0].astype(np.float64), None, None), (first[1] + 2.0, first[0].astype(np.float64), 1.0, 2.0)],
                              "period 4, half way, kind %d" % kind)
        tie = pair & (half["shift"][0] == first[0]) & ((half["shift"][1] == first[1]) | (half["shift"][1] == second[1]))
        print("period 4 kind %d: at %.1f %% of the pixels the two best basins tie in d2 and in cost and one of them is chosen" % (kind, 100 * tie.mean()))
        assert tie.any() and (half["shift"][1][tie] == first[1][tie]).all()
        # radius 0 around the integer prior (1, 1): exactly that shift, where it is a basin
        hit = res[6]["found"] == 1
        assert hit.any() and (res[6]["found"] <= 1).all() and (res[6]["shift"][:, hit] == 1).all()
        assert (res[5]["found"] == 0).all() and (res[4]["found"] >= res[5]["found"]).all()


# ----------------------------------------------------------------------------- 6. repeats and I/O sides

def test_repeats_device_arrays_and_a_staged_stack(hip_ns):
    import torch
    from umpa_amd import _lib
    sam, ref, c = _hp_stack()
    sam2 = np.ascontiguousarray(1.25 * sam[::-1])
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        pdx, pdy = _prior(c["ms"], m.sh, 70)
        host = m.track(pdx, pdy, lam=0.03, radius=3.0)
        hostn = {n: np.asarray(v) for n, v in host.items()}
        TE.assert_equal(m.track(pdx, pdy, lam=0.03, radius=3.0), hostn, "second call")
        # priors and outputs as HIP tensors, on a side stream
        dev = torch.device("cuda", m._device)
        stream = torch.cuda.Stream(device=dev)
        tdx, tdy = torch.from_numpy(pdx).to(dev), torch.from_numpy(pdy).to(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            out = m.track(tdx, tdy, lam=0.03, radius=3.0)
        stream.synchronize()
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in out.values())
        TE.assert_equal(out, hostn, "device arrays")
        with torch.cuda.stream(stream):
            out = m.track(tdx, 0.5, radius=3.0)                      # a scalar beside a tensor
        stream.synchronize()
        TE.assert_equal(out, {n: np.asarray(v) for n, v in m.track(pdx, 0.5, radius=3.0).items()}, "a scalar beside a tensor")
        with pytest.raises(ValueError, match="both numpy arrays"):
            m.track(tdx, pdy)
        # a staged stack is adopted as by basins(): once, and it stays the model's stack
        fresh = {n: np.asarray(v) for n, v in _model(hip_ns, kind, sam2, ref, c["Nw"], c["ms"], subpx=-1).track(pdx, pdy).items()}
        m.stage_sample(list(sam2))
        TE.assert_equal(m.track(pdx, pdy), fresh, "staged stack")
        assert not np.array_equal(fresh["cost"], hostn["cost"])
        TE.assert_equal(m.track(pdx, pdy), fresh, "after the staged stack")
        # the C ABI: df with the plain model is refused by name, and the model works afterwards
        if kind == 0:
            g = _lib.grid()
            N0, N1 = m.extent
            d = [np.zeros((N0, N1)) for _ in range(8)]
            q = [np.zeros((N0, N1), np.int32) for _ in range(3)]
            tail = [np.zeros((N0, N1)), np.zeros((N0, N1), np.int32), np.zeros((N0, N1), np.int32)]
            ptrs = [a.ctypes.data for a in d + q + tail]
            rc = g.track(m._handle, 0, 1, N0, 0, 1, N1, ptrs[0], ptrs[1], 0, 0.0, -1.0, *ptrs[2:], 0, None)
            assert rc < 0 and g.error() == "grid: track: a dark-field map (df) needs the dark-field model", (rc, g.error())
            ptrs[7] = None
            assert g.track(m._handle, 0, 1, N0, 0, 1, N1, ptrs[0], ptrs[1], 0, 0.0, -1.0, *ptrs[2:], _lib.F_USE_STAGED, None) == -1 \
                and "without a staged sample stack" in g.error()
            TE.assert_equal(m.track(pdx, pdy), fresh, "after two refusals")


def test_python_refusals_on_real_models_and_the_walk_afterwards(hip_ns):
    sam, ref, c = _hp_stack()
    kw = dict(window_size=c["Nw"], max_shift=c["ms"])
    mask = np.ones_like(sam)
    mask[:, 20:24, 30:40] = 0.0
    tail = r" \(grid search / cost volume\): "
    with pytest.raises(RuntimeError, match="track" + tail + "masked models are not supported"):
        hip_ns.UMPAModelDF(sam, ref, mask_list=mask, **kw).track(0.0, 0.0)
    with pytest.raises(RuntimeError, match="track" + tail + "frames at different positions"):
        hip_ns.UMPAModelNoDF(sam, ref, pos_list=[np.array(p) for p in ((0, 0), (2, 1), (1, 3))], **kw).track(0.0, 0.0)
    assert not hasattr(hip_ns.UMPAModelDFKernel(sam, ref, **kw), "track")
    m = hip_ns.UMPAModelDF(sam, ref, **kw)
    before = m.match(quiet=True)
    with pytest.raises(RuntimeError, match="track: .*grid"):
        m.track(0.0, 0.0, step=10)                                    # past the tiled path's limit: the library's refusal
    with pytest.raises(ValueError, match="track: lam must be None"):
        m.track(0.0, 0.0, lam=-1.0)
    with pytest.raises(ValueError, match="track: a prior must be a scalar or of shape"):
        m.track(np.zeros((3, 3)), 0.0)
    m.track(0.5, -0.5)
    m.track(0.5, -0.5, lam=0.1, radius=2.0)
    after = m.match(quiet=True)                                       # the consumer was cleared: the walk is what it was
    for n in before:
        np.testing.assert_array_equal(before[n], after[n], err_msg=n)


# ----------------------------------------------------------------------------- 7. use

def test_a_prior_recovers_the_true_shift_on_the_device(hip_ns):
    u = TE.use_case()
    use, known, sure = u["use"], u["known"], u["sure"]
    ty, tx = use["true"]
    assert known.sum() >= 20 and (sure & known).sum() >= 20
    m = _model(hip_ns, 0, u["sam"], u["ref"], use["Nw"], use["ms"], "sam", 0)   # sub-pixel mode 0: dx, dy are the integer shifts
    grid = m.match(quiet=True, search="grid")
    m.ROI = None
    np.testing.assert_array_equal(grid["dy"][known], ty)
    np.testing.assert_array_equal(grid["dx"][known], tx - use["period"])        # the alias, not the true shift
    near = m.track(float(tx), float(ty))
    np.testing.assert_array_equal(near["shift"][0][known], ty)
    np.testing.assert_array_equal(near["shift"][1][known], tx)
    np.testing.assert_array_equal(near["dy"][known], ty)
    np.testing.assert_array_equal(near["dx"][known], tx)
    assert (near["cost"] > near["cost0"])[known].all() and (near["err"][known] == 1).all()
    pen = m.track(float(tx), float(ty), lam=u["lam"])
    np.testing.assert_array_equal(pen["shift"][0][sure], ty)
    np.testing.assert_array_equal(pen["shift"][1][sure], tx)
    assert (pen["cost"] > pen["cost0"])[sure & known].all()
    print("use: penalty mode returns the true shift at %.1f %% of all pixels, the grid search at %.1f %%" % (
        100 * ((pen["shift"][0] == ty) & (pen["shift"][1] == tx)).mean(), 100 * ((grid["dy"] == ty) & (grid["dx"] == tx)).mean()))


def test_tracker_follows_the_true_shift_through_the_aliased_step(hip_ns):
    import torch
    from umpa_amd import Tracker
    u = TE.use_case()
    use, known = u["use"], u["known"]
    ty, tx = use["true"]
    m = _model(hip_ns, 0, u["sam0"], u["ref"], use["Nw"], use["ms"], "sam", 0)
    t = Tracker(m)
    r0 = t.step(list(u["sam0"]))                                      # the noise-free sample: the grid search finds the true shift everywhere
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r0.values())
    assert (r0["dy"] == ty).all() and (r0["dx"] == tx).all() and (r0["err"] == 1).all() and (r0["cost"] == r0["cost0"]).all()
    assert all(isinstance(p, torch.Tensor) and p.is_cuda for p in t.prior)
    r1 = t.step(list(u["sam"]))                                       # the aliased stack, tracked from step 0
    dy, dx = r1["dy"].cpu().numpy(), r1["dx"].cpu().numpy()
    np.testing.assert_array_equal(dy[known], ty)
    np.testing.assert_array_equal(dx[known], tx)
    t.reset()
    r2 = t.step(list(u["sam"]))                                       # without the prior: the alias
    np.testing.assert_array_equal(r2["dy"].cpu().numpy()[known], ty)
    np.testing.assert_array_equal(r2["dx"].cpu().numpy()[known], tx - use["period"])
    grid = m.match(quiet=True, search="grid")                         # the staged stack stayed the model's: the same answer
    np.testing.assert_array_equal(r2["dx"].cpu().numpy(), grid["dx"])
    np.testing.assert_array_equal(r2["dy"].cpu().numpy(), grid["dy"])
