"""
model.basins() / umpa_grid_basins on the GPU (libumpa_grid.so).  In every case each output EQUALS the restatement of
tests/basins_expect.py applied to the device's own cost_volume(with_fit=True) of the same model and region -- count, shift,
cost, err, T, df, and dx, dy, f bit for bit (the 4x4 fit of the sub-pixel modes -1 and 1 is the device's own entry point
for one array), empty slots included -- and rank 0 equals match(search='grid') map for map.

REACHES names, per test, the kernels of libumpa_grid.so it is there for (tests/test_basins_cpu.py checks on the CPU that
every grid_basins_kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import ctypes
import functools

import numpy as np
import pytest

import basins_expect as BE
import grid_expect as GE

pytestmark = pytest.mark.gpu

KTEMPL = 24                      # UMPA_KTEMPL: frame counts with their own instantiation (dark-field model)
REACHES = {
    "tests/test_hip_basins.py::test_every_frame_count": ["grid_basins_kernel<1, %d>" % (n if n <= KTEMPL else 0) for n in range(1, KTEMPL + 2)],
    "tests/test_hip_basins.py::test_every_k": ["grid_basins_kernel<0, 0>"],
}


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


def _rank0_is_the_grid_search(m, b, what="", **region):
    from umpa_amd import basins as B
    grid = m.match(quiet=True, search="grid", **region)
    m.ROI = None
    first = B.select(b, 0)                                            # an empty slot reads as the grid search's "no finite cost": err 0, zeros
    for n in ("dx", "dy", "f", "T", "err") + (("df",) if "df" in b else ()):
        np.testing.assert_array_equal(first[n], grid[n], err_msg="%s rank 0 against search='grid': %s" % (what, n))


def _check(m, k=8, what="", **region):
    """basins(k) of the region against the restatement on the device's own volume, and rank 0 against the grid search"""
    vol = m.cost_volume(with_fit=True, **region)
    b = m.basins(k=k, **region)
    sub = m.sub_pixel_mode
    want = BE.restate(vol["cost"], vol["T"], vol.get("df"), k, sub, fit=BE.device_fit(sub, m._device) if sub else None)
    BE.assert_equal(b, want, what)
    _rank0_is_the_grid_search(m, b, what, **region)
    return b, vol


# ----------------------------------------------------------------------------- 1. every instantiation, every k

@pytest.mark.parametrize("K", list(range(1, KTEMPL + 2)))
def test_every_frame_count(hip_ns, K):
    from umpa_amd.synth import make_stack
    Nw, ms = 2, 3
    sam, ref, _ = make_stack(44, 80, K, ms, df=True, seed=100 + K)
    for assign in ("sam", "ref"):
        for kind in (1, 0):
            m = _model(hip_ns, kind, sam, ref, Nw, ms, assign)
            (b, _), seen = _launches(m, lambda: _check(m, 4, "K %d %s kind %d" % (K, assign, kind)))
            assert seen.get("table_consumer") == 3 and "replay_walk" not in seen, seen
            assert (b["count"] >= 1).all()


@functools.lru_cache(maxsize=None)
def _hp_stack():
    return GE.stack("64x72x3")


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
@pytest.mark.parametrize("subpx", [-1, 0, 1])
def test_every_k(hip_ns, kind, subpx):
    sam, ref, c = _hp_stack()
    m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], "sam", subpx)
    b8, _ = _check(m, 8, "k 8 subpx %d" % subpx)
    assert (b8["count"] >= 2).mean() >= 0.70 and (b8["err"] == 1).any() and (b8["err"] == 0).any() and (b8["err"] == -1).any()
    for k in range(1, 8):
        b = m.basins(k=k)
        assert sorted(b) == sorted(b8)
        for n in b8:
            np.testing.assert_array_equal(b[n], b8[n] if n == "count" else b8[n][:k], err_msg="k %d %s" % (k, n))
    with pytest.raises(ValueError, match="k must be an integer from 1 to 8"):
        m.basins(k=9)


# ----------------------------------------------------------------------------- 2. search ranges

@pytest.mark.parametrize("ms,Nw,H,W", [(1, 2, 40, 80), (2, 2, 44, 84), (5, 3, 56, 96), (17, 2, 58, 108)], ids=["ms1", "ms2", "ms5", "ms17"])
def test_search_ranges(hip_ns, ms, Nw, H, W):
    """ms 1: a box of one shift (every finite pixel has exactly one basin, on the border); ms 2: every shift but the centre is
    on the border and no 4 x 4 neighbourhood fits; ms 17: the largest box the tiled path admits, 33 x 33 shifts -- the LDS
    ring of the kernel at its limit (50,688 bytes per wave), on the smallest frame that leaves 20 x 70 pixels (more than
    one block either way)."""
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(H, W, 3, 4, df=True, seed=300 + ms)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, "sam" if kind else "ref")
        b, _ = _check(m, 8, "ms %d kind %d" % (ms, kind))
        if ms == 1:
            assert (b["count"] == 1).all() and (b["err"][0] == 0).all() and (b["err"][1:] == -1).all()
        if ms == 2:
            assert (b["err"] != 1).all()                              # a box of 3 x 3 shifts holds no 4 x 4 neighbourhood
        if ms == 17:
            assert (b["count"] > 8).any() and (b["err"] == 1).any()


def test_wide_windows_through_the_marching_table(hip_ns):
    from umpa_amd.synth import make_stack
    K, Nw, ms = 20, 7, 8
    sam, ref, _ = make_stack(2 * (Nw + ms) + 24, 2 * (Nw + ms) + 60, K, ms, df=True, seed=5, order=1)   # 24 x 60 pixels: two strips of corr_march
    for kind, assign in ((1, "sam"), (0, "ref")):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, assign)
        (b, _), seen = _launches(m, lambda: _check(m, 8, "march kind %d" % kind))
        assert seen.get("corr_march", 0) >= 1 and seen.get("table_consumer") == 3 and "corr_volume" not in seen and "replay_walk" not in seen, seen
        print("march kind %d: pixels with >= 2 basins %.1f %%" % (kind, 100 * (b["count"] >= 2).mean()))


# ----------------------------------------------------------------------------- 3. chunks, regions

def _chunk_stack():
    from umpa_amd.synth import make_stack
    # 128 x 512 output pixels, 81 planes of 512 doubles per row: a 16 MB table holds 32 rows -> four row chunks
    return make_stack(144, 528, 4, 5, df=True, seed=9, order=1)[:2]


def test_four_row_chunks_change_nothing(hip_ns, monkeypatch):
    sam, ref = _chunk_stack()
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = _model(hip_ns, 1, sam, ref, 3, 5, subpx=-1)
        res[mb], seen = _launches(m, lambda: m.basins(k=8))
        assert seen.get("table_consumer") == (4 if mb else 1), (mb, seen)
    BE.assert_equal(res["16"], res[None], "four chunks")
    _rank0_is_the_grid_search(m, res["16"], "four chunks")


def test_roi_and_steps_are_slices_of_the_full_result(hip_ns):
    sam, ref = _chunk_stack()
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, 3, 5, subpx=-1)
        roi_before = m.ROI
        full = m.basins(k=5)
        cut = lambda s0, s1: {n: np.ascontiguousarray(v[..., s0, s1]) for n, v in full.items()}
        for step in (2, 3):
            BE.assert_equal(m.basins(k=5, step=step), cut(slice(None, None, step), slice(None, None, step)), "step %d" % step)
        BE.assert_equal(m.basins(k=5, ROI=((17, 90, 2), (5, 400, 3))), cut(slice(17, 90, 2), slice(5, 400, 3)), "ROI")
        assert m.ROI == roi_before                                    # the model's own ROI is left alone


# ----------------------------------------------------------------------------- 4. special pixels, ties

@pytest.mark.parametrize("march", [False, True], ids=["corr_volume", "corr_march"])
@pytest.mark.parametrize("bad", ["nan", "+inf", "zero"])
def test_special_pixels_on_the_seams(hip_ns, bad, march):
    """NaN, Inf and 0 pixels placed as tests/regimes.py places them: interior, on a tile seam (output row 32) and a strip seam
    (output column 48 / 32), in the padding border, in the last frame.  The footprint -- pixels without any basin, basins
    beside NaN cells -- must be the restatement's on the dirty volume."""
    import regimes
    from umpa_amd.synth import make_stack
    cfg = dict(Nw=6, K=3, ms=3, H=66, W=92) if march else dict(Nw=2, K=3, ms=3, H=60, W=70)
    sam, ref, _ = make_stack(cfg["H"], cfg["W"], cfg["K"], cfg["ms"], df=True, seed=77)
    pos = regimes.bad_positions(cfg)
    # the bad pixel sits in the stack whose window MOVES with the shift, so that a box can hold NaN and finite costs side by side
    for kind, where, assign in ((1, "ref", "sam"), (0, "sam", "ref")):
        s, r = regimes.bad_pixels(sam, ref, bad, where, pos)
        m = _model(hip_ns, kind, s, r, cfg["Nw"], cfg["ms"], assign)
        (b, vol), seen = _launches(m, lambda: _check(m, 4, "%s in %s" % (bad, where)))
        assert seen.get("corr_march" if march else "corr_volume", 0) >= 1, seen
        far = regimes.far_from(cfg, pos, b["count"].shape)
        assert (~far).any() and far.any()
        if bad != "zero":
            U = 2 * cfg["ms"] - 1
            with np.errstate(invalid="ignore"):
                holes = ~(vol["cost"] < np.inf).reshape(U * U, -1)
            assert (b["count"] == 0).any() and not (b["count"][far] == 0).any()
            beside = (b["count"].ravel() > 0) & holes.any(axis=0)    # pixels that have basins and NaN cells in one box
            assert beside.any()


def test_plateaus_and_equal_basins(hip_ns):
    """A stack that is constant along the columns: the cost does not depend on sj, every cost row is a plateau and only its
    earliest member can be a basin.  A reference of column period 4 (integer values, so that the sums are exact in any
    order) under ms = 4: the costs of shifts 4 columns apart are equal, non-adjacent basins of equal cost are ranked by
    scan order."""
    rng = np.random.default_rng(41)
    K, H, W, Nw, ms = 3, 48, 76, 2, 4
    col = rng.integers(1, 64, (K, H, 1)).astype(np.float64)
    flat_sam, flat_ref = np.repeat(col, W, axis=2), np.repeat(np.roll(col, 1, axis=1) + 3.0, W, axis=2)
    for kind in (0, 1):
        m = _model(hip_ns, kind, np.ascontiguousarray(flat_sam), np.ascontiguousarray(flat_ref), Nw, ms)
        b, vol = _check(m, 8, "column-constant kind %d" % kind)
        np.testing.assert_array_equal(vol["cost"], np.repeat(vol["cost"][:, :1], 2 * ms - 1, axis=1))   # the plateaus are exact
        kept = b["err"] >= 0
        assert kept.any() and (b["shift"][:, 1][kept] == 1 - ms).all()
    tile = rng.integers(1, 64, (K, H, 4)).astype(np.float64)
    per_ref = np.ascontiguousarray(np.tile(tile, (1, 1, W // 4)))
    sam = np.ascontiguousarray(np.roll(per_ref, (-1, -1), axis=(1, 2)) + rng.integers(0, 3, per_ref.shape))
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, per_ref, Nw, ms, "sam")
        b, vol = _check(m, 8, "period 4 kind %d" % kind)
        pair = (b["err"][0] >= 0) & (b["err"][1] >= 0) & (b["cost"][0] == b["cost"][1])
        print("period 4 kind %d: %.1f %% of the pixels have two best basins of equal cost" % (kind, 100 * pair.mean()))
        assert pair.mean() > 0.5
        d = b["shift"][1] - b["shift"][0]
        assert ((d[0][pair] == 0) & (d[1][pair] == 4)).all()          # the same row shift, 4 columns on: scan order


# ----------------------------------------------------------------------------- 5. repeats and I/O sides

def test_repeats_device_arrays_and_a_staged_stack(hip_ns):
    import torch
    from umpa_amd import _lib
    sam, ref, c = _hp_stack()
    sam2 = np.ascontiguousarray(1.25 * sam[::-1])
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        host = m.basins(k=6)
        BE.assert_equal(m.basins(k=6), host, "second call")
        # HIP tensors as outputs, on a side stream, the way smooth.py drives _grid_cost_volume
        dev = torch.device("cuda", m._device)
        stream = torch.cuda.Stream(device=dev)

        def alloc(k, N0, N1):
            out = {n: torch.full((k, N0, N1), -7.0, dtype=torch.float64, device=dev) for n in ("f", "T", "dx", "dy", "cost") + (("df",) if kind else ())}
            out.update({n: torch.full((k, N0, N1), -7, dtype=torch.int32, device=dev) for n in ("si", "sj", "err")})
            out["count"] = torch.full((N0, N1), -7, dtype=torch.int32, device=dev)
            return out
        with torch.cuda.stream(stream):
            out = m._grid_basins(6, None, None, alloc)[2]
        stream.synchronize()
        got = {n: t.cpu().numpy() for n, t in out.items()}
        got["shift"] = np.stack([got.pop("si"), got.pop("sj")], axis=1)
        BE.assert_equal(got, host, "device arrays")
        # a staged stack is adopted as by cost_volume(): once, and it stays the model's stack
        fresh = _model(hip_ns, kind, sam2, ref, c["Nw"], c["ms"], subpx=-1).basins(k=6)
        m.stage_sample(list(sam2))
        BE.assert_equal(m.basins(k=6), fresh, "staged stack")
        assert not np.array_equal(fresh["cost"], host["cost"])
        BE.assert_equal(m.basins(k=6), fresh, "after the staged stack")
        # the C ABI: df with the plain model is refused by name, and the model works afterwards
        if kind == 0:
            g = _lib.grid()
            N0, N1 = m.extent
            d = [np.zeros((1, N0, N1)) for _ in range(6)]
            q = [np.zeros((1, N0, N1), np.int32) for _ in range(3)] + [np.zeros((N0, N1), np.int32)]
            rc = g.basins(m._handle, 0, 1, N0, 0, 1, N1, 1, *[a.ctypes.data for a in d + q], 0, None)
            assert rc < 0 and g.error() == "grid: basins: a dark-field map (df) needs the dark-field model", (rc, g.error())
            assert g.basins(m._handle, 0, 1, N0, 0, 1, N1, 1, *[a.ctypes.data if n != 5 else None for n, a in enumerate(d + q)],
                            _lib.F_USE_STAGED, None) == -1 and "without a staged sample stack" in g.error()
            BE.assert_equal(m.basins(k=6), fresh, "after two refusals")


def test_python_refusals_on_real_models(hip_ns):
    sam, ref, c = _hp_stack()
    kw = dict(window_size=c["Nw"], max_shift=c["ms"])
    mask = np.ones_like(sam)
    mask[:, 20:24, 30:40] = 0.0
    tail = r" \(grid search / cost volume\): "
    with pytest.raises(RuntimeError, match="basins" + tail + "masked models are not supported"):
        hip_ns.UMPAModelDF(sam, ref, mask_list=mask, **kw).basins()
    with pytest.raises(RuntimeError, match="basins" + tail + "frames at different positions"):
        hip_ns.UMPAModelNoDF(sam, ref, pos_list=[np.array(p) for p in ((0, 0), (2, 1), (1, 3))], **kw).basins()
    assert not hasattr(hip_ns.UMPAModelDFKernel(sam, ref, **kw), "basins")
    m = hip_ns.UMPAModelDF(sam, ref, **kw)
    before = m.match(quiet=True)
    with pytest.raises(RuntimeError, match="basins: .*grid"):
        m.basins(step=10)                                             # past the tiled path's limit: the library's refusal
    for k in (0, 9):
        with pytest.raises(ValueError):
            m.basins(k=k)
    m.basins()
    after = m.match(quiet=True)                                       # the consumer was cleared: the walk is what it was
    for n in before:
        np.testing.assert_array_equal(before[n], after[n], err_msg=n)


# ----------------------------------------------------------------------------- 6. use

USE = dict(H=52, W=64, K=3, Nw=2, ms=4, seed=4242, true=(1, 1), period=4, noise=0.02, aperiodic=0.01)


@functools.lru_cache(maxsize=None)
def _use_case():
    """A stack whose true shift, (1, 1), is not the global minimum at a known set of pixels: the reference is a pattern of
    column period 4 plus a weak aperiodic part, the sample is the reference displaced by the true shift plus noise, so the
    alias (1, -3) competes and wins wherever the noise favours it.  The known set is decided on the CPU, from the
    extended-precision volume: pixels where both shifts are basins and the alias lies below the true shift by more than
    the fp64 bounds of the two costs."""
    u = USE
    rng = np.random.default_rng(u["seed"])
    K, H, W, ms, Nw = u["K"], u["H"], u["W"], u["ms"], u["Nw"]
    ty, tx = u["true"]
    ref = 1.0 + 0.5 * np.tile(rng.random((K, H + 2 * ms, u["period"])), (1, 1, (W + 2 * ms) // u["period"] + 1))[:, :, :W + 2 * ms]
    ref = ref + u["aperiodic"] * rng.random(ref.shape)
    sam = ref[:, ms + ty:ms + ty + H, ms + tx:ms + tx + W] + u["noise"] * rng.standard_normal((K, H, W))
    ref = np.ascontiguousarray(ref[:, ms:ms + H, ms:ms + W])
    sam = np.ascontiguousarray(sam)
    v = GE.hp_volumes(0, sam, ref, GE.window(Nw), ms, ms + Nw, "sam")
    cost = np.asarray(v["cost"], dtype=np.float64)
    basin = BE.is_basin(cost)
    at = lambda a, si, sj: a[si + ms - 1, sj + ms - 1]
    gap = at(v["cost"], ty, tx) - at(v["cost"], ty, tx - u["period"])
    known = at(basin, ty, tx) & at(basin, ty, tx - u["period"]) & (gap > at(v["bound"], ty, tx) + at(v["bound"], ty, tx - u["period"]))
    known &= np.argmin(cost.reshape((2 * ms - 1) ** 2, *known.shape), axis=0) == (ty + ms - 1) * (2 * ms - 1) + (tx - u["period"] + ms - 1)
    return sam, ref, np.asarray(known, dtype=bool)


def test_a_prior_recovers_the_true_shift_where_the_grid_search_does_not(hip_ns):
    from umpa_amd import basins as B
    u = USE
    ty, tx = u["true"]
    sam, ref, known = _use_case()
    print("use: %d of %d pixels have the alias as their global minimum" % (known.sum(), known.size))
    assert known.sum() >= 20 and (~known).sum() >= 20
    m = _model(hip_ns, 0, sam, ref, u["Nw"], u["ms"], "sam", 0)      # sub-pixel mode 0: dx, dy are the integer shifts
    grid = m.match(quiet=True, search="grid")
    m.ROI = None
    np.testing.assert_array_equal(grid["dy"][known], ty)
    np.testing.assert_array_equal(grid["dx"][known], tx - u["period"])   # the alias, not the true shift
    b = m.basins(k=4)
    idx = B.nearest(b, float(tx), float(ty))                          # the prior: e.g. the previous projection of a step scan
    sel = B.select(b, idx)
    assert (idx[known] > 0).all()
    np.testing.assert_array_equal(sel["shift"][0][known], ty)
    np.testing.assert_array_equal(sel["shift"][1][known], tx)
    assert (B.ambiguity(b)[known] > 0).all()
    walk = m.match(quiet=True, dxdy=B.start_shifts(b, idx))
    # the walk ends in that basin: every cell of the 5x5 around the true shift is a mismatch of one or two pixels against a
    # pattern of period 4, far above it, so the walk neither moves nor restarts (the CPU oracle's walk agrees: all of them)
    np.testing.assert_array_equal(walk["err"][known], 1)
    np.testing.assert_array_equal(walk["dy"][known], ty)
    np.testing.assert_array_equal(walk["dx"][known], tx)
    plain = m.match(quiet=True)
    print("use: the walk from (0, 0) ends on the true shift at %.0f %% of those pixels" % (100 * ((plain["dy"] == ty) & (plain["dx"] == tx))[known].mean()))
