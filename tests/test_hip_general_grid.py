"""
The grid consumers on the general table (model.general_grid, umpa_grid_set_general; libumpa_grid.so's general_table_kernel), on
the GPU: the table against the model's own cost() bit for bit and against extended precision (tests/general_expect.py) on a
sample-stepping stack of unequal shapes, every consumer EQUAL to its numpy restatement on the device's own volume, the grid
against the walk, a model forced onto the direct kernel, the edges of window, search range, frame count and wave, steps and the
global-memory fallback, row chunks, repeats, device arrays, a NaN pixel, the front ends, and the switch's life.

REACHES names, per test, the kernels of libumpa_grid.so it is there for (tests/test_general_grid_cpu.py checks on the CPU that
every general_table_kernel instantiation of the built library is claimed here, and that no claim is stale).
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity

import basins_expect as BE
import consumer_expect as CE
import general_expect as G
import grid_expect as GE
import sequence_expect as SE
import track_expect as TE

pytestmark = pytest.mark.gpu

T = "tests/test_hip_general_grid.py::"
GT = ["general_table_kernel<0, false>", "general_table_kernel<0, true>", "general_table_kernel<1, false>", "general_table_kernel<1, true>"]
REACHES = {
    T + "test_table_equals_model_cost": GT + ["masked_volume_kernel<0>", "masked_volume_kernel<1>"],
    T + "test_consumers_equal_their_restatements": GT + [
        "masked_min_kernel<0>", "masked_min_kernel<1>", "masked_basins_kernel<0>", "masked_basins_kernel<1>",
        "masked_track_kernel<0>", "masked_track_kernel<1>", "masked_sequence_kernel<0>", "masked_sequence_kernel<1>"],
    T + "test_edges_steps_and_the_fallback": GT,
}
POS = "frames at different positions (pos_list) or of different shapes are not supported"
FINISHED = "a finished cost is not linear in the windowed sums"
GENERAL_PATH = 5


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _build(hip_ns, sam, ref, pos, Nw, ms, kind, assign="sam", masks=None, subpx=-1, on=True):
    kw = dict(window_size=Nw, max_shift=ms)
    if pos is not None:
        kw["pos_list"] = [np.array(p) for p in pos]
    if masks is not None:
        kw["mask_list"] = list(masks)
    m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(list(sam), list(ref), **kw)
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    if on:
        m.general_grid = True
    return m


def _D(hip_ns, kind, assign, masked, subpx=-1, on=True):
    sam, ref, pos, Nw, ms = G.D()
    return _build(hip_ns, sam, ref, pos, Nw, ms, kind, assign, G.D_masks() if masked else None, subpx, on)


def _path(m):
    return m._lib.last_path(m._handle)


def _bare(d):
    return {n: v for n, v in d.items() if n != "covered"}


def _np(d):
    return {n: np.asarray(a) for n, a in d.items() if not n.startswith("_")}


def _same(a, b, what=""):
    assert sorted(a) == sorted(b), what
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg="%s %s" % (what, k))


def _fit(m):
    return BE.device_fit(m.sub_pixel_mode, m._device) if m.sub_pixel_mode else None


def _prior(ms, shape, seed):
    rng = np.random.default_rng(seed)
    pdx, pdy = (ms - 1) * (2 * rng.random(shape) - 1), (ms - 1) * (2 * rng.random(shape) - 1)
    pdx[rng.random(shape) < 0.05] = np.nan                               # NaN priors: the data term decides
    pdy[rng.random(shape) < 0.05] = np.nan
    return pdx, pdy


# ----------------------------------------------------------------------------- 1. the table against model.cost

@pytest.mark.parametrize("kind,assign,masked", G.D_CASES, ids=G.D_IDS)
def test_table_equals_model_cost(hip_ns, kind, assign, masked):
    """cost_volume(with_fit=True) on D equals model.cost(i, j, sx, sy) of the same model bit for bit in cost, T and df, at every
    shift of the pixel sample (the corners of every frame-set cell, the workgroup seams); every entry lies within the a-priori
    fp64 bound of the extended-precision helper; the 36 pixels no frame contributes to are NaN; `covered` is the coverage
    rule."""
    m = _D(hip_ns, kind, assign, masked)
    ms, pad = m.max_shift, m.padding
    vol = m.cost_volume(with_fit=True)
    assert _path(m) == GENERAL_PATH
    assert sorted(vol) == sorted(["cost", "T", "covered"] + (["df"] if kind else []))
    v = G.D_hp(kind, assign, masked)
    assert vol["cost"].shape == v["cost"].shape == (2 * ms - 1, 2 * ms - 1, 62, 72)
    np.testing.assert_array_equal(vol["covered"], G.D_covered(masked))
    dead = v["sets"] == 0
    assert dead.sum() == G.D_DEAD and np.isnan(vol["cost"][:, :, dead]).all()
    xi, xj = G.D_sample()
    keys = ("cost", "T") + (("df",) if kind else ())
    for a, b in zip(xi, xj):
        want = np.array([[m.cost(int(a) + pad, int(b) + pad, float(si), float(sj)) for sj in range(1 - ms, ms)] for si in range(1 - ms, ms)])
        for q, k in enumerate(keys):
            np.testing.assert_array_equal(vol[k][:, :, a, b], want[:, :, q], err_msg="%s at pixel (%d, %d)" % (k, a, b))
    worst = G.within_bound(vol["cost"], v, "D")
    fin = np.isfinite(v["cost"].astype(np.float64))
    rT = np.abs(vol["T"][fin] - v["T"][fin]) / np.abs(v["T"][fin])
    print("D kind %d %s masked %d: max |gpu - hp| / bound %.4f, T rel %.2e" % (kind, assign, masked, worst, rT.max()))
    assert np.all(rT <= CE.RTOL)
    if kind:
        rdf = np.abs(vol["df"][fin] - v["df"][fin]) / np.abs(v["df"][fin])
        assert np.all(rdf <= CE.RTOL)


# ----------------------------------------------------------------------------- 2. the consumers EQUAL their restatements

@pytest.mark.parametrize("kind,assign,masked", [(0, "sam", True), (0, "ref", False), (1, "sam", False), (1, "ref", True)],
                         ids=["NoDF-sam-mask", "NoDF-ref-plain", "DF-sam-plain", "DF-ref-mask"])
def test_consumers_equal_their_restatements(hip_ns, kind, assign, masked):
    """match(search='grid') in the three sub-pixel modes, basins(k), track in both modes and with a radius and sequence over
    two steps equal the restatements fed the device's own volume; the pixels under the coverage threshold are untouched by the
    grid match."""
    cov = G.D_covered(masked)
    for subpx in (-1, 0, 1):
        m = _D(hip_ns, kind, assign, masked, subpx)
        vol = m.cost_volume(with_fit=True)
        args = (vol["cost"], vol["T"], vol.get("df"))
        np.testing.assert_array_equal(vol["covered"], cov)
        for k in (1, 4):
            b = m.basins(k=k)
            BE.assert_equal(_bare(b), BE.restate(*args, k, subpx, fit=_fit(m)), "basins k %d subpx %d" % (k, subpx))
            np.testing.assert_array_equal(b["covered"], cov)
        g = m.match(quiet=True, search="grid")
        assert _path(m) == GENERAL_PATH
        for n in ("dx", "dy", "f", "T") + (("df",) if kind else ()):
            np.testing.assert_array_equal(g[n][cov], b[n][0][cov], err_msg=n)
            assert not np.asarray(g[n])[~cov].any(), n
        np.testing.assert_array_equal(g["err"][cov], np.maximum(b["err"][0], 0)[cov])
        assert not g["err"][~cov].any()
        if subpx == 1:
            continue                                                  # (track and sequence: two of the three modes)
        pdx, pdy = _prior(m.max_shift, m.sh, 31)
        for lam, radius in ((None, None), (None, 2.5), (0.02, None), (0.02, 3.0)):
            t = m.track(pdx, pdy, lam=lam, radius=radius)
            want = TE.restate(*args, pdy, pdx, TE.NEAREST if lam is None else TE.PENALTY, 0.0 if lam is None else lam, radius, subpx, fit=_fit(m))
            TE.assert_equal(_bare(t), want, "track lam %r radius %r" % (lam, radius))
            np.testing.assert_array_equal(t["covered"], cov)
        s0 = m.sequence(lam=0.3)
        SE.assert_equal(_bare(s0), SE.restate(*args, None, 0.3, None, subpx, fit=_fit(m)), "sequence, no state")
        scale = float(np.median(vol["cost"][np.isfinite(vol["cost"])]))
        s1 = m.sequence(state=s0["state"], lam=0.05 * scale, trunc=0.5 * scale)
        SE.assert_equal(_bare(s1), SE.restate(*args, s0["state"], 0.05 * scale, 0.5 * scale, subpx, fit=_fit(m)), "sequence, step 1")
        s2 = m.sequence(state=s1["state"], lam=0.05 * scale)
        SE.assert_equal(_bare(s2), SE.restate(*args, s1["state"], 0.05 * scale, None, subpx, fit=_fit(m)), "sequence, step 2")
        np.testing.assert_array_equal(s2["covered"], cov)


# ----------------------------------------------------------------------------- 3. the grid against the walk

@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_grid_against_the_walk(hip_ns, kind):
    """A twin forced onto the direct kernel runs match() (the walk).  Where walk and grid end on the same integer minimum with
    err = 1, dx, dy and f are bit-identical; the grid's minimum is never above a cost the walk has seen; and on those pixels
    the grid's dx, dy and f pass the suite's parity bar against D_stepping's recorded results (variant 0: DF, 1: NoDF).  T and
    df are not compared with a walk's: a walk returns the fit of its LAST evaluation, the grid search that of the integer
    minimum (include/umpa_grid.h) -- on D they differ on a tenth of the agreeing pixels, by up to 40 %, as
    tests/test_hip_grid.py's walk-against-grid tests, which compare dx, dy and f alone, already allow; the grid's T and df are
    held to the volume's entry at the minimum by test_consumers_equal_their_restatements."""
    from conftest import Case
    from oracle import hp_cost
    from umpa_amd import _lib
    out = {}
    for subpx in (0, -1):
        g = _D(hip_ns, kind, "sam", False, subpx)
        w = _D(hip_ns, kind, "sam", False, subpx, on=False)
        w._force = _lib.F_FORCE_DIRECT
        g.debug = w.debug = True
        out[subpx] = (_np(g.match(quiet=True, search="grid")), _np(w.match(quiet=True)))
    g0, w0 = out[0]
    g1, w1 = out[-1]
    agree = (g0["dx"] == w0["dx"]) & (g0["dy"] == w0["dy"]) & (g0["err"] == 1) & (w0["err"] == 1)
    assert agree.mean() > 0.7, agree.mean()
    for n in ("dx", "dy", "f"):
        np.testing.assert_array_equal(g1[n][agree], w1[n][agree], err_msg=n)
    (xi, xj, q), _, _ = hp_cost.memo_cells(w0, 6)
    gmin = g0["debug_d"][..., 12]                                        # the cost of the grid's integer minimum
    ok = g0["debug_Ncalls"][xi, xj] > 0                                  # (pixels the grid match did not skip)
    assert ok.all() and np.all(gmin[xi, xj] <= w0["debug_d"][xi, xj, q])
    want = Case("D_stepping").expected(0 if kind else 1)
    keys = ["err", "dx", "dy", "f", "T"] + (["df"] if kind else [])
    mine = {k: np.array(g1[k]) for k in keys}
    gold = {k: np.asarray(want[k]) for k in keys}
    for k in keys:
        mine[k][~agree] = gold[k][~agree]
    for k in keys[4:]:                                                # T, df: a walk's are its LAST evaluation's, the grid's the minimum's
        mine[k] = gold[k].copy()
    mine["debug_a"], mine["debug_d"] = g1["debug_a"], g1["debug_d"]   # (for the bar's own classification of ill-posed Newton pixels)
    st = assert_parity(mine, gold, 4, "general grid D_stepping %s" % ("DF" if kind else "NoDF"))
    print("D kind %d: walk and grid agree on %d of %d pixels, parity ok %d" % (kind, agree.sum(), agree.size, st["ok"]))


# ----------------------------------------------------------------------------- 4. P: forced direct

@pytest.mark.parametrize("kind,assign", G.MODES, ids=["%s-%s" % ("DF" if k else "NoDF", a) for k, a in G.MODES])
def test_forced_direct_model(hip_ns, kind, assign):
    from umpa_amd import _lib
    sam, ref, c = GE.stack(G.P_NAME)
    Nw, ms = c["Nw"], c["ms"]
    f = _build(hip_ns, sam, ref, None, Nw, ms, kind, assign)
    f._force = _lib.F_FORCE_DIRECT
    vol = f.cost_volume(with_fit=True)
    assert _path(f) == GENERAL_PATH and "covered" not in vol            # (coverage is trivial)
    v = GE.hp_volumes(kind, sam, ref, GE.window(Nw), ms, Nw + ms, assign)
    worst = G.within_bound(vol["cost"], v, "P")
    near = GE.near_tie(v["cost"], v["bound"])
    assert near.mean() <= GE.NEAR_TIE_CAP
    plain = _build(hip_ns, sam, ref, None, Nw, ms, kind, assign, on=False)
    off = _np(plain.cost_volume(with_fit=True))
    goff = _np(plain.match(quiet=True, search="grid"))
    ci, cj, _, found = CE.first_strict_minimum(vol["cost"])
    ti, tj, _, _ = CE.first_strict_minimum(off["cost"])
    assert found.all()
    np.testing.assert_array_equal(ci[~near], ti[~near])
    np.testing.assert_array_equal(cj[~near], tj[~near])
    print("P kind %d %s: max |gpu - hp| / bound %.4f, near-tie %d" % (kind, assign, worst, near.sum()))
    # with the switch on, the unforced model still goes tiled: bit for bit what it returned with the switch off
    plain.general_grid = True
    _same(_np(plain.cost_volume(with_fit=True)), off, "the tiled volume with the switch on")
    assert _path(plain) == 2
    _same(_np(plain.match(quiet=True, search="grid")), goff, "the tiled grid search with the switch on")
    # the forced model's grid search takes the general way too, and agrees with its own volume
    g = f.match(quiet=True, search="grid")
    assert _path(f) == GENERAL_PATH
    b = f.basins(k=1)
    for n in ("dx", "dy", "f", "T") + (("df",) if kind else ()):
        np.testing.assert_array_equal(g[n], b[n][0], err_msg=n)


# ----------------------------------------------------------------------------- 5. edges, steps, the fallback

@pytest.mark.parametrize("Nw,ms,Na,N1,kind,assign,masked", G.EDGE_CASES, ids=G.EDGE_IDS)
def test_edges_steps_and_the_fallback(hip_ns, Nw, ms, Na, N1, kind, assign, masked):
    """Window half-widths 1 and 8, search ranges 2 and 8, 1 and 26 frames, 64, 65 and 70 columns, 21 rows: the volume within
    the bound of extended precision; a (2, 3) step with an offset ROI, and a step of (5, 5) whose footprint does not fit LDS
    (the global-memory fallback: general_geometry), equal the same pixels of the unit-step result bit for bit."""
    sam, ref, pos, masks = G.edge_inputs(Nw, ms, Na, N1)
    m = _build(hip_ns, sam, ref, pos if Na > 1 else None, Nw, ms, kind, assign, masks if masked else None)
    if Na == 1 and not masked:
        from umpa_amd import _lib
        m._force = _lib.F_FORCE_DIRECT                                # (one frame at (0, 0) without masks: only force sends it here)
    assert m.extent == (G.EDGE_ROWS, N1)
    full = _np(m.cost_volume(with_fit=True))
    assert _path(m) == GENERAL_PATH
    worst = G.within_bound(full["cost"], G.edge_hp(Nw, ms, Na, N1, kind, assign, masked), "edge")
    print("edge Nw %d ms %d Na %d w %d: max |gpu - hp| / bound %.4f" % (Nw, ms, Na, N1, worst))
    b = _np(m.basins(k=2))
    for roi in (((3, G.EDGE_ROWS, 2), (5, N1, 3)), ((0, G.EDGE_ROWS, 5), (1, N1, 5))):
        s0, s1 = slice(*roi[0]), slice(*roi[1])
        part = _np(m.cost_volume(with_fit=True, ROI=roi))
        assert _path(m) == GENERAL_PATH
        _same(part, {n: np.ascontiguousarray(a[..., s0, s1]) for n, a in full.items()}, "ROI %r" % (roi,))
        _same(_np(m.basins(k=2, ROI=roi)), {n: np.ascontiguousarray(a[..., s0, s1]) for n, a in b.items()}, "basins, ROI %r" % (roi,))


# ----------------------------------------------------------------------------- 6. invariance

def _chunk_model(hip_ns, kind=1, sam=None):
    """53 x 65 output pixels, max_shift 8, dark-field: a row of the table is 225 x 3 x 65 doubles = 351 kB, so the smallest
    table budget (16 MiB) holds 47 rows -- 32 after rounding to the workgroup's 16 -- and a call takes two row chunks"""
    from umpa_amd.synth import make_stack
    Nw, ms = 1, 8
    pad = Nw + ms
    s, r, _ = make_stack(53 + 2 * pad - 3, 65 + 2 * pad - 5, 3, ms, df=True, seed=77, amplitude=3.0, order=1)
    pos = [(0, 0), (3, 5), (0, 5)]
    m = _build(hip_ns, s if sam is None else sam, r, pos, Nw, ms, kind)
    assert m.extent == (53, 65)
    return m, s, pos


def _five(m, pdx, pdy, state):
    out = {"grid": m.match(quiet=True, search="grid")}
    out["volume"] = m.cost_volume(with_fit=True)
    out["basins"] = m.basins(k=3)
    out["track"] = m.track(pdx, pdy, lam=0.02, radius=3.0)
    out["sequence"] = m.sequence(state=state, lam=0.01, trunc=0.5)
    return {k: _np(v) for k, v in out.items()}


def test_row_chunks_and_repeats_change_nothing(hip_ns, monkeypatch):
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m, _, _ = _chunk_model(hip_ns)
        pdx, pdy = _prior(8, (53, 65), 7)
        state = np.random.default_rng(8).random((15, 15, 53, 65))
        res[mb] = _five(m, pdx, pdy, state)
        again = _five(m, pdx, pdy, state)
        for k in again:
            _same(again[k], res[mb][k], "repeat %s (table budget %s)" % (k, mb))
    for k in res[None]:
        _same(res["16"][k], res[None][k], "row chunks " + k)


def test_device_arrays_on_a_side_stream(hip_ns):
    import torch
    m = _D(hip_ns, 1, "sam", True)
    N0, N1 = m.extent
    pdx, pdy = _prior(m.max_shift, (N0, N1), 3)
    host_vol = _np(m.cost_volume(with_fit=True))
    host_track = _np(m.track(pdx, pdy, lam=0.02, radius=3.0))
    dev = torch.device("cuda", m._device)
    stream = torch.cuda.Stream(device=dev)
    tdx, tdy = (torch.from_numpy(a).to(dev) for a in (pdx, pdy))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        vols = m._grid_cost_volume(None, None, lambda U, N0, N1: {k: torch.empty((U, U, N0, N1), dtype=torch.float64, device=dev)
                                                                  for k in ("cost", "T", "df")})[2]
        track = m.track(tdx, tdy, lam=0.02, radius=3.0)
    stream.synchronize()
    for k in ("cost", "T", "df"):
        np.testing.assert_array_equal(vols[k].cpu().numpy(), host_vol[k], err_msg="volume " + k)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for n, t in track.items() if n != "covered")
    TE.assert_equal(_bare(track), _bare(host_track), "track on device arrays")


@pytest.mark.parametrize("assign", ["sam", "ref"])
def test_a_nan_pixel_reaches_exactly_the_windows_that_hold_it(hip_ns, assign):
    """A NaN written into one sample frame makes exactly the entries NaN whose sample window, in a frame that contributes to
    the pixel, contains it, and leaves every other entry bit-identical."""
    sam, ref, pos, Nw, ms = G.D()
    k, r, c = 1, 30, 25                                               # frame 1, its pixel (30, 25): image pixel (30, 37)
    bad = [f.copy() for f in sam]
    bad[k][r, c] = np.nan
    clean = _np(_build(hip_ns, sam, ref, pos, Nw, ms, 0, assign).cost_volume(with_fit=True))
    got = _np(_build(hip_ns, bad, ref, pos, Nw, ms, 0, assign).cost_volume(with_fit=True))
    pad, U = Nw + ms, 2 * ms - 1
    contrib = G.contributes([f.shape for f in sam], pos, pad)[k]
    N0, N1 = contrib.shape
    xi, xj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    hit = np.zeros((U, U, N0, N1), dtype=bool)
    for a in range(U):
        for b in range(U):
            si, sj = (a - ms + 1, b - ms + 1) if assign == "ref" else (0, 0)     # the sample window moves in 'ref' mode only
            qi, qj = xi + pad - si - pos[k][0], xj + pad - sj - pos[k][1]         # its centre in frame k
            hit[a, b] = contrib & (np.abs(qi - r) <= Nw) & (np.abs(qj - c) <= Nw)
    assert hit.any()
    for n in ("cost", "T"):
        assert np.isnan(got[n][hit]).all(), n
        np.testing.assert_array_equal(got[n][~hit], clean[n][~hit], err_msg=n)


# ----------------------------------------------------------------------------- 7. the front ends

def test_front_ends_on_a_stepping_stack(hip_ns):
    """Tracker and Sequence run three staged steps on the 2 x 2 stepping stack E, match_smooth and basins.nearest run; a
    staged step is the call on a twin that was built with that sample stack."""
    from umpa_amd import basins as B, smooth
    from umpa_amd.sequence import Sequence
    from umpa_amd.track import Tracker
    p = G.E_PAR
    sam, ref, pos = G.E()
    stacks = [G.E(seed)[0] for seed in (1, 2, 3)]
    m = _build(hip_ns, sam, ref, pos, p["Nw"], p["ms"], 1)
    t, q = Tracker(m, lam=0.02), Sequence(m, 0.01)
    for step, s in enumerate(stacks):
        rt = t.step(list(s))
        assert _path(m) == GENERAL_PATH
        rq = q.step(list(s))
        twin = _build(hip_ns, s, ref, pos, p["Nw"], p["ms"], 1)
        if step == 0:
            g = twin.match(quiet=True, search="grid")
            cov = np.asarray(rt["covered"])
            for n in ("dx", "dy", "f", "T", "df"):
                np.testing.assert_array_equal(rt[n].cpu().numpy()[cov], g[n][cov], err_msg="Tracker step 0 " + n)
                np.testing.assert_array_equal(rq[n].cpu().numpy()[cov], g[n][cov], err_msg="Sequence step 0 " + n)
        np.testing.assert_array_equal(rt["cost0"].cpu().numpy(), twin.track(0.0, 0.0)["cost0"], err_msg="step %d" % step)
    got = smooth.match_smooth(m, lam=0.02, trunc=0.3)
    assert got["err"].shape == m.extent and got["err"].any()
    b = m.basins(k=4)
    idx = B.nearest(b, 0.0, 0.0)
    assert idx.shape == m.extent


# ----------------------------------------------------------------------------- 8. the switch's life

@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_switch_on_off_and_the_refusals_around_it(hip_ns, kind):
    from umpa_amd import _lib, levels, widen
    m = _D(hip_ns, kind, "sam", False, on=False)
    assert m.general_grid is False
    before = _np(m.match(quiet=True))
    calls = [("search='grid'", lambda: m.match(quiet=True, search="grid")), ("cost_volume", lambda: m.cost_volume()),
             ("basins", lambda: m.basins()), ("track", lambda: m.track(0.0, 0.0)), ("sequence", lambda: m.sequence(lam=0.0))]

    def refused():
        for what, call in calls:
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value) == "%s (grid search / cost volume): %s" % (what, POS), what
        # past the Python layer: the library's own refusal, with the code and the text it always had
        g = _lib.grid()
        n0, n1 = m.extent
        U = 2 * m.max_shift - 1
        vol = np.zeros((U, U, n0, n1))
        rc = g.cost_volume(m._handle, 0, 1, n0, 0, 1, n1, vol.ctypes.data, None, None, 0, None)
        assert rc == -4 and "a table consumer is set (grid search / cost volume): the plain tiled path does not take" in g.error(), (rc, g.error())
        _same(_np(m.match(quiet=True)), before, "the walk")

    refused()
    m.general_grid = True
    assert m.general_grid is True
    on = [_np(call()) for _, call in calls]
    assert all("covered" in r for r in on[1:]) and "covered" not in on[0]
    _same(_np(m.match(quiet=True)), before, "the walk with the switch on")
    # widening and scale space: refused by name while the switch is on, in Python and by the library; the walk works afterwards
    for call, name in ((lambda: m.cost_volume(widen=1), "widen=1"), (lambda: m.match(quiet=True, search="grid", widen=1), "widen=1"),
                       (lambda: widen.coarse_to_fine(m, levels=(2, 1, 0)), "coarse_to_fine"),
                       (lambda: levels.scale_space(m, levels=(2, 1, 0)), "scale_space")):
        with pytest.raises(RuntimeError) as e:
            call()
        assert FINISHED in str(e.value) and name in str(e.value), str(e.value)
    g = _lib.grid()
    n0, n1 = m.extent
    U = 2 * m.max_shift - 1
    vol = np.zeros((U, U, n0, n1))
    rc = g.wide_cost_volume(m._handle, 0, 1, n0, 0, 1, n1, 1, vol.ctypes.data, None, None, 0, None)
    assert rc == -4 and FINISHED in g.error() and "general table" in g.error(), (rc, g.error())
    _same(_np(m.match(quiet=True)), before, "the walk after the refusals")
    m.general_grid = False
    assert m.general_grid is False
    refused()
    m.general_grid = True
    for a, (_, call) in zip(on, calls):
        _same(_np(call()), a, "on again")
    # a NULL model: the code and the text, before anything touches a device
    assert g.set_general(None, 1) == -1 and g.error() == "grid: set_general: null model"
