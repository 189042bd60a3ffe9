"""
The masked grid consumers (model.masked_grid; libumpa_grid.so's masked_* kernels, which read EVERY entry of corr_masked's table
of finished costs) where tests/test_hip_masked_grid.py does not take them, on the GPU:

  A. the edges of the search range -- max_shift 2 (no 4x4 neighbourhood fits: every err is 0; the ring of 3 U rows is smaller
     than the 32 rows kept for the basin list), 3 (one placement), 6 (the last full-wave sequence state), 7 and 8 (a wave takes
     32 pixels: SequenceArgs::half) -- and region widths of 64, 65 and 70 columns, all five kernels, both kinds;
  B. every corr_masked instantiation (kind x Nw 1 .. 8) read in full at max_shift 4, where the last pass is ragged for every
     masked_ub, against extended precision on a lattice with the tile seam and the border of the search box;
  C. the input regimes of tests/regimes.py with binary, real and tiny (x 2^-24) masks: the volume within the a-priori bound,
     T and df at the parity bar, the grid search; exact powers of two change no bit of any of the five consumers;
  D. NaN, +Inf, -Inf and 0 pixels in the interior, on the tile seam, inside the padding border and in the last frame, with
     live mask weight and under a zero weight (0 * NaN: the mask does not hide it), and a zero weight on clean data.

tests/masked_grid_expect.py has the inputs and expectations, tests/test_masked_grid_cpu.py shows every condition used here on
the reference side.  The consumers are compared BIT FOR BIT with their numpy restatements (basins_expect, track_expect,
sequence_expect, consumer_expect.first_strict_minimum / grid_err_rule) on the device's own masked volume.

DF_FACTOR: at visibility 1e-3 the CPU oracle's own df is further than 1e-6 from extended precision on this stack (three frames,
5 x 5 windows), so the device is held to DF_FACTOR times the oracle's own largest error on the same sampled well-posed cells:
twice the largest r_gpu / r_ref observed on an MI355X (tests/golden/masked_grid_regimes_observed.json, written by a run with
UMPA_RECORD_REGIMES=<output directory>; the factor 2 because the maximum of a rounding-error sample moves with the seed).

Two bars come from the reference's own error rather than from a flat figure, both shown on the CPU
(tests/test_masked_grid_cpu.py): df is held to its a-priori relative bound (oracle/hp_cost.py: df_bound) on every well-posed
cell and to the flat 1e-5 where that bound is below it -- where df crosses zero the CPU oracle itself is 1.1e-4 off at
visibility 1e-2 --, and the number of pixels that may miss the sub-pixel bar in a regime case is the reference's own count of
ill-posed Newton pixels (masked_grid_expect.illposed_count; 0.05 % to 4.6 % of the ok pixels, above assert_parity's default
0.2 %).  Measured on an MI355X: max |gpu - hp| / bound 0.144 (plain), 0.073 (dark-field), max |df - hp| / bound 0.045, no
well-posed cell non-finite, every consumer equal to its restatement (profiles/masked_grid_regimes.txt).

121 cases, 107 s on an MI355X host, 3.6 s the slowest (max_shift 8); the host side dominates: one longdouble volume per case
and the python loops of the restatements.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import basins_expect as BE
import consumer_expect as CE
import grid_expect as GE
import masked_grid_expect as ME
import regimes as R
import sequence_expect as SE
import track_expect as TE
from conftest import GOLDEN, assert_parity

pytestmark = pytest.mark.gpu

DF_FACTOR = 1.71                 # df of the masked volume at visibility 1e-3: 0.16 .. 0.86 of the oracle's own error
_OBSERVED_PATH = os.path.join(GOLDEN, "masked_grid_regimes_observed.json")
RECORD = bool(os.environ.get("UMPA_RECORD_REGIMES"))
_seen, _stats = {}, {}
INF = float("inf")


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    yield model
    if RECORD and _seen:
        out = os.environ["UMPA_RECORD_REGIMES"]                       # the directory to write into
        os.makedirs(out, exist_ok=True)
        worst = max(v["r_gpu"] / v["r_ref"] for v in _seen.values())
        json.dump(dict(max_r_gpu_over_r_ref=worst, cases=_seen, volumes=_stats),
                  open(os.path.join(out, "masked_grid_regimes_observed.json"), "w"), indent=1, sort_keys=True)


def _mk(ns, sam, ref, mask, Nw, ms, kind, assign, subpx):
    m = (ns.UMPAModelDF if kind else ns.UMPAModelNoDF)(sam, ref, mask_list=mask, window_size=Nw, max_shift=ms)
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    m.masked_grid = True
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


def _bare(d):
    """a result without the key the masked models add (the restatements know the plain keys)"""
    return {n: v for n, v in d.items() if n != "covered"}


def _fit(m):
    return BE.device_fit(m.sub_pixel_mode, m._device) if m.sub_pixel_mode else None


def _rel(a, b):
    return np.abs(a - b) / np.abs(b)


def _against_hp(vol, v, kind, what, df_flat=True):
    """test_hip_masked_grid.py::test_cost_volume_against_extended_precision's judgement of a device volume (dict of
    [U, U, ...] arrays) against masked_grid_expect.hp_of's `v` on the same cells: dead cells are not < +Inf and not -Inf;
    held cells within the a-priori bound; a cell is lost only where deficient; T within consumer_expect.RTOL on the
    well-posed cells; df within its own a-priori relative bound (oracle/hp_cost.py: df_bound) on every well-posed cell, hence
    within RTOL wherever that bar can be met at all -- where df crosses zero, or at low contrast, its numerator cancels and
    the CPU oracle itself is further off than RTOL (tests/test_masked_grid_cpu.py) -- and, with `df_flat`, within RTOL on
    every cell whose bound is below RTOL.  Returns the figures, the relative df errors and the held cells."""
    cost = vol["cost"]
    assert cost.shape == v["cost"].shape, what
    dead, deficient = v["dead"], v["deficient"]
    with np.errstate(invalid="ignore"):
        assert not (cost[dead] < INF).any() and not (cost[dead] == -INF).any(), what
    valued = np.isfinite(v["cost"].astype(np.float64)) & ~v["singular"]
    assert not (~dead & ~valued & ~deficient).any(), what
    lost = ~dead & ~np.isfinite(cost)
    held = valued & np.isfinite(cost)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(cost.astype(np.longdouble) - v["cost"]) / v["bound"]
    well = held & ~deficient
    assert well.sum() > 0.8 * cost.size * (1 - dead.mean()), what
    rT = _rel(vol["T"][well], v["T"][well])
    st = dict(cells=int(cost.size), dead=int(dead.sum()), deficient=int(deficient.sum()), lost=int(lost.sum()),
              ratio=float(ratio[held].max()), T=float(rT.max()))
    rdf = None
    if kind:
        rdf = np.zeros(cost.shape)
        rdf[well] = _rel(vol["df"][well], v["df"][well])
        dfb = v["df_bound"].astype(np.float64)
        tight = well & (dfb < CE.RTOL)
        st["df"] = float(rdf[tight].max())
        st["df_all"] = float(rdf.max())
        st["df_over_bound"] = float((rdf[well] / dfb[well]).max())
        st["df_loose_cells"] = int((well & ~tight).sum())
    print("%s: %d cells, dead %d, rank-deficient %d of which non-finite on the device %d, max |gpu - hp| / bound %.4f, T rel %.2e%s" % (
        what, st["cells"], st["dead"], st["deficient"], st["lost"], st["ratio"], st["T"],
        ", df rel %.2e (%.2e with the %d cells whose own bound is above 1e-5), max |df - hp| / bound %.4f" % (
            st["df"], st["df_all"], st["df_loose_cells"], st["df_over_bound"]) if kind else ""))
    _stats[what] = st
    assert not (lost & ~deficient).any(), "%s: %d well-posed cells are not finite on the device" % (what, (lost & ~deficient).sum())
    assert lost.sum() <= deficient.sum(), what
    assert np.all(ratio[held] <= 1.0), "%s: max |gpu - hp| / bound = %.4f" % (what, ratio[held].max())
    assert np.all(rT <= CE.RTOL), "%s: T rel %.2e" % (what, rT.max())
    if kind:
        assert np.all(rdf[well] <= dfb[well]), "%s: max |df - hp| / bound = %.4f" % (what, st["df_over_bound"])
        assert tight.sum() > 0.8 * well.sum(), what
        if df_flat:
            assert np.all(rdf[tight] <= CE.RTOL), "%s: df rel %.2e" % (what, st["df"])
    return st, rdf, held


def _volume(m):
    """the device's volume with T (df), with pixels that have no finite cost and pixels that have some"""
    vol = m.cost_volume(with_fit=True)
    fin = np.isfinite(vol["cost"])
    U = fin.shape[0]
    n = fin.reshape((U * U,) + fin.shape[2:]).sum(axis=0)
    assert (n == 0).any() and ((n > 0) & (n < U * U)).any(), "the volume has pixels with NaN at all and at some shifts"
    return vol


def _grid_on_own_volume(m, got, vol, kind, what):
    """match(search='grid') against include/umpa_grid.h on the device's own volume: the first strict minimum and the err rule
    (consumer_expect) on the covered pixels; every map EQUAL to rank 0 of the basins restatement there (the lowest basin is
    the first strict minimum); uncovered pixels keep their zeros"""
    ms, subpx = m.max_shift, m.sub_pixel_mode
    cov = vol["covered"]
    cost = vol["cost"]
    ci, cj, cmin, found = CE.first_strict_minimum(cost)
    err, ip, jp = CE.grid_err_rule(ci, cj, cost, ms)
    sel = cov & found
    np.testing.assert_array_equal(got["debug_d"][..., 12][sel], cmin[sel], err_msg=what)
    np.testing.assert_array_equal(got["err"][sel], err[sel], err_msg=what)
    np.testing.assert_array_equal(got["dy"][sel & (err == 0)], ci[sel & (err == 0)], err_msg=what)
    np.testing.assert_array_equal(got["dx"][sel & (err == 0)], cj[sel & (err == 0)], err_msg=what)
    np.testing.assert_array_equal(got["f"][sel & (err == 0)], cmin[sel & (err == 0)], err_msg=what)
    if subpx == 0:
        np.testing.assert_array_equal(got["f"][sel & (err == 1)], (1.0 - ip)[sel & (err == 1)], err_msg=what)
    assert not got["err"][cov & ~found].any(), what
    np.testing.assert_array_equal(got["debug_Ncalls"][cov], cost.shape[0] ** 2, err_msg=what)
    keys = ("dx", "dy", "f", "T") + (("df",) if kind else ())
    for k in keys + ("err", "debug_Ncalls"):
        assert not np.asarray(got[k])[~cov].any(), (what, k)
    for k in keys:
        assert not np.asarray(got[k])[cov & ~found].any(), (what, k)
    want = BE.restate(cost, vol["T"], vol.get("df"), 1, subpx, fit=_fit(m))
    for k in keys:
        np.testing.assert_array_equal(got[k][sel], want[k][0][sel], err_msg="%s %s" % (what, k))
    np.testing.assert_array_equal(got["err"][sel], want["err"][0][sel], err_msg=what)
    return sel, err


def _grid_equal(t, g, cov, kind, what):
    for n in ("dx", "dy", "f", "T", "err") + (("df",) if kind else ()):
        np.testing.assert_array_equal(np.asarray(t[n])[cov], np.asarray(g[n])[cov], err_msg="%s against search='grid': %s" % (what, n))


def _consumers(m, vol, kind, what, ks=(4,), tracks=((0.5, 3.0),), seqs=None, seed=31, unit=None):
    """basins, track and sequence EQUAL their restatements on the device's own volume `vol`, at every pixel.
    tracks: (lam in units of the cost scale or None for nearest, radius or None); seqs: (state, lam, trunc) in the same
    units; the unit is `unit`, by default the volume's own scale.  Returns {name: [results]}."""
    subpx, fit = m.sub_pixel_mode, _fit(m)
    args = (vol["cost"], vol["T"], vol.get("df"))
    s = unit or ME.scale(vol["cost"])
    out = dict(basins=[], track=[], sequence=[])
    for k in ks:
        b = m.basins(k=k)
        BE.assert_equal(_bare(b), BE.restate(*args, k, subpx, fit=fit), "%s basins k %d" % (what, k))
        np.testing.assert_array_equal(b["covered"], vol["covered"])
        out["basins"].append(b)
    pdx, pdy = ME.prior(m.max_shift, vol["cost"].shape[2:], seed)
    for lam, radius in tracks:
        lam = None if lam is None else lam * s
        t = m.track(pdx, pdy, lam=lam, radius=radius)
        want = TE.restate(*args, pdy, pdx, TE.NEAREST if lam is None else TE.PENALTY, 0.0 if lam is None else lam, radius, subpx, fit=fit)
        TE.assert_equal(_bare(t), want, "%s track lam %r radius %r" % (what, lam, radius))
        np.testing.assert_array_equal(t["covered"], vol["covered"])
        out["track"].append(t)
    for state, lam, trunc in (seqs if seqs is not None else [(ME.state(vol["cost"], 11, special=True), 0.1, 3.0)]):
        lam, trunc = lam * s, None if trunc is None else trunc * s
        (q, seen) = _launches(m, lambda: m.sequence(state=state, lam=lam, trunc=trunc))
        assert seen.get("table_consumer") == 1 and "replay_cost" not in seen, (what, seen)
        SE.assert_equal(_bare(q), SE.restate(*args, state, lam, trunc, subpx, fit=fit), "%s sequence lam %r trunc %r" % (what, lam, trunc))
        np.testing.assert_array_equal(q["covered"], vol["covered"])
        out["sequence"].append(q)
    return out


# ----------------------------------------------------------------------------- A. search-range edges, wave edges

@pytest.mark.parametrize("Nw,ms,N1,kind,assign,which,subpx", ME.EDGE_CASES, ids=ME.EDGE_IDS)
def test_search_range_and_wave_edges(hip_ns, Nw, ms, N1, kind, assign, which, subpx):
    sam, ref, masks = ME.edge_inputs(Nw, ms, N1)
    mask = masks[which]
    U = 2 * ms - 1
    what = "edge Nw %d ms %d width %d %s %s %s subpx %d" % (Nw, ms, N1, "DF" if kind else "NoDF", assign, which, subpx)
    m = _mk(hip_ns, sam, ref, mask, Nw, ms, kind, assign, subpx)
    vol, seen = _launches(m, lambda: _volume(m))
    assert seen.get("corr_masked", 0) >= 1 and seen.get("table_consumer") == 1 and "replay_cost" not in seen, seen
    assert vol["cost"].shape == (U, U, ME.EDGE_ROWS, N1) and m.extent == (ME.EDGE_ROWS, N1)
    cov = ME.covered_of(mask, Nw, ms)
    np.testing.assert_array_equal(vol["covered"], cov)
    _against_hp(vol, ME.hp_of(sam, ref, mask, Nw, ms, kind, assign), kind, what)

    g, seen = _launches(m, lambda: m.match(quiet=True, search="grid"))
    m.ROI = None
    assert seen.get("table_consumer") == 1 and "replay_cost" not in seen, seen
    sel, _ = _grid_on_own_volume(m, g, vol, kind, what)
    assert sel.mean() > 0.9

    cost = vol["cost"]
    st = ME.state(cost, 7 + ms)
    res = _consumers(m, vol, kind, what, ks=(1, 8), tracks=((None, None), (None, 2.5), (0.5, None), (0.5, 3.0)),
                     seqs=[(None, 0.3, None), (st, 0.25, None), (st, 0.25, 1.5), (ME.state(cost, 11, special=True), 0.1, 3.0)])
    # two chained steps from the device's own state
    s0, s1 = res["sequence"][0], res["sequence"][1]
    chain = _consumers(m, vol, kind, what + " chained", ks=(), tracks=(), seqs=[(s1["state"], 0.25, 1.5)])["sequence"][0]
    _consumers(m, vol, kind, what + " chained twice", ks=(), tracks=(), seqs=[(chain["state"], 0.25, None)])
    # lam = 0 and "no state" are the grid search on the covered pixels
    lam0 = m.sequence(state=st, lam=0.0, trunc=0.7 * ME.scale(cost))
    for t, name in ((s0, "no state"), (lam0, "lam 0")):
        _grid_equal(t, g, cov, kind, "%s sequence %s" % (what, name))
        assert not np.asarray(t["moved"]).any()
    _grid_equal(m.track(0.0, 0.0, lam=0.0), g, cov, kind, what + " track lam 0")
    b1 = res["basins"][0]
    _grid_equal({n: (np.maximum(b1[n][0], 0) if n == "err" else b1[n][0]) for n in b1 if n not in ("count", "covered", "shift")}, g, cov, kind,
                what + " basins rank 0")
    assert {0, 1} == set(np.unique(s1["moved"]).tolist())
    errs = [("grid", g["err"][cov])] + [("basins", b["err"]) for b in res["basins"]] + [("track", t["err"]) for t in res["track"]] + \
           [("sequence", q["err"]) for q in res["sequence"]]
    for name, e in errs:
        if ms == 2:                                                   # a box of 3 x 3 shifts holds no 4 x 4 neighbourhood
            assert not (np.asarray(e) == 1).any() and (np.asarray(e) == 0).any(), (what, name)
        else:
            assert (np.asarray(e) == 1).any() and (np.asarray(e) == 0).any(), (what, name)


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_exact_ties_go_to_the_first_shift_in_scan_order(hip_ns, kind):
    """The reference stack and the mask repeat every three columns, so shifts three columns apart cost the same bit for bit
    (pinned in extended precision by tests/test_masked_grid_cpu.py): the minimum ties with itself, and every consumer must
    take the first one in scan order -- `<`, not `<=`."""
    sam, ref, mask = ME.tie_inputs()
    c, p = ME.TIE, ME.TIE["period"]
    what = "ties %s" % ("DF" if kind else "NoDF")
    m = _mk(hip_ns, sam, ref, mask, c["Nw"], c["ms"], kind, "sam", 0)
    vol = m.cost_volume(with_fit=True)
    cost = vol["cost"]
    assert np.array_equal(cost[:, :-p], cost[:, p:], equal_nan=True), "the device's table does not repeat with the stacks"
    ci, cj, cmin, found = CE.first_strict_minimum(cost)
    ii, jj = np.meshgrid(np.arange(cost.shape[2]), np.arange(cost.shape[3]), indexing="ij")
    again = cost[ci + c["ms"] - 1, np.minimum(cj + p, c["ms"] - 1) + c["ms"] - 1, ii, jj] == cmin
    assert found.mean() > 0.95 and (again & found & (cj < 0)).mean() > 0.5
    g = m.match(quiet=True, search="grid")
    m.ROI = None
    _grid_on_own_volume(m, g, vol, kind, what)
    np.testing.assert_array_equal(g["dx"][vol["covered"] & found & (g["err"] == 0)], cj[vol["covered"] & found & (g["err"] == 0)])
    st = ME.state(cost, 5)
    _consumers(m, vol, kind, what, ks=(1, 8), tracks=((None, None), (0.5, 3.0)), seqs=[(None, 0.3, None), (st, 0.25, 1.5)])


# ----------------------------------------------------------------------------- B. every corr_masked instantiation, read in full

@pytest.mark.parametrize("kind,Nw", ME.INST_CASES, ids=ME.INST_IDS)
def test_every_corr_masked_instantiation_read_in_full(hip_ns, kind, Nw):
    """max_shift 4: U = 7 columns of the search box in passes of masked_ub = 5, 3 or 2, the last one ragged.  The volume kernel
    copies every entry of the table, those at the border of the search box and of the last pass included."""
    sam, ref, mask = ME.inst_inputs(kind, Nw)
    assign, which = ME.inst_mode(kind, Nw)
    ms, U = ME.INST_MS, 2 * ME.INST_MS - 1
    m = _mk(hip_ns, sam, ref, mask, Nw, ms, kind, assign, 0)
    vol, seen = _launches(m, lambda: m.cost_volume(with_fit=True))
    assert seen.get("corr_masked", 0) >= 1 and seen.get("table_consumer") == 1 and "replay_cost" not in seen, seen
    assert vol["cost"].shape == (U, U) + ME.INST_EXTENT
    np.testing.assert_array_equal(vol["covered"], ME.covered_of(mask, Nw, ms))
    xi, xj = ME.inst_pixels()
    on = {k: a[:, :, xi, xj] for k, a in vol.items() if k != "covered"}
    v = ME.inst_hp(kind, Nw)
    _, _, held = _against_hp(on, v, kind, "instantiation %s Nw %d %s %s" % ("DF" if kind else "NoDF", Nw, assign, which))
    # the border of the search box and both sides of the tile seam are among the cells judged
    for a in (0, U - 1):
        assert held[a].mean() > 0.8 and held[:, a].mean() > 0.8
        for b in (0, U - 1):
            assert held[a, b].mean() > 0.8
    rows = xi[:, 0].tolist()
    assert held[:, :, rows.index(ME.INST_SEAM - 1)].mean() > 0.8 and held[:, :, rows.index(ME.INST_SEAM)].mean() > 0.8
    assert v["dead"].any()


# ----------------------------------------------------------------------------- C. the input regimes

@pytest.mark.parametrize("regime,which,kind,assign", ME.REGIME_CASES, ids=ME.REGIME_IDS)
def test_volume_and_grid_search_per_regime(hip_ns, port_ns, regime, which, kind, assign):
    sam, ref, c = ME.regime_stack(regime)
    mask = ME.regime_mask(which)
    Nw, ms = c["Nw"], c["ms"]
    what = "regime %s %s %s %s" % (regime, which, "DF" if kind else "NoDF", assign)
    m = _mk(hip_ns, sam, ref, mask, Nw, ms, kind, assign, 0)
    vol = m.cost_volume(with_fit=True)
    cov = ME.covered_of(mask, Nw, ms)
    np.testing.assert_array_equal(vol["covered"], cov)
    np.testing.assert_array_equal(cov, ME.covered(ME.SMALL, "real" if which == "tiny" else which))    # the mask alone, whatever its scale
    v = ME.regime_hp(regime, which, kind, assign)
    assert v["dead"].sum() == ME.DEAD_CELLS and v["deficient"].sum() == ME.DEFICIENT_CELLS[(kind, which)]
    loose = bool(kind) and regime == "vis1e-3" and (which, assign) in ME.ORACLE_LOOSE_DF
    _, rdf, _ = _against_hp(vol, v, kind, what, df_flat=not loose)
    if loose:
        r_ref, n = ME.oracle_df_error(port_ns, regime, which, assign)
        flat = ME.well_posed_sample(v)[0]
        r_gpu = float(rdf.ravel()[flat].max())
        print("%s: %d sampled cells: r_gpu %.2e, the oracle's r_ref %.2e, ratio %.3f" % (what, n, r_gpu, r_ref, r_gpu / r_ref))
        _seen["df " + what] = dict(r_gpu=r_gpu, r_ref=r_ref)
        assert r_ref > 1e-6
        assert r_gpu <= DF_FACTOR * r_ref, "r_gpu / r_ref = %.2f, above the factor %.2f" % (r_gpu / r_ref, DF_FACTOR)

    none, some, whole = ME.pixel_classes(v)
    keys = ("err", "debug_Ncalls", "dx", "dy", "f", "T", "debug_a", "debug_d") + (("df",) if kind else ())
    illposed = None
    for subpx in (0, -1, 1):
        if subpx and (regime, kind) in CE.PARITY_INADMISSIBLE:
            continue
        m.sub_pixel_mode = subpx
        got = m.match(quiet=True, search="grid")
        m.ROI = None
        exp, near, _ = ME.regime_expected(regime, which, kind, assign, subpx)
        judged = whole & ~near & cov
        assert judged.mean() > 0.8
        assert near.sum() <= GE.NEAR_TIE_CAP * (~none).sum()
        if subpx and illposed is None:
            # a pixel may miss the sub-pixel bar only where the reference's own Newton iteration is ill-posed; how many there
            # are is the reference's to say (it grows with the regime: 0.05 % to 4.6 % of the ok pixels here), not a flat share
            illposed = (ME.illposed_count(exp, judged) + 0.5) / max(1, int((exp["err"] == 1).sum()))
        for k in keys:
            assert not np.asarray(got[k])[~cov].any(), k
        assert not got["err"][none].any() and not any(np.asarray(got[k])[none].any() for k in ("dx", "dy", "f", "T"))
        want = {k: exp[k] for k in keys}
        mine = {k: np.array(got[k]) for k in keys}
        for k in keys:
            mine[k][~judged] = want[k][~judged]
        if subpx == 0:
            np.testing.assert_array_equal(got["dy"][judged], exp["ci"][judged])
            np.testing.assert_array_equal(got["dx"][judged], exp["cj"][judged])
        assert_parity(mine, want, ms, "masked grid %s subpx %d" % (what, subpx), subpx=subpx, allow_illposed=illposed if subpx else None)
        if subpx == 0:
            _grid_on_own_volume(m, got, vol, kind, what)


def test_df_factor_is_twice_the_recorded_ratio():
    """DF_FACTOR is a constant of this module, so that a change of the threshold shows in a diff; it must be what the recorded
    run (tests/golden/masked_grid_regimes_observed.json) gives."""
    obs = json.load(open(_OBSERVED_PATH))
    cases = obs["cases"]
    assert set(cases) == {"df regime vis1e-3 %s DF %s" % (w, a) for (w, a) in ME.ORACLE_LOOSE_DF}
    worst = max(v["r_gpu"] / v["r_ref"] for v in cases.values())
    assert abs(obs["max_r_gpu_over_r_ref"] - worst) < 1e-12
    assert worst <= 8.0 and abs(DF_FACTOR - 2.0 * worst) <= 0.006, (worst, DF_FACTOR)


def _five(m, pdx, pdy, state, lam_t, lam_s, trunc):
    out = {"grid": m.match(quiet=True, search="grid")}
    m.ROI = None
    out["volume"] = m.cost_volume(with_fit=True)
    out["basins"] = m.basins(k=5)
    out["track"] = m.track(pdx, pdy, lam=lam_t, radius=3.0)
    out["sequence"] = m.sequence(state=state, lam=lam_s, trunc=trunc)
    return {k: {n: np.asarray(a) for n, a in v.items() if not n.startswith("_")} for k, v in out.items()}


SCALED = ("cost", "f", "total", "state", "cost0", "debug_a")          # what goes with the costs; everything else keeps its bits


@pytest.mark.parametrize("which", ME.REGIME_MASKS)
@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_powers_of_two_change_no_bit_of_any_masked_consumer(hip_ns, kind, which):
    """Both stacks times 2^e, lam and trunc times 2^(2e): every cost, f, total and state is 2^(2e) times the base's, every
    other map keeps its bits -- the pair weight w ma mb / (ma + mb + 1e-8) reads the masks alone, and every other operation
    on these paths commutes with powers of two.  An absolute constant anywhere on them shows here."""
    sam, ref, c = ME.stack(ME.SMALL)
    mask = ME.regime_mask(which)
    assign = "sam" if kind else "ref"
    N0, N1 = CE.extent(c)
    pdx, pdy = ME.prior(c["ms"], (N0, N1), 17)
    base_m = _mk(hip_ns, sam, ref, mask, c["Nw"], c["ms"], kind, assign, -1)
    cost = base_m.cost_volume()["cost"]
    s = ME.scale(cost)
    state = ME.state(cost, 9, special=True)
    base = _five(base_m, pdx, pdy, state, 0.5 * s, 0.1 * s, 3.0 * s)
    assert base["sequence"]["moved"].any() and (base["track"]["found"] > 0).any() and (base["basins"]["count"] > 1).any()
    for e in (16, -5):
        s2, r2 = R.scaled(sam, ref, e, e)
        m = _mk(hip_ns, s2, r2, mask, c["Nw"], c["ms"], kind, assign, -1)
        got = _five(m, pdx, pdy, np.ldexp(state, 2 * e), np.ldexp(0.5 * s, 2 * e), np.ldexp(0.1 * s, 2 * e), np.ldexp(3.0 * s, 2 * e))
        for name in base:
            assert sorted(got[name]) == sorted(base[name])
            for k, a in base[name].items():
                want = a
                if k in SCALED:
                    want = np.ldexp(a, 2 * e)
                elif k == "debug_d":
                    want = np.where(a >= 0, np.ldexp(a, 2 * e), a)    # cells outside the box stay -1
                assert np.array_equal(got[name][k], want, equal_nan=True), "2^%d %s %s: %s differs on %d entries" % (
                    e, which, name, k, int((~((got[name][k] == want) | (np.isnan(got[name][k]) & np.isnan(want)))).sum()))


# ----------------------------------------------------------------------------- D. bad pixels

@functools.lru_cache(maxsize=None)
def _bad_state():
    """(state, unit): a sequence state and a cost unit that are the same for every run of this section, clean or dirty, so
    that lam and trunc are: from the extended-precision volume of the clean stack"""
    cost = np.ascontiguousarray(ME.hp(ME.SMALL, "real", 0, "sam")["cost"].astype(np.float64))
    return ME.state(cost, 11, special=True), ME.scale(cost)


def _bad_run(m, kind, what):
    """the volume and the grid search, basins, track and sequence of a model, each EQUAL to its restatement on that volume"""
    vol = m.cost_volume(with_fit=True)
    g = m.match(quiet=True, search="grid")
    m.ROI = None
    state, unit = _bad_state()
    _grid_on_own_volume(m, g, vol, kind, what)
    res = _consumers(m, vol, kind, what, seqs=[(state, 0.1, 3.0)], unit=unit)
    return dict(volume=vol, grid=g, basins=res["basins"][0], track=res["track"][0], sequence=res["sequence"][0])


@functools.lru_cache(maxsize=None)
def _clean(kind, assign, situation):
    """the clean stack under the situation's mask: the volume and the consumers"""
    from umpa_amd import model
    sam, ref, mask = ME.bad_inputs(None, "sam", kind, assign, situation)
    c = CE.CONFIGS["vol"]
    m = _mk(model, sam, ref, mask, c["Nw"], c["ms"], kind, assign, -1)
    return _bad_run(m, kind, "clean data, %s, %s" % (CE.mode_id(kind, assign), situation))


def _far_equal(got, clean, far, what):
    """pixels out of every bad pixel's reach: every map of every consumer is bit-identical to the clean run's"""
    for name in ("grid", "basins", "track", "sequence"):
        for k, a in got[name].items():
            if k.startswith("_") or k == "covered":
                continue
            a, b = np.asarray(a), np.asarray(clean[name][k])
            a, b = (a[far], b[far]) if k.startswith("debug_") else (a[..., far], b[..., far])
            assert np.array_equal(a, b, equal_nan=True), "%s: %s %s differs out of reach of the bad pixels" % (what, name, k)


BAD = ME.bad_cases()


@pytest.mark.parametrize("value,where,kind,assign,situation", BAD, ids=["%s-%s-%s-%s" % (v, w, CE.mode_id(k, a), s) for v, w, k, a, s in BAD])
def test_bad_pixels_with_and_under_the_mask(hip_ns, value, where, kind, assign, situation):
    """A mask weight of 0 does not hide a NaN or an Inf: the pair weight is 0 and 0 * NaN is NaN, in the reference
    (tests/test_regimes_cpu.py) and in corr_masked.  So the footprint of a bad pixel is the same with and without weight."""
    sam, ref, mask = ME.bad_inputs(value, where, kind, assign, situation)
    c = CE.CONFIGS["vol"]
    Nw, ms = c["Nw"], c["ms"]
    what = "%s in %s, %s, %s" % (value, where, CE.mode_id(kind, assign), situation)
    m = _mk(hip_ns, sam, ref, mask, Nw, ms, kind, assign, -1)
    got = _bad_run(m, kind, what)
    clean = _clean(kind, assign, situation)
    vol, cvol = got["volume"], clean["volume"]
    np.testing.assert_array_equal(vol["covered"], ME.covered_of(mask, Nw, ms))
    np.testing.assert_array_equal(vol["covered"], cvol["covered"])
    foot = ME.bad_footprint(where, assign)
    for k in ("cost", "T") + (("df",) if kind else ()):
        assert np.array_equal(vol[k][~foot], cvol[k][~foot], equal_nan=True), "%s: %s differs from the clean volume off the footprint" % (what, k)
    if value == "zero":
        v = ME.hp_of(sam, ref, mask, Nw, ms, kind, assign)
        _against_hp(vol, v, kind, what)
        assert np.isfinite(vol["cost"][foot & ~v["dead"] & ~v["deficient"]]).all()
        if situation == "live":
            assert (vol["cost"][foot] != cvol["cost"][foot]).mean() > 0.8
        elif kind == 0 or where == "sam":                             # a zero under a zero weight is hidden: 0 * 0 ...
            assert np.array_equal(vol["cost"], cvol["cost"], equal_nan=True)   # (... but from the dark-field model's window mean
            #                                                                     of the reference, which no mask weights)
    else:
        with np.errstate(invalid="ignore"):
            assert not (vol["cost"][foot] < INF).any() and not (vol["cost"][foot] == -INF).any(), what
    far = ME.bad_far()
    assert far.mean() > 0.3 and not foot[:, :, far].any()
    _far_equal(got, clean, far, what)


@pytest.mark.parametrize("kind,assign", CE.BAD_MODES, ids=[CE.mode_id(*c) for c in CE.BAD_MODES])
def test_a_zero_weight_on_clean_data(hip_ns, kind, assign):
    """what masks are for: the bad positions masked out of clean data.  Within bound of its own extended-precision volume, the
    footprint cells included; covered changes only through the mask edit; off the footprint nothing changes at all."""
    c = CE.CONFIGS["vol"]
    Nw, ms = c["Nw"], c["ms"]
    sam, ref, mask0 = ME.bad_inputs(None, "sam", kind, assign, "under0")
    what = "zero weight on clean data, %s" % CE.mode_id(kind, assign)
    got, live = _clean(kind, assign, "under0"), _clean(kind, assign, "live")
    _against_hp(got["volume"], ME.hp_of(sam, ref, mask0, Nw, ms, kind, assign), kind, what)
    np.testing.assert_array_equal(got["volume"]["covered"], ME.covered_of(mask0, Nw, ms))
    changed = got["volume"]["covered"] != live["volume"]["covered"]
    at = np.zeros_like(changed)
    for (_, r, col) in CE.bad_positions("vol"):
        if CE.pad(c) <= r < c["H"] - CE.pad(c) and CE.pad(c) <= col < c["W"] - CE.pad(c):
            at[r - CE.pad(c), col - CE.pad(c)] = True
    assert not (changed & ~at).any()
    # the pair weight of a window pixel needs both masks: the footprint of a zero weight is that of a bad pixel in BOTH stacks
    foot = ME.bad_footprint("sam", assign) | ME.bad_footprint("ref", assign)
    for k in ("cost", "T") + (("df",) if kind else ()):
        assert np.array_equal(got["volume"][k][~foot], live["volume"][k][~foot], equal_nan=True), k
    assert (got["volume"]["cost"][foot] != live["volume"]["cost"][foot]).mean() > 0.8
