"""
The masked grid consumers (model.masked_grid, umpa_grid_set_masked), what can be checked without a GPU: the inputs of the GPU
tests (tests/masked_grid_expect.py) meet the conditions the expectations rest on, the switch is off by default and the
refusals around it come before any device work, the library exports the switch and holds the five masked kernel families, each
claimed by a GPU test.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import grid_expect as GE
import masked_grid_expect as ME
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
TODAY = "masked models are not supported (their table holds finished costs)"
FAMILIES = ("masked_min_kernel", "masked_volume_kernel", "masked_basins_kernel", "masked_track_kernel", "masked_sequence_kernel")


# ----------------------------------------------------------------------------- 1. the inputs

def test_masks_are_the_issue_s():
    for name, c in GE.STACKS.items():
        m = ME.masks(name)
        rng = np.random.default_rng(100 + c["seed"])
        shape = (c["K"], c["H"], c["W"])
        binary = (rng.random(shape) >= 0.10).astype(np.float64)
        real = 0.2 + 0.8 * rng.random(shape)
        for a in (binary, real):
            a[:, 20:34, 24:40] = 0
        np.testing.assert_array_equal(m["binary"], binary)
        np.testing.assert_array_equal(m["real"], real)
        assert set(np.unique(m["binary"])) == {0.0, 1.0}
        live = m["real"][m["real"] != 0]
        assert live.min() >= 0.2 and live.max() <= 1.0 and len(np.unique(live)) > 1000


@pytest.mark.parametrize("name,which,kind,assign", ME.CASES, ids=ME.IDS)
def test_near_tie_shares_and_nan_pixel_counts(name, which, kind, assign):
    """The cap is a condition on the inputs, not on the device: recomputed here from the extended-precision volumes."""
    v = ME.hp(name, which, kind, assign)
    none, some, whole = ME.pixel_classes(v)
    near = ME.near_tie(v)
    share = near.sum() / float((~none).sum())
    print("%s %s kind %d %s: no finite cost %d, some NaN %d, near-tie %.3f %% of %d, deficient cells %d" % (
        name, which, kind, assign, none.sum(), some.sum(), 100.0 * share, (~none).sum(), v["deficient"].sum()))
    assert none.sum() == ME.NO_FINITE[name]
    assert some.sum() == ME.SOME_NAN[name]
    assert whole.sum() == none.size - ME.NO_FINITE[name] - ME.SOME_NAN[name]
    assert share <= GE.NEAR_TIE_CAP
    if which == "real":
        assert near.sum() == 0
    # a dead cell (wt = 0) is NaN in all three volumes; any other NaN is a window whose fit is singular: rank-deficient
    for k in ("cost", "T", "df"):
        if v[k] is not None:
            nan = np.isnan(v[k].astype(np.float64))
            assert nan[v["dead"]].all() and not (nan & ~v["dead"] & ~v["deficient"]).any(), k
    if kind == 0:
        assert np.array_equal(np.isnan(v["cost"].astype(np.float64)), v["dead"])
    # the pixels match() skips are among those the consumers mark: the dead block's centre is below the coverage threshold
    cov = ME.covered(name, which)
    assert not cov.all() and cov.mean() > 0.9
    assert not cov[none].any()


# ----------------------------------------------------------------------------- 2. the switch in Python

class _HipLib:
    is_hip = True


def _stub(cls="UMPAModelNoDF", **kw):
    """a model the way the CPU tests of the siblings build one: no native handle, only what _grid_check reads"""
    from umpa_amd import model
    m = object.__new__(type("Stub", (getattr(model, cls),), {"__del__": lambda self: None}))
    m._lib, m._mask, m._force, m._device = _HipLib(), None, 0, 0
    m._pos_list, m._shape_list, m._padding, m._max_shift = [(0, 0)] * 3, [(40, 48)] * 3, 6, 3
    m._ROI = ((0, 28, 1), (0, 36, 1))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


MASK = [np.ones((40, 48))] * 3
CALLS = ["search='grid'", "cost_volume", "basins", "track", "sequence"]


def _call(m, what, **kw):
    if what == "search='grid'":
        return m.match(quiet=True, search="grid", **kw)
    if what == "cost_volume":
        return m.cost_volume(**kw)
    if what == "basins":
        return m.basins(k=2, **kw)
    if what == "track":
        return m.track(0.0, 0.0, **kw)
    return m.sequence(lam=0.0)


def test_switch_defaults_to_off_and_a_stub_without_it_gives_today_s_text():
    from umpa_amd import model
    for cls in ("UMPAModelNoDF", "UMPAModelDF"):
        assert isinstance(getattr(model, cls).masked_grid, property) and _stub(cls).masked_grid is False
        m = _stub(cls, _mask=MASK)
        assert "_masked_grid" not in m.__dict__ and m.masked_grid is False
        for what in CALLS:
            with pytest.raises(RuntimeError) as e:
                _call(m, what)
            assert str(e.value) == "%s (grid search / cost volume): %s" % (what, TODAY), what
        # a stub of the base class's making, which has no such attribute at all, counts as off
        bare = object.__new__(type("Bare", (model.UMPAModelBase,), {"__del__": lambda self: None, "_kind": 0}))
        bare._lib, bare._mask, bare._force, bare._device = _HipLib(), MASK, 0, 0
        with pytest.raises(RuntimeError) as e:
            bare._grid_check("cost_volume")
        assert str(e.value) == "cost_volume (grid search / cost volume): " + TODAY
    assert not hasattr(model.UMPAModelDFKernel, "masked_grid")


def test_refusals_with_the_switch_on():
    from umpa_amd import levels, widen
    why = "a finished cost is not linear in the windowed sums, so a box average of costs is not the cost under a wider window"
    for cls in ("UMPAModelNoDF", "UMPAModelDF"):
        m = _stub(cls, _mask=MASK, _masked_grid=True)
        assert m.masked_grid is True
        m._grid_check("cost_volume")                                  # admitted
        # window widening and scale space: refused, and the text says why
        for what in CALLS[:4]:
            with pytest.raises(RuntimeError) as e:
                _call(m, what, widen=2)
            assert why in str(e.value) and "widen=2" in str(e.value), (what, str(e.value))
        with pytest.raises(RuntimeError) as e:
            widen.coarse_to_fine(m, levels=(2, 1, 0))
        assert why in str(e.value) and "coarse_to_fine" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            levels.scale_space(m, levels=(2, 1, 0))
        assert why in str(e.value) and "scale_space" in str(e.value)
        # positions and shapes are tested on their own: behind a mask they used to hide
        pos = "frames at different positions (pos_list) or of different shapes are not supported"
        for kw in (dict(_pos_list=[(0, 0), (2, 1), (1, 3)]), dict(_shape_list=[(40, 48), (40, 48), (40, 50)])):
            s = _stub(cls, _mask=MASK, _masked_grid=True, **kw)
            for what in CALLS:
                with pytest.raises(RuntimeError) as e:
                    _call(s, what)
                assert str(e.value) == "%s (grid search / cost volume): %s" % (what, pos), what
        # a forced direct kernel, as on a plain model
        f = _stub(cls, _mask=MASK, _masked_grid=True, _force=2)
        with pytest.raises(RuntimeError, match="forced onto the direct kernel"):
            f.cost_volume()
    # the kernel dark-field model has no table, whatever a switch says
    k = _stub("UMPAModelDFKernel", _mask=MASK, _masked_grid=True)
    with pytest.raises(RuntimeError) as e:
        k._grid_check("search='grid'")
    assert str(e.value) == "search='grid' (grid search / cost volume): the kernel dark-field model has no shift table"
    # a model without masks: the widened calls are not refused by this rule
    plain = _stub(_masked_grid=True)
    plain._no_masked_widening("widen")


# ----------------------------------------------------------------------------- 3. the library

def test_set_masked_is_declared_exported_and_refuses_a_null_model():
    g = _build()
    from umpa_amd import _lib
    assert "umpa_grid_set_masked" in declared("umpa_grid.h", "umpa_grid_")
    assert "set_masked" in _lib.GRID_SYMBOLS and "set_masked" in _lib._GRID_ABI
    assert _lib._GRID_ABI["set_masked"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert "umpa_grid_set_masked" in exported(GRID_LIB)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    lib = _lib.grid()
    for on in (0, 1):
        assert lib.set_masked(None, on) == -1                         # UMPA_HIP_E_ARG, before anything touches a device
        assert lib.error() == "grid: set_masked: null model"
    # the main library: no new public symbol; what the satellite needs of it is not in the public header
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    hdr = open(os.path.join(REPO, "include", "umpa_hip.h")).read()
    assert "masked_consumer" not in hdr and "umpa_hipx" not in hdr


def test_the_five_masked_families_exist_and_are_claimed():
    g = _build()
    keys = kernel_keys(GRID_LIB)
    syms = [k for k in keys if k.startswith("masked_")]
    want = ["%s<%d>" % (f, kind) for f in FAMILIES for kind in (0, 1)]
    assert sorted(syms) == sorted(want), sorted(set(syms) ^ set(want))
    assert_claimed(syms, "masked_grid")
    # the sibling families keep their instantiations
    family = lambda f: [k for k in keys if k.split("<", 1)[0] == f]
    for f in ("grid_min_kernel", "cost_volume_kernel", "grid_basins_kernel", "grid_track_kernel", "grid_sequence_kernel"):
        assert len(family(f)) == 26, f
    # the main library holds none of them
    assert not [k for k in kernel_keys(g.HIP_LIB) if k.startswith("masked_")]


# ----------------------------------------------------------------------------- 4. the inputs of tests/test_hip_masked_grid_regimes.py

import consumer_expect as CE


@pytest.mark.parametrize("Nw,ms,N1,kind,assign,which,subpx", ME.EDGE_CASES, ids=ME.EDGE_IDS)
def test_edge_inputs_hold_every_class_of_pixel(Nw, ms, N1, kind, assign, which, subpx):
    """Search-range and wave edges: the masks are built as masks() builds them, the exact-fit gate admits the stack, the
    extended-precision volume has pixels without a finite cost and pixels with some, and the grid rule gives only err = 0 at
    max_shift 2 and both values from 3 on."""
    sam, ref, masks = ME.edge_inputs(Nw, ms, N1)
    K, H, W = sam.shape
    pad = Nw + ms
    assert (H - 2 * pad, W - 2 * pad) == (ME.EDGE_ROWS, N1) and K * (2 * Nw + 1) ** 2 > 9
    assert set(np.unique(masks["binary"])) == {0.0, 1.0} and 0.08 < (masks["binary"] == 0).mean() < 0.14
    live = masks["real"][masks["real"] != 0]
    assert live.min() >= 0.2 and live.max() <= 1.0
    (r0, r1), (c0, c1) = ME.EDGE_BLOCK
    assert (r1 - r0, c1 - c0) == (8, 10) and c1 <= 64 and not masks[which][:, pad + r0:pad + r1, pad + c0:pad + c1].any()
    v = ME.hp_of(sam, ref, masks[which], Nw, ms, kind, assign)
    none, some, whole = ME.pixel_classes(v)
    assert none.sum() == (8 - 2 * Nw) * (10 - 2 * Nw) and some.sum() > 0 and whole.mean() > 0.8
    cov = ME.covered_of(masks[which], Nw, ms)
    assert not cov[none].any() and cov.mean() > 0.9
    assert ME.near_tie(v).sum() <= GE.NEAR_TIE_CAP * (~none).sum() + 1
    cost = v["cost"].astype(np.float64)
    ci, cj, _, found = CE.first_strict_minimum(cost)
    err = CE.grid_err_rule(ci, cj, cost, ms)[0][cov & found]
    assert set(np.unique(err).tolist()) == ({0} if ms == 2 else {0, 1})
    if ms > 2:
        assert 0.2 < err.mean() < 0.95


@pytest.mark.parametrize("kind,Nw", ME.INST_CASES, ids=ME.INST_IDS)
def test_instantiation_lattice_meets_the_seam_the_border_and_the_dead_block(kind, Nw):
    sam, ref, mask = ME.inst_inputs(kind, Nw)
    ms, pad = ME.INST_MS, Nw + ME.INST_MS
    K = sam.shape[0]
    assert K == (10 if Nw <= 2 else 3) and K * (2 * Nw + 1) ** 2 > 9
    assert (sam.shape[1] - 2 * pad, sam.shape[2] - 2 * pad) == ME.INST_EXTENT and ME.INST_EXTENT[0] > ME.INST_SEAM
    assert (len(np.unique(mask)) == 2) == (Nw % 2 == 0)
    assert ME.inst_mode(kind, Nw)[0] != ME.inst_mode(kind, Nw + 1)[0]
    xi, xj = ME.inst_pixels()
    assert {0, ME.INST_SEAM - 1, ME.INST_SEAM, ME.INST_EXTENT[0] - 1} <= set(xi.ravel().tolist())
    assert {0, 63, 64, 65, ME.INST_EXTENT[1] - 1} <= set(xj.ravel().tolist())
    assert 5000 < xi.size * (2 * ms - 1) ** 2 <= 10000
    v = ME.inst_hp(kind, Nw)
    well = ~v["dead"] & ~v["deficient"]
    print("%s Nw %d: %d cells, dead %d, deficient %d" % ("DF" if kind else "NoDF", Nw, well.size, v["dead"].sum(), v["deficient"].sum()))
    assert v["dead"].all(axis=(0, 1)).sum() >= 1 and well.mean() > 0.9
    assert np.isfinite(v["cost"].astype(np.float64))[well].all()
    U = 2 * ms - 1
    for a in (0, U - 1):                                              # |si| = ms - 1, |sj| = ms - 1: well-posed cells among those judged
        assert well[a].mean() > 0.9 and well[:, a].mean() > 0.9


@pytest.mark.parametrize("regime,which,kind,assign", ME.REGIME_CASES + [("x1", w, k, "sam") for w in ME.REGIME_MASKS for k in (0, 1)],
                         ids=ME.REGIME_IDS + ["x1-%s-%s-sam" % (w, "DF" if k else "NoDF") for w in ME.REGIME_MASKS for k in (0, 1)])
def test_regime_counts_and_near_tie_shares(regime, which, kind, assign):
    """What the GPU module's regime cases judge, pinned: dead and rank-deficient cells, the near-tie share of the all-finite
    pixels, the judged share of the grid-search comparison."""
    v = ME.regime_hp(regime, which, kind, assign)
    none, some, whole = ME.pixel_classes(v)
    near = ME.near_tie(v)
    c = GE.STACKS[ME.SMALL]
    cov = ME.covered_of(ME.regime_mask(which), c["Nw"], c["ms"])
    well = ~v["dead"] & ~v["deficient"]
    rel = float(np.median(v["bound"][well] / np.abs(v["cost"][well])))
    print("%s %s kind %d %s: dead %d, deficient %d, near-tie %.4f, judged %.3f, median bound / |cost| %.1e" % (
        regime, which, kind, assign, v["dead"].sum(), v["deficient"].sum(), near.sum() / float((~none).sum()), (whole & ~near & cov).mean(), rel))
    assert v["dead"].sum() == ME.DEAD_CELLS
    assert v["deficient"].sum() == ME.DEFICIENT_CELLS[(kind, which)]
    assert (near & whole).sum() == 0                                  # the share among the all-finite pixels: none at all
    assert near.sum() <= GE.NEAR_TIE_CAP * (~none).sum()              # (beside a rank-deficient cell a pixel may tie)
    assert (whole & ~near & cov).mean() > 0.8
    assert none.sum() == ME.NO_FINITE[ME.SMALL] and some.sum() == ME.SOME_NAN[ME.SMALL]
    if which == "tiny":
        np.testing.assert_array_equal(cov, ME.covered(ME.SMALL, "real"))
        assert ME.regime_mask("tiny").max() <= 2.0 ** -24 and np.array_equal(np.ldexp(ME.regime_mask("tiny"), 24), ME.masks(ME.SMALL)["real"])


@pytest.mark.parametrize("which", ME.REGIME_MASKS)
@pytest.mark.parametrize("assign", ["sam", "ref"])
def test_the_oracle_s_own_df_at_low_visibility(port_ns, which, assign):
    """At visibility 1e-3 the CPU oracle's masked dark-field model is itself further than 1e-6 from extended precision on the
    sampled well-posed cells of this stack (three frames, 5 x 5 windows), at 1e-2 it is not: the pairs on which the GPU module
    holds the device to a factor times the oracle's own error instead of the flat bar are masked_grid_expect.ORACLE_LOOSE_DF."""
    lo, n = ME.oracle_df_error(port_ns, "vis1e-3", which, assign)
    hi, _ = ME.oracle_df_error(port_ns, "vis1e-2", which, assign)
    print("%s %s: the oracle's df on %d cells: %.2e at visibility 1e-3, %.2e at 1e-2" % (which, assign, n, lo, hi))
    assert n > 1300
    assert (lo > 1e-6) == ((which, assign) in ME.ORACLE_LOOSE_DF)
    assert hi < 1e-6


BAD = ME.bad_cases()


@pytest.mark.parametrize("value,where,kind,assign,situation", BAD, ids=["%s-%s-%s-%s" % (v, w, CE.mode_id(k, a), s) for v, w, k, a, s in BAD])
def test_bad_pixels_reach_exactly_the_footprint_with_and_under_the_mask(value, where, kind, assign, situation):
    """On the pixels a bad one can reach (consumer_expect.band): a NaN / Inf makes every cell of the footprint NaN in extended
    precision, with weight 1 and with weight 0 alike (0 * NaN); off the footprint every cell is the clean volume's.  A zero
    leaves every cell with weight finite."""
    sam, ref, mask = ME.bad_inputs(value, where, kind, assign, situation)
    csam, cref, _ = ME.bad_inputs(None, where, kind, assign, situation)
    c = CE.CONFIGS["vol"]
    px = CE.band("vol")
    v = ME.hp_of(sam, ref, mask, c["Nw"], c["ms"], kind, assign, pixels=px)
    clean = ME.hp_of(csam, cref, mask, c["Nw"], c["ms"], kind, assign, pixels=px)
    foot = CE.footprint("vol", where, assign, pixels=px)
    assert foot.sum() == (3430 if where == assign else 3360)
    for (k, r, col) in CE.bad_positions("vol"):
        assert mask[k, r, col] == (1.0 if situation == "live" else 0.0)
    cost = v["cost"].astype(np.float64)
    assert np.array_equal(cost[~foot], clean["cost"].astype(np.float64)[~foot], equal_nan=True)
    np.testing.assert_array_equal(v["dead"], clean["dead"])           # the weights are the mask's alone
    if value == "zero":
        assert np.isfinite(cost[~v["dead"] & ~v["singular"]]).all()
    else:
        assert np.isnan(cost[foot]).all()                             # never +-Inf
    far = ME.bad_far()
    ii, jj = px
    assert far.mean() > 0.3 and not foot[:, :, far[ii, jj]].any()


def test_the_tie_input_ties_exactly():
    """Shifts three columns apart cost the same, bit for bit, for both models: the first strict minimum in scan order is at a
    column shift of -3 or 0, never 3, on every pixel whose minimum is finite -- what `<=` in place of `<` would turn round."""
    sam, ref, mask = ME.tie_inputs()
    c = ME.TIE
    for kind in (0, 1):
        v = ME.hp_of(sam, ref, mask, c["Nw"], c["ms"], kind, "sam")
        cost = v["cost"].astype(np.float64)
        p = c["period"]
        assert np.array_equal(cost[:, :-p], cost[:, p:], equal_nan=True) and np.array_equal(v["cost"][:, :-p], v["cost"][:, p:], equal_nan=True)
        ci, cj, cmin, found = CE.first_strict_minimum(cost)
        assert found.mean() > 0.95 and (cj[found] <= 0).all() and (cj[found] == -p).mean() > 0.5
        U = cost.shape[0]
        last = np.nanargmin(np.where(np.isnan(cost), np.inf, cost).reshape(U * U, -1)[::-1], axis=0)
        assert ((U * U - 1 - last).reshape(ci.shape) % U - (c["ms"] - 1))[found].max() > 0       # the last minimum is elsewhere


@pytest.mark.parametrize("regime,which,assign", [("x2^16", "binary", "sam"), ("vis1e-2", "real", "sam"), ("vis1e-3", "tiny", "sam"), ("zero_mean", "real", "ref")])
def test_where_the_oracle_s_df_misses_the_bar_its_own_bound_says_so(port_ns, regime, which, assign):
    """df = N_K / (N_beta + N_K) loses its relative accuracy where a numerator cancels: where df crosses zero (seen: df = -1.3e-7
    beside values of 1e-4, the oracle 1.1e-4 off at visibility 1e-2) and at low contrast.  oracle/hp_cost.py's df_bound is the
    a-priori bound of that: the CPU oracle is within it on EVERY well-posed cell, and within 1e-6 wherever it is below the
    parity bar of 1e-5 -- so the GPU module holds df to the bound everywhere and to the flat bar where the bound is below it."""
    err, bound = ME.oracle_df_all(port_ns, regime, which, assign)
    tight = bound < CE.RTOL
    print("%s %s %s: %d well-posed cells, the oracle's df: max %.2e, max / bound %.3f, %d cells with a bound above 1e-5, max on the others %.2e" % (
        regime, which, assign, err.size, err.max(), (err / bound).max(), (~tight).sum(), err[tight].max()))
    assert err.size > 140000 and np.all(err <= bound)
    assert err[tight].max() < 1e-6
    loose = (~tight).mean()
    assert loose == 0 if regime in ("x2^16", "zero_mean") else loose < (0.001 if regime == "vis1e-2" else 0.08)
    if regime == "vis1e-2":
        assert err.max() > CE.RTOL                                     # the flat bar on every cell is not the oracle's either


@pytest.mark.parametrize("regime,which,kind,assign", [("vis1e-2", "binary", 1, "sam"), ("vis1e-3", "tiny", 0, "sam"), ("zero_mean", "tiny", 1, "sam")])
def test_the_reference_s_own_newton_is_ill_posed_on_more_pixels_than_the_flat_cap(regime, which, kind, assign):
    """assert_parity waves a pixel through only where the reference's own sub-pixel Newton iteration is ill-posed, and by default
    caps their number at 0.2 % of the ok pixels.  On these regimes the reference ALONE has more than that (its own 4x4
    neighbourhoods, no implementation involved), so the GPU module takes the cap of a case from this count."""
    exp, near, whole = ME.regime_expected(regime, which, kind, assign, -1)
    c = GE.STACKS[ME.SMALL]
    judged = whole & ~near & ME.covered_of(ME.regime_mask(which), c["Nw"], c["ms"])
    n, ok = ME.illposed_count(exp, judged), int((exp["err"] == 1).sum())
    print("%s %s kind %d %s: %d of %d ok pixels ill-posed for the reference's own Newton iteration" % (regime, which, kind, assign, n, ok))
    assert 0.002 * ok < n < 0.05 * ok
