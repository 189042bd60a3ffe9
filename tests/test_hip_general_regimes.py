"""
The general shift table (libumpa_grid.so's general_table_kernel) and the consumers above it over input regimes, bad pixels and
the LDS limit, on the GPU.  The expectations are tests/general_expect.py's: extended precision with the a-priori fp64 bound
(no tolerance of this file's own), ``model.cost`` bit for bit, the consumers' numpy restatements on the device's own volume,
the unit-step volume for a stepped one.  The caps on near ties are conditions on the inputs and are checked on the CPU
(tests/test_general_regimes_cpu.py), as is the staged / fallback list the cases at the LDS limit are taken from.

  1  per regime (x 2^16, x 2^-5, counts, visibility 1e-2 and 1e-3, zero mean) on D, masked and plain, and on a 26-frame edge
     stack: every regime meets every kernel instantiation;
  2  powers of two change no bit: sam x 2^a, ref x 2^b;
  3  NaN, +Inf, -Inf and 0 in the sample and in the reference stack: a frame's interior, a workgroup seam, its first and last
     row and column; plain, under a zero mask weight, under weight 1;
  4  steps either side of the 64 KiB of LDS (general_geometry), max_shift 1 among them.
"""
import numpy as np
import pytest

import basins_expect as BE
import consumer_expect as CE
import general_expect as G
import masked_grid_expect as ME
import regimes as R
import sequence_expect as SE
import track_expect as TE

from test_hip_general_grid import GENERAL_PATH, GT, _bare, _build, _fit, _np, _path, _same, hip_ns   # noqa: F401  (hip_ns: the fixture)

pytestmark = pytest.mark.gpu

T = "tests/test_hip_general_regimes.py::"
CONSUMERS = ["masked_min_kernel<0>", "masked_min_kernel<1>", "masked_basins_kernel<0>", "masked_basins_kernel<1>",
             "masked_track_kernel<0>", "masked_track_kernel<1>", "masked_sequence_kernel<0>", "masked_sequence_kernel<1>"]
REACHES = {
    T + "test_volume_and_consumers_per_regime": GT + ["masked_volume_kernel<0>", "masked_volume_kernel<1>"] + CONSUMERS,
    T + "test_weighted_masks_against_model_cost_and_extended_precision": ["general_table_kernel<0, true>", "general_table_kernel<1, true>"] + CONSUMERS,
    T + "test_powers_of_two_change_no_bit_of_any_consumer": GT + CONSUMERS,
    T + "test_bad_pixels_reach_exactly_the_windows_that_hold_them": GT + ["masked_volume_kernel<0>", "masked_volume_kernel<1>"] + CONSUMERS[2:6],
    T + "test_steps_either_side_of_the_lds_limit": GT,
}


def _cost_at(m, a, b):
    """model.cost at every shift of output pixel (a, b): [U, U, 2 or 3]"""
    ms, pad = m.max_shift, m.padding
    return np.array([[m.cost(int(a) + pad, int(b) + pad, float(si), float(sj)) for sj in range(1 - ms, ms)] for si in range(1 - ms, ms)])


def _consumers(m, vol, cov, what, seed=31):
    """basins, the grid search, track in both modes and two steps of sequence EQUAL their restatements on the device's own
    volume; lam and trunc are on the scale of the volume's own costs"""
    subpx, ms = m.sub_pixel_mode, m.max_shift
    kind = "df" in vol
    args = (vol["cost"], vol["T"], vol.get("df"))
    b = m.basins(k=3)
    BE.assert_equal(_bare(b), BE.restate(*args, 3, subpx, fit=_fit(m)), what + ": basins")
    top = m.basins(k=1)
    g = m.match(quiet=True, search="grid")
    assert _path(m) == GENERAL_PATH
    for n in ("dx", "dy", "f", "T") + (("df",) if kind else ()):
        np.testing.assert_array_equal(g[n][cov], top[n][0][cov], err_msg=what + ": grid " + n)
    np.testing.assert_array_equal(g["err"][cov], np.maximum(top["err"][0], 0)[cov])
    s = ME.scale(vol["cost"])
    pdx, pdy = ME.prior(ms, vol["cost"].shape[2:], seed)
    for lam, radius in ((None, 2.5), (0.5 * s, 3.0)):
        t = m.track(pdx, pdy, lam=lam, radius=radius)
        want = TE.restate(*args, pdy, pdx, TE.NEAREST if lam is None else TE.PENALTY, 0.0 if lam is None else lam, radius, subpx, fit=_fit(m))
        TE.assert_equal(_bare(t), want, what + ": track lam %r" % (lam,))
    if ms >= 2:
        s0 = m.sequence(lam=0.1 * s)
        SE.assert_equal(_bare(s0), SE.restate(*args, None, 0.1 * s, None, subpx, fit=_fit(m)), what + ": sequence, no state")
        s1 = m.sequence(state=s0["state"], lam=0.1 * s, trunc=3.0 * s)
        SE.assert_equal(_bare(s1), SE.restate(*args, s0["state"], 0.1 * s, 3.0 * s, subpx, fit=_fit(m)), what + ": sequence, step 1")


def _fit_against_hp(vol, v, kind, what):
    """T within CE.RTOL of extended precision at every finite cell; df at every finite cell that admits the bar: where hp's
    a-priori relative bound of an fp64 df (oracle/hp_cost.py: df_bound, from the reference's sums alone) is itself within
    CE.RTOL.  Where a numerator of df cancels -- low visibility -- no fp64 evaluation has a relative accuracy to be held to;
    those cells are counted per case on the CPU (general_expect.DF_LOOSE, tests/test_general_regimes_cpu.py)."""
    fin = np.isfinite(v["cost"].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        rT = np.abs(vol["T"][fin] - v["T"][fin]) / np.abs(v["T"][fin])
        print("%s: T rel %.2e" % (what, rT.max()))
        assert np.all(rT <= CE.RTOL), "%s: T rel %.2e" % (what, rT.max())
        if kind:
            ok = fin & ~(v["df_bound"] > CE.RTOL)
            rdf = np.abs(vol["df"][ok] - v["df"][ok]) / np.abs(v["df"][ok])
            print("%s: df rel %.2e on %d of %d cells" % (what, rdf.max(), ok.sum(), fin.sum()))
            assert np.all(rdf <= CE.RTOL), "%s: df rel %.2e" % (what, rdf.max())
            return int(fin.sum() - ok.sum())
    return 0


# ----------------------------------------------------------------------------- 1. the regimes

@pytest.mark.parametrize("regime,stack,kind,assign,masked", G.REGIME_CASES, ids=G.REGIME_IDS)
def test_volume_and_consumers_per_regime(hip_ns, regime, stack, kind, assign, masked):
    """The volume within the a-priori fp64 bound of extended precision on the transformed inputs, T and df within CE.RTOL of
    it (_fit_against_hp); the table equal to model.cost bit for bit on the pixel sample; every consumer equal to its restatement on the device's own volume."""
    sam, ref, pos, Nw, ms, masks = G.regime_inputs(regime, stack)
    subpx = -1 if kind else 0
    m = _build(hip_ns, sam, ref, pos, Nw, ms, kind, assign, masks if masked else None, subpx)
    vol = _np(m.cost_volume(with_fit=True))
    assert _path(m) == GENERAL_PATH
    v = G.regime_hp(regime, stack, kind, assign, masked)
    what = "%s %s kind %d %s masked %d" % (regime, stack, kind, assign, masked)
    assert vol["cost"].shape == v["cost"].shape
    cov = G.covered_of([f.shape for f in sam], pos, Nw + ms, masks if masked else None)
    np.testing.assert_array_equal(vol["covered"], cov)
    worst = G.within_bound(vol["cost"], v, what)
    print("%s: max |gpu - hp| / bound %.4f" % (what, worst))
    case = G.REGIME_IDS[G.REGIME_CASES.index((regime, stack, kind, assign, masked))]
    assert _fit_against_hp(vol, v, kind, what) == G.DF_LOOSE.get(case, 0)
    xi, xj = G.D_sample() if stack == "D" else G.pixel_sample([f.shape for f in sam], pos, Nw + ms)
    keys = ("cost", "T") + (("df",) if kind else ())
    for a, b in zip(xi, xj):
        want = _cost_at(m, a, b)
        for q, k in enumerate(keys):
            np.testing.assert_array_equal(vol[k][:, :, a, b], want[:, :, q], err_msg="%s: %s at pixel (%d, %d)" % (what, k, a, b))
    _consumers(m, vol, cov, what)


@pytest.mark.parametrize("kind,assign", G.MODES, ids=["%s-%s" % ("DF" if k else "NoDF", a) for k, a in G.MODES])
def test_weighted_masks_against_model_cost_and_extended_precision(hip_ns, kind, assign):
    """D under real-valued masks, where every window element has a pair weight of its own: the volume within the a-priori
    bound, the table equal to model.cost bit for bit on the pixel sample (the table kernel forms the pair weight as
    eval_direct does: pair_weight, not pair_weight_fast -- under binary masks the two agree in every bit and no test told
    them apart), the consumers equal to their restatements."""
    sam, ref, pos, Nw, ms = G.D()
    masks = G.D_weights()
    m = _build(hip_ns, sam, ref, pos, Nw, ms, kind, assign, masks, 0)
    vol = _np(m.cost_volume(with_fit=True))
    assert _path(m) == GENERAL_PATH
    what = "D weighted kind %d %s" % (kind, assign)
    cov = G.covered_of([f.shape for f in sam], pos, Nw + ms, masks)
    np.testing.assert_array_equal(vol["covered"], cov)
    worst = G.within_bound(vol["cost"], G.D_hp_weighted(kind, assign), what)
    print("%s: max |gpu - hp| / bound %.4f" % (what, worst))
    assert _fit_against_hp(vol, G.D_hp_weighted(kind, assign), kind, what) == 0
    keys = ("cost", "T") + (("df",) if kind else ())
    for a, b in zip(*G.D_sample()):
        want = _cost_at(m, a, b)
        for q, k in enumerate(keys):
            np.testing.assert_array_equal(vol[k][:, :, a, b], want[:, :, q], err_msg="%s: %s at pixel (%d, %d)" % (what, k, a, b))
    _consumers(m, vol, cov, what)


# ----------------------------------------------------------------------------- 2. powers of two

SCALED = ("cost", "f", "total", "state", "cost0", "debug_a")          # what goes with the costs; T goes with sam / ref


def _five(m, pdx, pdy, state, lam_t, lam_s, trunc):
    out = {"grid": m.match(quiet=True, search="grid")}
    m.ROI = None
    out["volume"] = m.cost_volume(with_fit=True)
    out["basins"] = m.basins(k=5)
    out["track"] = m.track(pdx, pdy, lam=lam_t, radius=3.0)
    out["sequence"] = m.sequence(state=state, lam=lam_s, trunc=trunc)
    return {k: _np(v) for k, v in out.items()}


@pytest.mark.parametrize("kind,assign,masked", [(0, "sam", True), (0, "ref", False), (1, "ref", True), (1, "sam", False)],
                         ids=["NoDF-sam-mask", "NoDF-ref-plain", "DF-ref-mask", "DF-sam-plain"])
def test_powers_of_two_change_no_bit_of_any_consumer(hip_ns, kind, assign, masked):
    """sam x 2^a, ref x 2^b, lam and trunc x 2^(2a): dx, dy, err, shift, count and df keep their bits, every cost is 2^(2a)
    times the base's and T 2^(a - b) times -- the pair weight reads the masks alone, and every other operation on this path
    commutes with powers of two.  An absolute constant anywhere on it shows here."""
    sam, ref, pos, Nw, ms = G.D()
    masks = G.D_masks() if masked else None
    N0, N1 = G.extent_of([f.shape for f in sam], pos, Nw + ms)
    pdx, pdy = ME.prior(ms, (N0, N1), 17)
    base_m = _build(hip_ns, sam, ref, pos, Nw, ms, kind, assign, masks)
    cost = base_m.cost_volume()["cost"]
    s = ME.scale(cost)
    state = ME.state(cost, 9, special=True)
    base = _five(base_m, pdx, pdy, state, 0.5 * s, 0.1 * s, 3.0 * s)
    assert _path(base_m) == GENERAL_PATH
    assert base["sequence"]["moved"].any() and (base["track"]["found"] > 0).any() and (base["basins"]["count"] > 1).any()
    for a, b in ((16, 16), (-5, -5), (7, -3)):
        m = _build(hip_ns, [np.ldexp(f, a) for f in sam], [np.ldexp(f, b) for f in ref], pos, Nw, ms, kind, assign, masks)
        got = _five(m, pdx, pdy, np.ldexp(state, 2 * a), np.ldexp(0.5 * s, 2 * a), np.ldexp(0.1 * s, 2 * a), np.ldexp(3.0 * s, 2 * a))
        for name in base:
            assert sorted(got[name]) == sorted(base[name])
            for k, x in base[name].items():
                want = np.ldexp(x, 2 * a) if k in SCALED else np.ldexp(x, a - b) if k == "T" else x
                if k == "debug_d":
                    want = np.where(x >= 0, np.ldexp(x, 2 * a), x)    # cells outside the box stay -1
                assert np.array_equal(got[name][k], want, equal_nan=True), "2^(%d, %d) %s: %s differs on %d entries" % (
                    a, b, name, k, int((~((got[name][k] == want) | (np.isnan(got[name][k]) & np.isnan(want)))).sum()))


# ----------------------------------------------------------------------------- 3. bad pixels

SITUATIONS = ("plain", "weight0", "weight1")
BAD = [(v, w, p, k, a, SITUATIONS[(n + n // 6 + i) % 3])
       for n, (v, w, p) in enumerate((v, w, p) for v in R.BAD_VALUES for w in ("sam", "ref") for p in G.BAD_POSITIONS)
       for i, (k, a) in enumerate(((0, "sam"), (1, "ref")))]


@pytest.mark.parametrize("value,where,name,kind,assign,situation", BAD, ids=["%s-%s-%s-%s-%s-%s" % (v, w, p, "DF" if k else "NoDF", a, s)
                                                                                for v, w, p, k, a, s in BAD])
def test_bad_pixels_reach_exactly_the_windows_that_hold_them(hip_ns, value, where, name, kind, assign, situation):
    """One bad value in one frame of D.  Outside the hit set -- the entries whose window over that stack, in a frame that
    contributes to the pixel, holds it -- the volume is bit-identical to the clean one; inside it it equals model.cost bit
    for bit (NaN = NaN).  A frame's row 0 and column 0 have an EMPTY hit set: only the clamped staging loads read them.  The
    last row and column are hit at the extreme shift alone, and only by the window that moves.  Under a mask the rule is the same, whatever weight the pixel
    has: 0 x NaN is NaN.  The consumers on such a volume (basins, track) equal their restatements.

    The cross product is thinned: kind and coordinate mode go together as (no dark-field, 'sam') and (dark-field, 'ref'),
    so that each stack's window stays in one and moves in the other, and plain / weight 0 / weight 1 rotate over (value,
    stack, position, mode): each (value, stack, position) meets two of the three situations, every situation meets every
    value, every stack and every position, and (no dark-field, 'ref') and (dark-field, 'sam') do not occur here -- the regime cases and
    test_hip_general_grid.py's NaN case run those instantiations in those modes."""
    _, _, pos, Nw, ms = G.D()
    bsam, bref = G.bad_frames(value, where, name)
    masks = None if situation == "plain" else G.bad_masks(0.0 if situation == "weight0" else 1.0, name)
    csam, cref = G.D()[:2]
    clean = _np(_build(hip_ns, csam, cref, pos, Nw, ms, kind, assign, masks).cost_volume(with_fit=True))
    m = _build(hip_ns, bsam, bref, pos, Nw, ms, kind, assign, masks, subpx=0)
    got = _np(m.cost_volume(with_fit=True))
    assert _path(m) == GENERAL_PATH
    hit = G.bad_hit(where, assign, *G.BAD_POSITIONS[name])
    what = "%s in %s at %s, kind %d %s %s" % (value, where, name, kind, assign, situation)
    keys = ("cost", "T") + (("df",) if kind else ())
    for k in keys + ("covered",):
        sel = ~hit if k != "covered" else np.ones(got[k].shape, dtype=bool)
        assert np.array_equal(got[k][sel], clean[k][sel], equal_nan=True), "%s: %s differs from the clean volume outside the hit set on %d entries" % (
            what, k, int((~((got[k][sel] == clean[k][sel]) | (np.isnan(got[k][sel]) & np.isnan(clean[k][sel])))).sum()))
    moves = (where == "ref") == (assign == "sam")                     # the window over that stack moves with the shift
    if name in ("row0", "col0") or (name in ("last_row", "last_col") and not moves):
        assert not hit.any()                                          # the whole volume is the clean one, bit for bit
    else:
        assert hit.any()
        if value != "zero":
            assert not np.isfinite(got["cost"][hit]).any(), what        # NaN and Inf do not come out as numbers
        px = np.argwhere(hit.any(axis=(0, 1)))
        for a, b in px[:: max(1, len(px) // 6)]:
            want = _cost_at(m, a, b)
            for q, k in enumerate(keys):
                np.testing.assert_array_equal(got[k][:, :, a, b], want[:, :, q], err_msg="%s: %s at pixel (%d, %d)" % (what, k, a, b))
    subpx = m.sub_pixel_mode
    args = (got["cost"], got["T"], got.get("df"))
    BE.assert_equal(_bare(m.basins(k=3)), BE.restate(*args, 3, subpx, fit=_fit(m)), what + ": basins")
    pdx, pdy = ME.prior(ms, got["cost"].shape[2:], 5)
    t = m.track(pdx, pdy, lam=None, radius=2.5)
    TE.assert_equal(_bare(t), TE.restate(*args, pdy, pdx, TE.NEAREST, 0.0, 2.5, subpx, fit=_fit(m)), what + ": track")


# ----------------------------------------------------------------------------- 4. either side of the LDS limit

@pytest.mark.parametrize("case", G.LIMIT_CASES, ids=G.LIMIT_IDS)
def test_steps_either_side_of_the_lds_limit(hip_ns, case):
    """general_geometry stages the windows in LDS up to 64 KiB and goes to global memory past it.  Per row of
    general_expect.LIMIT_CASES, taken from the host sweep program's list: the step that still fits and the one that does not
    -- at Nw 1, max_shift 2 the unmasked footprints of step (4, 4) are 120 bytes past the limit -- each equal to the same
    pixels of the unit-step volume bit for bit, and that volume within the bound of extended precision.  max_shift 1: U = 1,
    every pass is one valid accumulator set and three that repeat it."""
    Nw, ms, kind, assign, masked, st, fb = case
    N1 = G.LIMIT_COLS
    sam, ref, pos, masks = G.edge_inputs(Nw, ms, 3, N1)
    m = _build(hip_ns, sam, ref, pos, Nw, ms, kind, assign, masks if masked else None)
    assert m.extent == (G.EDGE_ROWS, N1)
    full = _np(m.cost_volume(with_fit=True))
    assert _path(m) == GENERAL_PATH and full["cost"].shape[:2] == (2 * ms - 1, 2 * ms - 1)
    worst = G.within_bound(full["cost"], G.edge_hp(Nw, ms, 3, N1, kind, assign, masked), "limit")
    print("limit Nw %d ms %d kind %d %s masked %d: max |gpu - hp| / bound %.4f, %r" % (Nw, ms, kind, assign, masked, worst, G.limit_listed(case)))
    for s0, s1 in (st, fb, (1, 1)):
        roi = ((1, G.EDGE_ROWS, s0), (2, N1, s1))
        part = _np(m.cost_volume(with_fit=True, ROI=roi))
        assert _path(m) == GENERAL_PATH
        _same(part, {n: np.ascontiguousarray(a[..., slice(*roi[0]), slice(*roi[1])]) for n, a in full.items()}, "step %r" % ((s0, s1),))
