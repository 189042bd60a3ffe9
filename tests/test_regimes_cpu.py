"""
The input regimes of tests/regimes.py on the CPU: what the oracle itself does at other scales, at low contrast and around
bad pixels -- so that tests/test_hip_regimes.py holds the HIP kernels to the oracle only where the oracle can be held to
itself -- and the validation of the extended-precision cost (oracle/hp_cost.py) that the GPU module measures the table
kernels' costs against.  No GPU; `pytest -s` prints the figures (admissible set, changed-walk shares, r_ref).
"""
import os

import numpy as np
import pytest

import regimes as R
from conftest import GOLDEN, Case, assert_parity
from oracle import hp_cost

MAPS = ("err", "debug_Ncalls", "f", "T", "dx", "dy", "df", "debug_d", "debug_a")


def _same(a, b, sel=None):
    for k in MAPS:
        if k in a:
            x, y = (a[k], b[k]) if sel is None else (a[k][sel], b[k][sel])
            assert np.array_equal(x, y, equal_nan=True), k


# ----------------------------------------------------------------------------- oracle/hp_cost.py

HP_SETUPS = [("tiled_DF", "x1"), ("tiled_NoDF", "vis1e-3"), ("masked_tiny_DF", "x1"), ("masked_w_NoDF", "x2^16"), ("tiled_DF10", "vis1e-2")]


@pytest.mark.parametrize("name,regime", HP_SETUPS, ids=["%s-%s" % s for s in HP_SETUPS])
def test_hp_cost_against_mpmath(name, regime):
    """The longdouble evaluation against the same formula at 50 digits, 8 (pixel, shift) pairs per setup (40 in all):
    its error is below 2^-9 of the fp64 bound (2^-11 expected: the ratio of the two machine precisions)."""
    mpmath = pytest.importorskip("mpmath")
    cfg = R.CONFIGS[name]
    sam, ref = R.regime_stack(name, regime)
    mask = R.mask_of(name)
    S = 2 * cfg["Nw"] + 1
    win = np.multiply.outer(np.hamming(S), np.hamming(S))
    win /= win.sum()
    rng = np.random.default_rng(11)
    pad, ms = R.padding(cfg), cfg["ms"]
    n = 8
    pi, pj = rng.integers(pad, cfg["H"] - pad, n), rng.integers(pad, cfg["W"] - pad, n)
    si, sj = rng.integers(-ms + 1, ms, n), rng.integers(-ms + 1, ms, n)
    kind = 1 if cfg["df"] else 0
    hp = hp_cost.hp_cells(kind, sam, ref, win, pi, pj, si, sj, cfg["assign"], mask)
    worst = 0.0
    for q in range(n):
        c, T, df = hp_cost.mp_cost(kind, sam, ref, win, int(pi[q]), int(pj[q]), int(si[q]), int(sj[q]), cfg["assign"], mask)
        one = hp_cost.hp_cost(kind, sam, ref, win, int(pi[q]), int(pj[q]), int(si[q]), int(sj[q]), cfg["assign"], mask)
        assert one[0] == hp["cost"][q] and one[1] == hp["T"][q]
        r = abs(hp_cost.to_mp(hp["cost"][q]) - c) / hp_cost.to_mp(hp["bound"][q])
        worst = max(worst, float(r))
        assert r < 2.0 ** -9, (q, float(r))
        assert abs(hp_cost.to_mp(hp["T"][q]) - T) <= 1e-12 * abs(T)
        if df is not None:
            assert abs(hp_cost.to_mp(hp["df"][q]) - df) <= 1e-10 * abs(df)
    print("hp_cost vs mpmath %s %s: max |hp - mp| / bound = %.2e" % (name, regime, worst))


def test_hp_cost_against_the_cost_kats(port_ns):
    """F2_cost.npz (the reference's own cost(), T, v at 200 points of A_small): the recorded values and the oracle's lie
    within the fp64 bound of the extended-precision cost, and the vectorised volume holds the same numbers."""
    z = np.load(os.path.join(GOLDEN, "F2_cost.npz"))
    case = Case("A_small")
    pts = np.array([p for p in z["pts"] if abs(p[2]) < 4 and abs(p[3]) < 4])
    keep = np.array([abs(p[2]) < 4 and abs(p[3]) < 4 for p in z["pts"]])
    for mdl, kind in (("UMPAModelNoDF", 0), ("UMPAModelDF", 1)):
        for assign in ("sam", "ref"):
            m = getattr(port_ns, mdl)(case.sam, case.ref, window_size=2, max_shift=4)
            m.assign_coordinates = assign
            hp = hp_cost.hp_cells(kind, case.sam, case.ref, m.window, pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], assign)
            want = z["%s_%s" % (mdl, assign)][keep]
            got = np.array([m.cost(int(i), int(j), float(a), float(b)) for (i, j, a, b) in pts])
            for vals, tag in ((want, "recorded"), (got, "oracle")):
                r = np.abs(vals[:, 0] - hp["cost"]) / hp["bound"]
                assert r.max() < 1.0, (mdl, assign, tag, float(r.max()))
                np.testing.assert_allclose(vals[:, 1], hp["T"].astype(np.float64), rtol=1e-11)
                if kind:
                    np.testing.assert_allclose(vals[:, 2], hp["df"].astype(np.float64), rtol=1e-9)
    sam, ref = case.sam[:, :24, :26], case.ref[:, :24, :26]
    vol = hp_cost.hp_volume(1, sam, ref, m.window, 4, 6, "ref")
    assert vol.shape == (7, 7, 12, 14)
    assert vol[2, 5, 3, 4] == hp_cost.hp_cost(1, sam, ref, m.window, 9, 10, -1, 2, "ref")[0]


HP_CASES = [(n, r) for n in R.CONFIGS if R.CONFIGS[n].get("table") or n.startswith(("staged", "plain")) for r in R.HP_REGIMES]


@pytest.mark.parametrize("name,regime", HP_CASES, ids=["%s-%s" % c for c in HP_CASES])
def test_oracle_cost_against_extended_precision(port_ns, name, regime):
    """r_ref: the oracle's own distance from the extended-precision cost in units of the a-priori bound (the GPU module
    measures the kernels' in the same units on the same cells).  Not restricted to admissible cases: accuracy, not agreement."""
    sam, ref = R.regime_stack(name, regime)
    res, _ = R.run(port_ns, name, sam, ref, subpx=0)
    st = R.against_hp(name, {"oracle": res}, sam, ref)["oracle"]
    print("r_ref %-17s %-8s %6d cells (lattice %d): |oracle - hp| / bound %.4f, relative %.1e, T %.1e, df %.1e" % (
        name, regime, st["cells"], st["lattice"], st["ratio"], st["rel"], st["T_rel"], st.get("df_rel", 0.0)))
    assert st["cells"] > 3000
    assert st["ratio"] < 1.0
    assert st["T_rel"] < 1e-5 and st.get("df_rel", 0.0) < 1e-5


# ----------------------------------------------------------------------------- admissibility of the sweep

def _against_itself(port_ns, name, regime):
    cfg = R.CONFIGS[name]
    sam, ref = R.regime_stack(name, regime)
    a, _ = R.run(port_ns, name, sam, ref)
    b, _ = R.run(port_ns, name, sam, ref, permute=True)
    return assert_parity(a, b, cfg["ms"], "admissible %s %s" % (name, regime), allow_illposed=R.illposed_share(cfg))


SWEEP = R.sweep_cases()


@pytest.mark.parametrize("name,regime", SWEEP, ids=["%s-%s" % c for c in SWEEP])
def test_sweep_case_is_admissible(port_ns, name, regime):
    """The oracle on the stack and on a frame permutation of it (another summation order, nothing else) meets the parity
    bar against itself: only then can a kernel that sums in yet another order be held to it."""
    st = _against_itself(port_ns, name, regime)
    print("admissible %-17s %-9s ok %5d unconverged-Newton %d" % (name, regime, st["ok"], st["unconverged"]))
    assert st["ok"] > 500


@pytest.mark.parametrize("name,regime", sorted(R.INADMISSIBLE) + R.BEYOND_FP64)
def test_excluded_case_fails_the_bar_against_itself(port_ns, name, regime):
    """Why these cases are in no GPU sweep: the reference does not reproduce ITSELF to 1e-5 under a frame permutation --
    the expanded sums cancel by 1 / visibility^2 and the classifier of oracle/parity.py (a 1e-14 perturbation) does not see
    the 1e-9 noise that leaves.  A classifier that learns to will turn this test over: move the case into the sweep then."""
    with pytest.raises(AssertionError, match="misses the 1e-5 bar|max rel"):
        _against_itself(port_ns, name, regime)


# ----------------------------------------------------------------------------- scales

@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_oracle_is_exactly_scale_covariant(port_ns, name):
    """Powers of two commute with every operation of the cost and of the fits: 2^e (sam, ref) gives the same maps bit for
    bit and f times 4^e; 2^7 sam alone gives T times 128.  (Upwards only: downwards the absolute tie tolerance bites.)"""
    sam, ref = R.base_stack(name)
    base, _ = R.run(port_ns, name, sam, ref)
    for e in (4, 16):
        got, _ = R.run(port_ns, name, *R.scaled(sam, ref, e, e))
        for k in ("err", "debug_Ncalls", "dx", "dy", "T", "df"):
            if k in base:
                assert np.array_equal(got[k], base[k], equal_nan=True), (e, k)
        assert np.array_equal(got["f"], np.ldexp(base["f"], 2 * e)), e
    got, _ = R.run(port_ns, name, *R.scaled(sam, ref, 7, 0))
    for k in ("err", "debug_Ncalls", "dx", "dy", "df"):
        if k in base:
            assert np.array_equal(got[k], base[k], equal_nan=True), k
    assert np.array_equal(got["T"], base["T"] * 128.0)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_tie_factors_are_in_the_tie_regime(port_ns, name):
    """At the two scale factors of the tie-rule regime the absolute tolerance of 1e-8 decides walks (5 % .. 95 % of the
    pixels walk differently from scale 1) while at least 5 % still converge -- below about 2^-10 nothing does."""
    sam, ref = R.base_stack(name)
    base, _ = R.run(port_ns, name, sam, ref)
    for (e, m) in R.CONFIGS[name]["tie"]:
        got, _ = R.run(port_ns, name, *R.tie_scaled(sam, ref, e, m))
        changed = ((got["err"] != base["err"]) | (got["debug_Ncalls"] != base["debug_Ncalls"])).mean()
        ok = (got["err"] == 1).mean()
        print("tie %-17s %.2f * 2^%d: %.1f %% of the walks changed, %.1f %% converge" % (name, m, e, 100 * changed, 100 * ok))
        assert 0.05 < changed < 0.95 and ok >= 0.05


# ----------------------------------------------------------------------------- bad pixels

BAD = [(n, k, w) for n in R.CONFIGS for k in R.BAD_VALUES for w in ("sam", "ref")]
AGREEMENT = np.load(os.path.join(GOLDEN, "bad_pixel_agreement.npz"))        # tools/record_bad_pixel_agreement.py


@pytest.mark.parametrize("name,kind,where", BAD, ids=["%s-%s-%s" % c for c in BAD])
def test_bad_pixels_stay_local_in_the_oracle(port_ns, name, kind, where):
    """A NaN / Inf / 0 pixel changes nothing further than Nw + max_shift away, and every walk ends (R.NCALLS_MAX).
    Where oracle/_ref is built, the in-place build of the reference is compared as well: on a 0 (finite data) the two checkers
    meet the full bar everywhere; on NaN / Inf with the bad pixel in the stack whose window STAYS at the pixel ('sam' with
    assign_coordinates 'sam', 'ref' with 'ref': every cost of a touched pixel is NaN, the walk ends at once) they agree on
    every pixel in reach, as recorded in tests/golden/bad_pixel_agreement.npz; with the bad pixel in the stack whose window
    MOVES with the shift (only some shifts cost NaN) the reference never returns -- all 51 such cases of the 17 configurations,
    listed under "hangs" in that file (tools/record_bad_pixel_agreement.py runs each in a child under a time limit) -- its
    centre steps between two memoised cells for ever, see UMPA_MOVE_CAP, and only the plain-C oracle is run."""
    cfg = R.CONFIGS[name]
    sam, ref = R.base_stack(name)
    pos = R.bad_positions(cfg)
    clean, _ = R.run(port_ns, name, sam, ref)
    dirty, _ = R.run(port_ns, name, *R.bad_pixels(sam, ref, kind, where, pos))
    far = R.far_from(cfg, pos, clean["err"].shape)
    assert far.mean() > 0.9
    _same(clean, dirty, far)
    assert dirty["debug_Ncalls"].max() <= R.NCALLS_MAX and set(np.unique(dirty["err"])) <= {0, 1}
    changed = (clean["T"] != dirty["T"]) & ~(np.isnan(clean["T"]) & np.isnan(dirty["T"]))
    assert changed.any() and not (changed & far).any()
    from oracle import cpu_model
    key = R.bad_key(name, kind, where)
    assert kind == "zero" or key in AGREEMENT.files or key in AGREEMENT["hangs"], key + " is not recorded"
    if not cpu_model.have_ref() or key in AGREEMENT["hangs"]:
        return
    other, _ = R.run(cpu_model.ref, name, *R.bad_pixels(sam, ref, kind, where, pos))
    if kind == "zero":                                                # finite data: the two checkers at the full bar, everywhere
        assert_parity(dirty, other, cfg["ms"], "checkers " + key, allow_illposed=R.illposed_share(cfg))
        return
    agree = R.checkers_agree(dirty, other)
    print("checkers agree on %d of %d pixels in reach (%s)" % (agree[~far].sum(), (~far).sum(), key))
    assert agree[far].all()
    assert np.array_equal(np.packbits(agree), AGREEMENT[key]), "tests/golden/bad_pixel_agreement.npz is out of date for " + key


@pytest.mark.parametrize("name", [n for n in R.CONFIGS if R.CONFIGS[n].get("mask")])
def test_zero_mask_does_not_hide_a_nan(port_ns, name):
    """Reference behaviour, pinned as observed: the pair weight of a pixel with mask 0 is 0, and 0 * NaN is NaN -- the windows
    that hold the pixel still answer NaN.  (A mask value of 0 on a FINITE pixel does what a mask is for; far pixels are
    untouched either way.)"""
    cfg = R.CONFIGS[name]
    sam, ref = R.base_stack(name)
    pos = R.bad_positions(cfg)
    mask = R.mask_of(name).copy()
    for (k, r, c) in pos:
        mask[k, r, c] = 0.0
    clean, _ = R.run(port_ns, name, sam, ref, mask=mask)
    dirty, _ = R.run(port_ns, name, *R.bad_pixels(sam, ref, "nan", "sam", pos), mask=mask)
    far = R.far_from(cfg, pos, clean["err"].shape)
    _same(clean, dirty, far)
    assert np.isnan(dirty["T"]).sum() > np.isnan(clean["T"]).sum() and not np.isnan(dirty["T"][far]).any()


@pytest.mark.parametrize("name", ["masked_tiny_DF", "masked_tiny_NoDF"])
def test_the_pair_weights_constant_matters_under_a_tiny_mask(port_ns, name):
    """The "tiny" mask is the "weights" mask times 2^-24 exactly.  Without the 1e-8 of a b / (a + b + 1e-8) the two would
    give the same maps (the cost is a ratio of mask-weighted sums); with it, mask values of 6e-8 are comparable to the constant:
    same stack, same configuration, the two masks -- T moves by more than 1 % somewhere and some walks change."""
    sam, ref = R.base_stack(name)
    tiny = R.mask_of(name)
    order1 = np.ldexp(tiny, 24)
    assert np.array_equal(order1, R.mask_of(name.replace("tiny", "w")))
    a, _ = R.run(port_ns, name, sam, ref, mask=tiny)
    b, _ = R.run(port_ns, name, sam, ref, mask=order1)
    ok = (a["err"] == 1) & (b["err"] == 1)
    rel = np.abs(a["T"] - b["T"])[ok] / np.abs(b["T"][ok])
    walks = (a["debug_Ncalls"] != b["debug_Ncalls"]).sum()
    print("%s: T differs by up to %.1f %%, %d walks differ" % (name, 100 * rel.max(), walks))
    assert rel.max() > 0.01 and walks >= 5
