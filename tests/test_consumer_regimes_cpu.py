"""
The input regimes of tests/consumer_expect.py on the CPU: every condition tests/test_hip_consumer_regimes.py relies on, shown
on the reference side alone -- the extended-precision volumes (oracle/hp_cost.py), the plain-C oracle and the numpy
restatements.  No GPU; `pytest -s` prints the near-tie shares, the oracle's own errors and the restatement's deviations.

  * the near-tie share of every (configuration, regime, model, coordinate mode) is within grid_expect.NEAR_TIE_CAP, so the
    integer minimum is decided by the reference on all but that share of the pixels;
  * a NaN / +Inf / -Inf pixel makes the extended-precision volume non-finite (NaN, never +-Inf) on exactly the geometric
    footprint; a 0 leaves every cell finite;
  * the oracle's own cost() lies within the a-priori bound on the sampled cells, and the (regime, quantity) pairs on which its
    T or df is further than 1e-6 from extended precision are the pinned consumer_expect.ORACLE_LOOSE;
  * the fp64 restatement of the uncertainty solve against the same source text in longdouble on longdouble moments;
  * what a sub_pixel_mode-0 KernelSearch must return, on the CPU oracle.
"""
import numpy as np
import pytest

import consumer_expect as CE
import grid_expect as GE
import regimes as R
import sigma_expect as SE

VOL_CASES = [(r, k, a) for r in ["x1"] + CE.REGIMES for (k, a) in CE.MODES]
MARCH_CASES = [(r, k, a) for r in CE.REGIMES for (k, a) in CE.MARCH_MODES]


def _ids(cases):
    return ["%s-%s" % (c[0], CE.mode_id(*c[1:])) for c in cases]


# ----------------------------------------------------------------------------- near ties, the oracle's own accuracy

def _near_tie_and_oracle(port_ns, cfg_name, regime, kind, assign):
    sam, ref, c = CE.regime_stack(cfg_name, regime)
    hp = CE.hp_regime(cfg_name, regime, kind, assign)
    assert np.isfinite(hp["cost"].astype(np.float64)).all() and (hp["bound"] > 0).all()
    near = GE.near_tie(hp["cost"], hp["bound"])
    U = 2 * c["ms"] - 1
    arg = np.argmin(hp["cost"].reshape((U * U,) + near.shape), axis=0)
    inside = (np.abs(arg // U - (c["ms"] - 1)) < c["ms"] - 1) & (np.abs(arg % U - (c["ms"] - 1)) < c["ms"] - 1)
    flat = CE.sample_cells(cfg_name)[0]
    err = CE.cell_errors(CE.oracle_cells(port_ns, cfg_name, sam, ref, kind, assign), hp, flat)
    print("%-5s %-9s %-8s near-tie %.4f %% of %d pixels, minimum inside the box %.0f %%; oracle on %d cells: |cost - hp| / bound %.3f, T %.1e%s" % (
        cfg_name, regime, CE.mode_id(kind, assign), 100.0 * near.mean(), near.size, 100.0 * inside.mean(), flat.size, err["ratio"], err["T"],
        ", df %.1e" % err["df"] if kind else ""))
    assert near.mean() <= GE.NEAR_TIE_CAP
    assert err["ratio"] < 1.0
    loose = {q for q in ("T", "df") if err.get(q, 0.0) > 1e-6}
    return loose, err


@pytest.mark.parametrize("regime,kind,assign", VOL_CASES, ids=_ids(VOL_CASES))
def test_vol_near_ties_and_the_oracle_on_sampled_cells(port_ns, regime, kind, assign):
    loose, err = _near_tie_and_oracle(port_ns, "vol", regime, kind, assign)
    assert loose == {q for (r, q) in CE.ORACLE_LOOSE if r == regime and (kind or q != "df")}, (loose, err)
    assert err["T"] <= 0.1 * CE.RTOL
    if kind:                                                          # what goes through assert_parity has a tenth of its bar to itself
        assert (err["df"] > 0.1 * CE.RTOL) == ((regime, kind) in CE.PARITY_INADMISSIBLE), err


@pytest.mark.parametrize("regime,kind,assign", MARCH_CASES, ids=_ids(MARCH_CASES))
def test_march_near_ties_and_the_oracle_on_sampled_cells(port_ns, regime, kind, assign):
    """13 x 13 windows and five frames: the same pairs as `vol` (df at visibility 1e-3: 1.6e-6)."""
    loose, err = _near_tie_and_oracle(port_ns, "march", regime, kind, assign)
    assert loose == {q for (r, q) in CE.ORACLE_LOOSE if r == regime and (kind or q != "df")}, (loose, err)


def test_the_march_lattice_meets_the_strip_seam():
    c = CE.CONFIGS["march"]
    xi, xj = CE.lattice("march")
    assert {c["seam_col"] - 1, c["seam_col"]} <= set(xj.ravel().tolist())
    assert 5000 < xi.size * (2 * c["ms"] - 1) ** 2 <= R.HP_MAX_CELLS
    xi, xj = CE.lattice("vol")
    assert xi.shape == CE.extent(CE.CONFIGS["vol"]) and CE.CONFIGS["vol"]["seam_row"] < xi.shape[0]


# ----------------------------------------------------------------------------- bad pixels: the footprint

@pytest.mark.parametrize("value,where,kind,assign", CE.BAD_CASES, ids=["%s-%s-%s" % (v, w, CE.mode_id(k, a)) for v, w, k, a in CE.BAD_CASES])
def test_vol_bad_pixels_reach_exactly_the_footprint(value, where, kind, assign):
    sam, ref, c = CE.bad_stack("vol", value, where)
    px = CE.band("vol")
    with np.errstate(invalid="ignore", over="ignore"):
        hp = GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], CE.pad(c), assign, pixels=px)
    foot = CE.footprint("vol", where, assign, pixels=px)
    whole = CE.footprint("vol", where, assign)
    assert whole.sum() == foot.sum() == (3430 if where == assign else 3360)
    dead = whole.all(axis=(0, 1))
    assert dead.sum() == (70 if where == assign else 0)
    cost = hp["cost"].astype(np.float64)
    if value == "zero":
        assert np.isfinite(cost).all() and np.isfinite(hp["T"].astype(np.float64)).all()
        return
    np.testing.assert_array_equal(~np.isfinite(cost), foot)
    assert np.isnan(cost[foot]).all()                                 # Inf - Inf: never +-Inf


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("where", ["sam", "ref"])
def test_march_bad_pixels_reach_exactly_the_footprint(value, where):
    sam, ref, c = CE.bad_stack("march", value, where)
    for kind, assign in CE.MARCH_MODES:                               # the damaged window stays in one, moves in the other
        px = CE.band("march", stride=4)
        with np.errstate(invalid="ignore", over="ignore"):
            hp = GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], CE.pad(c), assign, pixels=px)
        foot = CE.footprint("march", where, assign, pixels=px)
        assert foot.any() and not foot.all()
        cost = hp["cost"].astype(np.float64)
        np.testing.assert_array_equal(~np.isfinite(cost), foot)
        assert np.isnan(cost[foot]).all()


def test_the_rules_of_the_grid_header_on_a_hand_made_volume():
    """first_strict_minimum / grid_err_rule / neighbourhood_finite, which the GPU module judges the grid kernel's dirty results
    with, on a volume whose answers are known by construction."""
    U, ms = 7, 4                                                      # index a <-> shift a - 3
    cost = np.full((U, U, 1, 8), 5.0)
    cost[3, 3, 0, 0] = 1.0                                            # a clean interior minimum
    cost[2, 4, 0, 1] = cost[5, 1, 0, 1] = 1.0                         # a tie: the first, rows first
    cost[:, :, 0, 2] = np.nan                                         # no shift below +Inf
    cost[:, :, 0, 3] = np.inf
    cost[0, 0, 0, 4], cost[3, 3, 0, 4] = np.nan, -np.inf              # -Inf is a cost like any other
    cost[3, 3, 0, 5], cost[3, 4, 0, 5], cost[6, 6, 0, 5] = 1.0, np.nan, 0.5    # the minimum on the border of the box
    cost[5, 3, 0, 6], cost[6, 3, 0, 6] = 1.0, 2.0                     # shift (2, 0), the row below is the lower: ip = 1, rows 1 .. 4 leave the box
    cost[5, 3, 0, 7], cost[6, 3, 0, 7] = 1.0, np.nan                  # the same with a NaN there: NaN < x is false, ip = 0, rows 0 .. 3 fit
    ci, cj, cmin, found = CE.first_strict_minimum(cost)
    np.testing.assert_array_equal(found[0], [True, True, False, False, True, True, True, True])
    np.testing.assert_array_equal(ci[0][found[0]], [0, -1, 0, 3, 2, 2])
    np.testing.assert_array_equal(cj[0][found[0]], [0, 1, 0, 3, 0, 0])
    np.testing.assert_array_equal(cmin[0][found[0]], [1.0, 1.0, -np.inf, 0.5, 1.0, 1.0])
    err, ip, jp = CE.grid_err_rule(ci, cj, cost, ms)
    np.testing.assert_array_equal(err[0][found[0]], [1, 1, 1, 0, 0, 1])
    np.testing.assert_array_equal(ip[0][found[0]], [0, 0, 0, 0, 1, 0])
    np.testing.assert_array_equal(CE.neighbourhood_finite(cost, ci, cj, found)[0], [True, True, False, False, False, True, True, False])


# ----------------------------------------------------------------------------- uncertainty: fp64 against longdouble

SIGMA_CASES = [(k, r) for k in (0, 1) for r in CE.SIGMA_REGIMES]


@pytest.mark.parametrize("kind,regime", SIGMA_CASES, ids=["%s-%s" % ("DF" if k else "NoDF", r) for k, r in SIGMA_CASES])
def test_sigma_restatement_against_the_longdouble_pipeline(kind, regime):
    ld, f64, bound = CE.sigma_yardstick(kind, regime)
    assert ld["unit"].dtype == np.longdouble and f64["unit"].dtype == np.float64
    assert (ld["valid"] == 1).all() and (f64["valid"] == 1).all()
    dev, both = CE.sigma_deviation(f64, ld)
    mom = float((np.abs(f64["moments"] - ld["moments"]).astype(np.float64) / bound).max())
    print("sigma %-4s %-9s fp64 restatement against longdouble on %d pixels: unit %.1e, s2 %.1e, dof %.1e; moments %.3f of the bound" % (
        "DF" if kind else "NoDF", regime, both.sum(), dev["unit"], dev["s2"], dev["dof"], mom))
    assert mom <= 1.0
    assert max(dev.values()) <= CE.SIGMA_REF_CEILING < CE.SIGMA_CEILING


def test_sigma_solve_default_dtype_is_the_float64_solve_bit_for_bit():
    """solve(dtype=np.float64) is the default, and feeding it float64 moments as longdouble changes the type, not the pixels'
    validity."""
    _, f64, _ = CE.sigma_yardstick(1, "x1")
    c = CE.SIGMA
    sv = SE.window_sv(SE.window(c["Nw"]))
    again = SE.solve(f64["moments"], 1, c["K"], sv, dtype=np.float64)
    for k in ("unit", "s2", "dof", "valid"):
        assert again[k].dtype == f64[k].dtype
        np.testing.assert_array_equal(again[k], f64[k], err_msg=k)
    wide = SE.solve(f64["moments"], 1, c["K"], sv, dtype=np.longdouble)
    assert wide["unit"].dtype == np.longdouble
    np.testing.assert_array_equal(wide["valid"], f64["valid"])


# ----------------------------------------------------------------------------- KernelSearch with sub_pixel_mode 0

def test_mode0_search_expectation_on_the_oracle():
    """The expectation of a sub_pixel_mode-0 search (consumer_expect.mode0_expectation): every candidate's f is 0 or 1 there,
    the cost of its integer minimum is the centre of its memo, and the fold on those costs names the true kernel where the
    fold on f -- what the search returned before it ranked by the memo -- names candidates by a quadrant flag."""
    import ddf_expect as DE
    want, planes, per, on_flag = CE.recovery_mode0()
    for p, q in zip(per, planes):
        ok = p["err"] == 1
        assert set(np.unique(p["f"][ok]).tolist()) <= {0.0, 1.0}      # 1 - ip
        assert (q["f"][ok] > 0).all() and np.isfinite(q["f"][ok]).all()
    np.testing.assert_array_equal(want["index"], DE.fold_brute(planes)["index"])
    truth, far = DE.recovery_truth()
    hit, flag_hit = (want["index"] == truth)[far].mean(), (on_flag["index"] == truth)[far].mean()
    differ = int((want["index"] != on_flag["index"]).sum())
    print("mode-0 search on the oracle: the fold on the memo's centre names the true kernel on %.1f %% of the pixels away from the seam, the "
          "fold on f = 1 - ip on %.1f %%; the two differ on %d of %d pixels" % (100 * hit, 100 * flag_hit, differ, truth.size))
    assert hit > 0.9 and flag_hit < 0.5 and differ > 0.3 * truth.size
    won = want["index"] >= 0
    picked = np.take_along_axis(np.stack([q["f"] for q in planes]), np.where(won, want["index"], 0)[None], axis=0)[0]
    np.testing.assert_array_equal(want["f"][won], picked[won])
