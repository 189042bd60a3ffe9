"""
Everything that reads the exhaustive shift table besides the walk, at the input regimes of tests/regimes.py, on the GPU:
search='grid' and cost_volume() (libumpa_grid.so), aggregate / match_smooth on a real volume (libumpa_smooth.so), the
uncertainty maps (libumpa_sigma.so) and KernelSearch (libumpa_ddf.so plus the fold).  tests/consumer_expect.py has the
configurations (`vol`: every cell of a 52 x 60 x 49 volume with a tile seam; `march`: corr_march's strip table on a lattice), the
footprint of a bad pixel and the rules of include/umpa_grid.h restated; tests/test_consumer_regimes_cpu.py shows every
condition used here on the reference side alone.

  a. per regime: the volume within the a-priori bound of oracle/hp_cost.py on every cell, T and df within 1e-5 -- except df on
     consumer_expect.ORACLE_LOOSE, where the oracle itself is further than 1e-6 from extended precision: there at most F times
     the oracle's own largest error on the same sampled cells; the grid search's integer minimum, err, Ncalls and quadrant
     off the near-tie pixels; sub-pixel modes -1 and 1 at the parity bar.
  b. powers of two change no bit of any consumer's result.
  c. NaN, +Inf, -Inf and 0 pixels on the seams of both configurations: the volume is non-finite on exactly the footprint and bit-identical elsewhere;
     the grid search is what include/umpa_grid.h says of its own dirty volume at every pixel; aggregate EQUALS the
     restatement; match_smooth is match(dxdy=start); the uncertainty maps are invalid on exactly the pixels that read a bad one.
  d. the uncertainty maps against the longdouble pipeline: at most G times the fp64 restatement's own deviation, never above 1e-5.
  e. KernelSearch at detector counts and at visibility 1e-2 against the search loop over the CPU oracle.
  f. KernelSearch with sub_pixel_mode 0 ranks the candidates by the cost at their integer minimum.

F and G are twice the largest r_gpu / r_ref observed on an MI355X (tests/golden/consumer_regimes_observed.json, written by a run
with UMPA_RECORD_REGIMES=<output directory>; the factor 2 because the maximum of a rounding-error sample moves with the
seed).  They stand here as constants so that a change of a threshold shows in a diff; a test ties them to the file.

91 cases, 38 s on an MI355X host.  The kernels take well under a second in all; what costs is the host side: the start of
torch (11 s, once), one longdouble volume of `vol` per case of (a) and the python loops of grid_expect.expected, one per
sub-pixel mode (0.6 s a case together).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import consumer_expect as CE
import ddf_expect as DE
import grid_expect as GE
import regimes as R
import sigma_expect as SE
import smooth_expect as SM
from conftest import GOLDEN, assert_parity

pytestmark = pytest.mark.gpu

F_FACTOR = 1.47                  # df of the volume kernels at visibility 1e-3: 0.29 .. 0.74 of the oracle's own error
G_FACTOR = 7.75                  # unit, s2, dof: 0.8 .. 1.3 of the restatement's own deviation, 3.9 for unit of the dark-field model under zero_mean
_OBSERVED_PATH = os.path.join(GOLDEN, "consumer_regimes_observed.json")
RECORD = bool(os.environ.get("UMPA_RECORD_REGIMES"))
_seen = {}
MAPS = ("err", "debug_Ncalls", "f", "T", "dx", "dy", "df", "debug_d", "debug_a")
ILLPOSED = 0.012                 # tests/test_hip_ddf.py's cap on unconverged-Newton pixels (plain model, 3 frames, Nw = 2)


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    yield model
    if RECORD and _seen:
        out = os.environ["UMPA_RECORD_REGIMES"]                       # the directory to write into
        os.makedirs(out, exist_ok=True)
        worst = {fam: max(v["r_gpu"] / v["r_ref"] for k, v in _seen.items() if k.startswith(fam)) for fam in ("df", "sigma")
                 if any(k.startswith(fam) for k in _seen)}
        json.dump(dict(max_r_gpu_over_r_ref=worst, cases=_seen), open(os.path.join(out, "consumer_regimes_observed.json"), "w"),
                  indent=1, sort_keys=True)


def _model(hip_ns, c, sam, ref, kind, assign, subpx=0):
    m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
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


def _same(a, b, sel=None, what="", keys=MAPS):
    for k in keys:
        if k in a:
            x, y = (np.asarray(a[k]), np.asarray(b[k])) if sel is None else (np.asarray(a[k])[sel], np.asarray(b[k])[sel])
            assert np.array_equal(x, y, equal_nan=True), "%s: %s differs on %d entries" % (
                what, k, int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum()))


def _rel(a, b):
    return np.abs(a - b) / np.abs(b)


# ----------------------------------------------------------------------------- a. volumes and minima per regime

A_CASES = [("vol", r, k, a) for r in CE.REGIMES for (k, a) in CE.MODES] + [("march", r, k, a) for r in CE.REGIMES for (k, a) in CE.MARCH_MODES]


@pytest.mark.parametrize("cfg_name,regime,kind,assign", A_CASES, ids=["%s-%s-%s" % (c[0], c[1], CE.mode_id(*c[2:])) for c in A_CASES])
def test_volume_and_grid_minimum_per_regime(hip_ns, port_ns, cfg_name, regime, kind, assign):
    sam, ref, c = CE.regime_stack(cfg_name, regime)
    ms, U = c["ms"], 2 * c["ms"] - 1
    m = _model(hip_ns, c, sam, ref, kind, assign, 0)
    vol, seen = _launches(m, lambda: m.cost_volume(with_fit=True))
    table = "corr_march" if cfg_name == "march" else "corr_volume"
    assert seen.get(table, 0) >= 1 and seen.get("table_consumer", 0) >= 1, seen
    N0, N1 = CE.extent(c)
    assert vol["cost"].shape == (U, U, N0, N1) and ("df" in vol) == (kind == 1)
    hp = CE.hp_regime(cfg_name, regime, kind, assign)
    xi, xj = CE.lattice(cfg_name)
    on = {k: v[:, :, xi, xj] for k, v in vol.items()}
    label = "%s %s %s" % (cfg_name, regime, CE.mode_id(kind, assign))
    # the cost: the a-priori bound, on every cell; T and df: the parity bar
    ratio = np.abs(on["cost"].astype(np.longdouble) - hp["cost"]) / hp["bound"]
    rT = _rel(on["T"], hp["T"])
    print("%s: %d cells, max |gpu - hp| / bound %.4f, T rel %.2e" % (label, ratio.size, ratio.max(), rT.max()), end="")
    assert np.all(ratio <= 1.0), "max |gpu - hp| / bound = %.4f" % ratio.max()
    assert np.all(rT <= CE.RTOL)
    if kind:
        rdf = _rel(on["df"], hp["df"])
        print(", df rel %.2e" % rdf.max(), end="")
        if (regime, "df") in CE.ORACLE_LOOSE:
            flat = CE.sample_cells(cfg_name)[0]
            r_ref = CE.cell_errors(CE.oracle_cells(port_ns, cfg_name, sam, ref, kind, assign), hp, flat)["df"]
            r_gpu = float(rdf.ravel()[flat].max())
            print(" (sampled cells: r_gpu %.2e, the oracle's r_ref %.2e, ratio %.3f)" % (r_gpu, r_ref, r_gpu / r_ref), end="")
            _seen["df " + label] = dict(r_gpu=r_gpu, r_ref=r_ref)
            assert r_ref > 1e-6
            assert r_gpu <= F_FACTOR * r_ref, "r_gpu / r_ref = %.2f, above F = %.2f" % (r_gpu / r_ref, F_FACTOR)
        else:
            assert np.all(rdf <= CE.RTOL)
    print()
    # the grid search: the first strict minimum of its own volume at every pixel ...
    got = m.match(quiet=True, search="grid")
    ci, cj, cmin, found = CE.first_strict_minimum(vol["cost"])
    assert found.all()
    np.testing.assert_array_equal(got["dy"], ci)
    np.testing.assert_array_equal(got["dx"], cj)
    np.testing.assert_array_equal(got["debug_d"][..., 12], cmin)
    np.testing.assert_array_equal(got["debug_Ncalls"], U * U)
    # ... and the extended-precision one off the near-tie pixels
    near = GE.near_tie(hp["cost"], hp["bound"])
    keep = ~near
    assert near.mean() <= GE.NEAR_TIE_CAP
    arg = np.argmin(hp["cost"].reshape((U * U,) + xi.shape), axis=0)
    np.testing.assert_array_equal(got["dy"][xi, xj][keep], (arg // U - (ms - 1))[keep])
    np.testing.assert_array_equal(got["dx"][xi, xj][keep], (arg % U - (ms - 1))[keep])
    if cfg_name != "vol":
        err, ip, _ = CE.grid_err_rule(ci, cj, vol["cost"], ms)
        np.testing.assert_array_equal(got["err"], err)             # (all 1 but under zero_mean: the stack's shifts stay below 0.6)
        return
    win = GE.window(c["Nw"])
    exp, near2 = GE.expected(kind, sam, ref, win, ms, CE.pad(c), assign, 0, volumes=hp)
    np.testing.assert_array_equal(near2, near)
    np.testing.assert_array_equal(got["err"][keep], exp["err"][keep])
    np.testing.assert_array_equal(got["debug_Ncalls"][keep], exp["debug_Ncalls"][keep])
    ok = keep & (exp["err"] == 1)
    np.testing.assert_array_equal(got["f"][ok], exp["f"][ok])        # 1 - ip: the quadrant
    assert np.array_equal(got["debug_d"][keep] < 0, exp["debug_d"][keep] < 0)
    for k in ("debug_a", "debug_d"):
        assert np.all(np.abs(got[k][keep] - exp[k][keep]) <= 1e-6 * np.abs(exp[k][keep])), k
    print("%s: %d of %d pixels near-tie, %d ok" % (label, near.sum(), near.size, exp["err"].sum()))
    assert {0, 1} <= set(np.unique(got["err"]).tolist())              # both outcomes occur (all that is asked under zero_mean)
    if regime != "zero_mean":
        assert exp["err"].mean() > 0.5
    if (regime, kind) in CE.PARITY_INADMISSIBLE:
        return
    for subpx in (-1, 1):
        m.sub_pixel_mode = subpx
        g = m.match(quiet=True, search="grid")
        e, _ = GE.expected(kind, sam, ref, win, ms, CE.pad(c), assign, subpx, volumes=hp)
        want = {k: e[k] for k in ("err", "debug_Ncalls", "dx", "dy", "f", "T", "debug_a", "debug_d") + (("df",) if kind else ())}
        g = {k: np.array(g[k]) for k in want}
        for k in want:                                                # near-tie pixels: out of both sides
            g[k][near] = want[k][near]
        assert_parity(g, want, ms, "consumer %s subpx %d" % (label, subpx), allow_illposed=ILLPOSED, subpx=subpx)


# ----------------------------------------------------------------------------- b. exact covariance

def _scaled_maps(base, e2, eT=0):
    """What a result must be bit for bit when every cost is 2^e2 times the base's (and T 2^eT times)."""
    want = dict(base)
    want["f"] = np.ldexp(base["f"], e2)
    want["debug_d"] = np.where(base["debug_d"] >= 0, np.ldexp(base["debug_d"], e2), base["debug_d"])    # cells outside the box stay -1
    want["debug_a"] = np.ldexp(base["debug_a"], e2)
    want["T"] = np.ldexp(base["T"], eT)
    return want


# the powers of two the planes of include/umpa_sigma.h take when sam is scaled by 2^es and ref by 2^er: S, V, MM, NM hold
# two reference factors, P and AM one of each, QQ two sample factors
def _moment_powers(kind, es, er):
    p = [2 * er] * 12 + [es + er] * 3 + [2 * es]
    if kind:
        p += [2 * er] * 15 + [es + er] * 3
    return np.array(p).reshape(-1, 1, 1)


SCALES = [(16, 16), (7, 0)]                                          # (sam, ref) exponents: costs times 2^32, resp. 2^14 and T times 128


@pytest.mark.parametrize("kind,assign", CE.BAD_MODES, ids=[CE.mode_id(*c) for c in CE.BAD_MODES])
def test_power_of_two_scales_change_no_bit_of_any_consumer(hip_ns, kind, assign):
    """Every operation on these paths is a multiply, an add, an fma, a division or a comparison, all of which commute with
    powers of two: an absolute constant anywhere on them shows here."""
    from umpa_amd import sigma, smooth
    sam, ref, c = CE.base("vol")
    ms = c["ms"]
    win = GE.window(c["Nw"])
    reg = SE.full_region(sam.shape, c["Nw"], ms)

    def everything(s, r):
        m = _model(hip_ns, c, s, r, kind, assign, -1)
        out = dict(vol=m.cost_volume(with_fit=True), grid=m.match(quiet=True, search="grid"), smooth=smooth.match_smooth(m))
        return out

    base = everything(sam, ref)
    shift = sigma.shift_field(base["grid"], ms)
    assert (shift != sigma.SKIP).all(axis=0).mean() > 0.5
    base["sigma"] = sigma.region(sam, ref, win, ms, kind, reg, shift, moments=True)
    assert base["smooth"]["valid"].all() and base["smooth"]["lam"] > 0 and np.isfinite(base["smooth"]["margin"]).any()
    for es, er in SCALES:
        e2, eT = 2 * es, es - er
        what = "2^%d sam, 2^%d ref" % (es, er)
        s, r = R.scaled(sam, ref, es, er)
        got = everything(s, r)
        np.testing.assert_array_equal(got["vol"]["cost"], np.ldexp(base["vol"]["cost"], e2), err_msg=what)
        np.testing.assert_array_equal(got["vol"]["T"], np.ldexp(base["vol"]["T"], eT), err_msg=what)
        if kind:
            np.testing.assert_array_equal(got["vol"]["df"], base["vol"]["df"], err_msg=what)
        _same(got["grid"], _scaled_maps(base["grid"], e2, eT), what="grid, " + what)
        sm, sb = got["smooth"], base["smooth"]
        _same(sm, _scaled_maps(sb, e2, eT), what="match_smooth, " + what)
        for k in ("start", "valid"):
            np.testing.assert_array_equal(sm[k], sb[k], err_msg="%s %s" % (what, k))
        np.testing.assert_array_equal(sm["margin"], np.ldexp(sb["margin"], e2), err_msg=what)
        assert sm["lam"] == np.ldexp(sb["lam"], e2) and sm["trunc"] == np.ldexp(sb["trunc"], e2), (what, sm["lam"], sb["lam"])
        sg = sigma.region(s, r, win, ms, kind, reg, shift, moments=True)
        bs = base["sigma"]
        assert np.array_equal(sg["moments"], np.ldexp(bs["moments"], _moment_powers(kind, es, er)), equal_nan=True), what
        for k in ("dof", "valid"):
            assert np.array_equal(sg[k], bs[k], equal_nan=True), (what, k)
        assert np.array_equal(sg["s2"], np.ldexp(bs["s2"], 2 * es), equal_nan=True), what
        assert np.array_equal(sg["unit"], np.ldexp(bs["unit"], -2 * es), equal_nan=True), what


def test_power_of_two_scales_change_no_bit_of_the_kernel_search(hip_ns):
    from umpa_amd import ddf
    sam, ref, c = CE.base("vol")
    cand = [DE.KERNELS[0], DE.KERNELS[1], DE.KERNELS[2]]

    def search(s, r):
        ks = ddf.KernelSearch(list(s), list(r), window_size=c["Nw"], max_shift=c["ms"])
        return ks.match(cand, keep=True)

    base = search(sam, ref)
    assert len(np.unique(base["index"])) >= 3
    for es, er in SCALES:
        got = search(*R.scaled(sam, ref, es, er))
        what = "2^%d sam, 2^%d ref" % (es, er)
        for k in ("index", "a", "b", "c", "dx", "dy", "err", "err_all"):
            assert np.array_equal(got[k], base[k], equal_nan=True), (what, k)
        np.testing.assert_array_equal(got["f"], np.ldexp(base["f"], 2 * es), err_msg=what)
        np.testing.assert_array_equal(got["f_all"], np.ldexp(base["f_all"], 2 * es), err_msg=what)
        np.testing.assert_array_equal(got["T"], np.ldexp(base["T"], es - er), err_msg=what)


# ----------------------------------------------------------------------------- c. bad pixels

@functools.lru_cache(maxsize=None)
def _clean(cfg_name, kind, assign):
    """the clean stack's volume, grid result (sub_pixel_mode 0) and uncertainty on the grid result's shift field"""
    from umpa_amd import model, sigma
    sam, ref, c = CE.base(cfg_name)
    m = _model(model, c, sam, ref, kind, assign, 0)
    vol, grid = m.cost_volume(with_fit=True), m.match(quiet=True, search="grid")
    shift = sigma.shift_field(grid, c["ms"])
    sg = sigma.region(sam, ref, GE.window(c["Nw"]), c["ms"], kind, SE.full_region(sam.shape, c["Nw"], c["ms"]), shift, moments=True)
    return vol, grid, shift, sg


@functools.lru_cache(maxsize=None)
def _hp_zero(cfg_name, where, kind, assign):
    """the extended-precision volume of the stack with zeros: every pixel of `vol`, every fourth pixel around the zeros of `march`"""
    sam, ref, c = CE.bad_stack(cfg_name, "zero", where)
    px = CE.lattice("vol") if cfg_name == "vol" else CE.band("march", stride=4)
    return px, GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], CE.pad(c), assign, pixels=px)


BAD_GPU_CASES = [(n,) + case for n in ("vol", "march") for case in CE.BAD_CASES]


@pytest.mark.parametrize("cfg_name,value,where,kind,assign", BAD_GPU_CASES, ids=["%s-%s-%s-%s" % (n, v, w, CE.mode_id(k, a)) for n, v, w, k, a in BAD_GPU_CASES])
def test_bad_pixels_through_every_consumer(hip_ns, cfg_name, value, where, kind, assign):
    """Bad pixels in the interior, on the tile seam (`vol`) resp. the strip seam (`march`), inside the padding border and in the
    last frame.  On `march` every shift of the stack is below 0.6, so the 5x5 around a minimum is the whole search box."""
    from umpa_amd import sigma, smooth
    sam, ref, c = CE.bad_stack(cfg_name, value, where)
    ms, U = c["ms"], 2 * c["ms"] - 1
    N0, N1 = CE.extent(c)
    cvol, cgrid, cshift, csig = _clean(cfg_name, kind, assign)
    foot = CE.footprint(cfg_name, where, assign, pixels=np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij"))
    m = _model(hip_ns, c, sam, ref, kind, assign, 0)
    what = "%s: %s in %s, %s" % (cfg_name, value, where, CE.mode_id(kind, assign))

    # -- the volume
    vol = m.cost_volume(with_fit=True)
    keys = ("cost", "T") + (("df",) if kind else ())
    for k in keys:
        assert np.array_equal(vol[k][~foot], cvol[k][~foot]), "%s: %s differs from the clean volume off the footprint" % (what, k)
    if value == "zero":
        (xi, xj), hp = _hp_zero(cfg_name, where, kind, assign)
        ratio = np.abs(vol["cost"][:, :, xi, xj].astype(np.longdouble) - hp["cost"]) / hp["bound"]
        assert np.all(ratio <= 1.0), "%s: max |gpu - hp| / bound = %.4f" % (what, ratio.max())
        assert np.all(_rel(vol["T"][:, :, xi, xj], hp["T"]) <= CE.RTOL) and (not kind or np.all(_rel(vol["df"][:, :, xi, xj], hp["df"]) <= CE.RTOL))
        assert (vol["cost"][foot] != cvol["cost"][foot]).mean() > 0.9
        dirty = np.zeros_like(foot)
    else:
        np.testing.assert_array_equal(~np.isfinite(vol["cost"]), foot, err_msg=what)
        dirty = foot
    touched = foot.any(axis=(0, 1))

    # -- the grid search on its own dirty volume: what include/umpa_grid.h says, at every pixel
    got = m.match(quiet=True, search="grid")
    ci, cj, cmin, found = CE.first_strict_minimum(vol["cost"])
    dead = dirty.all(axis=(0, 1))
    np.testing.assert_array_equal(~found, dead)
    # (`march`: a 13 x 13 window that moves by at most 2 keeps a bad pixel within 4 of its centre, so pixels without a finite
    #  shift occur there in the "moves" cases too)
    assert cfg_name != "vol" or dead.sum() == (70 if where == assign and value != "zero" else 0)
    assert value == "zero" or where != assign or dead.sum() > 0
    np.testing.assert_array_equal(got["debug_Ncalls"], U * U)
    np.testing.assert_array_equal(got["dy"][found], ci[found])
    np.testing.assert_array_equal(got["dx"][found], cj[found])
    np.testing.assert_array_equal(got["debug_d"][..., 12][found], cmin[found])
    assert set(np.unique(got["err"]).tolist()) <= {0, 1}
    for k in ("f", "T", "dx", "dy", "df", "err"):                     # no shift below +Inf: err 0, zero maps, the memo -1
        if k in got:
            assert (got[k][dead] == 0).all(), (what, k)
    assert (got["debug_d"][dead] == -1).all() and (got["debug_a"][dead] == 0).all()
    _same(got, cgrid, sel=~touched, what=what + ", pixels no footprint cell belongs to")
    err, ip, jp = CE.grid_err_rule(ci, cj, vol["cost"], ms)
    np.testing.assert_array_equal(got["err"][found], err[found])      # the range rule alone, NaN neighbours or not
    # pixels whose whole 5x5 is finite: the full comparison, against the volume's own cells
    full = CE.neighbourhood_finite(vol["cost"], ci, cj, found)
    if value == "zero":
        assert full.all() and touched.sum() >= 70
    elif where == assign:                                             # the window stays: a pixel is clean or has no finite shift
        np.testing.assert_array_equal(touched, dead)
    else:                                                             # the window moves: both kinds of neighbourhood occur
        assert (found & ~full).sum() > 20 and (cfg_name != "vol" or (full & touched).sum() > 50), ((full & touched).sum(), (found & ~full).sum())
    ii, jj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    pick = lambda a: a[ci + ms - 1, cj + ms - 1, ii, jj]
    np.testing.assert_array_equal(got["T"][found], pick(vol["T"])[found])
    if kind:
        np.testing.assert_array_equal(got["df"][found], pick(vol["df"])[found])
    okf = full & (err == 1)
    np.testing.assert_array_equal(got["f"][okf], (1.0 - ip)[okf])
    np.testing.assert_array_equal(got["f"][found & (err == 0)], cmin[found & (err == 0)])
    for q in range(25):
        a, b = ci + q // 5 - 2, cj + q % 5 - 2
        inside = found & (np.abs(a) < ms) & (np.abs(b) < ms)
        cell = vol["cost"][np.clip(a, 1 - ms, ms - 1) + ms - 1, np.clip(b, 1 - ms, ms - 1) + ms - 1, ii, jj]
        assert np.array_equal(got["debug_d"][..., q][inside], cell[inside], equal_nan=True), (what, q)
        assert (got["debug_d"][..., q][~inside] == -1).all(), (what, q)
    ok1 = found & (err == 1)
    for g in range(16):                                               # the 4x4 the quadrant picked, the cells as they are
        a, b = ci + ip - 2 + g // 4, cj + jp - 2 + g % 4
        cell = vol["cost"][np.clip(a, 1 - ms, ms - 1) + ms - 1, np.clip(b, 1 - ms, ms - 1) + ms - 1, ii, jj]
        assert np.array_equal(got["debug_a"][..., g][ok1], cell[ok1], equal_nan=True), (what, g)
        assert (got["debug_a"][..., g][~ok1] == 0).all(), (what, g)

    # -- aggregate on the dirty volume EQUALS the restatement; match_smooth is match(dxdy=start)
    unit = smooth.cost_scale(cvol["cost"])
    lam, trunc = 0.5 * unit, 4.0 * unit
    agg = smooth.aggregate(vol["cost"], lam, trunc, return_total=True)
    want = SM.aggregate(vol["cost"], lam, trunc)
    for k in ("shift", "smin", "margin", "valid", "total"):
        assert np.array_equal(agg[k], want[k], equal_nan=True), (what, k)
    np.testing.assert_array_equal(agg["valid"] == 0, dead)
    m.sub_pixel_mode = -1
    sm = smooth.match_smooth(m)
    again = m.match(dxdy=(sm["start"][0], sm["start"][1]), quiet=True)
    _same(sm, again, what=what + ", match_smooth against match(dxdy=start)")
    np.testing.assert_array_equal(sm["valid"] == 0, dead)

    # -- the uncertainty maps, on the clean shift field
    reg = SE.full_region(sam.shape, c["Nw"], ms)
    win = GE.window(c["Nw"])
    sg = sigma.region(sam, ref, win, ms, kind, reg, cshift, moments=True)
    reach = CE.sigma_reach(cfg_name, where, cshift)
    assert reach.any()
    for k in ("unit", "s2", "dof", "valid", "moments"):
        assert np.array_equal(sg[k][..., ~reach], csig[k][..., ~reach], equal_nan=True), (what, k)
    solved = SE.solve(sg["moments"], kind, c["K"], SE.window_sv(win))
    for k in ("unit", "s2", "dof", "valid"):                          # the solve's own rule, a 0 included
        assert np.array_equal(sg[k], solved[k], equal_nan=True), (what, k)
    if value != "zero":
        np.testing.assert_array_equal((sg["valid"] == 0) & (csig["valid"] == 1), reach & (csig["valid"] == 1), err_msg=what)
        assert (sg["valid"][reach] == 0).all()
        assert np.isnan(sg["unit"][:, reach]).all() and np.isnan(sg["s2"][reach]).all() and np.isnan(sg["dof"][reach]).all()
    if assign == "sam":                                               # (uncertainty() takes 'sam' coordinates only)
        m.sub_pixel_mode = 0
        unc = m.uncertainty(got)
        skipped = (sigma.shift_field(got, ms) == sigma.SKIP).any(axis=0)
        assert skipped[dead].all() and not unc.valid[skipped].any()


@pytest.mark.parametrize("value", ["nan", "+inf"])
def test_bad_reference_pixels_stay_local_in_the_kernel_search(hip_ns, value):
    from umpa_amd import ddf
    sam, ref, c = CE.base("vol")
    cand = [DE.KERNELS[0], DE.KERNELS[1], DE.KERNELS[2]]
    clean = ddf.KernelSearch(list(sam), list(ref), window_size=c["Nw"], max_shift=c["ms"]).match(cand, keep=True)
    s, r, _ = CE.bad_stack("vol", value, "ref")
    got = ddf.KernelSearch(list(s), list(r), window_size=c["Nw"], max_shift=c["ms"]).match(cand, keep=True)
    padk = c["Nw"] + c["ms"] + DE.HALF
    ii, jj = np.meshgrid(np.arange(c["H"] - 2 * padk) + padk, np.arange(c["W"] - 2 * padk) + padk, indexing="ij")
    far = np.ones(ii.shape, dtype=bool)
    for (_, row, col) in CE.bad_positions("vol"):
        far &= np.maximum(np.abs(ii - row), np.abs(jj - col)) > padk
    assert far.sum() > 100 and (~far).sum() > 100
    for k in ("index", "a", "b", "c", "f", "T", "dx", "dy", "err"):
        assert np.array_equal(got[k][far], clean[k][far], equal_nan=True), (value, k)
    for k in ("f_all", "err_all"):
        assert np.array_equal(got[k][:, far], clean[k][:, far], equal_nan=True), (value, k)
    assert set(np.unique(got["err"]).tolist()) <= {0, 1} and set(np.unique(got["err_all"]).tolist()) <= {0, 1}
    assert (got["index"] >= -1).all() and (got["index"] < len(cand)).all()
    np.testing.assert_array_equal(got["err"] == 1, got["index"] >= 0)


# ----------------------------------------------------------------------------- d. uncertainty against the longdouble pipeline

D_CASES = [(k, r) for k in (0, 1) for r in CE.SIGMA_REGIMES]
SIGMA_FLOOR = 2.0 ** -50


@pytest.mark.parametrize("kind,regime", D_CASES, ids=["%s-%s" % ("DF" if k else "NoDF", r) for k, r in D_CASES])
def test_uncertainty_against_the_longdouble_pipeline(hip_ns, kind, regime):
    from umpa_amd import sigma
    c = CE.SIGMA
    sam, ref = CE.sigma_stack(kind, regime)
    ld, f64, bound = CE.sigma_yardstick(kind, regime)
    reg = SE.full_region(sam.shape, c["Nw"], c["ms"])
    got = sigma.region(sam, ref, SE.window(c["Nw"]), c["ms"], kind, reg, np.zeros((2, reg[2], reg[5]), dtype=np.int32), moments=True)
    worst = float((np.abs(got["moments"] - ld["moments"]).astype(np.float64) / bound).max())
    assert worst <= 1.0, worst
    np.testing.assert_array_equal(got["valid"], f64["valid"])
    dev, both = CE.sigma_deviation(got, ld)
    ref_dev, both_ref = CE.sigma_deviation(f64, ld)
    np.testing.assert_array_equal(both, both_ref)
    label = "sigma %s %s" % ("DF" if kind else "NoDF", regime)
    print("%s: moments %.3f of the bound; deviation from longdouble on %d pixels, gpu / restatement: unit %.1e / %.1e, s2 %.1e / %.1e, dof %.1e / %.1e" % (
        label, worst, both.sum(), dev["unit"], ref_dev["unit"], dev["s2"], ref_dev["s2"], dev["dof"], ref_dev["dof"]))
    for k in ("unit", "s2", "dof"):
        # (a deviation of a few ulp is the rounding of the result itself -- dof is K minus a trace and comes out within one ulp
        #  on either side -- and no measure of the solve: both sides count from 8 ulp)
        r_gpu, r_ref = max(dev[k], SIGMA_FLOOR), max(ref_dev[k], SIGMA_FLOOR)
        _seen["%s %s" % (label, k)] = dict(r_gpu=r_gpu, r_ref=r_ref)
        assert dev[k] <= CE.SIGMA_CEILING
        assert r_gpu <= G_FACTOR * r_ref, "%s %s: r_gpu / r_ref = %.2f, above G = %.2f" % (label, k, r_gpu / r_ref, G_FACTOR)


def test_f_and_g_are_twice_the_recorded_ratios():
    """F_FACTOR and G_FACTOR are constants of this module, so that a change of a threshold shows in a diff; they must be what the
    recorded run (tests/golden/consumer_regimes_observed.json) gives."""
    obs = json.load(open(_OBSERVED_PATH))
    cases = obs["cases"]
    want_df = {"df %s %s %s" % (n, r, CE.mode_id(1, a)) for (r, q) in CE.ORACLE_LOOSE for n, modes in (("vol", CE.MODES), ("march", CE.MARCH_MODES))
               for (k, a) in modes if k == 1}
    want_sigma = {"sigma %s %s %s" % ("DF" if k else "NoDF", r, q) for k, r in D_CASES for q in ("unit", "s2", "dof")}
    assert set(cases) == want_df | want_sigma
    for fam, const in (("df", F_FACTOR), ("sigma", G_FACTOR)):
        worst = max(v["r_gpu"] / v["r_ref"] for k, v in cases.items() if k.startswith(fam))
        assert abs(obs["max_r_gpu_over_r_ref"][fam] - worst) < 1e-12
        assert worst <= 8.0 and abs(const - 2.0 * worst) <= 0.006, (fam, worst, const)


# ----------------------------------------------------------------------------- e. KernelSearch at counts and at low visibility

@pytest.mark.parametrize("regime", ["counts200", "vis1e-2"])
def test_kernel_search_per_regime(hip_ns, regime):
    """Per candidate at the bar of test_hip_ddf.py::test_one_candidate, and folded: the index of the restatement's loop over the
    CPU oracle except where some candidate's Newton iteration is unconverged or the two lowest costs lie within the parity bar
    of each other (either may then win)."""
    from oracle import parity
    from umpa_amd import ddf
    p = DE.IDENTITY
    sam0, ref0 = DE.identity_stack()
    sam, ref = R.REGIMES[regime](sam0, ref0, p)
    cand = np.array([DE.KERNELS[0], DE.KERNELS[1], DE.KERNELS[2]])
    want, per = DE.search(sam, ref, cand, p["Nw"], p["max_shift"])
    ks = ddf.KernelSearch(list(sam), list(ref), window_size=p["Nw"], max_shift=p["max_shift"])
    ks.debug = True
    got = ks.match(cand, keep=True)
    for n, abc in enumerate(cand):
        one = ks.match([abc])
        np.testing.assert_array_equal(got["f_all"][n], one["f"])
        np.testing.assert_array_equal(got["err_all"][n], one["err"])
        st = assert_parity(one, per[n], p["max_shift"], "consumer ddf %s candidate %d" % (regime, n), allow_illposed=ILLPOSED)
        assert st["ok"] > 100
    f = np.stack([np.where(q["err"] == 1, q["f"], np.inf) for q in per])
    two = np.sort(f, axis=0)[:2]
    with np.errstate(invalid="ignore"):
        tie = (two[1] - two[0]) <= 2 * CE.RTOL * np.abs(two[1])
    differ = np.argwhere(got["index"] != want["index"])
    waved = 0
    for xi, xj in differ:
        ill = tie[xi, xj] or any(parity.newton_unconverged(q["debug_a"][xi, xj], q["debug_d"][xi, xj]) or
                                 parity.newton_unstable(q["debug_a"][xi, xj], q["debug_d"][xi, xj]) for q in per if q["err"][xi, xj] == 1)
        assert ill, "pixel (%d, %d): index %d, restatement %d; costs %r against %r" % (
            xi, xj, got["index"][xi, xj], want["index"][xi, xj], got["f_all"][:, xi, xj], [q["f"][xi, xj] for q in per])
        waved += 1
    print("kernel search %s: %d of %d pixels differ from the restatement (unconverged or tied); %d candidates win somewhere" % (
        regime, waved, want["index"].size, len(np.unique(want["index"][want["index"] >= 0]))))
    assert waved <= 0.01 * want["index"].size
    sel = (got["index"] == want["index"]) & (got["err"] == 1)
    assert sel.sum() > 100
    assert np.all(_rel(got["T"][sel], want["T"][sel]) <= CE.RTOL)


# ----------------------------------------------------------------------------- f. the mode-0 search

def test_mode0_search_ranks_by_the_cost_at_the_integer_minimum(hip_ns):
    """sub_pixel_mode 0: the plain match's f is the start offset 1 - ip, 0 or 1, and no cost.  The search must choose, per
    pixel, the candidate whose cost at its own integer minimum -- the centre of its 5x5 memo -- is the lowest, first on ties,
    and return that cost as f and f_all: consumer_expect.mode0_expectation, on the GPU's own per-candidate results bit for bit
    and on the CPU oracle's wherever the two lowest costs are further apart than rounding."""
    from umpa_amd import ddf
    sam, ref, cand = DE.recovery_case()
    p = DE.RECOVERY
    want, planes, per, _ = CE.recovery_mode0()
    ks = ddf.KernelSearch(list(sam), list(ref), window_size=p["Nw"], max_shift=p["max_shift"])
    ks.sub_pixel_mode = 0
    ks.debug = True
    got = ks.match(cand, keep=True)
    own = []
    for n, abc in enumerate(cand):
        plain = hip_ns.UMPAModelNoDF(list(sam), list(ddf.blur_frames(np.array(ref), tuple(abc))), window_size=p["Nw"], max_shift=p["max_shift"])
        plain.sub_pixel_mode = 0
        res = plain.match(ROI=DE.shifted(DE.full_roi(sam[0].shape, p["Nw"], p["max_shift"])), quiet=True)
        ok = res["err"] == 1
        assert set(np.unique(res["f"][ok]).tolist()) <= {0.0, 1.0} and (res["debug_d"][..., 12][ok] > 0).all()
        np.testing.assert_array_equal(got["err_all"][n], res["err"])
        np.testing.assert_array_equal(got["f_all"][n], res["debug_d"][..., 12], err_msg="candidate %d: f_all is not the memo's centre" % n)
        own.append(res)
    mine, _ = CE.mode0_expectation(own)
    on_flag = DE.fold(own)                                            # what ranking by f = 1 - ip gives
    print("mode-0 search: ranking by the quadrant flag differs from ranking by the memo's centre on %d of %d pixels" % (
        int((on_flag["index"] != mine["index"]).sum()), mine["index"].size))
    for k in ("index", "f", "T", "dx", "dy", "err"):
        np.testing.assert_array_equal(got[k], mine[k], err_msg=k)
    for k in ("debug_d", "debug_a", "debug_Ncalls"):
        picked = np.take_along_axis(np.stack([r[k] for r in own]), np.maximum(mine["index"], 0).reshape((1,) + mine["index"].shape + (1,) * (own[0][k].ndim - 2)), axis=0)[0]
        np.testing.assert_array_equal(got[k], picked, err_msg=k)
    # against the CPU oracle: the same winner unless the oracle's winner and the GPU's are within rounding of each other
    f = np.stack([np.where(q["err"] == 1, q["f"], np.inf) for q in planes])
    differ = np.argwhere(got["index"] != want["index"])
    for xi, xj in differ:
        a, b = got["index"][xi, xj], want["index"][xi, xj]
        assert a >= 0 and b >= 0 and abs(f[a, xi, xj] - f[b, xi, xj]) <= 1e-9 * f[b, xi, xj], (xi, xj, a, b, f[:, xi, xj])
    assert len(differ) <= 0.001 * want["index"].size
    truth, far = DE.recovery_truth()
    assert (got["index"] == truth)[far].mean() > 0.9
    # debug off: the same maps, and no debug arrays in the result
    ks.debug = False
    quiet = ks.match(cand)
    for k in ("index", "f", "T", "dx", "dy", "err"):
        np.testing.assert_array_equal(quiet[k], got[k], err_msg=k)
    assert not any(k.startswith("debug_") for k in quiet)
