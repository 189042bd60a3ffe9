"""
tests/consumer_expect.py -- TEST INFRASTRUCTURE for tests/test_consumer_regimes_cpu.py and tests/test_hip_consumer_regimes.py
(imported by both; not a conftest): the input regimes of tests/regimes.py for everything that reads the exhaustive shift
table besides the walk -- search='grid' and cost_volume() (include/umpa_grid.h), aggregate / match_smooth on a real volume,
the uncertainty maps (include/umpa_sigma.h) and KernelSearch (include/umpa_ddf.h).

The walk reads about 18 of the (2 ms - 1)^2 table entries of a pixel, the grid kernels all of them: the entries at the border
of the search box, on tile and strip seams and next to a bad pixel are judged here, at the scales and contrasts real
measurements bring.  Nothing here imports the code under test.

Configurations
  vol    grid_expect.STACKS["64x72x3"] (K 3, Nw 2, ms 4; extent 52 x 60, output row 32 is a tile seam of corr_volume): every cell
         of the volume, both models, both coordinate modes;
  march  the geometry of regimes.CONFIGS["march_DF"] (150 x 190, K 5, Nw 6, ms 3: corr_march's strip table, a strip seam at
         output column 48): a lattice of pixels, every shift of each, at most regimes.HP_MAX_CELLS cells.
"""
import functools

import numpy as np

import grid_expect as GE
import regimes as R
import sigma_expect as SE

REGIMES = ["x2^16", "x2^-5", "counts200", "vis1e-2", "vis1e-3", "zero_mean"]      # (the tie regimes belong to the walk)
CONFIGS = {
    "vol": dict(GE.STACKS["64x72x3"], seam_row=32),
    "march": dict(H=150, W=190, K=5, Nw=6, ms=3, seam_col=48),
}
MODES = [(1, "sam"), (1, "ref"), (0, "sam"), (0, "ref")]                         # (kind, assign_coordinates)
MARCH_MODES = [(1, "sam"), (0, "ref")]
# the bad-pixel cases: (kind, assign) of each -- in the first the window of a damaged sample stack stays at the pixel and that
# of a damaged reference stack moves with the shift, in the second the other way round
BAD_MODES = [(1, "sam"), (0, "ref")]
BAD_CASES = [(v, w, k, a) for v in R.BAD_VALUES for w in ("sam", "ref") for (k, a) in BAD_MODES]
RTOL = 1e-5                                                                       # the parity bar on T and df


def mode_id(kind, assign):
    return "%s-%s" % ("DF" if kind else "NoDF", assign)


@functools.lru_cache(maxsize=None)
def base(cfg_name):
    """(sam, ref, configuration) at scale 1, read-only."""
    if cfg_name == "vol":
        sam, ref, _ = GE.stack("64x72x3")
    else:
        assert {k: R.CONFIGS["march_DF"][k] for k in ("H", "W", "K", "Nw", "ms")} == {k: CONFIGS["march"][k] for k in ("H", "W", "K", "Nw", "ms")}
        sam, ref = R.base_stack("march_DF")
    sam, ref = np.ascontiguousarray(sam).copy(), np.ascontiguousarray(ref).copy()
    sam.setflags(write=False)
    ref.setflags(write=False)
    return sam, ref, CONFIGS[cfg_name]


def regime_stack(cfg_name, regime):
    sam, ref, c = base(cfg_name)
    if regime in (None, "x1"):
        return sam, ref, c
    s, r = R.REGIMES[regime](sam, ref, c)
    return s, r, c


def pad(c):
    return c["Nw"] + c["ms"]


def extent(c):
    return c["H"] - 2 * pad(c), c["W"] - 2 * pad(c)


def lattice(cfg_name):
    """(xi, xj) index arrays of the pixels judged against extended precision: every pixel of `vol`; for `march` a lattice of
    stride 9 (odd: both parities of every blocking are met) plus the two columns either side of the strip seam."""
    c = CONFIGS[cfg_name]
    N0, N1 = extent(c)
    if cfg_name == "vol":
        return np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    rows = np.arange(4, N0, 9)
    cols = np.unique(np.concatenate([np.arange(4, N1, 9), [c["seam_col"] - 1, c["seam_col"]]]))
    xi, xj = np.meshgrid(rows, cols, indexing="ij")
    assert xi.size * (2 * c["ms"] - 1) ** 2 <= R.HP_MAX_CELLS
    return xi, xj


def hp(cfg_name, sam, ref, kind, assign):
    """oracle/hp_cost.py on the configuration's lattice: cost, T, df, bound as [U, U, ...lattice] longdouble arrays."""
    c = CONFIGS[cfg_name]
    return GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], pad(c), assign, pixels=lattice(cfg_name))


@functools.lru_cache(maxsize=None)
def hp_regime(cfg_name, regime, kind, assign):
    sam, ref, _ = regime_stack(cfg_name, regime)
    return hp(cfg_name, sam, ref, kind, assign)


# ----------------------------------------------------------------------------- bad pixels

def bad_positions(cfg_name):
    c = CONFIGS[cfg_name]
    return R.bad_positions(dict(Nw=c["Nw"], ms=c["ms"], H=c["H"], W=c["W"], K=c["K"]))


def bad_stack(cfg_name, kind_of_value, where):
    sam, ref, c = base(cfg_name)
    s, r = R.bad_pixels(sam, ref, kind_of_value, where, bad_positions(cfg_name))
    return s, r, c


def footprint(cfg_name, where, assign, pixels=None):
    """[U, U, ...pixels] bool: the cells (pixel, shift) whose window of the damaged stack `where` holds a bad pixel.  With
    assign_coordinates = `where` that window stays at the pixel, otherwise it moves with the shift: the reference window of
    'sam' coordinates lies at pixel + shift, the sample window of 'ref' coordinates at pixel - shift (Model.cpp:408-421)."""
    c = CONFIGS[cfg_name]
    U, Nw, p = 2 * c["ms"] - 1, c["Nw"], pad(c)
    xi, xj = lattice(cfg_name) if pixels is None else pixels
    sh = np.arange(U) - c["ms"] + 1
    si = sh.reshape((U, 1) + (1,) * xi.ndim)
    sj = sh.reshape((1, U) + (1,) * xi.ndim)
    sign = 0 if where == assign else (1 if where == "ref" else -1)
    wi, wj = xi + p + sign * si, xj + p + sign * sj
    wi, wj = np.broadcast_to(wi, (U, U) + xi.shape), np.broadcast_to(wj, (U, U) + xi.shape)
    out = np.zeros((U, U) + xi.shape, dtype=bool)
    for (_, r, col) in bad_positions(cfg_name):
        out |= (np.abs(wi - r) <= Nw) & (np.abs(wj - col) <= Nw)
    return out


def band(cfg_name, stride=1):
    """(xi, xj) of the pixels within Nw + ms + 1 (Chebyshev) of a bad pixel, every `stride`-th: all a bad pixel reaches and one
    ring more.  (An extended-precision cell is a function of its two windows alone, so cells further away are the clean
    volume's.)"""
    c = CONFIGS[cfg_name]
    N0, N1 = extent(c)
    ii, jj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    near = np.zeros((N0, N1), dtype=bool)
    for (_, r, col) in bad_positions(cfg_name):
        near |= np.maximum(np.abs(ii + pad(c) - r), np.abs(jj + pad(c) - col)) <= pad(c) + 1
    near &= (ii % stride == 0) & (jj % stride == 0)
    return np.nonzero(near)


def sigma_reach(cfg_name, where, shift):
    """[N0, N1] bool: the pixels whose uncertainty reads a bad pixel of stack `where` given the shift field [2, N0, N1]
    (include/umpa_sigma.h): the sample window at the pixel; on the reference side the window at pixel + shift and the four
    neighbours of each of its pixels (the central differences), i.e. the window widened by one along either axis, not along both."""
    c = CONFIGS[cfg_name]
    Nw, p = c["Nw"], pad(c)
    N0, N1 = extent(c)
    ok = SE.guard(shift, c["ms"])
    ci = np.arange(N0)[:, None] + p + (np.where(ok, shift[0], 0) if where == "ref" else 0)
    cj = np.arange(N1)[None, :] + p + (np.where(ok, shift[1], 0) if where == "ref" else 0)
    out = np.zeros((N0, N1), dtype=bool)
    for (_, r, col) in bad_positions(cfg_name):
        di, dj = np.abs(ci - r), np.abs(cj - col)
        if where == "ref":
            out |= ((di <= Nw) & (dj <= Nw + 1)) | ((di <= Nw + 1) & (dj <= Nw))
        else:
            out |= (di <= Nw) & (dj <= Nw)
    return out & ok


def first_strict_minimum(cost):
    """What include/umpa_grid.h says of the integer minimum, from a [U, U, N0, N1] float64 volume as it is: walk the shifts
    rows first, a shift wins iff its cost is < the best so far, which starts at +Inf.  Returns (ci, cj, cmin, found): the row
    and column shift and the cost of the winner, and whether any shift won."""
    U = cost.shape[0]
    flat = cost.reshape((U * U,) + cost.shape[2:])
    best = np.full(flat.shape[1:], np.inf)
    arg = np.zeros(flat.shape[1:], dtype=np.int64)
    found = np.zeros(flat.shape[1:], dtype=bool)
    for l in range(U * U):
        with np.errstate(invalid="ignore"):
            take = flat[l] < best
        best = np.where(take, flat[l], best)
        arg = np.where(take, l, arg)
        found |= take
    h = (U - 1) // 2
    return arg // U - h, arg % U - h, best, found


def grid_err_rule(ci, cj, cost, ms):
    """err of include/umpa_grid.h from the integer minimum and the volume: 1 iff the minimum is not on the border of the search
    box and the 4x4 neighbourhood the quadrant rule picks (plain `<` on the four neighbours) stays inside the box."""
    h = ms - 1
    N0, N1 = ci.shape
    ii, jj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    inner = (np.abs(ci) < h) & (np.abs(cj) < h)
    a, b = np.where(inner, ci, 0) + h, np.where(inner, cj, 0) + h
    with np.errstate(invalid="ignore"):
        ip = (cost[a + 1, b, ii, jj] < cost[a - 1, b, ii, jj]).astype(np.int64)
        jp = (cost[a, b + 1, ii, jj] < cost[a, b - 1, ii, jj]).astype(np.int64)
    i0, j0 = ci + ip - 2, cj + jp - 2
    fits = (i0 > -ms) & (i0 + 3 < ms) & (j0 > -ms) & (j0 + 3 < ms)
    return (inner & fits).astype(np.int32), ip, jp


def neighbourhood_finite(cost, ci, cj, found):
    """[N0, N1] bool: every cell of the 5x5 around the minimum that lies inside the search box is finite"""
    U = cost.shape[0]
    h = (U - 1) // 2
    N0, N1 = ci.shape
    ii, jj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    ok = found.copy()
    for q in range(25):
        a, b = ci + q // 5 - 2 + h, cj + q % 5 - 2 + h
        inside = (a >= 0) & (a < U) & (b >= 0) & (b < U)
        v = cost[np.clip(a, 0, U - 1), np.clip(b, 0, U - 1), ii, jj]
        ok &= ~inside | np.isfinite(v)
    return ok


# ----------------------------------------------------------------------------- the oracle's own accuracy on sampled cells

SAMPLE = 1500


def sample_cells(cfg_name, seed=5):
    """SAMPLE random cells of the configuration's lattice: (flat indices into the [U, U, ...lattice] arrays, pi, pj, si, sj)"""
    c = CONFIGS[cfg_name]
    xi, xj = lattice(cfg_name)
    U = 2 * c["ms"] - 1
    rng = np.random.default_rng(seed)
    n = min(SAMPLE, U * U * xi.size)
    flat = np.sort(rng.choice(U * U * xi.size, size=n, replace=False))
    a, b, q = np.unravel_index(flat, (U, U, xi.size))
    return flat, xi.ravel()[q] + pad(c), xj.ravel()[q] + pad(c), a - c["ms"] + 1, b - c["ms"] + 1


def oracle_cells(ns, cfg_name, sam, ref, kind, assign):
    """The CPU oracle's cost() on sample_cells: [n, 2 or 3] (cost, T, df)"""
    c = CONFIGS[cfg_name]
    m = (ns.UMPAModelDF if kind else ns.UMPAModelNoDF)(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    m.assign_coordinates = assign
    _, pi, pj, si, sj = sample_cells(cfg_name)
    return np.array([m.cost(int(i), int(j), float(a), float(b)) for i, j, a, b in zip(pi, pj, si, sj)])


def cell_errors(vals, hpv, flat):
    """ratio = max |cost - hp| / bound and the largest relative errors of T (and df) of [n, 2 or 3] values against the
    extended-precision volumes at the flat cell indices"""
    out = {}
    cost = hpv["cost"].ravel()[flat]
    out["ratio"] = float((np.abs(vals[:, 0].astype(np.longdouble) - cost) / hpv["bound"].ravel()[flat]).max())
    out["T"] = float((np.abs(vals[:, 1] - hpv["T"].ravel()[flat]) / np.abs(hpv["T"].ravel()[flat])).max())
    if vals.shape[1] > 2:
        out["df"] = float((np.abs(vals[:, 2] - hpv["df"].ravel()[flat]) / np.abs(hpv["df"].ravel()[flat])).max())
    return out


# (regime, quantity) on which the ORACLE's own relative error of T or df exceeds 1e-6 on the sampled cells, in both
# configurations: there the GPU is held to F times the oracle's own error instead of the parity bar's 1e-5, which the
# reference itself misses on `vol` (three frames, 5 x 5 windows: 3.0e-5 with 'sam' coordinates, 1.9e-6 with 'ref'; `march`:
# 1.6e-6; regimes.INADMISSIBLE has the walk's side of the same fact).  tests/test_consumer_regimes_cpu.py pins the list.
# (At visibility 1e-2 the oracle's df is within 2.0e-7, below the threshold: there the flat bar holds.)
ORACLE_LOOSE = [("vis1e-3", "df")]
# ... and the cases of `vol` that are not put through assert_parity (sub-pixel modes -1 and 1), whose bar on df is 1e-5 flat: the
# dark-field model at visibility 1e-3, the cases in which the oracle's own df uses up more than a tenth of that bar
PARITY_INADMISSIBLE = [("vis1e-3", 1)]


# ----------------------------------------------------------------------------- uncertainty

SIGMA = dict(H=60, W=70, K=6, Nw=2, ms=3)
SIGMA_REGIMES = ["x1"] + REGIMES


@functools.lru_cache(maxsize=None)
def sigma_stack(kind, regime):
    c = SIGMA
    sam, ref = SE.stack(c["H"], c["W"], c["K"], c["ms"], kind, noise=0.0)
    if regime != "x1":
        sam, ref = R.REGIMES[regime](sam, ref, c)
    return sam, ref


@functools.lru_cache(maxsize=None)
def sigma_yardstick(kind, regime):
    """The longdouble pipeline (longdouble moments, the same solve source in longdouble) and the fp64 restatement of
    include/umpa_sigma.h on the shift-0 field: (ld, f64, moment bound); the dictionaries hold unit, s2, dof, valid, moments."""
    c = SIGMA
    sam, ref = sigma_stack(kind, regime)
    win = SE.window(c["Nw"])
    reg = SE.full_region(sam.shape, c["Nw"], c["ms"])
    shift = np.zeros((2, reg[2], reg[5]), dtype=np.int32)
    mom_ld, bound = SE.moments(sam, ref, win, c["Nw"], c["ms"], kind, reg, shift, np.longdouble)
    ld = SE.solve(mom_ld, kind, c["K"], SE.window_sv(win), dtype=np.longdouble)
    ld["moments"] = mom_ld
    f64 = SE.restated(sam, ref, win, c["Nw"], c["ms"], kind, reg, shift)
    return ld, f64, bound


def sigma_deviation(out, ld):
    """the largest relative deviations of unit, s2, dof of a solve result from the longdouble pipeline, on the pixels valid on
    both sides: (dict, the pixel mask)"""
    both = (np.asarray(out["valid"]) == 1) & (ld["valid"] == 1)
    dev = {}
    for k in ("unit", "s2", "dof"):
        a, b = np.asarray(out[k])[..., both].astype(np.longdouble), ld[k][..., both]
        dev[k] = float((np.abs(a - b) / np.abs(b)).max()) if both.any() else 0.0
    return dev, both


SIGMA_CEILING = 1e-5
SIGMA_REF_CEILING = 2.1e-6          # the fp64 restatement's own deviations stay below this (vis1e-3, dark-field: 2.0e-6)


# ----------------------------------------------------------------------------- KernelSearch, sub_pixel_mode 0

def mode0_expectation(per):
    """What a sub_pixel_mode-0 search must return, from the per-candidate results of the plain model with the memo
    (debug_d): per pixel the candidate whose cost at its own integer minimum -- the centre of the 5x5 memo -- is the lowest,
    first on ties: ddf_expect.fold fed those costs.  (The plain result's f is 1 - ip there, a quadrant flag.)"""
    import ddf_expect as DE
    planes = [dict(f=np.ascontiguousarray(p["debug_d"][..., 12]), T=p["T"], dx=p["dx"], dy=p["dy"], err=p["err"]) for p in per]
    return DE.fold(planes), planes


@functools.lru_cache(maxsize=None)
def recovery_mode0():
    """(expectation, planes, per-candidate oracle results, the fold on the quadrant flag that the search used to return)"""
    import ddf_expect as DE
    sam, ref, cand = DE.recovery_case()
    _, per = DE.search(sam, ref, cand, DE.RECOVERY["Nw"], DE.RECOVERY["max_shift"], subpx=0)
    want, planes = mode0_expectation(per)
    return want, planes, per, DE.fold(per)
