"""
tests/masked_grid_expect.py -- the inputs and expectations of the masked grid consumers (model.masked_grid, umpa_grid_set_masked),
built WITHOUT the code under test.

The stacks are tests/grid_expect.py's.  The masks, per stack, from ``numpy.random.default_rng(100 + seed)``:

  ``binary``  ``rng.random((K, H, W)) >= 0.10`` as float64: corr_masked's one-multiply pair weight;
  ``real``    ``0.2 + 0.8 * rng.random((K, H, W))``, drawn after ``binary`` from the same generator: the reciprocal + Newton one;

both with a dead block ``[:, 20:34, 24:40] = 0`` on every frame.  The expected volumes are oracle/hp_cost.py's with ``mask=``
(numpy.longdouble, with the a-priori bound of an fp64 evaluation).  A cell (pixel, shift) whose windows share no pair weight has
wt = 0 there, hence a NaN cost, T and df: `dead`.  A cell is `deficient` where the bound is not below |cost| (or is not a
number), or where fewer window pixels carry weight than the model has parameters: the window is rank-deficient -- the fit is
exact or singular, the cost is rounding noise and an fp64 evaluation may come out non-finite.
"""
import functools

import numpy as np

import grid_expect as GE

MASKS = ("binary", "real")
BLOCK = (slice(None), slice(20, 34), slice(24, 40))
CASES = [(n, w, k, a) for n in sorted(GE.STACKS) for w in MASKS for k in (0, 1) for a in ("sam", "ref")]
IDS = ["%s-%s-%s-%s" % (n, w, "DF" if k else "NoDF", a) for n, w, k, a in CASES]

# what the issue's author counted on a CPU, per stack (both kinds, both coordinate modes, both masks): pixels without any
# finite cost, pixels with a NaN at some but not all shifts
NO_FINITE = {"64x72x3": 120, "96x112x4": 80}
SOME_NAN = {"64x72x3": 168, "96x112x4": 208}


@functools.lru_cache(maxsize=None)
def masks(name):
    """{'binary': [K, H, W], 'real': [K, H, W]} float64, read-only"""
    c = GE.STACKS[name]
    rng = np.random.default_rng(100 + c["seed"])
    shape = (c["K"], c["H"], c["W"])
    binary = (rng.random(shape) >= 0.10).astype(np.float64)
    real = 0.2 + 0.8 * rng.random(shape)
    out = {}
    for key, m in (("binary", binary), ("real", real)):
        m[BLOCK] = 0.0
        m.setflags(write=False)
        out[key] = m
    return out


@functools.lru_cache(maxsize=None)
def stack(name):
    sam, ref, c = GE.stack(name)
    for a in (sam, ref):
        a.setflags(write=False)
    return sam, ref, c


def pair_count(mask, Nw, ms, assign):
    """[U, U, N0, N1] int: the window pixels, over all frames, that carry pair weight.  The pair weight of a window pixel is
    w ma mb / (ma + mb + 1e-8) with w > 0 and ma, mb >= 0 (lib/Utils.cpp:125-130): it is non-zero iff both masks are, and
    wt, their sum, is 0 iff the count is."""
    pad = ms + Nw
    _, H, W = mask.shape
    N0, N1 = H - 2 * pad, W - 2 * pad
    U, S = 2 * ms - 1, 2 * Nw + 1
    live = mask != 0
    out = np.zeros((U, U, N0, N1), dtype=np.int64)
    for a in range(U):
        for b in range(U):
            si, sj = a - ms + 1, b - ms + 1
            if assign == "ref":                                   # the reference window stays, the sample's is at (i - si, j - sj)
                si, sj = -si, -sj
            # both[y, x]: the fixed window's pixel (y, x) and the moving window's pixel (y + si, x + sj), any frame
            both = np.zeros((H, W), dtype=np.int64)
            y0, y1, x0, x1 = max(0, -si), min(H, H - si), max(0, -sj), min(W, W - sj)
            both[y0:y1, x0:x1] = (live[:, y0:y1, x0:x1] & live[:, y0 + si:y1 + si, x0 + sj:x1 + sj]).sum(axis=0)
            cs = np.zeros((H + 1, W + 1), dtype=np.int64)
            cs[1:, 1:] = both.cumsum(axis=0).cumsum(axis=1)
            top, left = pad - Nw, pad - Nw                            # the window of output pixel (0, 0) starts here
            box = (cs[top + S:top + S + N0, left + S:left + S + N1] - cs[top:top + N0, left + S:left + S + N1]
                   - cs[top + S:top + S + N0, left:left + N1] + cs[top:top + N0, left:left + N1])
            out[a, b] = box
    return out


def pair_weight_count(name, which, assign):
    c = GE.STACKS[name]
    return pair_count(masks(name)[which], c["Nw"], c["ms"], assign)


def hp_of(sam, ref, mask, Nw, ms, kind, assign, pixels=None):
    """oracle/hp_cost.hp_cells with the mask on every shift of the output pixels `pixels` = (xi, xj) (default: all of them):
    cost, T, df (None without dark-field), bound as [U, U, ...pixels] longdouble arrays, plus the bool arrays `dead` (wt = 0),
    `singular` and `deficient`, read-only."""
    from oracle import hp_cost
    pad = ms + Nw
    N0, N1 = sam.shape[1] - 2 * pad, sam.shape[2] - 2 * pad
    U = 2 * ms - 1
    if pixels is None:
        pixels = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    xi, xj = (np.asarray(v) for v in pixels)
    sh = np.arange(U) - ms + 1
    shape = (U, U) + xi.shape
    si = np.broadcast_to(sh.reshape((U, 1) + (1,) * xi.ndim), shape)
    sj = np.broadcast_to(sh.reshape((1, U) + (1,) * xi.ndim), shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = hp_cost.hp_cells(kind, sam, ref, GE.window(Nw), np.broadcast_to(xi + pad, shape), np.broadcast_to(xj + pad, shape), si, sj,
                             assign, mask=mask)
    out = {k: (v.reshape(shape) if v is not None else None) for k, v in r.items()}
    count = pair_count(mask, Nw, ms, assign)[:, :, xi, xj]
    out["dead"] = count == 0
    assert np.isnan(out["cost"][out["dead"]]).all()
    # Rank-deficient: hp's bound is not below |cost| -- or the window has fewer weighted pixels than the model has parameters
    # (T; beta and K with dark-field).  Then the normal equations are singular in exact arithmetic (one weighted pixel of the
    # dark-field model: det = t2 t3 - t6^2 = w^2 mean^2 r^2 - (w mean r)^2 = 0), hp's own numbers are the quotient of two
    # rounding residues (seen: T = 0.5, 1, 2 exactly, beside bounds of 1e-14), and its bound, which takes the solve for
    # granted, says nothing.  This is a count on the inputs, not a reading of any implementation's output.
    out["singular"] = ~out["dead"] & (count < (2 if kind == 1 else 1))
    with np.errstate(invalid="ignore"):
        out["deficient"] = ~out["dead"] & (~(out["bound"] < np.abs(out["cost"])) | out["singular"])
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hp(name, which, kind, assign):
    """hp_of on every (pixel, shift) of a stack of grid_expect.STACKS.  Computed once, read-only."""
    sam, ref, c = stack(name)
    return hp_of(sam, ref, masks(name)[which], c["Nw"], c["ms"], kind, assign)


def pixel_classes(v):
    """(no finite cost, some but not all shifts NaN, every shift finite) as [N0, N1] bool, from hp()'s volumes"""
    fin = np.isfinite(v["cost"].astype(np.float64))
    U = fin.shape[0]
    n = fin.reshape((U * U,) + fin.shape[2:]).sum(axis=0)
    return n == 0, (n > 0) & (n < U * U), n == U * U


def near_tie(v):
    """grid_expect.near_tie on the finite costs: [N0, N1] bool, False where the pixel has no finite cost.  A NaN cost is no
    candidate: it is put at +Inf with a zero bound before the two smallest are taken."""
    fin = np.isfinite(v["cost"].astype(np.float64))
    cost = np.where(fin, v["cost"], np.longdouble(np.inf))
    bound = np.where(fin, v["bound"], np.longdouble(0))
    U = cost.shape[0]
    n = fin.reshape((U * U,) + fin.shape[2:]).sum(axis=0)
    with np.errstate(invalid="ignore"):
        near = GE.near_tie(cost, bound)
    return near & (n >= 2)


def expected(name, which, kind, assign, subpx):
    """grid_expect.expected fed with the masked volumes.  Its rule reads only `<` and takes numpy's argmin for the first strict
    minimum, which holds where every shift of the pixel is finite: (maps, near-tie mask, all-finite mask)."""
    sam, ref, c = stack(name)
    return expected_of(sam, ref, c["Nw"], c["ms"], kind, assign, subpx, hp(name, which, kind, assign))


def expected_of(sam, ref, Nw, ms, kind, assign, subpx, v):
    """expected() for any stack, from hp_of's volumes `v` of every pixel"""
    _, _, whole = pixel_classes(v)
    # pixels with a NaN are judged elsewhere (the restatements on the device's own volume): give argmin finite numbers there
    fill = {k: (np.where(np.isfinite(v[k].astype(np.float64)), v[k], np.longdouble(1)) if v[k] is not None else None)
            for k in ("cost", "T", "df", "bound")}
    maps, _ = GE.expected(kind, sam, ref, GE.window(Nw), ms, ms + Nw, assign, subpx, volumes=fill)
    return maps, near_tie(v), whole


@functools.lru_cache(maxsize=None)
def expected_for(name, which, kind, assign, subpx):
    return expected(name, which, kind, assign, subpx)


def covered_of(mask, Nw, ms):
    """``coverage >= thr`` as ``match()`` forms it (model.pyx:499-529, :431): the coverage of a pixel is the sum over the frames
    of the mask at the pixel; thr = 0.1 max / Na.  [N0, N1] bool."""
    pad = ms + Nw
    cov = mask[:, pad:mask.shape[1] - pad, pad:mask.shape[2] - pad].sum(axis=0)
    return cov >= 0.1 * cov.max() / mask.shape[0]


def covered(name, which):
    c = GE.STACKS[name]
    return covered_of(masks(name)[which], c["Nw"], c["ms"])


# ============================================================================= the regimes module (test_hip_masked_grid_regimes.py)
#
# Four sets of inputs beyond the two stacks above, each shown admissible on the CPU by tests/test_masked_grid_cpu.py:
#   A. the edges of the search range (max_shift 2, 3, 6, 7, 8) and region widths across a wave edge (64, 65, 70 columns);
#   B. every corr_masked instantiation (kind x Nw 1 .. 8) at max_shift 4, where the last pass of every masked_ub is ragged;
#   C. the input regimes of tests/regimes.py on "64x72x3" with the masks binary, real and tiny (real x 2^-24);
#   D. NaN / +Inf / -Inf / 0 pixels at consumer_expect.bad_positions("vol"), with live weight, under a zero mask weight, and
#      a zero mask weight on clean data.

SMALL = "64x72x3"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def scale(cost):
    """the scale of a volume's costs (from the volume alone): the median gap between the two lowest costs of a pixel"""
    U = cost.shape[0]
    with np.errstate(invalid="ignore"):
        c = np.sort(np.where(cost < np.inf, cost, np.inf).reshape(U * U, -1), axis=0)
        gap = (c[1] - c[0])[np.isfinite(c[1])]
    return float(np.median(gap)) if gap.size else 1.0


def state(cost, seed, special=False):
    """a previous sequence state on the scale of the volume, as tests/test_hip_sequence.py::_state builds it: the volume's own
    costs rolled among the shifts plus noise; with `special`, NaN and +Inf entries, an all-NaN pixel, an all-Inf pixel and a
    -Inf entry"""
    rng = np.random.default_rng(seed)
    c = np.where(np.isfinite(cost), cost, 0.0)
    U = c.shape[0]
    prev = np.roll(c, (1 + seed % (U - 1), 1 + (seed // 3) % (U - 1)), axis=(0, 1)) + scale(cost) * rng.random(c.shape)
    if special:
        w = rng.random(prev.shape)
        prev[w < 0.05] = np.nan
        prev[(w >= 0.05) & (w < 0.08)] = np.inf
        prev[:, :, 0, 0] = np.nan
        prev[:, :, 1, 2] = np.inf
        prev[0, 1, 2, 1] = -np.inf
    return np.ascontiguousarray(prev)


def prior(ms, shape, seed):
    """(prior_dx, prior_dy) inside the search box, 5 % NaN each (a NaN prior: the data term decides)"""
    rng = np.random.default_rng(seed)
    pdx, pdy = (ms - 1) * (2 * rng.random(shape) - 1), (ms - 1) * (2 * rng.random(shape) - 1)
    pdx[rng.random(shape) < 0.05] = np.nan
    pdy[rng.random(shape) < 0.05] = np.nan
    return pdx, pdy


# ----------------------------------------------------------------------------- A. search-range edges and wave edges

EDGE_ROWS = 34
# (Nw, max_shift, region width, kind, assign_coordinates, mask, sub_pixel_mode): every (Nw, max_shift) with both kinds and both
# masks, the coordinate and sub-pixel modes spread over the cases.  70 = 64 + 6 = 32 + 32 + 6 columns cut the waves of the
# 64-lane kernels and of the half-wave sequence kernel (max_shift 7, 8); 64 and 65 are a wave exactly and a wave plus one.
EDGE_CASES = [
    (1, 2, 70, 0, "sam", "binary", -1), (1, 2, 70, 1, "ref", "real", 0),
    (2, 3, 70, 1, "sam", "binary", 1), (2, 3, 70, 0, "ref", "real", -1),
    (1, 6, 70, 0, "ref", "binary", 0), (1, 6, 70, 1, "sam", "real", 1),
    (1, 7, 70, 1, "ref", "binary", -1), (1, 7, 70, 0, "sam", "real", 0),
    (1, 8, 70, 0, "sam", "binary", 1), (1, 8, 70, 1, "ref", "real", -1),
    (2, 4, 64, 1, "sam", "real", 0), (2, 4, 64, 0, "ref", "binary", 1),
    (2, 4, 65, 0, "sam", "real", -1), (2, 4, 65, 1, "ref", "binary", 0),
]
EDGE_IDS = ["Nw%d-ms%d-w%d-%s-%s-%s-subpx%d" % (c[0], c[1], c[2], "DF" if c[3] else "NoDF", c[4], c[5], c[6]) for c in EDGE_CASES]
EDGE_BLOCK = ((12, 20), (28, 38))                                    # the dead block in output coordinates: 8 x 10 pixels


@functools.lru_cache(maxsize=None)
def edge_inputs(Nw, ms, N1):
    """(sam, ref, {'binary', 'real'}) of three frames (3 (2 Nw + 1)^2 >= 27 > 9: not the exact-fit gate's) whose region is
    EDGE_ROWS x N1 pixels; the displacement reaches the border of the search box (amplitude max_shift - 1.2), so minima on the
    border (err = 0) and inside it (err = 1) both occur from max_shift 3 on.  The masks as masks() builds them, with a dead
    block of 8 x 10 pixels."""
    from umpa_amd.synth import make_stack
    pad = Nw + ms
    H, W, K = EDGE_ROWS + 2 * pad, N1 + 2 * pad, 3
    sam, ref, _ = make_stack(H, W, K, ms, df=True, seed=400 + 10 * ms + Nw, amplitude=ms - 1.2)
    rng = np.random.default_rng(500 + 10 * ms + Nw)
    binary = (rng.random((K, H, W)) >= 0.10).astype(np.float64)
    real = 0.2 + 0.8 * rng.random((K, H, W))
    (r0, r1), (c0, c1) = EDGE_BLOCK
    for m in (binary, real):
        m[:, pad + r0:pad + r1, pad + c0:pad + c1] = 0.0
    _frozen(sam, ref, binary, real)
    return sam, ref, {"binary": binary, "real": real}


# ----------------------------------------------------------------------------- B. every corr_masked instantiation

INST_MS = 4                                                          # U = 7: 5 + 2, 3 + 3 + 1, 2 + 2 + 2 + 1 columns per pass
INST_EXTENT = (34, 70)                                               # output row 32, a tile seam of corr_masked, is in it
INST_CASES = [(kind, Nw) for kind in (0, 1) for Nw in range(1, 9)]
INST_IDS = ["%s-Nw%d" % ("DF" if k else "NoDF", Nw) for k, Nw in INST_CASES]
INST_SEAM = 32


def inst_mode(kind, Nw):
    """(assign_coordinates, mask kind) of an instantiation's case: 'sam' / 'ref' alternate, binary for even Nw, real for odd"""
    return ("sam", "ref")[(Nw + kind) % 2], ("binary", "real")[Nw % 2]


@functools.lru_cache(maxsize=None)
def inst_inputs(kind, Nw):
    """(sam, ref, mask) with the frame count of test_hip_instantiations.py::test_masked_tiled_path (10 for Nw <= 2, else 3).
    The dead block is centred on output pixel (16, 40) with half-widths Nw + 2, Nw + 3: the windows of the pixels within 2
    rows and 3 columns of the centre lie inside it, so these pixels have no weight at any shift."""
    from umpa_amd.synth import make_stack
    ms, pad = INST_MS, Nw + INST_MS
    K = 10 if Nw <= 2 else 3
    H, W = INST_EXTENT[0] + 2 * pad, INST_EXTENT[1] + 2 * pad
    sam, ref, _ = make_stack(H, W, K, ms, df=bool(kind), seed=600 + 10 * Nw + kind, amplitude=0.6 * ms, order=1)
    rng = np.random.default_rng(700 + 10 * Nw + kind)
    binary = (rng.random((K, H, W)) >= 0.10).astype(np.float64)
    real = 0.2 + 0.8 * rng.random((K, H, W))
    mask = binary if inst_mode(kind, Nw)[1] == "binary" else real
    mask[:, pad + 16 - (Nw + 2):pad + 16 + (Nw + 2) + 1, pad + 40 - (Nw + 3):pad + 40 + (Nw + 3) + 1] = 0.0
    _frozen(sam, ref, mask)
    return sam, ref, mask


def inst_pixels():
    """(xi, xj) of the pixels judged against extended precision, every shift of each (so every border cell of the search box
    of each): 34 x 70 x 49 cells are beyond regimes.HP_MAX_CELLS, so a lattice of odd strides (9 rows, 3 columns) that meets
    the dead block's centre, plus the rows on either side of the tile seam, the first and last row and column and the
    columns on either side of the wave edge."""
    import regimes as R
    N0, N1 = INST_EXTENT
    rows = np.unique(np.concatenate([np.arange(7, N0, 9), [0, INST_SEAM - 1, INST_SEAM, N0 - 1]]))
    cols = np.unique(np.concatenate([np.arange(1, N1, 3), [0, 63, 65, N1 - 1]]))
    xi, xj = np.meshgrid(rows, cols, indexing="ij")
    assert xi.size * (2 * INST_MS - 1) ** 2 <= R.HP_MAX_CELLS
    return xi, xj


@functools.lru_cache(maxsize=None)
def inst_hp(kind, Nw):
    sam, ref, mask = inst_inputs(kind, Nw)
    return hp_of(sam, ref, mask, Nw, INST_MS, kind, inst_mode(kind, Nw)[0], pixels=inst_pixels())


# ----------------------------------------------------------------------------- C. the input regimes

REGIME_MASKS = ("binary", "real", "tiny")
# 'sam' for every regime, 'ref' for the two whose costs are the smallest beside their sums
REGIME_CASES = [(r, w, k, a) for r in ("x2^16", "x2^-5", "counts200", "vis1e-2", "vis1e-3", "zero_mean") for w in REGIME_MASKS
                for k in (0, 1) for a in (("sam", "ref") if r in ("vis1e-3", "zero_mean") else ("sam",))]
REGIME_IDS = ["%s-%s-%s-%s" % (r, w, "DF" if k else "NoDF", a) for r, w, k, a in REGIME_CASES]
# what the issue's author counted on a CPU with 'sam' coordinates, the same in every regime (and found again here with 'ref'):
# dead cells, and rank-deficient cells by (kind, mask)
DEAD_CELLS = 7584
DEFICIENT_CELLS = {(0, "binary"): 14, (1, "binary"): 50, (0, "real"): 0, (1, "real"): 0, (0, "tiny"): 0, (1, "tiny"): 0}


@functools.lru_cache(maxsize=None)
def regime_mask(which):
    """masks(SMALL) plus ``tiny``: ``real`` x 2^-24, where the 1e-8 of the pair weight w ma mb / (ma + mb + 1e-8) carries
    weight (a sixth of the denominator at the smallest weights)"""
    if which != "tiny":
        return masks(SMALL)[which]
    return _frozen(np.ldexp(masks(SMALL)["real"], -24))[0]


def regime_stack(regime):
    import consumer_expect as CE
    assert GE.STACKS[SMALL] == {k: v for k, v in CE.CONFIGS["vol"].items() if k != "seam_row"}
    return CE.regime_stack("vol", regime)


@functools.lru_cache(maxsize=4)
def regime_hp(regime, which, kind, assign):
    sam, ref, c = regime_stack(regime)
    return hp_of(sam, ref, regime_mask(which), c["Nw"], c["ms"], kind, assign)


def regime_expected(regime, which, kind, assign, subpx):
    sam, ref, c = regime_stack(regime)
    return expected_of(sam, ref, c["Nw"], c["ms"], kind, assign, subpx, regime_hp(regime, which, kind, assign))


def well_posed_sample(v):
    """consumer_expect.sample_cells("vol") restricted to the well-posed cells of hp_of's volumes `v`:
    (flat indices into [U, U, N0 * N1], pi, pj, si, sj)"""
    import consumer_expect as CE
    flat, pi, pj, si, sj = CE.sample_cells("vol")
    well = (~v["dead"] & ~v["deficient"] & np.isfinite(v["cost"].astype(np.float64))).ravel()[flat]
    return flat[well], pi[well], pj[well], si[well], sj[well]


def oracle_df_error(ns, regime, which, assign):
    """The CPU oracle's masked dark-field model: the largest relative error of its cost()'s df against extended precision on
    well_posed_sample: (error, cells)"""
    sam, ref, c = regime_stack(regime)
    v = regime_hp(regime, which, 1, assign)
    flat, pi, pj, si, sj = well_posed_sample(v)
    m = ns.UMPAModelDF(sam, ref, mask_list=regime_mask(which), window_size=c["Nw"], max_shift=c["ms"])
    m.assign_coordinates = assign
    vals = np.array([m.cost(int(i), int(j), float(a), float(b)) for i, j, a, b in zip(pi, pj, si, sj)])
    want = v["df"].ravel()[flat]
    return float((np.abs(vals[:, 2] - want) / np.abs(want)).max()), flat.size


def oracle_df_all(ns, regime, which, assign):
    """The same on EVERY well-posed cell: (relative errors, their a-priori bounds hp_cost's df_bound), float64 arrays"""
    sam, ref, c = regime_stack(regime)
    v = regime_hp(regime, which, 1, assign)
    m = ns.UMPAModelDF(sam, ref, mask_list=regime_mask(which), window_size=c["Nw"], max_shift=c["ms"])
    m.assign_coordinates = assign
    pad, h = c["Nw"] + c["ms"], c["ms"] - 1
    idx = np.argwhere(~v["dead"] & ~v["deficient"])
    got = np.array([m.cost(int(i) + pad, int(j) + pad, float(a - h), float(b - h))[2] for a, b, i, j in idx])
    want = v["df"][tuple(idx.T)]
    return (np.abs(got - want) / np.abs(want)).astype(np.float64), v["df_bound"][tuple(idx.T)].astype(np.float64)


# (mask, assign) of the dark-field model at visibility 1e-3 on which the ORACLE's own df is further than 1e-6 from extended
# precision on the sampled cells (tests/test_masked_grid_cpu.py pins the list): there the device is held to DF_FACTOR times
# the oracle's own error, elsewhere to consumer_expect.RTOL
ORACLE_LOOSE_DF = [(w, a) for w in REGIME_MASKS for a in ("sam", "ref")]


# ----------------------------------------------------------------------------- D. bad pixels

BAD_MASK = {(1, "sam"): "binary", (0, "ref"): "real"}                # the mask of each of consumer_expect.BAD_MODES
SITUATIONS = ("live", "under0")                                       # a bad pixel with mask weight 1; the same under weight 0


def bad_cases():
    import consumer_expect as CE
    return [(v, w, k, a, s) for (v, w, k, a) in CE.BAD_CASES for s in SITUATIONS]


@functools.lru_cache(maxsize=None)
def bad_mask(which, weight):
    """masks(SMALL)[which] with `weight` (1 or 0) at consumer_expect.bad_positions("vol")"""
    import consumer_expect as CE
    m = masks(SMALL)[which].copy()
    for (k, r, c) in CE.bad_positions("vol"):
        m[k, r, c] = weight
    return _frozen(m)[0]


def bad_inputs(value, where, kind, assign, situation):
    """(sam, ref, mask): `value` (None: clean data) at the bad positions of stack `where`, the mask there 1 ('live') or 0"""
    import consumer_expect as CE
    sam, ref, _ = CE.bad_stack("vol", value, where) if value is not None else CE.base("vol")
    return sam, ref, bad_mask(BAD_MASK[(kind, assign)], 1.0 if situation == "live" else 0.0)


def bad_footprint(where, assign):
    import consumer_expect as CE
    N0, N1 = CE.extent(CE.CONFIGS["vol"])
    return CE.footprint("vol", where, assign, pixels=np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij"))


def bad_far():
    """[N0, N1] bool: the pixels further than Nw + max_shift from every bad pixel"""
    import consumer_expect as CE
    import regimes as R
    c = CE.CONFIGS["vol"]
    return R.far_from(dict(Nw=c["Nw"], ms=c["ms"]), CE.bad_positions("vol"), CE.extent(c))


# ----------------------------------------------------------------------------- exact ties

TIE = dict(H=46, W=94, K=3, Nw=2, ms=4, period=3)


@functools.lru_cache(maxsize=None)
def tie_inputs():
    """(sam, ref, mask) whose reference stack and mask repeat every `period` columns: with 'sam' coordinates the reference
    window and its mask move with the shift, so the shifts (si, sj) and (si, sj + period) read the same numbers in the same
    order and their costs are EQUAL, in any arithmetic.  The sample is 0.8 ref plus noise of its own: the minimum lies at
    column shifts -3, 0 and 3 at once, and the first strict minimum in scan order is the one at -3."""
    c = TIE
    rng = np.random.default_rng(77)
    cols = np.arange(c["W"]) % c["period"]
    ref = (1.0 + 0.3 * rng.standard_normal((c["K"], c["H"], c["period"])))[:, :, cols]
    sam = 0.8 * ref + 0.01 * rng.standard_normal(ref.shape)
    mask = (rng.random((c["K"], c["H"], c["period"])) >= 0.10).astype(np.float64)[:, :, cols]
    sam, ref, mask = (np.ascontiguousarray(a) for a in (sam, ref, mask))
    return _frozen(sam, ref, mask)


def illposed_count(exp, judged):
    """The pixels among `judged` with err = 1 on which the REFERENCE's own sub-pixel Newton iteration is ill-posed on the
    expectation's own 4x4 neighbourhood (oracle/parity.py: not converged, or not reproducible under rounding noise of its
    inputs): the pixels on which an implementation may miss the sub-pixel bar."""
    from oracle import parity
    n = 0
    for xi, xj in np.argwhere(judged & (exp["err"] == 1)):
        a, d = exp["debug_a"][xi, xj], exp["debug_d"][xi, xj]
        n += bool(parity.newton_unconverged(a, d) or parity.newton_unstable(a, d))
    return n
