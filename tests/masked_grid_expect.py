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


def pair_weight_count(name, which, assign):
    """[U, U, N0, N1] int: the window pixels, over all frames, that carry pair weight.  The pair weight of a window pixel is
    w ma mb / (ma + mb + 1e-8) with w > 0 and ma, mb >= 0 (lib/Utils.cpp:125-130): it is non-zero iff both masks are, and
    wt, their sum, is 0 iff the count is."""
    c = GE.STACKS[name]
    ms, Nw, pad = c["ms"], c["Nw"], c["ms"] + c["Nw"]
    H, W = c["H"], c["W"]
    N0, N1 = H - 2 * pad, W - 2 * pad
    U, S = 2 * ms - 1, 2 * Nw + 1
    live = masks(name)[which] != 0
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


@functools.lru_cache(maxsize=None)
def hp(name, which, kind, assign):
    """oracle/hp_cost.hp_cells with the mask on every (pixel, shift): cost, T, df (None without dark-field), bound as
    [U, U, N0, N1] longdouble arrays, plus the bool arrays `dead` (wt = 0), `singular` and `deficient`.  Computed once, read-only."""
    from oracle import hp_cost
    sam, ref, c = stack(name)
    ms, pad = c["ms"], c["ms"] + c["Nw"]
    N0, N1 = c["H"] - 2 * pad, c["W"] - 2 * pad
    U = 2 * ms - 1
    sh = np.arange(U) - ms + 1
    si, sj, xi, xj = np.meshgrid(sh, sh, np.arange(N0) + pad, np.arange(N1) + pad, indexing="ij")
    with np.errstate(invalid="ignore", divide="ignore"):
        r = hp_cost.hp_cells(kind, sam, ref, GE.window(c["Nw"]), xi, xj, si, sj, assign, mask=masks(name)[which])
    out = {k: (v.reshape(si.shape) if v is not None else None) for k, v in r.items()}
    count = pair_weight_count(name, which, assign)
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
    v = hp(name, which, kind, assign)
    _, _, whole = pixel_classes(v)
    # pixels with a NaN are judged elsewhere (the restatements on the device's own volume): give argmin finite numbers there
    fill = {k: (np.where(np.isfinite(v[k].astype(np.float64)), v[k], np.longdouble(1)) if v[k] is not None else None)
            for k in ("cost", "T", "df", "bound")}
    maps, _ = GE.expected(kind, sam, ref, GE.window(c["Nw"]), c["ms"], c["ms"] + c["Nw"], assign, subpx, volumes=fill)
    return maps, near_tie(v), whole


@functools.lru_cache(maxsize=None)
def expected_for(name, which, kind, assign, subpx):
    return expected(name, which, kind, assign, subpx)


def covered(name, which):
    """``coverage >= thr`` as ``match()`` forms it (model.pyx:499-529, :431): the coverage of a pixel is the sum over the frames
    of the mask at the pixel; thr = 0.1 max / Na.  [N0, N1] bool."""
    c = GE.STACKS[name]
    pad = c["ms"] + c["Nw"]
    m = masks(name)[which]
    cov = m[:, pad:c["H"] - pad, pad:c["W"] - pad].sum(axis=0)
    return cov >= 0.1 * cov.max() / c["K"]
