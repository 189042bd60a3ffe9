"""
tests/track_expect.py -- what ``model.track()`` must return on a given volume, built WITHOUT the code under test.

The rules are those of include/umpa_grid.h (umpa_grid_track), restated on a volume ``cost[U, U, N0, N1]`` (and ``T``, ``df`` in
the same layout), ``U = 2 ms - 1``, on top of tests/basins_expect.py (``is_basin`` and the epilogue of a kept basin):

  * d2(s) = (si - p_i) * (si - p_i) + (sj - p_j) * (sj - p_j), every operation rounded to fp64 (numpy's elementwise
    arithmetic does not fuse); a pixel whose p_i or p_j is NaN has d2 = 0 everywhere;
  * a basin is admissible iff radius is None (or negative) or d2 <= radius * radius;
  * MODE 0 (nearest): the admissible basin with the smallest d2, then the smallest cost, then the earliest in scan order;
    MODE 1 (penalty): the admissible basins in scan order, the first is the best so far and a later one replaces it iff
    its key cost + lam * d2 is `<` the best's (a NaN key neither wins nor loses);
  * the chosen basin gets the epilogue of a kept basin; ``cost0`` is the lowest basin cost (0 without basins), ``count`` all
    basins, ``found`` the admissible ones; found == 0: zeros, and err = 0 in the dictionary (-1 at the C ABI).

``restate`` chooses with whole-array numpy operations (masked minima), ``brute`` with a Python loop over pixels and shifts
that follows the sentences above; tests/test_track_cpu.py holds the one against the other.
"""
import functools

import numpy as np

import basins_expect as BE

NEAREST, PENALTY = 0, 1


def _priors(prior_i, prior_j, N0, N1):
    pi = np.ascontiguousarray(np.broadcast_to(np.asarray(prior_i, dtype=np.float64), (N0, N1)))
    pj = np.ascontiguousarray(np.broadcast_to(np.asarray(prior_j, dtype=np.float64), (N0, N1)))
    return pi, pj


def _empty(kind_df, N0, N1):
    out = {n: np.zeros((N0, N1)) for n in ("dx", "dy", "f", "T", "cost", "cost0") + (("df",) if kind_df else ())}
    out["shift"] = np.zeros((2, N0, N1), np.int32)
    out.update({n: np.zeros((N0, N1), np.int32) for n in ("err", "count", "found")})
    return out


def _finish(out, chosen, cost, T, df, ms, subpx, fit):
    """the epilogue of a kept basin (tests/basins_expect.py) at every pixel with a chosen shift; `chosen(xi, xj)` -> (a, b) or None"""
    fit = fit or (BE.cpu_fit(subpx) if subpx != 0 else None)
    N0, N1 = cost.shape[2:]
    one = BE._empty(df is not None, 1, N0, N1)
    for xi in range(N0):
        for xj in range(N1):
            s = chosen(xi, xj)
            if s is None:
                continue
            at = lambda si, sj: cost[si + ms - 1, sj + ms - 1, xi, xj]
            fit_of = lambda n, si, sj: (T if n == "T" else df)[si + ms - 1, sj + ms - 1, xi, xj]
            BE._epilogue(one, 0, xi, xj, s[0], s[1], at, fit_of, ms, subpx, fit)
    for n in ("dx", "dy", "f", "T", "cost") + (("df",) if df is not None else ()):
        out[n][...] = one[n][0]
    out["shift"][...] = one["shift"][0]
    out["err"][...] = np.maximum(one["err"][0], 0)
    return out


def restate(cost, T, df, prior_i, prior_j, mode, lam, radius, subpx, fit=None):
    """The dictionary of ``model.track()`` from a volume (fp64 arrays ``[U, U, N0, N1]``; ``df`` None without dark-field).
    ``prior_i`` rows, ``prior_j`` columns: scalars or ``[N0, N1]``; ``radius`` None: no limit; ``lam`` is read in MODE 1 only."""
    cost = np.asarray(cost, dtype=np.float64)
    U, _, N0, N1 = cost.shape
    ms = (U + 1) // 2
    assert U == 2 * ms - 1 and mode in (NEAREST, PENALTY)
    pi, pj = _priors(prior_i, prior_j, N0, N1)
    sh = (np.arange(U) - (ms - 1)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = sh[:, None, None, None] - pi[None, None], sh[None, :, None, None] - pj[None, None]
        d2 = a * a + b * b
        d2 = np.where(np.isnan(pi) | np.isnan(pj), 0.0, d2).reshape(U * U, N0, N1)
        basin = BE.is_basin(cost).reshape(U * U, N0, N1)
        c = cost.reshape(U * U, N0, N1)
        adm = basin if radius is None or radius < 0 else basin & (d2 <= np.float64(radius) * np.float64(radius))
        out = _empty(df is not None, N0, N1)
        out["count"][...] = basin.sum(axis=0)
        out["found"][...] = adm.sum(axis=0)
        out["cost0"][...] = np.where(out["count"] > 0, np.where(basin, c, np.inf).min(axis=0), 0.0)
        if mode == NEAREST:                                           # neither d2 nor a basin's cost is ever NaN
            cand = adm & (d2 == np.where(adm, d2, np.inf).min(axis=0)[None])
            cand &= c == np.where(cand, c, np.inf).min(axis=0)[None]
            pick = np.argmax(cand, axis=0)
        else:
            key = c + np.float64(lam) * d2
            first = np.argmax(adm, axis=0)                            # the best so far, to begin with
            stuck = np.isnan(np.take_along_axis(key, first[None], axis=0)[0])
            live = adm & ~np.isnan(key)
            cand = live & (key == np.where(live, key, np.inf).min(axis=0)[None])
            pick = np.where(stuck, first, np.argmax(cand, axis=0))

    def chosen(xi, xj):
        if out["found"][xi, xj] == 0:
            return None
        s = int(pick[xi, xj])
        return s // U - (ms - 1), s % U - (ms - 1)
    return _finish(out, chosen, cost, T, df, ms, subpx, fit)


def brute(cost, T, df, prior_i, prior_j, mode, lam, radius, subpx, fit=None):
    """The same dictionary, the definition read out loud: per pixel, per shift, per neighbour."""
    cost = np.asarray(cost, dtype=np.float64)
    U, _, N0, N1 = cost.shape
    ms = (U + 1) // 2
    pi, pj = _priors(prior_i, prior_j, N0, N1)
    out = _empty(df is not None, N0, N1)
    inf = float("inf")
    r2 = None if radius is None or radius < 0 else float(np.float64(radius) * np.float64(radius))

    def chosen(xi, xj):
        cc = cost[:, :, xi, xj]
        p_i, p_j = np.float64(pi[xi, xj]), np.float64(pj[xi, xj])
        blind = bool(np.isnan(p_i) or np.isnan(p_j))
        best, count, found, low = None, 0, 0, inf
        for a in range(U):
            for b in range(U):
                s = float(cc[a, b])
                if not s < inf:
                    continue
                beaten = False
                for da in (-1, 0, 1):
                    for db in (-1, 0, 1):
                        na, nb = a + da, b + db
                        if (da == 0 and db == 0) or not (0 <= na < U and 0 <= nb < U):
                            continue
                        n = float(cc[na, nb])
                        if n < s or (n == s and (na, nb) < (a, b)):
                            beaten = True
                if beaten:
                    continue
                count += 1
                if s < low:
                    low = s
                with np.errstate(invalid="ignore", over="ignore"):
                    si, sj = np.float64(a - (ms - 1)), np.float64(b - (ms - 1))
                    d2 = np.float64(0.0) if blind else (si - p_i) * (si - p_i) + (sj - p_j) * (sj - p_j)
                    if r2 is not None and not d2 <= r2:
                        continue
                    found += 1
                    if mode == NEAREST:
                        better = best is not None and (d2 < best[0] or (d2 == best[0] and s < best[1]))
                        key = d2
                    else:
                        key = np.float64(s) + np.float64(lam) * d2
                        better = best is not None and key < best[0]
                if best is None or better:
                    best = (key, s, a, b)
        out["count"][xi, xj], out["found"][xi, xj] = count, found
        out["cost0"][xi, xj] = low if count else 0.0
        return None if best is None else (best[2] - (ms - 1), best[3] - (ms - 1))
    return _finish(out, chosen, cost, T, df, ms, subpx, fit)


@functools.lru_cache(maxsize=None)
def use_case():
    """The stack of tests/test_hip_basins.py's use case (true shift (1, 1), the alias one column period away wins at the
    ``known`` pixels), and what tracking it needs, all decided on the CPU from extended-precision volumes and their fp64
    bounds:

      ``lam``   2 max(gap) / period^2, gap = cost(true) - cost(alias) over ``known``: with the true shift as the prior the alias
                pays lam period^2 = 2 max(gap), twice what it has in hand anywhere;
      ``sure``  the pixels where the penalty choice is the true shift beyond doubt: every neighbour of the true shift lies
                above it by more than the two bounds (it is a basin in any fp64 evaluation), and every other shift's key lies
                above the true shift's cost by more than the two bounds plus the rounding of the key itself;
      ``sam0``  the noise-free sample of the same reference, and ``clean``: at every pixel its true shift lies below every
                other shift by more than the two bounds (checked by tests/test_track_cpu.py)."""
    import grid_expect as GE
    from nativelibs import gpu_test_module
    hb = gpu_test_module("basins")
    u = hb.USE
    sam, ref, known = hb._use_case()
    K, H, W, ms, Nw, period = u["K"], u["H"], u["W"], u["ms"], u["Nw"], u["period"]
    ty, tx = u["true"]
    U = 2 * ms - 1
    # the same construction without the noise term (the reference must come out the same, bit for bit)
    rng = np.random.default_rng(u["seed"])
    big = 1.0 + 0.5 * np.tile(rng.random((K, H + 2 * ms, period)), (1, 1, (W + 2 * ms) // period + 1))[:, :, :W + 2 * ms]
    big = big + u["aperiodic"] * rng.random(big.shape)
    assert np.array_equal(np.ascontiguousarray(big[:, ms:ms + H, ms:ms + W]), ref)
    sam0 = np.ascontiguousarray(big[:, ms + ty:ms + ty + H, ms + tx:ms + tx + W])

    def margins(stack, lam):
        """min over the other shifts of (key - bound) minus (cost + bound) of the true shift, per pixel, and the same over
        the eight neighbours with lam = 0"""
        v = GE.hp_volumes(0, stack, ref, GE.window(Nw), ms, ms + Nw, "sam")
        c, bd = v["cost"], v["bound"]
        sh = np.arange(U) - (ms - 1)
        d2 = ((sh[:, None] - ty) ** 2 + (sh[None, :] - tx) ** 2).astype(np.longdouble)[:, :, None, None]
        key = c + np.longdouble(lam) * d2
        slack = bd + 8 * np.finfo(np.float64).eps * np.abs(key)
        t = (ty + ms - 1, tx + ms - 1)
        m = key - slack - (c[t] + bd[t])[None, None]
        m[t] = np.inf
        nb = (c - bd - (c[t] + bd[t])[None, None])[t[0] - 1:t[0] + 2, t[1] - 1:t[1] + 2].copy()
        nb[1, 1] = np.inf
        return v, m.reshape(U * U, *m.shape[2:]).min(axis=0), nb.reshape(9, *nb.shape[2:]).min(axis=0)

    v = GE.hp_volumes(0, sam, ref, GE.window(Nw), ms, ms + Nw, "sam")
    gap = (v["cost"][ty + ms - 1, tx + ms - 1] - v["cost"][ty + ms - 1, tx - period + ms - 1])[known]
    lam = float(2 * gap.max() / period ** 2)
    _, m, nb = margins(sam, lam)
    _, m0, nb0 = margins(sam0, 0.0)
    return dict(sam=sam, ref=ref, known=known, sam0=sam0, lam=lam, gap=np.asarray(gap, dtype=np.float64),
                sure=np.asarray((m > 0) & (nb > 0), dtype=bool), clean=np.asarray((m0 > 0) & (nb0 > 0), dtype=bool), use=dict(u))


def assert_equal(got, want, what=""):
    """every map of `want`, bit for bit (NaN == NaN), with the right dtypes and shapes; HIP tensors are downloaded"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for n in sorted(want):
        g = got[n].cpu().numpy() if hasattr(got[n], "data_ptr") else np.asarray(got[n])
        assert g.dtype == want[n].dtype and g.shape == want[n].shape, (what, n, g.dtype, g.shape, want[n].dtype, want[n].shape)
        np.testing.assert_array_equal(g, want[n], err_msg="%s %s" % (what, n))
