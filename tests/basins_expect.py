"""
tests/basins_expect.py -- what ``model.basins()`` must return on a given volume, built WITHOUT the code under test.

The rules are those of include/umpa_grid.h (umpa_grid_basins), restated on a volume ``cost[U, U, N0, N1]`` (and ``T``, ``df``
in the same layout), ``U = 2 ms - 1``, scan order = rows first, then columns:

  * a neighbour n BEATS a shift s iff C[n] < C[s], or C[n] == C[s] and n precedes s in scan order;
  * s is a basin iff C[s] < +Inf and none of its up to eight neighbours inside the box beats it (plain ``<`` / ``==`` of
    doubles: a NaN neighbour never beats, a NaN shift is never a basin, -Inf is a cost like any other);
  * basins are ranked by cost ascending, scan order among equal costs; the first k are kept, ``count`` counts all;
  * per kept basin the epilogue of the grid search around it (tests/grid_expect.py has the same lines for the global
    minimum): quadrant rule, 4x4 neighbourhood, the sub-pixel fit the mode asks for (0: none, f = 1 - ip), T / df of the
    integer shift, err = 1; err = 0 with the integer shift and its cost where the 4x4 leaves the search range;
  * slots k >= count: err = -1, zeros, shift (0, 0).

``restate`` finds the basins with whole-array numpy operations, ``brute`` with a Python loop over pixels, shifts and
neighbours that follows the sentences above word for word; tests/test_basins_cpu.py holds the one against the other.
The sub-pixel fit is a parameter: ``cpu_fit`` is the oracle's (the helpers tests/grid_expect.py uses), ``device_fit`` the
HIP library's own entry points for one 4x4 array (the GPU tests compare bit for bit, and the oracle's fit agrees with the
device's to rounding only).
"""
import ctypes as C

import numpy as np

MAX_K = 8


def cpu_fit(subpx):
    """fit(nb16, p) -> f, ``p`` (start, then result) updated in place: the oracle's umpaor_spmin / umpaor_spmin_quad"""
    from oracle import cpu_model
    lib = cpu_model.native("port")
    dp = C.POINTER(C.c_double)
    fn = lib.spmin_quad if subpx == 1 else lib.spmin

    def fit(nb, p):
        return fn(nb.ctypes.data_as(dp), p.ctypes.data_as(dp))
    return fit


def device_fit(subpx, device=0):
    """The same call shape on umpa_hip_spmin / umpa_hip_spmin_quad: one 4x4 array, fitted by the device's own code."""
    from umpa_amd import _lib
    lib = _lib.hip()
    fn = lib.spmin_quad if subpx == 1 else lib.spmin
    val = np.zeros(1)

    def fit(nb, p):
        lib.check(fn(device, _lib._ptr(nb, _lib._dp), _lib._ptr(p, _lib._dp), _lib._ptr(val, _lib._dp)), "spmin")
        return val[0]
    return fit


def is_basin(cost):
    """[U, U, ...] bool: the basin rule, by shifted copies of the volume"""
    c = np.asarray(cost)
    U = c.shape[0]
    order = np.broadcast_to((np.arange(U)[:, None] * U + np.arange(U)[None, :]).reshape((U, U) + (1,) * (c.ndim - 2)), c.shape)
    ok = c < np.inf
    with np.errstate(invalid="ignore"):
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                if di == 0 and dj == 0:
                    continue
                n = np.full(c.shape, np.nan, dtype=c.dtype)           # a neighbour outside the box: NaN, beats nothing
                no = np.full(c.shape, U * U)
                dst = (slice(max(0, -di), U - max(0, di)), slice(max(0, -dj), U - max(0, dj)))
                src = (slice(max(0, di), U - max(0, -di)), slice(max(0, dj), U - max(0, -dj)))
                n[dst], no[dst] = c[src], order[src]
                ok &= ~((n < c) | ((n == c) & (no < order)))
    return ok


def _empty(kind_df, k, N0, N1):
    out = {n: np.zeros((k, N0, N1)) for n in ("dx", "dy", "f", "T", "cost") + (("df",) if kind_df else ())}
    out["shift"] = np.zeros((k, 2, N0, N1), np.int32)
    out["err"] = np.full((k, N0, N1), -1, np.int32)
    out["count"] = np.zeros((N0, N1), np.int32)
    return out


def _epilogue(out, r, xi, xj, a, b, at, fit_of, ms, subpx, fit):
    """slot r of pixel (xi, xj): the basin at shift (a, b); `at(si, sj)` the pixel's costs, `fit_of(name, si, sj)` its T / df"""
    out["shift"][r, :, xi, xj] = (a, b)
    out["cost"][r, xi, xj] = out["f"][r, xi, xj] = at(a, b)
    out["dy"][r, xi, xj], out["dx"][r, xi, xj] = a, b
    out["T"][r, xi, xj] = fit_of("T", a, b)
    if "df" in out:
        out["df"][r, xi, xj] = fit_of("df", a, b)
    out["err"][r, xi, xj] = 0
    if abs(a) > ms - 2 or abs(b) > ms - 2:                            # on the border of the box: a neighbour is missing
        return
    ip = 1 if at(a + 1, b) < at(a - 1, b) else 0
    jp = 1 if at(a, b + 1) < at(a, b - 1) else 0
    i0, j0 = a + ip - 2, b + jp - 2
    if i0 <= -ms or i0 + 3 >= ms or j0 <= -ms or j0 + 3 >= ms:
        return
    nb = np.array([at(i0 + g // 4, j0 + g % 4) for g in range(16)], dtype=np.float64)
    p = np.array([1.0 - ip, 1.0 - jp])
    f = p[0] if subpx == 0 else fit(nb, p)
    out["err"][r, xi, xj] = 1
    out["f"][r, xi, xj] = f
    out["dy"][r, xi, xj] = p[0] + (a + ip - 1.0)
    out["dx"][r, xi, xj] = p[1] + (b + jp - 1.0)


def _fill(out, basin_lists, cost, T, df, ms, k, subpx, fit):
    fit = fit or (cpu_fit(subpx) if subpx != 0 else None)
    N0, N1 = cost.shape[2:]
    for xi in range(N0):
        for xj in range(N1):
            kept = basin_lists(xi, xj)
            at = lambda si, sj: cost[si + ms - 1, sj + ms - 1, xi, xj]
            fit_of = lambda n, si, sj: (T if n == "T" else df)[si + ms - 1, sj + ms - 1, xi, xj]
            for r, (a, b) in enumerate(kept[:k]):
                _epilogue(out, r, xi, xj, a, b, at, fit_of, ms, subpx, fit)
    return out


def restate(cost, T, df, k, subpx, fit=None):
    """The dictionary of ``model.basins(k)`` from a volume (fp64 arrays ``[U, U, N0, N1]``; ``df`` None without dark-field)."""
    cost = np.asarray(cost, dtype=np.float64)
    U, _, N0, N1 = cost.shape
    ms = (U + 1) // 2
    assert 1 <= k <= MAX_K and U == 2 * ms - 1
    basin = is_basin(cost).reshape(U * U, N0, N1)
    out = _empty(df is not None, k, N0, N1)
    out["count"][...] = basin.sum(axis=0)
    # ranking: a stable sort by cost of the shifts in scan order, non-basins last (+Inf is no basin's cost)
    order = np.argsort(np.where(basin, cost.reshape(U * U, N0, N1), np.inf), axis=0, kind="stable")

    def kept(xi, xj):
        q = order[:min(k, int(out["count"][xi, xj])), xi, xj]
        return [(int(s) // U - (ms - 1), int(s) % U - (ms - 1)) for s in q]
    return _fill(out, kept, cost, T, df, ms, k, subpx, fit)


def brute(cost, T, df, k, subpx, fit=None):
    """The same dictionary, the definition read out loud: per pixel, per shift, per neighbour."""
    cost = np.asarray(cost, dtype=np.float64)
    U, _, N0, N1 = cost.shape
    ms = (U + 1) // 2
    out = _empty(df is not None, k, N0, N1)

    def kept(xi, xj):
        c = cost[:, :, xi, xj]
        found = []
        for a in range(U):
            for b in range(U):
                s = float(c[a, b])
                if not s < float("inf"):
                    continue
                beaten = False
                for da in (-1, 0, 1):
                    for db in (-1, 0, 1):
                        na, nb = a + da, b + db
                        if (da == 0 and db == 0) or not (0 <= na < U and 0 <= nb < U):
                            continue
                        n = float(c[na, nb])
                        if n < s or (n == s and (na, nb) < (a, b)):
                            beaten = True
                if not beaten:
                    found.append((s, a * U + b))
        out["count"][xi, xj] = len(found)
        found.sort()                                                  # cost, then scan order
        return [(q // U - (ms - 1), q % U - (ms - 1)) for _, q in found]
    return _fill(out, kept, cost, T, df, ms, k, subpx, fit)


def assert_equal(got, want, what=""):
    """every map of `want`, bit for bit (NaN == NaN), with the right dtypes and shapes"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for n in sorted(want):
        g = np.asarray(got[n])
        assert g.dtype == want[n].dtype and g.shape == want[n].shape, (what, n, g.dtype, g.shape, want[n].dtype, want[n].shape)
        np.testing.assert_array_equal(g, want[n], err_msg="%s %s" % (what, n))
