"""
tests/grid_expect.py -- what ``search='grid'`` must return, built WITHOUT the code under test.

The costs are oracle/hp_cost.py's (numpy.longdouble, with the a-priori bound of an fp64 evaluation), the sub-pixel fits the
oracle's ``umpaor_spmin`` / ``umpaor_spmin_quad``; the rules are those of include/umpa_grid.h:

  * integer minimum: the first strict minimum over the shifts, rows first, then columns;
  * quadrant (Optim.cpp:344-345): ip = cost(row + 1) < cost(row - 1), jp likewise on the columns; the 4x4 neighbourhood
    is rows ip .. ip + 3, columns jp .. jp + 3 of the 5x5 around the minimum: shifts ci + ip - 2 .. ci + ip + 1, cj + jp - 2 ..;
  * ok pixel: start (1 - ip, 1 - jp), fit as ``subpx`` says (0: none, f = 1 - ip), uv += (ci, cj) + (ip, jp) - 1; T / df of the
    integer minimum; Ncalls = (2 ms - 1)^2; debug_a the 4x4, debug_d the 5x5 around the minimum with -1 outside the range;
  * the 4x4 leaves the search range: err = 0, dx / dy the integer minimum, f its cost, T / df its fit, debug_a zero.

The near-tie mask: a pixel whose two smallest extended-precision costs differ by less than the sum of their fp64 bounds.
There an fp64 implementation may pick either shift, so the pixel says nothing about the search.
"""
import functools

import numpy as np

# the stacks of the GPU tests that are judged against extended precision (tests/test_hip_grid.py) and whose admissibility
# tests/test_grid_cpu.py checks: make_stack arguments + window half-width
STACKS = {
    "64x72x3": dict(H=64, W=72, K=3, Nw=2, ms=4, seed=21),
    "96x112x4": dict(H=96, W=112, K=4, Nw=3, ms=5, seed=22),
}
NEAR_TIE_CAP = 0.005            # the issue's cap on the share of pixels left out


def stack(name):
    from umpa_amd.synth import make_stack
    c = STACKS[name]
    sam, ref, _ = make_stack(c["H"], c["W"], c["K"], c["ms"], df=True, seed=c["seed"], amplitude=0.6 * c["ms"])
    return sam, ref, c


def window(Nw):
    w = np.multiply.outer(np.hamming(2 * Nw + 1), np.hamming(2 * Nw + 1))
    return np.ascontiguousarray(w / w.sum())


def hp_volumes(kind, sam, ref, win, ms, pad, assign, pixels=None):
    """cost, T, df (None without dark-field), bound as [U, U, ...pixels] longdouble arrays; `pixels` = (xi, xj) index
    arrays into the output maps (default: every pixel, shape N0 x N1)."""
    from oracle import hp_cost
    H, W = np.asarray(sam).shape[1:]
    N0, N1 = H - 2 * pad, W - 2 * pad
    U = 2 * ms - 1
    if pixels is None:
        xi, xj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    else:
        xi, xj = (np.asarray(v) for v in pixels)
    sh = np.arange(U) - ms + 1
    si = np.broadcast_to(sh.reshape((U, 1) + (1,) * xi.ndim), (U, U) + xi.shape)
    sj = np.broadcast_to(sh.reshape((1, U) + (1,) * xi.ndim), (U, U) + xi.shape)
    pi = np.broadcast_to(xi + pad, si.shape)
    pj = np.broadcast_to(xj + pad, si.shape)
    r = hp_cost.hp_cells(kind, sam, ref, win, pi, pj, si, sj, assign)
    return {k: (v.reshape(si.shape) if v is not None else None) for k, v in r.items()}


def near_tie(cost, bound):
    """[pixels...] bool from [U, U, pixels...] arrays."""
    U = cost.shape[0]
    c = cost.reshape((U * U,) + cost.shape[2:])
    b = bound.reshape(c.shape)
    order = np.argsort(c, axis=0, kind="stable")[:2]
    c2 = np.take_along_axis(c, order, axis=0)
    b2 = np.take_along_axis(b, order, axis=0)
    return (c2[1] - c2[0]) < (b2[0] + b2[1])


def expected(kind, sam, ref, win, ms, pad, assign, subpx, volumes=None):
    """(maps, near-tie mask): maps = dict of err, debug_Ncalls, dx, dy, f, T, (df,) debug_a, debug_d, plus `ci`, `cj` (the
    integer minimum) and `cmin` / `cmin_bound` (its extended-precision cost and fp64 bound).  `volumes`: what hp_volumes
    returned for these arguments, where the caller has it already."""
    from oracle import cpu_model
    import ctypes as C
    lib = cpu_model.native("port")
    dp = C.POINTER(C.c_double)
    v = hp_volumes(kind, sam, ref, win, ms, pad, assign) if volumes is None else volumes
    cost, bound = v["cost"], v["bound"]
    U = 2 * ms - 1
    N0, N1 = cost.shape[2:]
    flat = cost.reshape(U * U, N0, N1)
    arg = np.argmin(flat, axis=0)                                    # the first minimum in rows-first order
    ci, cj = arg // U - (ms - 1), arg % U - (ms - 1)
    out = dict(err=np.zeros((N0, N1), np.int32), debug_Ncalls=np.full((N0, N1), U * U, np.int32),
               dx=cj.astype(np.float64), dy=ci.astype(np.float64), f=np.zeros((N0, N1)), T=np.zeros((N0, N1)),
               debug_a=np.zeros((N0, N1, 16)), debug_d=np.full((N0, N1, 25), -1.0), ci=ci, cj=cj,
               cmin=np.zeros((N0, N1), np.longdouble), cmin_bound=np.zeros((N0, N1), np.longdouble))
    if kind == 1:
        out["df"] = np.zeros((N0, N1))
    c64 = cost.astype(np.float64)
    for xi in range(N0):
        for xj in range(N1):
            a, b = int(ci[xi, xj]), int(cj[xi, xj])
            at = lambda si, sj: c64[si + ms - 1, sj + ms - 1, xi, xj]
            out["cmin"][xi, xj] = cost[a + ms - 1, b + ms - 1, xi, xj]
            out["cmin_bound"][xi, xj] = bound[a + ms - 1, b + ms - 1, xi, xj]
            out["T"][xi, xj] = v["T"][a + ms - 1, b + ms - 1, xi, xj]
            if kind == 1:
                out["df"][xi, xj] = v["df"][a + ms - 1, b + ms - 1, xi, xj]
            out["f"][xi, xj] = at(a, b)
            for q in range(25):
                si, sj = a + q // 5 - 2, b + q % 5 - 2
                if abs(si) < ms and abs(sj) < ms:
                    out["debug_d"][xi, xj, q] = at(si, sj)
            if abs(a) > ms - 2 or abs(b) > ms - 2:
                continue
            ip = 1 if at(a + 1, b) < at(a - 1, b) else 0
            jp = 1 if at(a, b + 1) < at(a, b - 1) else 0
            i0, j0 = a + ip - 2, b + jp - 2
            if i0 <= -ms or i0 + 3 >= ms or j0 <= -ms or j0 + 3 >= ms:
                continue
            nb = np.array([at(i0 + g // 4, j0 + g % 4) for g in range(16)])
            p = np.array([1.0 - ip, 1.0 - jp])
            if subpx == 0:
                f = p[0]
            elif subpx == 1:
                f = lib.spmin_quad(nb.ctypes.data_as(dp), p.ctypes.data_as(dp))
            else:
                f = lib.spmin(nb.ctypes.data_as(dp), p.ctypes.data_as(dp))
            out["err"][xi, xj] = 1
            out["f"][xi, xj] = f
            out["dy"][xi, xj] = p[0] + (a + ip - 1.0)
            out["dx"][xi, xj] = p[1] + (b + jp - 1.0)
            out["debug_a"][xi, xj] = nb
    return out, near_tie(cost, bound)


@functools.lru_cache(maxsize=None)
def expected_for(name, kind, assign, subpx):
    sam, ref, c = stack(name)
    return expected(kind, sam, ref, window(c["Nw"]), c["ms"], c["ms"] + c["Nw"], assign, subpx)
