"""
tests/sequence_expect.py -- what ``model.sequence()`` must return on a given volume and state, built WITHOUT the code under
test (umpa_amd.sequence.restate is compared with this, not used by it).

The rules are those of include/umpa_grid.h (umpa_grid_sequence), on a volume ``cost[U, U, N0, N1]`` (and ``T``, ``df`` in the
same layout), ``U = 2 ms - 1``, and a state ``prev`` of the volume's shape or None.  Scan order = rows first, then columns;
every minimum starts at +Inf and takes a candidate iff it is ``<`` the best so far:

  * m0 = min prev; prev None or not m0 < +Inf: M = 0;
  * R[si'][sj] = min_{sj'} (prev[si'][sj'] + lam * (double)((sj - sj')^2)), sj' ascending;
    Q[si][sj]  = min_{si'} (R[si'][sj] + lam * (double)((si - si')^2));
    cap = m0 + trunc;  Q' = cap < Q ? cap : Q;  M = Q' - m0   -- every product, sum and difference rounded to fp64;
  * A = C + M is the next state; s* is the first strict minimum of A; cost = C[s*], total = A[s*]; cost0 the first strict
    minimum of C (0 where none); moved = s* differs from the argmin of C;
  * s* gets the epilogue of a kept basin (tests/basins_expect.py) on C; no A below +Inf: zeros, shift (0, 0), and err = 0 in the
    dictionary (-1 at the C ABI).

``restate`` runs the minima as running ``where(c < best, c, best)`` updates over whole arrays, ``brute`` as Python loops over
pixels, s and s' that follow the sentences above; tests/test_sequence_cpu.py holds the one against the other.
"""
import numpy as np

import basins_expect as BE
from track_expect import assert_equal  # noqa: F401  (bit for bit, dtypes and shapes; HIP tensors are downloaded)

INF = float("inf")


def _envelope(P, axis, lam):
    """out[o] = min_q (P[q] + lam * (double)((o - q)^2)) along `axis`, q ascending, as a running strict minimum"""
    U = P.shape[axis]
    out = np.empty(P.shape)
    idx = lambda q: tuple(q if a == axis else slice(None) for a in range(P.ndim))
    for o in range(U):
        best = np.full(P[idx(0)].shape, INF)
        for q in range(U):
            c = P[idx(q)] + np.float64(lam) * np.float64((o - q) * (o - q))
            best = np.where(c < best, c, best)
        out[idx(o)] = best
    return out


def transition(prev, lam, trunc, shape):
    """M[U, U, N0, N1]"""
    if prev is None:
        return np.zeros(shape)
    P = np.asarray(prev, dtype=np.float64)
    assert P.shape == tuple(shape)
    with np.errstate(invalid="ignore", over="ignore"):
        m0 = np.full(P.shape[2:], INF)
        for a in range(P.shape[0]):
            for b in range(P.shape[1]):
                m0 = np.where(P[a, b] < m0, P[a, b], m0)
        Q = _envelope(_envelope(P, 1, lam), 0, lam)
        cap = m0 + np.float64(INF if trunc is None else trunc)
        Q = np.where(cap < Q, cap, Q)
        return np.where(m0 < INF, Q - m0, 0.0)


def _empty(kind_df, U, N0, N1):
    out = {n: np.zeros((N0, N1)) for n in ("dx", "dy", "f", "T", "cost", "total", "cost0") + (("df",) if kind_df else ())}
    out["shift"] = np.zeros((2, N0, N1), np.int32)
    out.update({n: np.zeros((N0, N1), np.int32) for n in ("err", "moved")})
    out["state"] = np.zeros((U, U, N0, N1))
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


def restate(cost, T, df, prev, lam, trunc, subpx, fit=None):
    """The dictionary of ``model.sequence()`` from a volume (fp64 arrays ``[U, U, N0, N1]``; ``df`` None without dark-field)"""
    cost = np.asarray(cost, dtype=np.float64)
    U, _, N0, N1 = cost.shape
    ms = (U + 1) // 2
    assert U == 2 * ms - 1
    out = _empty(df is not None, U, N0, N1)
    with np.errstate(invalid="ignore", over="ignore"):
        A = cost + transition(prev, lam, trunc, cost.shape)
    out["state"][...] = A
    best, low = np.full((N0, N1), INF), np.full((N0, N1), INF)
    pick, lpick = np.full((N0, N1), -1), np.full((N0, N1), -1)
    for a in range(U):
        for b in range(U):
            w = A[a, b] < best
            best, pick = np.where(w, A[a, b], best), np.where(w, a * U + b, pick)
            w = cost[a, b] < low
            low, lpick = np.where(w, cost[a, b], low), np.where(w, a * U + b, lpick)
    out["total"][...] = np.where(pick >= 0, best, 0.0)
    out["cost0"][...] = np.where(lpick >= 0, low, 0.0)
    out["moved"][...] = (pick >= 0) & (pick != lpick)

    def chosen(xi, xj):
        s = int(pick[xi, xj])
        return None if s < 0 else (s // U - (ms - 1), s % U - (ms - 1))
    return _finish(out, chosen, cost, T, df, ms, subpx, fit)


def brute(cost, T, df, prev, lam, trunc, subpx, fit=None):
    """The same dictionary, the definition read out loud: per pixel, per shift s, per predecessor s'."""
    cost = np.asarray(cost, dtype=np.float64)
    U, _, N0, N1 = cost.shape
    ms = (U + 1) // 2
    out = _empty(df is not None, U, N0, N1)
    lam = float(lam)
    trunc = INF if trunc is None else float(trunc)

    def add(a, b):                                                    # Python floats are fp64, every operation rounded
        return a + b

    def chosen(xi, xj):
        C = [[float(cost[a, b, xi, xj]) for b in range(U)] for a in range(U)]
        M = [[0.0] * U for _ in range(U)]
        if prev is not None:
            P = [[float(prev[a, b, xi, xj]) for b in range(U)] for a in range(U)]
            m0 = INF
            for a in range(U):
                for b in range(U):
                    if P[a][b] < m0:
                        m0 = P[a][b]
            if m0 < INF:
                R = [[INF] * U for _ in range(U)]
                for a in range(U):
                    for b in range(U):
                        for bb in range(U):
                            c = add(P[a][bb], lam * float((b - bb) * (b - bb)))
                            if c < R[a][b]:
                                R[a][b] = c
                cap = add(m0, trunc)
                for a in range(U):
                    for b in range(U):
                        q = INF
                        for aa in range(U):
                            c = add(R[aa][b], lam * float((a - aa) * (a - aa)))
                            if c < q:
                                q = c
                        if cap < q:
                            q = cap
                        M[a][b] = q - m0
        best, pick, low, lpick = INF, -1, INF, -1
        for a in range(U):
            for b in range(U):
                A = add(C[a][b], M[a][b])
                out["state"][a, b, xi, xj] = A
                if A < best:
                    best, pick = A, a * U + b
                if C[a][b] < low:
                    low, lpick = C[a][b], a * U + b
        out["total"][xi, xj] = best if pick >= 0 else 0.0
        out["cost0"][xi, xj] = low if lpick >= 0 else 0.0
        out["moved"][xi, xj] = 1 if pick >= 0 and pick != lpick else 0
        return None if pick < 0 else (pick // U - (ms - 1), pick % U - (ms - 1))
    return _finish(out, chosen, cost, T, df, ms, subpx, fit)
