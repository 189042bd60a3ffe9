"""
The numpy restatement of include/umpa_smooth.h (path aggregation over a cost volume and the per-pixel selection), a
brute-force evaluation of the same recursion for tiny volumes, and the input makers of tests/test_smooth_cpu.py and
tests/test_hip_smooth.py.

The restatement walks a path step by step, as the header's recursion does, and is vectorised over the lines (all paths of
one direction advance together) and the labels.  It is made of the header's own fp64 additions, subtractions and
comparisons in the header's order, so the library's results must EQUAL it.
"""
import numpy as np

DIRECTIONS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]
INF = np.inf


def as_labels(cost):
    """[U, U, N0, N1] or [U * U, N0, N1] -> (U, the volume as [U, U, N0, N1] float64)"""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim == 3:
        U = int(round(cost.shape[0] ** 0.5))
        cost = cost.reshape(U, U, cost.shape[1], cost.shape[2])
    assert cost.ndim == 4 and cost.shape[0] == cost.shape[1] and cost.shape[0] % 2 == 1
    return cost.shape[0], cost


def conditioned(cost):
    return np.where(np.isfinite(cost), cost, INF)


def fmin(x, y):
    """the header's min(x, y) = x < y ? x : y"""
    return np.where(x < y, x, y)


def envelope(L, lam):
    """The four in-place sweeps on h[a][b][...] = L."""
    h = L.copy()
    U = h.shape[0]
    for b in range(1, U):
        h[:, b] = fmin(h[:, b], h[:, b - 1] + lam)
    for b in range(U - 2, -1, -1):
        h[:, b] = fmin(h[:, b], h[:, b + 1] + lam)
    for a in range(1, U):
        h[a] = fmin(h[a], h[a - 1] + lam)
    for a in range(U - 2, -1, -1):
        h[a] = fmin(h[a], h[a + 1] + lam)
    return h


def path_cost(cost, lam, trunc, d):
    """L_r of direction number d for the whole volume: [U, U, N0, N1]."""
    U, cost = as_labels(cost)
    C = conditioned(cost)
    N0, N1 = C.shape[2:]
    void = np.isinf(C).all(axis=(0, 1))
    dr, dc = DIRECTIONS[d]
    L = np.empty_like(C)
    if dr == 0:                                    # along the rows: all rows advance together, one column per step
        order = range(N1) if dc > 0 else range(N1 - 1, -1, -1)
        prev = None
        for j in order:
            L[:, :, :, j] = _step(C[:, :, :, j], void[:, j], None if prev is None else L[:, :, :, prev],
                                  None if prev is None else void[:, prev], np.ones(N0, dtype=bool), lam, trunc)
            prev = j
        return L
    order = range(N0) if dr > 0 else range(N0 - 1, -1, -1)
    cols = np.arange(N1)
    src = cols - dc                                # the predecessor's column
    inside = (src >= 0) & (src < N1)
    srcc = np.clip(src, 0, N1 - 1)
    prev = None
    for i in order:
        if prev is None:
            L[:, :, i, :] = _step(C[:, :, i, :], void[i], None, None, inside, lam, trunc)
        else:
            L[:, :, i, :] = _step(C[:, :, i, :], void[i], L[:, :, prev, :][:, :, srcc], void[prev][srcc], inside, lam, trunc)
        prev = i
    return L


def _step(Cp, pvoid, Lq, qvoid, has_q, lam, trunc):
    """One step of every line: Cp[U, U, n] the conditioned costs at the lines' pixels, Lq[U, U, n] the predecessors' L_r
    (None at the first step), qvoid[n], has_q[n] whether the predecessor lies inside the region."""
    if Lq is None:
        out = Cp.copy()
    else:
        with np.errstate(invalid="ignore"):        # lines without a predecessor carry values that are not used
            m = Lq.min(axis=(0, 1))
            h = envelope(Lq, lam)
            cont = Cp + (fmin(h, m + trunc) - m)
        out = np.where(has_q & ~qvoid, cont, Cp)
    return np.where(pvoid, 0.0, out)


def summed(cost, lam, trunc, dirs=0xFF):
    """total[U, U, N0, N1] in the header's grouping."""
    U, cost = as_labels(cost)
    groups = []
    for members in ((0, 1), (2, 3, 4, 5, 6, 7)):
        acc = None
        for d in members:
            if dirs & (1 << d):
                L = path_cost(cost, lam, trunc, d)
                acc = L if acc is None else acc + L
        if acc is not None:
            groups.append(acc)
    assert groups
    return groups[0] if len(groups) == 1 else groups[0] + groups[1]


def select(cost, total):
    """shift[2, N0, N1] int32, smin, margin, valid int32"""
    U, cost = as_labels(cost)
    total = total.reshape(cost.shape)
    N0, N1 = cost.shape[2:]
    void = ~np.isfinite(cost).any(axis=(0, 1))
    flat = total.reshape(U * U, N0, N1)
    best = flat[0].copy()
    lb = np.zeros((N0, N1), dtype=np.int64)
    for l in range(1, U * U):
        take = flat[l] < best
        best = np.where(take, flat[l], best)
        lb = np.where(take, l, lb)
    a_s, b_s = lb // U, lb % U
    far = np.full((N0, N1), INF)
    for a in range(U):
        for b in range(U):
            away = np.maximum(np.abs(a - a_s), np.abs(b - b_s)) >= 2
            far = np.where(away, fmin(far, total[a, b]), far)
    h = (U - 1) // 2
    with np.errstate(invalid="ignore"):
        margin = far - best
    out = {"shift": np.stack([a_s - h, b_s - h]).astype(np.int32), "smin": best, "margin": margin,
           "valid": np.ones((N0, N1), dtype=np.int32)}
    out["shift"][:, void] = 0
    out["smin"] = np.where(void, 0.0, out["smin"])
    out["margin"] = np.where(void, 0.0, out["margin"])
    out["valid"][void] = 0
    return out


def aggregate(cost, lam, trunc, dirs=0xFF):
    """What umpa_amd.smooth.aggregate(..., return_total=True) must return, in the shape of `cost`."""
    total = summed(cost, lam, trunc, dirs)
    out = select(cost, total)
    out["total"] = total.reshape(np.asarray(cost).shape)
    return out


# ----------------------------------------------------------------------------- brute force, for tiny volumes

def path_cost_brute(cost, lam, trunc, d):
    """L_r by the recursion written per pixel and label with the penalty in closed form:
    L(p, l) = C'(p, l) + (min_l' (L(q, l') + min(lam (|da| + |db|), trunc)) - min_l' L(q, l')).
    Equal to the sweeps wherever every sum is exact (dyadic lam, trunc and costs)."""
    U, cost = as_labels(cost)
    C = conditioned(cost)
    N0, N1 = C.shape[2:]
    dr, dc = DIRECTIONS[d]
    L = np.zeros_like(C)
    rows = range(N0) if dr >= 0 else range(N0 - 1, -1, -1)
    colsq = range(N1) if dc >= 0 else range(N1 - 1, -1, -1)
    isvoid = lambda i, j: not np.isfinite(C[:, :, i, j]).any()
    for i in rows:
        for j in colsq:
            qi, qj = i - dr, j - dc
            if isvoid(i, j):
                L[:, :, i, j] = 0.0
                continue
            if not (0 <= qi < N0 and 0 <= qj < N1) or isvoid(qi, qj):
                L[:, :, i, j] = C[:, :, i, j]
                continue
            Lq = L[:, :, qi, qj]
            m = Lq.min()
            for a in range(U):
                for b in range(U):
                    best = INF
                    for a2 in range(U):
                        for b2 in range(U):
                            pen = min(lam * (abs(a - a2) + abs(b - b2)), trunc)
                            best = min(best, Lq[a2, b2] + pen)
                    L[a, b, i, j] = C[a, b, i, j] + (best - m)
    return L


# ----------------------------------------------------------------------------- input makers

def random_volume(U, N0, N1, seed, dyadic=True, scale=1.0):
    """Costs that really compete: a bowl around a per-pixel centre plus noise.  dyadic: multiples of 1/8 below 64, so that
    every sum with dyadic penalties is exact."""
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.arange(U), np.arange(U), indexing="ij")
    ca = rng.integers(0, U, size=(N0, N1))
    cb = rng.integers(0, U, size=(N0, N1))
    bowl = np.abs(a[:, :, None, None] - ca) + np.abs(b[:, :, None, None] - cb)
    if dyadic:
        return (bowl + rng.integers(0, 64, size=(U, U, N0, N1)) / 8.0).astype(np.float64)
    return scale * (0.3 * bowl + rng.random((U, U, N0, N1)))


def with_specials(cost, seed, void_row=None, void_col=None, scattered=True):
    """NaN, +Inf, -Inf entries, scattered void pixels, a void row, a void column (copies)."""
    cost = np.array(cost, dtype=np.float64)
    U, U2, N0, N1 = cost.shape
    rng = np.random.default_rng(seed)
    if scattered:
        for val in (np.nan, np.inf, -np.inf):
            hit = rng.random(cost.shape) < 0.04
            cost[hit] = val
        void = rng.random((N0, N1)) < 0.08
        cost[:, :, void] = rng.choice([np.nan, np.inf, -np.inf], size=(U, U, int(void.sum())))
    if void_row is not None:
        cost[:, :, void_row, :] = np.nan
    if void_col is not None:
        cost[:, :, :, void_col] = np.inf
    return cost


BEHAVIOUR = dict(U=9, N0=40, N1=52, lam=2.0, trunc=8.0, depth=2.0, share=0.10, seed=11)


def behavioural_case():
    """A 40 x 52 volume at U = 9: a quadratic bowl (d si^2 + d sj^2) around a smooth true integer field, and at a seeded
    10 % of the pixels a spurious bowl whose bottom lies 2 below the true one's, 3 or 4 labels away along one axis.
    Returns (cost, truth[2, N0, N1], spoiled[N0, N1]).  Every value is a small integer, so all sums are exact.

    Why lam = 2, trunc = 8 suit it.  The true field moves by at most one step per axis between neighbours, so following
    it costs a path at most 2 lam = 4 per step, and mostly nothing.  A spoiled pixel's spurious label saves 2 in the data
    term of each path, but a path whose predecessor has its minimum at the truth pays min(3 lam, trunc) = 6 or more to
    enter it.  The spurious label wins only where neighbours along most paths are spoiled towards the same label, which a
    seeded 10 % with scattered offsets does not produce here.  A larger lam (3 and more) starts to hold the field back
    where it moves.  The tests assert the outcome, and the premise: the per-pixel argmin is wrong at every spoiled pixel."""
    p = BEHAVIOUR
    U, N0, N1 = p["U"], p["N0"], p["N1"]
    h = (U - 1) // 2
    rng = np.random.default_rng(p["seed"])
    i, j = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    ti = np.rint(2.0 * np.sin(2 * np.pi * i / N0) * np.cos(np.pi * j / N1)).astype(np.int64)
    tj = np.rint(2.0 * np.cos(2 * np.pi * j / N1)).astype(np.int64)
    a, b = np.meshgrid(np.arange(U) - h, np.arange(U) - h, indexing="ij")
    a, b = a[:, :, None, None], b[:, :, None, None]
    cost = ((a - ti) ** 2 + (b - tj) ** 2).astype(np.float64)
    spoiled = rng.random((N0, N1)) < p["share"]
    # the spurious centre: the true one moved by 3 or 4 labels along one axis, towards the side that has the room
    axis = rng.integers(0, 2, size=(N0, N1))
    dist = rng.integers(3, 5, size=(N0, N1))
    wi = np.where(axis == 0, np.where(ti <= 0, ti + dist, ti - dist), ti)
    wj = np.where(axis == 1, np.where(tj <= 0, tj + dist, tj - dist), tj)
    assert (np.abs(wi) <= h).all() and (np.abs(wj) <= h).all()
    bowl = ((a - wi) ** 2 + (b - wj) ** 2 - p["depth"]).astype(np.float64)
    cost = np.where(spoiled, np.minimum(cost, bowl), cost)
    return cost, np.stack([ti, tj]).astype(np.int32), spoiled


def argmin_field(cost):
    """the per-pixel first minimum as a shift field [2, N0, N1]"""
    U, cost = as_labels(cost)
    l = conditioned(cost).reshape(U * U, *cost.shape[2:]).argmin(axis=0)
    return np.stack([l // U - (U - 1) // 2, l % U - (U - 1) // 2]).astype(np.int32)
