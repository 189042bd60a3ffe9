"""
tests/sigma_expect.py -- TEST INFRASTRUCTURE: a numpy restatement of include/umpa_sigma.h.

moments() restates the header's MOMENTS (in float64, or in np.longdouble together with the header's rounding bound), solve()
its MODEL and SOLVE line by line in float64, brute() is an independent evaluation pixel by pixel that forms the Jacobian
explicitly in np.longdouble, fits (beta, K) by a weighted least-squares call and inverts with numpy's inv.  scatter_case()
is the behavioural case: the scatter of the CPU checker's own matches over noise realisations.  Nothing here imports
umpa_amd.sigma.
"""
import functools

import numpy as np

PLANES = (16, 34)
SKIP = -2 ** 31
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
(S00, S01, S02, S11, S12, S22, V00, V01, V02, V11, V12, V22, P0, P1, P2, QQ,
 MM00, MM01, MM02, MM11, MM12, MM22, NM00, NM01, NM02, NM10, NM11, NM12, NM20, NM21, NM22, AM0, AM1, AM2) = range(34)
U = 2.0 ** -53


def window(Nw):
    """the models' window: the outer product of two Hamming windows, normalised"""
    w = np.multiply.outer(np.hamming(2 * Nw + 1), np.hamming(2 * Nw + 1))
    return np.ascontiguousarray(w / w.sum())


def window_sv(win):
    sv = 0.0
    for w in np.asarray(win, dtype=np.float64).ravel():
        sv = sv + float(w) * float(w)
    return sv


def full_region(shape, Nw, ms):
    pad = Nw + ms
    return (0, 1, shape[-2] - 2 * pad, 0, 1, shape[-1] - 2 * pad)


def guard(shift, ms):
    return (np.abs(shift.astype(np.int64)) <= ms - 1).all(axis=0)


def _fields(sam, ref, Nw, ms, region, shift, dtype):
    """Generator over (k, tap index, a, u = (g_i, g_j, r)) as [N0, N1] arrays of `dtype`; skipped pixels read shift 0."""
    start0, step0, N0, start1, step1, N1 = region
    pad = Nw + ms
    ok = guard(shift, ms)
    si, sj = np.where(ok, shift[0], 0).astype(np.int64), np.where(ok, shift[1], 0).astype(np.int64)
    ci = (start0 + step0 * np.arange(N0) + pad)[:, None] + np.zeros((1, N1), dtype=np.int64)
    cj = (start1 + step1 * np.arange(N1) + pad)[None, :] + np.zeros((N0, 1), dtype=np.int64)
    half = dtype(0.5)
    for k in range(sam.shape[0]):
        A, R = sam[k].astype(dtype), ref[k].astype(dtype)
        for x, (di, dj) in enumerate(np.ndindex(2 * Nw + 1, 2 * Nw + 1)):
            ri, rj = ci + si + di - Nw, cj + sj + dj - Nw
            a, r = A[ci + di - Nw, cj + dj - Nw], R[ri, rj]
            gi, gj = half * (R[ri + 1, rj] - R[ri - 1, rj]), half * (R[ri, rj + 1] - R[ri, rj - 1])
            yield k, x, a, (gi, gj, r)


def moments(sam, ref, win, Nw, ms, kind, region, shift, dtype=np.float64):
    """[P, N0, N1] planes of the header in `dtype` (NaN at skipped pixels) and, for np.longdouble, the rounding bound of a
    double evaluation of each (float64, same shape); (moments, bound-or-None)."""
    N0, N1 = region[2], region[5]
    P, K, T = PLANES[kind], sam.shape[0], (2 * Nw + 1) ** 2
    want_bound = dtype is np.longdouble
    wv = np.asarray(win, dtype=np.float64).ravel()
    m, mag = np.zeros((P, N0, N1), dtype=dtype), np.zeros((P, N0, N1), dtype=dtype)
    per = per_abs = None
    last = -1
    def fold():
        f, n, fa = per[0:3], per[3:6], per[6]
        F, Nn, Fa = per_abs[0:3], per_abs[3:6], per_abs[6]
        for q, (i, j) in enumerate(PAIRS):
            m[MM00 + q] += f[i] * f[j]
            mag[MM00 + q] += F[i] * F[j]
        for i in range(3):
            for j in range(3):
                m[NM00 + 3 * i + j] += n[i] * f[j]
                mag[NM00 + 3 * i + j] += Nn[i] * F[j]
            m[AM0 + i] += fa * f[i]
            mag[AM0 + i] += Fa * F[i]
    for k, x, a, u in _fields(sam, ref, Nw, ms, region, shift, dtype):
        if k != last:
            if kind and last >= 0:
                fold()
            per, per_abs = np.zeros((7, N0, N1), dtype=dtype), np.zeros((7, N0, N1), dtype=dtype)
            last = k
        w = dtype(wv[x])
        v = w * w
        wa = w * a
        for q, (i, j) in enumerate(PAIRS):
            t = (w * u[i]) * u[j]
            m[S00 + q] += t
            mag[S00 + q] += np.abs(t)
            t = (v * u[i]) * u[j]
            m[V00 + q] += t
            mag[V00 + q] += np.abs(t)
        for i in range(3):
            t = wa * u[i]
            m[P0 + i] += t
            mag[P0 + i] += np.abs(t)
        m[QQ] += wa * a
        mag[QQ] += np.abs(wa * a)
        if kind:
            for i in range(3):
                per[i] += w * u[i]
                per[3 + i] += v * u[i]
                per_abs[i] += np.abs(w * u[i])
                per_abs[3 + i] += np.abs(v * u[i])
            per[6] += wa
            per_abs[6] += np.abs(wa)
    if kind:
        fold()
    ok = guard(shift, ms)
    m[:, ~ok] = np.nan
    if not want_bound:
        return m, None
    factor = np.full(P, (K * T + 6) * U)
    factor[16:] = (2 * T + K + 8) * U
    bound = (factor[:, None, None] * mag).astype(np.float64)
    bound[:, ~ok] = np.nan
    return m, bound


def _ldl_solve(L, D, b):
    n = len(b)
    y = [None] * n
    for i in range(n):
        y[i] = b[i]
        for k in range(i):
            y[i] = y[i] - L[i][k] * y[k]
    x = [y[i] / D[i] for i in range(n)]
    for i in range(n - 1, -1, -1):
        for k in range(i + 1, n):
            x[i] = x[i] - L[k][i] * x[k]
    return x


def solve(mom, kind, K, sv, dtype=np.float64):
    """MODEL and SOLVE of the header on [P, ...] moments, expression by expression, in `dtype` (float64: the header's
    arithmetic; np.longdouble: the same source text as the yardstick of tests/consumer_expect.py -- every constant below is a
    small integer or `sv`, a double, so the array's type decides the precision of every operation): a dictionary with unit
    ([3, ...]), s2, dof (`dtype`) and valid (int32)."""
    m = np.asarray(mom, dtype=dtype)
    assert m.shape[0] == PLANES[kind]
    n = 4 if kind else 3
    A = [[None] * n for _ in range(n)]
    B = [[None] * n for _ in range(n)]
    h = [None] * n
    with np.errstate(all="ignore"):
        if kind == 0:
            T = m[P2] / m[S22]
            TT = T * T
            A[0][0], A[1][0], A[1][1] = TT * m[S00], TT * m[S01], TT * m[S11]
            A[2][0], A[2][1], A[2][2] = T * m[S02], T * m[S12], m[S22]
            B[0][0], B[1][0], B[1][1] = TT * m[V00], TT * m[V01], TT * m[V11]
            B[2][0], B[2][1], B[2][2] = T * m[V02], T * m[V12], m[V22]
            h[0] = T * (m[P0] - T * m[S02])
            h[1] = T * (m[P1] - T * m[S12])
            h[2] = m[P2] - T * m[S22]
            rss0 = m[QQ] - m[P2] * T
        else:
            t1, t2, t3, t4, t5, t6 = m[QQ], m[MM22], m[S22], m[AM2], m[P2], m[MM22]
            det = t2 * t3 - t6 * t6
            Kc = (t2 * t5 - t4 * t6) / det
            beta = (t3 * t4 - t5 * t6) / det
            KK, c, bb, kb, bs = Kc * Kc, (2 * Kc) * beta + beta * beta, (beta * beta) * sv, Kc * beta, beta * sv
            A[0][0], A[1][0], A[1][1] = KK * m[S00] + c * m[MM00], KK * m[S01] + c * m[MM01], KK * m[S11] + c * m[MM11]
            A[2][0], A[2][1] = (Kc + beta) * m[MM02], (Kc + beta) * m[MM12]
            A[3][0], A[3][1] = Kc * m[S02] + beta * m[MM02], Kc * m[S12] + beta * m[MM12]
            A[2][2], A[3][2], A[3][3] = m[MM22], m[MM22], m[S22]
            B[0][0] = (KK * m[V00] + kb * (m[NM00] + m[NM00])) + bb * m[MM00]
            B[1][0] = (KK * m[V01] + kb * (m[NM01] + m[NM10])) + bb * m[MM01]
            B[1][1] = (KK * m[V11] + kb * (m[NM11] + m[NM11])) + bb * m[MM11]
            B[2][0], B[2][1] = Kc * m[NM02] + bs * m[MM02], Kc * m[NM12] + bs * m[MM12]
            B[3][0], B[3][1] = Kc * m[V02] + beta * m[NM20], Kc * m[V12] + beta * m[NM21]
            B[2][2], B[3][2], B[3][3] = sv * m[MM22], m[NM22], m[V22]
            h[0] = Kc * ((m[P0] - beta * m[MM02]) - Kc * m[S02]) + beta * ((m[AM0] - beta * m[MM02]) - Kc * m[MM02])
            h[1] = Kc * ((m[P1] - beta * m[MM12]) - Kc * m[S12]) + beta * ((m[AM1] - beta * m[MM12]) - Kc * m[MM12])
            h[2] = (m[AM2] - beta * m[MM22]) - Kc * m[MM22]
            h[3] = (m[P2] - beta * m[MM22]) - Kc * m[S22]
            rss0 = ((((t1 + (beta * beta) * t2) + (Kc * Kc) * t3) - (2 * beta) * t4) - (2 * Kc) * t5) + ((2 * beta) * Kc) * t6
        for i in range(n):
            for j in range(i + 1, n):
                A[i][j], B[i][j] = A[j][i], B[j][i]
        L = [[None] * n for _ in range(n)]
        D = [None] * n
        ok = np.ones(m.shape[1:], dtype=bool)
        for j in range(n):
            D[j] = A[j][j]
            for k in range(j):
                D[j] = D[j] - (L[j][k] * L[j][k]) * D[k]
            ok &= (D[j] > 0.0) & (D[j] < np.inf)
            for i in range(j + 1, n):
                t = A[i][j]
                for k in range(j):
                    t = t - (L[i][k] * L[j][k]) * D[k]
                L[i][j] = t / D[j]
        X = [_ldl_solve(L, D, [B[i][q] for i in range(n)]) for q in range(n)]
        tr = X[0][0]
        for q in range(1, n):
            tr = tr + X[q][q]
        Y0 = _ldl_solve(L, D, [X[q][0] for q in range(n)])
        Y1 = _ldl_solve(L, D, [X[q][1] for q in range(n)])
        d = _ldl_solve(L, D, h)
        hd = h[0] * d[0] + h[1] * d[1]
        for i in range(2, n):
            hd = hd + h[i] * d[i]
        rr = rss0 - hd
        df = float(K) - tr
        rss = np.where(rr > 0.0, rr, 0.0)
        s = rss / df
        ok &= df > 0.0
        for v in (Y0[0], Y1[1], Y1[0], rr, df, s):
            ok &= np.isfinite(v)
    nan = lambda v: np.where(ok, v, np.nan)
    return {"unit": np.stack([nan(Y0[0]), nan(Y1[1]), nan(Y1[0])]), "s2": nan(s), "dof": nan(df), "valid": ok.astype(np.int32)}


def restated(sam, ref, win, Nw, ms, kind, region, shift):
    """moments then solve, in float64: what umpa_sigma_region is to compute (its sums up to rounding)."""
    mom, _ = moments(sam, ref, win, Nw, ms, kind, region, shift)
    out = solve(mom, kind, sam.shape[0], window_sv(win))
    out["moments"] = mom
    return out


def brute(sam, ref, win, Nw, ms, kind, region, shift, pixels):
    """The definition evaluated independently at the listed pixels (xi, xj), in np.longdouble: the Jacobian is formed
    explicitly with the window as it is (no moments, sum w not taken for 1), (beta, K) resp. T come from a weighted
    least-squares call, A is inverted with numpy's inv.  Per pixel a dict unit, s2, dof, cond (of A)."""
    start0, step0, N0, start1, step1, N1 = region
    pad, side, K = Nw + ms, 2 * Nw + 1, sam.shape[0]
    ld = np.longdouble
    w = np.asarray(win, dtype=ld).reshape(side, side)
    out = []
    for xi, xj in pixels:
        ci, cj = start0 + step0 * xi + pad, start1 + step1 * xj + pad
        si, sj = int(shift[0, xi, xj]), int(shift[1, xi, xj])
        a = sam[:, ci - Nw:ci + Nw + 1, cj - Nw:cj + Nw + 1].astype(ld)
        big = ref[:, ci + si - Nw - 1:ci + si + Nw + 2, cj + sj - Nw - 1:cj + sj + Nw + 2].astype(ld)
        r = big[:, 1:-1, 1:-1]
        gi, gj = (big[:, 2:, 1:-1] - big[:, :-2, 1:-1]) / 2, (big[:, 1:-1, 2:] - big[:, 1:-1, :-2]) / 2
        W = np.broadcast_to(w, a.shape)
        mean = lambda f: np.broadcast_to((w * f).sum(axis=(1, 2), keepdims=True), f.shape)
        sq = np.sqrt(W.astype(np.float64)).ravel()
        if kind:
            design = np.stack([mean(r).ravel(), r.ravel()], axis=1).astype(np.float64)
            (beta, Kc), *_ = np.linalg.lstsq(design * sq[:, None], a.ravel().astype(np.float64) * sq, rcond=None)
            beta, Kc = ld(beta), ld(Kc)
            J = np.stack([Kc * gi + beta * mean(gi), Kc * gj + beta * mean(gj), mean(r), r]).reshape(4, -1)
            e = (a - beta * mean(r) - Kc * r).ravel()
        else:
            (T,), *_ = np.linalg.lstsq((r.ravel().astype(np.float64) * sq)[:, None], a.ravel().astype(np.float64) * sq, rcond=None)
            T = ld(T)
            J = np.stack([T * gi, T * gj, r]).reshape(3, -1)
            e = (a - T * r).ravel()
        wf = W.ravel()
        A = (J * wf) @ J.T
        B = (J * wf * wf) @ J.T
        h = (J * wf) @ e
        Ai = np.linalg.inv(A.astype(np.float64))
        C = Ai @ B.astype(np.float64) @ Ai
        rss = max(float((wf * e * e).sum()) - float(h.astype(np.float64) @ Ai @ h.astype(np.float64)), 0.0)
        dof = K - np.trace(Ai @ B.astype(np.float64))
        out.append({"unit": np.array([C[0, 0], C[1, 1], C[0, 1]]), "s2": rss / dof, "dof": dof, "cond": np.linalg.cond(A.astype(np.float64))})
    return out


# ----------------------------------------------------------------------------- the Python front's rules

def shift_field(result, ms):
    """clip(round half away from zero (d), +-(ms - 1)) of dy (rows), dx (columns); SKIP where err != 1 or a map is not finite"""
    dy, dx = np.asarray(result["dy"], dtype=np.float64), np.asarray(result["dx"], dtype=np.float64)
    ok = (np.asarray(result["err"]) == 1) & np.isfinite(dy) & np.isfinite(dx)
    for k in ("f", "T", "df"):
        if k in result:
            ok = ok & np.isfinite(np.asarray(result[k]))
    out = np.full((2,) + dy.shape, SKIP, dtype=np.int32)
    for n, d in enumerate((dy, dx)):
        d = np.where(ok, d, 0.0)
        r = np.clip(np.sign(d) * np.floor(np.abs(d) + 0.5), -(ms - 1), ms - 1).astype(np.int32)
        out[n][ok] = r[ok]
    return out


def sigmas(out, noise_var=None):
    """(sigma_dy, sigma_dx) of a solve result: sqrt((noise_var or s2) * unit)"""
    scale = out["s2"] if noise_var is None else noise_var
    with np.errstate(invalid="ignore"):
        return np.sqrt(scale * out["unit"][0]), np.sqrt(scale * out["unit"][1])


# ----------------------------------------------------------------------------- test stacks

@functools.lru_cache(maxsize=None)
def stack(H, W, K, ms, df, seed=1, noise=0.02, amplitude=None):
    from umpa_amd import synth
    sam, ref, _ = synth.make_stack(H, W, K, ms, df=bool(df), seed=seed, noise=noise, amplitude=ms - 1.2 if amplitude is None else amplitude)
    sam.setflags(write=False)
    ref.setflags(write=False)
    return sam, ref


def random_shift(N0, N1, ms, seed):
    """per-pixel random shifts within the guard, both extremes at the region's corners"""
    rng = np.random.default_rng(seed)
    s = rng.integers(-(ms - 1), ms, size=(2, N0, N1)).astype(np.int32)
    s[:, 0, 0] = -(ms - 1)
    s[:, -1, -1] = ms - 1
    s[0, 0, -1], s[1, 0, -1] = ms - 1, -(ms - 1)
    s[0, -1, 0], s[1, -1, 0] = -(ms - 1), ms - 1
    return s


# ----------------------------------------------------------------------------- the behavioural case: the matchers' scatter

# (name, model, Nw, ms, K, noise on the sample stack, noise on the reference stack, amplitude)
SCATTER_CASES = [
    ("plain_Nw2", "UMPAModelNoDF", 2, 3, 4, 0.03, 0.0, 0.45),
    ("df_Nw3", "UMPAModelDF", 3, 4, 8, 0.02, 0.02, 1.4),
    ("df_Nw2", "UMPAModelDF", 2, 3, 6, 0.01, 0.0, 0.8),
]
SCATTER_M, SCATTER_SIZE, T0 = 100, 64, 0.8


@functools.lru_cache(maxsize=None)
def scatter_case(name):
    """M matches of the CPU checker on a 64 x 64 noise-free stack plus seeded Gaussian noise, and the restatement's
    prediction on the first realisation.  Returns a dict: ratio_dy, ratio_dx (the median over the pixels with err == 1 in
    every realisation, at least pad from the map's border, of predicted sigma / empirical standard deviation, noise_var
    given as sigma_sam^2 + T0^2 sigma_ref^2), s2_ratio (the median of s2 / noise_var) and pixels (how many)."""
    from oracle import cpu_model
    from umpa_amd import synth
    _, cls, Nw, ms, K, ns, nr, amp = [c for c in SCATTER_CASES if c[0] == name][0]
    kind = int(cls == "UMPAModelDF")
    sam0, ref0, _ = synth.make_stack(SCATTER_SIZE, SCATTER_SIZE, K, ms, df=bool(kind), seed=11, noise=0.0, amplitude=amp)
    rng = np.random.default_rng(4242)
    dys, dxs, oks, first = [], [], [], None
    for _m in range(SCATTER_M):
        sam = sam0 + ns * rng.standard_normal(sam0.shape)
        ref = ref0 + nr * rng.standard_normal(ref0.shape) if nr else ref0
        res = getattr(cpu_model.port, cls)(list(sam), list(ref), window_size=Nw, max_shift=ms).match(quiet=True)
        dys.append(res["dy"].copy())
        dxs.append(res["dx"].copy())
        oks.append(res["err"] == 1)
        if first is None:
            first = (sam, ref, {k: np.array(res[k]) for k in ("dx", "dy", "err", "f", "T")})
    pad = Nw + ms
    use = np.all(oks, axis=0)
    inner = np.zeros_like(use)
    inner[pad:-pad, pad:-pad] = True
    use &= inner
    sam, ref, res = first
    region = full_region(sam.shape, Nw, ms)
    out = restated(sam, ref, window(Nw), Nw, ms, kind, region, shift_field(res, ms))
    use &= out["valid"] == 1
    noise_var = ns ** 2 + T0 ** 2 * nr ** 2
    sdy, sdx = sigmas(out, noise_var)
    return {"ratio_dy": float(np.median((sdy / np.std(dys, axis=0))[use])), "ratio_dx": float(np.median((sdx / np.std(dxs, axis=0))[use])),
            "s2_ratio": float(np.median((out["s2"] / noise_var)[use])), "pixels": int(use.sum())}
