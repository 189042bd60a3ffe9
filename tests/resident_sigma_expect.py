"""
tests/resident_sigma_expect.py -- TEST INFRASTRUCTURE: a numpy restatement of the masked definition of include/umpa_grid.h
("Model-resident uncertainty"); the unmasked one is tests/sigma_expect.py's.

moments() restates the header's MOMENTS of a model with masks (in float64, or in np.longdouble together with the header's
rounding bound), solve() its MODEL and SOLVE line by line in float64, brute() is an independent evaluation pixel by pixel
that forms the pair weights and the Jacobian explicitly, fits (beta, K) resp. T by a weighted least-squares call, inverts
with numpy's inv and takes dof = sum w - tr.  masks() builds the test masks, scatter_case() is the behavioural case: the
scatter of the CPU checker's own masked matches over noise realisations.  Nothing here imports umpa_amd.sigma.
"""
import functools

import numpy as np

import sigma_expect as SE

PLANES = (17, 50)
SKIP = SE.SKIP
U = SE.U
PAIRS = SE.PAIRS
NINE = [(i, j) for i in range(3) for j in range(3)]
(S00, S01, S02, S11, S12, S22, V00, V01, V02, V11, V12, V22, P0, P1, P2, QQ, WW) = range(17)
MU0, WM0, NU0, VM0, AU0 = 17, 26, 32, 41, 47                      # the first plane of each dark-field group


def MU(p, q):
    return MU0 + 3 * p + q


def NU(p, q):
    return NU0 + 3 * p + q


def WM(p, q):
    return WM0 + PAIRS.index((min(p, q), max(p, q)))


def VM(p, q):
    return VM0 + PAIRS.index((min(p, q), max(p, q)))


def win_sum(win):
    """the window summed in tap order in doubles (the model's win_sum)"""
    s = 0.0
    for w in np.asarray(win, dtype=np.float64).ravel():
        s = s + float(w)
    return s


# ----------------------------------------------------------------------------- masks

BLOCK_ROWS, BLOCK_COLS = 8, 10


def block_origin(shape, Nw, ms):
    """the frame coordinates of the dead block's first pixel: a few pixels inside the region, off the 32 x 8 tile"""
    pad = Nw + ms
    return pad + 5, pad + 9


@functools.lru_cache(maxsize=None)
def masks(shape, Nw, ms, seed=0):
    """{'binary', 'real'}: [K, H, W] float64 masks, every frame its own.  binary: 10 % random zeros; real: weights in
    [0.2, 1] with 5 % zeros; both with a dead block of 8 x 10 pixels in every frame (block_origin)."""
    rng = np.random.default_rng(900 + seed)
    binary = (rng.random(shape) >= 0.10).astype(np.float64)
    real = (0.2 + 0.8 * rng.random(shape)) * (rng.random(shape) >= 0.05)
    r0, c0 = block_origin(shape, Nw, ms)
    out = {}
    for key, m in (("binary", binary), ("real", real)):
        m[:, r0:r0 + BLOCK_ROWS, c0:c0 + BLOCK_COLS] = 0.0
        m.setflags(write=False)
        out[key] = m
    return out


def dead_pixels(shape, Nw, ms, region):
    """[N0, N1] bool: the pixels whose whole sample window lies in the dead block (no tap has pair weight)"""
    start0, step0, N0, start1, step1, N1 = region
    pad = Nw + ms
    r0, c0 = block_origin(shape, Nw, ms)
    ci = (start0 + step0 * np.arange(N0) + pad)[:, None]
    cj = (start1 + step1 * np.arange(N1) + pad)[None, :]
    return (ci - Nw >= r0) & (ci + Nw < r0 + BLOCK_ROWS) & (cj - Nw >= c0) & (cj + Nw < c0 + BLOCK_COLS)


# ----------------------------------------------------------------------------- MOMENTS

def _fields(sam, ref, mask, Nw, ms, region, shift, dtype):
    """Generator over (k, tap index, a, u = (g_i, g_j, r), p, q) as [N0, N1] arrays of `dtype`; skipped pixels read shift 0."""
    start0, step0, N0, start1, step1, N1 = region
    pad = Nw + ms
    ok = SE.guard(shift, ms)
    si, sj = np.where(ok, shift[0], 0).astype(np.int64), np.where(ok, shift[1], 0).astype(np.int64)
    ci = (start0 + step0 * np.arange(N0) + pad)[:, None] + np.zeros((1, N1), dtype=np.int64)
    cj = (start1 + step1 * np.arange(N1) + pad)[None, :] + np.zeros((N0, 1), dtype=np.int64)
    half = dtype(0.5)
    for k in range(sam.shape[0]):
        A, R, M = sam[k].astype(dtype), ref[k].astype(dtype), mask[k].astype(dtype)
        for x, (di, dj) in enumerate(np.ndindex(2 * Nw + 1, 2 * Nw + 1)):
            ri, rj = ci + si + di - Nw, cj + sj + dj - Nw
            ai, aj = ci + di - Nw, cj + dj - Nw
            a, r = A[ai, aj], R[ri, rj]
            gi, gj = half * (R[ri + 1, rj] - R[ri - 1, rj]), half * (R[ri, rj + 1] - R[ri, rj - 1])
            yield k, x, a, (gi, gj, r), M[ri, rj], M[ai, aj]


def moments(sam, ref, mask, win, Nw, ms, kind, region, shift, dtype=np.float64):
    """[P, N0, N1] planes of the header's masked definition in `dtype` (NaN at skipped pixels) and, for np.longdouble, the
    rounding bound of a double evaluation of each (float64, same shape); (moments, bound-or-None)."""
    N0, N1 = region[2], region[5]
    P, K, T = PLANES[kind], sam.shape[0], (2 * Nw + 1) ** 2
    want_bound = dtype is np.longdouble
    wv = np.asarray(win, dtype=np.float64).ravel()
    ws = dtype(win_sum(win))
    eps = dtype(1e-8)
    m, mag = np.zeros((P, N0, N1), dtype=dtype), np.zeros((P, N0, N1), dtype=dtype)
    per = per_abs = None                                              # 0..2 m_p, 3..5 n_p, 6 m_a, 7 omega, 8 nu, 9..11 sum win u_p
    last = -1

    def fold():
        m[WW] += per[7]
        mag[WW] += per_abs[7]
        if not kind:
            return
        mu, mua = per[9:12] / ws, per_abs[9:12] / ws
        for p, q in NINE:
            m[MU(p, q)] += per[p] * mu[q]
            mag[MU(p, q)] += per_abs[p] * mua[q]
            m[NU(p, q)] += per[3 + p] * mu[q]
            mag[NU(p, q)] += per_abs[3 + p] * mua[q]
        for p, q in PAIRS:
            m[WM(p, q)] += (per[7] * mu[p]) * mu[q]
            mag[WM(p, q)] += (per_abs[7] * mua[p]) * mua[q]
            m[VM(p, q)] += (per[8] * mu[p]) * mu[q]
            mag[VM(p, q)] += (per_abs[8] * mua[p]) * mua[q]
        for p in range(3):
            m[AU0 + p] += per[6] * mu[p]
            mag[AU0 + p] += per_abs[6] * mua[p]

    with np.errstate(invalid="ignore"):
        for k, x, a, u, p, q in _fields(sam, ref, mask, Nw, ms, region, shift, dtype):
            if k != last:
                if last >= 0:
                    fold()
                per, per_abs = np.zeros((12, N0, N1), dtype=dtype), np.zeros((12, N0, N1), dtype=dtype)
                last = k
            w0 = dtype(wv[x])
            c = (p * q) / ((p + q) + eps)
            w = c * w0
            v = w * w
            wa = w * a
            for n, (i, j) in enumerate(PAIRS):
                t = (w * u[i]) * u[j]
                m[S00 + n] += t
                mag[S00 + n] += np.abs(t)
                t = (v * u[i]) * u[j]
                m[V00 + n] += t
                mag[V00 + n] += np.abs(t)
            for i in range(3):
                t = wa * u[i]
                m[P0 + i] += t
                mag[P0 + i] += np.abs(t)
            m[QQ] += wa * a
            mag[QQ] += np.abs(wa * a)
            per[7] += w
            per_abs[7] += np.abs(w)
            if kind:
                for i in range(3):
                    per[i] += w * u[i]
                    per[3 + i] += v * u[i]
                    per[9 + i] += w0 * u[i]
                    per_abs[i] += np.abs(w * u[i])
                    per_abs[3 + i] += np.abs(v * u[i])
                    per_abs[9 + i] += np.abs(w0 * u[i])
                per[6] += wa
                per_abs[6] += np.abs(wa)
                per[8] += v
                per_abs[8] += np.abs(v)
        fold()
    ok = SE.guard(shift, ms)
    m[:, ~ok] = np.nan
    if not want_bound:
        return m, None
    factor = np.full(P, (K * T + 16) * U)
    factor[17:] = (3 * T + K + 20) * U
    bound = (factor[:, None, None] * mag).astype(np.float64)
    bound[:, ~ok] = np.nan
    return m, bound


# ----------------------------------------------------------------------------- MODEL and SOLVE

def solve(mom, kind):
    """MODEL and SOLVE of the header's masked definition on [P, ...] moments, expression by expression, in float64: a
    dictionary with unit ([3, ...]), s2, dof (float64) and valid (int32)."""
    m = np.asarray(mom, dtype=np.float64)
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
            t1, t2, t3, t4, t5, t6 = m[QQ], m[WM(2, 2)], m[S22], m[AU0 + 2], m[P2], m[MU(2, 2)]
            det = t2 * t3 - t6 * t6
            Kc = (t2 * t5 - t4 * t6) / det
            beta = (t3 * t4 - t5 * t6) / det
            KK, kb, bb = Kc * Kc, Kc * beta, beta * beta
            S = {(0, 0): S00, (0, 1): S01, (1, 1): S11, (0, 2): S02, (1, 2): S12}
            V = {k: v + 6 for k, v in S.items()}
            for (p, q) in ((0, 0), (0, 1), (1, 1)):
                A[q][p] = (KK * m[S[p, q]] + kb * (m[MU(p, q)] + m[MU(q, p)])) + bb * m[WM(p, q)]
                B[q][p] = (KK * m[V[p, q]] + kb * (m[NU(p, q)] + m[NU(q, p)])) + bb * m[VM(p, q)]
            for p in (0, 1):
                A[2][p] = Kc * m[MU(p, 2)] + beta * m[WM(p, 2)]
                A[3][p] = Kc * m[S[p, 2]] + beta * m[MU(2, p)]
                B[2][p] = Kc * m[NU(p, 2)] + beta * m[VM(p, 2)]
                B[3][p] = Kc * m[V[p, 2]] + beta * m[NU(2, p)]
                h[p] = Kc * ((m[P0 + p] - beta * m[MU(p, 2)]) - Kc * m[S[p, 2]]) + beta * ((m[AU0 + p] - beta * m[WM(p, 2)]) - Kc * m[MU(2, p)])
            A[2][2], A[3][2], A[3][3] = m[WM(2, 2)], m[MU(2, 2)], m[S22]
            B[2][2], B[3][2], B[3][3] = m[VM(2, 2)], m[NU(2, 2)], m[V22]
            h[2] = (m[AU0 + 2] - beta * m[WM(2, 2)]) - Kc * m[MU(2, 2)]
            h[3] = (m[P2] - beta * m[MU(2, 2)]) - Kc * m[S22]
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
        X = [SE._ldl_solve(L, D, [B[i][q] for i in range(n)]) for q in range(n)]
        tr = X[0][0]
        for q in range(1, n):
            tr = tr + X[q][q]
        Y0 = SE._ldl_solve(L, D, [X[q][0] for q in range(n)])
        Y1 = SE._ldl_solve(L, D, [X[q][1] for q in range(n)])
        d = SE._ldl_solve(L, D, h)
        hd = h[0] * d[0] + h[1] * d[1]
        for i in range(2, n):
            hd = hd + h[i] * d[i]
        rr = rss0 - hd
        df = m[WW] - tr
        rss = np.where(rr > 0.0, rr, 0.0)
        s = rss / df
        ok &= df > 0.0
        for v in (Y0[0], Y1[1], Y1[0], rr, df, s):
            ok &= np.isfinite(v)
    nan = lambda v: np.where(ok, v, np.nan)
    return {"unit": np.stack([nan(Y0[0]), nan(Y1[1]), nan(Y1[0])]), "s2": nan(s), "dof": nan(df), "valid": ok.astype(np.int32)}


def restated(sam, ref, mask, win, Nw, ms, kind, region, shift):
    """moments then solve, in float64: what umpa_grid_uncertainty is to compute on a masked model (its sums up to rounding)."""
    mom, _ = moments(sam, ref, mask, win, Nw, ms, kind, region, shift)
    out = solve(mom, kind)
    out["moments"] = mom
    return out


def brute(sam, ref, mask, win, Nw, ms, kind, region, shift, pixels):
    """The masked definition evaluated independently at the listed pixels (xi, xj), in np.longdouble: the pair weights and
    the Jacobian are formed explicitly (no moments), (beta, K) resp. T come from a weighted least-squares call, A is inverted
    with numpy's inv, dof = sum w - tr(A^-1 B).  Per pixel a dict unit, s2, dof, cond (of A), weight (sum w), taps (how many
    taps of all frames carry weight); None where the window has no pair weight."""
    start0, step0, N0, start1, step1, N1 = region
    pad, side = Nw + ms, 2 * Nw + 1
    ld = np.longdouble
    w0 = np.asarray(win, dtype=ld).reshape(side, side)
    wsum = w0.sum()
    out = []
    for xi, xj in pixels:
        ci, cj = start0 + step0 * xi + pad, start1 + step1 * xj + pad
        si, sj = int(shift[0, xi, xj]), int(shift[1, xi, xj])
        a = sam[:, ci - Nw:ci + Nw + 1, cj - Nw:cj + Nw + 1].astype(ld)
        big = ref[:, ci + si - Nw - 1:ci + si + Nw + 2, cj + sj - Nw - 1:cj + sj + Nw + 2].astype(ld)
        q = mask[:, ci - Nw:ci + Nw + 1, cj - Nw:cj + Nw + 1].astype(ld)
        p = mask[:, ci + si - Nw:ci + si + Nw + 1, cj + sj - Nw:cj + sj + Nw + 1].astype(ld)
        r = big[:, 1:-1, 1:-1]
        gi, gj = (big[:, 2:, 1:-1] - big[:, :-2, 1:-1]) / 2, (big[:, 1:-1, 2:] - big[:, 1:-1, :-2]) / 2
        Wt = (p * q) / (p + q + ld(1e-8)) * w0
        if not (Wt > 0).any():
            out.append(None)
            continue
        mean = lambda f: np.broadcast_to((w0 * f).sum(axis=(1, 2), keepdims=True) / wsum, f.shape)   # the UNMASKED mean
        sq = np.sqrt(Wt.astype(np.float64)).ravel()
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
        wf = Wt.ravel()
        A = (J * wf) @ J.T
        B = (J * wf * wf) @ J.T
        h = (J * wf) @ e
        Ai = np.linalg.inv(A.astype(np.float64))
        C = Ai @ B.astype(np.float64) @ Ai
        rss = max(float((wf * e * e).sum()) - float(h.astype(np.float64) @ Ai @ h.astype(np.float64)), 0.0)
        dof = float(wf.sum()) - np.trace(Ai @ B.astype(np.float64))
        out.append({"unit": np.array([C[0, 0], C[1, 1], C[0, 1]]), "s2": rss / dof, "dof": dof, "cond": np.linalg.cond(A.astype(np.float64)),
                    "weight": float(wf.sum()), "taps": int((wf > 0).sum())})
    return out


# ----------------------------------------------------------------------------- the behavioural case: the masked matchers' scatter

SCATTER_NAMES = ("plain_Nw2", "df_Nw3")
SCATTER_MASKS = ("binary", "real")


@functools.lru_cache(maxsize=None)
def scatter_case(name, which):
    """sigma_expect.scatter_case with mask_list=: M matches of the CPU checker on a 64 x 64 noise-free stack plus seeded
    Gaussian noise under the mask `which` (no dead block: every pixel keeps weight), and the masked restatement's prediction
    on the first realisation.  The same dictionary: ratio_dy, ratio_dx, s2_ratio, pixels."""
    from oracle import cpu_model
    from umpa_amd import synth
    _, cls, Nw, ms, K, ns, nr, amp = [c for c in SE.SCATTER_CASES if c[0] == name][0]
    kind = int(cls == "UMPAModelDF")
    size = SE.SCATTER_SIZE
    sam0, ref0, _ = synth.make_stack(size, size, K, ms, df=bool(kind), seed=11, noise=0.0, amplitude=amp)
    mrng = np.random.default_rng(77)
    shape = sam0.shape
    mask = (mrng.random(shape) >= 0.10).astype(np.float64) if which == "binary" else \
        (0.2 + 0.8 * mrng.random(shape)) * (mrng.random(shape) >= 0.05)
    rng = np.random.default_rng(4242)
    dys, dxs, oks, first = [], [], [], None
    for _m in range(SE.SCATTER_M):
        sam = sam0 + ns * rng.standard_normal(sam0.shape)
        ref = ref0 + nr * rng.standard_normal(ref0.shape) if nr else ref0
        res = getattr(cpu_model.port, cls)(list(sam), list(ref), mask_list=list(mask), window_size=Nw, max_shift=ms).match(quiet=True)
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
    region = SE.full_region(sam.shape, Nw, ms)
    out = restated(sam, ref, mask, SE.window(Nw), Nw, ms, kind, region, SE.shift_field(res, ms))
    use &= out["valid"] == 1
    noise_var = ns ** 2 + SE.T0 ** 2 * nr ** 2
    sdy, sdx = SE.sigmas(out, noise_var)
    return {"ratio_dy": float(np.median((sdy / np.std(dys, axis=0))[use])), "ratio_dx": float(np.median((sdx / np.std(dxs, axis=0))[use])),
            "s2_ratio": float(np.median((out["s2"] / noise_var)[use])), "pixels": int(use.sum())}
