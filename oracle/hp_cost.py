"""
oracle/hp_cost.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The windowed least-squares cost of one (pixel, shift) pair in ``numpy.longdouble`` (x87 extended precision, eps
1.1e-19), written from the formulas oracle/umpa_oracle.c cites (lib/Model.cpp:359-509 without dark-field, :631-862
with it; the pair weight of masked models is lib/Utils.cpp:125-130).  It evaluates the same expanded sums as every
implementation in this repository, so its own rounding error is about 2^-11 of an fp64 evaluation's: a yardstick
that does not depend on two fp64 implementations agreeing in the last bit.

    hp_cost(kind, sam, ref, win, i, j, si, sj, assign, mask=None) -> (cost, T, df)
    hp_cells(...)   the same for arrays of pixels and shifts, also returning the a-priori fp64 error bound
    hp_volume(...)  the whole (2 max_shift - 1)^2 cost volume of a small image

``(i, j)`` are image coordinates (padding included), ``(si, sj)`` the row / column shift, ``assign`` 'sam' or 'ref'
(which window stays at the pixel).  ``df`` is None for the model without dark-field.

The a-priori bound: an fp64 evaluation of the formula, in ANY summation order, differs from the exact value by at most
    n 2^-53 (|t1| + beta^2 t2 + K^2 t3 + 2 |beta t4| + 2 |K t5| + 2 |beta K t6|) / wt          (dark-field)
    n 2^-53 (t1 + |t5 T|) / wt                                                                  (without)
with n = Na (2 Nw + 1)^2 + 8 summands (first order; errors of beta, K and T enter the cost only in second order
because the cost is stationary in them).
"""
import numpy as np

LD = np.longdouble
KIND_NODF, KIND_DF = 0, 1
CHUNK = 2048


def _windows(stack, top, left, S):
    """[n, K, S, S] windows of a [K, H, W] stack whose upper left corners are (top[n], left[n])."""
    a = np.arange(S)
    rows = (top[:, None] + a[None, :])[:, None, :, None]
    cols = (left[:, None] + a[None, :])[:, None, None, :]
    return stack[np.arange(stack.shape[0])[None, :, None, None], rows, cols].astype(LD)


def hp_cells(kind, sam, ref, win, pi, pj, si, sj, assign="sam", mask=None):
    """Extended-precision cost, transmission, dark-field and the fp64 bound for n (pixel, shift) pairs: integer arrays
    ``pi, pj`` (image coordinates) and ``si, sj``.  All frames at position (0, 0), every frame contributes.
    Returns a dict of longdouble arrays: cost, T, df (DF only), bound, df_bound (DF only: the a-priori RELATIVE bound of df)."""
    sam, ref = np.asarray(sam, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    K = sam.shape[0]
    S = win.shape[0]
    Nw = (S - 1) // 2
    pi, pj, si, sj = (np.asarray(v, dtype=np.int64).ravel() for v in (pi, pj, si, sj))
    w = np.asarray(win, dtype=np.float64).astype(LD)[None, None]
    out = {k: [] for k in ("cost", "T", "df", "bound", "df_bound")}
    for a in range(0, pi.size, CHUNK):
        i, j, di, dj = pi[a:a + CHUNK], pj[a:a + CHUNK], si[a:a + CHUNK], sj[a:a + CHUNK]
        if assign == "ref":                                   # lib/Model.cpp:408-421: the reference window stays
            ri, rj, qi, qj = i, j, i - di, j - dj
        else:
            ri, rj, qi, qj = i + di, j + dj, i, j
        R = _windows(ref, ri - Nw, rj - Nw, S)
        Q = _windows(sam, qi - Nw, qj - Nw, S)
        ww = w
        if mask is not None:
            m = np.asarray(mask, dtype=np.float64)
            MR, MQ = _windows(m, ri - Nw, rj - Nw, S), _windows(m, qi - Nw, qj - Nw, S)
            ww = w * (MR * MQ / (MR + MQ + LD(1e-8)))         # 1e-8 as the fp64 constant the reference adds
            wt = ww.sum(axis=(1, 2, 3))
        else:
            wt = LD(K)
        t1 = (ww * Q * Q).sum(axis=(1, 2, 3))
        t3 = (ww * R * R).sum(axis=(1, 2, 3))
        t5 = (ww * R * Q).sum(axis=(1, 2, 3))
        if kind == KIND_DF:
            mean = (w * R).sum(axis=(2, 3)) / w.sum()         # [n, K], never mask-weighted (lib/Model.cpp:723-739)
            s2, s4, s6 = ww.sum(axis=(2, 3)), (ww * Q).sum(axis=(2, 3)), (ww * R).sum(axis=(2, 3))
            t2 = (mean * mean * s2).sum(axis=1) if mask is not None else (mean * mean).sum(axis=1)
            t4 = (mean * s4).sum(axis=1)
            t6 = (mean * s6).sum(axis=1)
            det = t2 * t3 - t6 * t6
            Kc = (t2 * t5 - t4 * t6) / det
            beta = (t3 * t4 - t5 * t6) / det
            T = beta + Kc
            out["df"].append(Kc / T)
            # df = K / (beta + K) = N_K / (N_beta + N_K) with N_K = t2 t5 - t4 t6, N_beta = t3 t4 - t5 t6 (det cancels): where a
            # numerator cancels -- df crosses zero, or the contrast is low -- no fp64 evaluation has a relative accuracy to be
            # held to.  First order, any summation order, with the sums of |terms| for data of mixed sign:
            a5, a4, a6 = (ww * np.abs(R * Q)).sum(axis=(1, 2, 3)), (np.abs(mean) * (ww * np.abs(Q)).sum(axis=(2, 3))).sum(axis=1), \
                (np.abs(mean) * (ww * np.abs(R)).sum(axis=(2, 3))).sum(axis=1)
            nk, nb = t2 * t5 - t4 * t6, t3 * t4 - t5 * t6
            nu = (K * S * S + S * S + 8) * LD(2.0) ** -53
            ek = nu * (t2 * np.abs(t5) + t2 * a5 + a4 * np.abs(t6) + np.abs(t4) * a6)
            eb = nu * (t3 * np.abs(t4) + t3 * a4 + a5 * np.abs(t6) + np.abs(t5) * a6)
            out["df_bound"].append(ek / np.abs(nk) + (ek + eb) / np.abs(nk + nb) + 3 * LD(2.0) ** -53)
            cost = (t1 + beta * beta * t2 + Kc * Kc * t3 - 2 * beta * t4 - 2 * Kc * t5 + 2 * beta * Kc * t6) / wt
            mag = np.abs(t1) + beta * beta * t2 + Kc * Kc * t3 + 2 * np.abs(beta * t4) + 2 * np.abs(Kc * t5) + 2 * np.abs(beta * Kc * t6)
        else:
            T = t5 / t3
            cost = (t1 - t5 * T) / wt
            mag = t1 + np.abs(t5 * T)
        n = K * S * S + 8
        out["cost"].append(cost)
        out["T"].append(T)
        out["bound"].append(n * LD(2.0) ** -53 * mag / wt)
    return {k: np.concatenate(v) if v else None for k, v in out.items()}


def hp_cost(kind, sam, ref, win, i, j, si, sj, assign="sam", mask=None):
    r = hp_cells(kind, sam, ref, win, [i], [j], [si], [sj], assign, mask)
    return r["cost"][0], r["T"][0], (r["df"][0] if r["df"] is not None else None)


def hp_volume(kind, sam, ref, win, max_shift, padding, assign="sam", mask=None):
    """cost[si + ms - 1, sj + ms - 1, xi, xj] for every shift inside the search box and every output pixel of a (small)
    image: the extent is shape - 2 padding, pixel (xi, xj) is image pixel (padding + xi, padding + xj)."""
    H, W = np.asarray(sam).shape[1:]
    N0, N1 = H - 2 * padding, W - 2 * padding
    U = 2 * max_shift - 1
    sh, sw, xi, xj = np.meshgrid(np.arange(U) - max_shift + 1, np.arange(U) - max_shift + 1,
                                 np.arange(N0) + padding, np.arange(N1) + padding, indexing="ij")
    r = hp_cells(kind, sam, ref, win, xi, xj, sh, sw, assign, mask)
    return r["cost"].reshape(U, U, N0, N1)


def memo_cells(res, pad, org=(0, 0), step=1):
    """The known cells of a result's 5x5 memo (``debug_d``, sub_pixel_mode 0) as (index arrays into debug_d, image
    pixel, shift): cell 5 r + c of a converged pixel is the cost at the shift (dy - 2 + r, dx - 2 + c) -- rows first
    (oracle/umpa_oracle.c ``minimise``: memo[CENTRE +- 5] are the row neighbours, +- 1 the column neighbours; dy = uv[0]
    is the row shift, dx = uv[1] the column shift).  Only err == 1 pixels: a failed walk's dx, dy are not its memo's centre."""
    d = res["debug_d"]
    known = (d >= 0) & (res["err"] == 1)[..., None]
    xi, xj, q = np.nonzero(known)
    ci = np.rint(res["dy"][xi, xj]).astype(np.int64)
    cj = np.rint(res["dx"][xi, xj]).astype(np.int64)
    return (xi, xj, q), (pad + org[0] + step * xi, pad + org[1] + step * xj), (ci - 2 + q // 5, cj - 2 + q % 5)


def to_mp(x):
    """An exact mpmath value of a longdouble (two fp64 pieces)."""
    import mpmath
    hi = np.float64(x)
    lo = np.float64(x - LD(hi))
    return mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))


def mp_cost(kind, sam, ref, win, i, j, si, sj, assign="sam", mask=None, dps=50):
    """The same formula with mpmath at ``dps`` digits, plain loops (validation of hp_cells on a few points)."""
    import mpmath
    mpmath.mp.dps = dps
    f = lambda v: mpmath.mpf(float(v))
    K, S = len(sam), win.shape[0]
    Nw = (S - 1) // 2
    ri, rj, qi, qj = (i, j, i - si, j - sj) if assign == "ref" else (i + si, j + sj, i, j)
    t1 = t2 = t3 = t4 = t5 = t6 = mpmath.mpf(0)
    wt = mpmath.mpf(0) if mask is not None else mpmath.mpf(K)
    wsum = sum(f(win[a, b]) for a in range(S) for b in range(S))
    for k in range(K):
        mean = sum(f(win[a, b]) * f(ref[k][ri - Nw + a, rj - Nw + b]) for a in range(S) for b in range(S)) / wsum
        s2 = s4 = s6 = mpmath.mpf(0)
        for a in range(S):
            for b in range(S):
                w, q, r = f(win[a, b]), f(sam[k][qi - Nw + a, qj - Nw + b]), f(ref[k][ri - Nw + a, rj - Nw + b])
                if mask is not None:
                    ma, mb = f(mask[k][ri - Nw + a, rj - Nw + b]), f(mask[k][qi - Nw + a, qj - Nw + b])
                    w = w * (ma * mb / (ma + mb + f(1e-8)))
                    wt += w
                t1 += w * q * q; t3 += w * r * r; t5 += w * r * q
                s2 += w; s4 += w * q; s6 += w * r
        if kind == KIND_DF:
            t2 += mean * mean * s2 if mask is not None else mean * mean
            t4 += mean * s4
            t6 += mean * s6
    if kind == KIND_DF:
        det = t2 * t3 - t6 * t6
        Kc, beta = (t2 * t5 - t4 * t6) / det, (t3 * t4 - t5 * t6) / det
        T = beta + Kc
        return (t1 + beta * beta * t2 + Kc * Kc * t3 - 2 * beta * t4 - 2 * Kc * t5 + 2 * beta * Kc * t6) / wt, T, Kc / T
    T = t5 / t3
    return (t1 - t5 * T) / wt, T, None
