"""
tests/widen_expect.py -- what window widening must return, built WITHOUT the code under test.

``widen=b`` (include/umpa_grid.h) pools the shift table and the maps over the (2b + 1)^2 dense pixels around a pixel; every
pooled quantity is linear in the window, so the costs are those of the reference model whose window is

    W' = (w (*) box_B) / B^2,   B = 2b + 1,   w the model's normalised Hamming window.

Here: ``window`` (W' by explicit shifted sums, not by the convolution umpa_amd.widen uses), ``pooled_cells`` (the box mean of
per-pixel extended-precision sums, solved once: the route the device takes, in longdouble), ``scale`` (the fp64 bound of the
pooled route against oracle/hp_cost.py's), ``volumes`` (hp_cost's volumes under W' with that bound) and the near-tie share.
"""
import functools

import numpy as np

import grid_expect as GE

LD = np.longdouble
BS = (1, 2, 4)                                 # the half-widths of the GPU tests on grid_expect.STACKS["64x72x3"]
CASES = [("64x72x3", b) for b in BS] + [("96x112x4", 2)]


def window(Nw, b):
    """W' from numpy.hamming by shifted sums: W'[a, c] = sum over the box offsets of w[a - da, c - dc], over B^2."""
    h = np.hamming(2 * Nw + 1)
    w = np.multiply.outer(h, h)
    w = w / w.sum()
    S, B = 2 * (Nw + b) + 1, 2 * b + 1
    out = np.zeros((S, S), dtype=LD)
    for da in range(B):
        for dc in range(B):
            out[da:da + 2 * Nw + 1, dc:dc + 2 * Nw + 1] += w.astype(LD)
    return np.ascontiguousarray((out / LD(B * B)).astype(np.float64))


def scale(Na, Nw, b):
    """n_pool / n_direct: how much larger the a-priori fp64 error of the pooled route is than that of a direct fp64
    evaluation under W', whose bound oracle/hp_cost.hp_cells returns with n_direct = Na (2 (Nw + b) + 1)^2 + 8 summands.

    The pooled route forms each windowed sum as B^2 sums of Na (2 Nw + 1)^2 terms (the per-pixel sums: at most that many
    roundings each, in any order), adds those B^2 numbers (B^2 more roundings at most), and then, c = 3:
      1  rB = 1 / B^2 is itself rounded (B^2 is no power of two);
      1  the product V * rB is rounded;
      1  the reference's W' is rounded to fp64 entry by entry, where the pooled route applies the exact box to w: the two
         sides differ by a relative 2^-53 per term, which is one more rounding of every sum.
    The solve's roundings (the 8 of hp_cells) are not counted again: Na B^2 (2 Nw + 1)^2 counts every term of a sum once
    per block pixel, far more often than n_direct does, which covers them many times over.
    n_pool = Na B^2 (2 Nw + 1)^2 + B^2 + 3."""
    B = 2 * b + 1
    n_pool = Na * B * B * (2 * Nw + 1) ** 2 + B * B + 3
    n_direct = Na * (2 * (Nw + b) + 1) ** 2 + 8
    return LD(n_pool) / LD(n_direct)


def volumes(kind, sam, ref, Nw, b, ms, assign, pixels=None):
    """grid_expect.hp_volumes under W' over the pixels whose widened window fits (pad = ms + Nw + b), its bound scaled."""
    v = GE.hp_volumes(kind, sam, ref, window(Nw, b), ms, ms + Nw + b, assign, pixels)
    v["bound"] = v["bound"] * scale(np.asarray(sam).shape[0], Nw, b)
    return v


@functools.lru_cache(maxsize=None)
def volumes_for(name, b, kind, assign):
    sam, ref, c = GE.stack(name)
    return volumes(kind, sam, ref, c["Nw"], b, c["ms"], assign)


def near_tie_share(v):
    return float(GE.near_tie(v["cost"], v["bound"]).mean())


def pooled_cells(kind, sam, ref, Nw, b, pi, pj, si, sj, assign="sam"):
    """cost, T, df of (pixel, shift) pairs the way the device forms them, in longdouble: the per-pixel sums of the model's
    own window w (t1, t3, t5, per frame W[s_k] and mean_k) at every pixel of the (2b + 1)^2 block, their mean, one solve."""
    from oracle import hp_cost
    sam, ref = np.asarray(sam, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    K, S, B = sam.shape[0], 2 * Nw + 1, 2 * b + 1
    w = GE.window(Nw).astype(LD)[None, None]
    pi, pj, si, sj = (np.asarray(v, dtype=np.int64).ravel() for v in (pi, pj, si, sj))
    acc = {k: 0 for k in ("t1", "t3", "t5", "ws", "mr")}
    for da in range(-b, b + 1):
        for dc in range(-b, b + 1):
            i, j = pi + da, pj + dc
            if assign == "ref":
                ri, rj, qi, qj = i, j, i - si, j - sj
            else:
                ri, rj, qi, qj = i + si, j + sj, i, j
            R = hp_cost._windows(ref, ri - Nw, rj - Nw, S)
            Q = hp_cost._windows(sam, qi - Nw, qj - Nw, S)
            acc["t1"] = acc["t1"] + (w * Q * Q).sum(axis=(1, 2, 3))
            acc["t3"] = acc["t3"] + (w * R * R).sum(axis=(1, 2, 3))
            acc["t5"] = acc["t5"] + (w * R * Q).sum(axis=(1, 2, 3))
            acc["ws"] = acc["ws"] + (w * Q).sum(axis=(2, 3))
            acc["mr"] = acc["mr"] + (w * R).sum(axis=(2, 3)) / w.sum()
    t1, t3, t5, ws, mr = (acc[k] / LD(B * B) for k in ("t1", "t3", "t5", "ws", "mr"))
    wt = LD(K)
    if kind == 1:
        t2 = (mr * mr).sum(axis=1)
        t4 = (mr * ws).sum(axis=1)
        t6 = w.sum() * t2
        det = t2 * t3 - t6 * t6
        Kc, beta = (t2 * t5 - t4 * t6) / det, (t3 * t4 - t5 * t6) / det
        T = beta + Kc
        # df = Kc / T, and Kc's numerator t2 t5 - t4 t6 cancels where the dark-field is weak: its condition number
        cond = (np.abs(t2 * t5) + np.abs(t4 * t6)) / np.abs(t2 * t5 - t4 * t6)
        return dict(cost=(t1 + beta * beta * t2 + Kc * Kc * t3 - 2 * beta * t4 - 2 * Kc * t5 + 2 * beta * Kc * t6) / wt, T=T, df=Kc / T, df_cond=cond)
    T = t5 / t3
    return dict(cost=(t1 - t5 * T) / wt, T=T, df=None)


# ----------------------------------------------------------------------------- the use case (tests/test_hip_basins.py::_use_case)

def use_case_sure(sam, ref, Nw, ms, b, true=(1, 1), assign="sam"):
    """For the aliased stack: (sure, valid shape).  `sure[xi, xj]`: the extended-precision cost under W' of the true shift
    lies below that of every other shift by more than the two (scaled) fp64 bounds, so any fp64 evaluation within its
    bound finds the true shift.  Over the pixels whose widened window fits (pad = ms + Nw + b)."""
    v = volumes(0, sam, ref, Nw, b, ms, assign) if b else GE.hp_volumes(0, sam, ref, GE.window(Nw), ms, ms + Nw, assign)
    U = 2 * ms - 1
    c, bd = v["cost"].reshape((U * U,) + v["cost"].shape[2:]), v["bound"].reshape((U * U,) + v["cost"].shape[2:])
    t = (true[0] + ms - 1) * U + (true[1] + ms - 1)
    other = np.ones(U * U, bool)
    other[t] = False
    return ((c[other] - bd[other]) > (c[t] + bd[t])[None]).all(axis=0)
