"""
What the tests of the scale-space search (umpa_grid_levels_track, umpa_amd.levels) share: the kernels the library must
have, the selection rule as a loop over pixels, the chain of separate track() calls a level must equal, and the use case's
pixel set, decided on the CPU in extended precision (tests/widen_expect.py).
"""
import functools
import itertools

import numpy as np

import grid_expect as GE
import widen_expect as WE

WIDTHS = (1, 2, 4, 8)
# the ten two- and three-element subsets of the widened half-widths, widest first
SUBSETS = [tuple(sorted(c, reverse=True)) for n in (2, 3) for c in itertools.combinations(WIDTHS, n)]
TABLE_KERNELS = ["levels_table_kernel<%d, %d, %d, %s>" % (s[0], s[1], s[2] if len(s) > 2 else 0, strip)
                 for s in SUBSETS for strip in ("false", "true")]
KERNELS = TABLE_KERNELS + ["levels_prior_kernel", "levels_select_kernel"]


def table_kernel(levels, strip):
    """the pooling kernel a list of levels reaches (None: one widened level, widen_table_kernel's)"""
    wide = [b for b in levels if b > 0]
    if len(wide) < 2:
        return None
    return "levels_table_kernel<%d, %d, %d, %s>" % (wide[0], wide[1], wide[2] if len(wide) > 2 else 0, "true" if strip else "false")


def brute_select(dx, dy, err, tol):
    """The rule of include/umpa_grid.h as a loop: dx, dy, err of shape [L, N0, N1], tol of L numbers -> level [N0, N1]."""
    L, N0, N1 = dx.shape
    level = np.full((N0, N1), -1, np.int32)
    for i in range(N0):
        for j in range(N1):
            ok = [err[l, i, j] == 1 and np.isfinite(dx[l, i, j]) and np.isfinite(dy[l, i, j]) for l in range(L)]
            for l in range(L):
                if not ok[l]:
                    continue
                good = True
                for m in range(l):
                    if ok[m] and not (abs(np.float64(dx[l, i, j]) - np.float64(dx[m, i, j])) <= tol[m]
                                      and abs(np.float64(dy[l, i, j]) - np.float64(dy[m, i, j])) <= tol[m]):
                        good = False
                if good:
                    level[i, j] = l
    return level


def cut(a, src, dst):
    """the pixels of region `dst` out of a map of region `src` (pairs of (start, end, step) triples of one grid; last two axes)"""
    s = []
    for p, q in zip(src, dst):
        assert p[2] == q[2] and (q[0] - p[0]) % p[2] == 0 and q[0] >= p[0]
        first = (q[0] - p[0]) // p[2]
        n = len(range(*q))
        assert first + n <= len(range(*p))
        s.append(slice(first, first + n))
    return a[(Ellipsis,) + tuple(s)]


def chain(m, levels, lam=None, radius=None, **region):
    """The levels as separate calls: track(widen=levels[0]) with an all-NaN prior, then track(widen=b) with prior_from the
    level before, laid into the level's own region (umpa_amd.widen.coarse_to_fine with its first level as a track result,
    on any region)."""
    from umpa_amd import widen
    from umpa_amd.track import prior_from
    out = []
    for n, b in enumerate(levels):
        reg = widen.valid_region(m, b, **region)
        if n == 0:
            pdx = pdy = np.full((len(range(*reg[0])), len(range(*reg[1]))), np.nan)
        else:
            pdx, pdy = (widen.embed(p, out[-1]["region"], reg) for p in prior_from(out[-1]))
        res = m.track(pdx, pdy, lam=lam, radius=radius, widen=b, **region)
        res.setdefault("region", reg)
        out.append(res)
    return out


def _sure_basin(sam, ref, Nw, ms, b, true):
    """the true shift lies below each of its eight neighbours by more than the two bounds (a basin for any fp64 evaluation
    within its bound), over the pixels whose widened window fits"""
    v = WE.volumes(0, sam, ref, Nw, b, ms, "sam") if b else GE.hp_volumes(0, sam, ref, GE.window(Nw), ms, ms + Nw, "sam")
    a, c = true[0] + ms - 1, true[1] + ms - 1
    ok = np.ones(v["cost"].shape[2:], bool)
    for da in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if da or dc:
                ok &= (v["cost"][a + da, c + dc] - v["bound"][a + da, c + dc]) > (v["cost"][a, c] + v["bound"][a, c])
    return ok


USE_LEVELS = (4, 2, 1, 0)


@functools.lru_cache(maxsize=None)
def use_case():
    """(USE, sam, ref, known, sure): the aliased stack of tests/test_hip_basins.py and, over its whole extent, the pixels
    where the true shift is sure at every level of USE_LEVELS -- the global minimum beyond the bounds under the widest
    window (widen_expect.use_case_sure), a basin beyond the bounds at every narrower level -- so that a chain of nearest-basin
    searches that starts on the true shift stays on it whatever fp64 evaluation within its bound decides."""
    from nativelibs import gpu_test_module
    mod = gpu_test_module("basins")
    sam, ref, known = mod._use_case()
    u = mod.USE
    Nw, ms, true = u["Nw"], u["ms"], u["true"]
    N0, N1 = known.shape
    sure = np.zeros((N0, N1), bool)
    b0 = USE_LEVELS[0]
    sure[b0:N0 - b0, b0:N1 - b0] = WE.use_case_sure(sam, ref, Nw, ms, b0, true)
    for b in USE_LEVELS[1:]:
        inside = np.zeros((N0, N1), bool)
        inside[b:N0 - b, b:N1 - b] = _sure_basin(sam, ref, Nw, ms, b, true)
        sure &= inside
    return u, sam, ref, known, sure
