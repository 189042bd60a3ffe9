// umpa_levels_geom.h -- scale-space search (include/umpa_grid.h): the level list and the uniform-lag row arithmetic.  Plain
// C++ with no HIP type in it, as umpa_widen_geom.h, so that the host program tests/levels_addr_check.cpp can sweep every
// address on the CPU under the sanitizers; the kernels of umpa_levels_kernels.h and the host code call the same functions.
//
// All levels lag by bmax = b[0]: a call pools the dense rows [drow0 - bmax, drow0 + drows - bmax) -- widen_rows at bmax --
// for EVERY level, from the chunk and a carry of the previous chunk's last 2 bmax raw rows (WidenGeom with b = bmax: the
// carry, widen_src and widen_carry_copy are window widening's own).  Level l's rows are then finished in the same call as
// level l - 1's, which are its prior.  A level of half-width b < bmax reads the raw rows r - b .. r + b of a pooled row r,
// inside r - bmax .. r + bmax; the level 0 (the model's own window) reads raw row r itself, from the carry where r < drow0.
#pragma once
#include "umpa_widen_geom.h"

#define UMPA_LEVELS_MAX 4                                            // UMPA_GRID_MAX_LEVELS

namespace umpa {

// The list: L half-widths, strictly decreasing, the widened ones from {1, 2, 4, 8} and at most three, a 0 only at the end.
// 0: good; 1: L out of range; 2: the list.
UMPA_WIDEN_HD inline int levels_check(int L, const int* b)
{
    if (L < 1 || L > UMPA_LEVELS_MAX) return 1;
    int wide = 0;
    for (int l = 0; l < L; l++) {
        const int v = b[l];
        if (!(v == 8 || v == 4 || v == 2 || v == 1 || (v == 0 && l == L - 1))) return 2;
        if (l > 0 && v >= b[l - 1]) return 2;
        if (v > 0) wide++;
    }
    return wide > 3 ? 2 : 0;
}

// the rows of pooled rows [ra, rb) at which a level of half-width b holds numbers: its block fits the N0d dense rows
UMPA_WIDEN_HD inline void levels_fit(int b, int N0d, int ra, int rb, int& sa, int& sb)
{
    sa = ra > b ? ra : b;
    sb = rb < N0d - b ? rb : N0d - b;
}

// the raw rows [lo, hi) a march over the pooled rows [ra, rb) loads for all levels (bmax the widest): every level's
// r - b .. r + b of its fitting rows lies inside
UMPA_WIDEN_HD inline void levels_raw_rows(int bmax, int N0d, int ra, int rb, int& lo, int& hi)
{
    lo = ra - bmax > 0 ? ra - bmax : 0;
    hi = rb + bmax < N0d ? rb + bmax : N0d;
}

// Level 0 (b = 0) of a call that pools [g.p0, g.p1): the dense rows it takes from the carry, [c0, c1), and from the chunk,
// [t0, t1).  Either may be empty.
UMPA_WIDEN_HD inline void levels_plain_rows(const WidenGeom& g, int& c0, int& c1, int& t0, int& t1)
{
    c0 = g.p0; c1 = g.p1 < g.drow0 ? g.p1 : g.drow0;
    if (c1 < c0) c1 = c0;
    t0 = g.p0 > g.drow0 ? g.p0 : g.drow0; t1 = g.p1;
    if (t1 < t0) t1 = t0;
}

// the output rows [row0, row0 + rows) of a region of N0 rows at `step` whose dense rows lie in [d0, d1)
UMPA_WIDEN_HD inline void levels_out_rows(int d0, int d1, int step, int N0, int& row0, int& rows)
{
    row0 = (d0 + step - 1) / step;
    int end = d1 > d0 ? (d1 - 1) / step + 1 : row0;
    if (end > N0) end = N0;
    rows = end > row0 ? end - row0 : 0;
}

} // namespace umpa
