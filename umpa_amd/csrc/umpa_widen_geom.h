// umpa_widen_geom.h -- window widening (include/umpa_grid.h): which dense rows a table consumer call pools, and where the
// raw rows they need lie.  Plain C++ with no HIP type in it, so that the host program tests/widen_addr_check.cpp can sweep
// every address on the CPU under the sanitizers; the kernels of umpa_widen_kernels.h call the same functions.
//
// The tiled path hands its consumer the table one row chunk at a time and reuses the chunk's memory.  A pooled row r needs
// the raw rows r - b .. r + b, so a call pools the rows whose block is complete: [drow0 - b, drow0 + drows - b), the first
// call from row 0 and the last one up to the region's last dense row (the first and last b rows of the region are NaN:
// their block leaves the region).  The raw rows [drow0 - 2b, drow0) it needs of the chunk before are kept in a carry
// buffer, in the chunk's own layout with 2b rows per plane or strip.  Every pooled entry is thus the same sum of the same
// raw entries in the same order whatever the chunking.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define UMPA_WIDEN_HD __host__ __device__
#else
#define UMPA_WIDEN_HD
#endif

namespace umpa {

struct WidenGeom {
    int b;                    // half-width of the box, 1 .. 8
    int U2;                   // table planes: (2 max_shift - 1)^2
    int N0d, N1d;             // the region's dense grid
    int drow0, drows;         // the raw dense rows the chunk's table holds
    int crows;                // the carry holds the raw rows [drow0 - crows, drow0): 0 on the first chunk, else 2b
    int strip_w, tw;          // the raw layout (ReplayArgs): strip_w > 0 is corr_march's [strip][rows][U2][tw]
    int N1p;                  // doubles per raw row and plane (strip-blocked: nstrips * tw)
    int p0, p1;               // the pooled dense rows [p0, p1) this call writes
    int N1q;                  // doubles per pooled row (plain layout: [U2][p1 - p0][N1q])
};

// the pooled rows of the chunk [drow0, drow0 + drows) of a region of N0d dense rows
UMPA_WIDEN_HD inline void widen_rows(int b, int N0d, int drow0, int drows, int& p0, int& p1)
{
    p0 = drow0 == 0 ? 0 : drow0 - b;
    p1 = drow0 + drows >= N0d ? N0d : drow0 + drows - b;
    if (p1 < p0) p1 = p0;
}

// a pooled entry (row, col) is a number iff its B x B block lies inside the dense grid; NaN otherwise
UMPA_WIDEN_HD inline bool widen_inside(const WidenGeom& g, int row, int col)
{
    return row >= g.b && row < g.N0d - g.b && col >= g.b && col < g.N1d - g.b;
}

UMPA_WIDEN_HD inline size_t widen_table_len(const WidenGeom& g, int rows) { return (size_t)g.U2 * (size_t)rows * (size_t)g.N1p; }

// Where raw entry (dense row, table plane `slot`, dense column) lies: an index into the carry (`in_carry`) or into the
// chunk's table.  row in [drow0 - crows, drow0 + drows), col in [0, N1d).
UMPA_WIDEN_HD inline size_t widen_src(const WidenGeom& g, int row, int slot, int col, bool& in_carry)
{
    in_carry = row < g.drow0;
    const int rows = in_carry ? g.crows : g.drows;
    const int r = in_carry ? row - (g.drow0 - g.crows) : row - g.drow0;
    if (g.strip_w > 0) {                                             // grid_table_px's addressing, any plane
        const int strip = col / g.strip_w;
        return (((size_t)strip * rows + (size_t)r) * (size_t)g.U2 + (size_t)slot) * (size_t)g.tw + (size_t)(col - strip * g.strip_w);
    }
    return ((size_t)slot * rows + (size_t)r) * (size_t)g.N1p + (size_t)col;
}

// where pooled entry (row in [p0, p1), slot, col in [0, N1q)) goes
UMPA_WIDEN_HD inline size_t widen_dst(const WidenGeom& g, int row, int slot, int col)
{
    return ((size_t)slot * (size_t)(g.p1 - g.p0) + (size_t)(row - g.p0)) * (size_t)g.N1q + (size_t)col;
}

// The carry is refilled from the chunk's last 2b rows as `nruns` runs of `run` doubles: run q starts at src_off + q * pitch
// of the table and at q * run of the carry (a plane's rows are contiguous in the plain layout, a strip's in the other).
struct WidenCarryCopy { size_t nruns, run, pitch, src_off; };
UMPA_WIDEN_HD inline WidenCarryCopy widen_carry_copy(const WidenGeom& g)
{
    const size_t keep = 2 * (size_t)g.b;
    WidenCarryCopy c;
    if (g.strip_w > 0) {
        const size_t row = (size_t)g.U2 * g.tw;
        c.nruns = (size_t)(g.N1p / g.tw); c.run = keep * row; c.pitch = (size_t)g.drows * row; c.src_off = ((size_t)g.drows - keep) * row;
    } else {
        c.nruns = (size_t)g.U2; c.run = keep * g.N1p; c.pitch = (size_t)g.drows * g.N1p; c.src_off = ((size_t)g.drows - keep) * g.N1p;
    }
    return c;
}

} // namespace umpa
