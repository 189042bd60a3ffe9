// umpa_general_geom.h -- the footprint arithmetic of the general shift-table kernel (umpa_general_table_kernels.h): how large
// the three LDS footprints of a workgroup are and where they lie, where a lane's windows start inside them, which shift an
// accumulator set of a pass stands for, and which frame element a staged element is loaded from.  Plain C++ on plain ints
// with no HIP type in it, so that the host program tests/general_addr_check.cpp can play every read on the CPU under the
// sanitizers.  general_geometry, which decides between LDS and the global-memory fallback, is a wrapper over
// general_footprints.  The kernel keeps its own spelling of the four index functions below: routed through them its four
// instantiations no longer disassemble to the parent's instructions (profiles/general_geom_codeobj.txt), so the functions
// here restate the kernel's expressions term for term and the host program is their check.
//
// A workgroup of by x bx pixels at steps (step0, step1) covers a box of (by - 1) step0 + 1 rows and (bx - 1) step1 + 1
// columns of the image.  The stack whose window stays needs the box widened by Nw, the one whose window moves with the shift
// (the reference in 'sam' mode, the sample in 'ref' mode) and the masks by Nw + ms - 1.  The footprints lie one behind the
// other, each at an even offset (16-byte alignment), the (2 Nw + 1)^2 window weights behind them.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define UMPA_GENERAL_HD __host__ __device__
#else
#define UMPA_GENERAL_HD
#endif

namespace umpa {

#define UMPA_GENERAL_LDS_BYTES (64 * 1024)   // what a kernel gets without asking
#define UMPA_GENERAL_MAX_SIDE 4096           // a footprint side past this is not tried at all

struct GeneralFootprints {
    int hq, hr, hm;                  // halo of the sample / reference / mask footprint around the pixel box
    int rowsQ, colsQ, rowsR, colsR, rowsM, colsM;
    int offR, offM, offW;            // offsets (doubles) of the reference and mask footprints (sample at 0) and of the window
    size_t lds_bytes;
};

// false: the footprints do not fit (the caller falls back to global memory); F is then not to be used
inline bool general_footprints(int Nw, int ms, int ref_mode, bool has_mask, int step0, int step1, int by, int bx, GeneralFootprints& F)
{
    const long boxr = (long)(by - 1) * step0 + 1, boxc = (long)(bx - 1) * step1 + 1;
    const int wide = Nw + (ms > 1 ? ms - 1 : 0);
    F.lds_bytes = 0;
    if (boxr + 2 * wide > UMPA_GENERAL_MAX_SIDE || boxc + 2 * wide > UMPA_GENERAL_MAX_SIDE) return false;
    F.hq = ref_mode ? wide : Nw;                                      // the sample window moves in 'ref' mode (Model.cpp:688-701)
    F.hr = ref_mode ? Nw : wide;
    F.hm = wide;
    F.rowsQ = (int)boxr + 2 * F.hq; F.colsQ = (int)boxc + 2 * F.hq;
    F.rowsR = (int)boxr + 2 * F.hr; F.colsR = (int)boxc + 2 * F.hr;
    F.rowsM = has_mask ? (int)boxr + 2 * F.hm : 0; F.colsM = has_mask ? (int)boxc + 2 * F.hm : 0;
    F.offR = (F.rowsQ * F.colsQ + 1) & ~1;
    F.offM = (F.offR + F.rowsR * F.colsR + 1) & ~1;
    F.offW = (F.offM + F.rowsM * F.colsM + 1) & ~1;
    const int S = 2 * Nw + 1;
    F.lds_bytes = (size_t)(F.offW + S * S + 2) * sizeof(double);
    return F.lds_bytes <= (size_t)UMPA_GENERAL_LDS_BYTES;
}

// the image coordinate of a workgroup's first pixel along one axis: the box origin
UMPA_GENERAL_HD inline int general_box_origin(int org, int step, int first_px) { return org + step * first_px; }

// where the window centred on image pixel (ci, cj) starts inside a footprint of halo `halo` and `cols` columns around the box
// at (gi0, gj0): its top-left element (ci - Nw, cj - Nw)
UMPA_GENERAL_HD inline int general_window_origin(int ci, int cj, int Nw, int gi0, int gj0, int halo, int cols)
{
    return (ci - Nw - (gi0 - halo)) * cols + (cj - Nw - (gj0 - halo));
}

// set c of the pass that starts at column shift sj0 stands for the shift sj0 + dc; past ms - 1 it repeats shift ms - 1
UMPA_GENERAL_HD inline int general_set_offset(int c, int ms, int sj0) { const int last = ms - 1 - sj0; return c < last ? c : last; }

// element `e` (row or column) of a footprint of halo `halo` whose box starts at frame coordinate f0 is loaded from frame
// coordinate f0 - halo + e, clamped to the frame's [0, n)
UMPA_GENERAL_HD inline int general_source(int f0, int halo, int e, int n)
{
    const int x = f0 - halo + e, lo = x > 0 ? x : 0;                  // min(max(x, 0), n - 1)
    return lo < n - 1 ? lo : n - 1;
}

} // namespace umpa
