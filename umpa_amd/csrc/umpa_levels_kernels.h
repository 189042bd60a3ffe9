// umpa_levels_kernels.h -- scale-space search (include/umpa_grid.h has the definition): every widening level of a row chunk
// from one read of its shift table, the prior handed from level to level on the device, and the choice of the level per pixel.
//
//   levels_table_kernel<HB0, HB1, HB2, STRIP>  the table pooled to two or three half-widths HB0 > HB1 (> HB2; 0: none) at
//                                  once: widen_march's scheme (umpa_widen_kernels.h) -- a wave owns 64 columns and goes down
//                                  the rows, a raw row goes through a double-buffered LDS segment with the widest level's
//                                  halo -- with one ring of horizontal sums per level.  Each raw element is loaded once; from
//                                  the segment every level forms its own H left to right, pushes it into its own ring and
//                                  re-adds that ring top to bottom for its output row, which trails the raw row by the
//                                  level's half-width.  The sums and their order are widen_table_kernel<b>'s: each pooled
//                                  table is that kernel's bit for bit.  Reads either raw layout through widen_src, writes
//                                  one plain-layout table per level.
//   levels_prior_kernel            rows of the prior planes: the level before's dy, dx where it matched (err == 1, both
//                                  finite), NaN elsewhere -- umpa_amd.track.prior_from; all NaN before the first level;
//   levels_select_kernel           rows of the selected planes: per pixel the narrowest level consistent with every wider
//                                  one that matched (Lepski's rule), a copy of that level's values, `level` and `halfwidth`.
//
// Nothing across lanes but the segment, no atomics: the output does not depend on waves, segments or row chunks.
#pragma once
#include "umpa_widen_kernels.h"
#include "umpa_levels_geom.h"

namespace umpa {

// one level of levels_table_kernel: its ring, the push of a raw row's horizontal sum and the output row that completes
template <int HB>
struct LevelsRing {
    static constexpr int B = 2 * HB + 1;
    double ring[B];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < B; k++) ring[k] = 0.0;
    }
    // `s`: the segment at this lane's column minus HBMAX; the level's window starts HBMAX - HB further right
    template <int HBMAX>
    __device__ __forceinline__ void push(const double* s)
    {
#pragma clang fp contract(off)
        double h = s[HBMAX - HB];                                    // H(r, c): left to right
#pragma unroll
        for (int k = 1; k < B; k++) h = h + s[HBMAX - HB + k];
#pragma unroll
        for (int k = 0; k < B - 1; k++) ring[k] = ring[k + 1];
        ring[B - 1] = h;
    }
    __device__ __forceinline__ double pooled() const
    {
#pragma clang fp contract(off)
        const double rB = 1.0 / (double)(B * B);
        double v = ring[0];                                          // V(r, c): top to bottom
#pragma unroll
        for (int k = 1; k < B; k++) v = v + ring[k];
        return v * rB;
    }
};

// grid (column blocks of 64, U^2 planes, segments of UMPA_WIDEN_SEG pooled rows); 64 threads.  g.b is HB0 (the lag).
template <int HB0, int HB1, int HB2, bool STRIP>
__global__ void __launch_bounds__(64)
levels_table_kernel(const double* table, const double* carry, double* out0, double* out1, double* out2, WidenGeom g)
{
    static_assert(HB0 > HB1 && HB1 > HB2 && HB2 >= 0 && HB0 <= 8, "half-widths: decreasing, the third may be absent (0)");
    __shared__ double seg[2 * 80];
    const int lane = threadIdx.x, c = blockIdx.x * 64 + lane, slot = blockIdx.y;
    const int ra = g.p0 + blockIdx.z * UMPA_WIDEN_SEG, rb = min(g.p1, ra + UMPA_WIDEN_SEG);
    int sa0, sb0, sa1, sb1, sa2 = 0, sb2 = 0;
    levels_fit(HB0, g.N0d, ra, rb, sa0, sb0);
    levels_fit(HB1, g.N0d, ra, rb, sa1, sb1);
    if (HB2 > 0) levels_fit(HB2, g.N0d, ra, rb, sa2, sb2);
    UMPA_GLOBAL double* __restrict__ o0 = gpw(out0);
    UMPA_GLOBAL double* __restrict__ o1 = gpw(out1);
    UMPA_GLOBAL double* __restrict__ o2 = gpw(out2);
    const double nan = __builtin_nan("");
    const bool wr = c < g.N1q;
    for (int r = ra; r < rb; r++) {                                  // the rows whose block leaves the dense grid
        if (!wr) break;
        const size_t at = widen_dst(g, r, slot, c);
        if (r < sa0 || r >= sb0) o0[at] = nan;
        if (r < sa1 || r >= sb1) o1[at] = nan;
        if (HB2 > 0 && (r < sa2 || r >= sb2)) o2[at] = nan;
    }
    int lo, hi;
    levels_raw_rows(HB0, g.N0d, ra, rb, lo, hi);
    const UMPA_GLOBAL double* __restrict__ t = gp(table);
    const UMPA_GLOBAL double* __restrict__ cy = gp(carry);
    WidenGeom gs = g;
    if (!STRIP) gs.strip_w = 0;                                      // (the layout test folds away)
    const bool in0 = c >= HB0 && c < g.N1d - HB0, in1 = c >= HB1 && c < g.N1d - HB1, in2 = c >= HB2 && c < g.N1d - HB2;
    auto load = [&](int row, int col) {
        bool in_carry;
        const size_t at = widen_src(gs, row, slot, col, in_carry);
        return in_carry ? cy[at] : t[at];
    };
    LevelsRing<HB0> r0;
    LevelsRing<HB1> r1;
    LevelsRing<(HB2 > 0 ? HB2 : 1)> r2;
    r0.clear(); r1.clear(); r2.clear();
    const int cl = c - HB0, cr = c - HB0 + 64;
    for (int rr = lo; rr < hi; rr++) {
        double* s = seg + ((rr - lo) & 1) * 80;
        s[lane] = (cl >= 0 && cl < g.N1d) ? load(rr, cl) : 0.0;
        if (lane < 2 * HB0) s[64 + lane] = (cr >= 0 && cr < g.N1d) ? load(rr, cr) : 0.0;
        __syncthreads();
        r0.template push<HB0>(s + lane);
        r1.template push<HB0>(s + lane);
        if (HB2 > 0) r2.template push<HB0>(s + lane);
        if (!wr) continue;
        const int q0 = rr - HB0, q1 = rr - HB1, q2 = rr - HB2;        // the output row each level completes with this raw row
        if (q0 >= sa0 && q0 < sb0) o0[widen_dst(g, q0, slot, c)] = in0 ? r0.pooled() : nan;
        if (q1 >= sa1 && q1 < sb1) o1[widen_dst(g, q1, slot, c)] = in1 ? r1.pooled() : nan;
        if (HB2 > 0 && q2 >= sa2 && q2 < sb2) o2[widen_dst(g, q2, slot, c)] = in2 ? r2.pooled() : nan;
    }
}

// the planes of one level or of the selection, [N0][N1] each, in the order of umpa_grid_wide_track's outputs
struct LevelsPlanes {
    double* f; double* T; double* dx; double* dy; double* cost; double* df; double* cost0;
    int* si; int* sj; int* err; int* count; int* found;
};

struct LevelsSelectArgs {
    LevelsPlanes lev;             // level 0's planes; level l's lie l * plane elements further
    LevelsPlanes sel;
    int* level; int* halfwidth;
    size_t plane;                 // N0 * N1
    int L, N1, row0, rows;        // the output rows [row0, row0 + rows) of this call
    int b[UMPA_LEVELS_MAX];
    double tol[UMPA_LEVELS_MAX];
};

__device__ __forceinline__ bool levels_ok(int err, double dx, double dy)
{
    return err == 1 && __builtin_isfinite(dx) && __builtin_isfinite(dy);
}

// grid (blocks of 256 pixels of the rows); prev_*: the level before's planes, NULL before the first level
__global__ void __launch_bounds__(256)
levels_prior_kernel(const double* prev_dx, const double* prev_dy, const int* prev_err, double* pi, double* pj,
                    int N1, int row0, int rows)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)rows * N1) return;
    const size_t px = (size_t)row0 * N1 + q;
    const double nan = __builtin_nan("");
    double vi = nan, vj = nan;
    if (prev_err) {
        const double dx = gp(prev_dx)[px], dy = gp(prev_dy)[px];
        if (levels_ok(gp(prev_err)[px], dx, dy)) { vi = dy; vj = dx; }
    }
    gpw(pi)[px] = vi; gpw(pj)[px] = vj;
}

__global__ void __launch_bounds__(256)
levels_select_kernel(LevelsSelectArgs a)
{
#pragma clang fp contract(off)
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.rows * a.N1) return;
    const size_t px = (size_t)a.row0 * a.N1 + q;
    double dx[UMPA_LEVELS_MAX], dy[UMPA_LEVELS_MAX];
    bool ok[UMPA_LEVELS_MAX];
    int level = -1;
#pragma unroll
    for (int l = 0; l < UMPA_LEVELS_MAX; l++) {
        ok[l] = false; dx[l] = 0.0; dy[l] = 0.0;
        if (l < a.L) {
            dx[l] = gp(a.lev.dx)[l * a.plane + px]; dy[l] = gp(a.lev.dy)[l * a.plane + px];
            ok[l] = levels_ok(gp(a.lev.err)[l * a.plane + px], dx[l], dy[l]);
            bool consistent = ok[l];
#pragma unroll
            for (int m = 0; m < l; m++)
                if (ok[m] && !(__builtin_fabs(dx[l] - dx[m]) <= a.tol[m] && __builtin_fabs(dy[l] - dy[m]) <= a.tol[m])) consistent = false;
            if (consistent) level = l;
        }
    }
    int hw = -1;
#pragma unroll
    for (int l = 0; l < UMPA_LEVELS_MAX; l++) if (l == level) hw = a.b[l];
    const size_t from = (size_t)(level < 0 ? a.L - 1 : level) * a.plane + px;
    gpw(a.sel.f)[px] = gp(a.lev.f)[from]; gpw(a.sel.T)[px] = gp(a.lev.T)[from];
    gpw(a.sel.dx)[px] = gp(a.lev.dx)[from]; gpw(a.sel.dy)[px] = gp(a.lev.dy)[from];
    gpw(a.sel.cost)[px] = gp(a.lev.cost)[from]; gpw(a.sel.cost0)[px] = gp(a.lev.cost0)[from];
    if (a.sel.df) gpw(a.sel.df)[px] = gp(a.lev.df)[from];
    gpw(a.sel.si)[px] = gp(a.lev.si)[from]; gpw(a.sel.sj)[px] = gp(a.lev.sj)[from];
    gpw(a.sel.err)[px] = gp(a.lev.err)[from]; gpw(a.sel.count)[px] = gp(a.lev.count)[from];
    gpw(a.sel.found)[px] = gp(a.lev.found)[from];
    gpw(a.level)[px] = level; gpw(a.halfwidth)[px] = hw;
}

} // namespace umpa
