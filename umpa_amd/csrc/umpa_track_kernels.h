// umpa_track_kernels.h -- the fourth kernel family of libumpa_grid.so, the table's fifth consumer: per pixel, among ALL
// basins of the cost over the search box, the one a per-pixel prior shift selects (include/umpa_grid.h: umpa_grid_track has
// the definition).
//
//   grid_track_kernel   grid_basins_kernel's scan, unchanged: one lane per pixel, one wave per workgroup, every shift of the
//                       box evaluated ONCE (eval_lookup), the costs of three consecutive rows of shifts in the [3][U][64]
//                       LDS ring (lane fastest: conflict-free), the 3x3 sliding window deciding the basins of row si - 1 once
//                       row si is complete.  Where that kernel inserts a basin into its sorted list of eight, this one
//                       compares it with ONE running best under the mode's order -- (d2, cost) or cost + lam d2, scan order
//                       last, which the scan itself provides: a later basin replaces the best only if strictly better --
//                       and keeps the lowest basin cost and two counters beside it.  Then grid_min_kernel's epilogue once,
//                       around the chosen basin (the basins kernel's loop over the ranks with K = 1).
//
// The prior is read once per lane, by the pixel's index in the output planes.  The mode is a kernel argument: the branch is
// the same for every lane.  No barrier, no atomics, nothing across lanes: the output does not depend on how pixels fall into
// waves, blocks or row chunks.  LDS: grid_basins_lds (the ring; after the scan its first 16 rows hold the 4x4 neighbourhood).
#pragma once
#include "umpa_basins_kernels.h"

#ifndef UMPA_GRID_TRACK_NEAREST                                  // include/umpa_grid.h
#define UMPA_GRID_TRACK_NEAREST 0
#define UMPA_GRID_TRACK_PENALTY 1
#endif

namespace umpa {

struct TrackArgs {
    const double* pi; const double* pj;                           // the prior, [N0][N1]: row shift, column shift
    double* f; double* T; double* dx; double* dy; double* cost;   // [N0][N1]
    double* df;                                                   // may be NULL (dark-field model only)
    double* cost0;
    int* si; int* sj; int* err; int* count; int* found;
    int mode;                                                     // UMPA_GRID_TRACK_*
    int limited;                                                  // radius >= 0: a basin is admissible iff d2 <= r2
    double lam, r2;                                               // r2 = radius * radius, formed once by the host
};

// The two expressions of the definition that numpy must reproduce bit for bit: no contraction (the pragma lives in the
// helper, as in umpa_cost.h).
__device__ __forceinline__ double track_d2(double si, double sj, double pi, double pj)
{
#pragma clang fp contract(off)
    const double a = si - pi, b = sj - pj;
    return a * a + b * b;
}

__device__ __forceinline__ double track_penalised(double cost, double lam, double d2)
{
#pragma clang fp contract(off)
    return cost + lam * d2;
}

template <int KIND, int NA>
__global__ void __launch_bounds__(64)
grid_track_kernel(ModelDev m, Maps M, ReplayArgs R, RegionArgs A, TrackArgs B)
{
    extern __shared__ double track_lds[];
    const int bwl = R.bw_log2;
    const int xj = (blockIdx.x << bwl) + (threadIdx.x & ((1 << bwl) - 1));
    const int xi = R.row0 + (blockIdx.y << (6 - bwl)) + (threadIdx.x >> bwl);
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;                        // in the prior and output planes
    const size_t tpx = grid_table_px(m, R, A, xi, xj);
    const int i = A.org0 + A.step0 * xi, j = A.org1 + A.step1 * xj;
    constexpr int NFIX = NA > 0 ? NA : UMPA_KFIX;
    double fixed[NFIX];
    PixConst pc;
    grid_pixel_consts<KIND, NA>(m, M, i, j, fixed, pc);

    const int ms = m.ms, ref_mode = m.ref_mode, U = 2 * ms - 1;
    double* const lane = track_lds + threadIdx.x;                    // cell (row, column) of the ring: lane[((row % 3) * U + column) * 64]
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    const double pi = gp(B.pi)[px], pj = gp(B.pj)[px];
    const bool blind = pi != pi || pj != pj;                         // a NaN prior: d2 = 0 for every shift, the data term decides
    const bool penalty = B.mode == UMPA_GRID_TRACK_PENALTY;
    const double lam = B.lam, r2 = B.r2;
    const bool limited = B.limited != 0;

    // the running best: key (d2, or cost + lam d2), cost, position; the lowest basin cost; all basins, admissible basins
    double bkey = 0.0, bcost = 0.0, low = inf;
    int bpos = 0, count = 0, found = 0;

#pragma unroll 1
    for (int r = 0; r <= U; r++) {
        if (r < U) {                                                 // row r of the box: each entry of the table once
            double* const row = lane + (size_t)(r % 3) * U * 64;
#pragma unroll 1
            for (int c = 0; c < U; c++) {
                double cost = 0.0;
                Fit fit = {0.0, 0.0};
                eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, r - (ms - 1), c - (ms - 1), fixed, pc, cost, fit);
                row[c * 64] = cost;
            }
        }
        if (r == 0) continue;
        // row q = r - 1 has its neighbours (grid_basins_kernel's window: NaN outside the box, `<=` for the neighbours that
        // precede in scan order, `<` for the others)
        const int q = r - 1;
        const bool has_up = q > 0, has_dn = r < U;
        const double* const up = lane + (size_t)((q + 2) % 3) * U * 64;
        const double* const mid = lane + (size_t)(q % 3) * U * 64;
        const double* const dn = lane + (size_t)(r % 3) * U * 64;
        const double fi = (double)(q - (ms - 1));
        double lu = nan, lm = nan, ld = nan;
        double cu = has_up ? up[0] : nan, cm = mid[0], cd = has_dn ? dn[0] : nan;
#pragma unroll 1
        for (int c = 0; c < U; c++) {
            const bool has_r = c + 1 < U;
            const double ru = has_r && has_up ? up[(c + 1) * 64] : nan;
            const double rm = has_r ? mid[(c + 1) * 64] : nan;
            const double rd = has_r && has_dn ? dn[(c + 1) * 64] : nan;
            const double s = cm;
            if (s < inf && !(lu <= s || cu <= s || ru <= s || lm <= s || rm < s || ld < s || cd < s || rd < s)) {
                count++;
                if (s < low) low = s;
                const double d2 = blind ? 0.0 : track_d2(fi, (double)(c - (ms - 1)), pi, pj);
                if (!limited || d2 <= r2) {
                    bool better;
                    double key;
                    if (penalty) {
                        key = track_penalised(s, lam, d2);
                        better = key < bkey;
                    } else {
                        key = d2;
                        better = d2 < bkey || (d2 == bkey && s < bcost);
                    }
                    if (found == 0 || better) { bkey = key; bcost = s; bpos = q * U + c; }
                    found++;
                }
            }
            lu = cu; lm = cm; ld = cd;
            cu = ru; cm = rm; cd = rd;
        }
    }

    gpw(B.count)[px] = count;
    gpw(B.found)[px] = found;
    gpw(B.cost0)[px] = count > 0 ? low : 0.0;

    auto cost_at = [&](int si, int sj) {                             // |si|, |sj| < ms
        double c = 0.0;
        Fit fit = {0.0, 0.0};
        eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, si, sj, fixed, pc, c, fit);
        return c;
    };
    double out = 0.0, uv0 = 0.0, uv1 = 0.0, cost = 0.0;
    Fit live = {0.0, 0.0};
    int bi = 0, bj = 0, status = -1;
    if (found > 0) {
        bi = bpos / U - (ms - 1); bj = bpos % U - (ms - 1);
        eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, bi, bj, fixed, pc, cost, live);   // the ring's cost again, and T (df)
        out = cost; uv0 = bi; uv1 = bj;
        status = 0;
        // grid_min_kernel's epilogue, around this basin (the ring is dead: its rows 0 .. 15 take the 4x4 neighbourhood)
        if (bi > 1 - ms && bi < ms - 1 && bj > 1 - ms && bj < ms - 1) {
            const int ip = cost_at(bi + 1, bj) < cost_at(bi - 1, bj) ? 1 : 0;   // Optim.cpp:344-345
            const int jp = cost_at(bi, bj + 1) < cost_at(bi, bj - 1) ? 1 : 0;
            const int i0 = bi + ip - 2, j0 = bj + jp - 2;
            if (i0 > -ms && i0 + 3 < ms && j0 > -ms && j0 + 3 < ms) {
#pragma unroll 1
                for (int g = 0; g < 16; g++) lane[g * 64] = cost_at(i0 + (g >> 2), j0 + (g & 3));
                double nb[16];
#pragma unroll
                for (int g = 0; g < 16; g++) nb[g] = lane[g * 64];
                double x = 1.0 - ip, y = 1.0 - jp;                  // Optim.cpp:395-396
                if (m.subpx == 0) out = x;                          // Optim.cpp:399
                else if (m.subpx == 1) out = spmin_quad(nb, x, y);
                else out = spmin(nb, x, y);
                uv0 = x + (bi + ip - 1.0);                          // Optim.cpp:407-408
                uv1 = y + (bj + jp - 1.0);
                status = 1;
            }
        }
        if (KIND == 1 && (live.t != 0.0 || live.v != 0.0)) live.v = live.v / live.t;   // Model.cpp:854
    }
    gpw(B.f)[px] = out; gpw(B.T)[px] = live.t; gpw(B.dx)[px] = uv1; gpw(B.dy)[px] = uv0; gpw(B.cost)[px] = cost;
    if (KIND == 1 && B.df) gpw(B.df)[px] = live.v;
    gpw(B.si)[px] = bi; gpw(B.sj)[px] = bj; gpw(B.err)[px] = status;
}

} // namespace umpa
