// umpa_basins_kernels.h -- the third consumer of the exhaustive shift table in libumpa_grid.so: per pixel, the K lowest
// local minima ("basins") of the cost over the search box (include/umpa_grid.h: umpa_grid_basins has the definition).
//
//   grid_basins_kernel  one lane per pixel, the block shapes of grid_min_kernel.  The lane evaluates every shift of the box
//                       ONCE (eval_lookup, rows first, then columns: the table read is what grid_min_kernel is bound by) and
//                       keeps the costs of three consecutive rows of shifts in an LDS ring; once row si is complete, row
//                       si - 1 has all its neighbours and its basins are decided.  The K best (cost, shift) pairs live in a
//                       sorted insertion list in registers.  Then, per kept basin, grid_min_kernel's epilogue around it.
//
// The ring is [3][U][64] doubles, lane fastest (U = 2 ms - 1): a wave's read or write of one cell is 64 consecutive
// doubles, 512 bytes over all 64 banks twice -- free of bank conflicts for ds_read_b64 and ds_write_b64 alike.  A lane
// touches its own column only: no barrier, no atomics, nothing across lanes, so the output does not depend on how pixels
// fall into waves, blocks or row chunks.  3 U 512 bytes per wave, 50,688 at U = 33 (the tiled path's largest box): one
// wave per workgroup keeps that under the 64 KiB a workgroup gets without asking, and three such workgroups fit a CU's
// 160 KiB.  T and df are not kept in the ring: the epilogue evaluates the kept basins again.
// After the scan the ring is dead; its first 32 rows of 64 doubles then hold the lane's 4x4 neighbourhood (16) and the
// kept list (8 costs, 8 shifts), so that the epilogue is ONE loop over the ranks and not eight copies of it.
#pragma once
#include "umpa_grid_kernels.h"

#define UMPA_GRID_MAX_BASINS 8

namespace umpa {

struct BasinArgs {
    double* f; double* T; double* dx; double* dy; double* cost;   // [K][N0][N1]
    double* df;                                                   // may be NULL (dark-field model only)
    int* si; int* sj; int* err;                                   // [K][N0][N1]
    int* count;                                                   // [N0][N1]
    size_t plane;                                                 // N0 * N1
    int K;                                                        // 1 .. UMPA_GRID_MAX_BASINS
};

// doubles of dynamic LDS a wave of grid_basins_kernel needs
inline size_t grid_basins_lds(int ms)
{
    const size_t U = 2 * (size_t)ms - 1, rows = 3 * U > 32 ? 3 * U : 32;
    return rows * 64 * sizeof(double);
}

template <int KIND, int NA>
__global__ void __launch_bounds__(64)
grid_basins_kernel(ModelDev m, Maps M, ReplayArgs R, RegionArgs A, BasinArgs B)
{
    extern __shared__ double basin_lds[];
    const int bwl = R.bw_log2;
    const int xj = (blockIdx.x << bwl) + (threadIdx.x & ((1 << bwl) - 1));
    const int xi = R.row0 + (blockIdx.y << (6 - bwl)) + (threadIdx.x >> bwl);
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;                        // in the output planes
    const int K = B.K;
    if (A.cover && gp(A.cover)[(size_t)xi * A.pitch + xj] < A.thr) return;   // as the grid search: the pixel is left alone
    const size_t tpx = grid_table_px(m, R, A, xi, xj);
    const int i = A.org0 + A.step0 * xi, j = A.org1 + A.step1 * xj;
    constexpr int NFIX = NA > 0 ? NA : UMPA_KFIX;
    double fixed[NFIX];
    PixConst pc;
    grid_pixel_consts<KIND, NA>(m, M, i, j, fixed, pc);

    const int ms = m.ms, ref_mode = m.ref_mode, U = 2 * ms - 1;
    double* const lane = basin_lds + threadIdx.x;                    // cell (row, column) of the ring: lane[((row % 3) * U + column) * 64]
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    // the kept list: costs ascending, scan order among equal costs; +Inf is no basin's cost, so it marks the free slots
    double bc[UMPA_GRID_MAX_BASINS];
    int bp[UMPA_GRID_MAX_BASINS];
#pragma unroll
    for (int k = 0; k < UMPA_GRID_MAX_BASINS; k++) { bc[k] = inf; bp[k] = 0; }
    int count = 0;

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
        // row q = r - 1 has its neighbours: q - 1 (if any) from the ring, q + 1 = r (if any) just written.  A neighbour
        // outside the box is a NaN here: it beats nothing.  Neighbours that precede in scan order (the row above, the cell
        // to the left) beat on `<=`, the others on `<`.
        const int q = r - 1;
        const bool has_up = q > 0, has_dn = r < U;
        const double* const up = lane + (size_t)((q + 2) % 3) * U * 64;
        const double* const mid = lane + (size_t)(q % 3) * U * 64;
        const double* const dn = lane + (size_t)(r % 3) * U * 64;
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
                double ic = s;
                int ip = q * U + c;
                bool moving = false;
#pragma unroll
                for (int k = 0; k < UMPA_GRID_MAX_BASINS; k++) {     // behind every kept cost <= s, the rest moves down one slot
                    moving = moving || ic < bc[k];
                    if (moving) { const double tc = bc[k]; const int tp = bp[k]; bc[k] = ic; bp[k] = ip; ic = tc; ip = tp; }
                }
            }
            lu = cu; lm = cm; ld = cd;
            cu = ru; cm = rm; cd = rd;
        }
    }

    // the ring is dead: rows 16 .. 31 take the kept list, rows 0 .. 15 the 4x4 neighbourhood of the rank at hand
#pragma unroll
    for (int k = 0; k < UMPA_GRID_MAX_BASINS; k++) { lane[(16 + k) * 64] = bc[k]; lane[(24 + k) * 64] = (double)bp[k]; }
    gpw(B.count)[px] = count;

    auto cost_at = [&](int si, int sj) {                             // |si|, |sj| < ms
        double c = 0.0;
        Fit fit = {0.0, 0.0};
        eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, si, sj, fixed, pc, c, fit);
        return c;
    };
#pragma unroll 1
    for (int k = 0; k < K; k++) {
        const size_t o = (size_t)k * B.plane + px;
        double out = 0.0, uv0 = 0.0, uv1 = 0.0, cost = 0.0;
        Fit live = {0.0, 0.0};
        int bi = 0, bj = 0, status = -1;
        if (k < count) {
            const int p = (int)lane[(24 + k) * 64];
            bi = p / U - (ms - 1); bj = p % U - (ms - 1);
            eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, bi, bj, fixed, pc, cost, live);   // the ring's cost again, and T (df)
            out = cost; uv0 = bi; uv1 = bj;
            status = 0;
            // grid_min_kernel's epilogue, around this basin
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
                    double x = 1.0 - ip, y = 1.0 - jp;              // Optim.cpp:395-396
                    if (m.subpx == 0) out = x;                      // Optim.cpp:399
                    else if (m.subpx == 1) out = spmin_quad(nb, x, y);
                    else out = spmin(nb, x, y);
                    uv0 = x + (bi + ip - 1.0);                      // Optim.cpp:407-408
                    uv1 = y + (bj + jp - 1.0);
                    status = 1;
                }
            }
            if (KIND == 1 && (live.t != 0.0 || live.v != 0.0)) live.v = live.v / live.t;   // Model.cpp:854
        }
        gpw(B.f)[o] = out; gpw(B.T)[o] = live.t; gpw(B.dx)[o] = uv1; gpw(B.dy)[o] = uv0; gpw(B.cost)[o] = cost;
        if (KIND == 1 && B.df) gpw(B.df)[o] = live.v;
        gpw(B.si)[o] = bi; gpw(B.sj)[o] = bj; gpw(B.err)[o] = status;
    }
}

} // namespace umpa
