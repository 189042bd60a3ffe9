// umpa_grid_kernels.h -- the kernels of libumpa_grid.so: consumers of the tiled path's exhaustive shift table.
//
// prep_maps and corr_volume / corr_march (umpa_tiled.h) leave, for a row chunk, the maps and the correlation term of EVERY
// integer shift of the search box.  replay_walk reads about 18 of those entries per pixel; the two kernels here read all:
//
//   grid_min_kernel     per pixel the first strict minimum over the (2 ms - 1)^2 shifts (rows first, then columns), then
//                       the walk's own epilogue on the 4x4 neighbourhood of that minimum (Optim.cpp:344-345, :386-410);
//   cost_volume_kernel  the cost (transmission, dark-field) of every shift as planes [shift][row][column].
//
// Every cost is eval_lookup's (umpa_tiled.h), with the frame-count template the replay dispatch picks: the numbers are
// replay_walk's bit for bit.  Each table entry is read once, plane by plane, a wave reading runs of consecutive doubles.
#pragma once
#include "umpa_tiled.h"

namespace umpa {

struct VolumeArgs {
    double* cost;             // [(2ms-1)^2][N0][N1]
    double* T;                // may be NULL
    double* df;               // may be NULL (dark-field model only)
    size_t plane;             // N0 * N1
};

// where pixel (xi, xj) of the region sits in the chunk's table (replay_walk's own addressing)
__device__ __forceinline__ size_t grid_table_px(const ModelDev& m, const ReplayArgs& R, const RegionArgs& A, int xi, int xj)
{
    if (R.strip_w > 0) {                                             // corr_march's strip-blocked table (umpa_march.h)
        const int dc = xj * A.step1, strip = dc / R.strip_w, UJr = 2 * m.ms - 1;
        return (((size_t)strip * R.drows + (size_t)(xi * A.step0 - R.drow0)) * (size_t)(UJr * UJr)) * R.tw + (size_t)(dc - strip * R.strip_w);
    }
    return (size_t)(xi * A.step0 - R.drow0) * R.N1d + (size_t)xj * A.step1;
}

// what eval_lookup wants of the pixel itself: the per-frame maps at the window that does not move, and the sums of the
// pixel's own window (as replay_walk forms them)
template <int KIND, int NA>
__device__ __forceinline__ void grid_pixel_consts(const ModelDev& m, const Maps& M, int i, int j,
                                                  double* fixed, PixConst& pc)
{
    constexpr int NFIX = NA > 0 ? NA : UMPA_KFIX;
    const size_t plane = (size_t)M.H * M.W, x0 = (size_t)i * M.W + j;
    if (KIND == 1) {
        const UMPA_GLOBAL double* __restrict__ fx = gp(m.ref_mode ? M.MR : M.WS);
        if constexpr (NA > 0) {
#pragma unroll
            for (int qq = 0; qq < (NA + 1) / 2; qq++) {
                const map_pair_t v = *reinterpret_cast<const UMPA_GLOBAL map_pair_t*>(fx + ((size_t)qq * plane + x0) * 2);
                fixed[2 * qq] = v[0];
                if (2 * qq + 1 < NFIX) fixed[2 * qq + 1] = v[1];
            }
        } else {
#pragma unroll
            for (int k = 0; k < NFIX; k++) fixed[k] = k < m.Na ? fx[map_at(k, x0, plane)] : 0.0;
        }
    }
    pc = {0.0, 0.0, 0.0, 0.0};
    if (m.ref_mode) {
        pc.t3 = gp(M.RefSq)[x0];
        if (KIND == 1) {
#pragma unroll
            for (int k = 0; k < NFIX; k++) if (NA > 0 || k < m.Na) pc.t2 = fma(fixed[k], fixed[k], pc.t2);
            for (int k = NFIX; k < m.Na; k++) { const double a = gp(M.MR)[map_at(k, x0, plane)]; pc.t2 = fma(a, a, pc.t2); }
            pc.t6 = m.win_sum * pc.t2;
        }
    } else pc.t1 = gp(M.SamSq)[x0];
}

// One lane per output pixel of the chunk; a wave takes a block of 2^bw_log2 x 2^(6 - bw_log2) pixels (ReplayArgs: the
// shapes replay_walk settled on for the two table layouts).
template <int KIND, int NA>
__global__ void __launch_bounds__(64)
grid_min_kernel(ModelDev m, Maps M, ReplayArgs R, RegionArgs A)
{
    const int bwl = R.bw_log2;
    const int xj = (blockIdx.x << bwl) + (threadIdx.x & ((1 << bwl) - 1));
    const int xi = R.row0 + (blockIdx.y << (6 - bwl)) + (threadIdx.x >> bwl);
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.pitch + xj;                     // in the output arrays
    if (A.cover && gp(A.cover)[px] < A.thr) return;
    const size_t tpx = grid_table_px(m, R, A, xi, xj);
    const int i = A.org0 + A.step0 * xi, j = A.org1 + A.step1 * xj;
    constexpr int NFIX = NA > 0 ? NA : UMPA_KFIX;
    double fixed[NFIX];
    PixConst pc;
    grid_pixel_consts<KIND, NA>(m, M, i, j, fixed, pc);

    const int ms = m.ms, ref_mode = m.ref_mode;
    double best = __builtin_inf();
    Fit bfit = {0.0, 0.0};
    int bi = 0, bj = 0;
    for (int si = 1 - ms; si < ms; si++)
        for (int sj = 1 - ms; sj < ms; sj++) {
            double c = 0.0;
            Fit fit = {0.0, 0.0};
            eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, si, sj, fixed, pc, c, fit);
            if (c < best) { best = c; bfit = fit; bi = si; bj = sj; }   // the first strict minimum; a NaN never wins
        }
    auto cost_at = [&](int si, int sj) {                             // |si|, |sj| < ms
        double c = 0.0;
        Fit fit = {0.0, 0.0};
        eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, si, sj, fixed, pc, c, fit);
        return c;
    };

    Walk w;                                                          // what store_pixel reads of a finished walk
    w.n = (2 * ms - 1) * (2 * ms - 1);
    w.status = 0;
    w.out = 0.0; w.uv0 = 0.0; w.uv1 = 0.0;
    w.live = {0.0, 0.0};
    w.known = 0; w.bi = 0; w.bj = 0; w.ci = 0; w.cj = 0;
    double nb[16];
#pragma unroll
    for (int g = 0; g < 16; g++) nb[g] = 0.0;
    const bool finite = best < __builtin_inf();
    if (finite) {
        w.ci = bi; w.cj = bj;
        w.out = best; w.uv0 = bi; w.uv1 = bj;
        w.live = bfit;
        // the four neighbours exist iff the minimum is not on the border of the search box (there the 4x4 cells leave it
        // for either quadrant)
        if (bi > 1 - ms && bi < ms - 1 && bj > 1 - ms && bj < ms - 1) {
            const int ip = cost_at(bi + 1, bj) < cost_at(bi - 1, bj) ? 1 : 0;   // Optim.cpp:344-345
            const int jp = cost_at(bi, bj + 1) < cost_at(bi, bj - 1) ? 1 : 0;
            const int i0 = bi + ip - 2, j0 = bj + jp - 2;            // cell (0, 0) of the 4x4 neighbourhood: rows ip .. ip + 3 of the 5x5
            if (i0 > -ms && i0 + 3 < ms && j0 > -ms && j0 + 3 < ms) {
#pragma unroll
                for (int g = 0; g < 16; g++) nb[g] = cost_at(i0 + (g >> 2), j0 + (g & 3));
                double x = 1.0 - ip, y = 1.0 - jp;                  // Optim.cpp:395-396
                if (m.subpx == 0) w.out = x;                        // Optim.cpp:399
                else if (m.subpx == 1) w.out = spmin_quad(nb, x, y);
                else w.out = spmin(nb, x, y);
                w.uv0 = x + (bi + ip - 1.0);                        // Optim.cpp:407-408
                w.uv1 = y + (bj + jp - 1.0);
                w.status = UMPA_ST_OK;
            }
        }
        if (KIND == 1 && (w.live.t != 0.0 || w.live.v != 0.0)) w.live.v = w.live.v / w.live.t;   // Model.cpp:854
    }
    if (A.dbg_d) {                                                   // the 5x5 around the minimum, -1 outside the search range
        for (int q = 0; q < 25; q++) {
            const int si = bi + q / 5 - 2, sj = bj + q % 5 - 2;
            const bool in = finite && si > -ms && si < ms && sj > -ms && sj < ms;
            gpw(A.dbg_d)[px * 25 + q] = in ? cost_at(si, sj) : -1.0;
        }
    }
    RegionArgs B = A;
    B.dbg_d = nullptr;                                               // written above: no walk memo here
    const LdsMemo<1> none = {nullptr};
    store_pixel(B, px, KIND, w, none, nb);
}

// Lanes along xj: every (shift, row) of the output is one coalesced run, and so is every read of the table.
template <int KIND, int NA>
__global__ void __launch_bounds__(64)
cost_volume_kernel(ModelDev m, Maps M, ReplayArgs R, RegionArgs A, VolumeArgs V)
{
    const int xj = blockIdx.x * 64 + threadIdx.x;
    const int xi = R.row0 + blockIdx.y;
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;
    const size_t tpx = grid_table_px(m, R, A, xi, xj);
    const int i = A.org0 + A.step0 * xi, j = A.org1 + A.step1 * xj;
    constexpr int NFIX = NA > 0 ? NA : UMPA_KFIX;
    double fixed[NFIX];
    PixConst pc;
    grid_pixel_consts<KIND, NA>(m, M, i, j, fixed, pc);
    const int ms = m.ms, ref_mode = m.ref_mode;
    size_t o = px;
    for (int si = 1 - ms; si < ms; si++)
        for (int sj = 1 - ms; sj < ms; sj++, o += V.plane) {
            double c = 0.0;
            Fit fit = {0.0, 0.0};
            eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, si, sj, fixed, pc, c, fit);
            gpw(V.cost)[o] = c;
            if (V.T) gpw(V.T)[o] = fit.t;
            if (KIND == 1 && V.df) gpw(V.df)[o] = (fit.t != 0.0 || fit.v != 0.0) ? fit.v / fit.t : 0.0;   // Model.cpp:854, the walk's guard
        }
}

} // namespace umpa
