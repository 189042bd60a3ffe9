// umpa_sequence_kernels.h -- the sixth kernel family of libumpa_grid.so: the forward step of a dynamic programme over a
// series of projections (include/umpa_grid.h: umpa_grid_sequence has the definition).  Per pixel a state of one accumulated
// cost per shift of the search box comes in (`prev`), the table's costs of this projection are added to the cheapest
// compatible predecessor, and the new state goes out (`next`) together with the maps of the cheapest shift.
//
//   grid_sequence_kernel   one lane per pixel, one wave per workgroup, the block shapes of the siblings.  The pixel's U x U
//                          state sits in LDS as [slot][lane] (lane fastest: the lanes of a wave read consecutive doubles,
//                          no bank is hit twice).  Three phases, nothing across lanes, no barrier, no atomics:
//                            1. prev -> LDS, m0 = its first strict minimum;
//                            2. the two-stage quadratic transition in place: the 1-D lower envelope
//                               out[o] = min_q (in[q] + lam (o - q)^2) along every row of the box (stage 2 of the
//                               definition), then along every column (stage 3).  A line is read into registers, its U
//                               outputs are formed from them and written back (sequence_line: unrolled to the largest U,
//                               15, with wave-uniform guards, so that every register index is a constant);
//                            3. the scan of the siblings over the shifts: C[s] from eval_lookup (the cost volume's number),
//                               M[s] from LDS with the truncation applied, A = C + M to `next` (a wave writes runs of
//                               consecutive doubles per shift), the running first strict minima of A and of C;
//                          then grid_track_kernel's epilogue around the minimum of A, on the DATA costs C.
//
// LDS per wave: U * U * (pixels per wave) * 8 bytes.  A wave takes 64 pixels up to U = 11 (61,952 bytes) and 32 pixels,
// with its upper half idle, at U = 13 and 15 (43,264 and 57,600 bytes): a workgroup never asks for more than 64 KB.
// Without a state (prev = NULL) a launch asks for the epilogue's 16 slots only.
#pragma once
#include "umpa_track_kernels.h"

namespace umpa {

#define UMPA_SEQUENCE_MAX_U 15                                    // max_shift 8

struct SequenceArgs {
    const double* prev;                                           // [U*U][N0][N1], may be NULL (a series starts)
    double* next;                                                 // the same layout, may be NULL
    double* f; double* T; double* dx; double* dy; double* cost;   // [N0][N1]
    double* df;                                                   // may be NULL (dark-field model only)
    double* total; double* cost0;
    int* si; int* sj; int* err; int* moved;
    double lam, trunc;
    size_t plane;                                                 // N0 * N1
    int half;                                                     // 1: 32 pixels per wave (U > 11)
};

// pixels per wave and the dynamic LDS of a launch
inline int sequence_half(int ms) { const int U = 2 * ms - 1; return (size_t)U * U * 64 * sizeof(double) > 65536 ? 1 : 0; }
inline size_t sequence_lds(int ms, bool has_prev)
{
    // without a state only the epilogue uses LDS: the 4x4 neighbourhood in the first 16 slots (more waves fit a CU)
    const int U = 2 * ms - 1, slots = has_prev && U * U > 16 ? U * U : 16;
    return (size_t)slots * (64 >> sequence_half(ms)) * sizeof(double);
}

// The expressions of the definition that numpy must reproduce bit for bit: no contraction (the pragma lives in the helper,
// as in umpa_cost.h).
__device__ __forceinline__ double sequence_penalty(double lam, int d)
{
#pragma clang fp contract(off)
    return lam * (double)(d * d);
}

__device__ __forceinline__ double sequence_sum(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ double sequence_diff(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}

// One line of the box, `U` cells `stride` doubles apart, in place: out[o] = min_q (in[q] + pen[|o - q|]), q ascending, the
// minimum starting at +Inf and taking a candidate iff it is `<` the best so far (NaN and +Inf never win).
__device__ __forceinline__ void sequence_line(double* p, int stride, int U, const double (&pen)[UMPA_SEQUENCE_MAX_U])
{
    const double inf = __builtin_inf();
    double v[UMPA_SEQUENCE_MAX_U];
#pragma unroll
    for (int q = 0; q < UMPA_SEQUENCE_MAX_U; q++) v[q] = q < U ? p[q * stride] : inf;
#pragma unroll
    for (int o = 0; o < UMPA_SEQUENCE_MAX_U; o++) {
        if (o < U) {
            double best = inf;
#pragma unroll
            for (int q = 0; q < UMPA_SEQUENCE_MAX_U; q++) {
                if (q < U) {
                    const double c = sequence_sum(v[q], pen[o > q ? o - q : q - o]);
                    if (c < best) best = c;
                }
            }
            p[o * stride] = best;
        }
    }
}

template <int KIND, int NA>
__global__ void __launch_bounds__(64)
grid_sequence_kernel(ModelDev m, Maps M, ReplayArgs R, RegionArgs A, SequenceArgs B)
{
    extern __shared__ double sequence_lds_mem[];
    const int bwl = R.bw_log2, ls = 64 >> B.half;                     // ls: pixels per wave, the lane stride of the LDS slots
    if ((int)threadIdx.x >= ls) return;
    const int xj = (blockIdx.x << bwl) + (threadIdx.x & ((1 << bwl) - 1));
    const int xi = R.row0 + blockIdx.y * (ls >> bwl) + (threadIdx.x >> bwl);
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;                        // in the state and output planes
    const size_t tpx = grid_table_px(m, R, A, xi, xj);
    const int i = A.org0 + A.step0 * xi, j = A.org1 + A.step1 * xj;
    constexpr int NFIX = NA > 0 ? NA : UMPA_KFIX;
    double fixed[NFIX];
    PixConst pc;
    grid_pixel_consts<KIND, NA>(m, M, i, j, fixed, pc);

    const int ms = m.ms, ref_mode = m.ref_mode, U = 2 * ms - 1, U2 = U * U;
    double* const lane = sequence_lds_mem + threadIdx.x;             // slot s of this pixel: lane[s * ls]
    const double inf = __builtin_inf();
    const size_t plane = B.plane;

    // 1. the state, and its first strict minimum
    double m0 = inf;
    if (B.prev) {
        const UMPA_GLOBAL double* __restrict__ pv = gp(B.prev) + px;
#pragma unroll 1
        for (int s = 0; s < U2; s++) {
            const double v = pv[(size_t)s * plane];
            lane[s * ls] = v;
            if (v < m0) m0 = v;
        }
        // 2. rows (stage 2), then columns (stage 3), in place.  A pixel that never matched (m0 not below +Inf) goes through
        // the same code on whatever its state holds; its M is zero below.
        double pen[UMPA_SEQUENCE_MAX_U];
#pragma unroll
        for (int d = 0; d < UMPA_SEQUENCE_MAX_U; d++) pen[d] = sequence_penalty(B.lam, d);
#pragma unroll 1
        for (int l = 0; l < 2 * U; l++) {
            const bool col = l >= U;
            const int q = col ? l - U : l;
            sequence_line(lane + (col ? q : q * U) * ls, col ? U * ls : ls, U, pen);
        }
    }
    const bool live = m0 < inf;                                       // (false without prev)
    const double cap = sequence_sum(m0, B.trunc);

    // 3. the scan: A = C + M, the first strict minima of A and of C
    double best = inf, low = inf;
    int bpos = 0, lpos = 0;
    UMPA_GLOBAL double* __restrict__ nx = B.next ? gpw(B.next) + px : nullptr;
#pragma unroll 1
    for (int r = 0; r < U; r++) {
#pragma unroll 1
        for (int c = 0; c < U; c++) {
            const int s = r * U + c;
            double cost = 0.0;
            Fit fit = {0.0, 0.0};
            eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, r - (ms - 1), c - (ms - 1), fixed, pc, cost, fit);
            double mv = 0.0;
            if (live) {
                const double q = lane[s * ls];
                mv = sequence_diff(cap < q ? cap : q, m0);
            }
            const double a = sequence_sum(cost, mv);
            if (nx) nx[(size_t)s * plane] = a;
            if (a < best) { best = a; bpos = s; }
            if (cost < low) { low = cost; lpos = s; }
        }
    }

    gpw(B.cost0)[px] = low < inf ? low : 0.0;
    const bool found = best < inf;
    gpw(B.total)[px] = found ? best : 0.0;
    gpw(B.moved)[px] = found && bpos != lpos ? 1 : 0;

    auto cost_at = [&](int si, int sj) {                             // |si|, |sj| < ms
        double c = 0.0;
        Fit fit = {0.0, 0.0};
        eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, si, sj, fixed, pc, c, fit);
        return c;
    };
    double out = 0.0, uv0 = 0.0, uv1 = 0.0, cost = 0.0;
    Fit live_fit = {0.0, 0.0};
    int bi = 0, bj = 0, status = -1;
    if (found) {
        bi = bpos / U - (ms - 1); bj = bpos % U - (ms - 1);
        eval_lookup<KIND, NA>(m, M, R, ref_mode, i, j, tpx, bi, bj, fixed, pc, cost, live_fit);   // the scan's cost again, and T (df)
        out = cost; uv0 = bi; uv1 = bj;
        status = 0;
        // grid_track_kernel's epilogue, around this shift (the state is dead: its slots 0 .. 15 take the 4x4 neighbourhood)
        if (bi > 1 - ms && bi < ms - 1 && bj > 1 - ms && bj < ms - 1) {
            const int ip = cost_at(bi + 1, bj) < cost_at(bi - 1, bj) ? 1 : 0;   // Optim.cpp:344-345
            const int jp = cost_at(bi, bj + 1) < cost_at(bi, bj - 1) ? 1 : 0;
            const int i0 = bi + ip - 2, j0 = bj + jp - 2;
            if (i0 > -ms && i0 + 3 < ms && j0 > -ms && j0 + 3 < ms) {
#pragma unroll 1
                for (int g = 0; g < 16; g++) lane[g * ls] = cost_at(i0 + (g >> 2), j0 + (g & 3));
                double nb[16];
#pragma unroll
                for (int g = 0; g < 16; g++) nb[g] = lane[g * ls];
                double x = 1.0 - ip, y = 1.0 - jp;                  // Optim.cpp:395-396
                if (m.subpx == 0) out = x;                          // Optim.cpp:399
                else if (m.subpx == 1) out = spmin_quad(nb, x, y);
                else out = spmin(nb, x, y);
                uv0 = x + (bi + ip - 1.0);                          // Optim.cpp:407-408
                uv1 = y + (bj + jp - 1.0);
                status = 1;
            }
        }
        if (KIND == 1 && (live_fit.t != 0.0 || live_fit.v != 0.0)) live_fit.v = live_fit.v / live_fit.t;   // Model.cpp:854
    }
    gpw(B.f)[px] = out; gpw(B.T)[px] = live_fit.t; gpw(B.dx)[px] = uv1; gpw(B.dy)[px] = uv0; gpw(B.cost)[px] = cost;
    if (KIND == 1 && B.df) gpw(B.df)[px] = live_fit.v;
    gpw(B.si)[px] = bi; gpw(B.sj)[px] = bj; gpw(B.err)[px] = status;
}

} // namespace umpa
