// umpa_masked_grid_kernels.h -- the consumers of the MASKED tiled path's shift table in libumpa_grid.so.
//
// corr_masked (umpa_masked.h) leaves, for a row chunk of a model with masks, a table of FINISHED results for every integer
// shift of the search box: [(2 ms - 1)^2][NV][drows][N1d] doubles, per shift the planes cost, T and (NV = 3, dark-field) the
// dark-field value replay_cost stores as it stands.  replay_cost reads about 18 of those entries per pixel; the five kernels
// here read all.  Each is its sibling of umpa_grid_kernels.h, umpa_basins_kernels.h, umpa_track_kernels.h and
// umpa_sequence_kernels.h with ONE difference: an evaluation is a read of the table (masked_entry / masked_cost) instead of
// eval_lookup.  Scan order, the first strict minimum, "beats" and "basin", the LDS ring and the sequence state in LDS, the
// epilogue (quadrant rule, 4x4 neighbourhood, spmin / spmin_quad / none), store_pixel and the NaN rules are the siblings',
// word for word (include/umpa_grid.h), with C[s] the table's cost.  No per-frame work, hence no frame-count template.
//
//   masked_min_kernel       grid_min_kernel          masked_track_kernel      grid_track_kernel
//   masked_volume_kernel    cost_volume_kernel       masked_sequence_kernel   grid_sequence_kernel
//   masked_basins_kernel    grid_basins_kernel
//
// These kernels gather no maps: a pixel's traffic is its (2 ms - 1)^2 costs and three values at the winners.  A wave takes
// 64 pixels IN A ROW (32 where the sequence state needs the room: SequenceArgs::half), lane = column: every read of a table
// plane and every store of an output row is a run of consecutive doubles (with a column step > 1 the dense table is read
// strided).  The siblings' 16 x 4 blocks exist for the gathers of eval_lookup, which are not made here.
// No atomics, no barrier, nothing across lanes: the output does not depend on how pixels fall into waves or row chunks.
// The bodies are written out beside the siblings', not shared with them: the siblings' machine code stays what it was.
#pragma once
#include "umpa_sequence_kernels.h"

namespace umpa {

// where pixel (xi, xj) of the region sits in a plane of the chunk's table (replay_cost's own addressing)
__device__ __forceinline__ size_t masked_table_px(const ReplayArgs& R, const RegionArgs& A, int xi, int xj)
{
    return (size_t)(xi * A.step0 - R.drow0) * R.N1d + (size_t)xj * A.step1;
}

// the pixel's entry of shift (si, sj), |si|, |sj| < ms: e[0] the cost, e[slot_stride] T, e[2 slot_stride] the dark-field value
template <int KIND>
__device__ __forceinline__ const UMPA_GLOBAL double* masked_entry(const UMPA_GLOBAL double* px, size_t slot_stride, int ms, int si, int sj)
{
    constexpr int NV = KIND == 1 ? 3 : 2;
    return px + (size_t)((si + ms - 1) * (2 * ms - 1) + (sj + ms - 1)) * NV * slot_stride;
}

template <int KIND>
__device__ __forceinline__ double masked_cost(const UMPA_GLOBAL double* px, size_t slot_stride, int ms, int si, int sj)
{
    return masked_entry<KIND>(px, slot_stride, ms, si, sj)[0];
}

// T and the dark-field value of a shift, as replay_cost hands them to store_pixel: corr_masked has divided already
// (umpa_masked.h: dst[2 slot_stride] = K / T, Model.cpp:854), nothing is left to form
template <int KIND>
__device__ __forceinline__ Fit masked_fit(const UMPA_GLOBAL double* px, size_t slot_stride, int ms, int si, int sj)
{
    const UMPA_GLOBAL double* e = masked_entry<KIND>(px, slot_stride, ms, si, sj);
    Fit fit;
    fit.t = e[slot_stride];
    fit.v = KIND == 1 ? e[2 * slot_stride] : 0.0;
    return fit;
}

// grid_min_kernel's epilogue around the shift (bi, bj) for the kernels that keep the 4x4 neighbourhood in LDS (the first 16
// slots of the lane's column, `ls` doubles apart): the basins, track and sequence kernels.  `out`, `uv0`, `uv1` come in as
// the shift's cost and the shift; status: 1 with the sub-pixel fit, else 0.
template <int KIND>
__device__ __forceinline__ int masked_finish(const UMPA_GLOBAL double* tp, size_t ss, int ms, int subpx, int bi, int bj,
                                             double* lane, int ls, double& out, double& uv0, double& uv1)
{
    if (!(bi > 1 - ms && bi < ms - 1 && bj > 1 - ms && bj < ms - 1)) return 0;
    const int ip = masked_cost<KIND>(tp, ss, ms, bi + 1, bj) < masked_cost<KIND>(tp, ss, ms, bi - 1, bj) ? 1 : 0;   // Optim.cpp:344-345
    const int jp = masked_cost<KIND>(tp, ss, ms, bi, bj + 1) < masked_cost<KIND>(tp, ss, ms, bi, bj - 1) ? 1 : 0;
    const int i0 = bi + ip - 2, j0 = bj + jp - 2;
    if (!(i0 > -ms && i0 + 3 < ms && j0 > -ms && j0 + 3 < ms)) return 0;
#pragma unroll 1
    for (int g = 0; g < 16; g++) lane[g * ls] = masked_cost<KIND>(tp, ss, ms, i0 + (g >> 2), j0 + (g & 3));
    double nb[16];
#pragma unroll
    for (int g = 0; g < 16; g++) nb[g] = lane[g * ls];
    double x = 1.0 - ip, y = 1.0 - jp;                              // Optim.cpp:395-396
    if (subpx == 0) out = x;                                        // Optim.cpp:399
    else if (subpx == 1) out = spmin_quad(nb, x, y);
    else out = spmin(nb, x, y);
    uv0 = x + (bi + ip - 1.0);                                      // Optim.cpp:407-408
    uv1 = y + (bj + jp - 1.0);
    return 1;
}

// One lane per output pixel of the chunk, 64 pixels of one row per wave.
template <int KIND>
__global__ void __launch_bounds__(64)
masked_min_kernel(ModelDev m, ReplayArgs R, RegionArgs A)
{
    const int xj = blockIdx.x * 64 + threadIdx.x;
    const int xi = R.row0 + blockIdx.y;
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.pitch + xj;                     // in the output arrays
    if (A.cover && gp(A.cover)[px] < A.thr) return;
    const UMPA_GLOBAL double* tp = gp(R.table) + masked_table_px(R, A, xi, xj);
    const size_t ss = R.slot_stride;
    constexpr int NV = KIND == 1 ? 3 : 2;

    const int ms = m.ms, U = 2 * ms - 1;
    double best = __builtin_inf();
    int bi = 0, bj = 0;
    {
        const UMPA_GLOBAL double* e = tp;
        for (int si = 1 - ms; si < ms; si++)
            for (int sj = 1 - ms; sj < ms; sj++, e += NV * ss) {
                const double c = e[0];
                if (c < best) { best = c; bi = si; bj = sj; }        // the first strict minimum; a NaN never wins
            }
    }
    auto cost_at = [&](int si, int sj) { return masked_cost<KIND>(tp, ss, ms, si, sj); };   // |si|, |sj| < ms

    Walk w;                                                          // what store_pixel reads of a finished walk
    w.n = U * U;
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
        w.live = masked_fit<KIND>(tp, ss, ms, bi, bj);
        if (bi > 1 - ms && bi < ms - 1 && bj > 1 - ms && bj < ms - 1) {
            const int ip = cost_at(bi + 1, bj) < cost_at(bi - 1, bj) ? 1 : 0;   // Optim.cpp:344-345
            const int jp = cost_at(bi, bj + 1) < cost_at(bi, bj - 1) ? 1 : 0;
            const int i0 = bi + ip - 2, j0 = bj + jp - 2;            // cell (0, 0) of the 4x4 neighbourhood
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

// Every (shift, row) of the output is one coalesced run, and so is every read of the table: a copy of the wanted planes
// from the chunk's layout into the volume's.
template <int KIND>
__global__ void __launch_bounds__(64)
masked_volume_kernel(ModelDev m, ReplayArgs R, RegionArgs A, VolumeArgs V)
{
    const int xj = blockIdx.x * 64 + threadIdx.x;
    const int xi = R.row0 + blockIdx.y;
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;
    const size_t ss = R.slot_stride;
    constexpr int NV = KIND == 1 ? 3 : 2;
    const UMPA_GLOBAL double* e = gp(R.table) + masked_table_px(R, A, xi, xj);
    const int U2 = (2 * m.ms - 1) * (2 * m.ms - 1);
    size_t o = px;
    for (int s = 0; s < U2; s++, o += V.plane, e += NV * ss) {
        gpw(V.cost)[o] = e[0];
        if (V.T) gpw(V.T)[o] = e[ss];
        if (KIND == 1 && V.df) gpw(V.df)[o] = e[2 * ss];
    }
}

template <int KIND>
__global__ void __launch_bounds__(64)
masked_basins_kernel(ModelDev m, ReplayArgs R, RegionArgs A, BasinArgs B)
{
    extern __shared__ double masked_basin_lds[];
    const int xj = blockIdx.x * 64 + threadIdx.x;
    const int xi = R.row0 + blockIdx.y;
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;                        // in the output planes
    const int K = B.K;
    if (A.cover && gp(A.cover)[(size_t)xi * A.pitch + xj] < A.thr) return;
    const UMPA_GLOBAL double* tp = gp(R.table) + masked_table_px(R, A, xi, xj);
    const size_t ss = R.slot_stride;
    constexpr int NV = KIND == 1 ? 3 : 2;

    const int ms = m.ms, U = 2 * ms - 1;
    double* const lane = masked_basin_lds + threadIdx.x;             // cell (row, column) of the ring: lane[((row % 3) * U + column) * 64]
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
            const UMPA_GLOBAL double* e = tp + (size_t)r * U * NV * ss;
#pragma unroll 1
            for (int c = 0; c < U; c++, e += NV * ss) row[c * 64] = e[0];
        }
        if (r == 0) continue;
        // row q = r - 1 has its neighbours (grid_basins_kernel's window: NaN outside the box, `<=` for the neighbours that
        // precede in scan order, `<` for the others)
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
                    if (moving) { const double tc = bc[k]; const int tq = bp[k]; bc[k] = ic; bp[k] = ip; ic = tc; ip = tq; }
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

#pragma unroll 1
    for (int k = 0; k < K; k++) {
        const size_t o = (size_t)k * B.plane + px;
        double out = 0.0, uv0 = 0.0, uv1 = 0.0, cost = 0.0;
        Fit live = {0.0, 0.0};
        int bi = 0, bj = 0, status = -1;
        if (k < count) {
            const int p = (int)lane[(24 + k) * 64];
            bi = p / U - (ms - 1); bj = p % U - (ms - 1);
            cost = masked_cost<KIND>(tp, ss, ms, bi, bj);            // the ring's cost again, and T (df)
            live = masked_fit<KIND>(tp, ss, ms, bi, bj);
            out = cost; uv0 = bi; uv1 = bj;
            status = masked_finish<KIND>(tp, ss, ms, m.subpx, bi, bj, lane, 64, out, uv0, uv1);
        }
        gpw(B.f)[o] = out; gpw(B.T)[o] = live.t; gpw(B.dx)[o] = uv1; gpw(B.dy)[o] = uv0; gpw(B.cost)[o] = cost;
        if (KIND == 1 && B.df) gpw(B.df)[o] = live.v;
        gpw(B.si)[o] = bi; gpw(B.sj)[o] = bj; gpw(B.err)[o] = status;
    }
}

template <int KIND>
__global__ void __launch_bounds__(64)
masked_track_kernel(ModelDev m, ReplayArgs R, RegionArgs A, TrackArgs B)
{
    extern __shared__ double masked_track_lds[];
    const int xj = blockIdx.x * 64 + threadIdx.x;
    const int xi = R.row0 + blockIdx.y;
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;                        // in the prior and output planes
    const UMPA_GLOBAL double* tp = gp(R.table) + masked_table_px(R, A, xi, xj);
    const size_t ss = R.slot_stride;
    constexpr int NV = KIND == 1 ? 3 : 2;

    const int ms = m.ms, U = 2 * ms - 1;
    double* const lane = masked_track_lds + threadIdx.x;             // cell (row, column) of the ring: lane[((row % 3) * U + column) * 64]
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
            const UMPA_GLOBAL double* e = tp + (size_t)r * U * NV * ss;
#pragma unroll 1
            for (int c = 0; c < U; c++, e += NV * ss) row[c * 64] = e[0];
        }
        if (r == 0) continue;
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

    double out = 0.0, uv0 = 0.0, uv1 = 0.0, cost = 0.0;
    Fit live = {0.0, 0.0};
    int bi = 0, bj = 0, status = -1;
    if (found > 0) {
        bi = bpos / U - (ms - 1); bj = bpos % U - (ms - 1);
        cost = masked_cost<KIND>(tp, ss, ms, bi, bj);                // the ring's cost again, and T (df)
        live = masked_fit<KIND>(tp, ss, ms, bi, bj);
        out = cost; uv0 = bi; uv1 = bj;
        status = masked_finish<KIND>(tp, ss, ms, m.subpx, bi, bj, lane, 64, out, uv0, uv1);   // (the ring is dead)
    }
    gpw(B.f)[px] = out; gpw(B.T)[px] = live.t; gpw(B.dx)[px] = uv1; gpw(B.dy)[px] = uv0; gpw(B.cost)[px] = cost;
    if (KIND == 1 && B.df) gpw(B.df)[px] = live.v;
    gpw(B.si)[px] = bi; gpw(B.sj)[px] = bj; gpw(B.err)[px] = status;
}

template <int KIND>
__global__ void __launch_bounds__(64)
masked_sequence_kernel(ModelDev m, ReplayArgs R, RegionArgs A, SequenceArgs B)
{
    extern __shared__ double masked_sequence_lds[];
    const int ls = 64 >> B.half;                                     // pixels per wave, the lane stride of the LDS slots
    if ((int)threadIdx.x >= ls) return;
    const int xj = blockIdx.x * ls + threadIdx.x;
    const int xi = R.row0 + blockIdx.y;
    if (xi >= R.row0 + R.rows || xj >= A.N1) return;
    const size_t px = (size_t)xi * A.N1 + xj;                        // in the state and output planes
    const UMPA_GLOBAL double* tp = gp(R.table) + masked_table_px(R, A, xi, xj);
    const size_t ss = R.slot_stride;
    constexpr int NV = KIND == 1 ? 3 : 2;

    const int ms = m.ms, U = 2 * ms - 1, U2 = U * U;
    double* const lane = masked_sequence_lds + threadIdx.x;          // slot s of this pixel: lane[s * ls]
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
        // 2. rows (stage 2), then columns (stage 3), in place (grid_sequence_kernel)
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
    {
        const UMPA_GLOBAL double* e = tp;
#pragma unroll 1
        for (int s = 0; s < U2; s++, e += NV * ss) {
            const double cost = e[0];
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

    double out = 0.0, uv0 = 0.0, uv1 = 0.0, cost = 0.0;
    Fit live_fit = {0.0, 0.0};
    int bi = 0, bj = 0, status = -1;
    if (found) {
        bi = bpos / U - (ms - 1); bj = bpos % U - (ms - 1);
        cost = masked_cost<KIND>(tp, ss, ms, bi, bj);                // the scan's cost again, and T (df)
        live_fit = masked_fit<KIND>(tp, ss, ms, bi, bj);
        out = cost; uv0 = bi; uv1 = bj;
        status = masked_finish<KIND>(tp, ss, ms, m.subpx, bi, bj, lane, ls, out, uv0, uv1);   // (the state is dead)
    }
    gpw(B.f)[px] = out; gpw(B.T)[px] = live_fit.t; gpw(B.dx)[px] = uv1; gpw(B.dy)[px] = uv0; gpw(B.cost)[px] = cost;
    if (KIND == 1 && B.df) gpw(B.df)[px] = live_fit.v;
    gpw(B.si)[px] = bi; gpw(B.sj)[px] = bj; gpw(B.err)[px] = status;
}

} // namespace umpa
