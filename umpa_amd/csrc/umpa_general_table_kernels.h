// umpa_general_table_kernels.h -- the general shift-table kernel of libumpa_grid.so.
//
// The consumers of umpa_masked_grid_kernels.h read a table of FINISHED results -- [(2 ms - 1)^2][NV][rows][N1d] doubles, per
// shift the planes cost, T and (NV = 3, dark-field) the dark-field value -- and do no per-frame work: they do not care who
// filled it.  corr_masked fills it for the masked models the tiled path takes.  general_table_kernel fills it for every
// model the general walk kernels take (match_direct / match_staged, umpa_direct.h): frames at different positions (sample
// stepping) and of unequal shapes, masks of any kind, both coordinate conventions, any window and search range.  The kernel
// dark-field model stays out: it has no per-shift table.
//
// An entry is what eval_direct<KIND, MASK> returns for the pixel and the shift -- cost, fit.t, fit.v -- bit for bit, hence
// what cost_one_kernel gives (umpa_hip_cost).  Per (pixel, shift) the terms are eval_direct's in eval_direct's order: frames
// outer, window rows, window columns; frame_misses per pixel and frame; wt = Na without masks and the sum of the pair weights
// (pair_weight, not pair_weight_fast) with them.  As in match_staged, the windows are served from LDS: a workgroup of
// UMPA_STAGED_BX x UMPA_STAGED_BY pixels stages, per frame, the footprints of StagedGeom -- the pixel box widened by Nw for
// the stack whose window stays, by Nw + ms - 1 for the one that moves and for the masks -- with coalesced loads clamped to
// the frame's own rectangle (what is clamped is never read by a lane the frame contributes to), and every lane sums its own
// windows out of LDS.
//
// Blocking.  Registers do not hold (2 ms - 1)^2 accumulator sets, and ms is a run-time value: a pass takes one shift row
// and UMPA_GENERAL_CJ consecutive column shifts, keeps that many accumulator sets, and goes through the frames, which are
// restaged per pass (a footprint is ~10 loads per lane, a pass 6 * CJ * (2 Nw + 1)^2 FMAs per lane and frame).  The last
// pass of a shift row may reach past ms - 1: those sets repeat shift ms - 1 (every LDS address stays that of a valid shift)
// and are not stored.  The window weights are read from LDS as a broadcast; the lanes of a pixel row read consecutive
// doubles.
//
// Layout.  The table lies on the OUTPUT grid: rows = the chunk's output rows, N1d = the region's N1 -- only requested pixels
// are computed at steps > 1.  The masked kernels use the region's steps in masked_table_px alone, so the host hands them a
// copy of RegionArgs with unit steps and R.drow0 = the chunk's first output row.
//
// Where the footprints do not fit LDS (general_geometry: large steps), GeneralArgs::staged is 0 and every lane evaluates its
// shifts through eval_direct itself from global memory: the same bits.
// A pixel no frame contributes to gets what eval_direct gives it: 0 / 0, NaN costs.
#pragma once
#include "umpa_direct.h"
#include "umpa_general_geom.h"

namespace umpa {

#define UMPA_GENERAL_CJ 4            // column shifts per pass

struct GeneralArgs {
    double* table;                   // [(2ms-1)^2][NV][rows][N1]
    size_t slot_stride;              // rows * N1
    int row0, rows;                  // the chunk's output rows [row0, row0 + rows)
    int staged;                      // 1: windows out of LDS (G is valid); 0: eval_direct from global memory
};

// staged_geometry (umpa_hip.hip) for this kernel: the same footprints; no walk memo beside them, no register staging and
// hence no cap on their rows and columns other than the 64 KiB of LDS a kernel gets without asking
inline bool general_geometry(const ModelDev& m, bool has_mask, const RegionArgs& A, StagedGeom& G, size_t& lds_bytes)
{
    GeneralFootprints F;                                              // umpa_general_geom.h: the arithmetic, on plain ints
    const bool fits = general_footprints(m.Nw, m.ms, m.ref_mode, has_mask, A.step0, A.step1, UMPA_STAGED_BY, UMPA_STAGED_BX, F);
    if (!F.lds_bytes) return false;                                   // (a box past UMPA_GENERAL_MAX_SIDE: G and lds_bytes stay)
    lds_bytes = F.lds_bytes;
    G.hq = F.hq; G.hr = F.hr; G.hm = F.hm;
    G.rowsQ = F.rowsQ; G.colsQ = F.colsQ; G.rowsR = F.rowsR; G.colsR = F.colsR; G.rowsM = F.rowsM; G.colsM = F.colsM;
    G.offR = F.offR; G.offM = F.offM; G.offW = F.offW;
    return fits;
}

template <int KIND, bool MASK>
__global__ void __launch_bounds__(UMPA_STAGED_THREADS)
general_table_kernel(ModelDev m, RegionArgs A, GeneralArgs T, StagedGeom G)
{
    extern __shared__ __attribute__((aligned(16))) char general_raw[];
    constexpr int NV = KIND == 1 ? 3 : 2, CJ = UMPA_GENERAL_CJ;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * UMPA_STAGED_BX + tx;
    const int xj = blockIdx.x * UMPA_STAGED_BX + tx, xi = T.row0 + blockIdx.y * UMPA_STAGED_BY + ty;
    const bool active = xi < T.row0 + T.rows && xj < A.N1;
    const int i = A.org0 + A.step0 * xi, j = A.org1 + A.step1 * xj;
    const int ms = m.ms, U = 2 * ms - 1;
    const size_t ss = T.slot_stride;
    UMPA_GLOBAL double* dst = gpw(T.table) + ((size_t)(active ? xi - T.row0 : 0) * A.N1 + (active ? xj : 0));
    if (ms < 1) return;

    if (!T.staged) {                                                  // (a kernel argument: the whole grid goes one way)
        if (!active) return;
        for (int si = 1 - ms; si < ms; si++)
            for (int sj = 1 - ms; sj < ms; sj++) {
                double c = 0.0;
                Fit fit = {0.0, 0.0};
                (void)eval_direct<KIND, MASK>(m, i, j, si, sj, c, fit);
                UMPA_GLOBAL double* e = dst + (size_t)((si + ms - 1) * U + (sj + ms - 1)) * NV * ss;
                e[0] = c; e[ss] = fit.t;
                if (KIND == 1) e[2 * ss] = fit.v;
            }
        return;
    }

    double* fq = reinterpret_cast<double*>(general_raw);
    double* fr = fq + G.offR;
    double* fm = fq + G.offM;
    double* wl = fq + G.offW;                                         // the window: every lane reads the same weight (LDS broadcast)
    // The index arithmetic from here on -- the box origin, q0 / r0 / mq0 / mr0, dc and the clamped source of a staged element --
    // is restated term for term in umpa_general_geom.h (general_box_origin, general_window_origin, general_set_offset,
    // general_source), which tests/general_addr_check.cpp sweeps on the host: change one and change the other.
    const int gi0 = A.org0 + A.step0 * (T.row0 + blockIdx.y * UMPA_STAGED_BY), gj0 = A.org1 + A.step1 * (blockIdx.x * UMPA_STAGED_BX);   // box origin
    const int Nw = m.Nw, S = 2 * Nw + 1, pad = m.padding;
    for (int q = tid; q < S * S; q += UMPA_STAGED_THREADS) wl[q] = gp(m.win)[q];   // (read behind the first frame's barriers)

    for (int si = 1 - ms; si < ms; si++) {
        for (int sj0 = 1 - ms; sj0 < ms; sj0 += CJ) {
            // window origins inside the staged footprints of the pass's first shift (si, sj0); set c of the pass is the
            // shift (si, sj0 + dc), dc = min(c, ms - 1 - sj0): its window lies dc columns further (reference, 'sam' mode) or
            // nearer (sample, 'ref' mode)
            int ri = i, rj = j, qi = i, qj = j;                      // Model.cpp:408-421 / :688-701
            if (m.ref_mode) { qi -= si; qj -= sj0; } else { ri += si; rj += sj0; }
            const int q0 = (qi - Nw - (gi0 - G.hq)) * G.colsQ + (qj - Nw - (gj0 - G.hq));     // general_window_origin (umpa_general_geom.h)
            const int r0 = (ri - Nw - (gi0 - G.hr)) * G.colsR + (rj - Nw - (gj0 - G.hr));
            const int mq0 = (qi - Nw - (gi0 - G.hm)) * G.colsM + (qj - Nw - (gj0 - G.hm));
            const int mr0 = (ri - Nw - (gi0 - G.hm)) * G.colsM + (rj - Nw - (gj0 - G.hm));
            int dq[CJ], dr[CJ];
#pragma unroll
            for (int c = 0; c < CJ; c++) {
                const int dc = min(c, ms - 1 - sj0);                  // general_set_offset (umpa_general_geom.h)
                dq[c] = m.ref_mode ? -dc : 0;
                dr[c] = m.ref_mode ? 0 : dc;
            }
            double t1[CJ], t2[CJ], t3[CJ], t4[CJ], t5[CJ], t6[CJ], wt[CJ];
#pragma unroll
            for (int c = 0; c < CJ; c++) {
                t1[c] = 0; t2[c] = 0; t3[c] = 0; t4[c] = 0; t5[c] = 0; t6[c] = 0;
                wt[c] = MASK ? 0.0 : (double)m.Na;                   // Model.cpp:425,:711 / :463,:777
            }

            for (int k = 0; k < m.Na; k++) {
                const FrameDesc f = load_frame(m.frames, k);
                __syncthreads();                                      // the previous frame's footprints have been read
                // ---- footprints of frame k.  Frame coordinates = image coordinates - position, clamped at the frame
                // edges: every address lies inside the frame, and what is clamped is never read by a lane the frame
                // contributes to.  The clamp is general_source's (umpa_general_geom.h).
                {
                    const int fi0 = gi0 - f.pi, fj0 = gj0 - f.pj;
                    for (int q = tid; q < G.rowsQ * G.colsQ; q += UMPA_STAGED_THREADS) {
                        const int r = q / G.colsQ, c = q - r * G.colsQ;
                        fq[q] = gp(f.sam)[(size_t)min(max(fi0 - G.hq + r, 0), f.H - 1) * f.W + min(max(fj0 - G.hq + c, 0), f.W - 1)];
                    }
                    for (int q = tid; q < G.rowsR * G.colsR; q += UMPA_STAGED_THREADS) {
                        const int r = q / G.colsR, c = q - r * G.colsR;
                        fr[q] = gp(f.ref)[(size_t)min(max(fi0 - G.hr + r, 0), f.H - 1) * f.W + min(max(fj0 - G.hr + c, 0), f.W - 1)];
                    }
                    if (MASK)
                        for (int q = tid; q < G.rowsM * G.colsM; q += UMPA_STAGED_THREADS) {
                            const int r = q / G.colsM, c = q - r * G.colsM;
                            fm[q] = gp(f.mask)[(size_t)min(max(fi0 - G.hm + r, 0), f.H - 1) * f.W + min(max(fj0 - G.hm + c, 0), f.W - 1)];
                        }
                }
                __syncthreads();
                const int li = i - f.pi, lj = j - f.pj;              // Model.cpp:430-433 / :716-719
                if (!active || frame_misses(f.H, f.W, li, lj, pad)) continue;
                double s2[CJ], s4[CJ], s6[CJ], sm[CJ];
#pragma unroll
                for (int c = 0; c < CJ; c++) { s2[c] = 0; s4[c] = 0; s6[c] = 0; sm[c] = 0; }
                constexpr int CH = 8;
                for (int a = 0; a < S; a++) {
                    const double* wrow = wl + a * S;
                    const double* __restrict__ Q = fq + q0 + a * G.colsQ;
                    const double* __restrict__ R = fr + r0 + a * G.colsR;
                    const double* __restrict__ MQ = fm + mq0 + a * G.colsM;
                    const double* __restrict__ MR = fm + mr0 + a * G.colsM;
                    for (int b0 = 0; b0 < S; b0 += CH) {
                        double wv[CH];
#pragma unroll
                        for (int b = 0; b < CH; b++) wv[b] = b0 + b < S ? wrow[b0 + b] : 0.0;
#pragma unroll
                        for (int c = 0; c < CJ; c++) {
                            // a window row of set c at a time: all its LDS reads are issued before the first term is summed
                            double rv[CH], qv[CH], mrv[CH], mqv[CH];
#pragma unroll
                            for (int b = 0; b < CH; b++) {
                                const bool in = b0 + b < S;
                                rv[b] = in ? R[dr[c] + b0 + b] : 0.0;
                                qv[b] = in ? Q[dq[c] + b0 + b] : 0.0;
                                mrv[b] = (MASK && in) ? MR[dr[c] + b0 + b] : 0.0;
                                mqv[b] = (MASK && in) ? MQ[dq[c] + b0 + b] : 0.0;
                            }
#pragma unroll
                            for (int b = 0; b < CH; b++)
                                if (b0 + b < S) {
                                    // one window element: the arithmetic and the order of Model.cpp:746-772 (and :813-841
                                    // with masks), as in eval_direct
                                    double w = wv[b];
                                    const double r = rv[b], q = qv[b];
                                    if (MASK) {
                                        if (KIND == 1) sm[c] += w * r;   // the ref mean is never mask-weighted (Model.cpp:804)
                                        w *= pair_weight(mrv[b], mqv[b]);
                                        wt[c] += w;
                                        s2[c] += w;
                                    }
                                    const double wq = w * q, wr = w * r;
                                    t1[c] += wq * q;
                                    t3[c] += wr * r;
                                    t5[c] += wr * q;
                                    if (KIND == 1) { s4[c] += wq; s6[c] += wr; }
                                }
                        }
                    }
                }
                if (KIND == 1) {                                     // Model.cpp:739,:770-772 / :808,:843-845
#pragma unroll
                    for (int c = 0; c < CJ; c++) {
                        const double mean = (MASK ? sm[c] : s6[c]) / m.win_sum;
                        t2[c] += MASK ? mean * mean * s2[c] : mean * mean;
                        t4[c] += mean * s4[c];
                        t6[c] += mean * s6[c];
                    }
                }
            }

            if (active) {
#pragma unroll
                for (int c = 0; c < CJ; c++) {
                    if (sj0 + c >= ms) continue;
                    double cost, ft, fv;
                    if (KIND == 1) {                                 // Model.cpp:849-858
                        const double det = t2[c] * t3[c] - t6[c] * t6[c];
                        const double K = (t2[c] * t5[c] - t4[c] * t6[c]) / det;
                        const double beta = (t3[c] * t4[c] - t5[c] * t6[c]) / det;
                        ft = beta + K;
                        fv = K / ft;
                        cost = (t1[c] + beta * beta * t2[c] + K * K * t3[c] - 2 * beta * t4[c] - 2 * K * t5[c] + 2 * beta * K * t6[c]) / wt[c];
                    } else {                                         // Model.cpp:502-505
                        ft = t5[c] / t3[c];
                        fv = 0.0;
                        cost = (t1[c] - t5[c] * ft) / wt[c];
                    }
                    UMPA_GLOBAL double* e = dst + (size_t)((si + ms - 1) * U + (sj0 + c + ms - 1)) * NV * ss;
                    e[0] = cost; e[ss] = ft;
                    if (KIND == 1) e[2 * ss] = fv;
                }
            }
        }
    }
}

} // namespace umpa
