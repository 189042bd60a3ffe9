// umpa_resident_kernels.h -- the kernel family of umpa_grid_uncertainty (include/umpa_grid.h, "Model-resident uncertainty"):
//   resident_moments_kernel<KIND, MASKED>   one lane per pixel: the windowed moments over all frames of the MODEL'S OWN device
//                                           frames (ModelDev, umpa_direct.h), then the solve on them
// KIND 0 plain, 1 dark-field; MASKED: the model has masks and the pair weight enters the window weight.  Four instantiations.
// The unmasked pair computes the operation of include/umpa_sigma.h, expression for expression (libumpa_sigma.so's
// sigma_moments_kernel on two bare stacks); the masked pair the definition written out in include/umpa_grid.h.
// libumpa_grid.so is built with the compiler's default contraction; every function here switches it off for its own body
// (#pragma clang fp contract(off)): the solve is + - * / in the header's order and nothing else, the sums say fma() where
// they mean one.  No atomics, one writer per output, no LDS.
#pragma once
#include "umpa_direct.h"

namespace umpa {

#define RESIDENT_INF (__builtin_huge_val())
#define RESIDENT_NAN (__builtin_nan(""))
#define RESIDENT_SKIP (-2147483647 - 1)                  // UMPA_SIGMA_SKIP (include/umpa_sigma.h)
#define RESIDENT_MAX_NW 8                                // UMPA_SIGMA_MAX_NW
constexpr int RESIDENT_TILE_X = 32, RESIDENT_TILE_Y = 8;   // pixels of one workgroup: 32 columns x 8 rows

// planes per pixel and unknowns of the linearised model
template <int KIND, bool MASKED> struct ResidentPlanes {
    static constexpr int P = MASKED ? (KIND ? 50 : 17) : (KIND ? 34 : 16), N = KIND ? 4 : 3;
};

// The plane indices: 0 .. 15 are common to all four; the unmasked dark-field planes are include/umpa_sigma.h's, the masked
// ones include/umpa_grid.h's.
enum { RS_S00, RS_S01, RS_S02, RS_S11, RS_S12, RS_S22, RS_V00, RS_V01, RS_V02, RS_V11, RS_V12, RS_V22, RS_P0, RS_P1, RS_P2, RS_QQ };
enum { RS_MM00 = 16, RS_MM01, RS_MM02, RS_MM11, RS_MM12, RS_MM22, RS_NM00, RS_NM01, RS_NM02, RS_NM10, RS_NM11, RS_NM12, RS_NM20, RS_NM21,
       RS_NM22, RS_AM0, RS_AM1, RS_AM2 };
enum { RS_WW = 16, RS_MU00, RS_MU01, RS_MU02, RS_MU10, RS_MU11, RS_MU12, RS_MU20, RS_MU21, RS_MU22,
       RS_WM00, RS_WM01, RS_WM02, RS_WM11, RS_WM12, RS_WM22, RS_NU00, RS_NU01, RS_NU02, RS_NU10, RS_NU11, RS_NU12, RS_NU20, RS_NU21, RS_NU22,
       RS_VM00, RS_VM01, RS_VM02, RS_VM11, RS_VM12, RS_VM22, RS_AU0, RS_AU1, RS_AU2 };

__device__ __forceinline__ bool resident_finite(double x) { return x > -RESIDENT_INF && x < RESIDENT_INF; }

// x = A^-1 b by the factors L, D of the header's SOLVE
template <int N>
__device__ __forceinline__ void resident_ldl_solve(const double (&L)[N][N], const double (&D)[N], const double (&b)[N], double (&x)[N])
{
#pragma clang fp contract(off)
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        y[i] = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) y[i] = y[i] - L[i][k] * y[k];
    }
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = y[i] / D[i];
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
#pragma unroll
        for (int k = i + 1; k < N; k++) x[i] = x[i] - L[k][i] * x[k];
    }
}

// MODEL and SOLVE on the moments m[] of one pixel: writes unit (three planes `plane` apart), s2, dof and valid at `at`.
// Unmasked: include/umpa_sigma.h's, dof = K - tr.  Masked: include/umpa_grid.h's, dof = W - tr.
template <int KIND, bool MASKED>
__device__ __forceinline__ void resident_solve(const double (&m)[ResidentPlanes<KIND, MASKED>::P], const double sv, const int K,
                                               const size_t at, const size_t plane, double* __restrict__ unit,
                                               double* __restrict__ s2, double* __restrict__ dof, int* __restrict__ valid)
{
#pragma clang fp contract(off)
    constexpr int N = ResidentPlanes<KIND, MASKED>::N;
    double A[N][N], B[N][N], h[N], rss0;
    if constexpr (KIND == 0) {
        const double T = m[RS_P2] / m[RS_S22], TT = T * T;
        A[0][0] = TT * m[RS_S00]; A[1][0] = TT * m[RS_S01]; A[1][1] = TT * m[RS_S11];
        A[2][0] = T * m[RS_S02]; A[2][1] = T * m[RS_S12]; A[2][2] = m[RS_S22];
        B[0][0] = TT * m[RS_V00]; B[1][0] = TT * m[RS_V01]; B[1][1] = TT * m[RS_V11];
        B[2][0] = T * m[RS_V02]; B[2][1] = T * m[RS_V12]; B[2][2] = m[RS_V22];
        h[0] = T * (m[RS_P0] - T * m[RS_S02]);
        h[1] = T * (m[RS_P1] - T * m[RS_S12]);
        h[2] = m[RS_P2] - T * m[RS_S22];
        rss0 = m[RS_QQ] - m[RS_P2] * T;
    } else if constexpr (!MASKED) {
        const double t1 = m[RS_QQ], t2 = m[RS_MM22], t3 = m[RS_S22], t4 = m[RS_AM2], t5 = m[RS_P2], t6 = m[RS_MM22];
        const double det = t2 * t3 - t6 * t6;
        const double Kc = (t2 * t5 - t4 * t6) / det;
        const double beta = (t3 * t4 - t5 * t6) / det;
        const double KK = Kc * Kc, c = (2 * Kc) * beta + beta * beta, bb = (beta * beta) * sv, kb = Kc * beta, bs = beta * sv;
        A[0][0] = KK * m[RS_S00] + c * m[RS_MM00]; A[1][0] = KK * m[RS_S01] + c * m[RS_MM01]; A[1][1] = KK * m[RS_S11] + c * m[RS_MM11];
        A[2][0] = (Kc + beta) * m[RS_MM02]; A[2][1] = (Kc + beta) * m[RS_MM12];
        A[3][0] = Kc * m[RS_S02] + beta * m[RS_MM02]; A[3][1] = Kc * m[RS_S12] + beta * m[RS_MM12];
        A[2][2] = m[RS_MM22]; A[3][2] = m[RS_MM22]; A[3][3] = m[RS_S22];
        B[0][0] = (KK * m[RS_V00] + kb * (m[RS_NM00] + m[RS_NM00])) + bb * m[RS_MM00];
        B[1][0] = (KK * m[RS_V01] + kb * (m[RS_NM01] + m[RS_NM10])) + bb * m[RS_MM01];
        B[1][1] = (KK * m[RS_V11] + kb * (m[RS_NM11] + m[RS_NM11])) + bb * m[RS_MM11];
        B[2][0] = Kc * m[RS_NM02] + bs * m[RS_MM02]; B[2][1] = Kc * m[RS_NM12] + bs * m[RS_MM12];
        B[3][0] = Kc * m[RS_V02] + beta * m[RS_NM20]; B[3][1] = Kc * m[RS_V12] + beta * m[RS_NM21];
        B[2][2] = sv * m[RS_MM22]; B[3][2] = m[RS_NM22]; B[3][3] = m[RS_V22];
        h[0] = Kc * ((m[RS_P0] - beta * m[RS_MM02]) - Kc * m[RS_S02]) + beta * ((m[RS_AM0] - beta * m[RS_MM02]) - Kc * m[RS_MM02]);
        h[1] = Kc * ((m[RS_P1] - beta * m[RS_MM12]) - Kc * m[RS_S12]) + beta * ((m[RS_AM1] - beta * m[RS_MM12]) - Kc * m[RS_MM12]);
        h[2] = (m[RS_AM2] - beta * m[RS_MM22]) - Kc * m[RS_MM22];
        h[3] = (m[RS_P2] - beta * m[RS_MM22]) - Kc * m[RS_S22];
        rss0 = ((((t1 + (beta * beta) * t2) + (Kc * Kc) * t3) - (2 * beta) * t4) - (2 * Kc) * t5) + ((2 * beta) * Kc) * t6;
    } else {
        const double t1 = m[RS_QQ], t2 = m[RS_WM22], t3 = m[RS_S22], t4 = m[RS_AU2], t5 = m[RS_P2], t6 = m[RS_MU22];
        const double det = t2 * t3 - t6 * t6;
        const double Kc = (t2 * t5 - t4 * t6) / det;
        const double beta = (t3 * t4 - t5 * t6) / det;
        const double KK = Kc * Kc, kb = Kc * beta, bb = beta * beta;
        A[0][0] = (KK * m[RS_S00] + kb * (m[RS_MU00] + m[RS_MU00])) + bb * m[RS_WM00];
        A[1][0] = (KK * m[RS_S01] + kb * (m[RS_MU01] + m[RS_MU10])) + bb * m[RS_WM01];
        A[1][1] = (KK * m[RS_S11] + kb * (m[RS_MU11] + m[RS_MU11])) + bb * m[RS_WM11];
        A[2][0] = Kc * m[RS_MU02] + beta * m[RS_WM02]; A[2][1] = Kc * m[RS_MU12] + beta * m[RS_WM12];
        A[3][0] = Kc * m[RS_S02] + beta * m[RS_MU20]; A[3][1] = Kc * m[RS_S12] + beta * m[RS_MU21];
        A[2][2] = m[RS_WM22]; A[3][2] = m[RS_MU22]; A[3][3] = m[RS_S22];
        B[0][0] = (KK * m[RS_V00] + kb * (m[RS_NU00] + m[RS_NU00])) + bb * m[RS_VM00];
        B[1][0] = (KK * m[RS_V01] + kb * (m[RS_NU01] + m[RS_NU10])) + bb * m[RS_VM01];
        B[1][1] = (KK * m[RS_V11] + kb * (m[RS_NU11] + m[RS_NU11])) + bb * m[RS_VM11];
        B[2][0] = Kc * m[RS_NU02] + beta * m[RS_VM02]; B[2][1] = Kc * m[RS_NU12] + beta * m[RS_VM12];
        B[3][0] = Kc * m[RS_V02] + beta * m[RS_NU20]; B[3][1] = Kc * m[RS_V12] + beta * m[RS_NU21];
        B[2][2] = m[RS_VM22]; B[3][2] = m[RS_NU22]; B[3][3] = m[RS_V22];
        h[0] = Kc * ((m[RS_P0] - beta * m[RS_MU02]) - Kc * m[RS_S02]) + beta * ((m[RS_AU0] - beta * m[RS_WM02]) - Kc * m[RS_MU20]);
        h[1] = Kc * ((m[RS_P1] - beta * m[RS_MU12]) - Kc * m[RS_S12]) + beta * ((m[RS_AU1] - beta * m[RS_WM12]) - Kc * m[RS_MU21]);
        h[2] = (m[RS_AU2] - beta * m[RS_WM22]) - Kc * m[RS_MU22];
        h[3] = (m[RS_P2] - beta * m[RS_MU22]) - Kc * m[RS_S22];
        rss0 = ((((t1 + (beta * beta) * t2) + (Kc * Kc) * t3) - (2 * beta) * t4) - (2 * Kc) * t5) + ((2 * beta) * Kc) * t6;
    }
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i + 1; j < N; j++) { A[i][j] = A[j][i]; B[i][j] = B[j][i]; }

    double L[N][N], D[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        D[j] = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) D[j] = D[j] - (L[j][k] * L[j][k]) * D[k];
        ok = ok && D[j] > 0.0 && D[j] < RESIDENT_INF;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) t = t - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = t / D[j];
        }
    }
    double X[N][N], tr = 0.0;                       // X[q] = A^-1 (column q of B)
#pragma unroll
    for (int q = 0; q < N; q++) {
        double b[N];
#pragma unroll
        for (int i = 0; i < N; i++) b[i] = B[i][q];
        resident_ldl_solve<N>(L, D, b, X[q]);
        tr = q == 0 ? X[0][0] : tr + X[q][q];
    }
    double r0[N], r1[N], Y0[N], Y1[N], d[N];
#pragma unroll
    for (int q = 0; q < N; q++) { r0[q] = X[q][0]; r1[q] = X[q][1]; }
    resident_ldl_solve<N>(L, D, r0, Y0);
    resident_ldl_solve<N>(L, D, r1, Y1);
    resident_ldl_solve<N>(L, D, h, d);
    double hd = h[0] * d[0] + h[1] * d[1];
#pragma unroll
    for (int i = 2; i < N; i++) hd = hd + h[i] * d[i];
    const double rr = rss0 - hd;
    double df;
    if constexpr (MASKED) df = m[RS_WW] - tr;
    else df = (double)K - tr;
    const double rss = rr > 0.0 ? rr : 0.0;
    const double s = rss / df;
    ok = ok && df > 0.0 && resident_finite(Y0[0]) && resident_finite(Y1[1]) && resident_finite(Y1[0]) && resident_finite(rr) &&
         resident_finite(df) && resident_finite(s);
    unit[at] = ok ? Y0[0] : RESIDENT_NAN;
    unit[plane + at] = ok ? Y1[1] : RESIDENT_NAN;
    unit[2 * plane + at] = ok ? Y1[0] : RESIDENT_NAN;
    s2[at] = ok ? s : RESIDENT_NAN;
    dof[at] = ok ? df : RESIDENT_NAN;
    valid[at] = ok ? 1 : 0;
}

struct ResidentArgs {
    int H, W;                        // the shape of every frame of the model (the host has checked that they share it)
    double sv;                       // sv of include/umpa_sigma.h (unmasked dark-field only)
    int start0, step0, N0, start1, step1, N1;
    const int* shift;                // [2][N0][N1]
    double* moments;                 // [P][N0][N1] or NULL
    double* unit;                    // [3][N0][N1]
    double* s2;
    double* dof;
    int* valid;
};

// MAPPING.  libumpa_sigma.so's (umpa_sigma.hip): a workgroup of 32 x 8 lanes takes 32 x 8 adjacent pixels of the region, one
// lane per pixel; a lane marches its window rows with r(dj - 1), r(dj), r(dj + 1) in a register ring, so a tap costs one
// load of the reference's centre row, one each of the rows above and below and one of the sample -- and, masked, one of the
// mask at the reference tap and one at the sample tap.  Lanes adjacent in x read adjacent addresses up to their shift
// difference; the patch of a workgroup stays in the L1 / L2 while its lanes sweep it.  The sums that are plain sums over
// the frames run on across the frames; the per-frame sums restart with each frame and fold into the product planes at its
// end: the register count does not grow with K.  The frame pointers come from the model's descriptor table through the
// constant address space (load_frame: scalar loads, k is wave-uniform).
// BOUNDS.  The host has checked that every frame is H x W at position (0, 0), that pad = Nw + ms is the model's padding,
// and start + step (N - 1) + 2 pad < H (resp. W); the guard below holds |si|, |sj| <= ms - 1, so the reference rows
// ci + si - Nw - 1 .. ci + si + Nw + 1 lie in 0 .. H - 1 (columns likewise), the sample rows ci - Nw .. ci + Nw too, and a
// mask is read at reference and sample taps only.
template <int KIND, bool MASKED>
__global__ void __launch_bounds__(RESIDENT_TILE_X * RESIDENT_TILE_Y)
resident_moments_kernel(const ModelDev dev, const ResidentArgs a)
{
#pragma clang fp contract(off)
    constexpr int P = ResidentPlanes<KIND, MASKED>::P;
    const int xj = blockIdx.x * RESIDENT_TILE_X + threadIdx.x, xi = blockIdx.y * RESIDENT_TILE_Y + threadIdx.y;
    if (xi >= a.N0 || xj >= a.N1) return;
    const int ms = dev.ms, Nw = dev.Nw, K = dev.Na, W = a.W;
    const size_t plane = (size_t)a.N0 * a.N1, at = (size_t)xi * a.N1 + xj;
    const int si = a.shift[at], sj = a.shift[plane + at];
    if (si < -(ms - 1) || si > ms - 1 || sj < -(ms - 1) || sj > ms - 1) {           // before any address is formed
        if (a.moments)
            for (int p = 0; p < P; p++) a.moments[p * plane + at] = RESIDENT_NAN;
        a.unit[at] = RESIDENT_NAN; a.unit[plane + at] = RESIDENT_NAN; a.unit[2 * plane + at] = RESIDENT_NAN;
        a.s2[at] = RESIDENT_NAN; a.dof[at] = RESIDENT_NAN; a.valid[at] = 0;
        return;
    }
    const int pad = Nw + ms, side = 2 * Nw + 1;
    const int ci = a.start0 + a.step0 * xi + pad, cj = a.start1 + a.step1 * xj + pad;
    const size_t offA = (size_t)(ci - Nw) * W + (cj - Nw), offR = (size_t)(ci + si - Nw) * W + (cj + sj - Nw);
    const double* __restrict__ win = dev.win;

    double m[P];
#pragma unroll
    for (int p = 0; p < P; p++) m[p] = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; k++) {
        const FrameDesc fr = load_frame(dev.frames, k);
        const double* __restrict__ A = fr.sam + offA;
        const double* __restrict__ R = fr.ref + offR;
        const double* __restrict__ MA = MASKED ? fr.mask + offA : nullptr;         // the mask at the sample taps
        const double* __restrict__ MR = MASKED ? fr.mask + offR : nullptr;         // and at the reference taps
        double f0 = 0.0, f1 = 0.0, f2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0, fa = 0.0;   // m_p, n_p, m_a of this frame
        double om = 0.0, nu = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;                   // masked: omega, nu, sum_x win u_p
#pragma unroll 1
        for (int di = 0; di < side; di++) {
            const double* __restrict__ rc = R + (size_t)di * W;
            const double* __restrict__ ar = A + (size_t)di * W;
            const double* __restrict__ wr = win + di * side;
            double rm = rc[-1], r = rc[0];
#pragma unroll 3
            for (int dj = 0; dj < side; dj++) {
                const double rp = rc[dj + 1];
                const double gi = 0.5 * (rc[dj + W] - rc[dj - W]), gj = 0.5 * (rp - rm);
                const double av = ar[dj], w0 = wr[dj];
                double w;
                if constexpr (MASKED) {
                    const double p = MR[(size_t)di * W + dj], q = MA[(size_t)di * W + dj];
                    const double c = (p * q) / ((p + q) + 1e-8);
                    w = c * w0;
                } else w = w0;
                const double v = w * w;
                const double wi = w * gi, wj = w * gj, w2 = w * r, vi = v * gi, vj = v * gj, v2 = v * r, wa = w * av;
                m[RS_S00] = fma(wi, gi, m[RS_S00]); m[RS_S01] = fma(wi, gj, m[RS_S01]); m[RS_S02] = fma(wi, r, m[RS_S02]);
                m[RS_S11] = fma(wj, gj, m[RS_S11]); m[RS_S12] = fma(wj, r, m[RS_S12]); m[RS_S22] = fma(w2, r, m[RS_S22]);
                m[RS_V00] = fma(vi, gi, m[RS_V00]); m[RS_V01] = fma(vi, gj, m[RS_V01]); m[RS_V02] = fma(vi, r, m[RS_V02]);
                m[RS_V11] = fma(vj, gj, m[RS_V11]); m[RS_V12] = fma(vj, r, m[RS_V12]); m[RS_V22] = fma(v2, r, m[RS_V22]);
                m[RS_P0] = fma(wa, gi, m[RS_P0]); m[RS_P1] = fma(wa, gj, m[RS_P1]); m[RS_P2] = fma(wa, r, m[RS_P2]);
                m[RS_QQ] = fma(wa, av, m[RS_QQ]);
                if constexpr (MASKED) om += w;
                if constexpr (KIND == 1) {
                    f0 += wi; f1 += wj; f2 += w2; n0 += vi; n1 += vj; n2 += v2; fa += wa;
                    if constexpr (MASKED) {
                        nu += v;
                        g0 = fma(w0, gi, g0); g1 = fma(w0, gj, g1); g2 = fma(w0, r, g2);
                    }
                }
                rm = r; r = rp;
            }
        }
        if constexpr (MASKED) m[RS_WW] = m[RS_WW] + om;
        if constexpr (KIND == 1 && !MASKED) {
            m[RS_MM00] = fma(f0, f0, m[RS_MM00]); m[RS_MM01] = fma(f0, f1, m[RS_MM01]); m[RS_MM02] = fma(f0, f2, m[RS_MM02]);
            m[RS_MM11] = fma(f1, f1, m[RS_MM11]); m[RS_MM12] = fma(f1, f2, m[RS_MM12]); m[RS_MM22] = fma(f2, f2, m[RS_MM22]);
            m[RS_NM00] = fma(n0, f0, m[RS_NM00]); m[RS_NM01] = fma(n0, f1, m[RS_NM01]); m[RS_NM02] = fma(n0, f2, m[RS_NM02]);
            m[RS_NM10] = fma(n1, f0, m[RS_NM10]); m[RS_NM11] = fma(n1, f1, m[RS_NM11]); m[RS_NM12] = fma(n1, f2, m[RS_NM12]);
            m[RS_NM20] = fma(n2, f0, m[RS_NM20]); m[RS_NM21] = fma(n2, f1, m[RS_NM21]); m[RS_NM22] = fma(n2, f2, m[RS_NM22]);
            m[RS_AM0] = fma(fa, f0, m[RS_AM0]); m[RS_AM1] = fma(fa, f1, m[RS_AM1]); m[RS_AM2] = fma(fa, f2, m[RS_AM2]);
        }
        if constexpr (KIND == 1 && MASKED) {
            const double u0 = g0 / dev.win_sum, u1 = g1 / dev.win_sum, u2 = g2 / dev.win_sum;   // mu_p: the UNMASKED windowed means
            const double o0 = om * u0, o1 = om * u1, o2 = om * u2, q0 = nu * u0, q1 = nu * u1, q2 = nu * u2;
            m[RS_MU00] = fma(f0, u0, m[RS_MU00]); m[RS_MU01] = fma(f0, u1, m[RS_MU01]); m[RS_MU02] = fma(f0, u2, m[RS_MU02]);
            m[RS_MU10] = fma(f1, u0, m[RS_MU10]); m[RS_MU11] = fma(f1, u1, m[RS_MU11]); m[RS_MU12] = fma(f1, u2, m[RS_MU12]);
            m[RS_MU20] = fma(f2, u0, m[RS_MU20]); m[RS_MU21] = fma(f2, u1, m[RS_MU21]); m[RS_MU22] = fma(f2, u2, m[RS_MU22]);
            m[RS_WM00] = fma(o0, u0, m[RS_WM00]); m[RS_WM01] = fma(o0, u1, m[RS_WM01]); m[RS_WM02] = fma(o0, u2, m[RS_WM02]);
            m[RS_WM11] = fma(o1, u1, m[RS_WM11]); m[RS_WM12] = fma(o1, u2, m[RS_WM12]); m[RS_WM22] = fma(o2, u2, m[RS_WM22]);
            m[RS_NU00] = fma(n0, u0, m[RS_NU00]); m[RS_NU01] = fma(n0, u1, m[RS_NU01]); m[RS_NU02] = fma(n0, u2, m[RS_NU02]);
            m[RS_NU10] = fma(n1, u0, m[RS_NU10]); m[RS_NU11] = fma(n1, u1, m[RS_NU11]); m[RS_NU12] = fma(n1, u2, m[RS_NU12]);
            m[RS_NU20] = fma(n2, u0, m[RS_NU20]); m[RS_NU21] = fma(n2, u1, m[RS_NU21]); m[RS_NU22] = fma(n2, u2, m[RS_NU22]);
            m[RS_VM00] = fma(q0, u0, m[RS_VM00]); m[RS_VM01] = fma(q0, u1, m[RS_VM01]); m[RS_VM02] = fma(q0, u2, m[RS_VM02]);
            m[RS_VM11] = fma(q1, u1, m[RS_VM11]); m[RS_VM12] = fma(q1, u2, m[RS_VM12]); m[RS_VM22] = fma(q2, u2, m[RS_VM22]);
            m[RS_AU0] = fma(fa, u0, m[RS_AU0]); m[RS_AU1] = fma(fa, u1, m[RS_AU1]); m[RS_AU2] = fma(fa, u2, m[RS_AU2]);
        }
    }
    if (a.moments) {
#pragma unroll
        for (int p = 0; p < P; p++) a.moments[p * plane + at] = m[p];
    }
    resident_solve<KIND, MASKED>(m, a.sv, K, at, plane, a.unit, a.s2, a.dof, a.valid);
}

} // namespace umpa
