// umpa_sigma.hip -- libumpa_sigma.so: the per-pixel covariance of a matched shift and the noise estimate from the residual
// (include/umpa_sigma.h, where the operation is defined).  gfx950 only.
//
// An eighth library beside libumpa_hip.so and its six satellites, for the reason those have their own (DESIGN.md section
// 4.9): the other libraries' kernel sets stay what they are.  It includes no kernel header and never sees a model.
// Two kernel families:
//   sigma_moments_kernel<KIND>  one lane per pixel: the windowed moments over all frames, then the solve on them
//   sigma_solve_kernel<KIND>    the solve alone on moments the caller supplies
// Both end in the same device function.  Built with -ffp-contract=off: the solve is + - * / in the header's order and
// nothing else; the sums say fma() where they mean one.  No atomics, one writer per output.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/umpa_sigma.h"
#include "umpa_host.h"

namespace umpa {

#define SIGMA_INF (__builtin_huge_val())
#define SIGMA_NAN (__builtin_nan(""))
constexpr int TILE_X = 32, TILE_Y = 8;             // pixels of one workgroup of the moments kernel: 32 columns x 8 rows

template <int KIND> struct Planes { static constexpr int P = KIND ? UMPA_SIGMA_PLANES_DF : UMPA_SIGMA_PLANES_PLAIN, N = KIND ? 4 : 3; };

// The plane indices of the header
enum { S00, S01, S02, S11, S12, S22, V00, V01, V02, V11, V12, V22, P0, P1, P2, QQ,
       MM00, MM01, MM02, MM11, MM12, MM22, NM00, NM01, NM02, NM10, NM11, NM12, NM20, NM21, NM22, AM0, AM1, AM2 };

__device__ __forceinline__ bool finite(double x) { return x > -SIGMA_INF && x < SIGMA_INF; }

// x = A^-1 b by the factors L, D of the header's SOLVE
template <int N>
__device__ __forceinline__ void ldl_solve(const double (&L)[N][N], const double (&D)[N], const double (&b)[N], double (&x)[N])
{
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

// MODEL and SOLVE of include/umpa_sigma.h on the moments m[] of one pixel: writes unit (three planes `plane` apart), s2,
// dof and valid at `at`.
template <int KIND>
__device__ __forceinline__ void sigma_solve(const double (&m)[Planes<KIND>::P], const double sv, const int K, const size_t at, const size_t plane,
                                            double* __restrict__ unit, double* __restrict__ s2, double* __restrict__ dof, int* __restrict__ valid)
{
    constexpr int N = Planes<KIND>::N;
    double A[N][N], B[N][N], h[N], rss0;
    if constexpr (KIND == 0) {
        const double T = m[P2] / m[S22], TT = T * T;
        A[0][0] = TT * m[S00]; A[1][0] = TT * m[S01]; A[1][1] = TT * m[S11];
        A[2][0] = T * m[S02]; A[2][1] = T * m[S12]; A[2][2] = m[S22];
        B[0][0] = TT * m[V00]; B[1][0] = TT * m[V01]; B[1][1] = TT * m[V11];
        B[2][0] = T * m[V02]; B[2][1] = T * m[V12]; B[2][2] = m[V22];
        h[0] = T * (m[P0] - T * m[S02]);
        h[1] = T * (m[P1] - T * m[S12]);
        h[2] = m[P2] - T * m[S22];
        rss0 = m[QQ] - m[P2] * T;
    } else {
        const double t1 = m[QQ], t2 = m[MM22], t3 = m[S22], t4 = m[AM2], t5 = m[P2], t6 = m[MM22];
        const double det = t2 * t3 - t6 * t6;
        const double Kc = (t2 * t5 - t4 * t6) / det;
        const double beta = (t3 * t4 - t5 * t6) / det;
        const double KK = Kc * Kc, c = (2 * Kc) * beta + beta * beta, bb = (beta * beta) * sv, kb = Kc * beta, bs = beta * sv;
        A[0][0] = KK * m[S00] + c * m[MM00]; A[1][0] = KK * m[S01] + c * m[MM01]; A[1][1] = KK * m[S11] + c * m[MM11];
        A[2][0] = (Kc + beta) * m[MM02]; A[2][1] = (Kc + beta) * m[MM12];
        A[3][0] = Kc * m[S02] + beta * m[MM02]; A[3][1] = Kc * m[S12] + beta * m[MM12];
        A[2][2] = m[MM22]; A[3][2] = m[MM22]; A[3][3] = m[S22];
        B[0][0] = (KK * m[V00] + kb * (m[NM00] + m[NM00])) + bb * m[MM00];
        B[1][0] = (KK * m[V01] + kb * (m[NM01] + m[NM10])) + bb * m[MM01];
        B[1][1] = (KK * m[V11] + kb * (m[NM11] + m[NM11])) + bb * m[MM11];
        B[2][0] = Kc * m[NM02] + bs * m[MM02]; B[2][1] = Kc * m[NM12] + bs * m[MM12];
        B[3][0] = Kc * m[V02] + beta * m[NM20]; B[3][1] = Kc * m[V12] + beta * m[NM21];
        B[2][2] = sv * m[MM22]; B[3][2] = m[NM22]; B[3][3] = m[V22];
        h[0] = Kc * ((m[P0] - beta * m[MM02]) - Kc * m[S02]) + beta * ((m[AM0] - beta * m[MM02]) - Kc * m[MM02]);
        h[1] = Kc * ((m[P1] - beta * m[MM12]) - Kc * m[S12]) + beta * ((m[AM1] - beta * m[MM12]) - Kc * m[MM12]);
        h[2] = (m[AM2] - beta * m[MM22]) - Kc * m[MM22];
        h[3] = (m[P2] - beta * m[MM22]) - Kc * m[S22];
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
        ok = ok && D[j] > 0.0 && D[j] < SIGMA_INF;
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
        ldl_solve<N>(L, D, b, X[q]);
        tr = q == 0 ? X[0][0] : tr + X[q][q];
    }
    double r0[N], r1[N], Y0[N], Y1[N], d[N];
#pragma unroll
    for (int q = 0; q < N; q++) { r0[q] = X[q][0]; r1[q] = X[q][1]; }
    ldl_solve<N>(L, D, r0, Y0);
    ldl_solve<N>(L, D, r1, Y1);
    ldl_solve<N>(L, D, h, d);
    double hd = h[0] * d[0] + h[1] * d[1];
#pragma unroll
    for (int i = 2; i < N; i++) hd = hd + h[i] * d[i];
    const double rr = rss0 - hd;
    const double df = (double)K - tr;
    const double rss = rr > 0.0 ? rr : 0.0;
    const double s = rss / df;
    ok = ok && df > 0.0 && finite(Y0[0]) && finite(Y1[1]) && finite(Y1[0]) && finite(rr) && finite(df) && finite(s);
    unit[at] = ok ? Y0[0] : SIGMA_NAN;
    unit[plane + at] = ok ? Y1[1] : SIGMA_NAN;
    unit[2 * plane + at] = ok ? Y1[0] : SIGMA_NAN;
    s2[at] = ok ? s : SIGMA_NAN;
    dof[at] = ok ? df : SIGMA_NAN;
    valid[at] = ok ? 1 : 0;
}

// MAPPING.  A workgroup of 32 x 8 lanes takes 32 x 8 adjacent pixels of the region, one lane per pixel; the work is K (2 Nw + 1)^2
// taps of 16 (plain) or 23 (dark-field) fp64 accumulations at a position that differs per pixel by its shift, so it does not
// separate across pixels.  A lane marches its window rows: along a row r(dj - 1), r(dj), r(dj + 1) live in a register ring,
// so a tap costs one load of the centre row, one each of the rows above and below, and one of the sample; lanes adjacent
// in x read adjacent (step 1) addresses up to their shift difference, and the patch of a workgroup -- (8 step + 2 pad) x
// (32 step + 2 pad) doubles per frame and stack at most, 11.6 KB at C2's shape -- stays in the L1 / L2 while its lanes sweep it.
// The 16 sums that are plain sums over frames run on across the frames; only the 7 per-frame sums of the dark-field model
// restart with each frame and fold into MM, NM, AM at its end: the register count does not grow with K.
// BOUNDS.  The host has checked start + step (N - 1) + 2 pad < H (resp. W) and pad = Nw + ms; the guard below holds
// |si|, |sj| <= ms - 1, so the reference rows ci + si - Nw - 1 .. ci + si + Nw + 1 lie in 0 .. H - 1 (columns likewise).
template <int KIND>
__global__ void __launch_bounds__(TILE_X * TILE_Y)
sigma_moments_kernel(const double* __restrict__ sam, const double* __restrict__ ref, const int K, const int H, const int W,
                     const double* __restrict__ win, const int Nw, const int ms, const double sv,
                     const int start0, const int step0, const int N0, const int start1, const int step1, const int N1,
                     const int* __restrict__ shift, double* __restrict__ moments,
                     double* __restrict__ unit, double* __restrict__ s2, double* __restrict__ dof, int* __restrict__ valid)
{
    constexpr int P = Planes<KIND>::P;
    const int xj = blockIdx.x * TILE_X + threadIdx.x, xi = blockIdx.y * TILE_Y + threadIdx.y;
    if (xi >= N0 || xj >= N1) return;
    const size_t plane = (size_t)N0 * N1, at = (size_t)xi * N1 + xj;
    const int si = shift[at], sj = shift[plane + at];
    if (si < -(ms - 1) || si > ms - 1 || sj < -(ms - 1) || sj > ms - 1) {           // before any address is formed
        if (moments)
            for (int p = 0; p < P; p++) moments[p * plane + at] = SIGMA_NAN;
        unit[at] = SIGMA_NAN; unit[plane + at] = SIGMA_NAN; unit[2 * plane + at] = SIGMA_NAN;
        s2[at] = SIGMA_NAN; dof[at] = SIGMA_NAN; valid[at] = 0;
        return;
    }
    const int pad = Nw + ms, side = 2 * Nw + 1;
    const int ci = start0 + step0 * xi + pad, cj = start1 + step1 * xj + pad;
    const size_t frame = (size_t)H * W;

    double m[P];
#pragma unroll
    for (int p = 0; p < P; p++) m[p] = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; k++) {
        const double* __restrict__ A = sam + k * frame + (size_t)(ci - Nw) * W + (cj - Nw);
        const double* __restrict__ R = ref + k * frame + (size_t)(ci + si - Nw) * W + (cj + sj - Nw);
        double f0 = 0.0, f1 = 0.0, f2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0, fa = 0.0;   // m_p, n_p, m_a of this frame
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
                const double a = ar[dj], w = wr[dj], v = w * w;
                const double wi = w * gi, wj = w * gj, w2 = w * r, vi = v * gi, vj = v * gj, v2 = v * r, wa = w * a;
                m[S00] = fma(wi, gi, m[S00]); m[S01] = fma(wi, gj, m[S01]); m[S02] = fma(wi, r, m[S02]);
                m[S11] = fma(wj, gj, m[S11]); m[S12] = fma(wj, r, m[S12]); m[S22] = fma(w2, r, m[S22]);
                m[V00] = fma(vi, gi, m[V00]); m[V01] = fma(vi, gj, m[V01]); m[V02] = fma(vi, r, m[V02]);
                m[V11] = fma(vj, gj, m[V11]); m[V12] = fma(vj, r, m[V12]); m[V22] = fma(v2, r, m[V22]);
                m[P0] = fma(wa, gi, m[P0]); m[P1] = fma(wa, gj, m[P1]); m[P2] = fma(wa, r, m[P2]);
                m[QQ] = fma(wa, a, m[QQ]);
                if constexpr (KIND == 1) {
                    f0 += wi; f1 += wj; f2 += w2; n0 += vi; n1 += vj; n2 += v2; fa += wa;
                }
                rm = r; r = rp;
            }
        }
        if constexpr (KIND == 1) {
            m[MM00] = fma(f0, f0, m[MM00]); m[MM01] = fma(f0, f1, m[MM01]); m[MM02] = fma(f0, f2, m[MM02]);
            m[MM11] = fma(f1, f1, m[MM11]); m[MM12] = fma(f1, f2, m[MM12]); m[MM22] = fma(f2, f2, m[MM22]);
            m[NM00] = fma(n0, f0, m[NM00]); m[NM01] = fma(n0, f1, m[NM01]); m[NM02] = fma(n0, f2, m[NM02]);
            m[NM10] = fma(n1, f0, m[NM10]); m[NM11] = fma(n1, f1, m[NM11]); m[NM12] = fma(n1, f2, m[NM12]);
            m[NM20] = fma(n2, f0, m[NM20]); m[NM21] = fma(n2, f1, m[NM21]); m[NM22] = fma(n2, f2, m[NM22]);
            m[AM0] = fma(fa, f0, m[AM0]); m[AM1] = fma(fa, f1, m[AM1]); m[AM2] = fma(fa, f2, m[AM2]);
        }
    }
    if (moments) {
#pragma unroll
        for (int p = 0; p < P; p++) moments[p * plane + at] = m[p];
    }
    sigma_solve<KIND>(m, sv, K, at, plane, unit, s2, dof, valid);
}

template <int KIND>
__global__ void __launch_bounds__(256)
sigma_solve_kernel(const double* __restrict__ moments, const double sv, const int K, const size_t n,
                   double* __restrict__ unit, double* __restrict__ s2, double* __restrict__ dof, int* __restrict__ valid)
{
    constexpr int P = Planes<KIND>::P;
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    double m[P];
#pragma unroll
    for (int p = 0; p < P; p++) m[p] = moments[p * n + at];
    sigma_solve<KIND>(m, sv, K, at, n, unit, s2, dof, valid);
}

} // namespace umpa

using namespace umpa;

#define UMPA_SIGMA_API extern "C" __attribute__((visibility("default")))

namespace {

// sv of the header: the squares of the window summed in tap order, as two roundings per tap
double window_sv(const double* win, int Nw)
{
    const int T = (2 * Nw + 1) * (2 * Nw + 1);
    volatile double sv = 0.0;                       // (volatile: no contraction of w * w + sv, whatever the host flags)
    for (int x = 0; x < T; x++) { volatile double v = win[x] * win[x]; sv = sv + v; }
    return sv;
}

int check_io(int kind, int K, int flags)
{
    if (kind != 0 && kind != 1) return fail(UMPA_HIP_E_ARG, "sigma: kind = %d (0 plain, 1 dark-field)", kind);
    if (K < 1) return fail(UMPA_HIP_E_ARG, "sigma: K = %d frames", K);
    if (flags & ~UMPA_HIP_F_DEVICE_IO) return fail(UMPA_HIP_E_ARG, "sigma: the call takes UMPA_HIP_F_DEVICE_IO and no other flag");
    return 0;
}

int check_axis(const char* name, int start, int step, int N, int extent)
{
    if (N < 1 || step < 1 || start < 0 || (long long)start + (long long)step * (N - 1) > (long long)extent - 1)
        return fail(UMPA_HIP_E_ARG, "sigma: region axis %s: start %d, step %d, %d pixels exceed the extent %d", name, start, step, N, extent);
    return 0;
}

void launch_solve(int kind, const double* moments, double sv, int K, size_t n, double* unit, double* s2, double* dof, int* valid, hipStream_t s)
{
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (kind) hipLaunchKernelGGL(sigma_solve_kernel<1>, grid, block, 0, s, moments, sv, K, n, unit, s2, dof, valid);
    else hipLaunchKernelGGL(sigma_solve_kernel<0>, grid, block, 0, s, moments, sv, K, n, unit, s2, dof, valid);
}

} // namespace

UMPA_SIGMA_API const char* umpa_sigma_last_error(void) { return g_err.c_str(); }

UMPA_SIGMA_API int umpa_sigma_region(const double* sam, const double* ref, int K, int H, int W, const double* win, int Nw, int max_shift,
                                     int kind, int start0, int step0, int N0, int start1, int step1, int N1, const int* shift,
                                     double* moments, double* unit, double* s2, double* dof, int* valid,
                                     int device, int flags, void* stream)
{
    if (!sam || !ref || !win || !shift || !unit || !s2 || !dof || !valid)
        return fail(UMPA_HIP_E_ARG, "sigma: null argument (sam, ref, win, shift, unit, s2, dof and valid are required)");
    if (int rc = check_io(kind, K, flags)) return rc;
    if (Nw < 1 || Nw > UMPA_SIGMA_MAX_NW) return fail(UMPA_HIP_E_ARG, "sigma: Nw = %d (1 to %d)", Nw, UMPA_SIGMA_MAX_NW);
    if (max_shift < 1 || max_shift > (1 << 20)) return fail(UMPA_HIP_E_ARG, "sigma: max_shift = %d", max_shift);
    const int pad = Nw + max_shift, side = 2 * Nw + 1;
    if (H < 2 * pad + 1 || W < 2 * pad + 1 || (long long)H * W > (1LL << 40))
        return fail(UMPA_HIP_E_ARG, "sigma: frames of %d x %d pixels (at least %d x %d for Nw = %d, max_shift = %d)", H, W, 2 * pad + 1, 2 * pad + 1, Nw, max_shift);
    double sw = 0.0;
    for (int x = 0; x < side * side; x++) {
        if (!(win[x] >= 0.0) || !std::isfinite(win[x])) return fail(UMPA_HIP_E_ARG, "sigma: window entry %d is %g (finite and >= 0)", x, win[x]);
        sw += win[x];
    }
    if (!(std::fabs(sw - 1.0) <= 1e-9)) return fail(UMPA_HIP_E_ARG, "sigma: the window sums to %.17g (it must be normalised)", sw);
    if (int rc = check_axis("0", start0, step0, N0, H - 2 * pad)) return rc;
    if (int rc = check_axis("1", start1, step1, N1, W - 2 * pad)) return rc;
    if (int rc = pick_device("sigma", device)) return rc;

    const bool dio = (flags & UMPA_HIP_F_DEVICE_IO) != 0;
    const size_t n = (size_t)N0 * N1, stack = (size_t)K * H * W * sizeof(double), wbytes = (size_t)side * side * sizeof(double);
    const int P = kind ? UMPA_SIGMA_PLANES_DF : UMPA_SIGMA_PLANES_PLAIN;
    const double sv = window_sv(win, Nw);
    hipStream_t s = dio ? (hipStream_t)stream : nullptr;

    // slots: 0 the window; host arrays: 1 sam, 2 ref, 3 shift, 4 moments, 5 unit, 6 s2, 7 dof, 8 valid
    DeviceMem S;
    HIPOK(S.alloc(0, wbytes), UMPA_HIP_E_NOMEM, "sigma: device memory for the window");
    HIPOK(hipMemcpyAsync(S.p[0], win, wbytes, hipMemcpyHostToDevice, s), UMPA_HIP_E_DEVICE, "sigma: upload of the window");
    const size_t bytes[5] = {moments ? P * n * 8 : 0, 3 * n * 8, n * 8, n * 8, n * 4};
    void* host[5] = {moments, unit, s2, dof, valid};
    void* dev[5] = {moments, unit, s2, dof, valid};
    const double *dsam = sam, *dref = ref;
    const int* dshift = shift;
    if (!dio) {
        HIPOK(S.alloc(1, stack), UMPA_HIP_E_NOMEM, "sigma: device memory for the sample stack");
        HIPOK(S.alloc(2, stack), UMPA_HIP_E_NOMEM, "sigma: device memory for the reference stack");
        HIPOK(S.alloc(3, 2 * n * 4), UMPA_HIP_E_NOMEM, "sigma: device memory for the shift field");
        for (int q = 0; q < 5; q++)
            if (host[q]) {
                HIPOK(S.alloc(4 + q, bytes[q]), UMPA_HIP_E_NOMEM, "sigma: device memory for the results");
                dev[q] = S.p[4 + q];
            }
        HIPOK(hipMemcpy(S.p[1], sam, stack, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "sigma: upload of the sample stack");
        HIPOK(hipMemcpy(S.p[2], ref, stack, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "sigma: upload of the reference stack");
        HIPOK(hipMemcpy(S.p[3], shift, 2 * n * 4, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "sigma: upload of the shift field");
        dsam = (const double*)S.p[1]; dref = (const double*)S.p[2]; dshift = (const int*)S.p[3];
    }
    const dim3 grid((N1 + TILE_X - 1) / TILE_X, (N0 + TILE_Y - 1) / TILE_Y), block(TILE_X, TILE_Y);
    if (kind)
        hipLaunchKernelGGL(sigma_moments_kernel<1>, grid, block, 0, s, dsam, dref, K, H, W, (const double*)S.p[0], Nw, max_shift, sv,
                           start0, step0, N0, start1, step1, N1, dshift, (double*)dev[0], (double*)dev[1], (double*)dev[2], (double*)dev[3], (int*)dev[4]);
    else
        hipLaunchKernelGGL(sigma_moments_kernel<0>, grid, block, 0, s, dsam, dref, K, H, W, (const double*)S.p[0], Nw, max_shift, sv,
                           start0, step0, N0, start1, step1, N1, dshift, (double*)dev[0], (double*)dev[1], (double*)dev[2], (double*)dev[3], (int*)dev[4]);
    LAUNCHED("sigma: launch of the moments kernel");
    if (dio) {
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "sigma: region");
        return 0;
    }
    for (int q = 0; q < 5; q++)
        if (host[q]) HIPOK(hipMemcpy(host[q], dev[q], bytes[q], hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "sigma: region");
    return 0;
}

UMPA_SIGMA_API int umpa_sigma_solve(const double* moments, int kind, int K, long long n, double sv,
                                    double* unit, double* s2, double* dof, int* valid, int device, int flags, void* stream)
{
    if (!moments || !unit || !s2 || !dof || !valid) return fail(UMPA_HIP_E_ARG, "sigma: null argument (moments, unit, s2, dof and valid are required)");
    if (int rc = check_io(kind, K, flags)) return rc;
    if (n < 1 || n > (1LL << 40)) return fail(UMPA_HIP_E_ARG, "sigma: n = %lld pixels", n);
    if (!(sv >= 0.0) || !std::isfinite(sv)) return fail(UMPA_HIP_E_ARG, "sigma: sv = %g (finite and >= 0)", sv);
    if (int rc = pick_device("sigma", device)) return rc;
    const size_t N = (size_t)n, P = kind ? UMPA_SIGMA_PLANES_DF : UMPA_SIGMA_PLANES_PLAIN;
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        hipStream_t s = (hipStream_t)stream;
        launch_solve(kind, moments, sv, K, N, unit, s2, dof, valid, s);
        LAUNCHED("sigma: launch of the solve kernel");
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "sigma: solve");
        return 0;
    }
    DeviceMem S;                                    // slots: 0 moments, 1 unit, 2 s2, 3 dof, 4 valid
    const size_t bytes[5] = {P * N * 8, 3 * N * 8, N * 8, N * 8, N * 4};
    void* host[5] = {nullptr, unit, s2, dof, valid};
    for (int q = 0; q < 5; q++) HIPOK(S.alloc(q, bytes[q]), UMPA_HIP_E_NOMEM, "sigma: device memory for the solve");
    HIPOK(hipMemcpy(S.p[0], moments, bytes[0], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "sigma: upload of the moments");
    launch_solve(kind, (const double*)S.p[0], sv, K, N, (double*)S.p[1], (double*)S.p[2], (double*)S.p[3], (int*)S.p[4], nullptr);
    LAUNCHED("sigma: launch of the solve kernel");
    for (int q = 1; q < 5; q++) HIPOK(hipMemcpy(host[q], S.p[q], bytes[q], hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "sigma: solve");
    return 0;
}
