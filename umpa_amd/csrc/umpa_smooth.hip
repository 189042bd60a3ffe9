// umpa_smooth.hip -- libumpa_smooth.so: path aggregation over a cost volume and the per-pixel selection
// (include/umpa_smooth.h, where the operation is defined).  gfx950 only.
//
// A seventh library beside libumpa_hip.so and its five satellites, for the reason those have their own (DESIGN.md section
// 4.9): the other libraries' kernel sets stay what they are.  It includes no kernel header and never sees a model.
// Three kernel families:
//   smooth_path_kernel<U, TW, FIRST>  one pass: L_r of one direction, marched down (or up) the rows, into an accumulator
//   smooth_transpose_kernel<ADD>      [l][R][C] -> [l][C][R] through LDS tiles; ADD: added to what the target holds
//   smooth_select_kernel<U>           l*, shift, smin, margin, valid of every pixel
// The horizontal directions 0 and 1 run through the same marching kernel on a transposed copy of the volume.  No atomics,
// no multiplication, one writer per (label, pixel) and pass.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/umpa_smooth.h"
#include "umpa_host.h"

namespace umpa {

// Columns of one workgroup of the marching kernel.  Measured on an MI355X, one accumulating pass: 2028 columns, U = 9:
// 4.9 ms with 8 columns (254 workgroups), 6.1 ms with 16 (127: half the CUs idle); 4066 columns, U = 15: 52 ms with 8 (64-byte
// rows: each 128-byte line is fetched by two workgroups), 29 ms with 16.  The switch sits between the two measured widths.
constexpr int TW_NARROW = 8, TW_WIDE = 16, WIDE_FROM = 3072;
constexpr int TT = 32;                             // the transpose's tile
#define SMOOTH_INF (__builtin_huge_val())

__device__ __forceinline__ double dmin(double x, double y) { return x < y ? x : y; }
__device__ __forceinline__ double conditioned(double c) { return (c > -SMOOTH_INF && c < SMOOTH_INF) ? c : SMOOTH_INF; }

// MAPPING.  A workgroup of TW x U threads takes TW adjacent columns (TW = 8, or 16 from WIDE_FROM columns on); thread
// (x, a) holds the U labels (a, 0 .. U - 1) of the pixel its column is at: one a-row of the label array in registers.  Lanes
// adjacent in a wave are adjacent columns of one label plane (64 or 128 contiguous bytes per label and a-row), never U * U
// doubles per lane and never a [label][lane] block of LDS per wave.  All threads march together over the N0 rows,
// down (dr = +1) or up (dr = -1); the column of a thread moves by dc per step and wraps modulo N1, and a wrap is a path
// start, so the diagonals keep every lane busy and their loads as coalesced as the verticals'.
// A STEP.  The b sweeps run in the registers of the a-row's owner.  The a sweeps need the label array's columns: the
// swept rows go to LDS (X[a][b][x]), and after a barrier thread (x, a) takes COLUMN b = a, sweeps it and writes it back,
// while it also folds the row minima of L_r(q, .) (m) and of C'(p, .) (is p void) that every thread left in M and V.
// After a second barrier each thread reads its own row back.  Two barriers per step suffice: between them only columns
// are touched (disjoint among the threads), outside them each thread touches only its own row and its own M, V slot, and
// a thread that writes them for step t + 1 has passed the second barrier of step t, behind which nobody reads them.
// PREFETCH.  C' of step t + 1 and the accumulator's values of step t are requested before step t's chain of dependent
// min / add starts; the chain itself touches no global memory.
// Threads whose column is beyond N1 load and store nothing but take part in the barriers.
template <int U, int TW, bool FIRST>
__global__ void __launch_bounds__(TW * U)
smooth_path_kernel(const double* __restrict__ cost, double* __restrict__ acc, const int N0, const int N1,
                   const int dr, const int dc, const double lam, const double trunc)
{
    __shared__ double X[U * U * TW];
    __shared__ double M[U * TW];
    __shared__ double V[U * TW];
    const int x = threadIdx.x, a = threadIdx.y;
    const size_t plane = (size_t)N0 * N1;
    const int j0 = blockIdx.x * TW + x;
    const bool live = j0 < N1;
    const double* __restrict__ crow = cost + (size_t)a * U * plane;
    double* __restrict__ arow = acc + (size_t)a * U * plane;

    int i = dr > 0 ? 0 : N0 - 1, j = live ? j0 : 0;
    double L[U], c[U], cn[U], old[U], h[U];
#pragma unroll
    for (int b = 0; b < U; b++) { L[b] = 0.0; c[b] = SMOOTH_INF; cn[b] = SMOOTH_INF; old[b] = 0.0; }
    if (live) {
        const size_t at = (size_t)i * N1 + j;
#pragma unroll
        for (int b = 0; b < U; b++) c[b] = conditioned(crow[b * plane + at]);
    }
    bool fresh = true;                             // the pixel of this step starts a path, or its predecessor is void

#pragma unroll 1
    for (int t = 0; t < N0; t++) {
        const size_t at = (size_t)i * N1 + j;
        const int in = i + dr;
        int jn = j + dc;
        bool wrap = false;
        if (jn >= N1) { jn = 0; wrap = true; }
        else if (jn < 0) { jn = N1 - 1; wrap = true; }
        if (live) {
            if (t + 1 < N0) {
                const size_t nx = (size_t)in * N1 + jn;
#pragma unroll
                for (int b = 0; b < U; b++) cn[b] = crow[b * plane + nx];
            }
            if (!FIRST) {
#pragma unroll
                for (int b = 0; b < U; b++) old[b] = arow[b * plane + at];
            }
        }

        double lm = L[0], cm = c[0];
#pragma unroll
        for (int b = 0; b < U; b++) { h[b] = L[b]; lm = dmin(lm, L[b]); cm = dmin(cm, c[b]); }
#pragma unroll
        for (int b = 1; b < U; b++) h[b] = dmin(h[b], h[b - 1] + lam);
#pragma unroll
        for (int b = U - 2; b >= 0; b--) h[b] = dmin(h[b], h[b + 1] + lam);
#pragma unroll
        for (int b = 0; b < U; b++) X[(a * U + b) * TW + x] = h[b];
        M[a * TW + x] = lm;
        V[a * TW + x] = cm;
        __syncthreads();

        {
            double g[U];
#pragma unroll
            for (int k = 0; k < U; k++) g[k] = X[(k * U + a) * TW + x];
#pragma unroll
            for (int k = 1; k < U; k++) g[k] = dmin(g[k], g[k - 1] + lam);
#pragma unroll
            for (int k = U - 2; k >= 0; k--) g[k] = dmin(g[k], g[k + 1] + lam);
#pragma unroll
            for (int k = 0; k < U; k++) X[(k * U + a) * TW + x] = g[k];
        }
        double m = M[x], pv = V[x];
#pragma unroll
        for (int k = 1; k < U; k++) { m = dmin(m, M[k * TW + x]); pv = dmin(pv, V[k * TW + x]); }
        __syncthreads();

        const bool pvoid = !(pv < SMOOTH_INF);
        const double mt = m + trunc;
#pragma unroll
        for (int b = 0; b < U; b++) {
            const double e = dmin(X[(a * U + b) * TW + x], mt) - m;
            const double v = fresh ? c[b] : c[b] + e;
            L[b] = pvoid ? 0.0 : v;
        }
        if (live) {
#pragma unroll
            for (int b = 0; b < U; b++) arow[b * plane + at] = FIRST ? L[b] : old[b] + L[b];
        }
        fresh = pvoid || wrap;
#pragma unroll
        for (int b = 0; b < U; b++) c[b] = conditioned(cn[b]);
        i = in; j = jn;
    }
}

// out[l][c][r] = in[l][r][c] (ADD: + what out[l][c][r] holds), one 32 x 32 tile of one label plane per workgroup of 32 x 8
// threads, through LDS with a pitch of 33 doubles: reads and writes of global memory both run along rows.
template <bool ADD>
__global__ void __launch_bounds__(TT * 8)
smooth_transpose_kernel(const double* __restrict__ in, double* __restrict__ out, const int R, const int C)
{
    __shared__ double tile[TT][TT + 1];
    const size_t base = (size_t)blockIdx.z * ((size_t)R * C);
    const int c0 = blockIdx.x * TT, r0 = blockIdx.y * TT;
    const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
    for (int k = 0; k < TT; k += 8) {
        const int r = r0 + ty + k, c = c0 + tx;
        if (r < R && c < C) tile[ty + k][tx] = in[base + (size_t)r * C + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TT; k += 8) {
        const int c = c0 + ty + k, r = r0 + tx;
        if (c < C && r < R) {
            const size_t at = base + (size_t)c * R + r;
            const double v = tile[tx][ty + k];
            out[at] = ADD ? v + out[at] : v;
        }
    }
}

// The selection of include/umpa_smooth.h, one lane per pixel; smin, margin and valid may be null.
template <int U>
__global__ void __launch_bounds__(256)
smooth_select_kernel(const double* __restrict__ cost, const double* __restrict__ total, const size_t plane,
                     int* __restrict__ shift, double* __restrict__ smin, double* __restrict__ margin, int* __restrict__ valid)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    bool any = false;
#pragma unroll 5
    for (int l = 0; l < U * U; l++) {
        const double c = cost[l * plane + p];
        any = any || (c > -SMOOTH_INF && c < SMOOTH_INF);
    }
    int si = 0, sj = 0, ok = 0;
    double best = 0.0, gap = 0.0;
    if (any) {
        int lb = 0;
        best = total[p];
#pragma unroll 5
        for (int l = 1; l < U * U; l++) {
            const double v = total[l * plane + p];
            if (v < best) { best = v; lb = l; }
        }
        const int as = lb / U, bs = lb - as * U;
        double far = SMOOTH_INF;
        for (int a = 0; a < U; a++)
            for (int b = 0; b < U; b++) {
                const int da = a > as ? a - as : as - a, db = b > bs ? b - bs : bs - b;
                if (da >= 2 || db >= 2) far = dmin(far, total[(size_t)(a * U + b) * plane + p]);
            }
        si = as - (U - 1) / 2; sj = bs - (U - 1) / 2; ok = 1;
        gap = far - best;
    }
    shift[p] = si;
    shift[plane + p] = sj;
    if (smin) smin[p] = best;
    if (margin) margin[p] = gap;
    if (valid) valid[p] = ok;
}

} // namespace umpa

using namespace umpa;

#define UMPA_SMOOTH_API extern "C" __attribute__((visibility("default")))

namespace {

// (row step, column step) of the eight directions
const int DIRS[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};

int check_shape(int U, int N0, int N1, int dirs)
{
    if (U < UMPA_SMOOTH_MIN_U || U > UMPA_SMOOTH_MAX_U || U % 2 == 0)
        return fail(UMPA_HIP_E_ARG, "smooth: U = %d (odd, %d to %d)", U, UMPA_SMOOTH_MIN_U, UMPA_SMOOTH_MAX_U);
    if (N0 < 1 || N1 < 1) return fail(UMPA_HIP_E_ARG, "smooth: a region of %d x %d pixels", N0, N1);
    if (dirs < 1 || dirs > UMPA_SMOOTH_ALL_DIRS) return fail(UMPA_HIP_E_ARG, "smooth: dirs = 0x%x (a mask of the directions 0 to 7, at least one)", dirs);
    return 0;
}

size_t volume_bytes(int U, int N0, int N1) { return (size_t)U * U * N0 * N1 * sizeof(double); }

template <int U>
void launch_path(bool first, const double* cost, double* acc, int N0, int N1, int dr, int dc, double lam, double trunc, hipStream_t s)
{
    if (N1 >= WIDE_FROM) {
        const dim3 grid((N1 + TW_WIDE - 1) / TW_WIDE), block(TW_WIDE, U);
        if (first) hipLaunchKernelGGL((smooth_path_kernel<U, TW_WIDE, true>), grid, block, 0, s, cost, acc, N0, N1, dr, dc, lam, trunc);
        else hipLaunchKernelGGL((smooth_path_kernel<U, TW_WIDE, false>), grid, block, 0, s, cost, acc, N0, N1, dr, dc, lam, trunc);
        return;
    }
    const dim3 grid((N1 + TW_NARROW - 1) / TW_NARROW), block(TW_NARROW, U);
    if (first) hipLaunchKernelGGL((smooth_path_kernel<U, TW_NARROW, true>), grid, block, 0, s, cost, acc, N0, N1, dr, dc, lam, trunc);
    else hipLaunchKernelGGL((smooth_path_kernel<U, TW_NARROW, false>), grid, block, 0, s, cost, acc, N0, N1, dr, dc, lam, trunc);
}

template <int U>
void launch_select(const double* cost, const double* total, size_t plane, int* shift, double* smin, double* margin, int* valid, hipStream_t s)
{
    hipLaunchKernelGGL(smooth_select_kernel<U>, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, cost, total, plane, shift, smin, margin, valid);
}

#define FOR_U(U, call, ...) switch (U) { \
    case 3: call<3>(__VA_ARGS__); break; case 5: call<5>(__VA_ARGS__); break; case 7: call<7>(__VA_ARGS__); break; \
    case 9: call<9>(__VA_ARGS__); break; case 11: call<11>(__VA_ARGS__); break; case 13: call<13>(__VA_ARGS__); break; \
    default: call<15>(__VA_ARGS__); break; }

// in[U * U][R][C] -> out[U * U][C][R]
void launch_transpose(bool add, const double* in, double* out, int U, int R, int C, hipStream_t s)
{
    const dim3 grid((C + TT - 1) / TT, (R + TT - 1) / TT, U * U), block(TT, 8);
    if (add) hipLaunchKernelGGL(smooth_transpose_kernel<true>, grid, block, 0, s, in, out, R, C);
    else hipLaunchKernelGGL(smooth_transpose_kernel<false>, grid, block, 0, s, in, out, R, C);
}

// Everything on device arrays: the passes in direction order, the sum, the selection.  `tot` is the volume the sum is
// left in; costT and HT (the transposed input and the transposed H) are needed where direction 0 or 1 is selected.
int run(const double* cost, int U, int N0, int N1, double lam, double trunc, int dirs, double* tot, double* costT, double* HT,
        int* shift, double* smin, double* margin, int* valid, hipStream_t s)
{
    const bool hasH = (dirs & 0x03) != 0, hasV = (dirs & 0xFC) != 0;
    if (hasH) {
        launch_transpose(false, cost, costT, U, N0, N1, s);
        LAUNCHED("smooth: launch of the transpose");
        bool first = true;
        for (int d = 0; d < 2; d++)
            if (dirs & (1 << d)) {                  // a row of the region is a column of the transposed copy
                FOR_U(U, launch_path, first, costT, HT, N1, N0, DIRS[d][1], 0, lam, trunc, s);
                LAUNCHED("smooth: launch of direction %d", d);
                first = false;
            }
    }
    bool first = true;
    for (int d = 2; d < 8; d++)
        if (dirs & (1 << d)) {
            FOR_U(U, launch_path, first, cost, tot, N0, N1, DIRS[d][0], DIRS[d][1], lam, trunc, s);
            LAUNCHED("smooth: launch of direction %d", d);
            first = false;
        }
    if (hasH) {
        launch_transpose(hasV, HT, tot, U, N1, N0, s);
        LAUNCHED("smooth: launch of the transpose");
    }
    FOR_U(U, launch_select, cost, tot, (size_t)N0 * N1, shift, smin, margin, valid, s);
    LAUNCHED("smooth: launch of the selection");
    return 0;
}

} // namespace

UMPA_SMOOTH_API const char* umpa_smooth_last_error(void) { return g_err.c_str(); }

UMPA_SMOOTH_API long long umpa_smooth_workspace_bytes(int U, int N0, int N1, int dirs)
{
    if (check_shape(U, N0, N1, dirs)) return -1;
    return (long long)volume_bytes(U, N0, N1) * ((dirs & 0x03) ? 3 : 1);
}

UMPA_SMOOTH_API int umpa_smooth_aggregate(const double* cost, int U, int N0, int N1, double lam, double trunc, int dirs,
                                          int* shift, double* smin, double* margin, int* valid, double* total,
                                          int device, int flags, void* stream)
{
    if (int rc = check_shape(U, N0, N1, dirs)) return rc;
    if (!(lam >= 0.0)) return fail(UMPA_HIP_E_ARG, "smooth: lam = %g (the penalty per label step must be >= 0)", lam);
    if (!(trunc >= 0.0)) return fail(UMPA_HIP_E_ARG, "smooth: trunc = %g (the truncation must be >= 0; +INF: none)", trunc);
    if (!cost || !shift) return fail(UMPA_HIP_E_ARG, "smooth: null argument (cost and shift are required)");
    if (flags & ~UMPA_HIP_F_DEVICE_IO) return fail(UMPA_HIP_E_ARG, "smooth: aggregate takes UMPA_HIP_F_DEVICE_IO and no other flag");
    if (int rc = pick_device("smooth", device)) return rc;

    const bool dio = (flags & UMPA_HIP_F_DEVICE_IO) != 0, hasH = (dirs & 0x03) != 0;
    const size_t vol = volume_bytes(U, N0, N1), n = (size_t)N0 * N1;
    size_t need = (hasH ? 2 : 0) * vol + ((dio && total) ? 0 : vol);
    if (!dio) need += vol + n * (2 * 4 + 8 + 8 + 4);
    size_t free_b = 0, all_b = 0;
    HIPOK(hipMemGetInfo(&free_b, &all_b), UMPA_HIP_E_DEVICE, "smooth: hipMemGetInfo");
    if (need > free_b)
        return fail(UMPA_HIP_E_UNSUPPORTED, "smooth: %zu bytes of device memory needed for a %d x %d x %d x %d volume, %zu free", need, U, U, N0, N1, free_b);

    // slots: 0 the sum, 1 the transposed input, 2 the transposed H; host arrays: 3 the input, 4 shift, 5 smin, 6 margin, 7 valid
    DeviceMem S;
    double* tot = dio ? total : nullptr;
    if (!tot) {
        HIPOK(S.alloc(0, vol), UMPA_HIP_E_NOMEM, "smooth: device memory for the sum");
        tot = (double*)S.p[0];
    }
    if (hasH) {
        HIPOK(S.alloc(1, vol), UMPA_HIP_E_NOMEM, "smooth: device memory for the transposed volume");
        HIPOK(S.alloc(2, vol), UMPA_HIP_E_NOMEM, "smooth: device memory for the transposed sum");
    }
    if (dio) {
        hipStream_t s = (hipStream_t)stream;
        if (int rc = run(cost, U, N0, N1, lam, trunc, dirs, tot, (double*)S.p[1], (double*)S.p[2], shift, smin, margin, valid, s)) return rc;
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "smooth: aggregate");
        return 0;
    }
    const size_t bytes[4] = {n * 8, n * 8, n * 8, n * 4};       // shift (two planes of ints), smin, margin, valid
    void* host[4] = {shift, smin, margin, valid};
    HIPOK(S.alloc(3, vol), UMPA_HIP_E_NOMEM, "smooth: device memory for the volume");
    for (int q = 0; q < 4; q++)
        if (host[q]) HIPOK(S.alloc(4 + q, bytes[q]), UMPA_HIP_E_NOMEM, "smooth: device memory for the results");
    HIPOK(hipMemcpy(S.p[3], cost, vol, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "smooth: upload of the volume");
    if (int rc = run((const double*)S.p[3], U, N0, N1, lam, trunc, dirs, tot, (double*)S.p[1], (double*)S.p[2],
                     (int*)S.p[4], (double*)S.p[5], (double*)S.p[6], (int*)S.p[7], nullptr)) return rc;
    for (int q = 0; q < 4; q++)
        if (host[q]) HIPOK(hipMemcpy(host[q], S.p[4 + q], bytes[q], hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "smooth: aggregate");
    if (total) HIPOK(hipMemcpy(total, tot, vol, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "smooth: download of the sum");
    return 0;
}
