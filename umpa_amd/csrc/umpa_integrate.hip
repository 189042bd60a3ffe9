// umpa_integrate.hip -- libumpa_integrate.so: weighted least-squares phase integration by multigrid-preconditioned
// conjugate gradients (include/umpa_integrate.h, where the operation and every elementwise expression is defined).
// gfx950 only.
//
// A fifth library beside libumpa_hip.so, libumpa_grid.so, libumpa_unwarp.so and libumpa_register.so, for the reason those
// have their own: the other libraries' kernel sets stay what they are.
//
// MAPPING.  Every kernel but two is one launch of 256-lane workgroups over the pixels of one level in row-major order: a
// wave's lanes are 64 adjacent pixels of a row (or the end of one and the start of the next), every load and store a
// contiguous run.  A level keeps the pixel weights w and the diagonal d; the edge weights are min() of two adjacent w,
// recomputed where they are used (two loads that the neighbouring lanes make anyway, instead of two more arrays).
//   setup      weights (w0), diag (d of any level), rhs (b), coarsen (w_c)
//   V-cycle    sweep0, sweep (L x fused with the Jacobi update), restrict (b - L x fused with P'), prolong (P fused with the
//              correction), jacobi (the F_JACOBI baseline), tail (below)
//   CG         apply_dot (L p with p . L p), update (the two axpys with |r|^2), residual (b - L x with |r|^2), dot,
//              direction (p = z + beta p), gauge (the sum and count of the d > 0 pixels), output
//   scalars    one workgroup adds the partial sums of the kernel before it and lane 0 derives alpha, beta and the flags;
//              they stay on the device (struct State) and the next kernel reads them through a pointer
// THE TAIL.  The coarse levels are launch-bound, so all levels from the first one at which 3 arrays (x, its ping-pong
// partner, b) of it and of every level below fit 160 KiB of LDS run in ONE workgroup of 1024 lanes: down, the coarsest
// sweeps, up, a barrier where the launched path has a launch boundary.  It calls the same per-pixel functions as the
// launched kernels, so it is bit-identical to them (UMPA_INTEGRATE_F_NO_TAIL launches every level; a test compares).
// No kernel waits for another workgroup; every dependence between workgroups is a launch boundary.
// No CPU fallback.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/umpa_integrate.h"
#include "umpa_host.h"

#pragma clang fp contract(off)

namespace umpa {

constexpr double OMEGA = 0.8;
constexpr int NU = 2;
constexpr int COARSE_SWEEPS = 30;
constexpr int COARSEST = 4;
constexpr int TAIL_DOUBLES = 160 * 1024 / 8;        // the whole LDS of a CU
constexpr int TAIL_LEVELS = 16;
constexpr int TAIL_THREADS = 1024;

// The scalars of one solve, on the device.
struct State {
    double rz, alpha, beta, bb, rr, resid, mean;
    int iters, done, verify, reset, status;
};

enum Step { S_BNORM, S_RZ0, S_ALPHA, S_CHECK, S_VERIFY, S_BETA, S_FINAL, S_MEAN };

// ----------------------------------------------------------------------------- the header's expressions, per pixel

struct Edges { double l, r, u, d; };

__device__ __forceinline__ double emin(double a, double b) { return a < b ? a : b; }

__device__ __forceinline__ Edges edges(const double* w, int H, int W, int i, int j)
{
    const int idx = i * W + j;
    const double w0 = w[idx];
    Edges e;
    e.l = j > 0 ? emin(w[idx - 1], w0) : 0.0;
    e.r = j + 1 < W ? emin(w0, w[idx + 1]) : 0.0;
    e.u = i > 0 ? emin(w[idx - W], w0) : 0.0;
    e.d = i + 1 < H ? emin(w0, w[idx + W]) : 0.0;
    return e;
}

__device__ __forceinline__ double diag_px(const double* w, int H, int W, int i, int j)
{
    const Edges e = edges(w, H, W, i, j);
    return ((e.l + e.r) + e.u) + e.d;
}

__device__ __forceinline__ double apply_px(const double* w, const double* x, int H, int W, int i, int j)
{
    const Edges e = edges(w, H, W, i, j);
    const int idx = i * W + j;
    const double x0 = x[idx];
    const double xl = j > 0 ? x[idx - 1] : x0;
    const double xr = j + 1 < W ? x[idx + 1] : x0;
    const double xu = i > 0 ? x[idx - W] : x0;
    const double xd = i + 1 < H ? x[idx + W] : x0;
    return ((e.l * (x0 - xl) + e.r * (x0 - xr)) + e.u * (x0 - xu)) + e.d * (x0 - xd);
}

__device__ __forceinline__ double sweep0_px(double d, double b) { return d > 0.0 ? OMEGA * (b / d) : 0.0; }

__device__ __forceinline__ double sweep_px(const double* w, const double* dg, const double* x, const double* b, int H, int W, int i, int j)
{
    const int idx = i * W + j;
    const double d = dg[idx], x0 = x[idx];
    return d > 0.0 ? x0 + OMEGA * ((b[idx] - apply_px(w, x, H, W, i, j)) / d) : x0;
}

// the 1-D weights of the fine nodes 2 I - 1, 2 I, 2 I + 1 on the coarse node I of an axis of n fine, nc coarse nodes
__device__ __forceinline__ void pweights(int I, int n, int nc, double& pm, double& pp)
{
    pm = I >= 1 ? 0.5 : 0.0;
    pp = 2 * I + 1 < n ? (I + 1 < nc ? 0.5 : 1.0) : 0.0;
}

// (P' v)[I, J] for v = b - L x (RESIDUAL) or v = x (the weights), den: P' 1
template <bool RESIDUAL>
__device__ __forceinline__ double restrict_px(const double* w, const double* x, const double* b, int H, int W, int Hc, int Wc,
                                              int I, int J, double* den)
{
    double am, ap, bm, bp;
    pweights(I, H, Hc, am, ap);
    pweights(J, W, Wc, bm, bp);
    const double a3[3] = {am, 1.0, ap}, b3[3] = {bm, 1.0, bp};
    double s[3], o[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int i = 2 * I + a - 1;
        double v[3], one[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int j = 2 * J + c - 1;
            const bool in = i >= 0 && i < H && j >= 0 && j < W;
            one[c] = in ? 1.0 : 0.0;
            if (!in) v[c] = 0.0;
            else if (RESIDUAL) v[c] = b[i * W + j] - apply_px(w, x, H, W, i, j);
            else v[c] = x[i * W + j];
        }
        s[a] = (b3[0] * v[0] + b3[1] * v[1]) + b3[2] * v[2];
        o[a] = (b3[0] * one[0] + b3[1] * one[1]) + b3[2] * one[2];
    }
    if (den) *den = (a3[0] * o[0] + a3[1] * o[1]) + a3[2] * o[2];
    return (a3[0] * s[0] + a3[1] * s[1]) + a3[2] * s[2];
}

// (P e)[i, j]
__device__ __forceinline__ double prolong_px(const double* e, int Hc, int Wc, int i, int j)
{
    const int I = i >> 1, J = j >> 1;
    const bool jo = (j & 1) && J + 1 < Wc, io = (i & 1) && I + 1 < Hc;
    const double* r0 = e + I * Wc + J;
    const double v0 = jo ? 0.5 * (r0[0] + r0[1]) : r0[0];
    if (!io) return v0;
    const double* r1 = r0 + Wc;
    const double v1 = jo ? 0.5 * (r1[0] + r1[1]) : r1[0];
    return 0.5 * (v0 + v1);
}

// the sum of the workgroup's 256 values in a fixed tree; the result is valid in lane 0
__device__ __forceinline__ double block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

#define PIXEL(n) const unsigned uidx_ = blockIdx.x * 256u + threadIdx.x; const bool in = uidx_ < (unsigned)(n); const int idx = (int)uidx_
#define SKIP_IF_DONE(st) if ((st) && (st)->done) return

// ----------------------------------------------------------------------------- setup

__global__ void __launch_bounds__(256)
integrate_weights_kernel(const double* __restrict__ w, const double* __restrict__ gx, const double* __restrict__ gy,
                         double* __restrict__ w0, int n)
{
    PIXEL(n);
    if (!in) return;
    double v = 1.0;
    if (w) v = w[idx] > 0.0 ? w[idx] : 0.0;
    else if (gx) v = (isfinite(gx[idx]) && isfinite(gy[idx])) ? 1.0 : 0.0;
    w0[idx] = v;
}

__global__ void __launch_bounds__(256)
integrate_diag_kernel(const double* __restrict__ w, double* __restrict__ d, int H, int W)
{
    PIXEL(H * W);
    if (!in) return;
    const int i = idx / W, j = idx - i * W;
    d[idx] = diag_px(w, H, W, i, j);
}

__global__ void __launch_bounds__(256)
integrate_rhs_kernel(const double* __restrict__ w, const double* __restrict__ gx, const double* __restrict__ gy,
                     double* __restrict__ b, int H, int W)
{
    PIXEL(H * W);
    if (!in) return;
    const int i = idx / W, j = idx - i * W;
    const Edges e = edges(w, H, W, i, j);
    const double tl = e.l > 0.0 ? e.l * (0.5 * (gx[idx - 1] + gx[idx])) : 0.0;
    const double tr = e.r > 0.0 ? e.r * (0.5 * (gx[idx] + gx[idx + 1])) : 0.0;
    const double tu = e.u > 0.0 ? e.u * (0.5 * (gy[idx - W] + gy[idx])) : 0.0;
    const double td = e.d > 0.0 ? e.d * (0.5 * (gy[idx] + gy[idx + W])) : 0.0;
    b[idx] = ((tl - tr) + tu) - td;
}

__global__ void __launch_bounds__(256)
integrate_coarsen_kernel(const double* __restrict__ wf, int H, int W, double* __restrict__ wc, int Hc, int Wc)
{
    PIXEL(Hc * Wc);
    if (!in) return;
    const int I = idx / Wc, J = idx - I * Wc;
    double den;
    const double num = restrict_px<false>(nullptr, wf, nullptr, H, W, Hc, Wc, I, J, &den);
    wc[idx] = num / den;
}

// ----------------------------------------------------------------------------- the V-cycle, level by level

__global__ void __launch_bounds__(256)
integrate_sweep0_kernel(const double* __restrict__ d, const double* __restrict__ b, double* __restrict__ x, int n, const State* st)
{
    SKIP_IF_DONE(st);
    PIXEL(n);
    if (in) x[idx] = sweep0_px(d[idx], b[idx]);
}

__global__ void __launch_bounds__(256)
integrate_sweep_kernel(const double* __restrict__ w, const double* __restrict__ d, const double* __restrict__ x,
                       const double* __restrict__ b, double* __restrict__ xn, int H, int W, const State* st)
{
    SKIP_IF_DONE(st);
    PIXEL(H * W);
    if (!in) return;
    const int i = idx / W, j = idx - i * W;
    xn[idx] = sweep_px(w, d, x, b, H, W, i, j);
}

__global__ void __launch_bounds__(256)
integrate_restrict_kernel(const double* __restrict__ w, const double* __restrict__ x, const double* __restrict__ b, int H, int W,
                          double* __restrict__ bc, int Hc, int Wc, const State* st)
{
    SKIP_IF_DONE(st);
    PIXEL(Hc * Wc);
    if (!in) return;
    const int I = idx / Wc, J = idx - I * Wc;
    bc[idx] = restrict_px<true>(w, x, b, H, W, Hc, Wc, I, J, nullptr);
}

__global__ void __launch_bounds__(256)
integrate_prolong_kernel(const double* __restrict__ xc, int Hc, int Wc, double* __restrict__ x, int H, int W, const State* st)
{
    SKIP_IF_DONE(st);
    PIXEL(H * W);
    if (!in) return;
    const int i = idx / W, j = idx - i * W;
    x[idx] = x[idx] + prolong_px(xc, Hc, Wc, i, j);
}

__global__ void __launch_bounds__(256)
integrate_jacobi_kernel(const double* __restrict__ d, const double* __restrict__ r, double* __restrict__ z, int n, const State* st)
{
    SKIP_IF_DONE(st);
    PIXEL(n);
    if (in) z[idx] = d[idx] > 0.0 ? r[idx] / d[idx] : 0.0;
}

// The levels of the tail: level 0 of it reads its right-hand side from b_in and leaves its result in x_out (global);
// everything between lives in LDS, three arrays per level.
struct TailArgs {
    int nlev;
    int H[TAIL_LEVELS], W[TAIL_LEVELS];
    const double* w[TAIL_LEVELS];
    const double* d[TAIL_LEVELS];
    const double* b_in;
    double* x_out;
};

__device__ __forceinline__ void tail_sweep0(const double* d, const double* b, double* x, int n)
{
    for (int e = threadIdx.x; e < n; e += TAIL_THREADS) x[e] = sweep0_px(d[e], b[e]);
    __syncthreads();
}

__device__ __forceinline__ void tail_sweep(const double* w, const double* d, const double* x, const double* b, double* xn, int H, int W)
{
    for (int e = threadIdx.x; e < H * W; e += TAIL_THREADS) {
        const int i = e / W, j = e - i * W;
        xn[e] = sweep_px(w, d, x, b, H, W, i, j);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(TAIL_THREADS)
integrate_tail_kernel(const TailArgs a, const State* st)
{
    __shared__ double lds[TAIL_DOUBLES];
    SKIP_IF_DONE(st);
    // level l keeps x, t, b at lds + off, + n, + 2 n; the offsets are walked, not stored (no private array)
    {
        double* B0 = lds + 2 * a.H[0] * a.W[0];
        for (int e = threadIdx.x; e < a.H[0] * a.W[0]; e += TAIL_THREADS) B0[e] = a.b_in[e];
        __syncthreads();
    }
    const int last = a.nlev - 1;
    int off = 0;
    for (int l = 0; l < last; l++) {
        const int H = a.H[l], W = a.W[l], Hc = a.H[l + 1], Wc = a.W[l + 1], n = H * W;
        double *X = lds + off, *T = X + n, *B = T + n, *Bc = B + n + 2 * Hc * Wc;
        tail_sweep0(a.d[l], B, X, n);
        tail_sweep(a.w[l], a.d[l], X, B, T, H, W);            // NU = 2: the second sweep, x -> t
        for (int e = threadIdx.x; e < Hc * Wc; e += TAIL_THREADS) {
            const int I = e / Wc, J = e - I * Wc;
            Bc[e] = restrict_px<true>(a.w[l], T, B, H, W, Hc, Wc, I, J, nullptr);
        }
        __syncthreads();
        off += 3 * n;
    }
    {
        const int H = a.H[last], W = a.W[last], n = H * W;
        double *X = lds + off, *T = X + n, *B = T + n;
        tail_sweep0(a.d[last], B, X, n);
        for (int s = 1; s < COARSE_SWEEPS; s++) {             // 29 sweeps, the last one x -> t
            if (s & 1) tail_sweep(a.w[last], a.d[last], X, B, T, H, W);
            else tail_sweep(a.w[last], a.d[last], T, B, X, H, W);
        }
    }
    for (int l = last - 1; l >= 0; l--) {
        const int H = a.H[l], W = a.W[l], Hc = a.H[l + 1], Wc = a.W[l + 1], n = H * W;
        const double* Tc = lds + off + Hc * Wc;
        off -= 3 * n;
        double *X = lds + off, *T = X + n, *B = T + n;
        for (int e = threadIdx.x; e < n; e += TAIL_THREADS) {
            const int i = e / W, j = e - i * W;
            T[e] = T[e] + prolong_px(Tc, Hc, Wc, i, j);
        }
        __syncthreads();
        tail_sweep(a.w[l], a.d[l], T, B, X, H, W);
        tail_sweep(a.w[l], a.d[l], X, B, T, H, W);
    }
    {
        const double* T = lds + a.H[0] * a.W[0];
        for (int e = threadIdx.x; e < a.H[0] * a.W[0]; e += TAIL_THREADS) a.x_out[e] = T[e];
    }
}

// ----------------------------------------------------------------------------- conjugate gradients

__global__ void __launch_bounds__(256)
integrate_apply_dot_kernel(const double* __restrict__ w, const double* __restrict__ p, double* __restrict__ Ap,
                           double* __restrict__ part, int H, int W, const State* st)
{
    __shared__ double sh[256];
    SKIP_IF_DONE(st);
    PIXEL(H * W);
    double term = 0.0;
    if (in) {
        const int i = idx / W, j = idx - i * W;
        const double v = apply_px(w, p, H, W, i, j);
        Ap[idx] = v;
        term = p[idx] * v;
    }
    const double s = block_sum(term, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
integrate_update_kernel(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p, const double* __restrict__ Ap,
                        double* __restrict__ part, int n, const State* st)
{
    __shared__ double sh[256];
    SKIP_IF_DONE(st);
    PIXEL(n);
    const double alpha = st->alpha;
    double term = 0.0;
    if (in) {
        x[idx] = x[idx] + alpha * p[idx];
        const double rv = r[idx] - alpha * Ap[idx];
        r[idx] = rv;
        term = rv * rv;
    }
    const double s = block_sum(term, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// r = b - L x and the partial sums of |r|^2; runs when the state asks for the true residual, or always (force)
__global__ void __launch_bounds__(256)
integrate_residual_kernel(const double* __restrict__ w, const double* __restrict__ x, const double* __restrict__ b,
                          double* __restrict__ r, double* __restrict__ part, int H, int W, const State* st, int force)
{
    __shared__ double sh[256];
    if (!force && (st->done || !st->verify)) return;
    PIXEL(H * W);
    double term = 0.0;
    if (in) {
        const int i = idx / W, j = idx - i * W;
        const double rv = b[idx] - apply_px(w, x, H, W, i, j);
        r[idx] = rv;
        term = rv * rv;
    }
    const double s = block_sum(term, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
integrate_dot_kernel(const double* __restrict__ u, const double* __restrict__ v, double* __restrict__ part, int n, const State* st)
{
    __shared__ double sh[256];
    SKIP_IF_DONE(st);
    PIXEL(n);
    const double s = block_sum(in ? u[idx] * v[idx] : 0.0, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
integrate_direction_kernel(const double* __restrict__ z, double* __restrict__ p, int n, const State* st)
{
    SKIP_IF_DONE(st);
    PIXEL(n);
    if (in) p[idx] = z[idx] + st->beta * p[idx];
}

// the partial sums of x over the pixels with d > 0 (part) and of their count (cnt)
__global__ void __launch_bounds__(256)
integrate_gauge_kernel(const double* __restrict__ x, const double* __restrict__ d, double* __restrict__ part, double* __restrict__ cnt, int n)
{
    __shared__ double sh[256];
    PIXEL(n);
    const bool on = in && d[idx] > 0.0;
    const double s = block_sum(on ? x[idx] : 0.0, sh);
    __syncthreads();
    const double c = block_sum(on ? 1.0 : 0.0, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = s; cnt[blockIdx.x] = c; }
}

__global__ void __launch_bounds__(256)
integrate_output_kernel(const double* __restrict__ x, const double* __restrict__ d, double* __restrict__ phi, double fill, int n, const State* st)
{
    PIXEL(n);
    if (in) phi[idx] = d[idx] > 0.0 ? x[idx] - st->mean : fill;
}

// Stage two of every reduction and the scalar step that follows it: ONE workgroup; lane t adds the partial sums t, t + 256,
// ... in that order, the 256 sums go through the fixed tree, lane 0 updates the state.
__global__ void __launch_bounds__(256)
integrate_scalar_kernel(const double* __restrict__ part, const double* __restrict__ part2, int nparts, State* st, int step, double tol)
{
    __shared__ double sh[256];
    const bool iteration = step == S_ALPHA || step == S_CHECK || step == S_VERIFY || step == S_BETA || step == S_RZ0;
    if (iteration && st->done) return;
    if (step == S_VERIFY && !st->verify) return;
    double acc = 0.0, acc2 = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) {
        acc = acc + part[k];
        if (part2) acc2 = acc2 + part2[k];
    }
    const double sum = block_sum(acc, sh);
    __syncthreads();
    const double sum2 = part2 ? block_sum(acc2, sh) : 0.0;
    if (threadIdx.x != 0) return;
    switch (step) {
    case S_BNORM:
        st->bb = sum;
        if (!isfinite(sum)) { st->done = 1; st->status = UMPA_INTEGRATE_BREAKDOWN; }
        else if (sum == 0.0) { st->done = 1; st->status = UMPA_INTEGRATE_CONVERGED; }
        break;
    case S_RZ0:
        st->rz = sum;
        if (!isfinite(sum)) { st->done = 1; st->status = UMPA_INTEGRATE_BREAKDOWN; }
        break;
    case S_ALPHA:
        if (!(sum > 0.0) || !isfinite(sum)) { st->done = 1; st->status = UMPA_INTEGRATE_BREAKDOWN; }
        else st->alpha = st->rz / sum;
        break;
    case S_CHECK:
        st->rr = sum;
        st->iters = st->iters + 1;
        if (!isfinite(sum)) { st->done = 1; st->status = UMPA_INTEGRATE_BREAKDOWN; }
        else if (sqrt(sum) <= tol * sqrt(st->bb)) st->verify = 1;
        break;
    case S_VERIFY:
        st->verify = 0;
        st->rr = sum;
        if (sqrt(sum) <= tol * sqrt(st->bb)) { st->done = 1; st->status = UMPA_INTEGRATE_CONVERGED; }
        else st->reset = 1;
        break;
    case S_BETA:
        st->beta = st->reset ? 0.0 : sum / st->rz;
        st->rz = sum;
        st->reset = 0;
        if (!isfinite(sum)) { st->done = 1; st->status = UMPA_INTEGRATE_BREAKDOWN; }
        break;
    case S_FINAL:
        st->resid = st->bb > 0.0 ? sqrt(sum) / sqrt(st->bb) : 0.0;
        if (!st->done) st->status = UMPA_INTEGRATE_MAXITER;
        break;
    case S_MEAN:
        st->mean = sum2 > 0.0 ? sum / sum2 : 0.0;
        break;
    }
}

} // namespace umpa

using namespace umpa;

#define UMPA_INTEGRATE_API extern "C" __attribute__((visibility("default")))

namespace {

struct Level { int H, W; double *w, *d, *x, *t, *b; };

inline dim3 blocks(int n) { return dim3((unsigned)((n + 255) / 256)); }

// The device memory of one call: one allocation, carved into arrays of doubles.
struct Slab {
    char* base = nullptr;
    size_t used = 0, size = 0;
    ~Slab() { if (base) (void)hipFree(base); }
    static size_t pad(size_t n) { return (n * sizeof(double) + 255) / 256 * 256; }
    double* take(size_t n) { double* p = (double*)(base + used); used += pad(n); return p; }
};

struct Hierarchy {
    std::vector<Level> lv;
    int tail = 0;              // the first level of the tail kernel; lv.size() when every level is launched
    TailArgs targs;
};

std::vector<std::pair<int, int>> level_shapes(int H, int W, bool jacobi)
{
    std::vector<std::pair<int, int>> s;
    s.push_back({H, W});
    while (!jacobi && std::min(s.back().first, s.back().second) > COARSEST)
        s.push_back({(s.back().first + 1) / 2, (s.back().second + 1) / 2});
    return s;
}

// the doubles a hierarchy takes from the slab: w, d, x per level, t and b below the fine level (the caller owns the fine ones)
size_t hierarchy_doubles(const std::vector<std::pair<int, int>>& s)
{
    size_t n = 0;
    for (size_t l = 0; l < s.size(); l++)
        n += (l == 0 ? 3 : 5) * Slab::pad((size_t)s[l].first * s[l].second) / sizeof(double);
    return n;
}

void carve(Hierarchy& h, const std::vector<std::pair<int, int>>& s, Slab& slab, bool no_tail)
{
    for (size_t l = 0; l < s.size(); l++) {
        Level v;
        v.H = s[l].first; v.W = s[l].second;
        const size_t n = (size_t)v.H * v.W;
        v.w = slab.take(n); v.d = slab.take(n); v.x = slab.take(n);
        v.t = l ? slab.take(n) : nullptr;
        v.b = l ? slab.take(n) : nullptr;
        h.lv.push_back(v);
    }
    const int L = (int)h.lv.size();
    h.tail = L;
    if (!no_tail) {
        long long sum = 0;
        for (int l = L - 1; l >= 0 && L - l <= TAIL_LEVELS; l--) {
            sum += 3LL * h.lv[l].H * h.lv[l].W;
            if (sum > TAIL_DOUBLES) break;
            h.tail = l;
        }
    }
}

// w0 of the fine level is written already: d of it, then w_c and d of every coarser level
hipError_t build_levels(Hierarchy& h, hipStream_t s)
{
    for (size_t l = 0; l < h.lv.size(); l++) {
        Level& v = h.lv[l];
        if (l) {
            const Level& f = h.lv[l - 1];
            hipLaunchKernelGGL(integrate_coarsen_kernel, blocks(v.H * v.W), dim3(256), 0, s, (const double*)f.w, f.H, f.W, v.w, v.H, v.W);
        }
        hipLaunchKernelGGL(integrate_diag_kernel, blocks(v.H * v.W), dim3(256), 0, s, (const double*)v.w, v.d, v.H, v.W);
    }
    return hipGetLastError();
}

void sweep(const Level& v, const double* x, double* xn, const State* st, hipStream_t s)
{
    hipLaunchKernelGGL(integrate_sweep_kernel, blocks(v.H * v.W), dim3(256), 0, s, (const double*)v.w, (const double*)v.d, x,
                       (const double*)v.b, xn, v.H, v.W, st);
}

// z = M r: the fine level's b is r and its t is z.  Every level leaves its result in t (NU = 2 and 29 sweeps after the
// one from zero: x -> t is always the last sweep).
static_assert(NU == 2 && COARSE_SWEEPS % 2 == 0, "the ping-pong of vcycle() and of the tail kernel ends in t");

hipError_t vcycle(Hierarchy& h, const double* r, double* z, const State* st, hipStream_t s)
{
    h.lv[0].b = const_cast<double*>(r);
    h.lv[0].t = z;
    const int L = (int)h.lv.size();
    int bottom = 0;
    for (int l = 0; ; l++) {
        const Level& v = h.lv[l];
        const int n = v.H * v.W;
        bottom = l;
        if (l == h.tail) {
            TailArgs a;
            memset(&a, 0, sizeof(a));
            a.nlev = L - l;
            for (int k = l; k < L; k++) { a.H[k - l] = h.lv[k].H; a.W[k - l] = h.lv[k].W; a.w[k - l] = h.lv[k].w; a.d[k - l] = h.lv[k].d; }
            a.b_in = v.b; a.x_out = v.t;
            hipLaunchKernelGGL(integrate_tail_kernel, dim3(1), dim3(TAIL_THREADS), 0, s, a, st);
            break;
        }
        hipLaunchKernelGGL(integrate_sweep0_kernel, blocks(n), dim3(256), 0, s, (const double*)v.d, (const double*)v.b, v.x, n, st);
        if (l == L - 1) {
            double *src = v.x, *dst = v.t;
            for (int k = 1; k < COARSE_SWEEPS; k++) { sweep(v, src, dst, st, s); std::swap(src, dst); }
            break;
        }
        sweep(v, v.x, v.t, st, s);
        const Level& c = h.lv[l + 1];
        hipLaunchKernelGGL(integrate_restrict_kernel, blocks(c.H * c.W), dim3(256), 0, s, (const double*)v.w, (const double*)v.t,
                           (const double*)v.b, v.H, v.W, c.b, c.H, c.W, st);
    }
    for (int l = bottom - 1; l >= 0; l--) {
        const Level& v = h.lv[l];
        const Level& c = h.lv[l + 1];
        hipLaunchKernelGGL(integrate_prolong_kernel, blocks(v.H * v.W), dim3(256), 0, s, (const double*)c.t, c.H, c.W, v.t, v.H, v.W, st);
        sweep(v, v.t, v.x, st, s);
        sweep(v, v.x, v.t, st, s);
    }
    return hipGetLastError();
}

hipError_t precondition(Hierarchy& h, bool jacobi, const double* r, double* z, const State* st, hipStream_t s)
{
    if (!jacobi) return vcycle(h, r, z, st, s);
    const Level& v = h.lv[0];
    hipLaunchKernelGGL(integrate_jacobi_kernel, blocks(v.H * v.W), dim3(256), 0, s, (const double*)v.d, r, z, v.H * v.W, st);
    return hipGetLastError();
}

int check_common(int H, int W, int device, int flags, int allowed)
{
    if (flags & ~allowed) return fail(UMPA_HIP_E_ARG, "integrate: flags %d: UMPA_HIP_F_DEVICE_IO, UMPA_INTEGRATE_F_NO_TAIL, UMPA_INTEGRATE_F_JACOBI, UMPA_INTEGRATE_F_DEBUG and no other flag", flags);
    if (H < 2 || W < 2 || (long long)H * W >= (1LL << 31)) return fail(UMPA_HIP_E_ARG, "integrate: maps of %d x %d pixels (H, W >= 2 and H * W < 2^31)", H, W);
    (void)device;
    return 0;
}

constexpr int ALL_FLAGS = UMPA_HIP_F_DEVICE_IO | UMPA_INTEGRATE_F_NO_TAIL | UMPA_INTEGRATE_F_JACOBI | UMPA_INTEGRATE_F_DEBUG;

} // namespace

UMPA_INTEGRATE_API const char* umpa_integrate_last_error(void) { return g_err.c_str(); }

UMPA_INTEGRATE_API int umpa_integrate_vcycle(const double* w, const double* r, double* z, int H, int W, int device, int flags, void* stream)
{
    if (!r || !z) return fail(UMPA_HIP_E_ARG, "integrate: null argument");
    if (int rc = check_common(H, W, device, flags, ALL_FLAGS)) return rc;
    const bool dev_io = flags & UMPA_HIP_F_DEVICE_IO, jacobi = flags & UMPA_INTEGRATE_F_JACOBI;
    const int n = H * W;
    if (w && !dev_io) {
        const size_t i = bad_weight(w, (size_t)n);
        if (i < (size_t)n) return fail(UMPA_HIP_E_ARG, "integrate: weights must be finite and >= 0 (pixel (%d, %d))", (int)(i / W), (int)(i % W));
    }
    if (int rc = pick_device("integrate", device)) return rc;
    hipStream_t s = dev_io ? (hipStream_t)stream : nullptr;
    const auto shapes = level_shapes(H, W, jacobi);
    Slab slab;
    slab.size = hierarchy_doubles(shapes) * sizeof(double) + (dev_io ? 0 : 3 * Slab::pad(n));
    HIPOK(hipMalloc((void**)&slab.base, slab.size), UMPA_HIP_E_NOMEM, "integrate: device memory for the workspace");
    Hierarchy h;
    carve(h, shapes, slab, flags & UMPA_INTEGRATE_F_NO_TAIL);
    const double *dw = w, *dr = r;
    double* dz = z;
    if (!dev_io) {
        double* hw = slab.take(n); double* hr = slab.take(n); dz = slab.take(n);
        if (w) HIPOK(hipMemcpy(hw, w, (size_t)n * 8, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "integrate: upload");
        HIPOK(hipMemcpy(hr, r, (size_t)n * 8, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "integrate: upload");
        dw = w ? hw : nullptr; dr = hr;
    }
    hipLaunchKernelGGL(integrate_weights_kernel, blocks(n), dim3(256), 0, s, dw, (const double*)nullptr, (const double*)nullptr, h.lv[0].w, n);
    LAUNCHED("integrate: weights");
    HIPOK(build_levels(h, s), UMPA_HIP_E_LAUNCH, "integrate: building the levels");
    if (flags & UMPA_INTEGRATE_F_DEBUG)
        HIPOK(hipMemcpyAsync(dz, h.lv[0].d, (size_t)n * 8, hipMemcpyDeviceToDevice, s), UMPA_HIP_E_LAUNCH, "integrate: copy of d");
    else
        HIPOK(precondition(h, jacobi, dr, dz, nullptr, s), UMPA_HIP_E_LAUNCH, "integrate: the V-cycle");
    HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "integrate: the V-cycle");
    if (!dev_io) HIPOK(hipMemcpy(z, dz, (size_t)n * 8, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "integrate: download");
    return 0;
}

UMPA_INTEGRATE_API int umpa_integrate_solve(const double* gx, const double* gy, const double* w, int K, int H, int W,
                                            double tol, int maxiter, double fill, double* phi, int* iters, double* resid, int* status,
                                            int device, int flags, void* stream)
{
    if (!gx || !gy || !phi || !iters || !resid || !status) return fail(UMPA_HIP_E_ARG, "integrate: null argument");
    if (K < 0) return fail(UMPA_HIP_E_ARG, "integrate: K = %d", K);
    if (int rc = check_common(H, W, device, flags, ALL_FLAGS)) return rc;
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(UMPA_HIP_E_ARG, "integrate: tol = %g (finite and >= 0)", tol);
    if (maxiter < 0) return fail(UMPA_HIP_E_ARG, "integrate: maxiter = %d", maxiter);
    const bool dev_io = flags & UMPA_HIP_F_DEVICE_IO, jacobi = flags & UMPA_INTEGRATE_F_JACOBI, debug = flags & UMPA_INTEGRATE_F_DEBUG;
    const int n = H * W;
    if (w && !dev_io) {
        const size_t i = bad_weight(w, (size_t)n * K);
        if (i < (size_t)n * K) return fail(UMPA_HIP_E_ARG, "integrate: weights must be finite and >= 0 (map %d, pixel (%d, %d))", (int)(i / n), (int)(i % n / W), (int)(i % W));
    }
    if (int rc = pick_device("integrate", device)) return rc;
    if (K == 0) return 0;
    hipStream_t s = dev_io ? (hipStream_t)stream : nullptr;

    const auto shapes = level_shapes(H, W, jacobi);
    const int nb = (n + 255) / 256;
    Slab slab;
    // x, r, z, p, Ap, b; two arrays of partial sums; the state; host arrays: gx, gy, w, phi
    slab.size = hierarchy_doubles(shapes) * sizeof(double) + 6 * Slab::pad(n) + 2 * Slab::pad(nb) + Slab::pad(32) + (dev_io ? 0 : 4 * Slab::pad(n));
    HIPOK(hipMalloc((void**)&slab.base, slab.size), UMPA_HIP_E_NOMEM, "integrate: device memory for the workspace");
    Hierarchy h;
    carve(h, shapes, slab, flags & UMPA_INTEGRATE_F_NO_TAIL);
    double *x = slab.take(n), *r = slab.take(n), *z = slab.take(n), *p = slab.take(n), *Ap = slab.take(n), *b = slab.take(n);
    double *part = slab.take(nb), *part2 = slab.take(nb);
    static_assert(sizeof(State) <= 32 * sizeof(double), "the state's slot");
    State* st = (State*)slab.take(32);
    double *hgx = nullptr, *hgy = nullptr, *hw = nullptr, *hphi = nullptr;
    if (!dev_io) { hgx = slab.take(n); hgy = slab.take(n); hw = slab.take(n); hphi = slab.take(n); }
    const Level& f = h.lv[0];
    const dim3 grid = blocks(n), one(1), tb(256);
    const double* none = nullptr;

    for (int k = 0; k < K; k++) {
        const double *dgx = gx + (size_t)k * n, *dgy = gy + (size_t)k * n, *dw = w ? w + (size_t)k * n : nullptr;
        double* dphi = phi + (size_t)k * n;
        if (!dev_io) {
            HIPOK(hipMemcpy(hgx, dgx, (size_t)n * 8, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "integrate: upload");
            HIPOK(hipMemcpy(hgy, dgy, (size_t)n * 8, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "integrate: upload");
            if (w) HIPOK(hipMemcpy(hw, dw, (size_t)n * 8, hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "integrate: upload");
            dgx = hgx; dgy = hgy; dw = w ? hw : nullptr; dphi = hphi;
        }
        hipLaunchKernelGGL(integrate_weights_kernel, grid, tb, 0, s, dw, dgx, dgy, f.w, n);
        LAUNCHED("integrate: weights");
        HIPOK(build_levels(h, s), UMPA_HIP_E_LAUNCH, "integrate: building the levels");
        hipLaunchKernelGGL(integrate_rhs_kernel, grid, tb, 0, s, (const double*)f.w, dgx, dgy, b, H, W);
        LAUNCHED("integrate: rhs");
        State host;
        memset(&host, 0, sizeof(host));
        host.status = UMPA_INTEGRATE_MAXITER;
        if (debug) {
            HIPOK(hipMemcpyAsync(dphi, b, (size_t)n * 8, hipMemcpyDeviceToDevice, s), UMPA_HIP_E_LAUNCH, "integrate: copy of b");
            HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "integrate: rhs");
        } else {
            HIPOK(hipMemsetAsync(st, 0, sizeof(State), s), UMPA_HIP_E_LAUNCH, "integrate: state");
            HIPOK(hipMemsetAsync(x, 0, (size_t)n * 8, s), UMPA_HIP_E_LAUNCH, "integrate: x = 0");
            HIPOK(hipMemsetAsync(p, 0, (size_t)n * 8, s), UMPA_HIP_E_LAUNCH, "integrate: p = 0");
            HIPOK(hipMemcpyAsync(r, b, (size_t)n * 8, hipMemcpyDeviceToDevice, s), UMPA_HIP_E_LAUNCH, "integrate: r = b");
            hipLaunchKernelGGL(integrate_dot_kernel, grid, tb, 0, s, (const double*)b, (const double*)b, part, n, (const State*)nullptr);
            hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_BNORM, tol);
            HIPOK(precondition(h, jacobi, r, z, st, s), UMPA_HIP_E_LAUNCH, "integrate: the V-cycle");
            hipLaunchKernelGGL(integrate_dot_kernel, grid, tb, 0, s, (const double*)r, (const double*)z, part, n, (const State*)st);
            hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_RZ0, tol);
            hipLaunchKernelGGL(integrate_direction_kernel, grid, tb, 0, s, (const double*)z, p, n, (const State*)st);   // beta = 0 and p = 0: p = z
            LAUNCHED("integrate: the start of the iteration");
            for (int it = 0; it < maxiter; it++) {
                hipLaunchKernelGGL(integrate_apply_dot_kernel, grid, tb, 0, s, (const double*)f.w, (const double*)p, Ap, part, H, W, (const State*)st);
                hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_ALPHA, tol);
                hipLaunchKernelGGL(integrate_update_kernel, grid, tb, 0, s, x, r, (const double*)p, (const double*)Ap, part, n, (const State*)st);
                hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_CHECK, tol);
                hipLaunchKernelGGL(integrate_residual_kernel, grid, tb, 0, s, (const double*)f.w, (const double*)x, (const double*)b, r, part, H, W, (const State*)st, 0);
                hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_VERIFY, tol);
                HIPOK(precondition(h, jacobi, r, z, st, s), UMPA_HIP_E_LAUNCH, "integrate: the V-cycle");
                hipLaunchKernelGGL(integrate_dot_kernel, grid, tb, 0, s, (const double*)r, (const double*)z, part, n, (const State*)st);
                hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_BETA, tol);
                hipLaunchKernelGGL(integrate_direction_kernel, grid, tb, 0, s, (const double*)z, p, n, (const State*)st);
                LAUNCHED("integrate: an iteration");
                if ((it + 1) % UMPA_INTEGRATE_CHECK_EVERY == 0 && it + 1 < maxiter) {
                    HIPOK(hipMemcpyAsync(&host, st, sizeof(State), hipMemcpyDeviceToHost, s), UMPA_HIP_E_LAUNCH, "integrate: reading the flags");
                    HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "integrate: an iteration");
                    if (host.done) break;
                }
            }
            hipLaunchKernelGGL(integrate_residual_kernel, grid, tb, 0, s, (const double*)f.w, (const double*)x, (const double*)b, r, part, H, W, (const State*)st, 1);
            hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, none, nb, st, (int)S_FINAL, tol);
            hipLaunchKernelGGL(integrate_gauge_kernel, grid, tb, 0, s, (const double*)x, (const double*)f.d, part, part2, n);
            hipLaunchKernelGGL(integrate_scalar_kernel, one, tb, 0, s, (const double*)part, (const double*)part2, nb, st, (int)S_MEAN, tol);
            hipLaunchKernelGGL(integrate_output_kernel, grid, tb, 0, s, (const double*)x, (const double*)f.d, dphi, fill, n, (const State*)st);
            LAUNCHED("integrate: the output");
            HIPOK(hipMemcpyAsync(&host, st, sizeof(State), hipMemcpyDeviceToHost, s), UMPA_HIP_E_LAUNCH, "integrate: reading the state");
            HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "integrate: the solve");
        }
        iters[k] = host.iters; resid[k] = host.resid; status[k] = host.status;
        if (!dev_io) HIPOK(hipMemcpy(phi + (size_t)k * n, hphi, (size_t)n * 8, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "integrate: download");
    }
    return 0;
}
