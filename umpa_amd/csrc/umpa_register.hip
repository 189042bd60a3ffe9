// umpa_register.hip -- libumpa_register.so: frame registration over a bounded box of shifts (include/umpa_register.h).
// gfx950 only.
//
// A fourth library beside libumpa_hip.so, libumpa_grid.so and libumpa_unwarp.so, for the same reason those two have their
// own: the other libraries' kernel sets stay what they are.  Three kernel families:
//   register_tile_kernel<T, WEIGHTED, BOUNDARY>   the windowed reduction, one tile of one pair per workgroup
//   register_norm_kernel<T>                       sum of squares of a frame (the constants of the unweighted periodic case)
//   register_reduce_kernel                        adds the tiles' partial sums in index order
// The operation is defined in the public header; the sub-pixel fit is host arithmetic (umpa_amd/register.py).
// No CPU fallback.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

#include "../../include/umpa_register.h"
#include "umpa_host.h"

#pragma clang fp contract(off)

namespace umpa {

// The shapes of one call, fixed on the host (geometry() below) and the same for every pair of the call.
struct RegGeom {
    int H, W, S0, S1, U0, U1;
    int NG, QN;              // groups of 4 adjacent column shifts per row shift; lanes' work items, U0 * NG
    int TH, TW, ntx, nty;    // tile of pixels, tiles per frame
    int HB, WB, pitch;       // the b tile with its halo: TH + 2 S0 rows of TW + 2 S1 + 3 columns, row pitch (odd)
    int tt, nteams, passes;  // threads of a team (a multiple of 64), teams per workgroup, work items per thread
};

// MAPPING.  A workgroup of 256 threads takes one TH x TW tile of one pair.  It stages in LDS the tile of w a (and w, and
// w a a), and the tile of b with a halo of S0 rows above and below, S1 + 3 columns left and S1 right, the wrap or the clip
// folded into that staging.  A lane owns a row shift ri and FOUR adjacent column shifts rj = r0 .. r0 + 3 and runs over
// pixels: along a tile row it keeps the last four b values in registers, so each step reads ONE new b value (addresses
// 4 doubles apart across the lanes of one ri, a row pitch apart across ri) and one a value (one address per wave: a
// broadcast) for FOUR fused multiply-adds per sum.  Nothing is ever added across lanes.
// The U0 * NG work items of a box fill QN lanes; where that is at most 128 the workgroup splits into 256 / tt teams that
// take the tile's rows in turn, each with its own slot of partial sums; where it is more than 256 a thread takes `passes`
// items one after the other.  Partial sums go to part[slot][plane][shift] with plain stores; register_reduce_kernel,
// launched after this one, adds the slots in index order.
template <class T, bool WEIGHTED, int BOUNDARY>
__global__ void __launch_bounds__(256)
register_tile_kernel(const T* __restrict__ a, const T* __restrict__ b, const double* __restrict__ w,
                     double* __restrict__ part, const RegGeom g)
{
    extern __shared__ double lds[];
    constexpr bool OVERLAP = BOUNDARY == UMPA_REGISTER_OVERLAP;
    constexpr bool FULL = WEIGHTED || OVERLAP;                 // Q and A are summed here (else: constants, not this kernel's)
    constexpr int NA = WEIGHTED ? 3 : (FULL ? 2 : 1);
    constexpr int NP = FULL ? 3 : 1;
    const int H = g.H, W = g.W, TW = g.TW, pitch = g.pitch, nA = g.TH * g.TW;
    double* bs = lds;                                          // [HB][pitch]
    double* as = bs + g.HB * pitch;                            // [NA][TH][TW]: w a | w | (w a) a    (unweighted: a | a a)
    double* mx = as + NA * nA;                                 // [WB], OVERLAP: 1 where the halo column is inside the frame
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / g.ntx, tx = blockIdx.x - ty * g.ntx;
    const int y0 = ty * g.TH, x0 = tx * TW;
    const int th = min(g.TH, H - y0), tw = min(TW, W - x0);

    for (int e = tid; e < g.HB * g.WB; e += 256) {
        const int yy = e / g.WB, xx = e - yy * g.WB;
        int sy = y0 - g.S0 + yy, sx = x0 - g.S1 - 3 + xx;
        double v;
        if (!OVERLAP) {
            sy %= H; if (sy < 0) sy += H;
            sx %= W; if (sx < 0) sx += W;
            v = (double)b[(size_t)sy * W + sx];
        } else {
            const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
            v = in ? (double)b[(size_t)sy * W + sx] : 0.0;
        }
        bs[yy * pitch + xx] = v;
    }
    for (int e = tid; e < nA; e += 256) {
        const int ly = e / TW, lx = e - ly * TW;
        const bool in = ly < th && lx < tw;
        const size_t idx = in ? (size_t)(y0 + ly) * W + (x0 + lx) : 0;
        const double av = in ? (double)a[idx] : 0.0;
        if (WEIGHTED) {
            const double wv = in ? w[idx] : 0.0;
            const double wa = wv * av;
            as[e] = wa; as[nA + e] = wv; as[2 * nA + e] = wa * av;
        } else {
            as[e] = av;
            if (FULL) as[nA + e] = av * av;
        }
    }
    if (OVERLAP)
        for (int xx = tid; xx < g.WB; xx += 256) {
            const int sx = x0 - g.S1 - 3 + xx;
            mx[xx] = (sx >= 0 && sx < W) ? 1.0 : 0.0;
        }
    __syncthreads();

    const int team = tid / g.tt, lt = tid - team * g.tt;
    if (team >= g.nteams) return;
    const int NS = g.U0 * g.U1;
    double* slot = part + (size_t)(blockIdx.x * g.nteams + team) * NP * NS;
    for (int pass = 0; pass < g.passes; pass++) {
        const int q = lt + pass * g.tt;
        if (q >= g.QN) break;
        const int ri_i = q / g.NG, gi = q - ri_i * g.NG;
        const int ri = ri_i - g.S0;
        const int c0 = 2 * g.S1 + 3 - 4 * gi;                  // halo column of pixel lx = 0 under rj = r0 = -S1 + 4 gi
        double p0 = 0, p1 = 0, p2 = 0, p3 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0, a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int ly = team; ly < th; ly += g.nteams) {
            const double* arow = as + ly * TW;
            const double* brow = bs + (ly - ri + g.S0) * pitch + c0;          // brow[lx - j]: b under rj = r0 + j
            const double* mrow = mx + c0;
            double b1 = brow[-1], b2 = brow[-2], b3 = brow[-3];
            double s1 = b1 * b1, s2 = b2 * b2, s3 = b3 * b3;
            double m1 = 0, m2 = 0, m3 = 0, my = 0;
            if (OVERLAP) {
                const int sy = y0 + ly - ri;
                my = (sy >= 0 && sy < H) ? 1.0 : 0.0;
                m1 = mrow[-1]; m2 = mrow[-2]; m3 = mrow[-3];
            }
#pragma unroll 4
            for (int lx = 0; lx < tw; lx++) {
                const double b0 = brow[lx];
                const double av = arow[lx];                                   // w a (unweighted: a)
                p0 = fma(av, b0, p0); p1 = fma(av, b1, p1); p2 = fma(av, b2, p2); p3 = fma(av, b3, p3);
                if (FULL) {
                    const double s0 = b0 * b0;
                    if (WEIGHTED) {
                        const double wv = arow[nA + lx];
                        q0 = fma(wv, s0, q0); q1 = fma(wv, s1, q1); q2 = fma(wv, s2, q2); q3 = fma(wv, s3, q3);
                    } else {
                        q0 = q0 + s0; q1 = q1 + s1; q2 = q2 + s2; q3 = q3 + s3;
                    }
                    const double waa = arow[(NA - 1) * nA + lx];              // (w a) a (unweighted: a a)
                    if (OVERLAP) {
                        const double m0 = mrow[lx], t = waa * my;
                        a0 = fma(t, m0, a0); a1 = fma(t, m1, a1); a2 = fma(t, m2, a2); a3 = fma(t, m3, a3);
                        m3 = m2; m2 = m1; m1 = m0;
                    } else {
                        a0 = a0 + waa;                                        // periodic: the same for every shift
                    }
                    s3 = s2; s2 = s1; s1 = s0;
                }
                b3 = b2; b2 = b1; b1 = b0;
            }
        }
        if (FULL && !OVERLAP) { a1 = a0; a2 = a0; a3 = a0; }
        const double pv[4] = {p0, p1, p2, p3}, qv[4] = {q0, q1, q2, q3}, av4[4] = {a0, a1, a2, a3};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int rj_i = 4 * gi + j;
            if (rj_i < g.U1) {
                const int s = ri_i * g.U1 + rj_i;
                slot[s] = pv[j];
                if (FULL) { slot[NS + s] = qv[j]; slot[2 * NS + s] = av4[j]; }
            }
        }
    }
}

// Sum of squares of a frame in NORM_BLOCKS pieces: a thread takes every 256th pixel of its block's piece, thread 0 adds the
// 256 sums in index order (through LDS, after a barrier; no cross-lane operation), register_reduce_kernel adds the pieces.
constexpr int NORM_BLOCKS = 64;

template <class T>
__global__ void __launch_bounds__(256)
register_norm_kernel(const T* __restrict__ f, unsigned n, double* __restrict__ out)
{
    __shared__ double sums[256];
    const unsigned chunk = (n + NORM_BLOCKS - 1) / NORM_BLOCKS;
    const unsigned lo = min(n, blockIdx.x * chunk), hi = min(n, lo + chunk);
    double acc = 0.0;
    for (unsigned i = lo + threadIdx.x; i < hi; i += 256) {
        const double v = (double)f[i];
        acc = fma(v, v, acc);
    }
    sums[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; i++) t = t + sums[i];
        out[blockIdx.x] = t;
    }
}

// out[plane][shift] = the slots' partial sums added in index order.  With np == 1 (unweighted periodic) Q and A are
// filled with the two constants, the NORM_BLOCKS pieces of norm_b and norm_a added in index order.
__global__ void __launch_bounds__(256)
register_reduce_kernel(const double* __restrict__ part, int nslots, int np, int NS,
                       const double* __restrict__ norm_a, const double* __restrict__ norm_b,
                       double* __restrict__ P, double* __restrict__ Q, double* __restrict__ A)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= np * NS) return;
    const int plane = t / NS, s = t - plane * NS;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < nslots; k++) acc = acc + part[((size_t)k * np + plane) * NS + s];
    if (plane == 0) P[s] = acc; else if (plane == 1) Q[s] = acc; else A[s] = acc;
    if (np == 1) {
        double na = 0.0, nb = 0.0;
        for (int i = 0; i < NORM_BLOCKS; i++) { na = na + norm_a[i]; nb = nb + norm_b[i]; }
        Q[s] = nb; A[s] = na;
    }
}

} // namespace umpa

using namespace umpa;

#define UMPA_REGISTER_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr size_t LDS_BUDGET = 64 * 1024;

size_t lds_bytes(const RegGeom& g, bool weighted, bool overlap)
{
    const int na = weighted ? 3 : (overlap ? 2 : 1);
    return sizeof(double) * ((size_t)g.HB * g.pitch + (size_t)na * g.TH * g.TW + (overlap ? g.WB : 0));
}

// The largest tile whose images fit LDS_BUDGET: the halo (2 S0 rows, 2 S1 + 3 columns) is read again by every tile, so a
// larger tile reads less; wide tiles first, they keep the inner loop long.  The last shape fits every box the header
// admits (weighted overlap at (32, 32): 63960 bytes), so this fails only if UMPA_REGISTER_MAX_SHIFT is raised.
bool geometry(int H, int W, int S0, int S1, bool weighted, bool overlap, RegGeom& g)
{
    static const int shapes[][2] = {{32, 64}, {16, 64}, {16, 32}, {8, 32}};
    g.H = H; g.W = W; g.S0 = S0; g.S1 = S1; g.U0 = 2 * S0 + 1; g.U1 = 2 * S1 + 1;
    g.NG = (g.U1 + 3) / 4; g.QN = g.U0 * g.NG;
    g.passes = (g.QN + 255) / 256;
    g.tt = (((g.QN + g.passes - 1) / g.passes) + 63) / 64 * 64;
    g.nteams = 256 / g.tt;
    for (const auto& s : shapes) {
        g.TH = s[0]; g.TW = s[1];
        g.HB = g.TH + 2 * S0; g.WB = g.TW + 2 * S1 + 3; g.pitch = g.WB | 1;
        if (lds_bytes(g, weighted, overlap) <= LDS_BUDGET) {
            g.ntx = (W + g.TW - 1) / g.TW; g.nty = (H + g.TH - 1) / g.TH;
            return true;
        }
    }
    return false;
}

template <class T>
void launch_tile(const void* a, const void* b, const double* w, double* part, const RegGeom& g, bool overlap, size_t lds, hipStream_t s)
{
    const dim3 grid(g.ntx * g.nty), block(256);
    const T* ta = (const T*)a;
    const T* tb = (const T*)b;
    if (w) {
        if (overlap) hipLaunchKernelGGL((register_tile_kernel<T, true, UMPA_REGISTER_OVERLAP>), grid, block, lds, s, ta, tb, w, part, g);
        else hipLaunchKernelGGL((register_tile_kernel<T, true, UMPA_REGISTER_WRAP>), grid, block, lds, s, ta, tb, w, part, g);
    } else {
        if (overlap) hipLaunchKernelGGL((register_tile_kernel<T, false, UMPA_REGISTER_OVERLAP>), grid, block, lds, s, ta, tb, w, part, g);
        else hipLaunchKernelGGL((register_tile_kernel<T, false, UMPA_REGISTER_WRAP>), grid, block, lds, s, ta, tb, w, part, g);
    }
}

template <class T>
void launch_norm(const void* f, unsigned n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL((register_norm_kernel<T>), dim3(NORM_BLOCKS), dim3(256), 0, s, (const T*)f, n, out);
}

// One pair, every pointer a device pointer.  part: nslots * np * NS doubles; norms: 2 * NORM_BLOCKS doubles (a, then b).
hipError_t run_pair(const void* a, const void* b, const double* w, int dtype, const RegGeom& g, bool overlap, size_t lds,
                    double* part, double* norms, bool norm_a_done, double* P, double* Q, double* A, hipStream_t s)
{
    const bool full = w || overlap;
    const int np = full ? 3 : 1, NS = g.U0 * g.U1, nslots = g.ntx * g.nty * g.nteams;
    const unsigned n = (unsigned)g.H * (unsigned)g.W;
    if (dtype == 0) launch_tile<double>(a, b, w, part, g, overlap, lds, s);
    else if (dtype == 1) launch_tile<float>(a, b, w, part, g, overlap, lds, s);
    else launch_tile<unsigned short>(a, b, w, part, g, overlap, lds, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (!full) {
        for (int which = norm_a_done ? 1 : 0; which < 2; which++) {
            const void* f = which ? b : a;
            double* out = norms + which * NORM_BLOCKS;
            if (dtype == 0) launch_norm<double>(f, n, out, s);
            else if (dtype == 1) launch_norm<float>(f, n, out, s);
            else launch_norm<unsigned short>(f, n, out, s);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(register_reduce_kernel, dim3((np * NS + 255) / 256), dim3(256), 0, s,
                       (const double*)part, nslots, np, NS, (const double*)norms, (const double*)(norms + NORM_BLOCKS), P, Q, A);
    return hipGetLastError();
}

} // namespace

UMPA_REGISTER_API const char* umpa_register_last_error(void) { return g_err.c_str(); }

UMPA_REGISTER_API int umpa_register_sums(const void* a, const void* b, const double* w, int dtype, int K, int H, int W,
                                         int S0, int S1, int boundary, double* P, double* Q, double* A,
                                         int device, int flags, void* stream)
{
    if (!a || !b || !P || !Q || !A) return fail(UMPA_HIP_E_ARG, "register: null argument");
    if (dtype < 0 || dtype > 2) return fail(UMPA_HIP_E_ARG, "register: dtype %d: 0 float64, 1 float32, 2 uint16", dtype);
    if (K < 0) return fail(UMPA_HIP_E_ARG, "register: K = %d", K);
    if (flags & ~(UMPA_HIP_F_DEVICE_IO | UMPA_REGISTER_F_SHARED_A | UMPA_REGISTER_F_SHARED_W))
        return fail(UMPA_HIP_E_ARG, "register: sums takes UMPA_HIP_F_DEVICE_IO, UMPA_REGISTER_F_SHARED_A, UMPA_REGISTER_F_SHARED_W and no other flag");
    if (boundary != UMPA_REGISTER_WRAP && boundary != UMPA_REGISTER_OVERLAP)
        return fail(UMPA_HIP_E_ARG, "register: boundary %d (0 wrap, 1 overlap)", boundary);
    if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return fail(UMPA_HIP_E_ARG, "register: frames of %d x %d pixels (H * W must be in [1, 2^31))", H, W);
    if (S0 < 0 || S1 < 0) return fail(UMPA_HIP_E_ARG, "register: half-widths (%d, %d) of the box", S0, S1);
    if (S0 > UMPA_REGISTER_MAX_SHIFT || S1 > UMPA_REGISTER_MAX_SHIFT)
        return fail(UMPA_HIP_E_UNSUPPORTED, "register: half-widths (%d, %d) of the box: at most %d", S0, S1, UMPA_REGISTER_MAX_SHIFT);
    if (2 * S0 + 1 > H || 2 * S1 + 1 > W)
        return fail(UMPA_HIP_E_ARG, "register: a box of %d x %d shifts is wider than the frame of %d x %d pixels", 2 * S0 + 1, 2 * S1 + 1, H, W);
    const bool dev_io = flags & UMPA_HIP_F_DEVICE_IO, shared_a = flags & UMPA_REGISTER_F_SHARED_A, shared_w = flags & UMPA_REGISTER_F_SHARED_W;
    const bool overlap = boundary == UMPA_REGISTER_OVERLAP;
    const size_t n = (size_t)H * W;
    if (w && !dev_io) {
        const size_t nw = shared_w ? n : n * (size_t)K, i = bad_weight(w, nw);
        if (i < nw)
            return fail(UMPA_HIP_E_ARG, "register: weights must be finite and >= 0 (plane %d, pixel (%d, %d))", (int)(i / n), (int)(i % n / W), (int)(i % W));
    }
    RegGeom g;
    if (!geometry(H, W, S0, S1, w != nullptr, overlap, g))
        return fail(UMPA_HIP_E_UNSUPPORTED, "register: no tile of a box of (%d, %d) fits the LDS", S0, S1);
    const size_t lds = lds_bytes(g, w != nullptr, overlap);
    if (int rc = pick_device("register", device)) return rc;
    if (K == 0) return 0;

    const bool full = w || overlap;
    const int np = full ? 3 : 1, NS = g.U0 * g.U1, nslots = g.ntx * g.nty * g.nteams;
    const size_t esz = dtype_size(dtype);
    DeviceMem S;                                               // 0 part, 1 norms, 2 a, 3 b, 4 w, 5 P Q A
    HIPOK(S.alloc(0, (size_t)nslots * np * NS * sizeof(double)), UMPA_HIP_E_NOMEM, "register: device memory for the partial sums");
    HIPOK(S.alloc(1, 2 * NORM_BLOCKS * sizeof(double)), UMPA_HIP_E_NOMEM, "register: device memory");
    double* part = (double*)S.p[0];
    double* norms = (double*)S.p[1];
    const char* ca = (const char*)a;
    const char* cb = (const char*)b;
    if (dev_io) {
        hipStream_t s = (hipStream_t)stream;
        for (int k = 0; k < K; k++)
            HIPOK(run_pair(shared_a ? ca : ca + (size_t)k * n * esz, cb + (size_t)k * n * esz, w ? (shared_w ? w : w + (size_t)k * n) : nullptr,
                           dtype, g, overlap, lds, part, norms, shared_a && k > 0,
                           P + (size_t)k * NS, Q + (size_t)k * NS, A + (size_t)k * NS, s),
                  UMPA_HIP_E_LAUNCH, "register: launch of pair %d", k);
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "register");
        return 0;
    }
    // host arrays: device copies of one pair's arrays, pair after pair on the null stream
    const size_t bytes[4] = {n * esz, n * esz, w ? n * 8 : 0, (size_t)3 * NS * 8};
    for (int q = 0; q < 4; q++)
        if (bytes[q]) HIPOK(S.alloc(2 + q, bytes[q]), UMPA_HIP_E_NOMEM, "register: device memory for a pair");
    double* dout = (double*)S.p[5];
    for (int k = 0; k < K; k++) {
        if (!shared_a || k == 0) HIPOK(hipMemcpy(S.p[2], shared_a ? ca : ca + (size_t)k * n * esz, bytes[0], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "register: upload of pair %d", k);
        HIPOK(hipMemcpy(S.p[3], cb + (size_t)k * n * esz, bytes[1], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "register: upload of pair %d", k);
        if (w && (!shared_w || k == 0)) HIPOK(hipMemcpy(S.p[4], shared_w ? w : w + (size_t)k * n, bytes[2], hipMemcpyHostToDevice), UMPA_HIP_E_DEVICE, "register: upload of pair %d", k);
        HIPOK(run_pair(S.p[2], S.p[3], (const double*)S.p[4], dtype, g, overlap, lds, part, norms, shared_a && k > 0,
                       dout, dout + NS, dout + 2 * NS, nullptr), UMPA_HIP_E_LAUNCH, "register: launch of pair %d", k);
        HIPOK(hipMemcpy(P + (size_t)k * NS, dout, (size_t)NS * 8, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "register: pair %d", k);
        HIPOK(hipMemcpy(Q + (size_t)k * NS, dout + NS, (size_t)NS * 8, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "register: pair %d", k);
        HIPOK(hipMemcpy(A + (size_t)k * NS, dout + 2 * NS, (size_t)NS * 8, hipMemcpyDeviceToHost), UMPA_HIP_E_LAUNCH, "register: pair %d", k);
    }
    return 0;
}
