// umpa_widen_kernels.h -- window widening (include/umpa_grid.h has the definition): the B x B box sum, B = 2b + 1, of the
// chunk's shift table and of the map planes, into workspace of libumpa_grid.so.  The consumer kernels then run on the
// pooled planes as they are.
//
//   widen_table_kernel<HB, STRIP>  the table: U^2 planes read once in either raw layout (widen_src, umpa_widen_geom.h),
//                                  written once in the plain layout;
//   widen_map_kernel<HB, PAIR>     a stack of H x W map planes of doubles (SamSq, RefSq) or, PAIR, of 16-byte frame pairs
//                                  (WS, MR: both frames of a pair plane at once);
//   widen_carry_kernel             the chunk's last 2b raw rows into the carry buffer.
//
// One marching routine serves both filters (widen_march): a wave owns 64 columns and goes down the rows.  Per raw row each
// lane loads one element (and the first 2b lanes the right halo) into an LDS segment, forms its horizontal sum left to
// right from the segment, and pushes it into a ring of the last B horizontal sums held in registers; every output row
// re-adds the ring top to bottom and scales by 1 / B^2.  No running sums: every output is the defined sum in the defined
// order, whichever wave, segment or chunk forms it.  Streaming: every element is loaded (almost) once and stored once,
// 8 or 16 bytes per lane, consecutive lanes on consecutive elements; no atomics, nothing across workgroups.
#pragma once
#include "umpa_tiled.h"
#include "umpa_widen_geom.h"
#include <type_traits>

namespace umpa {

#define UMPA_WIDEN_SEG 64     // output rows per workgroup: 2b of 64 + 2b raw rows are read twice (b = 4: 11 %)

// Output rows [ra, rb) of the wave's 64 columns (this lane: column c): load(row, col) gives raw element (row, col) for
// col in [clo, chi), rows ra - HB .. rb - 1 + HB; store(row, v) takes the lane's pooled element.  `seg`: 2 x 80 elements of LDS.
template <int HB, class T, class Load, class Store>
__device__ __forceinline__ void widen_march(int ra, int rb, int c, int clo, int chi, T* seg, Load load, Store store)
{
#pragma clang fp contract(off)
    constexpr int B = 2 * HB + 1;
    const double rB = 1.0 / (double)(B * B);
    const int lane = threadIdx.x;
    T ring[B];
#pragma unroll
    for (int k = 0; k < B; k++) ring[k] = T{};
    for (int rr = ra - HB; rr < rb + HB; rr++) {
        T* s = seg + ((rr - ra + HB) & 1) * 80;
        const int cl = c - HB, cr = c - HB + 64;
        s[lane] = (cl >= clo && cl < chi) ? load(rr, cl) : T{};
        if (lane < 2 * HB) s[64 + lane] = (cr >= clo && cr < chi) ? load(rr, cr) : T{};
        __syncthreads();
        T h = s[lane];                                               // H(r, c): left to right
#pragma unroll
        for (int k = 1; k < B; k++) h = h + s[lane + k];
#pragma unroll
        for (int k = 0; k < B - 1; k++) ring[k] = ring[k + 1];
        ring[B - 1] = h;
        if (rr - HB >= ra) {
            T v = ring[0];                                           // V(r, c): top to bottom
#pragma unroll
            for (int k = 1; k < B; k++) v = v + ring[k];
            store(rr - HB, v * rB);
        }
    }
}

// grid (column blocks of 64, U^2 planes, segments of UMPA_WIDEN_SEG pooled rows); 64 threads
template <int HB, bool STRIP>
__global__ void __launch_bounds__(64)
widen_table_kernel(const double* table, const double* carry, double* out, WidenGeom g)
{
    __shared__ double seg[2 * 80];
    const int c = blockIdx.x * 64 + threadIdx.x, slot = blockIdx.y;
    const int ra = g.p0 + blockIdx.z * UMPA_WIDEN_SEG, rb = min(g.p1, ra + UMPA_WIDEN_SEG);
    const int sa = max(ra, g.b), sb = min(rb, g.N0d - g.b);          // the rows of the segment whose block fits
    const bool col_in = c >= g.b && c < g.N1d - g.b;
    UMPA_GLOBAL double* __restrict__ o = gpw(out);
    for (int r = ra; r < rb; r++)
        if ((r < sa || r >= sb) && c < g.N1q) o[widen_dst(g, r, slot, c)] = __builtin_nan("");
    if (sa >= sb) return;
    const UMPA_GLOBAL double* __restrict__ t = gp(table);
    const UMPA_GLOBAL double* __restrict__ cy = gp(carry);
    WidenGeom gs = g;
    if (!STRIP) gs.strip_w = 0;                                      // (the layout test folds away)
    widen_march<HB, double>(sa, sb, c, 0, g.N1d, seg,
        [&](int row, int col) { bool in_carry; const size_t at = widen_src(gs, row, slot, col, in_carry); return in_carry ? cy[at] : t[at]; },
        [&](int row, double v) { if (c < g.N1q) o[widen_dst(g, row, slot, c)] = col_in ? v : __builtin_nan(""); });
}

struct WidenMapArgs {
    int W;                    // elements per row of a plane
    size_t plane;             // elements per plane
    int r0, r1, c0, c1;       // the pooled rectangle [r0, r1) x [c0, c1); raw rows r0 - b .. r1 - 1 + b, columns alike
};

// grid (column blocks of 64 from c0, segments of UMPA_WIDEN_SEG rows from r0, planes); 64 threads
template <int HB, bool PAIR>
__global__ void __launch_bounds__(64)
widen_map_kernel(const void* src, void* dst, WidenMapArgs a)
{
    using T = typename std::conditional<PAIR, map_pair_t, double>::type;
    __shared__ T seg[2 * 80];
    const int c = a.c0 + blockIdx.x * 64 + threadIdx.x;
    const int ra = a.r0 + blockIdx.y * UMPA_WIDEN_SEG, rb = min(a.r1, ra + UMPA_WIDEN_SEG);
    if (ra >= rb) return;
    const UMPA_GLOBAL T* __restrict__ s = gp((const T*)src) + (size_t)blockIdx.z * a.plane;
    UMPA_GLOBAL T* __restrict__ d = gpw((T*)dst) + (size_t)blockIdx.z * a.plane;
    widen_march<HB, T>(ra, rb, c, a.c0 - HB, a.c1 + HB, seg,
        [&](int row, int col) { return s[(size_t)row * a.W + col]; },
        [&](int row, T v) { if (c < a.c1) d[(size_t)row * a.W + c] = v; });
}

// run q of `run` doubles: from table[src_off + q * pitch ...] to carry[q * run ...] (widen_carry_copy)
__global__ void __launch_bounds__(256)
widen_carry_kernel(const double* table, double* carry, WidenCarryCopy cc)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cc.run) return;
    gpw(carry)[(size_t)blockIdx.y * cc.run + i] = gp(table)[cc.src_off + (size_t)blockIdx.y * cc.pitch + i];
}

} // namespace umpa
