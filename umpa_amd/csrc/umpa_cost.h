// umpa_cost.h -- the reference's cost function (UMPA/lib/Model.cpp:359-509 NoDF, :631-862 DF), each piece of its
// arithmetic that more than one kernel needs and that can be shared without changing a kernel's machine code
// (profiles/r06_cost_refactor.txt says what could not, and why), stated once.
#pragma once
#include "umpa_walk.h"

namespace umpa {

// Search-range status of a shift (Model.cpp:372-399 / :654-681; the flags are asymmetric in the reference; kept)
__device__ __forceinline__ int shift_status(int ms, int si, int sj)
{
    if (si <= -ms || si >= ms) return UMPA_ST_BOUND;
    if (sj <= -ms) return UMPA_ST_BOUND | UMPA_ST_DIM;
    if (sj >= ms) return UMPA_ST_BOUND | UMPA_ST_DIM | UMPA_ST_POSITIVE;
    return UMPA_ST_OK;
}

// A frame of H x W pixels does not contribute at the pixel whose frame coordinates are (li, lj) (Model.cpp:430-433 / :716-719)
__device__ __forceinline__ bool frame_misses(int H, int W, int li, int lj, int pad) { return li - pad < 0 || li + pad > H || lj - pad < 0 || lj + pad > W; }

// combine_weights (Utils.cpp:125-130), twice, and deliberately not the same number: pair_weight (the explicit window sums
// of eval_direct and match_staged, the first-principles check of everything else) has fast_rcp's full-precision
// reciprocal; pair_weight_fast (corr_masked, which spends its time here) ONE Newton step, relative error ~1e-14 of a weight
// that enters every sum linearly: a perturbation of the window, not of a cancellation.  Its caller passes (mask under b,
// mask under a): a + b rounds in that order.
__device__ __forceinline__ double pair_weight(double a, double b) { return a * b * fast_rcp(a + b + 1e-8); }
__device__ __forceinline__ double pair_weight_fast(double a, double b)
{
    const double d = a + b + 1e-8;
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    return a * b * r;
}

// The closed-form solve (Model.cpp:849-858 DF, :502-505 otherwise) for the table lookups of the tiled path: one reciprocal
// instead of the reference's three divisions by the determinant (those: eval_direct, match_staged, corr_masked_tile),
// `rwt` = 1 / wt (1-ulp level differences; the bar is 1e-5); `fit.v` carries K, replay_walk divides by T once at the end.
// No implicit contraction here (a * b + c stays two roundings unless written as fma()): left to the compiler, inlined
// copies were fused differently and answered T an ulp apart on 27 k pixels (round 4).  The pragma lives in the helper.
template <int KIND>
__device__ __forceinline__ void solve_rcp(double t1, double t2, double t3, double t4, double t5, double t6, double rwt,
                                          double& cost, Fit& fit)
{
#pragma clang fp contract(off)
    if (KIND == 1) {
        const double rdet = fast_rcp(t2 * t3 - t6 * t6);
        const double K = (t2 * t5 - t4 * t6) * rdet;
        const double beta = (t3 * t4 - t5 * t6) * rdet;
        fit.t = beta + K;
        fit.v = K;
        cost = (t1 + beta * beta * t2 + K * K * t3 - 2 * beta * t4 - 2 * K * t5 + 2 * beta * K * t6) * rwt;
    } else {
        fit.t = t5 / t3;                                 // Model.cpp:502-505
        fit.v = 0.0;
        cost = (t1 - t5 * fit.t) * rwt;
    }
}

} // namespace umpa
