/*
 * umpa_smooth.h -- regularised shift search: path aggregation over a cost volume (libumpa_smooth.so, gfx950).
 *
 * Every matcher of libumpa_hip.so and libumpa_grid.so decides each pixel on its own.  This library is the spatially
 * regularised consumer of the cost volume umpa_grid_cost_volume writes (semi-global matching, as stereo and optical-flow
 * packages ship it): the costs are aggregated along up to 8 path directions under a truncated-linear smoothness penalty,
 * then the minimum is taken per pixel.  It works on a plain volume and never sees a model.  The operation is DEFINED
 * here, expression by expression; tests/smooth_expect.py restates it in numpy and the two are EQUAL, bit for bit: it is
 * made of fp64 additions, subtractions and comparisons only.  No CPU fallback.
 *
 * INPUT.  cost[U * U][N0][N1], float64, U odd, 3 <= U <= 15 (U = 2 max_shift - 1: max_shift 2 .. 8).  Label
 * l = a U + b stands for the shift (si, sj) = (a - (U - 1) / 2, b - (U - 1) / 2), si the row shift.
 *
 * CONDITIONING.  C'(p, l) = cost[l][p] if that is finite, else +INF (NaN, +Inf and -Inf alike).  A pixel p all of whose
 * labels are +INF is VOID.
 *
 * DIRECTIONS (row step, column step), bit d of `dirs` selects direction d:
 *     0 (0, +1)   1 (0, -1)   2 (+1, 0)   3 (-1, 0)   4 (+1, +1)   5 (+1, -1)   6 (-1, +1)   7 (-1, -1)
 * A path of direction r is a maximal straight line of pixels of the N0 x N1 region in that direction; it starts on the
 * border it enters through.  The predecessor q of p on its path is p - r; p is a path's first pixel where p - r lies
 * outside the region.
 *
 * RECURSION along a path, with min(x, y) = x < y ? x : y:
 *     p is a path's first pixel, or q is void:    L_r(p, l) = C'(p, l)
 *     p is void:                                  L_r(p, l) = 0                         (this rule comes first)
 *     otherwise, with m = min_l L_r(q, l) and h = L_r(q, .) as a U x U array h[a][b], swept IN PLACE in this order
 *         1.  b = 1 .. U - 1 ascending:    h[a][b] = min(h[a][b], h[a][b - 1] + lam)    for every a
 *         2.  b = U - 2 .. 0 descending:   h[a][b] = min(h[a][b], h[a][b + 1] + lam)    for every a
 *         3.  a = 1 .. U - 1 ascending:    h[a][b] = min(h[a][b], h[a - 1][b] + lam)    for every b
 *         4.  a = U - 2 .. 0 descending:   h[a][b] = min(h[a][b], h[a + 1][b] + lam)    for every b
 *     (the lower envelope of L_r(q, .) under the penalty lam (|d si| + |d sj|)),
 *                                                 L_r(p, l) = C'(p, l) + (min(h[l], m + trunc) - m)
 * in exactly that association.  Nothing is multiplied.  m is finite whenever q is not void, so no NaN arises; a label
 * whose C' is +INF has L_r = +INF.
 *
 * SUM.  H = L_0 + L_1,  V = ((((L_2 + L_3) + L_4) + L_5) + L_6) + L_7, directions that are not selected left out of
 * their group; total = H + V, or the one group that is not empty.  (The grouping lets the horizontal directions be
 * accumulated apart from the others, on a transposed copy.)
 *
 * SELECTION per pixel.  l* = the first label, in label order, whose total is strictly below that of every earlier one;
 *     shift[0] = si(l*), shift[1] = sj(l*);   smin = total(l*);   valid = 1;
 *     margin = min { total(l) : max(|si(l) - si(l*)|, |sj(l) - sj(l*)|) >= 2 } - smin,  +INF where no such label exists
 * (how far the best label of another basin lies above the minimum).  A void pixel gets shift (0, 0), smin = 0,
 * margin = 0, valid = 0.
 *
 * Nothing is atomic, the passes run in direction order on one stream and every (label, pixel) of an accumulator is
 * written by exactly one lane per pass: results are bit-identical from run to run and between host and device arrays.
 *
 * DEVICE MEMORY.  Beside the input volume and the results the call allocates a workspace of at most THREE volumes of
 * U * U * N0 * N1 doubles: the sum `total`, and, where direction 0 or 1 is selected, a transposed copy of the input and
 * the transposed sum H (umpa_smooth_workspace_bytes; one volume less where `total` is a device array of the caller).
 * Host arrays additionally take device copies of the input and of the results.  Where that exceeds the free device
 * memory the call fails with UMPA_HIP_E_UNSUPPORTED before anything is launched.
 *
 * Link libumpa_smooth.so and libumpa_hip.so.  Error text of every call here: umpa_smooth_last_error().
 */
#ifndef UMPA_SMOOTH_H
#define UMPA_SMOOTH_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMPA_SMOOTH_MIN_U 3
#define UMPA_SMOOTH_MAX_U 15
#define UMPA_SMOOTH_ALL_DIRS 0xFF

/* cost: U * U * N0 * N1 doubles (read).  shift: 2 * N0 * N1 ints; smin, margin: N0 * N1 doubles; valid: N0 * N1 ints;
 * total: U * U * N0 * N1 doubles; smin, margin, valid and total may each be NULL.  Host arrays by default; with
 * UMPA_HIP_F_DEVICE_IO they are device arrays on `device` and the kernels run on `stream`.  Either way the call returns
 * when the results are written.  No other flag.
 * Checked before any device is touched (UMPA_HIP_E_ARG): U even or outside 3 .. 15; N0 or N1 < 1; lam or trunc negative
 * or NaN (trunc = +INF is allowed: no truncation); dirs 0 or above 0xFF; a null cost or shift. */
int umpa_smooth_aggregate(const double *cost, int U, int N0, int N1, double lam, double trunc, int dirs,
                          int *shift, double *smin, double *margin, int *valid, double *total,
                          int device, int flags, void *stream);

/* The workspace of umpa_smooth_aggregate in bytes (see DEVICE MEMORY); -1 (and an error text) for U, N0, N1 or dirs
 * that umpa_smooth_aggregate refuses.  Needs no device. */
long long umpa_smooth_workspace_bytes(int U, int N0, int N1, int dirs);

const char *umpa_smooth_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_SMOOTH_H */
