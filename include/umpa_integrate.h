/*
 * umpa_integrate.h -- weighted least-squares phase integration (libumpa_integrate.so, gfx950).
 *
 * The maps dx, dy of a match are the two components of the DIFFERENTIAL phase; the image is the phase Phi with
 * dPhi/dx ~ dx, dPhi/dy ~ dy.  This library integrates them with per-pixel weights, so that failed pixels (err == 0),
 * strong absorbers and dead detector areas are ignored instead of streaking across the image as they do with the Fourier
 * one-liner.  The operation is DEFINED here; tests/integrate_expect.py restates it in numpy.  No CPU fallback.
 *
 * INPUTS.  gx, gy: [H, W] doubles, the gradient along the columns (j) and along the rows (i), in units of Phi per pixel;
 * w: optional [H, W] doubles, finite and >= 0; H, W >= 2, H * W < 2^31.  The weight of a pixel is
 *
 *     w0 = (w > 0) ? w : 0                                  with w
 *     w0 = (gx and gy both finite) ? 1 : 0                  without w
 *
 * and the gradients of a pixel with w0 = 0 may be anything, NaN included.
 *
 * EDGES.  One unknown per pixel.  The edge between horizontal neighbours p = (i, j), q = (i, j + 1) has the weight
 * min(w0[p], w0[q]) and the datum 0.5 * (gx[p] + gx[q]); vertical edges likewise with gy.  Seen from a pixel, its four
 * edges are wl, wr, wu, wd (left, right, up: i - 1, down: i + 1), 0 where the neighbour is outside the grid, and
 *
 *     d  = ((wl + wr) + wu) + wd
 *     tl = (wl > 0) ? wl * (0.5 * (gx[i, j - 1] + gx[i, j])) : 0        tr = (wr > 0) ? wr * (0.5 * (gx[i, j] + gx[i, j + 1])) : 0
 *     tu = (wu > 0) ? wu * (0.5 * (gy[i - 1, j] + gy[i, j])) : 0        td = (wd > 0) ? wd * (0.5 * (gy[i, j] + gy[i + 1, j])) : 0
 *     b  = ((tl - tr) + tu) - td
 *     (L x)[p] = ((wl * (x - xl) + wr * (x - xr)) + wu * (x - xu)) + wd * (x - xd)
 *
 * where a neighbour outside the grid stands for the pixel's own value (its term is 0 * 0).  A datum of a weight-0 edge is
 * dropped by the select, never multiplied: a NaN at a weight-0 pixel reaches no output.
 *
 * THE PROBLEM.  Minimise sum over the edges of w_e (Phi_q - Phi_p - e)^2.  Its normal equations are L Phi = b with L the
 * weighted graph Laplacian above.  L is singular: every connected component of the positive-weight graph is determined up
 * to its own constant; the system is consistent.
 *
 * THE SOLVER.  Conjugate gradients from x = 0, preconditioned by one symmetric geometric multigrid V-cycle z = M r.
 *   Coarse grid     vertex-centred, the coarse node I at the fine node 2 I: Hc = (H + 1) / 2, Wc = (W + 1) / 2 (integer division).
 *   Prolongation P  bilinear, one axis after the other.  Along an axis of n nodes: v[2 I] = e[I]; v[2 I + 1] =
 *                   0.5 * (e[I] + e[I + 1]), or e[I] where I + 1 is no coarse node (the last node of an even axis).  First
 *                   along the rows (j) for the coarse rows I and I + 1, then along the columns (i).
 *   Restriction P'  unscaled.  With the 1-D weights of the fine nodes 2 I - 1, 2 I, 2 I + 1 on the coarse node I, (pm, p0,
 *                   pp) = (0.5 or 0 for I = 0, 1, 0.5 / 1 (last node of an even axis) / 0 (no such node)), and values
 *                   outside the grid 0:  s_a = (bm * r[2I + a, 2J - 1] + b0 * r[2I + a, 2J]) + bp * r[2I + a, 2J + 1] for
 *                   a = -1, 0, 1, then (P' r)[I, J] = (am * s_-1 + a0 * s_0) + ap * s_1.
 *   Coarse weights  w_c = (P' w0) / (P' 1), the two restrictions as above: the P-weighted mean of the pixel weights.  The
 *                   coarse operator is the same 5-point construction from w_c; with R = P' it keeps the graph Laplacian at
 *                   unit scale in two dimensions, so no h^2 factor appears.
 *   Smoother        damped Jacobi, x <- (d > 0) ? x + OMEGA * ((b - L x) / d) : x, OMEGA = 0.8; from zero it is
 *                   x = (d > 0) ? OMEGA * (b / d) : 0.  NU = 2 sweeps before (the first from zero) and 2 after.
 *   V-cycle         smooth; restrict r_c = P' (b - L x); z_c = V-cycle(r_c) on the next level; x <- x + P z_c; smooth.
 *                   Coarsening stops at the first level with min(H, W) <= 4; that level does 30 sweeps (the first from zero).
 * All counts are fixed: M is a fixed symmetric linear operator.  It contains no reduction, so with the expressions above
 * (fp64, no contraction) every stage of it has exactly one bit pattern.
 *
 * STOPPING.  On the TRUE residual: when the recursively updated residual reaches |r|_2 <= tol * |b|_2, r = b - L x is
 * recomputed; if that passes the solve stops, otherwise it continues from it with the direction reset to the new
 * preconditioned residual.  b = 0 returns zeros after 0 iterations.  A non-finite or non-positive p' L p, or a non-finite
 * norm, ends the solve with UMPA_INTEGRATE_BREAKDOWN.
 *
 * OUTPUT.  Phi minus its mean over the pixels with d > 0; pixels with d = 0 (no positive-weight edge) receive `fill`.
 * The gauge is ONE global mean: components other than the largest keep an arbitrary constant against it.  Per map also
 * the iteration count, the true relative residual |b - L x|_2 / |b|_2 of the returned map (0 for b = 0) and a status.
 *
 * REDUCTIONS.  The dots of CG, the norms and the gauge mean are two-stage sums with a partition that depends on H * W
 * only: a workgroup adds its 256 products in a fixed tree and stores the sum, a single workgroup adds those partial sums
 * (a fixed stride per lane, then the same tree) and derives alpha, beta and the flags from them on the device.  Plain
 * stores, no atomics: results are bit-identical from run to run and between host and device arrays, and every sum lies
 * within (n + 2) * 2^-53 * sum |terms| of the exact one (the rule of umpa_register.h).  The host reads the flags back
 * every UMPA_INTEGRATE_CHECK_EVERY iterations; the kernels enqueued after the iteration that met the criterion see the
 * flag on the device and do nothing, so the iterate and the count do not depend on when the host looks.
 *
 * Link libumpa_integrate.so and libumpa_hip.so.  Error text of every call here: umpa_integrate_last_error().
 */
#ifndef UMPA_INTEGRATE_H
#define UMPA_INTEGRATE_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMPA_INTEGRATE_CONVERGED 0
#define UMPA_INTEGRATE_MAXITER   1
#define UMPA_INTEGRATE_BREAKDOWN 2

#define UMPA_INTEGRATE_CHECK_EVERY 8

/* flags beside UMPA_HIP_F_DEVICE_IO */
#define UMPA_INTEGRATE_F_NO_TAIL 256    /* every level of the V-cycle by kernel launches (otherwise the levels that fit
                                           the LDS of one workgroup run in one kernel); the results are bit-identical */
#define UMPA_INTEGRATE_F_JACOBI  512    /* z = (d > 0) ? r / d : 0 instead of the V-cycle: the baseline preconditioner */
#define UMPA_INTEGRATE_F_DEBUG   1024   /* solve: phi receives b and nothing is iterated; vcycle: z receives d */

/* gx, gy, phi: contiguous [K, H, W] doubles; w: NULL or [K, H, W]; iters, status: K ints; resid: K doubles.  K independent
 * maps.  Host arrays by default (weights are then checked to be finite and >= 0).  With UMPA_HIP_F_DEVICE_IO gx, gy, w
 * and phi are device arrays on `device` and the kernels run on `stream`; iters, resid and status are host arrays always.  Either way the call
 * returns when the outputs are written; it allocates its workspace on the device and frees it before it returns.
 * tol >= 0, maxiter >= 0.  K = 0 is legal and does nothing. */
int umpa_integrate_solve(const double *gx, const double *gy, const double *w, int K, int H, int W,
                         double tol, int maxiter, double fill, double *phi, int *iters, double *resid, int *status,
                         int device, int flags, void *stream);

/* The preconditioner alone: z = M r on the hierarchy of the weights w ([H, W], NULL: all 1). */
int umpa_integrate_vcycle(const double *w, const double *r, double *z, int H, int W, int device, int flags, void *stream);

const char *umpa_integrate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_INTEGRATE_H */
