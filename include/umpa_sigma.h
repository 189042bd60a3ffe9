/*
 * umpa_sigma.h -- per-pixel uncertainty of a matched shift: the covariance of (dy, dx) from the linearised model at the
 * solution, and a noise estimate from the residual (libumpa_sigma.so, gfx950).
 *
 * No matcher says how good a pixel's dx, dy are, and the result map f cannot: with the sub-pixel step on it is the value
 * of a smoothing spline surface, not a residual.  This library evaluates what every least-squares estimator offers: with
 * window weights that are NOT inverse variances, the SANDWICH covariance A^-1 B A^-1 of the estimated parameters, and the
 * residual after a linearised sub-pixel refit, divided by its expected value per unit noise variance.  It never sees a
 * model: it takes the two stacks, the window and an integer shift field.  The operation is DEFINED here, expression by
 * expression; tests/sigma_expect.py restates it in numpy.  The sums (MOMENTS) are held to a rounding bound, everything
 * after them (SOLVE) is made of fp64 + - * / in the order written here, without contraction, and the restatement fed the
 * same moments gives the same bits.  No square root is taken (the caller does), nothing is atomic.  No CPU fallback.
 *
 * INPUT.  sam[K][H][W], ref[K][H][W], float64.  win[(2 Nw + 1)^2], float64, row-major, 1 <= Nw <= 8, every entry finite
 * and >= 0, normalised: |sum win - 1| <= 1e-9 (the definition takes sum win = 1).  max_shift ms >= 1, pad = Nw + ms.  kind:
 * 0 plain, 1 dark-field.  A region start0, step0, N0, start1, step1, N1 of output pixels: pixel (xi, xj) has the output
 * coordinates (start0 + step0 xi, start1 + step1 xj) and the frame coordinates (ci, cj) = those + pad; required:
 * start >= 0, step >= 1, N >= 1 and start + step (N - 1) <= H - 2 pad - 1 (resp. W).  shift[2][N0][N1], int32: the row
 * shift si and the column shift sj of every pixel.  The sample window sits at the pixel, the reference window at the
 * pixel + shift (the matchers' default coordinate mode).
 *
 * PIXEL GUARD.  A pixel with si or sj outside -(ms - 1) .. ms - 1 (UMPA_SIGMA_SKIP is such a value) is skipped before any
 * address is formed: valid = 0, every output of the pixel NaN.  Within the guard every read below lies inside the frames.
 *
 * FIELDS per frame k and window tap x = (di, dj), di, dj = -Nw .. Nw, row-major:
 *     a   = sam[k][ci + di][cj + dj]                r = ref[k][ci + si + di][cj + sj + dj]
 *     g_i = 0.5 * (r one row below - r one row above)            g_j = 0.5 * (r one column right - r one column left)
 *     w   = win[x]      v = w * w      u = (u_0, u_1, u_2) = (g_i, g_j, r)      sv = sum_x v, summed in tap order
 *
 * MOMENTS, [P][N0][N1] planes, P = 16 (plain) or 34 (dark-field), sum_x over the taps, sum_k over the frames:
 *      0 ..  5   S_pq  = sum_k sum_x (w u_p) u_q        (p, q) = 00 01 02 11 12 22
 *      6 .. 11   V_pq  = sum_k sum_x (v u_p) u_q        same order
 *     12 .. 14   P_p   = sum_k sum_x (w a) u_p          p = 0 1 2
 *     15         Q     = sum_k sum_x (w a) a
 *   dark-field only, with the per-frame sums m_p = sum_x w u_p, n_p = sum_x v u_p, m_a = sum_x w a:
 *     16 .. 21   MM_pq = sum_k m_p m_q                  (p, q) = 00 01 02 11 12 22
 *     22 .. 30   NM_pq = sum_k n_p m_q                  (p, q) = 00 01 02 10 11 12 20 21 22
 *     31 .. 33   AM_p  = sum_k m_a m_p                  p = 0 1 2
 * S, V, MM are symmetric: S_qp = S_pq.  ROUNDING BOUND of a double evaluation, u = 2^-53, T = (2 Nw + 1)^2:
 *     planes 0 .. 15:   (K T + 6) u sum |term|          (a term: at most 2 products, v = w w and the roundings of two
 *                                                        differences g, 5 in all; K T additions; 1 to spare)
 *     planes 16 .. 33:  (2 T + K + 8) u sum_k (sum_x |w' u_p|) (sum_x |w u_q|), w' = w, v or (AM) w a in place of w' u_p
 *                                                       (each factor: T additions and at most 3 roundings per term; the
 *                                                        product 1; K additions; 1 to spare)
 *
 * MODEL at the shift.  With t1 = Q, t3 = S_22, t5 = P_2 and, dark-field, t2 = t6 = MM_22, t4 = AM_2 (the sums t1 .. t6 of
 * the matchers' cost function; r-bar_k = m_2 of frame k):
 *     plain        a ~ T r                        T = t5 / t3
 *                  theta = (delta_i, delta_j, T)                 J = (T g_i, T g_j, r)
 *                  rss0 = t1 - t5 * T
 *     dark-field   a ~ beta r-bar_k + Kc r        det = t2 * t3 - t6 * t6
 *                  Kc = (t2 * t5 - t4 * t6) / det                beta = (t3 * t4 - t5 * t6) / det
 *                  theta = (delta_i, delta_j, beta, Kc)          J = (Kc g_i + beta m_0, Kc g_j + beta m_1, m_2, r)
 *                  rss0 = ((((t1 + (beta * beta) * t2) + (Kc * Kc) * t3) - (2 * beta) * t4) - (2 * Kc) * t5) + ((2 * beta) * Kc) * t6
 * e = a - model.  A = sum w J J', B = sum v J J', h = sum w J e, rss0 = sum w e e, all polynomials in the moments:
 *     plain (n = 3), p, q in {0, 1}, TT = T * T:
 *         A_pq = TT * S_pq       A_p2 = T * S_p2       A_22 = S_22        B likewise from V
 *         h_p  = T * (P_p - T * S_p2)                  h_2  = P_2 - T * S_22
 *     dark-field (n = 4), p, q in {0, 1}, KK = Kc * Kc, c = (2 * Kc) * beta + beta * beta, bb = (beta * beta) * sv, kb = Kc * beta:
 *         A_pq = KK * S_pq + c * MM_pq                 A_p2 = (Kc + beta) * MM_p2        A_p3 = Kc * S_p2 + beta * MM_p2
 *         A_22 = MM_22        A_23 = MM_22             A_33 = S_22
 *         B_pq = (KK * V_pq + kb * (NM_pq + NM_qp)) + bb * MM_pq
 *         B_p2 = Kc * NM_p2 + (beta * sv) * MM_p2      B_p3 = Kc * V_p2 + beta * NM_2p
 *         B_22 = sv * MM_22   B_23 = NM_22             B_33 = V_22
 *         h_p  = Kc * ((P_p - beta * MM_p2) - Kc * S_p2) + beta * ((AM_p - beta * MM_p2) - Kc * MM_p2)
 *         h_2  = (AM_2 - beta * MM_22) - Kc * MM_22    h_3  = (P_2 - beta * MM_22) - Kc * S_22
 *
 * SOLVE.  A = L D L' without pivoting, column by column, j = 0 .. n - 1:
 *     D_j  = A_jj, then for k = 0 .. j - 1 ascending   D_j = D_j - (L_jk * L_jk) * D_k;     the pivot is BAD unless 0 < D_j < +INF
 *     for i = j + 1 .. n - 1:   t = A_ij, then for k = 0 .. j - 1 ascending   t = t - (L_ik * L_jk) * D_k;   L_ij = t / D_j
 * solve(b): y_i = b_i, then for k = 0 .. i - 1 ascending y_i = y_i - L_ik * y_k   (i ascending);   z_i = y_i / D_i;
 *           x_i = z_i, then for k = i + 1 .. n - 1 ascending x_i = x_i - L_ki * x_k   (i descending).
 *     X_q = solve(column q of B), q = 0 .. n - 1;          tr  = ((X_0[0] + X_1[1]) + X_2[2]) (+ X_3[3])
 *     Y0 = solve((X_0[0], X_1[0], ..)), Y1 = solve((X_0[1], X_1[1], ..))   (rows 0 and 1 of A^-1 B: C = A^-1 (A^-1 B)')
 *     d = solve(h);      hd = ((h_0 * d_0 + h_1 * d_1) + h_2 * d_2) (+ h_3 * d_3);      rr = rss0 - hd
 *     dof = K - tr;      rss = rr > 0 ? rr : 0;      s2 = rss / dof
 *
 * OUTPUT per pixel: unit[3][N0][N1] = (Y0[0], Y1[1], Y1[0]) = (C_00, C_11, C_01), the covariance of (dy, dx) per unit noise
 * variance; s2; dof; valid (int32).  valid = 1 iff no pivot is bad, dof > 0 and C_00, C_11, C_01, rr, dof, s2 are all finite;
 * otherwise valid = 0 and unit, s2, dof are NaN.  (A constant reference has g = 0: the first pivot is 0.)
 *
 * Link libumpa_sigma.so and libumpa_hip.so.  Error text of every call here: umpa_sigma_last_error().
 */
#ifndef UMPA_SIGMA_H
#define UMPA_SIGMA_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMPA_SIGMA_MAX_NW 8
#define UMPA_SIGMA_PLANES_PLAIN 16
#define UMPA_SIGMA_PLANES_DF 34
#define UMPA_SIGMA_SKIP (-2147483647 - 1)

/* sam, ref: K * H * W doubles (read).  win: (2 Nw + 1)^2 doubles, ALWAYS a host array.  shift: 2 * N0 * N1 ints (read).
 * moments: P * N0 * N1 doubles or NULL; unit: 3 * N0 * N1 doubles; s2, dof: N0 * N1 doubles; valid: N0 * N1 ints.
 * Host arrays by default; with UMPA_HIP_F_DEVICE_IO sam, ref, shift and the outputs are device arrays on `device` and the
 * kernel runs on `stream`.  Either way the call returns when the results are written.  No other flag.
 * Checked before any device is touched (UMPA_HIP_E_ARG): a null sam, ref, win, shift, unit, s2, dof or valid; K < 1; kind
 * not 0 or 1; Nw outside 1 .. 8; max_shift < 1; frames smaller than 2 pad + 1; a window that is not finite, non-negative
 * and normalised; a region outside the rule above; another flag. */
int umpa_sigma_region(const double *sam, const double *ref, int K, int H, int W, const double *win, int Nw, int max_shift,
                      int kind, int start0, int step0, int N0, int start1, int step1, int N1, const int *shift,
                      double *moments, double *unit, double *s2, double *dof, int *valid,
                      int device, int flags, void *stream);

/* The SOLVE stage alone on moments the caller supplies: moments[P][n] -> unit[3][n], s2[n], dof[n], valid[n]; sv as
 * defined above (not used by kind 0).  Arrays and flags as above.  UMPA_HIP_E_ARG: a null array, kind not 0 or 1, K < 1,
 * n < 1, sv not finite and >= 0, another flag. */
int umpa_sigma_solve(const double *moments, int kind, int K, long long n, double sv,
                     double *unit, double *s2, double *dof, int *valid, int device, int flags, void *stream);

const char *umpa_sigma_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_SIGMA_H */
