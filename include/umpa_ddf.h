/*
 * umpa_ddf.h -- directional dark-field search over blur-kernel candidates (libumpa_ddf.so, gfx950).
 *
 * The kernel dark-field model (UMPAModelDFKernel) describes the sample as the reference blurred by a 17 x 17 Gaussian
 * exp(-a i^2 - b i j - c j^2); (a, b, c) is an INPUT of that model.  Where (a, b, c) is the same for every pixel -- which
 * is what a candidate of a search is -- the blurred reference value a window asks for does not depend on which window asks,
 * so the model's cost is the plain model's (UMPAModelNoDF) cost on the reference stack blurred ONCE as a whole image.  This
 * library holds the two operations such a search needs beside the plain match of libumpa_hip.so: the whole-image blur and
 * the fold of one candidate's maps into the running best.  The operations are DEFINED here; tests/ddf_expect.py restates
 * them in numpy.  No CPU fallback.
 *
 * KERNEL.  For a candidate (a, b, c), finite with a > 0, c > 0 and 4 a c - b^2 > 0,
 *
 *     e[k][l] = exp(-a (k - 8)^2 - b (k - 8) (l - 8) - c (l - 8)^2)        k, l = 0 .. 16, k the row
 *     g[k][l] = e[k][l] / S,   S = the sum of e in the order k = 0 .. 16, l = 0 .. 16 (l fastest)
 *
 * in double on the HOST (the reference's CostArgsDFKernel constructor); the device never calls exp.  The exponent is
 * evaluated as written, from the left.
 *
 * BLUR.  For a frame `in` of H x W doubles, H >= 17 and W >= 17,
 *
 *     out[i][j] = sum_k sum_l g[k][l] * in[i + k - 8][j + l - 8]           for 8 <= i < H - 8 and 8 <= j < W - 8
 *     out[i][j] = in[i][j], bit for bit                                    for every other pixel
 *
 * Order and contraction of the sum are free; the contract is |out - exact| <= 291 * 2^-53 * sum_k sum_l g |in| (289 fused
 * multiply-adds in a chain, the rule of umpa_register.h).  Every tap is multiplied, also where g underflowed to 0: a NaN
 * in `in` reaches exactly the 17 x 17 outputs around it (and itself, where it is copied).  Nothing is added across lanes and
 * nothing is atomic: results are bit-identical from run to run and between host and device arrays.  `in` and `out` may not
 * alias.
 *
 * The relation to the models: UMPAModelDFKernel pads by max_shift + Nw + 8, UMPAModelNoDF by max_shift + Nw, so the
 * former's pixel (xi, xj) is the latter's pixel (xi + 8, xj + 8) and nothing that region reads comes within 8 pixels of the
 * frame edge: only the interior of the blur matters to a match.
 *
 * FOLD.  Candidate m's planes f, T, dx, dy (doubles) and err (ints), N pixels each, are folded into the running best:
 *
 *     m == 0:  index = (err_m == 1) ? 0 : -1;  best f, T, dx, dy = the candidate's
 *     m  > 0:  where err_m == 1 and (index < 0 or f_m < best f):  index = m;  best f, T, dx, dy = the candidate's
 *     always:  best err = (index >= 0) ? 1 : 0
 *
 * The comparison is a strict <: of equal costs the first stays, and a NaN cost never replaces anything.  A search over a
 * single candidate returns that candidate's match untouched.
 *
 * The fold ranks by whatever the caller passes as f, so f must be a COST.  The plain match's f is one with sub-pixel modes
 * -1 and 1 (the fitted minimum).  With sub_pixel_mode 0 it is the start offset 1 - ip of the reference, 0 or 1: a search in
 * that mode passes the cost at the candidate's integer minimum instead, the centre dbg_d[12] of the match's 5 x 5 memo
 * (umpa_amd/ddf.py does, and returns that cost as f).
 *
 * Link libumpa_ddf.so and libumpa_hip.so.  Error text of every call here: umpa_ddf_last_error().
 */
#ifndef UMPA_DDF_H
#define UMPA_DDF_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMPA_DDF_TAPS 17                /* the kernel is UMPA_DDF_TAPS x UMPA_DDF_TAPS */
#define UMPA_DDF_HALF 8
#define UMPA_DDF_MAX_FRAMES 32          /* frames of one launch; a longer stack takes several */

/* out[17 * k + l] = g[k][l].  Host arithmetic, needs no device.  UMPA_HIP_E_ARG for an inadmissible candidate. */
int umpa_ddf_kernel(double a, double b, double c, double *out);

/* in, out: K pointers to frames of H x W contiguous doubles each; kern: 289 doubles (any finite values; umpa_ddf_kernel
 * makes the Gaussian).  Host arrays by default; with UMPA_HIP_F_DEVICE_IO the frames are device arrays on `device` and the
 * kernel runs on `stream`.  Either way the call returns when `out` is written.  No other flag.  K = 0 does nothing. */
int umpa_ddf_blur(const double *const *in, double *const *out, int K, int H, int W, const double *kern,
                  int device, int flags, void *stream);

/* Planes of N pixels: the candidate's f, T, dx, dy, err (read) and the best's f, T, dx, dy, index, err (read and written;
 * for m == 0 only written).  Host arrays by default, device arrays on `device` and the kernel on `stream` with
 * UMPA_HIP_F_DEVICE_IO; the call returns when the planes are written.  m >= 0, 0 <= N. */
int umpa_ddf_fold(int m, long long N, const double *f, const double *T, const double *dx, const double *dy, const int *err,
                  double *best_f, double *best_T, double *best_dx, double *best_dy, int *index, int *best_err,
                  int device, int flags, void *stream);

const char *umpa_ddf_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_DDF_H */
