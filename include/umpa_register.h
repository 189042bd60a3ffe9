/*
 * umpa_register.h -- frame registration over a bounded box of shifts (libumpa_register.so, gfx950).
 *
 * The reference's registration utilities (UMPA/align.py: shift_dist, shift_best, get_diff_pos, find_sam_shift,
 * get_new_sam_pos) all rest on one distance: for two frames a, b of H x W pixels, a weight plane w and every relative
 * shift r,
 *
 *     D(r) = sum_x w(x) * (a(x) - alpha(r) * b(x - r))^2        with the scale alpha(r) that minimises it.
 *
 * The reference evaluates it for all H * W periodic shifts with three whole-frame FFTs.  The shifts that matter are motor
 * errors and drift of a few pixels, and over a bounded box D is a windowed reduction; the operation is therefore DEFINED
 * here, on the box, and this library evaluates it on the GPU.  No CPU fallback.
 *
 * THE OPERATION.  K pairs of frames (a_k, b_k), float64, float32 or uint16, converted to double first (exact); either K
 * frames a_k or one frame a shared by all pairs (UMPA_REGISTER_F_SHARED_A); an optional weight plane w of doubles, finite
 * and >= 0, per pair or shared (UMPA_REGISTER_F_SHARED_W), w = 1 when omitted.  Half-widths S0, S1 give the box of shifts
 * r = (ri, rj), ri = -S0 .. S0, rj = -S1 .. S1, i.e. U0 x U1 shifts with U = 2 S + 1.  Three planes of doubles [K, U0, U1],
 * the entry of r at [ri + S0, rj + S1]:
 *
 *     P(r) = sum_x w(x) a(x) b_r(x)        Q(r) = sum_x w(x) b_r(x)^2        A(r) = sum_x w(x) a(x)^2
 *
 *   UMPA_REGISTER_WRAP     b_r(x) = b((x0 - ri) mod H, (x1 - rj) mod W), the sum over every pixel x of the frame: the
 *                          reference's periodic convention.
 *   UMPA_REGISTER_OVERLAP  the sum runs over those x whose source pixel x - r lies inside the frame.  It is evaluated as
 *                          the sum over every x with b and the indicator of the frame continued by zero, so a non-finite
 *                          a(x) or w(x) reaches every shift (0 * NaN = NaN).
 *
 * A term is formed as (w * a) * b, w * (b * b), ((w * a) * a) [* indicator], each product rounded once, and accumulated
 * with fused multiply-adds, tile by tile; the tiles' partial sums are added in index order by a second kernel.  No float
 * atomics, no in-launch flags: a result does not depend on scheduling and is bit-identical from run to run.  Against the
 * exact sums every result is within (n + 2) * 2^-53 * sum |terms| (n: the number of pixels summed), for any order.
 * In the unweighted periodic case Q = sum b^2 and A = sum a^2 do not depend on r: the tile kernel computes only P, the
 * two constants come from a separate reduction and fill their planes.
 *
 * A NaN or infinity in a frame poisons every sum it touches; in the periodic case that is every shift.  This is what the
 * definition says and it is not worked around.
 *
 * LIMITS.  1 <= U0 <= H, 1 <= U1 <= W, H * W < 2^31 (UMPA_HIP_E_ARG otherwise); S0, S1 <= UMPA_REGISTER_MAX_SHIFT
 * (UMPA_HIP_E_UNSUPPORTED): beyond that the b tile with its halo no longer fits the 64 KiB of LDS a workgroup uses, and a
 * box that large is a search, not a registration (the matching path of libumpa_hip.so does that).
 *
 * THE DISTANCE AND THE SUB-PIXEL FIT are host arithmetic on these planes (umpa_amd/register.py does it; a C caller can
 * restate it):
 *
 *     D(r) = A(r) - P(r)^2 / (Q(r) + eps)        alpha(r) = P(r) / (Q(r) + eps)
 *
 * with eps = 1e-10 when weights are given or the boundary is OVERLAP and eps = 0 in the unweighted periodic case (the two
 * branches of the reference's formula).  The integer minimum is the first strict minimum of D over the box, rows first.
 * If it lies on the border of the box it is returned as it is (widen the box).  Otherwise, with z[u, v] = D at the
 * minimum + (u, v), u, v = -1, 0, 1, the least-squares paraboloid c0 + c1 u + c2 v + c3 u^2 + c4 v^2 + c5 u v is
 *
 *     c1 = sum u z / 6    c2 = sum v z / 6    c5 = sum u v z / 4
 *     c3 = sum (u^2 - 2/3) z / 2              c4 = sum (v^2 - 2/3) z / 2        c0 = sum z / 9 - 2 (c3 + c4) / 3
 *
 * and, if c3 > 0, c4 > 0 and 4 c3 c4 - c5^2 > 0, its optimum (u*, v*) solves [2 c3, c5; c5, 2 c4] (u*, v*)' = -(c1, c2)',
 * with the value c0 + (c1 u* + c2 v*) / 2.  If the paraboloid is not a minimum, the two parabolas through the centre
 * column z[., 0] and the centre row z[0, .] give u* and v* separately (u* = -(z[1,0] - z[-1,0]) / (2 (z[1,0] + z[-1,0]
 * - 2 z[0,0])), 0 where the denominator is not positive), and the value is the larger of the two parabolas' minima.
 *
 * Link libumpa_register.so and libumpa_hip.so.  Error text of every call here: umpa_register_last_error().
 */
#ifndef UMPA_REGISTER_H
#define UMPA_REGISTER_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMPA_REGISTER_WRAP    0
#define UMPA_REGISTER_OVERLAP 1

#define UMPA_REGISTER_MAX_SHIFT 32

/* flags beside UMPA_HIP_F_DEVICE_IO */
#define UMPA_REGISTER_F_SHARED_A 256   /* `a` is one frame, used by all K pairs (otherwise K frames) */
#define UMPA_REGISTER_F_SHARED_W 512   /* `w` is one plane, used by all K pairs (otherwise K planes) */

/* a, b: contiguous [K, H, W] (a: [H, W] with F_SHARED_A) of dtype 0 float64, 1 float32, 2 uint16 (umpa_hip_stage_sample's
 * codes); w: NULL or contiguous doubles [K, H, W] ([H, W] with F_SHARED_W); P, Q, A: [K, 2 S0 + 1, 2 S1 + 1] doubles.
 * Host arrays by default.  With UMPA_HIP_F_DEVICE_IO every array is a device array on `device` and the kernels run on
 * `stream`; weights are then not checked.  Either way the call returns when P, Q and A are written (it owns scratch
 * memory on the device that it gives back before it returns).  K = 0 is legal and does nothing. */
int umpa_register_sums(const void *a, const void *b, const double *w, int dtype, int K, int H, int W,
                       int S0, int S1, int boundary, double *P, double *Q, double *A,
                       int device, int flags, void *stream);

const char *umpa_register_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_REGISTER_H */
