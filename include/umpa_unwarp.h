/*
 * umpa_unwarp.h -- detector distortion correction (libumpa_unwarp.so, gfx950).
 *
 * The reference's batch script resamples every raw frame through a calibrated distortion map before it flat-corrects and
 * matches it (UMPA/umpa_multi.py:127-130, "Do unwarp: slowest step by far!"); its `unwarp` module is not part of the
 * reference tree, so the operation is DEFINED here.  This library runs it on the GPU, stand-alone (umpa_unwarp_frames) or
 * fused into umpa_hip_stage_sample of a model of libumpa_hip.so (umpa_unwarp_attach), where it takes the place of the
 * flat-field kernel on the upload stream.  No CPU fallback.
 *
 * THE OPERATION.  An unwarp map belongs to a detector of H x W pixels: two float32 planes d0, d1 of shape [H, W] (row and
 * column displacement) and an interpolation kind.  It is a backward map: output pixel (i, j) reads the raw frame at
 *
 *     y = (double)i + (double)d0[i,j]          x = (double)j + (double)d1[i,j]
 *     i0 = floor(y)   fy = y - i0              j0 = floor(x)   fx = x - j0
 *
 * Raw samples (float64, float32 or uint16) are converted to double first (exact).  v(a, b) below is the raw sample at row
 * clamp(i0 + a, 0, H - 1), column clamp(j0 + b, 0, W - 1): taps that leave the frame read its edge pixel ("edge" is the only
 * border rule).  Every operation is an IEEE double operation, rounded once, in the order written; nothing is contracted
 * into a fused multiply-add.
 *
 *   UMPA_UNWARP_LINEAR   u = (1 - fy) * ((1 - fx) * v(0,0) + fx * v(0,1))  +  fy * ((1 - fx) * v(1,0) + fx * v(1,1))
 *
 *   UMPA_UNWARP_CUBIC    (Keys' kernel with a = -0.5, i.e. Catmull-Rom; taps a, b = -1 .. 2.)  For t = fx and t = fy:
 *                            w[-1] = ((-t + 2) * t - 1) * t / 2
 *                            w[ 0] = ((3 * t - 5) * t * t + 2) / 2           ( = (((3 * t - 5) * t) * t + 2) / 2 )
 *                            w[ 1] = ((-3 * t + 4) * t + 1) * t / 2
 *                            w[ 2] = (t - 1) * t * t / 2                     ( = (((t - 1) * t) * t) / 2 )
 *                        per tap row a, left to right:   r[a] = ((wx[-1] * v(a,-1) + wx[0] * v(a,0)) + wx[1] * v(a,1)) + wx[2] * v(a,2)
 *                        then top to bottom:             u = ((wy[-1] * r[-1] + wy[0] * r[0]) + wy[1] * r[1]) + wy[2] * r[2]
 *
 *   then                 out[i,j] = (u - dark[i,j]) / flat[i,j]
 *
 * with dark and flat at the OUTPUT pixel, each optional (a missing dark subtracts nothing, a missing flat divides by
 * nothing).  That is the reference's order -- unwarp, then (proj - dark) / flat (umpa_multi.py:130, :144) -- so references,
 * flats and the dark frame are expected in unwarped geometry; umpa_unwarp_frames is how they get there.
 *
 * Cubic is the default of the Python layer: bilinear resampling blurs speckle by an amount that depends on the sub-pixel
 * phase, i.e. it modulates visibility across the frame.
 *
 * Non-finite raw values: a NaN or infinity reaches EVERY output whose footprint (2 x 2 or 4 x 4 taps) contains it, the
 * taps of weight zero included (0 * NaN = NaN): an integer shift under the cubic kind spreads one NaN pixel over a 4 x 4
 * block of outputs.  That is what the expressions above say and it is not worked around; mend bad pixels first
 * (umpa_hip_correct_bad_pixels works on a model's frames, not on raw ones).
 * Map values must be finite (umpa_unwarp_map_create refuses others).
 *
 * Link libumpa_unwarp.so and libumpa_hip.so.  Error text of every call here: umpa_unwarp_last_error().
 */
#ifndef UMPA_UNWARP_H
#define UMPA_UNWARP_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMPA_UNWARP_LINEAR 0
#define UMPA_UNWARP_CUBIC  1

typedef struct umpa_unwarp_map umpa_unwarp_map;

/* d0, d1: host planes of H * W floats, copied to the memory of `device` once.  H * W must stay below 2^31.
 * Returns NULL on error (UMPA_HIP_E_DEVICE without a HIP device). */
umpa_unwarp_map *umpa_unwarp_map_create(int H, int W, const float *d0, const float *d1, int interp, int device);

/* Gives up the caller's reference.  A map that is still attached to models keeps unwarping what they stage: its device
 * planes are freed when the last of those models detaches (umpa_unwarp_attach(m, NULL)), attaches another map or is
 * destroyed.  Destroying the model first is equally safe.  The handle must not be used afterwards. */
void umpa_unwarp_map_destroy(umpa_unwarp_map *map);

/* The stand-alone operation on K frames: out[k] = unwarp(raw[k]), then dark[k] / flat[k] as above.
 *   raw[k]   H * W samples, raw_dtype 0 float64, 1 float32, 2 uint16 (umpa_hip_stage_sample's codes)
 *   dark, flat   tables of K pointers to H * W doubles, or NULL; out[k]: H * W doubles, must not overlap raw[k]
 * Host arrays by default (the call returns when out[] is written).  With UMPA_HIP_F_DEVICE_IO every array is a device
 * array on the map's device (the pointer tables themselves stay host arrays) and the call only enqueues K kernels on
 * `stream`.  No other flag. */
int umpa_unwarp_frames(umpa_unwarp_map *map, const void *const *raw, int raw_dtype, int K,
                       const double *const *dark, const double *const *flat, double *const *out,
                       int flags, void *stream);

/* While a map is attached, every umpa_hip_stage_sample on `m` unwarps each raw frame on its way into the model's back
 * sample buffer (one kernel per frame on the upload stream, in place of the flat-field kernel; also for a float64 stack
 * without dark / flat, which is otherwise a plain copy).  map = NULL detaches: umpa_hip_stage_sample is what it was.
 * Attaching replaces an earlier map.  UMPA_HIP_E_ARG for a model that borrows its frames (UMPA_HIP_F_DEVICE_FRAMES) and
 * for a map on another device than the model's; UMPA_HIP_E_UNSUPPORTED unless every frame of the model is H x W. */
int umpa_unwarp_attach(umpa_hip_model *m, umpa_unwarp_map *map);

const char *umpa_unwarp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_UNWARP_H */
