// umpa_hipx.h -- what libumpa_hip.so exports beside its public C ABI (include/umpa_hip.h), for libraries that are built from
// these very headers by the same build and may therefore pass the internal structs: libumpa_grid.so (umpa_grid.hip) and
// libumpa_unwarp.so (umpa_unwarp.hip).
// Not installed, not versioned, not for other callers.
//
// UMPA_HIPX_STAGE_ONLY (defined by umpa_unwarp.hip before it includes this file): only the stage filter.  It passes no
// internal struct, and a translation unit that includes umpa_tiled.h carries that header's kernels in its own code object
// (and their compile time) whether it launches them or not.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/umpa_hip.h"
#ifndef UMPA_HIPX_STAGE_ONLY
#include "umpa_tiled.h"
#endif

extern "C" {

#ifndef UMPA_HIPX_STAGE_ONLY
// Set (fn != NULL) or clear the model's table consumer (umpa::TableConsumer, umpa_tiled.h).  While one is set a match
//   * must go down the plain tiled path whole (no masks, all frames at one position, steps and search range within the
//     path's limits, not forced direct): anything else fails with UMPA_HIP_E_UNSUPPORTED before a kernel is launched;
//   * fills the maps and the exhaustive table of every row chunk as always (prep_maps, corr_volume / corr_march; the
//     on-demand stages are off: the consumer reads every plane) and calls `fn(user, dev, M, R, A, stream)` where it would
//     launch replay_walk.
// With no consumer set every launch is what it was.  The caller clears it again, also after a failed match.
int umpa_hipx_set_table_consumer(umpa_hip_model* m, umpa::TableConsumer fn, void* user);

// The per-model switch of include/umpa_grid.h (umpa_grid_set_masked), off by default; it lives with the model and changes
// nothing on a model without masks.  While it is on, a match of a masked model under a table consumer goes down the masked
// tiled path whole (corr_masked, umpa_masked.h; on-demand stages off) and calls the consumer where it would launch
// replay_cost, with a ReplayArgs that describes the chunk's table of FINISHED costs: [(2 ms - 1)^2][NV][drows][N1d] doubles,
// slot_stride = drows * N1d, strip_w = 0; per slot the planes cost, T and (NV = 3: dark-field) v.  Maps holds what
// tiled_match_masked filled (the reference means of the dark-field model, else nothing).  What that path does not take of
// its own accord is UMPA_HIP_E_UNSUPPORTED with a text that names the reason: a window size without a corr_masked
// configuration, exact-fit windows, a pair plane past 4 GiB, a step product past the masked limit.
int umpa_hipx_set_masked_consumer(umpa_hip_model* m, int on);
// NV of the table a consumer of `m` would be handed by the masked path (2, or 3 for the dark-field model); 0: the model has
// no masks or its switch is off, the table is the plain path's.
int umpa_hipx_masked_table(const umpa_hip_model* m);

// The general consumer of a model (include/umpa_grid.h: umpa_grid_set_general), set (fn != NULL) or cleared; it lives with the
// model.  Where a table consumer is set and a match is about to be refused because no tiled path takes the model and the
// region whole -- frames at different positions or of unequal shapes, forced direct, a masked model whose switch is off or
// that the masked path does not admit, steps or search ranges past the tiled limits; never the kernel dark-field model --
// the match calls `fn(user, dev, kind, has_mask, A, stream)` ONCE instead: `user` is the table consumer's, `dev` the
// model's ModelDev, `kind` UMPA_HIP_KIND_*, `A` the full region as the general kernels take it (dense arrays, device
// pointers, cover and thr as given).  `fn` fills tables of finished costs with kernels of its own and runs the table
// consumer on them; hipSuccess, or an error the match reports (hipErrorOutOfMemory: UMPA_HIP_E_NOMEM).  Everything around
// the call is umpa_hip_match_region's as it is: uploads, the staged stack, device I/O, planar maps, asynchronous matches,
// the downloads (one piece: all rows), the coverage threshold.  What a tiled path takes whole keeps going there, unless
// `always` is set (the caller wants the explicit window x frame sum everywhere, as a model forced onto the direct kernel
// does).  With no general consumer set every call, refusal and text is what it was.  Host code only: no kernel of
// libumpa_hip.so knows of it.
typedef hipError_t (*umpa_hipx_general_consumer)(void* user, const umpa::ModelDev& dev, int kind, int has_mask,
                                                 const umpa::RegionArgs& A, hipStream_t stream);
int umpa_hipx_set_general_consumer(umpa_hip_model* m, umpa_hipx_general_consumer fn, int always);

// The model as its own kernels see it (umpa_grid_uncertainty runs a kernel of libumpa_grid.so on the model's device frames):
// `*dev` is the model's ModelDev -- the descriptor table (per frame sam, ref, mask, shape and position), the window and its
// sum, Na, Nw, max_shift, padding, ref_mode -- `*kind` UMPA_HIP_KIND_*, `*has_mask` 0 or 1, `*device` its device, `*stream`
// the stream of its host-array entry points.  The sample pointers are those of the stack the LAST MATCH ADOPTED: a stack
// that umpa_hip_stage_sample uploaded and no call has adopted yet is not it, and this call takes no UMPA_HIP_F_USE_STAGED.
// The descriptor table is rewritten in stream order by the call that adopts a staged stack: a caller that reads it on another
// stream waits for the model's work first.  Host code only: nothing is enqueued.  UMPA_HIP_E_ARG for a NULL argument.
int umpa_hipx_model_view(umpa_hip_model* m, umpa::ModelDev* dev, int* kind, int* has_mask, int* device, hipStream_t* stream);
#endif

// A stage filter takes the place of flat_correct_kernel in umpa_hip_stage_sample: frame k of the raw stack (k >= 0) lies in
// device memory as it came from the host (`raw_dtype`: 0 float64, 1 float32, 2 uint16); the filter enqueues, on
// `upload_stream`, whatever writes the H x W float64 frame `out_k` of the model's back sample buffer from it (dark_k /
// flat_k: the caller's device frames, or NULL) and returns 0 or a UMPA_HIP_E_* code.  k = -1 (every other argument 0) is
// the release call: the model lets go of the filter -- it was replaced or cleared, or the model is being destroyed (after
// its upload stream has drained) -- and never calls it again.
typedef int (*umpa_hipx_stage_filter)(void* user, int k, const void* staged_raw, int raw_dtype, const double* dark_k,
                                      const double* flat_k, double* out_k, int H, int W, hipStream_t upload_stream);

// Set (fn != NULL) or clear the model's stage filter.  While one is set, umpa_hip_stage_sample always stages the raw bytes
// on the device (a float64 stack without dark / flat too, which is otherwise copied straight into the sample buffer) and
// calls `fn` per frame where it would launch flat_correct_kernel; events and the double buffer are what they were.
// Setting is refused, and the filter in place stays, with UMPA_HIP_E_ARG for a model that borrows its frames and for
// `device` other than the model's, with UMPA_HIP_E_UNSUPPORTED unless every frame of the model is H x W.  An earlier
// filter gets its release call before the new one is installed.  With no filter set the call is what it was.
int umpa_hipx_set_stage_filter(umpa_hip_model* m, umpa_hipx_stage_filter fn, void* user, int H, int W, int device);

}
