// umpa_hipx.h -- what libumpa_hip.so exports beside its public C ABI (include/umpa_hip.h), for libraries that are built from
// these very headers by the same build and may therefore pass the internal structs: libumpa_grid.so (umpa_grid.hip).
// Not installed, not versioned, not for other callers.
#pragma once
#include "../../include/umpa_hip.h"
#include "umpa_tiled.h"

extern "C" {

// Set (fn != NULL) or clear the model's table consumer (umpa::TableConsumer, umpa_tiled.h).  While one is set a match
//   * must go down the plain tiled path whole (no masks, all frames at one position, steps and search range within the
//     path's limits, not forced direct): anything else fails with UMPA_HIP_E_UNSUPPORTED before a kernel is launched;
//   * fills the maps and the exhaustive table of every row chunk as always (prep_maps, corr_volume / corr_march; the
//     on-demand stages are off: the consumer reads every plane) and calls `fn(user, dev, M, R, A, stream)` where it would
//     launch replay_walk.
// With no consumer set every launch is what it was.  The caller clears it again, also after a failed match.
int umpa_hipx_set_table_consumer(umpa_hip_model* m, umpa::TableConsumer fn, void* user);

}
