// umpa_prep_plan.h -- which sides of the maps a match computes, and what the record of the reference side becomes.
// Host code without a HIP type in it: tests/prep_plan_check.cpp drives it against a brute-force model of the tiles.
//
// The maps of a model (umpa_tiled.h: Maps) have a sample side (SamSq, WS_k) and a reference side (RefSq, MR_k).  The sample
// side is recomputed by every match for the tiles it reads.  The reference side is kept: RefMapsRecord says for which
// reference stack geometry and for which ONE rectangle of tiles the planes are current, and a match whose tiles lie inside
// that rectangle leaves them alone -- if it may trust that nobody has written the reference frames since (prep_reuse).
#pragma once
#include <cstddef>

namespace umpa {

// tiles [tx0, tx1) x [ty0, ty1) of the maps (prep_rect)
struct PrepRect { int tx0, tx1, ty0, ty1; };

// What the reference-side maps hold.  `ref_maps_ok`: the tiles of `ref_rect` are maps of the reference stack as it was at
// the model's last match, for this (kind, frame count, plane size).  Cleared by whoever changes the reference frames, the
// window or the allocation; frames the model borrows can change without the library hearing of it.
struct RefMapsRecord {
    bool ref_maps_ok = false;
    int ref_kind = -1, ref_K = 0;
    size_t ref_plane = 0;
    int ref_rect[4] = {0, 0, 0, 0};   // tiles (tx0, tx1, ty0, ty1) of the reference side that were computed last
};

// May this match take the reference side from the record?  Frames the library owns are written by umpa_hip_update_frames
// alone, which clears the record: nothing more to ask.  Frames it borrows (UMPA_HIP_F_DEVICE_FRAMES) belong to a caller who
// can overwrite them at any time: only UMPA_HIP_F_REUSE_REF_MAPS (`vouched`) says they are those of the previous match.  A
// frame subset (one rectangle of a sample-stepping stack) fills the planes with its own frames: never.
inline bool prep_reuse(bool subset, bool owns_frames, bool vouched) { return !subset && (owns_frames || vouched); }

inline void prep_plan_invalidate(RefMapsRecord& st) { st.ref_maps_ok = false; }

// The planes of the coming match: another kind, frame count or plane size lays them out anew, and so does a new allocation.
inline void prep_plan_layout(RefMapsRecord& st, int kind, int K, size_t plane, bool reallocated)
{
    if (reallocated || st.ref_kind != kind || st.ref_K != K || st.ref_plane != plane) st.ref_maps_ok = false;
}

inline bool prep_plan_covered(const RefMapsRecord& st, const PrepRect& PR)
{
    return st.ref_rect[0] <= PR.tx0 && st.ref_rect[1] >= PR.tx1 && st.ref_rect[2] <= PR.ty0 && st.ref_rect[3] >= PR.ty1;
}

// The sides prep_maps computes for the tiles PR (bit 0 sample, bit 1 reference): both, or `reuse_sides` where the reference
// side may be trusted (`reuse`: prep_reuse) and the record covers PR -- 1, the sample side (plain path), or 0, nothing (masked
// path: only the reference means are read).  The record is not valid while the launch is pending: prep_plan_done.
inline int prep_plan_sides(RefMapsRecord& st, const PrepRect& PR, bool reuse, int reuse_sides)
{
    const int sides = (reuse && st.ref_maps_ok && prep_plan_covered(st, PR)) ? reuse_sides : 3;
    st.ref_maps_ok = false;
    return sides;
}

// After the launch of `sides` over PR succeeded (or nothing had to be launched).  The rectangle is the one the reference
// side was last WRITTEN for: a sample-only pass over fewer tiles (a ROI after the whole region) leaves the larger
// rectangle in place, whose tiles are as valid as before.  One rectangle, no unions: a reference pass over tiles the
// record does not cover replaces it.
inline void prep_plan_done(RefMapsRecord& st, const PrepRect& PR, int sides, int kind, int K, size_t plane)
{
    if (sides & 2) { st.ref_rect[0] = PR.tx0; st.ref_rect[1] = PR.tx1; st.ref_rect[2] = PR.ty0; st.ref_rect[3] = PR.ty1; }
    st.ref_maps_ok = true; st.ref_kind = kind; st.ref_K = K; st.ref_plane = plane;
}

} // namespace umpa
