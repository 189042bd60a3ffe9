// prep_plan_check.cpp -- umpa_amd/csrc/umpa_prep_plan.h against a brute-force model of the map tiles.  Host code only.
//
//   c++ -std=c++17 -O1 -I umpa_amd/csrc tests/prep_plan_check.cpp -o prep_plan_check && ./prep_plan_check [steps] [seed]
//
// The header keeps ONE rectangle and a flag for the reference-side maps of a model.  The model here keeps, per tile, what
// the tile's reference-side planes were computed from: the reference stack's version, the window's, the layout (kind,
// frame count, plane size), the frame subset and the allocation they live in.  A random sequence of what a model lives
// through -- matches on random tile rectangles, reference and sample updates, new windows, kinds, frame counts and plane
// sizes, subset matches, reallocations, frames the library owns and frames it borrows, with the flag and without -- is run
// through the header exactly as run_tiled / tiled_maps / tiled_prep call it (umpa_hip.hip, umpa_tiled.h), and after every
// match:
//   1. every tile the match reads holds reference-side maps of the current reference stack, window, layout and allocation;
// and, injected every so often into whatever state the sequence has reached:
//   2. [whole region, a ROI inside it, whole region] with nothing changed in between: the third match (and the second)
//      leaves the reference side alone.
// A caller that borrows frames passes UMPA_HIP_F_REUSE_REF_MAPS truthfully: only when it has not written the reference
// stack since the model's previous match (include/umpa_hip.h).  Exit status 0 and a line of counts, or 1 and the step.
#include "umpa_prep_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

using namespace umpa;

namespace {

const int NTX = 7, NTY = 6;

struct Rng {                                   // xorshift64*: the same sequence everywhere
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1DULL) >> 32); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool one_in(int n) { return below(n) == 0; }
};

// what a tile's reference-side planes were computed from; alloc < 0: never written in this allocation
struct Tag {
    long ref_version, win_version, alloc;
    int kind, K, subset;
    size_t plane;
    bool operator==(const Tag& o) const
    {
        return ref_version == o.ref_version && win_version == o.win_version && alloc == o.alloc && kind == o.kind && K == o.K &&
               subset == o.subset && plane == o.plane;
    }
};

struct World {
    // the library's side: the record and what tiled_maps knows of the allocation
    RefMapsRecord rec;
    size_t maps_cap = 0;
    // the model
    bool owns_frames = true, masked = false;
    int kind = 1, K = 10;
    size_t plane = 45 * 61;
    // the truth
    long ref_version = 0, win_version = 0, alloc = 0;
    bool ref_written_since_match = false;       // by the owner of borrowed frames
    Tag tile[NTY][NTX];
    // counts
    long matches = 0, reused = 0, ref_passes = 0, triples = 0;

    World() { drop_tiles(); }
    void drop_tiles()
    {
        for (int y = 0; y < NTY; y++)
            for (int x = 0; x < NTX; x++) tile[y][x] = Tag{-1, -1, -1, -1, -1, -1, 0};
    }
    void fresh_model(Rng& r)
    {
        rec = RefMapsRecord();
        maps_cap = 0;
        owns_frames = !r.one_in(3); masked = r.one_in(4);
        kind = masked ? 1 : r.below(2);         // (a masked model without dark field never touches the maps)
        K = 1 + r.below(12);
        plane = r.one_in(2) ? 45 * 61 : 61 * 45 + r.below(3);
        ref_version++; win_version++; alloc++;
        ref_written_since_match = false;
        drop_tiles();
    }
    // umpa_hip_update_frames(ref) on frames the library owns; the owner's own write into frames it lent
    void update_reference()
    {
        ref_version++;
        if (owns_frames) prep_plan_invalidate(rec);
        else ref_written_since_match = true;
    }
    void set_window() { win_version++; prep_plan_invalidate(rec); }               // upload_win -> tiled_factor_window
    void release() { maps_cap = 0; alloc++; prep_plan_invalidate(rec); drop_tiles(); }   // tiled_release

    // One match of the tiles PR, as run_tiled -> tiled_maps -> tiled_prep do it.  `subset` > 0: a frame subset of that many
    // frames (one rectangle of a sample-stepping stack).  Returns the sides, or -1 where property 1 fails.
    int match(const PrepRect& PR, bool flag, int subset)
    {
        const bool sub = subset > 0;
        const int Keff = sub ? subset : K;
        if (sub) prep_plan_invalidate(rec);
        const bool reuse = prep_reuse(sub, owns_frames, flag);
        // tiled_maps
        const size_t KP = ((size_t)Keff + 1) / 2, need = (kind == 1 ? 2 + 4 * KP : 2) * plane;
        const bool grow = maps_cap < need;
        prep_plan_layout(rec, kind, Keff, plane, grow);
        if (grow) { maps_cap = need; alloc++; drop_tiles(); }
        // tiled_prep
        const int sides = prep_plan_sides(rec, PR, reuse, masked ? 0 : 1);
        const Tag now = Tag{ref_version, win_version, alloc, kind, Keff, subset, plane};
        bool ok = true;
        for (int y = PR.ty0; y < PR.ty1; y++)
            for (int x = PR.tx0; x < PR.tx1; x++) {
                if (sides & 2) tile[y][x] = now;                      // prep_maps writes the reference side of the tile
                if (!(tile[y][x] == now)) ok = false;                 // ... and the match reads it
            }
        prep_plan_done(rec, PR, sides, kind, Keff, plane);
        if (sub) prep_plan_invalidate(rec);
        matches++;
        if (sides & 2) ref_passes++; else reused++;
        ref_written_since_match = false;
        return ok ? sides : -1;
    }
};

PrepRect random_rect(Rng& r)
{
    if (r.one_in(4)) return PrepRect{0, NTX, 0, NTY};
    PrepRect R;
    R.tx0 = r.below(NTX); R.tx1 = R.tx0 + (r.one_in(20) ? 0 : 1 + r.below(NTX - R.tx0));
    R.ty0 = r.below(NTY); R.ty1 = R.ty0 + (r.one_in(20) ? 0 : 1 + r.below(NTY - R.ty0));
    return R;
}

} // namespace

int main(int argc, char** argv)
{
    const long steps = argc > 1 ? atol(argv[1]) : 200000;
    Rng r = {argc > 2 ? (uint64_t)atoll(argv[2]) | 1 : 0x9E3779B97F4A7C15ULL};
    World w;
    w.fresh_model(r);
    for (long step = 0; step < steps; step++) {
        const int op = r.below(100);
        if (op < 55) {
            // a caller that borrows frames vouches only for what is true
            const bool may_vouch = !w.ref_written_since_match && w.matches > 0;
            const bool flag = r.one_in(2) && (w.owns_frames || may_vouch);
            const int subset = r.one_in(8) && w.K > 1 ? 1 + r.below(w.K - 1) : 0;
            const PrepRect PR = random_rect(r);
            if (w.match(PR, flag, subset) < 0) {
                fprintf(stderr, "step %ld: a match of tiles [%d,%d) x [%d,%d) (owns %d flag %d subset %d masked %d) reads reference-side "
                                "maps that are not those of the current reference stack\n",
                        step, PR.tx0, PR.tx1, PR.ty0, PR.ty1, (int)w.owns_frames, (int)flag, subset, (int)w.masked);
                return 1;
            }
        } else if (op < 67) w.update_reference();
        else if (op < 77) { /* umpa_hip_update_frames(sam), stage_sample: the library hears of it and has nothing to do */ }
        else if (op < 82) w.set_window();
        else if (op < 86) { if (!w.masked) w.kind = r.below(2); }
        else if (op < 90) w.K = 1 + r.below(12);
        else if (op < 93) w.plane = r.one_in(2) ? 45 * 61 : 61 * 45 + r.below(3);
        else if (op < 96) w.release();
        else if (op < 98) w.fresh_model(r);
        else {
            // property 2, from whatever state the sequence is in: frames the library owns without the flag, borrowed
            // ones with it (the first match of the three computes what it must; the owner writes nothing afterwards)
            const PrepRect whole = {0, NTX, 0, NTY};
            PrepRect roi = random_rect(r);
            const int s1 = w.match(whole, false, 0);
            const int s2 = w.match(roi, !w.owns_frames, 0);
            const int s3 = w.match(whole, !w.owns_frames, 0);
            w.triples++;
            if (s1 < 0 || s2 < 0 || s3 < 0) { fprintf(stderr, "step %ld: whole / ROI / whole reads stale maps (%d %d %d)\n", step, s1, s2, s3); return 1; }
            if ((s2 & 2) || (s3 & 2)) {
                fprintf(stderr, "step %ld: whole region, ROI [%d,%d) x [%d,%d), whole region with nothing changed: sides %d, %d, %d -- "
                                "the reference side was computed again\n", step, roi.tx0, roi.tx1, roi.ty0, roi.ty1, s1, s2, s3);
                return 1;
            }
        }
    }
    if (w.reused == 0 || w.ref_passes == 0 || w.triples == 0) { fprintf(stderr, "the sequence never reused, or never computed: nothing was checked\n"); return 1; }
    printf("prep_plan_check: %ld steps, %ld matches (%ld computed the reference side, %ld reused it), %ld whole/ROI/whole triples: OK\n",
           steps, w.matches, w.ref_passes, w.reused, w.triples);
    return 0;
}
