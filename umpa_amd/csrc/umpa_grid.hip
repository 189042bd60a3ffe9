// umpa_grid.hip -- libumpa_grid.so: exhaustive grid search and the cost volume (include/umpa_grid.h).  gfx950 only.
//
// A second library, built from the headers of libumpa_hip.so by the same build: it holds the kernel families of
// umpa_grid_kernels.h, umpa_basins_kernels.h, umpa_track_kernels.h, umpa_widen_kernels.h, umpa_levels_kernels.h and
// umpa_sequence_kernels.h, their twins on a masked model's table of finished costs (umpa_masked_grid_kernels.h), the kernel
// that fills such a table for the models no tiled path takes (umpa_general_table_kernels.h) and no other feature code.  A call sets itself as the model's table
// consumer (umpa_hipx.h), runs umpa_hip_match_region down the tiled path -- whose argument checks, uploads, row chunks, downloads and callbacks are
// therefore the existing ones -- and clears the consumer again.  No CPU fallback.
// One call is no table consumer: umpa_grid_uncertainty (umpa_resident_kernels.h, at the end of this file) runs one kernel on the
// model's own device frames, which umpa_hipx_model_view lends it.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>

#include "../../include/umpa_grid.h"
#include "umpa_host.h"
#include "umpa_hipx.h"
#include "umpa_grid_kernels.h"
#include "umpa_basins_kernels.h"
#include "umpa_track_kernels.h"
#include "umpa_widen_kernels.h"
#include "umpa_levels_kernels.h"
#include "umpa_sequence_kernels.h"
#include "umpa_masked_grid_kernels.h"
#include "umpa_general_table_kernels.h"
#include "umpa_resident_kernels.h"

using namespace umpa;

#define UMPA_GRID_API extern "C" __attribute__((visibility("default")))

namespace {

struct GridJob {
    bool volume = false;              // cost_volume_kernel instead of grid_min_kernel
    VolumeArgs V = {nullptr, nullptr, nullptr, 0};
    // host-array cost volume: device copies of the wanted arrays (cost, T, df), allocated at the first chunk (the model's
    // search range is known there)
    bool host = false, want[3] = {false, false, false};
    double* dev[3] = {nullptr, nullptr, nullptr};
    size_t count = 0;                 // doubles per array
    const char* refused = nullptr;
    // umpa_grid_basins: grid_basins_kernel instead of either; host arrays: one device block for all ten outputs
    bool basins = false;
    BasinArgs B = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    bool want_df = false;
    void* block = nullptr;
    // umpa_grid_track: grid_track_kernel; host arrays: one device block for the two priors and the twelve outputs, the
    // priors uploaded by the consumer before the first chunk's kernel
    bool track = false;
    TrackArgs K = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                   0, 0, 0.0, 0.0};
    const double* host_pi = nullptr;
    const double* host_pj = nullptr;
    // window widening (umpa_grid_wide_*, b > 0): the consumer's kernels run on the box-pooled table and maps.  One workspace
    // from the stream-ordered allocator, taken at the first chunk on the call's stream and given back on it when the call
    // has enqueued its last kernel: the pooled table of a call's rows, the carry (the chunk's last 2b raw rows), the pooled maps
    int b = 0;
    void* ws = nullptr;
    hipStream_t ws_stream = nullptr;
    double* pool = nullptr;
    double* carry = nullptr;
    double* wmaps = nullptr;
    int pool_rows = 0, next_drow0 = 0;
    // umpa_grid_wide_match_region on host arrays: a pooled row is finished one chunk late, so the match entry point's
    // chunk-by-chunk download would fetch rows before they are written.  The maps go to one device block instead (allocated
    // by the consumer on the model's device) and are downloaded when all is enqueued.
    bool mhost = false;
    RegionArgs mh = {};               // the caller's host arrays (values, err, cover, dbg_*) and nparam
    void* mblock = nullptr;
    RegionArgs md = {};               // their device twins
    // umpa_grid_levels_track (L > 0): `track` per level on one table pass.  lb[0] is the lag of every level; the workspace
    // holds a pooled table and a set of pooled maps per widened level (pools, lmaps), the carry and two prior planes.
    // lev / sel: the caller's device arrays, or their places in `block` (host arrays)
    int L = 0, lb[UMPA_LEVELS_MAX] = {0, 0, 0, 0};
    double ltol[UMPA_LEVELS_MAX] = {0.0, 0.0, 0.0, 0.0};
    double* pools[3] = {nullptr, nullptr, nullptr};
    double* lmaps[3] = {nullptr, nullptr, nullptr};
    double* prior = nullptr;
    LevelsPlanes lev = {}, sel = {};
    int* sel_level = nullptr;
    int* sel_hw = nullptr;
    bool want_sel = false;
    // umpa_grid_sequence: grid_sequence_kernel; host arrays: `block` holds the previous state (uploaded by the consumer before
    // the first chunk's kernel), the next state and the twelve maps
    bool sequence = false;
    SequenceArgs Q = {};
    const double* host_prev = nullptr;
    bool want_next = false;
    size_t state_len = 0;             // doubles per state: U * U * N0 * N1 (known at the first chunk)
    // a refusal of the consumer with a code of its own (otherwise the match entry point's) and a text that names a value
    int refused_code = 0;
    std::string refused_text;
    // an admitted masked model (umpa_grid_set_masked): the planes per shift of its table of finished costs, 2 or 3
    // (umpa_hipx_masked_table); 0: the plain path's table.  The kernels are then those of umpa_masked_grid_kernels.h.
    int masked = 0;
    // the general table (umpa_grid_set_general): one table of finished costs for the call's row chunks, from the stream-ordered
    // allocator on the call's stream, given back on it when the call has enqueued its last kernel
    void* gtable = nullptr;
    hipStream_t gstream = nullptr;
};

// the block of umpa_grid_wide_match_region's host path: values, dbg_d, dbg_a, cover (doubles), then err, dbg_n (ints)
size_t match_carve(RegionArgs& d, const RegionArgs& h, void* block, size_t n)
{
    double* q = (double*)block;
    d = h;
    d.values = q; q += n * h.nparam;
    d.dbg_d = h.dbg_d ? q : nullptr; q += h.dbg_d ? n * 25 : 0;
    d.dbg_a = h.dbg_a ? q : nullptr; q += h.dbg_a ? n * 16 : 0;
    d.cover = h.cover ? q : nullptr; q += h.cover ? n : 0;
    int* r = (int*)q;
    d.err = r; r += n;
    d.dbg_n = h.dbg_n ? r : nullptr; r += h.dbg_n ? n : 0;
    return (size_t)((char*)r - (char*)block);
}

// the ten output arrays of umpa_grid_basins in the order of its arguments: six of doubles, then four of ints ([K] planes, count one)
void basins_carve(BasinArgs& B, void* block, size_t plane, int K, bool df)
{
    double* d = (double*)block;
    B.f = d; B.T = d + K * plane; B.dx = d + 2 * K * plane; B.dy = d + 3 * K * plane; B.cost = d + 4 * K * plane;
    B.df = df ? d + 5 * K * plane : nullptr;
    int* q = (int*)(d + 6 * K * plane);
    B.si = q; B.sj = q + K * plane; B.err = q + 2 * K * plane; B.count = q + 3 * K * plane;
}
size_t basins_bytes(size_t plane, int K) { return 6 * K * plane * sizeof(double) + (3 * K + 1) * plane * sizeof(int); }

// umpa_grid_track's block: nine planes of doubles (the priors, then the seven double outputs in the order of its
// arguments), then five of ints
void track_carve(TrackArgs& K, void* block, size_t plane, bool df)
{
    double* d = (double*)block;
    K.pi = d; K.pj = d + plane;
    K.f = d + 2 * plane; K.T = d + 3 * plane; K.dx = d + 4 * plane; K.dy = d + 5 * plane; K.cost = d + 6 * plane;
    K.df = df ? d + 7 * plane : nullptr;
    K.cost0 = d + 8 * plane;
    int* q = (int*)(d + 9 * plane);
    K.si = q; K.sj = q + plane; K.err = q + 2 * plane; K.count = q + 3 * plane; K.found = q + 4 * plane;
}
size_t track_bytes(size_t plane) { return 9 * plane * sizeof(double) + 5 * plane * sizeof(int); }

// umpa_grid_sequence's block: the two states (U2 planes each; absent ones take no room), eight planes of doubles (the six
// double maps in the order of the arguments, total, cost0), then four of ints
void sequence_carve(SequenceArgs& Q, void* block, size_t plane, int U2, bool prev, bool next, bool df)
{
    double* d = (double*)block;
    Q.prev = prev ? d : nullptr; d += prev ? U2 * plane : 0;
    Q.next = next ? d : nullptr; d += next ? U2 * plane : 0;
    Q.f = d; Q.T = d + plane; Q.dx = d + 2 * plane; Q.dy = d + 3 * plane; Q.cost = d + 4 * plane;
    Q.df = df ? d + 5 * plane : nullptr;
    Q.total = d + 6 * plane; Q.cost0 = d + 7 * plane;
    int* q = (int*)(d + 8 * plane);
    Q.si = q; Q.sj = q + plane; Q.err = q + 2 * plane; Q.moved = q + 3 * plane;
}
size_t sequence_bytes(size_t plane, int U2, bool prev, bool next)
{
    return ((size_t)U2 * ((prev ? 1 : 0) + (next ? 1 : 0)) + 8) * plane * sizeof(double) + 4 * plane * sizeof(int);
}

// the frame count as a template constant exactly where replay_walk's dispatch has it (tiled_match)
template <int KIND, int NA>
void launch(const GridJob& J, const ModelDev& dev, const Maps& M, const ReplayArgs& R, const RegionArgs& A, hipStream_t s)
{
    if (J.sequence) {                                                 // (a wave takes 64 or 32 pixels: SequenceArgs::half)
        const int bw = 1 << R.bw_log2, bh = (64 >> J.Q.half) >> R.bw_log2;
        hipLaunchKernelGGL((grid_sequence_kernel<KIND, NA>), dim3((A.N1 + bw - 1) / bw, (R.rows + bh - 1) / bh), dim3(64),
                           sequence_lds(dev.ms, J.Q.prev != nullptr), s, dev, M, R, A, J.Q);
    } else if (J.track) {
        const int bw = 1 << R.bw_log2, bh = 64 >> R.bw_log2;
        hipLaunchKernelGGL((grid_track_kernel<KIND, NA>), dim3((A.N1 + bw - 1) / bw, (R.rows + bh - 1) / bh), dim3(64),
                           grid_basins_lds(dev.ms), s, dev, M, R, A, J.K);
    } else if (J.basins) {
        const int bw = 1 << R.bw_log2, bh = 64 >> R.bw_log2;
        hipLaunchKernelGGL((grid_basins_kernel<KIND, NA>), dim3((A.N1 + bw - 1) / bw, (R.rows + bh - 1) / bh), dim3(64),
                           grid_basins_lds(dev.ms), s, dev, M, R, A, J.B);
    } else if (J.volume) {
        hipLaunchKernelGGL((cost_volume_kernel<KIND, NA>), dim3((A.N1 + 63) / 64, R.rows), dim3(64), 0, s, dev, M, R, A, J.V);
    } else {
        const int bw = 1 << R.bw_log2, bh = 64 >> R.bw_log2;
        hipLaunchKernelGGL((grid_min_kernel<KIND, NA>), dim3((A.N1 + bw - 1) / bw, (R.rows + bh - 1) / bh), dim3(64), 0, s, dev, M, R, A);
    }
}

#define UMPA_WIDEN_HB(...) switch (b) { case 1: { constexpr int HB = 1; __VA_ARGS__; } break; case 2: { constexpr int HB = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int HB = 3; __VA_ARGS__; } break; case 4: { constexpr int HB = 4; __VA_ARGS__; } break; case 5: { constexpr int HB = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int HB = 6; __VA_ARGS__; } break; case 7: { constexpr int HB = 7; __VA_ARGS__; } break; case 8: { constexpr int HB = 8; __VA_ARGS__; } break; }

// the pooled maps of half-width b (prep_maps has filled the raw ones for the whole region): zero where nothing is pooled
// (only pixels whose table entries are NaN read there)
hipError_t widen_maps(int b, const ModelDev& dev, const Maps& M, const RegionArgs& A, int N0d, int N1d, double* wmaps, hipStream_t s)
{
    const int KP = (dev.Na + 1) / 2;
    const bool df = M.WS != nullptr;
    const size_t plane = (size_t)M.H * M.W, nmap = (2 + (df ? 4 * (size_t)KP : 0)) * plane;
    hipError_t e;
    if ((e = hipMemsetAsync(wmaps, 0, nmap * sizeof(double), s)) != hipSuccess) return e;
    WidenMapArgs a;
    a.W = M.W; a.plane = plane;
    a.r0 = std::max(A.org0 - (dev.ms - 1) + b, b); a.r1 = std::min(A.org0 + N0d - 1 + (dev.ms - 1) - b + 1, M.H - b);
    a.c0 = std::max(A.org1 - (dev.ms - 1) + b, b); a.c1 = std::min(A.org1 + N1d - 1 + (dev.ms - 1) - b + 1, M.W - b);
    if (a.r0 < a.r1 && a.c0 < a.c1) {
        const dim3 grd((a.c1 - a.c0 + 63) / 64, (a.r1 - a.r0 + UMPA_WIDEN_SEG - 1) / UMPA_WIDEN_SEG, 2);
        UMPA_WIDEN_HB(hipLaunchKernelGGL((widen_map_kernel<HB, false>), grd, dim3(64), 0, s, (const void*)M.SamSq, (void*)wmaps, a))
        if (df) {                                                     // (tiled_maps) WS and MR lie behind each other: 2 KP planes of pairs
            const dim3 grp(grd.x, grd.y, 2 * KP);
            UMPA_WIDEN_HB(hipLaunchKernelGGL((widen_map_kernel<HB, true>), grp, dim3(64), 0, s, (const void*)M.WS, (void*)(wmaps + 2 * plane), a))
        }
    }
    return hipGetLastError();
}

// the pooled table of the rows [g.p0, g.p1) at half-width g.b, from the chunk's table and the carry
void widen_table(const WidenGeom& g, const double* table, const double* carry, double* pool, hipStream_t s)
{
    const int b = g.b;
    const dim3 grd((g.N1q + 63) / 64, g.U2, (g.p1 - g.p0 + UMPA_WIDEN_SEG - 1) / UMPA_WIDEN_SEG);
    if (g.strip_w > 0) { UMPA_WIDEN_HB(hipLaunchKernelGGL((widen_table_kernel<HB, true>), grd, dim3(64), 0, s, table, carry, pool, g)) }
    else { UMPA_WIDEN_HB(hipLaunchKernelGGL((widen_table_kernel<HB, false>), grd, dim3(64), 0, s, table, carry, pool, g)) }
}
#undef UMPA_WIDEN_HB

// Window widening, one row chunk: the pooled maps (first chunk; prep_maps has filled the raw ones for the whole region), the
// pooled table of the dense rows whose block is complete (widen_rows), the carry for the next chunk.  `Mw`, `Rw`: what the
// consumer's kernel gets in place of M and R -- the plain table layout, the output rows among the pooled ones.
hipError_t widen_chunk(GridJob& J, const ModelDev& dev, const Maps& M, const ReplayArgs& R, const RegionArgs& A, hipStream_t s,
                       Maps& Mw, ReplayArgs& Rw)
{
    const int b = J.b, U = 2 * dev.ms - 1, KP = (dev.Na + 1) / 2;
    const bool df = M.WS != nullptr;
    WidenGeom g;
    g.b = b; g.U2 = U * U;
    g.N0d = A.step0 * (A.N0 - 1) + 1; g.N1d = A.step1 * (A.N1 - 1) + 1;
    g.drow0 = R.drow0; g.drows = R.drows; g.crows = R.drow0 == 0 ? 0 : 2 * b;
    g.strip_w = R.strip_w; g.tw = R.tw; g.N1p = R.N1d; g.N1q = (g.N1d + 31) / 32 * 32;
    widen_rows(b, g.N0d, g.drow0, g.drows, g.p0, g.p1);
    const bool last = R.drow0 + R.drows >= g.N0d;
    if (R.drow0 != J.next_drow0 || (!last && R.drows < 2 * b)) { J.refused = "widen: the row chunks do not follow each other"; return hipErrorInvalidValue; }
    const size_t plane = (size_t)M.H * M.W, nmap = (2 + (df ? 4 * (size_t)KP : 0)) * plane;
    if (!J.ws) {
        J.pool_rows = std::min(g.N0d, g.drows + b);
        if ((size_t)J.pool_rows * g.N1q >= ((size_t)1 << 32)) { J.refused = "widen: a plane of the pooled table passes the 32-bit stride of the lookups"; return hipErrorInvalidValue; }
        const size_t pool_len = (size_t)g.U2 * J.pool_rows * g.N1q, carry_len = last ? 0 : widen_table_len(g, 2 * b);
        hipError_t e = hipMallocAsync(&J.ws, (pool_len + carry_len + nmap) * sizeof(double), s);
        if (e != hipSuccess) { J.ws = nullptr; return hipErrorOutOfMemory; }
        J.ws_stream = s;
        J.pool = (double*)J.ws; J.carry = J.pool + pool_len; J.wmaps = J.carry + carry_len;
        if ((e = widen_maps(b, dev, M, A, g.N0d, g.N1d, J.wmaps, s)) != hipSuccess) return e;
    }
    if (g.p1 - g.p0 > J.pool_rows) { J.refused = "widen: a row chunk larger than the first"; return hipErrorInvalidValue; }
    if (g.p1 > g.p0) widen_table(g, R.table, J.carry, J.pool, s);
    if (!last) {
        const WidenCarryCopy cc = widen_carry_copy(g);
        hipLaunchKernelGGL(widen_carry_kernel, dim3((unsigned)((cc.run + 255) / 256), (unsigned)cc.nruns), dim3(256), 0, s, R.table, J.carry, cc);
    }
    J.next_drow0 = R.drow0 + R.drows;
    Mw.SamSq = J.wmaps; Mw.RefSq = J.wmaps + plane;
    Mw.WS = df ? J.wmaps + 2 * plane : nullptr;
    Mw.MR = df ? J.wmaps + (2 + 2 * (size_t)KP) * plane : nullptr;
    Rw.table = J.pool; Rw.slot_stride = (size_t)(g.p1 - g.p0) * g.N1q; Rw.drow0 = g.p0; Rw.N1d = g.N1q;
    Rw.strip_w = 0; Rw.tw = 0; Rw.drows = g.p1 - g.p0;
    Rw.bw_log2 = 4;                                                   // the plain table's block shape (tiled_match)
    Rw.row0 = (g.p0 + A.step0 - 1) / A.step0;
    Rw.rows = g.p1 > g.p0 ? std::max(0, std::min(A.N0, (g.p1 - 1) / A.step0 + 1) - Rw.row0) : 0;
    return hipGetLastError();
}

// the masked twins: a wave takes 64 pixels of one row (32: SequenceArgs::half), whatever R.bw_log2 says
template <int KIND>
void launch_masked_grid(const GridJob& J, const ModelDev& dev, const ReplayArgs& R, const RegionArgs& A, hipStream_t s)
{
    const dim3 grd((A.N1 + 63) / 64, R.rows), blk(64);
    if (J.sequence) {
        const int ls = 64 >> J.Q.half;
        hipLaunchKernelGGL((masked_sequence_kernel<KIND>), dim3((A.N1 + ls - 1) / ls, R.rows), blk,
                           sequence_lds(dev.ms, J.Q.prev != nullptr), s, dev, R, A, J.Q);
    } else if (J.track) hipLaunchKernelGGL((masked_track_kernel<KIND>), grd, blk, grid_basins_lds(dev.ms), s, dev, R, A, J.K);
    else if (J.basins) hipLaunchKernelGGL((masked_basins_kernel<KIND>), grd, blk, grid_basins_lds(dev.ms), s, dev, R, A, J.B);
    else if (J.volume) hipLaunchKernelGGL((masked_volume_kernel<KIND>), grd, blk, 0, s, dev, R, A, J.V);
    else hipLaunchKernelGGL((masked_min_kernel<KIND>), grd, blk, 0, s, dev, R, A);
}

// the consumer's kernel on the output rows R.rows of the table R, with the frame count as a template constant where
// replay_walk's dispatch has it (tiled_match)
hipError_t dispatch(const GridJob& J, const ModelDev& dev, const Maps& M, const ReplayArgs& R, const RegionArgs& A, hipStream_t s)
{
    if (R.rows <= 0 || A.N1 <= 0) return hipSuccess;
    if (J.masked) {
        if (J.masked == 3) launch_masked_grid<1>(J, dev, R, A, s);
        else launch_masked_grid<0>(J, dev, R, A, s);
        return hipGetLastError();
    }
    const int kind = M.WS ? 1 : 0;
    const bool small = (size_t)M.H * M.W * 2 * sizeof(double) < ((size_t)1 << 32);   // a pair plane (tiled_match)
#define UMPA_GRID_NA(n) case n: launch<1, n>(J, dev, M, R, A, s); break;
    if (kind == 1 && small && dev.Na <= UMPA_KTEMPL) {
        switch (dev.Na) {
            UMPA_GRID_NA(1) UMPA_GRID_NA(2) UMPA_GRID_NA(3) UMPA_GRID_NA(4) UMPA_GRID_NA(5) UMPA_GRID_NA(6)
            UMPA_GRID_NA(7) UMPA_GRID_NA(8) UMPA_GRID_NA(9) UMPA_GRID_NA(10) UMPA_GRID_NA(11) UMPA_GRID_NA(12)
            UMPA_GRID_NA(13) UMPA_GRID_NA(14) UMPA_GRID_NA(15) UMPA_GRID_NA(16) UMPA_GRID_NA(17) UMPA_GRID_NA(18)
            UMPA_GRID_NA(19) UMPA_GRID_NA(20) UMPA_GRID_NA(21) UMPA_GRID_NA(22) UMPA_GRID_NA(23) UMPA_GRID_NA(24)
        }
    } else if (kind == 1) launch<1, 0>(J, dev, M, R, A, s);
    else launch<0, 0>(J, dev, M, R, A, s);
#undef UMPA_GRID_NA
    return hipGetLastError();
}

// umpa_grid_levels_track's block (host arrays): seven planes of doubles per level and seven selected ones in the order of
// LevelsPlanes, then five planes of ints per level, five selected ones, `level` and `halfwidth`
void levels_carve(GridJob& J, void* block, size_t n)
{
    const size_t L = (size_t)J.L;
    double* d = (double*)block;
    double** const lv[7] = {&J.lev.f, &J.lev.T, &J.lev.dx, &J.lev.dy, &J.lev.cost, &J.lev.df, &J.lev.cost0};
    double** const sv[7] = {&J.sel.f, &J.sel.T, &J.sel.dx, &J.sel.dy, &J.sel.cost, &J.sel.df, &J.sel.cost0};
    for (int q = 0; q < 7; q++) { *lv[q] = d; d += L * n; }
    for (int q = 0; q < 7; q++) { *sv[q] = d; d += n; }
    int* i = (int*)d;
    int** const li[5] = {&J.lev.si, &J.lev.sj, &J.lev.err, &J.lev.count, &J.lev.found};
    int** const si[5] = {&J.sel.si, &J.sel.sj, &J.sel.err, &J.sel.count, &J.sel.found};
    for (int q = 0; q < 5; q++) { *li[q] = i; i += L * n; }
    for (int q = 0; q < 5; q++) { *si[q] = i; i += n; }
    J.sel_level = i; J.sel_hw = i + n;
    if (!J.want_df) J.lev.df = J.sel.df = nullptr;
}
size_t levels_bytes(int L, size_t n) { return 7 * ((size_t)L + 1) * n * sizeof(double) + (5 * ((size_t)L + 1) + 2) * n * sizeof(int); }

// the multi-level pooling of the rows [g.p0, g.p1): two or three widened levels hb[0] > hb[1] (> hb[2]) from one read
bool levels_table(const WidenGeom& g, const int* hb, int nw, const double* table, const double* carry, double* const* pools, hipStream_t s)
{
    const dim3 grd((g.N1q + 63) / 64, g.U2, (g.p1 - g.p0 + UMPA_WIDEN_SEG - 1) / UMPA_WIDEN_SEG);
    const bool strip = g.strip_w > 0;
#define UMPA_LEVELS_CASE(A, B, C) case A * 100 + B * 10 + C: \
        if (strip) hipLaunchKernelGGL((levels_table_kernel<A, B, C, true>), grd, dim3(64), 0, s, table, carry, pools[0], pools[1], pools[2], g); \
        else hipLaunchKernelGGL((levels_table_kernel<A, B, C, false>), grd, dim3(64), 0, s, table, carry, pools[0], pools[1], pools[2], g); \
        return true;
    switch (hb[0] * 100 + hb[1] * 10 + (nw > 2 ? hb[2] : 0)) {
        UMPA_LEVELS_CASE(2, 1, 0) UMPA_LEVELS_CASE(4, 1, 0) UMPA_LEVELS_CASE(4, 2, 0)
        UMPA_LEVELS_CASE(8, 1, 0) UMPA_LEVELS_CASE(8, 2, 0) UMPA_LEVELS_CASE(8, 4, 0)
        UMPA_LEVELS_CASE(4, 2, 1) UMPA_LEVELS_CASE(8, 2, 1) UMPA_LEVELS_CASE(8, 4, 1) UMPA_LEVELS_CASE(8, 4, 2)
    }
#undef UMPA_LEVELS_CASE
    return false;
}

// Scale-space search, one row chunk (umpa_levels_geom.h has the row arithmetic): every widened level's pooled table of the
// rows [drow0 - bmax, drow0 + drows - bmax) from one read of the raw rows, then level after level the prior and
// grid_track_kernel on those rows, then the selection, then the carry for the next chunk.
hipError_t levels_chunk(GridJob& J, const ModelDev& dev, const Maps& M, const ReplayArgs& R, const RegionArgs& A, hipStream_t s)
{
    const int bmax = J.lb[0], U = 2 * dev.ms - 1, KP = (dev.Na + 1) / 2;
    const bool df = M.WS != nullptr;
    int nw = 0;
    for (int l = 0; l < J.L; l++) nw += J.lb[l] > 0 ? 1 : 0;
    if (J.want_df && !df) { J.refused = "track: a dark-field map (df) needs the dark-field model"; return hipErrorInvalidValue; }
    if (grid_basins_lds(dev.ms) > 64 * 1024) { J.refused = "track: the search box does not fit the kernel's ring of cost rows"; return hipErrorInvalidValue; }
    const size_t n = (size_t)A.N0 * A.N1;
    if (J.host && !J.block) {
        if (hipMalloc(&J.block, levels_bytes(J.L, n)) != hipSuccess) { J.block = nullptr; return hipErrorOutOfMemory; }
        levels_carve(J, J.block, n);
    }
    WidenGeom g;
    g.b = bmax; g.U2 = U * U;
    g.N0d = A.step0 * (A.N0 - 1) + 1; g.N1d = A.step1 * (A.N1 - 1) + 1;
    g.drow0 = R.drow0; g.drows = R.drows; g.crows = R.drow0 == 0 ? 0 : 2 * bmax;
    g.strip_w = R.strip_w; g.tw = R.tw; g.N1p = R.N1d; g.N1q = (g.N1d + 31) / 32 * 32;
    widen_rows(bmax, g.N0d, g.drow0, g.drows, g.p0, g.p1);
    const bool last = R.drow0 + R.drows >= g.N0d;
    if (R.drow0 != J.next_drow0 || (!last && R.drows < 2 * bmax)) { J.refused = "levels: the row chunks do not follow each other"; return hipErrorInvalidValue; }
    const size_t plane = (size_t)M.H * M.W, nmap = (2 + (df ? 4 * (size_t)KP : 0)) * plane;
    if (!J.ws) {
        J.pool_rows = std::min(g.N0d, g.drows + bmax);
        if ((size_t)J.pool_rows * g.N1q >= ((size_t)1 << 32)) { J.refused = "levels: a plane of the pooled table passes the 32-bit stride of the lookups"; return hipErrorInvalidValue; }
        const size_t pool_len = (size_t)g.U2 * J.pool_rows * g.N1q, carry_len = (last || bmax == 0) ? 0 : widen_table_len(g, 2 * bmax);
        hipError_t e = hipMallocAsync(&J.ws, ((size_t)nw * (pool_len + nmap) + carry_len + 2 * n) * sizeof(double), s);
        if (e != hipSuccess) { J.ws = nullptr; return hipErrorOutOfMemory; }
        J.ws_stream = s;
        double* q = (double*)J.ws;
        for (int w = 0; w < nw; w++) { J.pools[w] = q; q += pool_len; }
        J.carry = q; q += carry_len;
        for (int w = 0; w < nw; w++) { J.lmaps[w] = q; q += nmap; }
        J.prior = q;
        for (int w = 0; w < nw; w++)                                   // (the widened levels come first in the list)
            if ((e = widen_maps(J.lb[w], dev, M, A, g.N0d, g.N1d, J.lmaps[w], s)) != hipSuccess) return e;
    }
    if (g.p1 - g.p0 > J.pool_rows) { J.refused = "levels: a row chunk larger than the first"; return hipErrorInvalidValue; }
    if (g.p1 > g.p0 && nw == 1) widen_table(g, R.table, J.carry, J.pools[0], s);   // g.b is that level's half-width
    else if (g.p1 > g.p0 && nw > 1 && !levels_table(g, J.lb, nw, R.table, J.carry, J.pools, s)) {
        J.refused = "levels: no pooling kernel for this list of half-widths"; return hipErrorInvalidValue;
    }
    int row0, rows;
    levels_out_rows(g.p0, g.p1, A.step0, A.N0, row0, rows);
    const unsigned blocks = (unsigned)(((size_t)rows * A.N1 + 255) / 256);
    for (int l = 0; l < J.L && rows > 0 && A.N1 > 0; l++) {
        const size_t at = (size_t)l * n, pv = l > 0 ? at - n : 0;
        hipLaunchKernelGGL(levels_prior_kernel, dim3(blocks), dim3(256), 0, s, l > 0 ? (const double*)J.lev.dx + pv : nullptr,
                           l > 0 ? (const double*)J.lev.dy + pv : nullptr, l > 0 ? (const int*)J.lev.err + pv : nullptr,
                           J.prior, J.prior + n, A.N1, row0, rows);
        J.K.pi = J.prior; J.K.pj = J.prior + n;
        J.K.f = J.lev.f + at; J.K.T = J.lev.T + at; J.K.dx = J.lev.dx + at; J.K.dy = J.lev.dy + at; J.K.cost = J.lev.cost + at;
        J.K.df = J.lev.df ? J.lev.df + at : nullptr; J.K.cost0 = J.lev.cost0 + at;
        J.K.si = J.lev.si + at; J.K.sj = J.lev.sj + at; J.K.err = J.lev.err + at; J.K.count = J.lev.count + at; J.K.found = J.lev.found + at;
        hipError_t e = hipSuccess;
        if (J.lb[l] > 0) {                                            // widen_chunk's Mw, Rw: the level's pooled maps and table
            Maps Mw = M;
            ReplayArgs Rw = R;
            Mw.SamSq = J.lmaps[l]; Mw.RefSq = J.lmaps[l] + plane;
            Mw.WS = df ? J.lmaps[l] + 2 * plane : nullptr;
            Mw.MR = df ? J.lmaps[l] + (2 + 2 * (size_t)KP) * plane : nullptr;
            Rw.table = J.pools[l]; Rw.slot_stride = (size_t)(g.p1 - g.p0) * g.N1q; Rw.drow0 = g.p0; Rw.N1d = g.N1q;
            Rw.strip_w = 0; Rw.tw = 0; Rw.drows = g.p1 - g.p0;
            Rw.bw_log2 = 4;
            Rw.row0 = row0; Rw.rows = rows;
            e = dispatch(J, dev, Mw, Rw, A, s);
        } else {                                                      // the model's own window: the raw rows, of the carry and of the chunk
            int c0, c1, t0, t1;
            levels_plain_rows(g, c0, c1, t0, t1);
            ReplayArgs Rc = R, Rt = R;
            Rc.table = J.carry; Rc.drow0 = g.drow0 - g.crows; Rc.drows = g.crows;
            if (R.strip_w == 0) Rc.slot_stride = (size_t)g.crows * g.N1p;
            levels_out_rows(c0, c1, A.step0, A.N0, Rc.row0, Rc.rows);
            levels_out_rows(t0, t1, A.step0, A.N0, Rt.row0, Rt.rows);
            e = dispatch(J, dev, M, Rc, A, s);
            if (e == hipSuccess) e = dispatch(J, dev, M, Rt, A, s);
        }
        if (e != hipSuccess) return e;
    }
    if (J.want_sel && rows > 0 && A.N1 > 0) {
        LevelsSelectArgs a;
        a.lev = J.lev; a.sel = J.sel; a.level = J.sel_level; a.halfwidth = J.sel_hw;
        a.plane = n; a.L = J.L; a.N1 = A.N1; a.row0 = row0; a.rows = rows;
        for (int l = 0; l < UMPA_LEVELS_MAX; l++) { a.b[l] = J.lb[l]; a.tol[l] = J.ltol[l]; }
        hipLaunchKernelGGL(levels_select_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
    if (!last && bmax > 0) {
        const WidenCarryCopy cc = widen_carry_copy(g);
        hipLaunchKernelGGL(widen_carry_kernel, dim3((unsigned)((cc.run + 255) / 256), (unsigned)cc.nruns), dim3(256), 0, s, R.table, J.carry, cc);
    }
    J.next_drow0 = R.drow0 + R.drows;
    return hipGetLastError();
}

hipError_t consumer(void* user, const ModelDev& dev, const Maps& M0, const ReplayArgs& R0, const RegionArgs& A0, hipStream_t s)
{
    GridJob& J = *(GridJob*)user;
    Maps M = M0;
    ReplayArgs R = R0;
    RegionArgs A = A0;
    const int kind = J.masked ? (J.masked == 3 ? 1 : 0) : M.WS ? 1 : 0;
    if (J.L > 0) return levels_chunk(J, dev, M0, R0, A0, s);
    if (J.mhost) {
        const size_t n = (size_t)A.N0 * A.N1;
        if (!J.mblock) {
            J.mh.nparam = A.nparam;
            if (hipMalloc(&J.mblock, match_carve(J.md, J.mh, nullptr, n)) != hipSuccess) { J.mblock = nullptr; return hipErrorOutOfMemory; }
            (void)match_carve(J.md, J.mh, J.mblock, n);
            if (J.mh.cover) {                                         // pixels under the threshold keep what the caller's arrays hold
                hipError_t e = hipMemcpy(J.md.values, J.mh.values, n * A.nparam * sizeof(double), hipMemcpyHostToDevice);
                if (e == hipSuccess) e = hipMemcpy(J.md.err, J.mh.err, n * sizeof(int), hipMemcpyHostToDevice);
                if (e == hipSuccess) e = hipMemcpy((void*)J.md.cover, J.mh.cover, n * sizeof(double), hipMemcpyHostToDevice);
                if (e == hipSuccess && J.md.dbg_d) e = hipMemset(J.md.dbg_d, 0, n * 25 * sizeof(double));
                if (e == hipSuccess && J.md.dbg_a) e = hipMemset(J.md.dbg_a, 0, n * 16 * sizeof(double));
                if (e == hipSuccess && J.md.dbg_n) e = hipMemset(J.md.dbg_n, 0, n * sizeof(int));
                if (e != hipSuccess) return e;
            }
        }
        A.values = J.md.values; A.err = J.md.err; A.cover = J.md.cover;
        A.dbg_d = J.md.dbg_d; A.dbg_a = J.md.dbg_a; A.dbg_n = J.md.dbg_n;
    }
    if (J.volume) {
        if (J.want[2] && kind != 1) { J.refused = "a dark-field volume needs the dark-field model"; return hipErrorInvalidValue; }
        const int U = 2 * dev.ms - 1;
        J.V.plane = (size_t)A.N0 * A.N1;
        if (J.host && J.count == 0) {
            J.count = (size_t)U * U * J.V.plane;
            for (int q = 0; q < 3; q++)
                if (J.want[q] && hipMalloc((void**)&J.dev[q], J.count * sizeof(double)) != hipSuccess) { J.dev[q] = nullptr; return hipErrorOutOfMemory; }
            J.V.cost = J.dev[0]; J.V.T = J.dev[1]; J.V.df = J.dev[2];
        }
    }
    if (J.basins) {
        if (J.want_df && kind != 1) { J.refused = "basins: a dark-field map (df) needs the dark-field model"; return hipErrorInvalidValue; }
        if (grid_basins_lds(dev.ms) > 64 * 1024) { J.refused = "basins: the search box does not fit the kernel's ring of cost rows"; return hipErrorInvalidValue; }
        J.B.plane = (size_t)A.N0 * A.N1;
        if (J.host && !J.block) {
            if (hipMalloc(&J.block, basins_bytes(J.B.plane, J.B.K)) != hipSuccess) { J.block = nullptr; return hipErrorOutOfMemory; }
            basins_carve(J.B, J.block, J.B.plane, J.B.K, J.want_df);
        }
    }
    if (J.track) {
        if (J.want_df && kind != 1) { J.refused = "track: a dark-field map (df) needs the dark-field model"; return hipErrorInvalidValue; }
        if (grid_basins_lds(dev.ms) > 64 * 1024) { J.refused = "track: the search box does not fit the kernel's ring of cost rows"; return hipErrorInvalidValue; }
        if (J.host && !J.block) {
            const size_t plane = (size_t)A.N0 * A.N1;
            if (hipMalloc(&J.block, track_bytes(plane)) != hipSuccess) { J.block = nullptr; return hipErrorOutOfMemory; }
            track_carve(J.K, J.block, plane, J.want_df);
            hipError_t e = hipMemcpy((void*)J.K.pi, J.host_pi, plane * sizeof(double), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy((void*)J.K.pj, J.host_pj, plane * sizeof(double), hipMemcpyHostToDevice);
            if (e != hipSuccess) return e;
        }
    }
    if (J.sequence) {
        if (dev.ms < 2 || dev.ms > UMPA_GRID_SEQUENCE_MAX_SHIFT) {
            char text[128];
            snprintf(text, sizeof(text), "sequence: max_shift must be 2 to %d, not %d", UMPA_GRID_SEQUENCE_MAX_SHIFT, dev.ms);
            J.refused_text = text; J.refused = J.refused_text.c_str(); J.refused_code = UMPA_HIP_E_UNSUPPORTED;
            return hipErrorInvalidValue;
        }
        if (J.want_df && kind != 1) { J.refused = "sequence: a dark-field map (df) needs the dark-field model"; return hipErrorInvalidValue; }
        const int U = 2 * dev.ms - 1;
        const size_t plane = (size_t)A.N0 * A.N1;
        J.Q.plane = plane;
        J.Q.half = sequence_half(dev.ms);
        J.state_len = (size_t)U * U * plane;
        if (J.host && !J.block) {
            if (hipMalloc(&J.block, sequence_bytes(plane, U * U, J.host_prev != nullptr, J.want_next)) != hipSuccess) { J.block = nullptr; return hipErrorOutOfMemory; }
            sequence_carve(J.Q, J.block, plane, U * U, J.host_prev != nullptr, J.want_next, J.want_df);
            if (J.host_prev) {
                const hipError_t e = hipMemcpy((void*)J.Q.prev, J.host_prev, J.state_len * sizeof(double), hipMemcpyHostToDevice);
                if (e != hipSuccess) return e;
            }
        }
    }
    if (J.b > 0) {
        const hipError_t e = widen_chunk(J, dev, M0, R0, A, s, M, R);
        if (e != hipSuccess) return e;
    }
    return dispatch(J, dev, M, R, A, s);
}

const char* const FINISHED_COST = "a finished cost is not linear in the windowed sums, so a box average of costs is not the cost under a wider window";

template <int KIND, bool MASK>
void launch_general(const ModelDev& dev, const RegionArgs& A, const GeneralArgs& T, const StagedGeom& G, size_t lds, hipStream_t s)
{
    const dim3 grd((A.N1 + UMPA_STAGED_BX - 1) / UMPA_STAGED_BX, (T.rows + UMPA_STAGED_BY - 1) / UMPA_STAGED_BY);
    hipLaunchKernelGGL((general_table_kernel<KIND, MASK>), grd, dim3(UMPA_STAGED_BX, UMPA_STAGED_BY), T.staged ? lds : 0, s, dev, A, T, G);
}

// The general consumer (umpa_hipx_set_general_consumer): the match entry point calls it once, with the full region, where a
// table consumer is set and no tiled path takes the model and the region whole.  Per row chunk of the region -- as many
// output rows as the tiled paths' table budget holds (UMPA_HIP_TABLE_MB) -- general_table_kernel fills a table of finished
// costs on the OUTPUT grid (umpa_general_table_kernels.h), and the call's consumer runs on it as on the masked path's: the
// ReplayArgs of that path, GridJob::masked = NV, and the region with unit steps (the masked kernels use the steps only to
// find a pixel in the table).
hipError_t general(void* user, const ModelDev& dev, int kind, int has_mask, const RegionArgs& A, hipStream_t s)
{
    GridJob& J = *(GridJob*)user;
    if (J.b > 0 || J.L > 0) {
        J.refused_text = std::string("window widening and scale space are not built for the general table (umpa_grid_set_general): it "
                                     "holds finished costs, and ") + FINISHED_COST;
        J.refused = J.refused_text.c_str(); J.refused_code = UMPA_HIP_E_UNSUPPORTED;
        return hipErrorInvalidValue;
    }
    if (A.N0 <= 0 || A.N1 <= 0 || dev.ms < 1) return hipSuccess;
    const int U = 2 * dev.ms - 1, NV = kind == UMPA_HIP_KIND_DF ? 3 : 2;
    const TiledEnv E = tiled_env();
    const size_t per_row = (size_t)U * U * NV * A.N1;                 // doubles per output row
    long rows_chunk = (long)(E.table_bytes / (per_row * sizeof(double))) / UMPA_STAGED_BY * UMPA_STAGED_BY;
    if (rows_chunk < UMPA_STAGED_BY) rows_chunk = UMPA_STAGED_BY;
    if (rows_chunk > A.N0) rows_chunk = A.N0;
    if (hipMallocAsync(&J.gtable, per_row * rows_chunk * sizeof(double), s) != hipSuccess) { J.gtable = nullptr; return hipErrorOutOfMemory; }
    J.gstream = s;
    J.masked = NV;
    StagedGeom G = {};
    size_t lds = 0;
    const bool staged = general_geometry(dev, has_mask != 0, A, G, lds);
    RegionArgs Au = A;                                                // the table lies on the output grid
    Au.step0 = 1; Au.step1 = 1;
    const Maps none = {};
    for (int row0 = 0; row0 < A.N0; row0 += (int)rows_chunk) {
        const int rows = std::min((int)rows_chunk, A.N0 - row0);
        GeneralArgs T;
        T.table = (double*)J.gtable; T.slot_stride = (size_t)rows * A.N1; T.row0 = row0; T.rows = rows; T.staged = staged ? 1 : 0;
        if (kind == UMPA_HIP_KIND_DF) { if (has_mask) launch_general<1, true>(dev, A, T, G, lds, s); else launch_general<1, false>(dev, A, T, G, lds, s); }
        else { if (has_mask) launch_general<0, true>(dev, A, T, G, lds, s); else launch_general<0, false>(dev, A, T, G, lds, s); }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ReplayArgs R;
        memset(&R, 0, sizeof(R));
        R.table = T.table; R.slot_stride = T.slot_stride; R.drow0 = row0; R.N1d = A.N1;
        R.strip_w = 0; R.tw = 0; R.drows = rows;
        R.row0 = row0; R.rows = rows;
        R.bw_log2 = 4;
        if ((e = consumer(user, dev, none, R, Au, s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// umpa_hip_match_region down the tiled path with `J` as the model's table consumer; the consumer is cleared whatever happens
int run(umpa_hip_model* m, GridJob& J, int start0, int step0, int N0, int start1, int step1, int N1,
        double* values, int nparam, int* err, const double* covermap, double thr,
        double* dbg_d, double* dbg_a, int* dbg_n, int flags, void* stream)
{
    J.masked = umpa_hipx_masked_table(m);
    if (J.masked && (J.b > 0 || J.L > 0))
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: window widening and scale space are not built for masked models: the table of a masked "
                                            "model holds finished costs, and a finished cost is not linear in the windowed sums, so a box "
                                            "average of costs is not the cost under a wider window");
    if (int rc = umpa_hipx_set_table_consumer(m, consumer, &J)) return fail(rc, "%s", umpa_hip_last_error());
    const int rc = umpa_hip_match_region(m, start0, step0, N0, start1, step1, N1, values, nparam, nullptr, err, covermap, thr,
                                         dbg_d, dbg_a, dbg_n, flags | UMPA_HIP_F_FORCE_TILED, stream);
    (void)umpa_hipx_set_table_consumer(m, nullptr, nullptr);
    if (J.ws) { (void)hipFreeAsync(J.ws, J.ws_stream); J.ws = nullptr; }   // (widening) behind the call's last kernel on its stream
    if (J.gtable) { (void)hipFreeAsync(J.gtable, J.gstream); J.gtable = nullptr; }   // (the general table) likewise
    if (rc < 0) return fail(J.refused && J.refused_code ? J.refused_code : rc, "grid: %s", J.refused ? J.refused : umpa_hip_last_error());
    return rc;
}

// The entry points, each with the half-width `b` of the widening box: 0 for umpa_grid_<name>, whose checks and texts these
// are; umpa_grid_wide_<name> has checked `b` before.
int match_region(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                 double* values, int nparam, double* uv, int* err, const double* covermap, double cover_threshold,
                 double* dbg_d, double* dbg_a, int* dbg_ncalls, int flags, void* stream)
{
    if (!m) return fail(UMPA_HIP_E_ARG, "grid: null model");
    if (uv) return fail(UMPA_HIP_E_ARG, "grid search takes no start shifts (uv must be NULL)");
    GridJob J;
    J.b = b;
    if (b == 0 || (flags & UMPA_HIP_F_DEVICE_IO))
        return run(m, J, start0, step0, N0, start1, step1, N1, values, nparam, err, covermap, cover_threshold,
                   dbg_d, dbg_a, dbg_ncalls, flags, stream);
    // widened, host arrays (GridJob::mhost): the match entry point sees device I/O on the null stream, the consumer swaps
    // in its block; the maps are complete when the call returns, so UMPA_HIP_F_ASYNC has nothing left to wait for
    J.mhost = true;
    J.mh.values = values; J.mh.err = err; J.mh.cover = covermap; J.mh.dbg_d = dbg_d; J.mh.dbg_a = dbg_a; J.mh.dbg_n = dbg_ncalls;
    int rc = run(m, J, start0, step0, N0, start1, step1, N1, values, nparam, err, covermap, cover_threshold,
                 dbg_d, dbg_a, dbg_ncalls, (flags & ~UMPA_HIP_F_ASYNC) | UMPA_HIP_F_DEVICE_IO, nullptr);
    if (!J.mblock) return rc;                                         // refused before the consumer ran: nothing was enqueued
    hipError_t e = hipSuccess;
    if (rc >= 0) {
        const size_t n = (size_t)N0 * N1;
        const struct { void* host; const void* dev; size_t bytes; } copies[5] = {
            {values, J.md.values, n * nparam * sizeof(double)}, {err, J.md.err, n * sizeof(int)}, {dbg_d, J.md.dbg_d, n * 25 * sizeof(double)},
            {dbg_a, J.md.dbg_a, n * 16 * sizeof(double)}, {dbg_ncalls, J.md.dbg_n, n * sizeof(int)}};
        for (int q = 0; q < 5 && e == hipSuccess; q++)
            if (copies[q].host && copies[q].dev) e = hipMemcpy(copies[q].host, copies[q].dev, copies[q].bytes, hipMemcpyDeviceToHost);
    }
    if (rc < 0 || e != hipSuccess) (void)hipDeviceSynchronize();      // nothing of this call may still use the block freed here
    (void)hipFree(J.mblock);
    if (rc >= 0 && e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: download of the result maps: %s", hipGetErrorString(e));
    return rc;
}

int cost_volume(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                double* cost, double* T, double* df, int flags, void* stream)
{
    if (!m || !cost) return fail(UMPA_HIP_E_ARG, "grid: null argument");
    if (flags & ~(UMPA_HIP_F_DEVICE_IO | UMPA_HIP_F_USE_STAGED))
        return fail(UMPA_HIP_E_ARG, "grid: cost_volume takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag");
    // a staged sample stack is adopted by the match entry point underneath, as by any match: the volume is then that stack's
    const int staged = flags & UMPA_HIP_F_USE_STAGED;
    GridJob J;
    J.b = b;
    J.volume = true;
    // the match entry point wants value and status arrays; this consumer's kernel touches neither, and with device I/O the
    // entry point hands the pointers to the kernels as they are, nothing is copied, seeded or cleared (noted at that branch
    // of umpa_hip_match_region): placeholders
    double* const no_values = cost;
    int* const no_err = (int*)cost;
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        J.V.cost = cost; J.V.T = T; J.V.df = df;
        J.want[2] = df != nullptr;
        return run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                   UMPA_HIP_F_DEVICE_IO | staged, stream);
    }
    // host arrays: device copies for the duration of the call, allocated by the consumer (the model's device is current
    // there and stays this thread's current device afterwards), filled on that device's null stream
    J.host = true; J.want[0] = true; J.want[1] = T != nullptr; J.want[2] = df != nullptr;
    int rc = run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                 UMPA_HIP_F_DEVICE_IO | staged, nullptr);
    double* const host[3] = {cost, T, df};
    hipError_t e = hipSuccess;
    for (int q = 0; q < 3 && rc >= 0 && e == hipSuccess; q++)
        if (J.dev[q]) e = hipMemcpy(host[q], J.dev[q], J.count * sizeof(double), hipMemcpyDeviceToHost);
    if (J.dev[0] || J.dev[1] || J.dev[2]) {                           // (none: refused before the consumer ran, nothing was enqueued)
        if (rc < 0 || e != hipSuccess) (void)hipDeviceSynchronize();  // nothing of this call may still use the arrays freed here
        for (int q = 0; q < 3; q++) if (J.dev[q]) (void)hipFree(J.dev[q]);
    }
    if (rc >= 0 && e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: download of the cost volume: %s", hipGetErrorString(e));
    return rc;
}

int basins(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b, int K,
           double* f, double* T, double* dx, double* dy, double* cost, double* df,
           int* si, int* sj, int* err, int* count, int flags, void* stream)
{
    if (!m || !f || !T || !dx || !dy || !cost || !si || !sj || !err || !count) return fail(UMPA_HIP_E_ARG, "grid: basins: null argument");
    if (K < 1 || K > UMPA_GRID_MAX_BASINS)
        return fail(UMPA_HIP_E_ARG, "grid: basins keeps 1 to %d basins per pixel, not %d", UMPA_GRID_MAX_BASINS, K);
    if (flags & ~(UMPA_HIP_F_DEVICE_IO | UMPA_HIP_F_USE_STAGED))
        return fail(UMPA_HIP_E_ARG, "grid: basins takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag");
    const int staged = flags & UMPA_HIP_F_USE_STAGED;
    GridJob J;
    J.b = b;
    J.basins = true;
    J.B.K = K;
    J.want_df = df != nullptr;
    // value and status placeholders for the match entry point, as in umpa_grid_cost_volume: with device I/O nothing reads,
    // seeds or clears them
    double* const no_values = cost;
    int* const no_err = (int*)cost;
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        J.B.f = f; J.B.T = T; J.B.dx = dx; J.B.dy = dy; J.B.cost = cost; J.B.df = df;
        J.B.si = si; J.B.sj = sj; J.B.err = err; J.B.count = count;
        return run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                   UMPA_HIP_F_DEVICE_IO | staged, stream);
    }
    // host arrays: one device block for the duration of the call, allocated by the consumer on the model's device (which
    // stays this thread's current device), filled on that device's null stream
    J.host = true;
    int rc = run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                 UMPA_HIP_F_DEVICE_IO | staged, nullptr);
    if (!J.block) return rc;                                          // refused before the consumer ran: nothing was enqueued
    hipError_t e = hipSuccess;
    if (rc >= 0) {
        const size_t kp = (size_t)K * J.B.plane;
        const struct { void* host; const void* dev; size_t bytes; } copies[10] = {
            {f, J.B.f, kp * sizeof(double)}, {T, J.B.T, kp * sizeof(double)}, {dx, J.B.dx, kp * sizeof(double)},
            {dy, J.B.dy, kp * sizeof(double)}, {cost, J.B.cost, kp * sizeof(double)}, {df, J.B.df, kp * sizeof(double)},
            {si, J.B.si, kp * sizeof(int)}, {sj, J.B.sj, kp * sizeof(int)}, {err, J.B.err, kp * sizeof(int)},
            {count, J.B.count, J.B.plane * sizeof(int)}};
        for (int q = 0; q < 10 && e == hipSuccess; q++)
            if (copies[q].host && copies[q].dev) e = hipMemcpy(copies[q].host, copies[q].dev, copies[q].bytes, hipMemcpyDeviceToHost);
    }
    if (rc < 0 || e != hipSuccess) (void)hipDeviceSynchronize();      // nothing of this call may still use the block freed here
    (void)hipFree(J.block);
    if (rc >= 0 && e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: download of the basins: %s", hipGetErrorString(e));
    return rc;
}

int track(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
          const double* prior_i, const double* prior_j, int mode, double lam, double radius,
          double* f, double* T, double* dx, double* dy, double* cost, double* df,
          int* si, int* sj, int* err, double* cost0, int* count, int* found, int flags, void* stream)
{
    if (!m || !prior_i || !prior_j || !f || !T || !dx || !dy || !cost || !si || !sj || !err || !cost0 || !count || !found)
        return fail(UMPA_HIP_E_ARG, "grid: track: null argument");
    if (mode != UMPA_GRID_TRACK_NEAREST && mode != UMPA_GRID_TRACK_PENALTY)
        return fail(UMPA_HIP_E_ARG, "grid: track: mode must be UMPA_GRID_TRACK_NEAREST (0) or UMPA_GRID_TRACK_PENALTY (1), not %d", mode);
    if (mode == UMPA_GRID_TRACK_PENALTY && !(lam >= 0.0 && lam < __builtin_inf()))
        return fail(UMPA_HIP_E_ARG, "grid: track: lam must be finite and not negative");
    if (radius != radius) return fail(UMPA_HIP_E_ARG, "grid: track: radius must not be NaN");
    if (flags & ~(UMPA_HIP_F_DEVICE_IO | UMPA_HIP_F_USE_STAGED))
        return fail(UMPA_HIP_E_ARG, "grid: track takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag");
    const int staged = flags & UMPA_HIP_F_USE_STAGED;
    GridJob J;
    J.b = b;
    J.track = true;
    J.want_df = df != nullptr;
    J.K.mode = mode;
    J.K.lam = mode == UMPA_GRID_TRACK_PENALTY ? lam : 0.0;
    J.K.limited = radius < 0.0 ? 0 : 1;
    J.K.r2 = radius < 0.0 ? 0.0 : radius * radius;
    // value and status placeholders for the match entry point, as in umpa_grid_cost_volume: with device I/O nothing reads,
    // seeds or clears them
    double* const no_values = cost;
    int* const no_err = (int*)cost;
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        J.K.pi = prior_i; J.K.pj = prior_j;
        J.K.f = f; J.K.T = T; J.K.dx = dx; J.K.dy = dy; J.K.cost = cost; J.K.df = df; J.K.cost0 = cost0;
        J.K.si = si; J.K.sj = sj; J.K.err = err; J.K.count = count; J.K.found = found;
        return run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                   UMPA_HIP_F_DEVICE_IO | staged, stream);
    }
    // host arrays: one device block for the duration of the call, allocated and given the priors by the consumer on the
    // model's device (which stays this thread's current device), filled on that device's null stream
    J.host = true;
    J.host_pi = prior_i; J.host_pj = prior_j;
    int rc = run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                 UMPA_HIP_F_DEVICE_IO | staged, nullptr);
    if (!J.block) return rc;                                          // refused before the consumer ran: nothing was enqueued
    hipError_t e = hipSuccess;
    if (rc >= 0) {
        const size_t plane = (size_t)N0 * N1;
        const struct { void* host; const void* dev; size_t bytes; } copies[12] = {
            {f, J.K.f, plane * sizeof(double)}, {T, J.K.T, plane * sizeof(double)}, {dx, J.K.dx, plane * sizeof(double)},
            {dy, J.K.dy, plane * sizeof(double)}, {cost, J.K.cost, plane * sizeof(double)}, {df, J.K.df, plane * sizeof(double)},
            {cost0, J.K.cost0, plane * sizeof(double)},
            {si, J.K.si, plane * sizeof(int)}, {sj, J.K.sj, plane * sizeof(int)}, {err, J.K.err, plane * sizeof(int)},
            {count, J.K.count, plane * sizeof(int)}, {found, J.K.found, plane * sizeof(int)}};
        for (int q = 0; q < 12 && e == hipSuccess; q++)
            if (copies[q].host && copies[q].dev) e = hipMemcpy(copies[q].host, copies[q].dev, copies[q].bytes, hipMemcpyDeviceToHost);
    }
    if (rc < 0 || e != hipSuccess) (void)hipDeviceSynchronize();      // nothing of this call may still use the block freed here
    (void)hipFree(J.block);
    if (rc >= 0 && e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: download of the track maps: %s", hipGetErrorString(e));
    return rc;
}

int sequence(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
             const double* prev, double lam, double trunc, double* next,
             double* f, double* T, double* dx, double* dy, double* cost, double* df,
             int* si, int* sj, int* err, double* total, double* cost0, int* moved, int flags, void* stream)
{
    if (!m) return fail(UMPA_HIP_E_ARG, "grid: sequence: null model");
    if (!f || !T || !dx || !dy || !cost || !si || !sj || !err || !total || !cost0 || !moved)
        return fail(UMPA_HIP_E_ARG, "grid: sequence: null output plane (only df and next may be NULL)");
    if (!(lam >= 0.0 && lam < __builtin_inf())) return fail(UMPA_HIP_E_ARG, "grid: sequence: lam must be finite and not negative, not %g", lam);
    if (!(trunc >= 0.0)) return fail(UMPA_HIP_E_ARG, "grid: sequence: trunc must be >= 0 or +Inf, not %g", trunc);
    if (flags & ~(UMPA_HIP_F_DEVICE_IO | UMPA_HIP_F_USE_STAGED))
        return fail(UMPA_HIP_E_ARG, "grid: sequence takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag, not 0x%x", (unsigned)flags);
    const int staged = flags & UMPA_HIP_F_USE_STAGED;
    GridJob J;
    J.sequence = true;
    J.want_df = df != nullptr;
    J.want_next = next != nullptr;
    J.Q.lam = lam; J.Q.trunc = trunc;
    // value and status placeholders for the match entry point, as in umpa_grid_cost_volume: with device I/O nothing reads,
    // seeds or clears them
    double* const no_values = cost;
    int* const no_err = (int*)cost;
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        J.Q.prev = prev; J.Q.next = next;
        J.Q.f = f; J.Q.T = T; J.Q.dx = dx; J.Q.dy = dy; J.Q.cost = cost; J.Q.df = df; J.Q.total = total; J.Q.cost0 = cost0;
        J.Q.si = si; J.Q.sj = sj; J.Q.err = err; J.Q.moved = moved;
        return run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                   UMPA_HIP_F_DEVICE_IO | staged, stream);
    }
    // host arrays: one device block for the duration of the call, allocated and given the previous state by the consumer on
    // the model's device (which stays this thread's current device), filled on that device's null stream
    J.host = true;
    J.host_prev = prev;
    int rc = run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                 UMPA_HIP_F_DEVICE_IO | staged, nullptr);
    if (!J.block) return rc;                                          // refused before the consumer allocated: nothing was enqueued
    hipError_t e = hipSuccess;
    if (rc >= 0) {
        const size_t plane = (size_t)N0 * N1;
        const struct { void* host; const void* dev; size_t bytes; } copies[13] = {
            {next, J.Q.next, J.state_len * sizeof(double)},
            {f, J.Q.f, plane * sizeof(double)}, {T, J.Q.T, plane * sizeof(double)}, {dx, J.Q.dx, plane * sizeof(double)},
            {dy, J.Q.dy, plane * sizeof(double)}, {cost, J.Q.cost, plane * sizeof(double)}, {df, J.Q.df, plane * sizeof(double)},
            {total, J.Q.total, plane * sizeof(double)}, {cost0, J.Q.cost0, plane * sizeof(double)},
            {si, J.Q.si, plane * sizeof(int)}, {sj, J.Q.sj, plane * sizeof(int)}, {err, J.Q.err, plane * sizeof(int)},
            {moved, J.Q.moved, plane * sizeof(int)}};
        for (int q = 0; q < 13 && e == hipSuccess; q++)
            if (copies[q].host && copies[q].dev) e = hipMemcpy(copies[q].host, copies[q].dev, copies[q].bytes, hipMemcpyDeviceToHost);
    }
    if (rc < 0 || e != hipSuccess) (void)hipDeviceSynchronize();      // nothing of this call may still use the block freed here
    (void)hipFree(J.block);
    if (rc >= 0 && e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: download of the sequence maps and state: %s", hipGetErrorString(e));
    return rc;
}

// `b` outside 0 .. UMPA_GRID_MAX_WIDEN
int bad_widen(int b) { return fail(UMPA_HIP_E_ARG, "grid: widen: the half-width b must be 0 to %d, not %d", UMPA_GRID_MAX_WIDEN, b); }

// the list of half-widths as the refusal shows it: "(4, 2, 3)"
std::string levels_text(int L, const int* b)
{
    std::string t = "(";
    for (int l = 0; l < L; l++) t += (l ? ", " : "") + std::to_string(b[l]);
    return t + ")";
}

int levels_track(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                 int L, const int* b, int mode, double lam, double radius, const double* tol,
                 const LevelsPlanes& lev, const LevelsPlanes& sel, int* level, int* halfwidth, int flags, void* stream)
{
    if (!m || !b || !lev.f || !lev.T || !lev.dx || !lev.dy || !lev.cost || !lev.si || !lev.sj || !lev.err || !lev.cost0 || !lev.count || !lev.found)
        return fail(UMPA_HIP_E_ARG, "grid: levels: null argument");
    if (L < 1 || L > UMPA_GRID_MAX_LEVELS) return fail(UMPA_HIP_E_ARG, "grid: levels: 1 to %d levels, not %d", UMPA_GRID_MAX_LEVELS, L);
    if (levels_check(L, b))
        return fail(UMPA_HIP_E_ARG, "grid: levels: the half-widths must decrease, the widened ones from {1, 2, 4, 8} and at most three, "
                                    "a 0 only at the end, not %s", levels_text(L, b).c_str());
    for (int l = 0; tol && l < L; l++)
        if (!(tol[l] >= 0.0)) return fail(UMPA_HIP_E_ARG, "grid: levels: tol[%d] must be >= 0 or +Inf", l);
    const int given = (sel.f != nullptr) + (sel.T != nullptr) + (sel.dx != nullptr) + (sel.dy != nullptr) + (sel.cost != nullptr) + (sel.si != nullptr)
        + (sel.sj != nullptr) + (sel.err != nullptr) + (sel.cost0 != nullptr) + (sel.count != nullptr) + (sel.found != nullptr) + (level != nullptr) + (halfwidth != nullptr);
    if ((given != 0 && given != 13) || (given == 0 && sel.df))
        return fail(UMPA_HIP_E_ARG, "grid: levels: the selected arrays must be all given or all NULL");
    if (mode != UMPA_GRID_TRACK_NEAREST && mode != UMPA_GRID_TRACK_PENALTY)
        return fail(UMPA_HIP_E_ARG, "grid: track: mode must be UMPA_GRID_TRACK_NEAREST (0) or UMPA_GRID_TRACK_PENALTY (1), not %d", mode);
    if (mode == UMPA_GRID_TRACK_PENALTY && !(lam >= 0.0 && lam < __builtin_inf()))
        return fail(UMPA_HIP_E_ARG, "grid: track: lam must be finite and not negative");
    if (radius != radius) return fail(UMPA_HIP_E_ARG, "grid: track: radius must not be NaN");
    if (flags & ~(UMPA_HIP_F_DEVICE_IO | UMPA_HIP_F_USE_STAGED))
        return fail(UMPA_HIP_E_ARG, "grid: track takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag");
    const int staged = flags & UMPA_HIP_F_USE_STAGED;
    GridJob J;
    J.track = true;
    J.L = L;
    for (int l = 0; l < L; l++) { J.lb[l] = b[l]; J.ltol[l] = tol ? tol[l] : __builtin_inf(); }
    J.want_df = lev.df != nullptr;
    J.want_sel = given != 0;
    J.K.mode = mode;
    J.K.lam = mode == UMPA_GRID_TRACK_PENALTY ? lam : 0.0;
    J.K.limited = radius < 0.0 ? 0 : 1;
    J.K.r2 = radius < 0.0 ? 0.0 : radius * radius;
    // value and status placeholders for the match entry point, as in umpa_grid_cost_volume
    double* const no_values = lev.cost;
    int* const no_err = (int*)lev.cost;
    if (flags & UMPA_HIP_F_DEVICE_IO) {
        J.lev = lev; J.sel = sel; J.sel_level = level; J.sel_hw = halfwidth;
        if (!J.want_df) J.sel.df = nullptr;
        return run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                   UMPA_HIP_F_DEVICE_IO | staged, stream);
    }
    // host arrays: one device block for the duration of the call, allocated by the consumer on the model's device, filled on
    // that device's null stream and downloaded once when every chunk is enqueued (a level's rows are finished a chunk late)
    J.host = true;
    int rc = run(m, J, start0, step0, N0, start1, step1, N1, no_values, 7, no_err, nullptr, 0.0, nullptr, nullptr, nullptr,
                 UMPA_HIP_F_DEVICE_IO | staged, nullptr);
    if (!J.block) return rc;                                          // refused before the consumer ran: nothing was enqueued
    hipError_t e = hipSuccess;
    if (rc >= 0) {
        const size_t n = (size_t)N0 * N1, ln = (size_t)L * n;
        const struct { void* host; const void* dev; size_t bytes; } copies[26] = {
            {lev.f, J.lev.f, ln * sizeof(double)}, {lev.T, J.lev.T, ln * sizeof(double)}, {lev.dx, J.lev.dx, ln * sizeof(double)},
            {lev.dy, J.lev.dy, ln * sizeof(double)}, {lev.cost, J.lev.cost, ln * sizeof(double)}, {lev.df, J.lev.df, ln * sizeof(double)},
            {lev.cost0, J.lev.cost0, ln * sizeof(double)},
            {lev.si, J.lev.si, ln * sizeof(int)}, {lev.sj, J.lev.sj, ln * sizeof(int)}, {lev.err, J.lev.err, ln * sizeof(int)},
            {lev.count, J.lev.count, ln * sizeof(int)}, {lev.found, J.lev.found, ln * sizeof(int)},
            {sel.f, J.sel.f, n * sizeof(double)}, {sel.T, J.sel.T, n * sizeof(double)}, {sel.dx, J.sel.dx, n * sizeof(double)},
            {sel.dy, J.sel.dy, n * sizeof(double)}, {sel.cost, J.sel.cost, n * sizeof(double)}, {sel.df, J.sel.df, n * sizeof(double)},
            {sel.cost0, J.sel.cost0, n * sizeof(double)},
            {sel.si, J.sel.si, n * sizeof(int)}, {sel.sj, J.sel.sj, n * sizeof(int)}, {sel.err, J.sel.err, n * sizeof(int)},
            {sel.count, J.sel.count, n * sizeof(int)}, {sel.found, J.sel.found, n * sizeof(int)},
            {level, J.sel_level, n * sizeof(int)}, {halfwidth, J.sel_hw, n * sizeof(int)}};
        for (int q = 0; q < 26 && e == hipSuccess; q++)
            if (copies[q].host && copies[q].dev) e = hipMemcpy(copies[q].host, copies[q].dev, copies[q].bytes, hipMemcpyDeviceToHost);
    }
    if (rc < 0 || e != hipSuccess) (void)hipDeviceSynchronize();      // nothing of this call may still use the block freed here
    (void)hipFree(J.block);
    if (rc >= 0 && e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: download of the level maps: %s", hipGetErrorString(e));
    return rc;
}

} // namespace

UMPA_GRID_API const char* umpa_grid_last_error(void) { return g_err.c_str(); }

UMPA_GRID_API int umpa_grid_set_masked(umpa_hip_model* m, int on)
{
    if (!m) return fail(UMPA_HIP_E_ARG, "grid: set_masked: null model");
    if (int rc = umpa_hipx_set_masked_consumer(m, on)) return fail(rc, "%s", umpa_hip_last_error());
    return 0;
}

UMPA_GRID_API int umpa_grid_set_general(umpa_hip_model* m, int on)
{
    if (!m) return fail(UMPA_HIP_E_ARG, "grid: set_general: null model");
    if (int rc = umpa_hipx_set_general_consumer(m, on ? general : nullptr, (on & 2) ? 1 : 0)) return fail(rc, "%s", umpa_hip_last_error());
    return 0;
}

UMPA_GRID_API int umpa_grid_match_region(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                                         double* values, int nparam, double* uv, int* err,
                                         const double* covermap, double cover_threshold,
                                         double* dbg_d, double* dbg_a, int* dbg_ncalls, int flags, void* stream)
{
    return match_region(m, start0, step0, N0, start1, step1, N1, 0, values, nparam, uv, err, covermap, cover_threshold,
                        dbg_d, dbg_a, dbg_ncalls, flags, stream);
}

UMPA_GRID_API int umpa_grid_cost_volume(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                                        double* cost, double* T, double* df, int flags, void* stream)
{
    return cost_volume(m, start0, step0, N0, start1, step1, N1, 0, cost, T, df, flags, stream);
}

UMPA_GRID_API int umpa_grid_basins(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int K,
                                   double* f, double* T, double* dx, double* dy, double* cost, double* df,
                                   int* si, int* sj, int* err, int* count, int flags, void* stream)
{
    return basins(m, start0, step0, N0, start1, step1, N1, 0, K, f, T, dx, dy, cost, df, si, sj, err, count, flags, stream);
}

UMPA_GRID_API int umpa_grid_track(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                                  const double* prior_i, const double* prior_j, int mode, double lam, double radius,
                                  double* f, double* T, double* dx, double* dy, double* cost, double* df,
                                  int* si, int* sj, int* err, double* cost0, int* count, int* found, int flags, void* stream)
{
    return track(m, start0, step0, N0, start1, step1, N1, 0, prior_i, prior_j, mode, lam, radius,
                 f, T, dx, dy, cost, df, si, sj, err, cost0, count, found, flags, stream);
}

UMPA_GRID_API int umpa_grid_sequence(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                                     const double* prev, double lam, double trunc, double* next,
                                     double* f, double* T, double* dx, double* dy, double* cost, double* df,
                                     int* si, int* sj, int* err, double* total, double* cost0, int* moved, int flags, void* stream)
{
    return sequence(m, start0, step0, N0, start1, step1, N1, prev, lam, trunc, next, f, T, dx, dy, cost, df, si, sj, err,
                    total, cost0, moved, flags, stream);
}

// Window widening: the NULL check of the sibling, the range of `b`, then the sibling's checks in their order.
UMPA_GRID_API int umpa_grid_wide_match_region(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                                              double* values, int nparam, double* uv, int* err,
                                              const double* covermap, double cover_threshold,
                                              double* dbg_d, double* dbg_a, int* dbg_ncalls, int flags, void* stream)
{
    if (!m) return fail(UMPA_HIP_E_ARG, "grid: null model");
    if (b < 0 || b > UMPA_GRID_MAX_WIDEN) return bad_widen(b);
    return match_region(m, start0, step0, N0, start1, step1, N1, b, values, nparam, uv, err, covermap, cover_threshold,
                        dbg_d, dbg_a, dbg_ncalls, flags, stream);
}

UMPA_GRID_API int umpa_grid_wide_cost_volume(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                                             double* cost, double* T, double* df, int flags, void* stream)
{
    if (!m || !cost) return fail(UMPA_HIP_E_ARG, "grid: null argument");
    if (b < 0 || b > UMPA_GRID_MAX_WIDEN) return bad_widen(b);
    return cost_volume(m, start0, step0, N0, start1, step1, N1, b, cost, T, df, flags, stream);
}

UMPA_GRID_API int umpa_grid_wide_basins(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b, int K,
                                        double* f, double* T, double* dx, double* dy, double* cost, double* df,
                                        int* si, int* sj, int* err, int* count, int flags, void* stream)
{
    if (!m || !f || !T || !dx || !dy || !cost || !si || !sj || !err || !count) return fail(UMPA_HIP_E_ARG, "grid: basins: null argument");
    if (b < 0 || b > UMPA_GRID_MAX_WIDEN) return bad_widen(b);
    return basins(m, start0, step0, N0, start1, step1, N1, b, K, f, T, dx, dy, cost, df, si, sj, err, count, flags, stream);
}

UMPA_GRID_API int umpa_grid_wide_track(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                                       const double* prior_i, const double* prior_j, int mode, double lam, double radius,
                                       double* f, double* T, double* dx, double* dy, double* cost, double* df,
                                       int* si, int* sj, int* err, double* cost0, int* count, int* found, int flags, void* stream)
{
    if (!m || !prior_i || !prior_j || !f || !T || !dx || !dy || !cost || !si || !sj || !err || !cost0 || !count || !found)
        return fail(UMPA_HIP_E_ARG, "grid: track: null argument");
    if (b < 0 || b > UMPA_GRID_MAX_WIDEN) return bad_widen(b);
    return track(m, start0, step0, N0, start1, step1, N1, b, prior_i, prior_j, mode, lam, radius,
                 f, T, dx, dy, cost, df, si, sj, err, cost0, count, found, flags, stream);
}

// Scale-space search: every level of half-widths b[0] > ... > b[L-1] from one table pass, and the selection per pixel.
UMPA_GRID_API int umpa_grid_levels_track(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                                         int L, const int* b, int mode, double lam, double radius, const double* tol,
                                         double* f, double* T, double* dx, double* dy, double* cost, double* df,
                                         int* si, int* sj, int* err, double* cost0, int* count, int* found,
                                         double* sel_f, double* sel_T, double* sel_dx, double* sel_dy, double* sel_cost, double* sel_df,
                                         int* sel_si, int* sel_sj, int* sel_err, double* sel_cost0, int* sel_count, int* sel_found,
                                         int* level, int* halfwidth, int flags, void* stream)
{
    const LevelsPlanes lev = {f, T, dx, dy, cost, df, cost0, si, sj, err, count, found};
    const LevelsPlanes sel = {sel_f, sel_T, sel_dx, sel_dy, sel_cost, sel_df, sel_cost0, sel_si, sel_sj, sel_err, sel_count, sel_found};
    return levels_track(m, start0, step0, N0, start1, step1, N1, L, b, mode, lam, radius, tol, lev, sel, level, halfwidth, flags, stream);
}

// Model-resident uncertainty (umpa_resident_kernels.h): no table, no match -- one kernel on the model's own device frames.
namespace {

// sv of include/umpa_sigma.h: the squares of the window summed in tap order, as two roundings per tap
double resident_sv(const double* win, int T)
{
    volatile double sv = 0.0;                       // (volatile: no contraction of w * w + sv, whatever the host flags)
    for (int x = 0; x < T; x++) { volatile double v = win[x] * win[x]; sv = sv + v; }
    return sv;
}

int resident_axis(const char* name, int start, int step, int N, int extent)
{
    if (N < 1 || step < 1 || start < 0 || (long long)start + (long long)step * (N - 1) > (long long)extent - 1)
        return fail(UMPA_HIP_E_ARG, "grid: uncertainty: region axis %s: start %d, step %d, %d pixels exceed the extent %d", name, start, step, N, extent);
    return 0;
}

void resident_launch(int kind, bool masked, const ModelDev& dev, const ResidentArgs& a, hipStream_t s)
{
    const dim3 grd((a.N1 + RESIDENT_TILE_X - 1) / RESIDENT_TILE_X, (a.N0 + RESIDENT_TILE_Y - 1) / RESIDENT_TILE_Y), blk(RESIDENT_TILE_X, RESIDENT_TILE_Y);
    if (kind && masked) hipLaunchKernelGGL((resident_moments_kernel<1, true>), grd, blk, 0, s, dev, a);
    else if (kind) hipLaunchKernelGGL((resident_moments_kernel<1, false>), grd, blk, 0, s, dev, a);
    else if (masked) hipLaunchKernelGGL((resident_moments_kernel<0, true>), grd, blk, 0, s, dev, a);
    else hipLaunchKernelGGL((resident_moments_kernel<0, false>), grd, blk, 0, s, dev, a);
}

} // namespace

UMPA_GRID_API int umpa_grid_uncertainty(umpa_hip_model* m, int start0, int step0, int N0, int start1, int step1, int N1,
                                        const int* shift, double* moments, double* unit, double* s2, double* dof, int* valid,
                                        int flags, void* stream)
{
    if (!m || !shift || !unit || !s2 || !dof || !valid)
        return fail(UMPA_HIP_E_ARG, "grid: uncertainty: null argument (the model, shift, unit, s2, dof and valid are required)");
    if (flags & ~UMPA_HIP_F_DEVICE_IO) return fail(UMPA_HIP_E_ARG, "grid: uncertainty takes UMPA_HIP_F_DEVICE_IO and no other flag");
    if (int rc = resident_axis("0", start0, step0, N0, 1 << 30)) return rc;       // N, step, start; the extent below
    if (int rc = resident_axis("1", start1, step1, N1, 1 << 30)) return rc;
    ModelDev dev;
    int mkind = 0, has_mask = 0, device = 0;
    hipStream_t ms = nullptr;
    if (int rc = umpa_hipx_model_view(m, &dev, &mkind, &has_mask, &device, &ms)) return fail(rc, "grid: uncertainty: %s", umpa_hip_last_error());
    // what the host knows of the model
    if (mkind != UMPA_HIP_KIND_NODF && mkind != UMPA_HIP_KIND_DF)
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: the kernel dark-field model (kind %d) is not supported", mkind);
    if (dev.ref_mode != 0)
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: a reference-coordinate model (ref_mode = %d) is not supported", dev.ref_mode);
    if (dev.Nw < 1 || dev.Nw > RESIDENT_MAX_NW)
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: Nw = %d (1 to %d are supported)", dev.Nw, RESIDENT_MAX_NW);
    if (dev.ms < 1 || dev.padding != dev.Nw + dev.ms)
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: padding = %d, Nw + max_shift = %d + %d (a window narrower than the model was "
                                            "built with is not supported)", dev.padding, dev.Nw, dev.ms);
    if (dev.Na < 1 || dev.Na > (1 << 20)) return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: a model of %d frames", dev.Na);
    HIPOK(hipSetDevice(device), UMPA_HIP_E_DEVICE, "grid: uncertainty: hipSetDevice(%d)", device);
    // after everything the model has enqueued, on whatever stream: the descriptor table is rewritten in stream order by the
    // call that adopts a staged stack, and the frames may still be written by an upload
    HIPOK(hipDeviceSynchronize(), UMPA_HIP_E_DEVICE, "grid: uncertainty: waiting for the model's work");
    const int side = 2 * dev.Nw + 1, T = side * side, pad = dev.padding;
    std::vector<FrameDesc> desc((size_t)dev.Na);
    double win[(2 * RESIDENT_MAX_NW + 1) * (2 * RESIDENT_MAX_NW + 1)];
    HIPOK(hipMemcpy(desc.data(), dev.frames, (size_t)dev.Na * sizeof(FrameDesc), hipMemcpyDeviceToHost), UMPA_HIP_E_DEVICE, "grid: uncertainty: the frame table");
    HIPOK(hipMemcpy(win, dev.win, (size_t)T * sizeof(double), hipMemcpyDeviceToHost), UMPA_HIP_E_DEVICE, "grid: uncertainty: the window");
    const int H = desc[0].H, W = desc[0].W;
    for (int k = 0; k < dev.Na; k++) {
        const FrameDesc& f = desc[k];
        if (f.H != H || f.W != W || f.pi != 0 || f.pj != 0)
            return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: frame %d has %d x %d pixels at (%d, %d), frame 0 %d x %d at (0, 0): frames at "
                                                "different positions or of different shapes are not supported", k, f.H, f.W, f.pi, f.pj, H, W);
        if (!f.sam || !f.ref || (has_mask && !f.mask)) return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: frame %d has no device frames", k);
    }
    if (H < 2 * pad + 1 || W < 2 * pad + 1)
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: frames of %d x %d pixels (at least %d x %d for padding %d)", H, W, 2 * pad + 1, 2 * pad + 1, pad);
    double sw = 0.0;
    for (int x = 0; x < T; x++) {
        if (!(win[x] >= 0.0) || !std::isfinite(win[x]))
            return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: window entry %d is %g (finite and >= 0)", x, win[x]);
        sw += win[x];
    }
    if (!(std::fabs(sw - 1.0) <= 1e-9))
        return fail(UMPA_HIP_E_UNSUPPORTED, "grid: uncertainty: the window sums to %.17g (it must be normalised)", sw);
    if (int rc = resident_axis("0", start0, step0, N0, H - 2 * pad)) return rc;
    if (int rc = resident_axis("1", start1, step1, N1, W - 2 * pad)) return rc;

    const bool dio = (flags & UMPA_HIP_F_DEVICE_IO) != 0, masked = has_mask != 0;
    const int kind = mkind == UMPA_HIP_KIND_DF ? 1 : 0;
    const size_t n = (size_t)N0 * N1;
    const int P = masked ? (kind ? UMPA_GRID_SIGMA_PLANES_DF : UMPA_GRID_SIGMA_PLANES_PLAIN) : (kind ? 34 : 16);
    hipStream_t s = dio ? (hipStream_t)stream : ms;
    ResidentArgs a;
    a.H = H; a.W = W; a.sv = resident_sv(win, T);
    a.start0 = start0; a.step0 = step0; a.N0 = N0; a.start1 = start1; a.step1 = step1; a.N1 = N1;
    a.shift = shift; a.moments = moments; a.unit = unit; a.s2 = s2; a.dof = dof; a.valid = valid;
    if (dio) {
        resident_launch(kind, masked, dev, a, s);
        LAUNCHED("grid: uncertainty: launch of the moments kernel");
        HIPOK(hipStreamSynchronize(s), UMPA_HIP_E_LAUNCH, "grid: uncertainty");
        return 0;
    }
    // host arrays: slots 0 shift, 1 moments, 2 unit, 3 s2, 4 dof, 5 valid
    DeviceMem S;
    const size_t bytes[5] = {moments ? P * n * 8 : 0, 3 * n * 8, n * 8, n * 8, n * 4};
    void* host[5] = {moments, unit, s2, dof, valid};
    HIPOK(S.alloc(0, 2 * n * 4), UMPA_HIP_E_NOMEM, "grid: uncertainty: device memory for the shift field");
    for (int q = 0; q < 5; q++)
        if (host[q]) HIPOK(S.alloc(1 + q, bytes[q]), UMPA_HIP_E_NOMEM, "grid: uncertainty: device memory for the results");
    HIPOK(hipMemcpyAsync(S.p[0], shift, 2 * n * 4, hipMemcpyHostToDevice, s), UMPA_HIP_E_DEVICE, "grid: uncertainty: upload of the shift field");
    a.shift = (const int*)S.p[0]; a.moments = (double*)S.p[1]; a.unit = (double*)S.p[2]; a.s2 = (double*)S.p[3]; a.dof = (double*)S.p[4];
    a.valid = (int*)S.p[5];
    resident_launch(kind, masked, dev, a, s);
    const hipError_t le = hipGetLastError();
    hipError_t e = le;
    for (int q = 0; q < 5 && e == hipSuccess; q++)
        if (host[q]) e = hipMemcpyAsync(host[q], S.p[1 + q], bytes[q], hipMemcpyDeviceToHost, s);
    const hipError_t se = hipStreamSynchronize(s);       // nothing of this call may still use the memory freed on return
    if (le != hipSuccess) return fail(UMPA_HIP_E_LAUNCH, "grid: uncertainty: launch of the moments kernel: %s", hipGetErrorString(le));
    if (e != hipSuccess) return fail(UMPA_HIP_E_DEVICE, "grid: uncertainty: download of the results: %s", hipGetErrorString(e));
    if (se != hipSuccess) return fail(UMPA_HIP_E_LAUNCH, "grid: uncertainty: %s", hipGetErrorString(se));
    return 0;
}
