/*
 * umpa_grid.h -- exhaustive grid search and the cost volume (libumpa_grid.so, gfx950).
 *
 * The tiled fast path of libumpa_hip.so computes the windowed cost's correlation term for EVERY integer shift of the
 * search box at every pixel (the exhaustive table).  The default minimiser, the reference's walk,
 * reads about 18 of its entries per pixel.  This library reads all of them:
 *
 *   umpa_grid_match_region  the global minimum over the (2 max_shift - 1)^2 integer shifts of every pixel, followed by
 *                           the walk's own sub-pixel step on the 4x4 neighbourhood of that minimum;
 *   umpa_grid_cost_volume   the cost (and optionally transmission and dark-field) of every shift at every pixel;
 *   umpa_grid_basins        per pixel the K lowest local minima ("basins") of the cost over the search box, each with the
 *                           sub-pixel step and fit umpa_grid_match_region would give it, and the count of all basins;
 *   umpa_grid_track         per pixel, among ALL its basins, the one nearest a prior shift (or the best under cost plus a
 *                           distance penalty), finished like a kept basin: one set of maps, the prior may live on the device.
 *   umpa_grid_wide_<name>   each of the four on a shift table and maps box-averaged over the (2b + 1)^2 dense pixels around a
 *                           pixel: the same search under a window b pixels wider, on the same model ("window widening");
 *   umpa_grid_levels_track  umpa_grid_wide_track at up to four half-widths from one pass over the table, each level the prior
 *                           of the next, and per pixel the narrowest level that agrees with the wider ones ("scale space").
 *   umpa_grid_sequence      a per-pixel cost state over all shifts carried from projection to projection: each call adds its
 *                           costs to the cheapest compatible predecessor (forward dynamic programming, "sequence search").
 *   umpa_grid_uncertainty   the uncertainty maps of include/umpa_sigma.h on the model's own device frames, masks included; it
 *                           reads no table and runs no match (its own rules are at its declaration, not the paragraph below).
 *
 * All work on models that the plain tiled path takes whole: no masks, not the kernel dark-field model, all frames of
 * one shape at position (0, 0), steps and search ranges within that path's limits.  Anything else fails with
 * UMPA_HIP_E_UNSUPPORTED before a kernel is launched.  A model WITH masks is admitted once umpa_grid_set_masked has
 * switched it on (below; off by default).  Models are created, configured and destroyed through
 * include/umpa_hip.h; link both libraries.  Error text: umpa_hip_last_error() for codes that umpa_hip_match_region
 * produced, umpa_grid_last_error() for this library's own.
 */
#ifndef UMPA_GRID_H
#define UMPA_GRID_H

#include "umpa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Masked models: the per-model switch, off by default.  A NULL model is UMPA_HIP_E_ARG; on a model without masks the call
 * changes nothing; the state lives with the model and dies with it.
 *
 * With the switch off, every function below refuses a model with masks as before (UMPA_HIP_E_UNSUPPORTED, the same text).
 * With it on, umpa_grid_match_region, _cost_volume, _basins, _track, _sequence and the umpa_grid_wide_ four with b = 0 run on
 * the MASKED tiled path's table, which holds, for every integer shift of the search box at every dense pixel, the finished
 * cost, transmission and dark-field of the masked model (the numbers its walk reads: DESIGN.md sections 4.4 and 4.16).  Every
 * rule stated below then holds word for word with C[s] that cost: argument checks, their order and texts, flags, chunked
 * downloads and the rows callback are unchanged, and so are the equivalences (rank 0 of the basins is the grid minimum,
 * track with lam = 0 and sequence with lam = 0 or without a state are the grid search).
 * Coverage.  umpa_grid_match_region takes `covermap` / `cover_threshold` and skips the pixels below the threshold, as
 * umpa_hip_match_region does.  The other functions have no such argument: on a masked model they compute EVERY pixel of the
 * region, and the caller drops the pixels it does not trust.  A window without any pair weight has a weight sum of 0, all
 * its costs are NaN, and the NaN rules below give the "no finite cost" result; a window that keeps some weight has costs,
 * however few pixels carry them.
 * What the masked tiled path does not take is UMPA_HIP_E_UNSUPPORTED with a text that names the reason: a window size without
 * a masked table kernel, exact-fit windows (frames x window pixels <= 9), a dark-field pair plane past 4 GiB, a step product
 * past the masked limit (16 dense pixels per requested one, 5 for the dark-field model, at up to 81 shifts; fewer beyond),
 * frames at different positions or of different shapes.
 * Window widening (b > 0) and umpa_grid_levels_track on such a model are UMPA_HIP_E_UNSUPPORTED: a finished cost is not linear
 * in the windowed sums, so a box average of costs is not the cost under a wider window. */
int umpa_grid_set_masked(umpa_hip_model *m, int on);

/* The general table: the per-model switch for everything no tiled path takes whole, off by default.  A NULL model is
 * UMPA_HIP_E_ARG; the state lives with the model and dies with it.  `on`: 0 off; 1 on; 3 on, and also for a model and region
 * a tiled path would take (the caller wants the explicit sum everywhere, as a model forced onto the direct kernel does).
 *
 * With the switch off every function below refuses what it refused before, with the same text.  With it on,
 * umpa_grid_match_region, _cost_volume, _basins, _track, _sequence and the umpa_grid_wide_ four with b = 0 also take: frames at
 * different positions (sample stepping) or of unequal shapes, a model forced onto the direct kernel
 * (UMPA_HIP_F_FORCE_DIRECT), a model with masks whose umpa_grid_set_masked switch is off or that the masked tiled path does
 * not admit, steps and search ranges past the tiled limits -- everything the general kernels of umpa_hip_match_region
 * take, except the kernel dark-field model, which has no per-shift table.  Whatever a tiled path takes whole keeps going
 * there (on = 1): its numbers do not change with the switch.
 * The general table holds, for every requested pixel and every integer shift of the search box, the FINISHED cost,
 * transmission and dark-field value of the model: the reference's own window x frame sum (frames outer, window rows, then
 * columns; a frame contributes to a pixel iff the pixel keeps `padding` from its edges; the cost is divided by the frame
 * count without masks and by the sum of the pair weights with them), equal bit for bit to umpa_hip_cost of the same pixel
 * and shift.  It is filled per row chunk within the table budget of the tiled paths (UMPA_HIP_TABLE_MB), on the requested
 * pixels only, whatever the steps.  Every rule stated below then holds word for word with C[s] that cost, as on a masked
 * model (umpa_grid_set_masked): argument checks, their order and texts, flags, the staged stack, device I/O; the result maps of
 * umpa_grid_match_region are downloaded in one piece.
 * Coverage.  umpa_grid_match_region takes `covermap` / `cover_threshold` and skips the pixels below the threshold; the other
 * functions compute EVERY pixel of the region.  A pixel no frame contributes to (and, with masks, a window without any pair
 * weight) has NaN costs, and the NaN rules below give the "no finite cost" result.
 * Window widening (b > 0) and umpa_grid_levels_track on a model and region that go this way are UMPA_HIP_E_UNSUPPORTED: a
 * finished cost is not linear in the windowed sums, so a box average of costs is not the cost under a wider window.
 * The arithmetic per pixel is 3 * frames * window pixels FMAs for EVERY shift: about 38 times the plain tiled path's at ten
 * frames, an 11 x 11 window and 81 shifts. */
int umpa_grid_set_general(umpa_hip_model *m, int on);

/* The arguments, flags (UMPA_HIP_F_DEVICE_IO, _PLANAR, _REUSE_REF_MAPS, _USE_STAGED, _ASYNC), chunked downloads and the
 * rows callback of umpa_hip_match_region.  `uv` must be NULL (start shifts mean nothing to an exhaustive search:
 * UMPA_HIP_E_ARG).  Per pixel:
 *   the integer minimum is the first shift, rows first then columns, whose cost is strictly below every earlier one
 *   (a NaN cost never wins);
 *   err = 1: the quadrant rule of the walk applied to the four neighbours of the minimum picks the 4x4 neighbourhood;
 *     dx, dy, f come from the sub-pixel fit the model is set to (mode 0: the integer minimum, f = 1 - ip as in the
 *     reference); T (and df) are those of the integer minimum; dbg_ncalls = (2 max_shift - 1)^2; dbg_a is the 4x4
 *     neighbourhood, dbg_d the 5x5 one around the minimum with -1 outside the search range;
 *   err = 0 where that 4x4 neighbourhood leaves the search range: dx, dy are the integer minimum, f its cost, T (df) its
 *     fit; dbg_a is zero;
 *   err = 0 and zeros (dbg_d: -1) where no shift has a finite cost.
 *
 * Non-finite costs (a NaN or an Inf pixel inside a window makes the costs of that window NaN; tests/consumer_expect.py
 * has the footprint).  Every comparison above is a plain `<` of doubles, and nothing else looks at a cost:
 *   the minimum: a shift wins iff its cost is `<` the best so far, which starts at +Inf.  NaN and +Inf never win.  -Inf
 *   is a cost like any other: the first -Inf shift wins and stays (no input of the tests produces one; Inf pixels give
 *   NaN costs, Inf - Inf);
 *   "no shift has a finite cost" means: no cost is < +Inf.  Such a pixel has err = 0, f = T = dx = dy (= df) = 0, dbg_a
 *   zero, every dbg_d cell -1 and dbg_ncalls = (2 max_shift - 1)^2 like every other pixel: the count is of the shifts
 *   looked at, not of the finite ones;
 *   a pixel with a finite minimum but a NaN among the 5x5 cells around it: the quadrant tests `cost(+1) < cost(-1)` are
 *   false on a NaN (ip, jp = 0), the 4x4 neighbourhood and the sub-pixel fit are evaluated on the cells as they are, so
 *   err is 0 or 1 by the range rule alone and dx, dy, f of an err = 1 pixel may be NaN with sub-pixel modes -1 and 1;
 *   dbg_d and dbg_a hold the cells, NaN included.  T (df) stay the integer minimum's.  Callers that need
 *   finite maps test them (umpa_amd.sigma.shift_field does).
 */
int umpa_grid_match_region(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1,
                           double *values, int nparam, double *uv, int *err,
                           const double *covermap, double cover_threshold,
                           double *dbg_d, double *dbg_a, int *dbg_ncalls, int flags, void *stream);

/* cost[(si + max_shift - 1) * U + (sj + max_shift - 1)][xi][xj], U = 2 max_shift - 1, for the region's N0 x N1 pixels
 * (si: row shift, sj: column shift); `T` and `df` (dark-field model only) in the same layout, each may be NULL.
 * Host arrays, or device arrays with UMPA_HIP_F_DEVICE_IO (the call then only enqueues work on `stream`).
 * UMPA_HIP_F_USE_STAGED: the stack uploaded by umpa_hip_stage_sample is adopted first, as by umpa_hip_match_region, and
 * the volume is that stack's; the matches that follow read it too.  Any other flag is UMPA_HIP_E_ARG.
 * An array holds U * U * N0 * N1 doubles. */
int umpa_grid_cost_volume(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1,
                          double *cost, double *T, double *df, int flags, void *stream);

/* Basin enumeration: per pixel, the K lowest local minima ("basins") of the cost over the search box, 1 <= K <= 8.
 *
 * Let C[si][sj], -max_shift < si, sj < max_shift, be the costs of umpa_grid_cost_volume for one pixel.  Scan order is the
 * grid search's: rows (si) first, then columns (sj).
 *   Beats.   A neighbour n BEATS a shift s iff C[n] < C[s], or C[n] == C[s] and n precedes s in scan order.
 *   Basin.   A shift s is a basin iff C[s] < +Inf and none of its up to eight neighbours inside the box beats it.
 *            Neighbours outside the box do not exist.  Every comparison is a plain `<` or `==` of doubles: a NaN neighbour
 *            never beats anything and a NaN shift is never a basin; -Inf is a cost like any other.  A run of equal adjacent
 *            costs yields only its earliest member, and only if nothing else beats that member.
 *   Ranking. Basins are ordered by cost ascending, by scan order among equal costs.  The first K are kept; count is the
 *            number of ALL basins of the pixel and may exceed K.
 *   Consequence: rank 0 is the integer minimum of umpa_grid_match_region.  The first strict minimum has nothing below it
 *            and no equal cost before it, so nothing beats it; no basin costs less, and an equally cheap one comes later.
 *   Per kept basin, the epilogue of umpa_grid_match_region around it instead of around the global minimum: the quadrant
 *            rule picks the 4x4 neighbourhood, dx, dy, f come from the sub-pixel fit the model is set to (mode 0: the
 *            integer shift, f = 1 - ip), T (and df) are those of the integer shift, err = 1; err = 0 where that 4x4
 *            neighbourhood leaves the search range: dx, dy are the integer shift, f its cost.  A NaN among the cells
 *            around a basin is treated as umpa_grid_match_region treats it.  cost is always the cost of the integer shift.
 *   Slots k >= count: err = -1, every double 0, the shift (0, 0).  A pixel without any finite cost: count = 0, all slots
 *            empty.
 *
 * The model and the region as for umpa_grid_cost_volume.  Outputs are planes [K][N0][N1]: doubles f, T, dx (column shift),
 * dy (row shift), cost and df (may be NULL; dark-field model only: UMPA_HIP_E_* with a plain model); ints si (row), sj
 * (column), err; and count[N0][N1].  Host arrays, or device arrays with UMPA_HIP_F_DEVICE_IO (the call then only enqueues
 * work on `stream`); UMPA_HIP_F_USE_STAGED as for umpa_grid_cost_volume; any other flag is UMPA_HIP_E_ARG.  Checked in this
 * order, before anything touches a device: a NULL model or array (other than df), K outside 1 .. 8, the flags -- each
 * UMPA_HIP_E_ARG.  No coverage map: every pixel of the region is computed; on a masked model (umpa_grid_set_masked) a window
 * without any pair weight has NaN costs and comes out as a pixel without a finite cost.
 * One pass over the table, no atomics: the output is the same bit for bit from run to run, for host and device arrays and
 * under any row chunking. */
int umpa_grid_basins(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1, int K,
                     double *f, double *T, double *dx, double *dy, double *cost, double *df,
                     int *si, int *sj, int *err, int *count, int flags, void *stream);

/* Tracked search: per pixel, among ALL basins of the cost over the search box, the one a prior shift selects.
 *
 * C[si][sj], "beats", "basin" and scan order are those of umpa_grid_basins, unchanged.
 *   Prior.   (p_i, p_j) per pixel: two planes [N0][N1] of doubles indexed like the outputs, p_i the row shift, p_j the
 *            column shift, in the units of the shifts (si, sj) of umpa_grid_basins.  Those are also the units of the maps
 *            dy (rows) and dx (columns) of umpa_hip_match_region, under either coordinate assignment: with the reference
 *            coordinates ('ref') the kernels move the other stack's window, but a pixel's result is stored as the shift the
 *            search indexed, without a change of sign or of origin.  So (dy, dx) of an earlier match, or of an earlier
 *            call of this function, on the same model settings is a prior as it stands: p_i = dy, p_j = dx.
 *   Distance. d2(s) = (si - p_i) * (si - p_i) + (sj - p_j) * (sj - p_j) in doubles: two subtractions, two products, one
 *            addition, each rounded (no fused multiply-add).  A pixel whose p_i or p_j is NaN has d2(s) = 0 for every
 *            shift: it falls back to the data term alone.  An infinite prior is a number like any other (d2 = +Inf).
 *   Admissible. radius < 0: every basin.  Otherwise a basin s is admissible iff d2(s) <= r2, r2 = radius * radius formed
 *            once.
 *   Choice.  The admissible basins are gone through in scan order; the first is the best so far, and a later one replaces
 *            the best iff it is strictly better:
 *              UMPA_GRID_TRACK_NEAREST (0): d2(s) < d2(best), or d2(s) == d2(best) and C[s] < C[best] -- the smallest d2,
 *                then the smallest cost, then scan order: the rule of umpa_amd.basins.nearest, over all basins;
 *              UMPA_GRID_TRACK_PENALTY (1): key(s) < key(best), key(s) = C[s] + lam * d2(s), one product and one addition,
 *                each rounded -- the smallest key, then scan order.  With lam = 0 (and finite priors) this is rank 0 of
 *                umpa_grid_basins, the integer minimum of umpa_grid_match_region.  A NaN key (0 * Inf, Inf - Inf) is never
 *                `<` anything and nothing is `<` it.
 *            Every comparison is a plain `<`, `<=` or `==` of doubles.
 *   Outputs, planes [N0][N1].  For the chosen basin f, T, dx, dy, cost, df (doubles) and si, sj, err (ints), exactly what
 *            umpa_grid_basins writes for a kept basin: quadrant rule, 4x4 neighbourhood, the model's sub-pixel mode, T (df)
 *            of the integer shift, err = 1, or err = 0 with the integer shift and its cost where the 4x4 leaves the box.
 *            cost0: the lowest cost of any basin of the pixel (rank 0's); cost > cost0 says the prior overruled the data
 *            term.  count: all basins of the pixel.  found: its admissible basins.
 *            found == 0: err = -1, f = T = dx = dy = cost (= df) = 0, si = sj = 0; cost0 and count are written all the
 *            same; count == 0: cost0 = 0.
 *
 * The model and the region as for umpa_grid_basins.  Host arrays, or device arrays with UMPA_HIP_F_DEVICE_IO (the call then
 * only enqueues work on `stream`) -- the priors and the outputs alike; UMPA_HIP_F_USE_STAGED as for umpa_grid_cost_volume.
 * df may be NULL (dark-field model only: UMPA_HIP_E_* with a plain model).  Checked in this order, before anything touches
 * a device, each UMPA_HIP_E_ARG: a NULL model or array (other than df); a mode other than 0 and 1; with mode 1, a lam that
 * is not finite or is negative (mode 0 ignores lam); a NaN radius; a flag other than the two above.
 * One pass over the table, no atomics: the output is the same bit for bit from run to run, for host and device arrays and
 * under any row chunking. */
#define UMPA_GRID_TRACK_NEAREST 0
#define UMPA_GRID_TRACK_PENALTY 1
int umpa_grid_track(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1,
                    const double *prior_i, const double *prior_j, int mode, double lam, double radius,
                    double *f, double *T, double *dx, double *dy, double *cost, double *df,
                    int *si, int *sj, int *err, double *cost0, int *count, int *found, int flags, void *stream);

/* Window widening: the four consumers above on a box-pooled shift table.
 *
 * b is 0 to UMPA_GRID_MAX_WIDEN, B = 2b + 1, rB = 1.0 / (double)(B * B).  For a plane q on the region's dense (unit-step)
 * grid, in doubles:
 *   H(r, c)  = q(r, c-b) + q(r, c-b+1) + ... + q(r, c+b), added left to right;
 *   V(r, c)  = H(r-b, c) + H(r-b+1, c) + ... + H(r+b, c), added top to bottom;
 *   q'(r, c) = V(r, c) * rB.
 * Every operation is rounded, nothing is contracted into a fused multiply-add, and there are no running sums (add the new
 * element, subtract the old one depends on where the sum started): q' is this sum in this order for every element,
 * whatever row chunks the table was computed in.
 * The planes are every plane of the shift table at a fixed shift, t5(., s), and the maps the tiled path keeps per pixel:
 * SamSq, RefSq and each frame's WS and MR.  A cost, its transmission and dark-field are then the
 * one evaluation every consumer above already uses (eval_lookup, umpa_amd/csrc/umpa_tiled.h), on the pooled planes.
 * All these planes are windowed sums, linear in the window w, so q' is the same quantity under the window
 *   W' = (w (*) box_B) / B^2   ((*): convolution),
 * which is separable, has the sum of w and the half-width Nw + b.  The results are therefore those of the reference model
 * with window W' (up to rounding; tests/widen_expect.py has the bound), at the same pixel and shift.
 *
 * Border.  A pixel of the region whose B x B block of dense pixels leaves the region's dense grid (the first and last b
 * dense rows and columns) has NaN table entries, hence NaN costs, and the siblings' rules for NaN apply:
 *   umpa_grid_wide_match_region  err = 0 and zeros;       umpa_grid_wide_cost_volume  NaN (cost, T and df);
 *   umpa_grid_wide_basins        count = 0, empty slots;  umpa_grid_wide_track        found = 0, err = -1 (count = 0, cost0 = 0).
 * A caller who wants numbers there asks for a region b dense pixels larger on every side (umpa_amd.widen does).
 *
 * Each function is its sibling with `int b` after N1, and with b = 0 it is the sibling, bit for bit.  Checked in this order
 * before anything touches a device: the sibling's NULL arguments (same text), b outside 0 .. UMPA_GRID_MAX_WIDEN
 * (UMPA_HIP_E_ARG, the text names the value), then the sibling's other checks in their order.
 * The pooled planes live in workspace from the device's stream-ordered allocator (hipMallocAsync on the call's stream at
 * the first row chunk, given back on that stream behind the last kernel): with UMPA_HIP_F_DEVICE_IO the call still only
 * enqueues work.  The output is the same bit for bit from run to run, for host and device arrays and under any row chunking.
 * With b > 0 a dense row is finished one row chunk late.  umpa_grid_wide_match_region on host arrays therefore downloads
 * its maps when all chunks are enqueued, not chunk by chunk, and returns with the maps complete also under
 * UMPA_HIP_F_ASYNC; a rows callback (umpa_hip_set_rows_callback) may be told of rows that the next chunk completes. */
#define UMPA_GRID_MAX_WIDEN 8
int umpa_grid_wide_match_region(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                                double *values, int nparam, double *uv, int *err,
                                const double *covermap, double cover_threshold,
                                double *dbg_d, double *dbg_a, int *dbg_ncalls, int flags, void *stream);
int umpa_grid_wide_cost_volume(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                               double *cost, double *T, double *df, int flags, void *stream);
int umpa_grid_wide_basins(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1, int b, int K,
                          double *f, double *T, double *dx, double *dy, double *cost, double *df,
                          int *si, int *sj, int *err, int *count, int flags, void *stream);
int umpa_grid_wide_track(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1, int b,
                         const double *prior_i, const double *prior_j, int mode, double lam, double radius,
                         double *f, double *T, double *dx, double *dy, double *cost, double *df,
                         int *si, int *sj, int *err, double *cost0, int *count, int *found, int flags, void *stream);

/* Scale-space search: umpa_grid_wide_track at several half-widths from one table pass, and the level to trust per pixel.
 *
 * Levels.  L levels, 1 <= L <= UMPA_GRID_MAX_LEVELS, of half-widths b[0] > b[1] > ... > b[L-1].  The widened half-widths
 *   come from {1, 2, 4, 8}, at most three of them; an optional final 0 is the model's own window.  Any other list is
 *   UMPA_HIP_E_ARG, and the text names the list.
 * Level 0 is umpa_grid_wide_track at b[0] with a prior that is NaN at every pixel: by the rule of umpa_grid_track (a NaN prior
 *   leaves the pixel to the data term) the grid search under the window widened by b[0], finished as a track result.
 * Level l > 0 is umpa_grid_wide_track at b[l] on the same region, with the call's mode, lam and radius, and the prior
 *     ok    = err == 1 && isfinite(dx) && isfinite(dy)      of level l - 1,
 *     p_i   = ok ? dy : NaN,   p_j = ok ? dx : NaN,
 *   which is umpa_amd.track.prior_from, expression for expression.
 * Each level's planes -- f, T, dx, dy, cost, df, si, sj, err, cost0, count, found, [L][N0][N1] each -- are exactly what
 *   the sibling writes for that region, b and prior, the NaN rules of window widening included: level l holds found = 0,
 *   err = -1, count = 0 and zeros at the pixels whose (2 b[l] + 1)^2 block leaves the region's dense grid.
 * Selection.  tol: L doubles, each >= 0 or +Inf (NaN and negative values are UMPA_HIP_E_ARG); NULL: all +Inf.  With
 *     ok_l  = err_l == 1 && isfinite(dx_l) && isfinite(dy_l),
 *   level l is CONSISTENT iff ok_l and, for every wider level m < l with ok_m,
 *     fabs(dx_l - dx_m) <= tol[m]  &&  fabs(dy_l - dy_m) <= tol[m]
 *   (one rounded subtraction, fabs, one comparison of doubles each).  level(p) is the largest consistent l, -1 where no
 *   level is ok: the narrowest window that still agrees with every wider one that matched (Lepski's rule).  tol[L-1] is
 *   read by nothing.  The selected planes, the same twelve as [N0][N1], are copies of level level(p)'s values; at -1 they
 *   are copies of level L - 1's, which hold the sibling's values for a pixel without a match.  `level` is level(p) and
 *   `halfwidth` b[level(p)], or -1, as ints.  The thirteen selected arrays (df aside) are all given or all NULL.
 *
 * The model and the region as for umpa_grid_wide_track.  Host arrays, or device arrays with UMPA_HIP_F_DEVICE_IO (the call
 * then only enqueues work on `stream`); UMPA_HIP_F_USE_STAGED as for umpa_grid_cost_volume.  df and sel_df may be NULL
 * (dark-field model only).  Checked in this order before anything touches a device, each UMPA_HIP_E_ARG: a NULL model, list or
 * per-level array (other than df); L; the list b; tol; a selected group that is given in part; then umpa_grid_wide_track's
 * checks with its texts (mode, lam, radius, flags).
 * One pass.  The shift table and the maps are computed once; a row chunk's table is pooled to every widened level in one
 * read of its raw rows, and all levels lag by b[0] rows, so that a level's prior is finished when its rows are searched.
 * The workspace (up to three pooled chunk tables, the carry of 2 b[0] raw rows, the pooled maps per level, two prior planes)
 * comes from the stream-ordered allocator as for window widening.  The output is the same bit for bit from run to run, for
 * host and device arrays and under any row chunking. */
#define UMPA_GRID_MAX_LEVELS 4
int umpa_grid_levels_track(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1,
                           int L, const int *b, int mode, double lam, double radius, const double *tol,
                           double *f, double *T, double *dx, double *dy, double *cost, double *df,
                           int *si, int *sj, int *err, double *cost0, int *count, int *found,
                           double *sel_f, double *sel_T, double *sel_dx, double *sel_dy, double *sel_cost, double *sel_df,
                           int *sel_si, int *sel_sj, int *sel_err, double *sel_cost0, int *sel_count, int *sel_found,
                           int *level, int *halfwidth, int flags, void *stream);

/* Sequence search: one forward step of a dynamic programme over a series of projections.
 *
 * U = 2 max_shift - 1.  Shifts s = (si, sj) run in the grid search's scan order, rows (si) first, then columns (sj).  C[s] is
 * the cost of umpa_grid_cost_volume at the pixel.  Everything is fp64 and nothing is contracted into a fused multiply-add.
 * Every comparison is a plain `<` of doubles; every minimum starts at +Inf and takes a candidate iff it is `<` the best so
 * far, the candidates in scan order (the first strict minimum): NaN and +Inf never win, -Inf is a number like any other.
 *   State.   prev and next: [U * U][N0][N1] doubles in the slot order of the cost volume,
 *            state[(si + max_shift - 1) * U + (sj + max_shift - 1)][xi][xj].  prev may be NULL: a series starts.  next may be
 *            NULL (the state is not kept).  prev and next must not overlap.
 *   Transition.  lam is finite and >= 0, trunc is >= 0 or +Inf.
 *            1. m0 = min_{s'} prev[s'].  If prev is NULL or !(m0 < +Inf) -- the pixel never matched -- M[s] = 0 for all s.
 *               Otherwise
 *            2. R[si'][sj] = min_{sj'} (prev[si'][sj'] + lam * (double)((sj - sj') * (sj - sj'))), sj' ascending: the square
 *               in ints, one conversion, one product and one sum, each rounded;
 *            3. Q[si][sj]  = min_{si'} (R[si'][sj] + lam * (double)((si - si') * (si - si'))), si' ascending;
 *            4. cap = m0 + trunc;  Q'[s] = (cap < Q[s]) ? cap : Q[s];
 *            5. M[s] = Q'[s] - m0.
 *            This two-stage form IS the definition of the quadratic penalty here, not an approximation of the joint minimum
 *            over s' (with exact arithmetic the two agree; in doubles the order of the two sums is this one).  The truncation
 *            lets a pixel jump to any shift at the fixed price trunc.  Taking m0 off keeps the numbers on the scale of one
 *            projection's costs however long the series is.
 *   Update.  A[s] = C[s] + M[s], one sum; next[s] = A[s] where next is not NULL.  A[s] is NaN where C[s] is NaN.
 *   Choice.  s* is the first strict minimum of A.
 *   Outputs, planes [N0][N1].  For s*: f, T, dx, dy, df (doubles) and si, sj, err (ints), exactly what umpa_grid_track writes
 *            for a chosen basin, evaluated on the DATA costs C: quadrant rule, 4x4 neighbourhood, the model's sub-pixel mode,
 *            T (df) of the integer shift, err = 1, or err = 0 with the integer shift and its cost where the 4x4 leaves the
 *            box.  cost = C[s*].  total = A[s*].  cost0: the first strict minimum of C (0 where no C[s] < +Inf).  moved (int):
 *            1 iff s* differs from the first strict minimum of C.
 *            No A[s] < +Inf: err = -1, f = T = dx = dy = cost = total (= df) = 0, si = sj = 0, moved = 0; next is written all
 *            the same.
 *   Consequences.  With lam = 0 (and a prev without -Inf) Q = m0 everywhere, so M = 0 and A = C + 0.0, which compares like C:
 *            f, T, dx, dy, df, err are those of umpa_grid_match_region, and cost = total = cost0, moved = 0.  The same with
 *            prev = NULL.  With trunc = 0, M = 0 at every pixel whose m0 is finite.
 *            A pixel's result depends on that pixel's state and costs alone: the maps and next are the same bit for bit from
 *            run to run, for host and device arrays and under any row chunking.  No atomics.
 *
 * The model and the region as for umpa_grid_track, with max_shift from 2 to UMPA_GRID_SEQUENCE_MAX_SHIFT (the range of
 * umpa_smooth); any other max_shift is UMPA_HIP_E_UNSUPPORTED and the text names the value.  Host arrays, or device arrays
 * with UMPA_HIP_F_DEVICE_IO (the call then only enqueues work on `stream`) -- prev, next and the maps alike;
 * UMPA_HIP_F_USE_STAGED as for umpa_grid_cost_volume.  df may be NULL (dark-field model only: UMPA_HIP_E_* with a plain model).
 * Checked in this order, before anything touches a device, each UMPA_HIP_E_ARG with a text that names the value: a NULL
 * model; a NULL output plane (other than df and next); a lam that is NaN, infinite or negative; a trunc that is NaN or
 * negative; a flag other than the two above. */
#define UMPA_GRID_SEQUENCE_MAX_SHIFT 8
int umpa_grid_sequence(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1,
                       const double *prev, double lam, double trunc, double *next,
                       double *f, double *T, double *dx, double *dy, double *cost, double *df,
                       int *si, int *sj, int *err, double *total, double *cost0, int *moved,
                       int flags, void *stream);

/* Model-resident uncertainty: the per-pixel covariance of a matched shift and the noise estimate from the residual, computed
 * on the MODEL'S OWN device frames -- no stack is passed and none is uploaded; masked models are admitted.
 *
 * The operation, its notation and its outputs are those of include/umpa_sigma.h (libumpa_sigma.so, which takes two bare stacks
 * and never sees a model): the region rule, shift[2][N0][N1] with UMPA_SIGMA_SKIP, the PIXEL GUARD, FIELDS, MOMENTS, MODEL,
 * SOLVE and OUTPUT.  sam, ref (and mask) are the model's frames, win its window, Nw, ms = max_shift and pad = its padding.  The
 * sample stack is the one the LAST MATCH ADOPTED: after umpa_hip_stage_sample and a match with UMPA_HIP_F_USE_STAGED that is
 * the staged, flat-corrected stack; a stack staged and not yet adopted is not read, and this call takes no
 * UMPA_HIP_F_USE_STAGED.  kind: 0 for UMPA_HIP_KIND_NODF, 1 for UMPA_HIP_KIND_DF.
 *
 * A model WITHOUT masks: the definition is include/umpa_sigma.h's, unchanged and not restated: P = 16 / 34 planes, their
 * rounding bound, dof = K - tr.  Fed the same frames and shifts, the moments agree with umpa_sigma_region's within that bound.
 *
 * A model WITH masks (no switch: umpa_grid_set_masked is not needed).  The pair weight of the matchers' cost enters the window
 * weight and is held fixed at the integer shift; it is not differentiated.
 * FIELDS per frame k and tap x, in addition to a, r, g_i, g_j, u = (u_0, u_1, u_2) = (g_i, g_j, r) of include/umpa_sigma.h:
 *     p = mask[k] at the reference tap (where r is read)        q = mask[k] at the sample tap (where a is read)
 *     c = (p * q) / ((p + q) + 1e-8)                            (the reference's combine_weights)
 *     w = c * win[x]                                            v = w * w
 *   per frame, sum_x in tap order:
 *     omega = sum_x w              nu  = sum_x v                 (plain additions)
 *     m_p   = sum_x w u_p          n_p = sum_x v u_p             m_a = sum_x w a        (each term one product, plain additions)
 *     mu_p  = (sum_x win[x] u_p) / win_sum        dark-field only; each term one fma(win[x], u_p, sum); win_sum: the window
 *             summed in tap order in doubles.  This is the UNMASKED windowed mean of the reference, as in the masked cost
 *             function of the reference, and (p = 0, 1) its central differences.
 * MOMENTS, [P][N0][N1] planes, P = UMPA_GRID_SIGMA_PLANES_PLAIN = 17 or UMPA_GRID_SIGMA_PLANES_DF = 50; every accumulation
 * into a plane is one fma(first factor, last factor, plane), the first factor a rounded product where it is bracketed:
 *      0 ..  5   S_pq  = sum_k sum_x (w u_p) u_q        (p, q) = 00 01 02 11 12 22
 *      6 .. 11   V_pq  = sum_k sum_x (v u_p) u_q        same order
 *     12 .. 14   P_p   = sum_k sum_x (w a) u_p          p = 0 1 2
 *     15         Q     = sum_k sum_x (w a) a
 *     16         W     = sum_k omega                    (a plain addition per frame)
 *   dark-field only:
 *     17 .. 25   MU_pq = sum_k m_p mu_q                 (p, q) = 00 01 02 10 11 12 20 21 22
 *     26 .. 31   WM_pq = sum_k (omega mu_p) mu_q        (p, q) = 00 01 02 11 12 22
 *     32 .. 40   NU_pq = sum_k n_p mu_q                 nine as MU
 *     41 .. 46   VM_pq = sum_k (nu mu_p) mu_q           six as WM
 *     47 .. 49   AU_p  = sum_k m_a mu_p                 p = 0 1 2
 * S, V, WM, VM are symmetric.  ROUNDING BOUND of a double evaluation, u = 2^-53, T = (2 Nw + 1)^2, derived as the sibling's:
 *     planes 0 .. 16:   (K T + 16) u sum |term|        (c: 4 roundings -- p q, p + q, + 1e-8, the division; w: 1 more, 5 in
 *                                                      all; v = w w: 2 x 5 + 1 = 11; the two differences g: 2; at most 2
 *                                                      products: 15 for the worst term, a V_pq; K T additions; 1 to spare.
 *                                                      W: its terms are w, 5 roundings and T + K additions)
 *     planes 17 .. 49:  (3 T + K + 20) u sum_k of the product of the factors' sums of absolute terms
 *                                                     (the worst plane, VM: nu: T additions and 11 roundings per term; each
 *                                                      mu: T additions, at most 2 roundings per term and the division by
 *                                                      win_sum, which is the double both evaluations divide by, T + 3;
 *                                                      2 products; K additions: 3 T + K + 19; 1 to spare.  The factors'
 *                                                      sums: sum_x |w' u_p| with w' = w or v, sum_x |w a|, sum_x w, sum_x v,
 *                                                      (sum_x |win[x] u_q|) / win_sum)
 * MODEL at the shift.
 *     plain        as include/umpa_sigma.h: T = P_2 / S_22 and A, B, h, rss0 of its plain model, from the planes 0 .. 15.
 *     dark-field   a ~ beta mu_2 + Kc r, with t1 = Q, t2 = WM_22, t3 = S_22, t4 = AU_2, t5 = P_2, t6 = MU_22 (the sums t1 .. t6
 *                  of the matchers' masked cost function) and det, Kc, beta, rss0 the sibling's expressions in t1 .. t6.
 *                  theta = (delta_i, delta_j, beta, Kc)      J = (Kc g_i + beta mu_0, Kc g_j + beta mu_1, mu_2, r)
 *                  e = a - beta mu_2 - Kc r.   With p, q in {0, 1}, KK = Kc * Kc, kb = Kc * beta, bb = beta * beta:
 *         A_pq = (KK * S_pq + kb * (MU_pq + MU_qp)) + bb * WM_pq
 *         A_p2 = Kc * MU_p2 + beta * WM_p2             A_p3 = Kc * S_p2 + beta * MU_2p
 *         A_22 = WM_22        A_23 = MU_22             A_33 = S_22
 *         B is A with V, NU, VM in place of S, MU, WM:
 *         B_pq = (KK * V_pq + kb * (NU_pq + NU_qp)) + bb * VM_pq
 *         B_p2 = Kc * NU_p2 + beta * VM_p2             B_p3 = Kc * V_p2 + beta * NU_2p
 *         B_22 = VM_22        B_23 = NU_22             B_33 = V_22
 *         h_p  = Kc * ((P_p - beta * MU_p2) - Kc * S_p2) + beta * ((AU_p - beta * WM_p2) - Kc * MU_2p)
 *         h_2  = (AU_2 - beta * WM_22) - Kc * MU_22    h_3  = (P_2 - beta * MU_22) - Kc * S_22
 * SOLVE is include/umpa_sigma.h's, word for word, with one change:  dof = W - tr.  The expected weighted residual per unit
 * noise variance is tr(diag w) - tr(A^-1 B); with weights that sum to 1 per frame that is K - tr, with pair weights it is W - tr.
 * OUTPUT as include/umpa_sigma.h.  A window without any pair weight has all moments 0: T (Kc, beta) is 0 / 0, the first pivot
 * is NaN, hence BAD: valid = 0 and NaN outputs.  A NaN pixel under a zero weight still poisons every window that holds it
 * (0 * NaN), as it poisons the reference's masked cost.
 * Everything after the moments is fp64 + - * / in the order written, without contraction.
 *
 * Arrays: shift 2 * N0 * N1 ints (read); moments P * N0 * N1 doubles or NULL; unit 3 * N0 * N1 doubles; s2, dof N0 * N1
 * doubles; valid N0 * N1 ints.  Host arrays by default: the shift field is uploaded and the results are downloaded, the frames
 * stay where they are.  With UMPA_HIP_F_DEVICE_IO they are device arrays on the model's device and the kernel runs on `stream`.
 * Either way the call is ordered after everything the model has enqueued on any stream (it waits for the model's device
 * first) and returns when the results are written.
 * UMPA_HIP_E_ARG, before anything touches a device: a NULL model, shift, unit, s2, dof or valid; a flag other than
 * UMPA_HIP_F_DEVICE_IO; N < 1, step < 1 or start < 0 on either axis.  UMPA_HIP_E_ARG, before any kernel is launched or memory
 * allocated (the extent is the model's): start + step (N - 1) > H - 2 pad - 1 (resp. W).
 * UMPA_HIP_E_UNSUPPORTED, before any kernel is launched, with a text that names the reason and the values: the kernel
 * dark-field model; frames of unequal shapes or at non-zero positions; a reference-coordinate model (ref_mode != 0); Nw
 * outside 1 .. 8; padding != Nw + max_shift; a window that is not finite, non-negative and normalised (|sum win - 1| <= 1e-9).
 * One lane per pixel, one writer per output, no atomics: the output is the same bit for bit from run to run and for host and
 * device arrays. */
#define UMPA_GRID_SIGMA_PLANES_PLAIN 17
#define UMPA_GRID_SIGMA_PLANES_DF 50
int umpa_grid_uncertainty(umpa_hip_model *m, int start0, int step0, int N0, int start1, int step1, int N1,
                          const int *shift, double *moments, double *unit, double *s2, double *dof, int *valid,
                          int flags, void *stream);

const char *umpa_grid_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UMPA_GRID_H */
