#!/usr/bin/env python3
"""what the grid consumers cost on a masked model, beside its walk, beside their siblings on the
unmasked stack and beside a copy of the bytes they must read.

    python tools/masked_grid_rate.py [--out FILE] [--repeats N] [--size 2048]

BASELINE config C2's stack (tools/masked_rate.py's: 2048^2 x 10 frames, Nw 5, max_shift 5, dark-field) with a 95 % binary mask,
switch on, and the same stack without masks, in ONE process, device-resident arrays (F_DEVICE_IO, no transfers), alternating, N
times after a warm-up of each call:
    search='walk' (forced onto the tiled path), search='grid', cost_volume of 256 rows with T and df, basins (k = 4), track in
    nearest mode (a seeded random prior), sequence with a state in and out
the per-kernel HIP-event times of the library's own timers (`table_consumer` brackets the masked_* kernel or its sibling,
`corr_masked` / `corr_volume` the table kernel; with a consumer set the on-demand stages are off, so the table kernel computes
every pass) and the host wall time of the call around a stream synchronise.  Then a device-to-device copy of (2 max_shift - 1)^2
N0 N1 doubles -- the cost plane of every shift at every pixel, what a masked consumer must read at the least; the copy reads and
writes that much -- timed with HIP events.  Median and range over the repeats.  No pass mark: the rows are the measurement.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import basins_rate as BR     # noqa: E402
import grid_rate as GR       # noqa: E402
import sequence_rate as SR   # noqa: E402
import track_rate as TR      # noqa: E402

K, NW, MS = 10, 5, 5


def covered_grid(m):
    """search='grid' with the coverage map match() forms (device-resident), for a masked model"""
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    dev = torch.device("cuda", m._device)
    values = torch.zeros((m.Nparam, N0, N1), dtype=torch.float64, device=dev)
    err = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
    cm = m.coverage()
    cover = torch.from_numpy(cm).to(dev)
    thr = float(.1 * cm.max() / K)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    flags = _lib.F_DEVICE_IO | _lib.F_PLANAR
    region = (m._handle, 0, 1, N0, 0, 1, N1, values.data_ptr(), m.Nparam, None, err.data_ptr(), cover.data_ptr(), thr, None, None, None)

    def walk():
        m._lib.check(m._lib.match_region(*region, flags | _lib.F_FORCE_TILED, sp), "match_region")

    def grid():
        g = _lib.grid()
        g.check(g.match_region(*region, flags, sp), "grid match_region")
    return dict(walk=walk, grid=grid), (values, err, cover)


def calls_of(m, masked):
    calls, keep = GR.device_calls(m)
    if masked:
        more, keep0 = covered_grid(m)
        calls.update(more)
        keep = (keep, keep0)
    b, keep1 = BR.basins_calls(m)
    calls["basins4"] = b["basins4"]
    pdx, pdy = TR.prior(m)
    t, keep2 = TR.track_calls(m, pdx, pdy)
    calls["track_nearest"] = t["track_nearest"]
    s, keep3 = SR.sequence_calls(m, 1e-3)
    calls["sequence_start"], calls["sequence"] = s["sequence_start"], s["sequence"]
    return calls, (keep, keep1, keep2, keep3)


def measure(m, masked, repeats):
    calls, keep = calls_of(m, masked)
    for fn in calls.values():                                        # warm-up: code objects, scratch, the table; the state of "sequence"
        GR.timed(m, fn)
    series = {k: [] for k in calls if k != "sequence_start"}
    for _ in range(repeats):
        for k in series:                                             # alternating
            series[k].append(GR.timed(m, calls[k]))
    out = {}
    for k, runs in series.items():
        out[k] = {}
        for kern in sorted(set().union(*runs)):
            val = [r.get(kern, 0.0) for r in runs]
            out[k][kern] = dict(median=round(statistics.median(val), 3), min=round(min(val), 3), max=round(max(val), 3))
    cp = SR.copy_ms(keep[3][0], repeats)                             # the two states: U^2 N0 N1 doubles each
    nbytes = keep[3][0][0].numel() * 8
    return out, dict(median=statistics.median(cp), min=min(cp), max=max(cp), bytes=nbytes)


LABEL = {"walk": "search='walk', forced onto the tiled path", "grid": "search='grid'", "volume": "cost_volume, %d rows, with T and df" % GR.ROI_ROWS,
         "basins4": "basins, k = 4", "track_nearest": "track, nearest mode", "sequence": "sequence, state in and out"}


def fmt(title, res, cp):
    lines = ["%s; ms per call, median [min .. max]" % title]
    for call, kernels in res.items():
        lines.append("  %s" % LABEL[call])
        for kern, v in kernels.items():
            lines.append("    %-16s %9.3f  [%9.3f .. %9.3f]" % (kern, v["median"], v["min"], v["max"]))
    lines.append("  device copy of the cost planes (%.2f GB read, as much written): %9.3f  [%9.3f .. %9.3f] ms, %.0f GB/s of traffic" % (
        cp["bytes"] / 1e9, cp["median"], cp["min"], cp["max"], 2 * cp["bytes"] / cp["median"] / 1e6))
    return lines


def main():
    import numpy as np
    from umpa_amd import model
    from umpa_amd.synth import make_stack
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    a = ap.parse_args()
    sam, ref, _ = make_stack(a.size, a.size, K, MS, df=True, seed=0, order=1)
    mask = (np.random.default_rng(1).uniform(size=sam.shape) < 0.95).astype(np.float64)
    lines, med = [], {}
    for masked in (True, False):
        m = model.UMPAModelDF(sam, ref, mask_list=mask if masked else None, window_size=NW, max_shift=MS)
        if masked:
            m.masked_grid = True
        res, cp = measure(m, masked, a.repeats)
        med[masked] = (res, cp)
        title = "C2%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field" % (" + 95 % binary mask, masked_grid on" if masked else ", no masks", a.size, K, NW, MS)
        first = len(lines)
        lines += fmt(title, res, cp)
        print("\n".join(lines[first:]), flush=True)
        del m
    rm, cm = med[True]
    rp, _ = med[False]
    first = len(lines)
    lines.append("masked consumer: table_consumer ms | wall / the masked walk's wall | table_consumer / the plain sibling's | table_consumer / the copy")
    for call in ("grid", "volume", "basins4", "track_nearest", "sequence"):
        tc, sib = rm[call]["table_consumer"]["median"], rp[call]["table_consumer"]["median"]
        # (the volume call covers ROI_ROWS of the rows: the copy of as many rows is that share of the whole copy)
        share = min(1.0, GR.ROI_ROWS / float(a.size - 2 * (NW + MS))) if call == "volume" else 1.0
        lines.append("  %-14s %9.3f | %6.2f | %6.2f | %6.2f" % (call, tc, rm[call]["wall"]["median"] / rm["walk"]["wall"]["median"], tc / sib,
                                                              tc / (cm["median"] * share)))
    lines.append("  corr_masked under a consumer (every pass): %.3f ms; under the walk (on-demand passes): %.3f ms" % (
        rm["grid"]["corr_masked"]["median"], rm["walk"]["corr_masked"]["median"]))
    print("\n".join(lines[first:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
