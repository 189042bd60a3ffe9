#!/usr/bin/env python3
"""what the tracked search costs beside the table's other consumers and beside the host route it
replaces.

    python tools/track_rate.py [--out FILE] [--repeats N] [--configs C2,C3]

Per config (tools/grid_rate.py's: BASELINE C2 and C3, dark-field, synthetic stacks) in ONE process, alternating, N times
after a warm-up of each:
    search='grid', basins with K = 1 and 4, track in nearest mode and in penalty mode (a seeded random prior within
    +-(max_shift + 1), on the device)
the per-kernel HIP-event times of the library's own timers (`table_consumer` brackets grid_min_kernel, grid_basins_kernel
or grid_track_kernel), device-resident priors and outputs (F_DEVICE_IO, no transfers), and the host wall time of the whole
call around a stream synchronise; then the ratios of grid_track_kernel to grid_min_kernel and to grid_basins_kernel K = 1,
which read the same table entries once.  Then the host-array API, transfers included: model.track() beside match(),
match(search='grid') and the host route it replaces, basins(k=4) + basins.nearest + basins.select.  Median and range over
the repeats.  No pass mark: the rows are the measurement.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import basins_rate as BR   # noqa: E402
import grid_rate as GR     # noqa: E402

BR.KS = (1, 4)               # basins_calls() reads it: the two K this comparison wants
LAM, RADIUS = 0.05, 3.0


def prior(m, seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    r = m.max_shift + 1
    return rng.uniform(-r, r, m.extent), rng.uniform(-r, r, m.extent)      # (prior_dx, prior_dy)


def track_calls(m, pdx, pdy):
    """track in both modes on device-resident priors and outputs: closures that enqueue on the current torch stream"""
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    dev = torch.device("cuda", m._device)
    pj, pi = torch.from_numpy(pdx).to(dev), torch.from_numpy(pdy).to(dev)
    dbl = [torch.zeros((N0, N1), dtype=torch.float64, device=dev) for _ in range(7)]          # f T dx dy cost df | cost0
    ints = [torch.zeros((N0, N1), dtype=torch.int32, device=dev) for _ in range(5)]           # si sj err | count found
    ptrs = [t.data_ptr() for t in dbl[:6] + ints[:3] + dbl[6:] + ints[3:]]
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(mode, lam, radius):
        def fn():
            g = _lib.grid()
            g.check(g.track(m._handle, 0, 1, N0, 0, 1, N1, pi.data_ptr(), pj.data_ptr(), mode, lam, radius, *ptrs, _lib.F_DEVICE_IO, sp), "grid track")
        return fn
    return {"track_nearest": call(_lib.GRID_TRACK_NEAREST, 0.0, -1.0), "track_penalty": call(_lib.GRID_TRACK_PENALTY, LAM, RADIUS)}, (pi, pj, dbl, ints)


def host_api(m, pdx, pdy, repeats):
    """wall time of the host-array calls, transfers included"""
    from umpa_amd import basins as B

    def host_route():
        b = m.basins(k=4)
        return B.select(b, B.nearest(b, pdx, pdy))
    calls = {"match()": lambda: m.match(quiet=True), "match(search='grid')": lambda: m.match(quiet=True, search="grid"),
             "basins(k=4) + nearest + select": host_route, "track()": lambda: m.track(pdx, pdy),
             "track(lam, radius)": lambda: m.track(pdx, pdy, lam=LAM, radius=RADIUS)}
    for fn in calls.values():
        fn()
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            series[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in series.items()}


def run_config(name, repeats):
    from umpa_amd import model
    from umpa_amd.synth import make_stack
    c = GR.CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    pdx, pdy = prior(m)
    calls, keep = GR.device_calls(m, with_volume=False)
    calls = {"grid": calls["grid"]}
    more, keep2 = BR.basins_calls(m)
    calls.update(more)
    more, keep3 = track_calls(m, pdx, pdy)
    calls.update(more)
    for fn in calls.values():                                        # warm-up: code objects, scratch, the table
        GR.timed(m, fn)
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                                  # alternating
            series[k].append(GR.timed(m, fn))
    out = {}
    for k, runs in series.items():
        out[k] = {}
        for kern in sorted(set().union(*runs)):
            v = [r.get(kern, 0.0) for r in runs]
            out[k][kern] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    del keep, keep2, keep3
    return out, host_api(m, pdx, pdy, repeats)


def fmt(name, res, host, c):
    label = {"grid": "search='grid' (grid_min_kernel)", "track_nearest": "track, nearest mode (grid_track_kernel)",
             "track_penalty": "track, penalty mode, lam %g, radius %g (grid_track_kernel)" % (LAM, RADIUS)}
    label.update({"basins%d" % k: "basins, K = %d (grid_basins_kernel)" % k for k in BR.KS})
    lines = ["%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field; ms per call, median [min .. max]" % (name, c["n"], c["K"], c["Nw"], c["ms"])]
    for call, kernels in res.items():
        lines.append("  %s" % label[call])
        for kern, v in kernels.items():
            lines.append("    %-16s %9.3f  [%9.3f .. %9.3f]" % (kern, v["median"], v["min"], v["max"]))
    tc = lambda call: res[call]["table_consumer"]["median"]
    for call in ("track_nearest", "track_penalty"):
        lines.append("  grid_track_kernel (%s) / grid_min_kernel: %.2f, / grid_basins_kernel K = 1: %.2f, K = 4: %.2f (medians of table_consumer)" % (
            call.split("_")[1], tc(call) / tc("grid"), tc(call) / tc("basins1"), tc(call) / tc("basins4")))
    lines.append("  host-array API, transfers included, wall ms")
    for call, v in host.items():
        lines.append("    %-32s %9.3f  [%9.3f .. %9.3f]" % (call, v["median"], v["min"], v["max"]))
    lines.append("  track() / (basins(k=4) + nearest + select), medians: %.2f" % (host["track()"]["median"] / host["basins(k=4) + nearest + select"]["median"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="C2,C3")
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        res, host = run_config(name, a.repeats)
        first = len(lines)
        lines += fmt(name, res, host, GR.CONFIGS[name])
        print("\n".join(lines[first:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
