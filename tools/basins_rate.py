#!/usr/bin/env python3
"""what basin enumeration costs beside the table's other consumers.

    python tools/basins_rate.py [--out FILE] [--repeats N] [--configs C2,C3]

Per config (tools/grid_rate.py's: BASELINE C2 and C3, dark-field, synthetic stacks) in ONE process, alternating, N times
after a warm-up of each:
    search='walk', search='grid', cost_volume(with_fit) of a 256-row ROI, basins with K = 1, 4, 8
the per-kernel HIP-event times of the library's own timers (`table_consumer` brackets grid_min_kernel, cost_volume_kernel
or grid_basins_kernel, launched where `replay_walk` would be), device-resident outputs (F_DEVICE_IO, no downloads), and
the host wall time of the whole call around a stream synchronise; then the ratio of grid_basins_kernel to
grid_min_kernel, which reads the same table entries once.  Then the host-array API, downloads included:
model.basins(k=4) beside match(search='grid') and match().  Median and range over the repeats.
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

import grid_rate as GR   # noqa: E402

KS = (1, 4, 8)


def basins_calls(m):
    """basins(K) on device-resident outputs for every K of KS: closures that enqueue on the current torch stream"""
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    dev = torch.device("cuda", m._device)
    kmax = max(KS)
    dbl = [torch.zeros((kmax, N0, N1), dtype=torch.float64, device=dev) for _ in range(6)]
    ints = [torch.zeros((kmax, N0, N1), dtype=torch.int32, device=dev) for _ in range(3)] + [torch.zeros((N0, N1), dtype=torch.int32, device=dev)]
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(k):
        def fn():
            g = _lib.grid()
            g.check(g.basins(m._handle, 0, 1, N0, 0, 1, N1, k, *[t.data_ptr() for t in dbl + ints], _lib.F_DEVICE_IO, sp), "grid basins")
        return fn
    return {"basins%d" % k: call(k) for k in KS}, (dbl, ints)


def host_api(m, repeats):
    """wall time of the host-array calls, downloads included"""
    calls = {"match()": lambda: m.match(quiet=True), "match(search='grid')": lambda: m.match(quiet=True, search="grid"),
             "basins(k=4)": lambda: m.basins(k=4)}
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
    calls, keep = GR.device_calls(m)
    more, keep2 = basins_calls(m)
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
    del keep, keep2
    return out, host_api(m, max(3, repeats // 2))


def fmt(name, res, host, c):
    label = {"walk": "search='walk'", "grid": "search='grid' (grid_min_kernel)",
             "volume": "cost_volume, %d rows, with T and df (cost_volume_kernel)" % GR.ROI_ROWS}
    label.update({"basins%d" % k: "basins, K = %d (grid_basins_kernel)" % k for k in KS})
    lines = ["%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field; ms per call, median [min .. max]" % (name, c["n"], c["K"], c["Nw"], c["ms"])]
    for call, kernels in res.items():
        lines.append("  %s" % label[call])
        for kern, v in kernels.items():
            lines.append("    %-16s %9.3f  [%9.3f .. %9.3f]" % (kern, v["median"], v["min"], v["max"]))
    gm = res["grid"]["table_consumer"]["median"]
    lines.append("  grid_basins_kernel / grid_min_kernel (medians of table_consumer): " +
                 ", ".join("K = %d: %.2f" % (k, res["basins%d" % k]["table_consumer"]["median"] / gm) for k in KS))
    lines.append("  host-array API, downloads included, wall ms")
    for call, v in host.items():
        lines.append("    %-22s %9.3f  [%9.3f .. %9.3f]" % (call, v["median"], v["min"], v["max"]))
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
