#!/usr/bin/env python3
"""what window widening costs beside the same search without it, beside its floor, and beside the
model it stands in for.

    python tools/widen_rate.py [--out FILE] [--repeats N] [--configs C2,C3] [--widths 1,4]

Per config (tools/grid_rate.py's: BASELINE C2 and C3, dark-field, synthetic stacks) in ONE process, alternating, N times
after a warm-up of each:
    search='grid' through umpa_grid_wide_match_region at widen = 0 and at each half-width b, device-resident outputs
    (F_DEVICE_IO, no transfers): the library's own per-kernel HIP-event times (`table_consumer` brackets the widen kernels
    -- maps, table, carry -- and grid_min_kernel) and the host wall time around a stream synchronise;
    a device-to-device copy of as many bytes as the whole shift table has, timed with events in the same process: the
    filter reads and writes each entry once, so the copy is its floor.
`table_consumer` at b less `table_consumer` at 0 is what the widen kernels add (grid_min_kernel runs on fewer valid pixels
then, so the difference is if anything an underestimate by the border's share).  Where Nw + b <= 8, the host-array call
match(search='grid', widen=b) is set beside the call without widen and beside a fresh model of window_size = Nw + b,
its construction and its match(search='grid') included.  Median and range over the repeats.  No pass mark: the rows are the measurement.
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

import grid_rate as GR     # noqa: E402


def wide_calls(m, widths):
    """search='grid' at widen 0 and every b of `widths` on device-resident outputs"""
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    dev = torch.device("cuda", m._device)
    values = torch.zeros((m.Nparam, N0, N1), dtype=torch.float64, device=dev)
    err = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(b):
        def fn():
            g = _lib.grid()
            g.check(g.wide_match_region(m._handle, 0, 1, N0, 0, 1, N1, b, values.data_ptr(), m.Nparam, None, err.data_ptr(), None, 0.0,
                                        None, None, None, _lib.F_DEVICE_IO | _lib.F_PLANAR, sp), "grid wide_match_region")
        return fn
    return {"widen %d" % b: call(b) for b in (0,) + tuple(widths)}, (values, err)


def copy_floor(m, repeats):
    """ms of a device-to-device copy of the whole table's bytes (in pieces of at most 1 GiB, as the table itself is chunked)"""
    import torch
    N0, N1 = m.extent
    U = 2 * m.max_shift - 1
    total = U * U * N0 * ((N1 + 31) // 32 * 32) * 8
    piece = min(total, 1 << 30)
    dev = torch.device("cuda", m._device)
    a, b = (torch.empty(piece // 8, dtype=torch.float64, device=dev) for _ in range(2))
    a.zero_()
    out = []
    for n in range(repeats + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        done = 0
        while done < total:
            k = min(piece, total - done) // 8
            b[:k].copy_(a[:k])
            done += k * 8
        t1.record()
        torch.cuda.synchronize()
        if n:
            out.append(t0.elapsed_time(t1))
    return total, out


def host_api(m, sam, ref, c, widths, repeats):
    """wall ms of the host-array calls: match(search='grid', widen=b) beside a fresh model of the wider window"""
    from umpa_amd import model
    calls = {"match(search='grid')": lambda: m.match(quiet=True, search="grid")}
    for b in widths:
        calls["match(search='grid', widen=%d)" % b] = lambda b=b: m.match(quiet=True, search="grid", widen=b)
        if c["Nw"] + b <= 8:
            calls["fresh model, window_size %d, match(search='grid')" % (c["Nw"] + b)] = \
                lambda b=b: model.UMPAModelDF(sam, ref, window_size=c["Nw"] + b, max_shift=c["ms"]).match(quiet=True, search="grid")
    for fn in calls.values():
        fn()
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            series[k].append((time.perf_counter() - t0) * 1e3)
    return series


def stat(v):
    return "%9.3f  [%9.3f .. %9.3f]" % (statistics.median(v), min(v), max(v))


def run_config(name, repeats, widths):
    from umpa_amd import model
    from umpa_amd.synth import make_stack
    c = GR.CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    calls, keep = wide_calls(m, widths)
    for fn in calls.values():
        GR.timed(m, fn)
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                                  # alternating
            series[k].append(GR.timed(m, fn))
    lines = ["%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field; ms per call, median [min .. max] of %d" % (name, c["n"], c["K"], c["Nw"], c["ms"], repeats)]
    for k, runs in series.items():
        lines.append("  search='grid', %s (umpa_grid_wide_match_region, device arrays)" % k)
        for kern in sorted(set().union(*runs)):
            lines.append("    %-16s %s" % (kern, stat([r.get(kern, 0.0) for r in runs])))
    base = statistics.median([r.get("table_consumer", 0.0) for r in series["widen 0"]])
    total, floor = copy_floor(m, repeats)
    lines.append("  device-to-device copy of the table's %.2f GB (read once, written once: the filter's floor)  %s" % (total / 1e9, stat(floor)))
    for b in widths:
        tc = statistics.median([r.get("table_consumer", 0.0) for r in series["widen %d" % b]])
        lines.append("  widen %d: table_consumer %.3f - %.3f at widen 0 = %.3f ms for the widen kernels, %.2f x the copy" % (
            b, tc, base, tc - base, (tc - base) / statistics.median(floor)))
    lines.append("  host-array API, transfers included, wall ms")
    for k, v in host_api(m, sam, ref, c, widths, repeats).items():
        lines.append("    %-56s %s" % (k, stat(v)))
    del keep
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--widths", default="1,4")
    a = ap.parse_args()
    widths = tuple(int(b) for b in a.widths.split(","))
    lines = []
    for name in a.configs.split(","):
        first = len(lines)
        lines += run_config(name, a.repeats, widths)
        print("\n".join(lines[first:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
