#!/usr/bin/env python3
"""what the sequence search costs beside the tracked search, the grid search and a plain copy of its
state.

    python tools/sequence_rate.py [--out FILE] [--repeats N] [--configs C2,C3]

Per config (tools/grid_rate.py's: BASELINE C2 and C3, dark-field, synthetic stacks) in ONE process, alternating, N times
after a warm-up of each, on device-resident arrays (F_DEVICE_IO, no transfers):
    search='grid', track in nearest mode (a seeded random prior), sequence without a state (a series starts: the next state
    is written), sequence with a state (read and written; the state is the first call's output)
the per-kernel HIP-event times of the library's own timers (`table_consumer` brackets grid_min_kernel, grid_track_kernel or
grid_sequence_kernel) and the host wall time of the call around a stream synchronise; then a device-to-device copy of one
state, 2 U^2 8 N0 N1 bytes of traffic, timed with HIP events: the floor of any kernel that reads one state and writes another.
At C2 also the wall time of Sequence.step beside Tracker.step and stage_sample + match(search='grid') on the same host frames.
Median and range over the repeats.  No pass mark: the rows are the measurement.
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
import track_rate as TR    # noqa: E402

LAM_SHARE = 0.2              # lam as a share of the median gap between a pixel's two lowest costs (a 64-row sample)


def sequence_calls(m, lam):
    """sequence without and with a state on device-resident arrays: closures that enqueue on the current torch stream"""
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    U = 2 * m.max_shift - 1
    dev = torch.device("cuda", m._device)
    states = [torch.zeros((U, U, N0, N1), dtype=torch.float64, device=dev) for _ in range(2)]
    dbl = [torch.zeros((N0, N1), dtype=torch.float64, device=dev) for _ in range(8)]          # f T dx dy cost df | total cost0
    ints = [torch.zeros((N0, N1), dtype=torch.int32, device=dev) for _ in range(4)]           # si sj err | moved
    ptrs = [t.data_ptr() for t in dbl[:6] + ints[:3] + dbl[6:] + ints[3:]]
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(prev, nxt):
        def fn():
            g = _lib.grid()
            g.check(g.sequence(m._handle, 0, 1, N0, 0, 1, N1, prev.data_ptr() if prev is not None else None, lam, float("inf"),
                               nxt.data_ptr(), *ptrs, _lib.F_DEVICE_IO, sp), "grid sequence")
        return fn
    return {"sequence_start": call(None, states[0]), "sequence": call(states[0], states[1])}, (states, dbl, ints)


def copy_ms(states, repeats):
    import torch
    a, b = states
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(repeats + 1):
        ev[0].record()
        b.copy_(a)
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return out[1:]


def steps(m, sam, lam, repeats):
    """wall time per projection of the three step series on the same host frames, uploads included"""
    import torch
    from umpa_amd import Sequence, Tracker
    frames = list(sam)
    seq, trk = Sequence(m, lam), Tracker(m)

    def grid():
        m.stage_sample(frames)
        return m.match(quiet=True, search="grid")
    calls = {"stage_sample + match(search='grid')": grid, "Tracker.step": lambda: trk.step(frames), "Sequence.step": lambda: seq.step(frames)}
    series = {k: [] for k in calls}
    for r in range(repeats + 2):                                      # two warm-ups: the first step of a series has no state
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                series[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in series.items()}


def run_config(name, repeats):
    import numpy as np
    from umpa_amd import model
    from umpa_amd.synth import make_stack
    c = GR.CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    N0, N1 = m.extent
    v = m.cost_volume(ROI=((N0 // 2, N0 // 2 + 64, 1), (0, N1, 1)))["cost"]
    low = np.sort(v.reshape(v.shape[0] ** 2, -1), axis=0)[:2]
    lam = LAM_SHARE * float(np.median(low[1] - low[0]))
    pdx, pdy = TR.prior(m)
    calls, keep = GR.device_calls(m, with_volume=False)
    calls = {"grid": calls["grid"]}
    more, keep2 = TR.track_calls(m, pdx, pdy)
    calls["track_nearest"] = more["track_nearest"]
    more, keep3 = sequence_calls(m, lam)
    calls.update(more)
    for fn in calls.values():                                        # warm-up: code objects, scratch, the table; the state of "sequence"
        GR.timed(m, fn)
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                                  # alternating
            series[k].append(GR.timed(m, fn))
    out = {}
    for k, runs in series.items():
        out[k] = {}
        for kern in sorted(set().union(*runs)):
            val = [r.get(kern, 0.0) for r in runs]
            out[k][kern] = dict(median=round(statistics.median(val), 3), min=round(min(val), 3), max=round(max(val), 3))
    cp = copy_ms(keep3[0], repeats)
    state_bytes = keep3[0][0].numel() * 8
    del keep, keep2, keep3
    host = steps(m, sam, lam, repeats) if name == "C2" else None
    return out, dict(median=statistics.median(cp), min=min(cp), max=max(cp), bytes=2 * state_bytes), host, lam


def fmt(name, res, cp, host, lam, c):
    label = {"grid": "search='grid' (grid_min_kernel)", "track_nearest": "track, nearest mode (grid_track_kernel)",
             "sequence_start": "sequence, no state in, state out (grid_sequence_kernel)",
             "sequence": "sequence, state in and out, lam %.3e, no truncation (grid_sequence_kernel)" % lam}
    lines = ["%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field; ms per call, median [min .. max]" % (name, c["n"], c["K"], c["Nw"], c["ms"])]
    for call, kernels in res.items():
        lines.append("  %s" % label[call])
        for kern, v in kernels.items():
            lines.append("    %-16s %9.3f  [%9.3f .. %9.3f]" % (kern, v["median"], v["min"], v["max"]))
    tc = lambda call: res[call]["table_consumer"]["median"]
    lines.append("  device copy of one state (%.2f GB read + written): %9.3f  [%9.3f .. %9.3f] ms, %.0f GB/s" % (
        cp["bytes"] / 1e9, cp["median"], cp["min"], cp["max"], cp["bytes"] / cp["median"] / 1e6))
    lines.append("  grid_sequence_kernel / grid_track_kernel: %.2f (no state in: %.2f), / grid_min_kernel: %.2f, / the copy: %.2f (medians of table_consumer)" % (
        tc("sequence") / tc("track_nearest"), tc("sequence_start") / tc("track_nearest"), tc("sequence") / tc("grid"), tc("sequence") / cp["median"]))
    if host:
        lines.append("  step series on host frames, upload included, wall ms per projection")
        for call, v in host.items():
            lines.append("    %-36s %9.3f  [%9.3f .. %9.3f]" % (call, v["median"], v["min"], v["max"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="C2,C3")
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        res, cp, host, lam = run_config(name, a.repeats)
        first = len(lines)
        lines += fmt(name, res, cp, host, lam, GR.CONFIGS[name])
        print("\n".join(lines[first:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
