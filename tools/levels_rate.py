#!/usr/bin/env python3
"""what the scale-space search costs beside the chain of separate calls it replaces.

    python tools/levels_rate.py [--out FILE] [--repeats N] [--configs C2,C3] [--levels 4,2,1,0]

Per config (tools/grid_rate.py's: BASELINE C2 and C3, dark-field, synthetic stacks, here as HIP tensors so that every map
stays on the device) in ONE process, alternating, N times after a warm-up of each:
    umpa_amd.levels.scale_space(model, levels)       one call: one table pass, every level, the selection;
    umpa_amd.widen.coarse_to_fine(model, levels)     one call per level, each with its own table and maps (unchanged
                                                     from the commit before this module);
the library's own per-kernel HIP-event times (`table_consumer` brackets everything a consumer enqueues per chunk: the
pooling, the priors, grid_track_kernel per level, the selection) and the host wall time around a synchronise; then a
device-to-device copy of as many bytes as the whole shift table has, timed with events in the same process.  The peak of
the device allocator's reserved bytes is read around each call for the workspace.  Median and range over the repeats.  No
pass mark: the rows are the measurement.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_rate as GR     # noqa: E402
import widen_rate as WR    # noqa: E402


def run_config(name, repeats, levels):
    import torch
    from umpa_amd import levels as LV, model, widen
    from umpa_amd.synth import make_stack
    c = GR.CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    dev = torch.device("cuda", 0)
    sam, ref = ([torch.as_tensor(f, device=dev).contiguous() for f in s] for s in (sam, ref))
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    calls = {"scale_space": lambda: LV.scale_space(m, levels=levels), "coarse_to_fine": lambda: widen.coarse_to_fine(m, levels=levels)}
    free = {}
    for k, fn in calls.items():                                      # warm-up; the device memory a call takes beyond the model
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(dev)[0]
        out = fn()
        torch.cuda.synchronize()
        free[k] = before - torch.cuda.mem_get_info(dev)[0]
        del out
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                                  # alternating
            series[k].append(GR.timed(m, fn))
    lines = ["%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field, HIP-tensor model, levels %s; ms per call, median [min .. max] of %d"
             % (name, c["n"], c["K"], c["Nw"], c["ms"], tuple(levels), repeats)]
    for k, runs in series.items():
        lines.append("  %s (device memory held after the first call, outputs and pools included: %.2f GB)" % (k, free[k] / 1e9))
        for kern in sorted(set().union(*runs)):
            lines.append("    %-16s %s" % (kern, WR.stat([r.get(kern, 0.0) for r in runs])))
    total, floor = WR.copy_floor(m, repeats)
    lines.append("  device-to-device copy of the table's %.2f GB (read once, written once)  %s" % (total / 1e9, WR.stat(floor)))
    med = lambda k, kern: statistics.median([r.get(kern, 0.0) for r in series[k]])
    lines.append("  wall: coarse_to_fine / scale_space = %.2f; table_consumer %.3f against %.3f ms; the table kernels %.3f against %.3f ms"
                 % (med("coarse_to_fine", "wall") / med("scale_space", "wall"), med("scale_space", "table_consumer"), med("coarse_to_fine", "table_consumer"),
                    med("scale_space", "corr_volume") + med("scale_space", "corr_march"), med("coarse_to_fine", "corr_volume") + med("coarse_to_fine", "corr_march")))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--levels", default="4,2,1,0")
    a = ap.parse_args()
    levels = tuple(int(b) for b in a.levels.split(","))
    lines = []
    for name in a.configs.split(","):
        first = len(lines)
        lines += run_config(name, a.repeats, levels)
        print("\n".join(lines[first:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
