#!/usr/bin/env python3
"""Rate of the model-resident uncertainty maps (umpa_grid_uncertainty) on one GPU, at BASELINE config C2's shape (2048 x 2048,
10 frames, Nw = 5, max_shift = 5).  Medians of 3 after a warm-up, all in one process:

  front     the wall time of model.uncertainty(result, resident=True) beside model.uncertainty(result) of the same
            host-frame dark-field model (the default call stacks and uploads both stacks per call);
  kernel    the resident call on a device shift field (UMPA_HIP_F_DEVICE_IO: the kernel and its launch) beside
            umpa_sigma_region on device copies of the same stacks, dark-field and plain;
  masked    the resident call on the same stacks with the 95 % binary mask of tools/masked_rate.py, beside the unmasked one.

    python tools/resident_sigma_rate.py [--out FILE] [--size N]

Writes profiles/resident_sigma_rate.txt (or FILE).  Nothing here is a gate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps=3):
    import torch
    fn()                                                              # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_sigma_rate.txt"))
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    import torch
    from umpa_amd import model, sigma
    from umpa_amd.synth import make_stack

    H = W = args.size
    K, Nw, ms = 10, 5, 5
    sam, ref, _ = make_stack(H, W, K, ms, df=True, seed=0, order=1)
    mask = (np.random.default_rng(1).uniform(size=sam.shape) < 0.95).astype(np.float64)
    dev = torch.device("cuda", 0)
    lines = ["# tools/resident_sigma_rate.py: %s, %d x %d pixels, %d frames, Nw = %d, max_shift = %d; ms, medians of 3 after a warm-up"
             % (torch.cuda.get_device_name(0), H, W, K, Nw, ms), "# (the three runs in brackets)"]

    def row(name, fn):
        med, times = median_ms(fn)
        lines.append("%-64s %9.2f   [%s]" % (name, med, ", ".join("%.2f" % t for t in times)))
        print(lines[-1], flush=True)
        return med

    tsam, tref = torch.from_numpy(sam).to(dev), torch.from_numpy(ref).to(dev)
    for df in (True, False):
        tag = "dark-field" if df else "plain"
        cls = model.UMPAModelDF if df else model.UMPAModelNoDF
        kind = int(df)
        m = cls(list(sam), list(ref), window_size=Nw, max_shift=ms, device=0)
        res = m.match(quiet=True)
        N0, N1 = res["dx"].shape
        reg = (0, 1, N0, 0, 1, N1)
        shift = sigma.shift_field(res, ms)
        tshift = torch.from_numpy(shift).to(dev)
        if df:
            lines.append("## front: host-frame %s model, %d x %d pixels, match() %.2f ms" % (tag, N0, N1, median_ms(lambda: m.match(quiet=True))[0]))
            a = row("model.uncertainty(result, resident=True)   wall", lambda: m.uncertainty(res, resident=True))
            b = row("model.uncertainty(result)                  wall", lambda: m.uncertainty(res))
            lines.append("#   default / resident = %.1f" % (b / a))
        lines.append("## kernel: %s, device shift field and device outputs" % tag)
        a = row("umpa_grid_uncertainty, model's frames (unmasked)", lambda: sigma.resident(m, reg, tshift))
        b = row("umpa_sigma_region, device copies of the stacks", lambda: sigma.region(tsam, tref, m.window, ms, kind, reg, tshift))
        lines.append("#   resident / sibling = %.3f" % (a / b))
        del m
        mm = cls(list(sam), list(ref), mask_list=list(mask), window_size=Nw, max_shift=ms, device=0)
        c = row("umpa_grid_uncertainty, 95 %% binary mask (%s)" % tag, lambda: sigma.resident(mm, reg, tshift))
        lines.append("#   masked / unmasked = %.3f" % (c / a))
        del mm
    lines.append("# LDS staging of the workgroup's patches: NOT BUILT, NOT MEASURED (the kernels read through the caches).")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
