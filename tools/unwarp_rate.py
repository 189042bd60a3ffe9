#!/usr/bin/env python3
"""what the unwarp kernel costs, alone and inside the step-scan pipeline.

    python tools/unwarp_rate.py [--out FILE] [--repeats N] [--n-proj P] [--skip-series]

1. The stand-alone kernel on device arrays, 2048^2 x 5 frames, for each raw dtype x interpolation kind, with dark and flat
   (the streaming case) and without: HIP events around windows of `--launch-reps` x 5 launches on one stream after a warm-up
   of each variant, `--repeats` windows per variant, the variants alternating.  ms per frame, and algorithmic GB/s
   (8 B map + raw sample + 0 / 16 B dark, flat + 8 B stored per pixel; tap re-reads are cache traffic and not counted)
   beside the 6.3 TB/s a streaming kernel achieves from HBM on this part.  The five frames and their maps (about 0.4 GB with
   float64 raw) exceed the 256 MiB Infinity Cache only in part: read the rates as "at most HBM-bound".
2. A C5-shaped series (bench_c5's parameters: 2048^2 x 5, Nw 5, max_shift 5, dark-field, uint16 counts, two references,
   flats and dark) through one StreamingMatcher per variant -- no map / a cubic radial map of up to 3 px -- in one process,
   alternating, `--repeats` series each after a warm-up series: ms per projection, median [min .. max]; and the upload
   stream alone (stage_sample + wait, nothing matched) both ways, which says whether that stream or the match bounds the
   series.
Needs a GPU; there is no fallback.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12          # bytes/s, streaming (float4 copy) rate of the part


def radial(h, w, amplitude=3.0):
    ii, jj = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ri, rj = (ii - 0.48 * h) / (h / 2.0), (jj - 0.53 * w) / (w / 2.0)
    r2 = ri * ri + rj * rj
    d0, d1 = r2 * ri + 0.137 * rj + 0.0113, r2 * rj - 0.211 * ri + 0.0271
    s = amplitude / max(np.abs(d0).max(), np.abs(d1).max())
    return (d0 * s).astype(np.float32), (d1 * s).astype(np.float32)


def med(v):
    return "%9.4f  [%9.4f .. %9.4f]" % (statistics.median(v), min(v), max(v))


def kernel_rates(repeats, launch_reps, n=2048, K=5):
    import torch
    from umpa_amd import UnwarpMap
    dev = torch.device("cuda", 0)
    d0, d1 = radial(n, n)
    maps = {it: UnwarpMap(d0, d1, interp=it) for it in ("linear", "cubic")}
    rng = np.random.default_rng(1)
    base = np.clip(20000.0 * (1.0 + 0.3 * rng.standard_normal((K, n, n))), 100.0, 60000.0)
    raws = {"uint16": list(torch.from_numpy(np.rint(base).astype(np.uint16)).to(dev)),
            "float32": list(torch.from_numpy(base.astype(np.float32)).to(dev)),
            "float64": list(torch.from_numpy(base).to(dev))}
    dark = list(torch.full((K, n, n), 100.0, dtype=torch.float64, device=dev))
    flat = list((0.9 + 0.2 * torch.rand((K, n, n), dtype=torch.float64, device=dev)))
    out = [torch.zeros((n, n), dtype=torch.float64, device=dev) for _ in range(K)]
    stream = torch.cuda.Stream(device=dev)
    variants = [(dt, it, corr) for dt in raws for it in maps for corr in (True, False)]

    def window(dt, it, corr, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            for _ in range(reps):
                maps[it].apply_device(raws[dt], out, dark=dark if corr else None, flat=flat if corr else None, stream=stream.cuda_stream)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / (reps * K)                       # ms per frame

    for v in variants:
        window(*v, 3)                                                 # warm-up: code objects, clocks
    t = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:                                            # alternating
            t[v].append(window(*v, launch_reps))
    lines = ["unwarp_kernel alone: %d^2 x %d frames on device arrays, radial map of up to 3 px; HIP events around %d x %d launches, "
             "%d windows per variant, alternating" % (n, K, launch_reps, K, repeats),
             "  %-8s %-7s %-10s  ms per frame, median [min .. max]        algorithmic B/px   GB/s (median)   of %.1f TB/s" % (
                 "raw", "interp", "dark+flat", HBM_ACHIEVABLE / 1e12)]
    esz = {"uint16": 2, "float32": 4, "float64": 8}
    for (dt, it, corr), v in t.items():
        bpp = 8 + esz[dt] + (16 if corr else 0) + 8
        rate = bpp * n * n / (statistics.median(v) * 1e-3)
        lines.append("  %-8s %-7s %-10s %s   %3d   %10.1f   %5.1f %%" % (dt, it, "yes" if corr else "no", med(v), bpp, rate / 1e9, 100.0 * rate / HBM_ACHIEVABLE))
    return lines


def c5_series(repeats, n_proj):
    from umpa_amd import UnwarpMap
    from umpa_amd.farm import StreamingMatcher, nearest_reference
    from umpa_amd.synth import CONFIGS, make_stack
    cfg = CONFIGS["C5"]
    H, W, K, Nw, ms = cfg["H"], cfg["W"], cfg["K"], cfg["Nw"], cfg["max_shift"]
    sam0, ref0, _ = make_stack(H, W, K, ms, df=True, seed=0, order=1)
    sam1, ref1, _ = make_stack(H, W, K, ms, df=True, seed=100, order=1)
    refs = np.stack([ref0, ref1])
    rng = np.random.default_rng(5)
    dark = 100.0 + rng.uniform(0, 2, size=(K, H, W))
    flats = 20000.0 * (1.0 + 0.05 * rng.standard_normal((2, K, H, W)))
    ref_nums = [0, n_proj - 1]
    d0, d1 = radial(H, W)
    sms = {"no map": StreamingMatcher(refs, Nw, ms, df=True, device=0, flats=flats, dark=dark, ref_nums=ref_nums),
           "cubic map": StreamingMatcher(refs, Nw, ms, df=True, device=0, flats=flats, dark=dark, ref_nums=ref_nums,
                                         unwarp=UnwarpMap(d0, d1, interp="cubic"))}
    bufs = []
    for p in range(n_proj):
        r = nearest_reference(p, ref_nums)
        b = sms["no map"].input_buffer(np.uint16)
        b[...] = np.rint((sam0 if r == 0 else sam1) * (1.0 - 0.004 * p) * flats[r] + dark).astype(np.uint16)
        bufs.append(b)

    def series(sm):
        t0 = time.perf_counter()
        n = sum(1 for _ in sm.run((p, bufs[p]) for p in range(n_proj)))
        assert n == n_proj
        return (time.perf_counter() - t0) * 1e3 / n_proj

    def upload_only(sm):
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in range(n_proj):
            sm._stage(p, bufs[p])
        torch.cuda.synchronize()
        sm.model._use_staged = False                                  # nothing adopts these uploads
        return (time.perf_counter() - t0) * 1e3 / n_proj

    for sm in sms.values():
        series(sm)                                                    # warm-up
    t = {k: [] for k in sms}
    u = {k: [] for k in sms}
    for _ in range(repeats):
        for k, sm in sms.items():                                     # alternating
            t[k].append(series(sm))
    for _ in range(repeats):
        for k, sm in sms.items():
            u[k].append(upload_only(sm))
    lines = ["C5-shaped series through StreamingMatcher: %d projections of %d x %d x %d uint16, Nw %d, max_shift %d, dark-field, two references; "
             "%d series per variant after a warm-up series, alternating; host clock around the whole series, transfers included" % (
                 n_proj, H, W, K, Nw, ms, repeats),
             "  %-10s ms per projection, median [min .. max]" % ""]
    for k in sms:
        lines.append("  %-10s %s" % (k, med(t[k])))
    a, b = statistics.median(t["no map"]), statistics.median(t["cubic map"])
    spread = max(max(v) - min(v) for v in t.values())
    lines.append("  with the map the series takes %+.2f %% (%.4f ms per projection); run-to-run spread of a variant here: %.4f ms" % (
        100.0 * (b - a) / a, b - a, spread))
    lines.append("  upload stream alone (stage_sample of every projection, then one synchronise; nothing matched)")
    for k in sms:
        lines.append("  %-10s %s" % (k, med(u[k])))
    lines.append("  the series is bound by %s" % (
        "the match (the upload stream, map included, needs less than a projection's match)" if statistics.median(u["cubic map"]) < a
        else "the upload stream once it unwarps"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launch-reps", type=int, default=100)
    ap.add_argument("--n-proj", type=int, default=32)
    ap.add_argument("--skip-series", action="store_true")
    a = ap.parse_args()
    from umpa_amd import _lib
    if _lib.hip().device_count() < 1:
        sys.exit("unwarp_rate needs a GPU (there is no fallback): NOT MEASURED")
    lines = kernel_rates(a.repeats, a.launch_reps)
    print("\n".join(lines), flush=True)
    if not a.skip_series:
        more = c5_series(a.repeats, a.n_proj)
        print("\n".join(more), flush=True)
        lines += more
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
