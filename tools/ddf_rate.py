"""
Times of the directional dark-field search (libumpa_ddf.so, umpa_amd/ddf.py) at the flagship workload's parameters.

    python tools/ddf_rate.py [--out FILE] [--candidates 32] [--size 2048] [--skip-parent]
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR -- python tools/ddf_rate.py --blur-only   (a counter run of its own)

1. `ddf_blur_kernel` alone on a 2048 x 2048 x 10 device stack, an isotropic and an oblique kernel: milliseconds between two
   events on the stream (median and minimum of the repetitions) and the fraction of the 39 TFMA/s fp64 vector peak DESIGN.md
   uses, counting 289 FMAs per interior pixel and frame.
2. A search over --candidates kernels at BASELINE config C2's parameters (2048 x 2048, 10 frames, Nw = 5, max_shift = 5), whole
   image: total and per candidate, split into blur, plain match and fold (host clock; every phase ends synchronised; the match
   downloads its maps and the fold uploads them again).
3. Beside it the kernel model itself, `UMPAModelDFKernel.match` with the same (a, b, c) at every pixel, on the band of 32 rows
   that tools/dfkernel_rate.py c2 times, scaled to the rows of the whole image: the ratio of the two per-candidate times.

One JSON line per measurement.  No GPU: the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFMA = 39.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--blur-only", action="store_true", help="part 1 with three repetitions only (for a profiler run)")
    ap.add_argument("--skip-parent", action="store_true")
    args = ap.parse_args()
    import torch
    from umpa_amd import _lib, ddf, model
    from umpa_amd.synth import make_stack
    if _lib.hip().device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("ddf_rate: no HIP device (a rate is measured on the GPU or not at all)")
    n, K, Nw, ms = args.size, args.frames, 5, 5
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # 1. the blur alone
    rng = np.random.default_rng(1)
    stack = torch.from_numpy(1.0 + 0.3 * rng.standard_normal((K, n, n))).to("cuda:0")
    out = torch.empty_like(stack)
    fin, fout = [stack[k] for k in range(K)], [out[k] for k in range(K)]
    stream = torch.cuda.current_stream().cuda_stream
    fma = 289.0 * (n - 16) * (n - 16) * K
    for name, abc in (("isotropic", (0.1, 0.0, 0.1)), ("oblique", ddf.kernel_from_sigma(2.0, 0.6, np.pi / 4))):
        g = ddf.gaussian_kernel(*abc)
        ts = []
        for rep in range(3 if args.blur_only else 25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ddf._blur_device(fin, fout, g, 0, stream)
            e1.record()
            e1.synchronize()
            if rep >= 2:
                ts.append(e0.elapsed_time(e1))
        med, best = float(np.median(ts)), float(min(ts))
        emit(dict(what="ddf_blur_kernel", kernel=name, abc=list(abc), size=n, frames=K, gfma=fma / 1e9, ms_median=med, ms_min=best,
                  reps=len(ts), tfma_s=fma / (med * 1e-3) / 1e12, fraction_of_39_tfma_peak=fma / (med * 1e-3) / 1e12 / PEAK_TFMA))
    del stack, out, fin, fout
    if args.blur_only:
        return

    # 2. the search at C2's parameters
    sam, ref, _ = make_stack(n, n, K, ms, df=True, seed=40, amplitude=1.5, order=1)
    cand = ddf.candidate_grid([0.7, 1.2, 2.0], [1.0, 0.6, 0.3], 8)[:args.candidates]
    M = len(cand)
    s = ddf.KernelSearch(list(sam), list(ref), window_size=Nw, max_shift=ms)
    s.match(cand[:2])                                                 # warm-up
    t0 = time.perf_counter()
    res = s.match(cand)
    total = time.perf_counter() - t0
    tm = s.last_times
    N0, N1 = res["f"].shape
    per = total / M
    emit(dict(what="search", size=n, frames=K, Nw=Nw, max_shift=ms, candidates=M, output_px=N0 * N1, s_total=total, ms_per_candidate=1e3 * per,
              ms_blur_per_candidate=1e3 * tm["blur"] / M, ms_match_per_candidate=1e3 * tm["match"] / M,
              ms_fold_per_candidate=1e3 * tm["fold"] / M, err_ok=float(res["err"].mean()),
              winners=np.bincount(res["index"][res["index"] >= 0], minlength=M).tolist()))
    del s

    # 3. the kernel model itself on the band of tools/dfkernel_rate.py c2
    if not args.skip_parent:
        m = model.UMPAModelDFKernel(sam, ref, window_size=Nw, max_shift=ms)
        m.debug = "ncalls"
        E0, E1 = m.extent
        assert (E0, E1) == (N0, N1)
        rows = 32
        r0 = min(1000, E0 - rows)
        abc = np.zeros((rows, E1, 3))
        abc[...] = cand[0]
        roi = ((r0, r0 + rows, 1), (0, E1, 1))
        m.match(abc=abc, ROI=roi, quiet=True)
        t0 = time.perf_counter()
        m.match(abc=abc, ROI=roi, quiet=True)
        band = time.perf_counter() - t0
        scaled = band * E0 / rows
        emit(dict(what="UMPAModelDFKernel_uniform_abc", rows=rows, ms_band=1e3 * band, extent_rows=E0, ms_scaled_to_the_image=1e3 * scaled,
                  ratio_to_search_per_candidate=scaled / per))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
