"""
Time of the registration sums (libumpa_register.so) per pair of frames, and of the three-FFT formula on the host.

    python tools/register_rate.py [--size 2048] [--pairs 4] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/register_rate.py --once --no-fft

GPU: umpa_register_sums on device arrays (K pairs, one shared `a`), boxes +-4, +-8, +-16, unweighted and weighted,
float64 and uint16, both boundaries for +-8.  A call enqueues three kernels per pair (tiles, norms where unweighted and
periodic, reduction), waits for them and gives its scratch memory back, so the time per pair is the host clock around
the call over K: it contains the call's allocation and its synchronise.  That is the time a caller sees, NOT a kernel
time, and `tfma_per_s` derived from it is a rate of the call.  Kernel times come from a profiler run of its own: `--once`
makes one call per configuration (after one warm-up call), so that the kernel statistics of a `rocprofv3 --kernel-trace
--stats` run divide evenly: per configuration 2 K launches of register_tile_kernel.  Every shape is warmed up twice; a
configuration is repeated until it has run for 0.5 s and at least 5 times; median and minimum are reported, and the fused multiply-adds the definition needs (H W U0 U1 per plane summed) over the
median.  No GPU: the tool fails.

Host: D over ALL periodic shifts as the reference evaluates it, restated from the mathematics with scipy.fft --
cab = ifft2(fft2(a) conj(fft2(b))), D = |a|^2 - |cab|^2 / |b|^2 -- with one worker (the reference's call) and with 16.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fft_distance(a, b, workers):
    import scipy.fft as fft
    cab = fft.ifft2(fft.fft2(a, workers=workers) * np.conj(fft.fft2(b, workers=workers)), workers=workers)
    b2 = float(np.vdot(b, b).real)
    return float(np.vdot(a, a).real) - np.abs(cab) ** 2 / b2


def timed(fn, min_time=0.5, min_reps=5):
    fn(); fn()
    ts = []
    while len(ts) < min_reps or sum(ts) < min_time:
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-fft", action="store_true")
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed call per configuration (for a profiler run)")
    args = ap.parse_args()
    import torch
    from umpa_amd import _lib, register
    if _lib.hip().device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("register_rate: no HIP device (a rate is measured on the GPU or not at all)")
    n, K = args.size, args.pairs
    rng = np.random.default_rng(0)
    a64 = 1.0 + 0.3 * rng.standard_normal((n, n))
    b64 = np.stack([0.9 * np.roll(a64, (k + 1, -k), axis=(0, 1)) + 0.01 * rng.standard_normal((n, n)) for k in range(K)])
    w = torch.from_numpy(0.5 + rng.random((n, n))).to("cuda:0")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for dtype in ("float64", "uint16"):
        if dtype == "float64":
            a, b = torch.from_numpy(a64).to("cuda:0"), torch.from_numpy(b64).to("cuda:0")
        else:
            a = torch.from_numpy(np.rint(a64.clip(0, 3) * 20000).astype(np.uint16)).to("cuda:0")
            b = torch.from_numpy(np.rint(b64.clip(0, 3) * 20000).astype(np.uint16)).to("cuda:0")
        for S in (4, 8, 16):
            for weighted in (False, True):
                for boundary in (("wrap", "overlap") if S == 8 else ("wrap",)):
                    fn = lambda: register.shift_sums(a, b, w if weighted else None, max_shift=S, boundary=boundary)
                    if args.once:
                        fn()
                        t0 = time.perf_counter(); fn(); med = best = time.perf_counter() - t0; reps = 1
                    else:
                        med, best, reps = timed(fn)
                    planes = 3 if (weighted or boundary == "overlap") else 1
                    fma = float(n) * n * (2 * S + 1) ** 2 * planes
                    emit(dict(what="register_sums", size=n, pairs=K, dtype=dtype, max_shift=S, weighted=weighted, boundary=boundary,
                              ms_per_pair_median=1e3 * med / K, ms_per_pair_min=1e3 * best / K, reps=reps,
                              gfma_per_pair=fma / 1e9, tfma_per_s=fma * K / med / 1e12))
    if not args.no_fft:
        for workers in (1, 16):
            med, best, reps = timed(lambda: fft_distance(a64, b64[0], workers), min_time=2.0, min_reps=3)
            emit(dict(what="fft_distance_host", size=n, workers=workers, ms_per_pair_median=1e3 * med, ms_per_pair_min=1e3 * best, reps=reps))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
