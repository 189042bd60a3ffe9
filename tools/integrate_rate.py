"""
Time of the phase integration (libumpa_integrate.so) on maps of the flagship workload's size.

    python tools/integrate_rate.py [--size 2028] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/integrate_rate.py --once

Device arrays, `w = 1` and the hole pattern of the tests (5 % random zeros, a zero block, a zero column, 10 % at 0.3,
NaN gradients at weight 0).  Per pattern: the solve at the default tolerance (time, iterations, residual), the V-cycle
alone, the V-cycle with UMPA_INTEGRATE_F_NO_TAIL (every level launched) and the solve with it, and the solve with
UMPA_INTEGRATE_F_JACOBI (the diagonal preconditioner, at most --jacobi-maxiter iterations).

Every time is the host clock around a call that allocates its workspace, builds the hierarchy, enqueues its kernels,
waits for them and frees the workspace: the time a caller sees, NOT a kernel time.  The V-cycle call therefore contains the
build of the levels; the difference between the two V-cycle calls is the saving of the tail kernel against launching the
levels it covers, reported also as a share of the call that launches them.  The tail kernel's own time needs a
profiler run (`--once`: one warm-up and one timed call per configuration).  A configuration is repeated until it has run
for 0.5 s and at least 5 times; median and minimum are reported.  No GPU: the tool fails.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, once, min_time=0.5, min_reps=5):
    import torch
    fn()
    if not once:
        fn()
    ts = []
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        if once or (len(ts) >= min_reps and sum(ts) >= min_time):
            return float(np.median(ts)), float(min(ts)), len(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2028)
    ap.add_argument("--out", default=None)
    ap.add_argument("--jacobi-maxiter", type=int, default=4000)
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed call per configuration (for a profiler run)")
    args = ap.parse_args()
    import torch
    import integrate_expect as E
    from umpa_amd import _lib
    I = importlib.import_module("umpa_amd.integrate")
    if _lib.hip().device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("integrate_rate: no HIP device (a rate is measured on the GPU or not at all)")
    n = args.size
    i, j = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    phi = 2.5 * np.sin(5.1 * i + 0.3) * np.cos(4.3 * j + 1.1)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for pattern in ("ones", "holes"):
        gx, gy = E.gradients(phi, 11, noise=1e-4)
        w = np.ones((n, n)) if pattern == "ones" else E.hole_weights((n, n), 11)
        gx[w == 0] = np.nan
        gy[w == 0] = np.nan
        tgx, tgy, tw = (torch.from_numpy(a).to("cuda:0") for a in (gx, gy, w))
        r = torch.from_numpy(np.random.default_rng(3).standard_normal((n, n))).to("cuda:0")
        base = dict(size=n, pattern=pattern)
        vc = {}
        for name, kw in (("vcycle", {}), ("vcycle_no_tail", dict(no_tail=True))):
            med, best, reps, _ = timed(lambda: I.vcycle(r, tw, **kw), args.once)
            vc[name] = med
            emit(dict(base, what=name, ms_median=1e3 * med, ms_min=1e3 * best, reps=reps))
        emit(dict(base, what="tail_saving", ms_per_vcycle=1e3 * (vc["vcycle_no_tail"] - vc["vcycle"]),
                  share_of_no_tail_vcycle_call=(vc["vcycle_no_tail"] - vc["vcycle"]) / vc["vcycle_no_tail"]))
        for name, kw in (("solve", {}), ("solve_no_tail", dict(no_tail=True)), ("solve_jacobi", dict(jacobi=True, maxiter=args.jacobi_maxiter))):
            med, best, reps, res = timed(lambda: I.integrate(tgx, tgy, tw, **kw), args.once, min_reps=3 if name == "solve_jacobi" else 5)
            emit(dict(base, what=name, ms_median=1e3 * med, ms_min=1e3 * best, reps=reps, iterations=res.iterations,
                      residual=res.residual, status=res.status, ms_per_iteration=1e3 * med / max(res.iterations, 1)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
