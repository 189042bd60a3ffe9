#!/usr/bin/env python3
"""what the uncertainty maps of libumpa_sigma.so cost.

    python tools/sigma_rate.py [--out FILE] [--repeats N] [--kernel C2,C3] [--call C2]

Per config of --kernel (BASELINE C2: 2048^2 x 10 frames, Nw 5, max_shift 5; C3: 4096^2 x 20 frames, Nw 7, max_shift 8; both
kinds): umpa_sigma_region on random device-resident stacks and a random shift field within the guard (the kernel's work
does not depend on the values), whole extent: the call is the moments kernel, the upload of the window and a synchronise.
Beside it the fp64-FMA floor of the accumulations the kernel executes -- 16 per tap and pixel (plain) or 16 and 7 additions,
priced as 23 (dark-field), K (2 Nw + 1)^2 taps -- at the 78.6 TFLOP/s (39.3 T FMA/s) fp64 vector peak of an MI355X.
Per config of --call: the whole model.uncertainty(result) on a model of host frames (it uploads both stacks), beside one
model.match() of the same model.  Host clock around a device synchronise, median [min .. max] of N repeats after a warm-up.
Needs a GPU; there is no fallback.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C2": dict(n=2048, K=10, Nw=5, ms=5, seed=0), "C3": dict(n=4096, K=20, Nw=7, ms=8, seed=11)}
FMA_PER_S = 39.3e12


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def show(v):
    return "%10.2f  [%10.2f .. %10.2f]" % (statistics.median(v), min(v), max(v))


def window(Nw):
    import numpy as np
    w = np.multiply.outer(np.hamming(2 * Nw + 1), np.hamming(2 * Nw + 1))
    return w / w.sum()


def kernel(name, repeats, say):
    import torch
    from umpa_amd import sigma
    c = CONFIGS[name]
    n, K, Nw, ms = c["n"], c["K"], c["Nw"], c["ms"]
    N = n - 2 * (Nw + ms)
    sam = torch.rand((K, n, n), dtype=torch.float64, device="cuda") + 0.5
    ref = torch.rand((K, n, n), dtype=torch.float64, device="cuda") + 0.5
    shift = torch.randint(-(ms - 1), ms, (2, N, N), dtype=torch.int32, device="cuda")
    taps = K * (2 * Nw + 1) ** 2
    say("%s: %d^2 x %d frames, Nw %d, max_shift %d: %d x %d pixels, %d taps each; ms, median [min .. max] of %d" % (name, n, K, Nw, ms, N, N, taps, repeats))
    for kind, per_tap in ((0, 16), (1, 23)):
        t = timed(lambda: sigma.region(sam, ref, window(Nw), ms, kind, (0, 1, N, 0, 1, N), shift), repeats)
        floor = per_tap * taps * N * N / FMA_PER_S * 1e3
        say("  umpa_sigma_region, kind %d        %s   fp64-FMA floor of %d accumulations per tap: %.2f ms (%.1f %% of it reached)" % (
            kind, show(t), per_tap, floor, 100 * floor / statistics.median(t)))
    del sam, ref, shift
    torch.cuda.empty_cache()


def call(name, repeats, say):
    import torch
    from umpa_amd import model
    from umpa_amd.synth import make_stack
    c = CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    m.debug = False
    res = m.match(quiet=True)
    say("%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field model of host frames; host wall time of the call, ms, median [min .. max] of %d" % (
        name, c["n"], c["K"], c["Nw"], c["ms"], repeats))
    say("  model.match()                    %s" % show(timed(lambda: m.match(quiet=True), repeats)))
    say("  model.uncertainty(result)        %s" % show(timed(lambda: m.uncertainty(res), repeats)))
    u = m.uncertainty(res)
    say("  valid pixels: %.4f of %d; median sigma_dx %.4f, sigma_dy %.4f px (residual mode)" % (
        u.valid.mean(), u.valid.size, float(statistics.median(u.sigma_dx[u.valid].tolist())), float(statistics.median(u.sigma_dy[u.valid].tolist()))))
    del m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel", default="C2,C3")
    ap.add_argument("--call", default="C2")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sigma_rate.py needs a GPU: nothing is measured without one")

    def say(s):
        print(s, flush=True)
        if a.out:                                                     # as it goes: a time limit must not lose what is measured
            with open(a.out, "a") as f:
                f.write(s + "\n")

    for name in filter(None, a.kernel.split(",")):
        kernel(name, a.repeats, say)
    for name in filter(None, a.call.split(",")):
        call(name, a.repeats, say)


if __name__ == "__main__":
    main()
