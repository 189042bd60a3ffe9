#!/usr/bin/env python3
"""what the path aggregation of libumpa_smooth.so costs, and what bounds it.

    python tools/smooth_rate.py [--out FILE] [--repeats N] [--sizes 2028:9,4066:15] [--match C2,C3]

Per size N:U (a volume of U * U * N * N doubles, random, device-resident; the kernels' work does not depend on the values):
    the whole aggregation with 8 and with 4 paths;
    every pass by itself, as the difference between an aggregation over two directions and one over the first of them
    (the second pass reads C and reads and writes the accumulator: 3 volumes of compulsory traffic), and that traffic
    over the time, beside the 6.3 TB/s the HBM of an MI355X sustains;
    what remains of a single direction beside its pass: the selection (and, for directions 0 and 1, the two transposes).
Per config of --match (BASELINE C2: 2048^2 x 10 frames, Nw 5, max_shift 5; C3: 4096^2 x 20 frames, Nw 7, max_shift 8):
    match_smooth beside match(search='walk') and match(search='grid'), host wall time of the whole call.
Host clock around a device synchronise, median [min .. max] of N repeats after a warm-up.  Needs a GPU; there is no fallback.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C2": dict(n=2048, K=10, Nw=5, ms=5, seed=0), "C3": dict(n=4096, K=20, Nw=7, ms=8, seed=11)}
HBM_TBS = 6.3


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


def aggregation(N, U, repeats, say):
    import torch
    from umpa_amd import smooth
    cost = torch.rand((U, U, N, N), dtype=torch.float64, device="cuda")
    vol = cost.numel() * 8
    unit = 0.25
    # return_total: the sum is then a tensor of torch's caching allocator, and a call without a horizontal direction allocates
    # nothing (hipMalloc and hipFree of tens of GB cost more than the kernels)
    run = lambda dirs: (lambda: smooth.aggregate(cost, 0.25 * unit, 2.0 * unit, dirs=dirs, return_total=True))
    say("aggregation, %d x %d pixels, U = %d: a volume of %.2f GB; ms, median [min .. max] of %d" % (N, N, U, vol / 1e9, repeats))
    say("  8 paths                        %s" % show(timed(run(0xFF), repeats)))
    say("  4 paths                        %s" % show(timed(run(0x0F), repeats)))
    single = {d: timed(run(1 << d), repeats) for d in range(8)}
    for d in range(8):
        say("  direction %d alone              %s" % (d, show(single[d])))
        if d in (0, 2):                                               # its group's first direction is never a second pass
            continue
        base = 0 if d == 1 else 2                                     # accumulated first; direction d then reads and adds
        t = statistics.median(timed(run((1 << base) | (1 << d)), repeats)) - statistics.median(single[base])
        say("  direction %d as a second pass   %10.2f  -> %.2f TB/s of compulsory traffic (3 volumes; HBM sustains %.1f)" % (
            d, t, 3 * vol / (t * 1e-3) / 1e12 if t > 0 else float("nan"), HBM_TBS))
    del cost
    torch.cuda.empty_cache()


def matches(name, repeats, say):
    import torch
    from umpa_amd import model, smooth
    from umpa_amd.synth import make_stack
    c = CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    m.debug = False
    say("%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field; host wall time of the call, ms, median [min .. max] of %d" % (
        name, c["n"], c["K"], c["Nw"], c["ms"], repeats))
    say("  match(search='walk')           %s" % show(timed(lambda: m.match(quiet=True), repeats)))
    say("  match(search='grid')           %s" % show(timed(lambda: m.match(quiet=True, search="grid"), repeats)))
    say("  match_smooth, 8 paths          %s" % show(timed(lambda: smooth.match_smooth(m), repeats)))
    say("  match_smooth, 4 paths          %s" % show(timed(lambda: smooth.match_smooth(m, paths=4), repeats)))
    del m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="2028:9,4066:15")
    ap.add_argument("--match", default="C2,C3")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("smooth_rate.py needs a GPU: nothing is measured without one")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        if a.out:                                                     # as it goes: a time limit must not lose what is measured
            with open(a.out, "a") as f:
                f.write(s + "\n")

    for item in filter(None, a.sizes.split(",")):
        N, U = (int(v) for v in item.split(":"))
        aggregation(N, U, a.repeats, say)
    for name in filter(None, a.match.split(",")):
        matches(name, a.repeats, say)


if __name__ == "__main__":
    main()
