#!/usr/bin/env python3
"""
How the default penalties of umpa_amd.smooth (LAM_REL, TRUNC_REL, in units of cost_scale) were chosen.  Runs on the CPU:
the costs come from oracle/hp_cost.hp_volume (extended precision, rounded to fp64), the aggregation is the numpy
restatement tests/smooth_expect.py.  Stacks: umpa_amd/synth.py at 96 x 112, 4 frames, Nw = 3, max_shift = 5, displacement
amplitude 2.5, three noise levels.  The figure of merit is the RMS distance, in labels, of the regularised integer field
from the true displacement rounded to integers, over all pixels and both components; the pair with the lowest sum over the
noise levels is kept.  `--out FILE` also writes the table there (DESIGN.md section 4.10 holds a copy).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NOISES = (0.02, 0.05, 0.10)
LAMS = (0.1, 0.25, 0.5, 1.0, 2.0)
TRUNCS = (1.0, 2.0, 4.0, 8.0)
H, W, K, NW, MS = 96, 112, 4, 3, 5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import smooth_expect as SE
    from oracle import hp_cost
    from umpa_amd.smooth import cost_scale
    from umpa_amd.synth import make_stack

    win = np.multiply.outer(np.hamming(2 * NW + 1), np.hamming(2 * NW + 1))
    win = np.ascontiguousarray(win / win.sum())
    pad = MS + NW
    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))
    rms = np.zeros((len(NOISES), len(LAMS), len(TRUNCS)))
    plain = np.zeros(len(NOISES))
    for n, noise in enumerate(NOISES):
        sam, ref, (u_row, u_col) = make_stack(H, W, K, MS, df=True, seed=40 + n, noise=noise, amplitude=2.5)
        cost = hp_cost.hp_volume(hp_cost.KIND_DF, sam, ref, win, MS, pad).astype(np.float64)
        truth = np.stack([np.rint(u_row), np.rint(u_col)])[:, pad:H - pad, pad:W - pad]
        unit = cost_scale(cost)
        dist = lambda field: float(np.sqrt(np.mean((field - truth) ** 2)))
        plain[n] = dist(SE.argmin_field(cost))
        say("noise %.2f: cost_scale %.4g, per-pixel argmin RMS %.4f labels" % (noise, unit, plain[n]))
        for a, lam in enumerate(LAMS):
            for b, trunc in enumerate(TRUNCS):
                rms[n, a, b] = dist(SE.aggregate(cost, lam * unit, trunc * unit)["shift"])
    say("")
    say("RMS of the regularised start against the true integer field, labels; columns: noise " + ", ".join("%.2f" % v for v in NOISES) + ", sum")
    say("| lam_rel | trunc_rel | " + " | ".join("%.2f" % v for v in NOISES) + " | sum |")
    say("|---|---|" + "---|" * (len(NOISES) + 1))
    say("| per-pixel argmin | | " + " | ".join("%.4f" % v for v in plain) + " | %.4f |" % plain.sum())
    for a, lam in enumerate(LAMS):
        for b, trunc in enumerate(TRUNCS):
            say("| %g | %g | " % (lam, trunc) + " | ".join("%.4f" % v for v in rms[:, a, b]) + " | %.4f |" % rms[:, a, b].sum())
    a, b = np.unravel_index(np.argmin(rms.sum(axis=0)), rms.shape[1:])
    say("")
    say("lowest sum: lam_rel = %g, trunc_rel = %g" % (LAMS[a], TRUNCS[b]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
