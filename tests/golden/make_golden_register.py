#!/usr/bin/env python3
"""
Golden fixtures for the registration utilities (umpa_amd/register.py): `UMPA.align.shift_dist`, `shift_best`,
`get_diff_pos`, `find_sam_shift`, `get_new_sam_pos` of the unmodified reference (UMPA/align.py:119-265, 468-543,
734-772, 936-1041).  Run in the BUILD container only; tests/golden/make_golden.py makes the scratch build of the
reference that `import UMPA` needs.

Only data is written (tests/golden/J_register.npz): the input arrays (built by the functions of tests/register_expect.py)
and the reference's output arrays.

The generator fails if a fixture does not meet the conditions the tests rely on: the reference's global minimum strictly
inside the +-8 box, and its unrounded positions at least 5e-4 px from a rounding tie of the 0.01 grid.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

S = 8


def box(full, S0=S, S1=S):
    """the entries of a whole-frame periodic array at the shifts of the box, [ri + S0, rj + S1]"""
    ii = np.arange(-S0, S0 + 1) % full.shape[0]
    jj = np.arange(-S1, S1 + 1) % full.shape[1]
    return np.ascontiguousarray(full[ii[:, None], jj[None, :]])


def tie_distance(v):
    """distance (px) of the values from the nearest rounding tie of the 0.01 grid"""
    f = np.abs(np.asarray(v)) * 100.0
    return np.abs((f - np.floor(f)) - 0.5).min() / 100.0


def main():
    import make_golden as MG
    MG.build_reference(False)
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, MG.SCRATCH)
    from UMPA import align as RA                                     # the unmodified reference
    import register_expect as RE

    out = {}
    for n, (shape, seed, d) in enumerate(RE.PAIRS):
        a, b = RE.make_pair(shape, seed, d)
        w = RE.weights(shape, seed)
        out["p%d_a" % n], out["p%d_b" % n] = a, b
        cc, coeff = RA.shift_dist(a, b)
        assert np.abs(cc.imag).max() == 0 or np.abs(cc.imag).max() < 1e-9 * np.abs(cc).max()
        i, j = np.unravel_index(np.argmin(cc.real), cc.shape)
        r = np.array([(i + shape[0] // 2) % shape[0] - shape[0] // 2, (j + shape[1] // 2) % shape[1] - shape[1] // 2])
        if np.abs(r).max() >= S:
            raise SystemExit("pair %d: the reference's global minimum %r is not strictly inside the +-%d box" % (n, r, S))
        out["p%d_cc" % n], out["p%d_coeff" % n] = box(cc.real), box(coeff.real)
        out["p%d_ccmax" % n] = np.abs(cc).max()
        ccw, coeffw = RA.shift_dist(a, b, w=w)
        iw, jw = np.unravel_index(np.argmin(ccw.real), ccw.shape)
        if (iw, jw) != (i, j):
            raise SystemExit("pair %d: the weighted minimum is elsewhere" % n)
        out["p%d_ccw" % n], out["p%d_coeffw" % n] = box(ccw.real), box(coeffw.real)
        out["p%d_ccwmax" % n] = np.abs(ccw).max()
        bb, r0, alpha = RA.shift_best(a, b)
        out["p%d_best_r" % n], out["p%d_best_alpha" % n] = r0, alpha
        if n == 0:
            out["p0_best_b"] = bb
        out["p%d_best_mindist" % n] = RA.shift_best.mindist
        td = tie_distance(r0)
        print("pair %d %r: minimum %r, -r* = %r, tie distance %.2e px" % (n, shape, r, r0, td))
        if td < 5e-4:
            raise SystemExit("pair %d: %.2e px from a rounding tie" % (n, td))

    refs = RE.make_diffuser_stack()
    out["dp_refs"] = refs
    unrounded = RE.wrap_centred([RA.shift_best(refs[0], r)[1] for r in refs], refs.shape[1:])
    if np.abs(unrounded).max() >= S - 1:
        raise SystemExit("diffuser stack: a position is not strictly inside the box")
    td = tie_distance(unrounded[1:])
    print("diffuser stack: unrounded positions\n%r\ntie distance %.2e px" % (unrounded, td))
    if td < 5e-4:
        raise SystemExit("diffuser stack: %.2e px from a rounding tie" % td)
    out["dp_unrounded"] = unrounded
    out["dp_pos"] = RA.get_diff_pos(refs)

    T, pos, err = RE.make_transmission_maps()
    out["T"], out["T_pos"], out["T_err"] = T, pos, err
    chain = np.array(RA.find_sam_shift(T=T, sample_pos=pos))
    out["T_chain"] = chain
    print("find_sam_shift chain\n%r\nexpected about\n%r" % (chain, np.vstack([[0, 0], np.diff(err, axis=0)])))
    if np.abs(chain).max() >= S - 1:
        raise SystemExit("transmission maps: a shift is not strictly inside the box")
    ov = RA.overlap(pos, T[-1].shape)[2]
    pairs = [(i, j) for i in range(len(T)) for j in range(i + 1, len(T)) if ov[i, j] > 0.5]
    out["T_pairs"] = np.array(pairs)
    out["T_found"] = np.array([RA.find_sam_shift(T=T[list(m)], sample_pos=pos[list(m)])[1] for m in pairs])
    out["T_newpos"] = RA.get_new_sam_pos(T=T, sample_pos=pos)
    print("pairs %r\nfound\n%r\nnew positions\n%r" % (pairs, out["T_found"], out["T_newpos"]))
    np.savez_compressed(os.path.join(HERE, "J_register.npz"), **out)
    print("wrote J_register.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
